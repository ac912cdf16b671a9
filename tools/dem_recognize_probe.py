"""Time of fir_dem_recognize against the pieces path it replaces in DirectedEnumeration::recognize_batch: per 8 queries
fir_dem_likelihoods (n likelihoods per query to the host), a partial sort of the candidate positions on one CPU thread
(np.argpartition + a stable sort of the kept ones), and per query fir_rows_distances plus the walk. The pieces are composed
here in Python the way host/fir_classifiers.cpp composed them in C++; their entry points are unchanged, so both run from
one build. Threshold = getThreshold(min_other, 0.01), 40 pivots (32 kept).

    3 000 x 1536 with 1, 8 and 64 queries, 100 000 x 512 with 64 queries, each at M = 0.05 n and M = n
    one warm-up, then the median (min .. max) of --reps host-clock times of the synchronous host-pointer calls, alternating
    the two paths; the device time of fir_dem_recognize_dev between two events on its stream, and the device time of each of
    its stages (events between the stages: the library's measurement hook fir_dem_probe_, summed over the call's batches of 8)
    --sweep: 100 000 x 512, 64 queries, threshold 0: event times of the gather and the dense candidate-distance form
             (forced through fir_dem_probe_) over Mc / n, for the crossover constant kGatherDiv of csrc/fir_dem.hip

    python tools/dem_recognize_probe.py [--reps 20] [--sweep] [--small]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--small", action="store_true", help="only the 3 000-row shapes")
args = ap.parse_args()

fir = ge.load_package()
dev = torch.device("cuda", 0)
FLT_MAX = np.finfo(np.float32).max


def make(n, d, qb_max, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((n, d), generator=gen, device=dev)
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    cls = (torch.arange(n, device=dev, dtype=torch.int32) // 10).contiguous()
    pick = torch.randint(0, n, (qb_max,), generator=gen, device=dev)
    q = x[pick] + 0.02 * torch.rand((qb_max, d), generator=gen, device=dev) / d ** 0.5
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    return x, cls, q


def pieces(g, dem, piv, order, q, thr, M):
    """The parent commit's recognize_batch."""
    n, used = dem.n, dem.n_used
    out = []
    cand = order[used:]
    for i0 in range(0, len(q), 8):
        pd, lik = dem.likelihoods(q[i0:i0 + 8])
        for i in range(len(pd)):
            best, row, calc, found = FLT_MAX, -1, 0, 0
            for k in range(used):
                calc += 1
                if pd[i, k] < best:
                    best, row = pd[i, k], int(piv[k])
                    if best < thr:
                        found = 1
                        break
            if not found and M > used:
                mc = M - used
                cl = lik[i][cand]
                keep = np.argpartition(cl, mc - 1)[:mc] if mc < cand.size else np.arange(cand.size)
                keep = keep[np.argsort(cl[keep], kind="stable")]
                rows = cand[keep]
                dist = g.rows_distances(q[i0 + i], rows)[0]
                below = np.flatnonzero(dist < thr)
                stop = below[0] + 1 if below.size else mc
                j = int(np.argmin(dist[:stop]))
                calc += stop
                if dist[j] < best:
                    best, row = dist[j], int(rows[j])
                found = int(below.size > 0)
            out.append((row, best, found, calc))
    return out


STAGES = ("pivots", "likelihoods", "select", "mark", "cand. distances", "fold+finish+count")


def probe(dem, form=0, timing=0):
    fir.capi._check(fir.lib().fir_dem_probe_(dem._h, form, timing))


def stage_times(dem, g, dq, qb, thr, M, st, reps):
    """median over reps of the per-stage device times (ms) of one call"""
    outs = [torch.empty(qb, device=dev, dtype=torch.float32 if k == 1 else torch.int32) for k in range(5)]
    ms = np.zeros(len(STAGES), np.float32)
    rows = []
    for _ in range(reps):
        probe(dem, 0, 1)
        dem.recognize_dev(dq.data_ptr(), qb, thr, M, *(o.data_ptr() for o in outs), stream=st.cuda_stream)
        g.sync()
        fir.capi._check(fir.lib().fir_dem_probe_times_(dem._h, ms.ctypes.data_as(ctypes.c_void_p)))
        rows.append(ms.copy())
    probe(dem, 0, 0)
    return np.median(np.array(rows), axis=0)


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def host_times(fa, fb, reps):
    fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); t1 = time.perf_counter(); fb(); t2 = time.perf_counter()
        ta.append(t1 - t0); tb.append(t2 - t1)
    return stats(ta), stats(tb)


def event_time(dem, g, dq, qb, thr, M, st, reps):
    outs = [torch.empty(qb, device=dev, dtype=torch.float32 if k == 1 else torch.int32) for k in range(5)]
    f = lambda: dem.recognize_dev(dq.data_ptr(), qb, thr, M, *(o.data_ptr() for o in outs), stream=st.cuda_stream)
    f(); g.sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(st); f(); b.record(st)
    g.sync(); st.synchronize()
    return stats([a.elapsed_time(b) * 1e-3 for a, b in ev])


def shape(n, d, qbs, seed, sweep):
    x, cls, q_all = make(n, d, max(qbs), seed)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    g = fir.Gallery(dev_ptr=x.data_ptr(), n=n, d=d, metric=0, device=0, dev_class_ptr=cls.data_ptr())
    dem = fir.Dem(g, 17, 40)
    piv, mo, _, order = dem.get(want_table=False)
    thr = float(np.sort(mo[: dem.n_built])[int(dem.n_built * 0.01)])
    print(f"--- {n} x {d}, {dem.n_used} pivots kept, threshold {thr:.6g}", flush=True)
    if sweep:
        qb = max(qbs)
        for div in (128, 64, 32, 16, 8, 4, 2):
            M = dem.n_used + n // div
            t = {}
            for code, form in ((1, "gather"), (2, "dense")):
                probe(dem, code, 0)
                t[form] = event_time(dem, g, q_all[:qb], qb, 0.0, M, st, args.reps)
            probe(dem, 0, 0)
            print(f"qb={qb} Mc=n/{div:<3d}: gather {t['gather'][0]:8.3f} ms ({t['gather'][1]:.3f} .. {t['gather'][2]:.3f})   "
                  f"dense {t['dense'][0]:8.3f} ms ({t['dense'][1]:.3f} .. {t['dense'][2]:.3f})   gather/dense {t['gather'][0] / t['dense'][0]:5.2f}",
                  flush=True)
    else:
        for qb in qbs:
            q = q_all[:qb].cpu().numpy()
            for M in (int(0.05 * n), n):
                new = lambda: dem.recognize(q, thr, M)
                old = lambda: pieces(g, dem, piv, order, q, thr, M)
                r = new()
                ok = r[4] != 0
                for i, w in enumerate(old()):                      # same answers wherever no tie is flagged
                    assert ok[i] or (r[0][i], r[1][i], r[2][i], r[3][i]) == w, (i, w, [a[i] for a in r])
                tn, to = host_times(new, old, args.reps)
                te = event_time(dem, g, q_all[:qb], qb, thr, M, st, args.reps)
                print(f"qb={qb:3d} M={M:6d}: fir_dem_recognize {tn[0]:9.3f} ms ({tn[1]:.3f} .. {tn[2]:.3f})   pieces {to[0]:9.3f} ms "
                      f"({to[1]:.3f} .. {to[2]:.3f})   pieces/new {to[0] / tn[0]:7.2f}   device time of the call {te[0]:8.3f} ms "
                      f"({te[1]:.3f} .. {te[2]:.3f})   found {int(r[2].sum())}/{qb} ties {int(ok.sum())}", flush=True)
                sm = stage_times(dem, g, q_all[:qb], qb, thr, M, st, args.reps)
                print("        stages (ms): " + "  ".join(f"{name} {v:.3f}" for name, v in zip(STAGES, sm)), flush=True)
    dem.close()
    g.close()


if args.sweep:
    shape(100_000, 512, (64,), 2, True)
else:
    shape(3_000, 1536, (1, 8, 64), 1, False)
    if not args.small:
        shape(100_000, 512, (64,), 2, False)
