"""The K nearest rows of a large L2 batch for 8 < K <= 256: the matrix-core form (fir_gemm_search_knn_keys_dev, reached through
fir_search_knn with fir_gallery_set_large_batch_mfma(g, 1)) against store + select (the only form before it; here behind a threshold
no call reaches -- threshold 0 is the same form but frees the fp16 copy, which the next matrix-core call would rebuild inside its
timed interval), same process, same gallery, whole host-pointer calls of fir_search_knn.

    gallery: --rows x --dim uniform [0, 1) rows, normalised (tests/synth.py's distribution), queries drawn the same way
    per (K, queries per call): one warm-up call of each form, then --reps timed calls of each, ALTERNATING, each timed on the host
    clock: the call is synchronous (upload, search on the handle's own stream, download, its own synchronisation), so this is the
    whole call as a caller sees it, not a sum of kernel times; the table gives the median queries/s of both forms and their ratio,
    and the queries the matrix-core form left to store + select in ALL the timed calls together (fir_gallery_mfma_stats_ex).
    idx and distance bits of the two forms are compared at every timed call.
    The "audit" line is one more call of fir_gemm_search_knn_keys_dev through the audit build with FIR_GEMM_DEBUG_COUNTS, which
    synchronises and reports the LAST super-batch of the call: appended rows per query (mean, max), lists that overflowed and the
    device time of that super-batch's three phases between events -- the sample bound (with the query preparation), the fp16 append
    pass, the re-rank. --sample-div: FIR_GEMM_KNN_SAMPLE_DIV (rows sampled = min(n, max(32768, n K / div))).

    python tools/knn_gemm_probe.py [--rows 1000000] [--dim 512] [--ks 9,16,32,64,128,256] [--batches 128,1024,8192] [--reps 3] [--sample-div 1024]
"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--ks", default="9,16,32,64,128,256")
ap.add_argument("--batches", default="128,1024,8192")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sample-div", type=int, default=0)
ap.add_argument("--no-audit", action="store_true", help="skip the audit-build call (appended rows, phases)")
args = ap.parse_args()
if args.sample_div:
    os.environ["FIR_GEMM_KNN_SAMPLE_DIV"] = str(args.sample_div)

fir = ge.load_package()
dev = torch.device("cuda", 0)
n, d = args.rows, args.dim
ks = [int(k) for k in args.ks.split(",")]
batches = [int(b) for b in args.batches.split(",")]


NEVER = 1 << 30        # a caller's threshold no call reaches: store + select


def unit_rows(count, gen):
    x = torch.rand((count, d), generator=gen, device=dev)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


gen = torch.Generator(device=dev).manual_seed(13)
h_rows = unit_rows(n, gen).cpu().numpy()
h_q = unit_rows(max(batches), gen).cpu().numpy()


def stderr_of(fn):
    """what fn() writes to file descriptor 2 (the library prints there)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def timed(fn):
    """(result, host ms around the whole synchronous call)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


print(f"# {n} x {d}, reps = {args.reps}, sample div = {args.sample_div or 1024}; device: {fir.device_info(0)}")
print(f"#   K   queries   store+select q/s   matrix q/s   ratio  uncertified in {args.reps} calls   # ms per call")
with fir.Gallery(h_rows, None, 0, 0) as g:
    for k in ks:
        for qb in batches:
            q = h_q[:qb]

            def call(threshold):
                g.set_large_batch_mfma(threshold)
                return g.search_knn(q, k)

            (si, sd), _ = timed(lambda: call(NEVER))                   # warm-up (scratch, the fp16 copy, kernel loading)
            (mi, md), _ = timed(lambda: call(1))
            assert g.last_dispatch()["path"] == "mfma", g.last_dispatch()
            assert np.array_equal(si, mi) and np.array_equal(sd.view(np.uint32), md.view(np.uint32)), (k, qb)
            ts, tg = [], []
            before = g.mfma_stats()["fallback_queries"]
            for _ in range(args.reps):
                ts.append(timed(lambda: call(NEVER))[1])
                (mi, md), t = timed(lambda: call(1))
                tg.append(t)
                assert np.array_equal(si, mi) and np.array_equal(sd.view(np.uint32), md.view(np.uint32)), (k, qb)
            unc = g.mfma_stats()["fallback_queries"] - before
            rs, rg = qb / np.median(ts) * 1e3, qb / np.median(tg) * 1e3
            print(f"{k:5d} {qb:9d} {rs:18.0f} {rg:12.0f} {rg / rs:7.2f} {unc:12d}   # store+select {min(ts):.2f}..{max(ts):.2f}, "
                  f"matrix cores {min(tg):.2f}..{max(tg):.2f}", flush=True)
if not args.no_audit:
    # the audit build's report: its own handles on the same data, the device-pointer call (its phases follow one another on the device)
    aud = ge.load_package(audit=True)
    os.environ["FIR_GEMM_DEBUG_COUNTS"] = "1"
    print("#   audit K queries | appended rows per query mean, max, lists overflowed | sample bound ms, append pass ms, re-rank ms (the call's last super-batch) | fir_gemm_stats_ex")
    tq = torch.from_numpy(h_q).to(dev)
    with aud.Gallery(h_rows, None, 0, 0) as g, aud.GemmSearch(g, 2) as m:
        for k in ks:
            for qb in batches:
                keys = torch.zeros(qb * k, dtype=torch.int64, device=dev)
                one = lambda: m.search_knn_keys_dev(tq.data_ptr(), qb, k, keys.data_ptr())
                one()
                text = stderr_of(one)
                r = re.search(r"last super-batch of (\d+)\): mean ([\d.]+), max (\d+);.*?(\d+) uncertified; (\d+) lists overflowed; preparation ([\d.]+) ms, "
                              r"full passes ([\d.]+) ms, re-rank ([\d.]+) ms", text)
                if r:
                    print(f"#   audit {k:5d} {qb:7d} | {float(r.group(2)):13.1f} {int(r.group(3)):6d} {int(r.group(5)):11d} | {float(r.group(6)):8.3f} "
                          f"{float(r.group(7)):8.3f} {float(r.group(8)):11.3f}  ({r.group(1)} queries, {r.group(4)} uncertified) | {m.stats()}", flush=True)
                else:
                    print(f"#   audit {k} {qb}: no report: {text!r}", flush=True)
    del os.environ["FIR_GEMM_DEBUG_COUNTS"]
