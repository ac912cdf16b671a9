"""Times of fir_search_top1_other_class, its routed form and fir_gallery_far_threshold -- one GPU, L2, 512 features, 10 rows per
class (class-major runs, or the same labels permuted).

  (a) the scan form (fir_search_top1_other_class_keys_dev) against the exact top-1 scan on the same handle and batch
      (fir_search_top1_keys_dev with set_large_batch_mfma(0), set_tuning(8, 0)): device time through fir_profile_enable /
      fir_profile_read (the sum of the call's event pairs), median of --reps calls after 2 warm-up calls; 64 and 1 024 queries.
      At 100 000 rows also over features [1, 512): that range is no whole number of chunks, so the top-1 call runs the generic
      k_scan too, and the two kernels differ by the epilogue alone
  (b) the routed form against the scan form, whole host-pointer calls of fir_search_top1_other_class on the host clock
      (set_large_batch_mfma(1) against set_large_batch_mfma(0)), 128 / 1 024 / 8 192 queries, median of --reps after 1 warm-up; the
      two forms' answers are compared on the way
  (c) fir_gallery_far_threshold whole calls (host clock, one call after one warm-up at 100 000 rows): the scan form at 100 000
      rows only -- it is one exact scan per 8 rows of the gallery --, the routed form at both sizes

Every configuration runs in a child process of its own under its own time limit, one at a time; the first one that fails or runs
out of time ends the run. The lines go to stdout and to profiles/other_class.txt.

    python tools/other_class_probe.py [--reps 5] [--limit 240] [--small]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "other_class.txt")


def child(cfg):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    fir = ge.load_package()
    dev = torch.device("cuda", 0)
    n, d, layout, part, reps = cfg["n"], cfg["d"], cfg["layout"], cfg["part"], cfg["reps"]
    gen = torch.Generator(device=dev).manual_seed(7 + n)
    x = torch.rand((n, d), generator=gen, device=dev)
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    cls = torch.arange(n, device=dev, dtype=torch.int32) // 10
    if layout == "permuted":
        cls = cls[torch.randperm(n, generator=gen, device=dev)]
    cls = cls.contiguous()
    qmax = max(cfg["qbs"]) if cfg["qbs"] else 1
    pick = torch.randint(0, n, (qmax,), generator=gen, device=dev)
    q = x[pick] + 0.02 * torch.rand((qmax, d), generator=gen, device=dev) / d ** 0.5
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    ex = cls[pick].contiguous()                                    # each query passes over the class of the row it was made from
    torch.cuda.synchronize()
    tag = f"{n:>8d} x {d} {layout:<11s}"
    with fir.Gallery(dev_ptr=x.data_ptr(), n=n, d=d, metric=0, device=0, dev_class_ptr=cls.data_ptr()) as g:
        if part == "a":
            g.set_large_batch_mfma(0)
            g.set_tuning(8, 0)
            for qb in cfg["qbs"]:
                keys = torch.empty(qb, dtype=torch.int64, device=dev)

                def timed(call):
                    ts = []
                    for r in range(reps + 2):
                        g.profile_enable(True)
                        call()
                        g.sync()
                        ms, _ = g.profile_read()
                        g.profile_enable(False)
                        if r >= 2:
                            ts.append(float(ms.sum()))
                    return float(np.median(ts))

                for start in (0, 1) if n <= 100_000 else (0,):
                    t1 = timed(lambda: g.search_top1_keys_dev(q.data_ptr(), qb, keys.data_ptr(), start, d))
                    k1 = g.last_dispatch()["kernel"]
                    k1 = k1 if start else k1.split("<")[0]
                    t2 = timed(lambda: g.search_top1_other_class_keys_dev(q.data_ptr(), qb, ex.data_ptr(), keys.data_ptr(), start, d))
                    k2 = g.last_dispatch()["kernel"]
                    print(f"(a) {tag} qb={qb:5d} [{start},{d}): top-1 scan {t1:9.3f} ms ({qb / t1:6.1f} k queries/s, {k1})   other-class scan {t2:9.3f} ms "
                          f"({qb / t2:6.1f} k queries/s, {k2})   ratio {t2 / t1:5.2f}", flush=True)
        elif part == "b":
            qh, eh = q.cpu().numpy(), ex.cpu().numpy()

            def clocked(call, warm=1):
                ts = []
                for r in range(reps + warm):
                    t0 = time.perf_counter()
                    out = call()
                    if r >= warm:
                        ts.append((time.perf_counter() - t0) * 1e3)
                return float(np.median(ts)), out

            for qb in cfg["qbs"]:
                g.set_tuning(-1, 0)
                g.set_large_batch_mfma(0)
                ts, a = clocked(lambda: g.search_top1_other_class(qh[:qb], eh[:qb]))
                assert g.last_dispatch()["path"] == "scan"
                g.set_large_batch_mfma(1)                              # (a caller's threshold: routed whatever the library's default is)
                tr, b = clocked(lambda: g.search_top1_other_class(qh[:qb], eh[:qb]), warm=2)
                assert g.last_dispatch()["path"] == "mfma", g.last_dispatch()
                same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
                st = g.mfma_stats()
                print(f"(b) {tag} qb={qb:5d}: scan form {ts:10.3f} ms   routed form {tr:10.3f} ms   scan/routed {ts / tr:6.2f}   same answers {same}   "
                      f"exact-scan fallbacks so far {st['fallback_queries']}", flush=True)
                assert same
        else:
            for form in cfg["forms"]:
                g.set_large_batch_mfma(1 if form == "routed" else 0)
                if n <= 100_000:
                    g.far_threshold(0.01)
                t0 = time.perf_counter()
                thr, lo, hi, cnt = g.far_threshold(0.01)
                t = time.perf_counter() - t0
                print(f"(c) {tag} far_threshold(0.01), {form:>6s} form: {t:8.3f} s   ({n / t / 1e3:7.1f} k rows/s)   threshold {thr:.6g} min {lo:.6g} max {hi:.6g} "
                      f"counted {cnt}   last dispatch {g.last_dispatch()['path']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--small", action="store_true", help="100 000 rows only")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        child(json.loads(args.one))
        return 0
    sizes = (100_000,) if args.small else (100_000, 1_000_000)
    cfgs = []
    for n in sizes:
        for layout in ("class-major", "permuted"):
            cfgs.append(dict(part="a", n=n, d=512, layout=layout, qbs=[64, 1024], reps=args.reps))
    for n in sizes:
        for layout in ("class-major", "permuted"):
            cfgs.append(dict(part="b", n=n, d=512, layout=layout, qbs=[128, 1024, 8192], reps=max(3, args.reps // 2 + 1)))
    cfgs.append(dict(part="c", n=100_000, d=512, layout="class-major", qbs=[], forms=["scan", "routed"], reps=1))
    if not args.small:
        cfgs.append(dict(part="c", n=1_000_000, d=512, layout="class-major", qbs=[], forms=["routed"], reps=1))
    lines = ["fir_search_top1_other_class / fir_gallery_far_threshold -- tools/other_class_probe.py, one GPU, L2, 512 features, 10 rows per class",
             "(a) device time of the *_dev call (fir_profile_read, median) against the exact top-1 scan, set_tuning(8, 0), same handle and batch",
             "(b) whole host-pointer calls on the host clock (median): scan form against routed form (set_large_batch_mfma(1))",
             "(c) fir_gallery_far_threshold whole calls on the host clock; the scan form is one exact scan per 8 gallery rows and is not run at 1M rows"]
    rc = 0
    for cfg in cfgs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", json.dumps(cfg)], capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"STOPPED: {json.dumps(cfg)} did not finish within {args.limit} s")
            rc = 1
            break
        got = [ln for ln in p.stdout.split("\n") if ln.startswith("(")]
        lines += got
        print("\n".join(got), flush=True)
        if p.returncode != 0:
            lines.append(f"STOPPED: {json.dumps(cfg)} failed with status {p.returncode}: {p.stderr.strip().splitlines()[-1:] or ''}")
            rc = 1
            break
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1] if rc else f"wrote {OUT}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
