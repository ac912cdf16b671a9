"""Time of fir_search_top_classes_keys_dev against the exact 8-queries-per-read top-1 scan on the same gallery and batch.

1M x 512 f32, L2; 64 and 512 queries per call; k = 5 and 20; labels class-major with 10 rows per class, then the same labels
permuted. HIP events around every call. The class scan reads the gallery bytes of the top-1 scan plus 4 bytes of label per row and
pass, so the ratio of the two times is what the epilogue, the select kernels and the row sample cost.

    python tools/class_rank_probe.py [--rows N] [--one QB K ORDER]     (--one: a single warmed call, for a kernel trace)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--one", nargs=3, metavar=("QB", "K", "ORDER"))
args = ap.parse_args()

fir = ge.load_package()
dev = torch.device("cuda", 0)
n, d, per_class = args.rows, 512, 10
nc = (n + per_class - 1) // per_class
gen = torch.Generator(device=dev).manual_seed(1)
x = torch.rand((n, d), generator=gen, device=dev)
x = x / x.norm(dim=1, keepdim=True)
major = torch.arange(n, device=dev, dtype=torch.int32) // per_class
labels = {"class-major": major, "permuted": major[torch.randperm(n, generator=gen, device=dev)].contiguous()}
st = torch.cuda.Stream(dev)


def timed(fn, reps=5):
    fn(); fn()
    st.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(st); fn(); b.record(st)
    st.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


for order, lab in labels.items():
    if args.one and args.one[2] != order:
        continue
    g = fir.Gallery(dev_ptr=x.data_ptr(), n=n, d=d, metric=0, device=0, dev_class_ptr=lab.data_ptr())
    g.set_large_batch_mfma(0)          # the yardstick: the exact scan, 8 queries per gallery read
    g.set_tuning(8, 0)
    for qb in (64, 512):
        q = torch.rand((qb, d), generator=gen, device=dev)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
        k1 = torch.empty(qb, device=dev, dtype=torch.int64)
        t1 = None
        for k in (5, 20):
            if args.one and (int(args.one[0]), int(args.one[1])) != (qb, k):
                continue
            keys = torch.empty(qb * k, device=dev, dtype=torch.int64)
            cls = torch.empty(qb * k, device=dev, dtype=torch.int32)
            f = lambda: g.search_top_classes_keys_dev(q.data_ptr(), qb, nc, k, keys.data_ptr(), cls.data_ptr(), stream=st.cuda_stream)
            if args.one:
                f(); f(); st.synchronize()
                print("one call:", g.last_dispatch()["kernel"])
                continue
            if t1 is None:
                t1 = timed(lambda: g.search_top1_keys_dev(q.data_ptr(), qb, k1.data_ptr(), stream=st.cuda_stream))
                top1_kernel = g.last_dispatch()["kernel"]
            tc = timed(f)
            assert torch.equal(keys.view(qb, k)[:, 0], k1)        # the nearest class's row is the nearest row
            print(f"{order:12s} qb={qb:4d} k={k:2d}: top-1 scan {t1:8.3f} ms ({qb / t1:6.1f} k queries/s, {top1_kernel.split('<')[0]})   "
                  f"class scan {tc:8.3f} ms ({qb / tc:6.1f} k queries/s)   ratio {tc / t1:5.2f}", flush=True)
    g.close()
