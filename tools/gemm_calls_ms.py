#!/usr/bin/env python3
"""ms per call of the GemmSearch calls in which host work is a visible share (a host-side change of fir_gemm.hip shows here first), one
JSON line. For A/B runs of two builds: tools/ab_libs.sh <rounds> <lib A> <lib B> -- tools/gemm_calls_ms.py
  100 000 x 512: top-1 with 128 queries (one super-batch, one stream), top-1 and top-5 with 4 096
  1M x 512:      top-1 with 32 768 queries, int8 nomination by the automatic rule and off; the 8-query few-keys call"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

fir = ge.load_package()
dev = torch.device("cuda", 0)
set_int8 = C.CDLL(fir.lib_path()).fir_gemm_set_int8_
set_int8.restype, set_int8.argtypes = None, [C.c_void_p, C.c_int32]


def ms_per_call(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = (time.perf_counter() - t0) / 2
    if best > 0.2:                                      # (queries that end in the exact device scan: seconds per call, nothing to learn from repeats)
        return round(best * 1e3, 4)
    for _ in range(5):                                  # the best of five timed groups: what the call costs, not what the box was doing
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps)
    return round(best * 1e3, 4)


def unit_rows(n, d, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.rand((n, d), generator=g, device=dev)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


out = {"lib": os.path.basename(os.path.dirname(fir.lib_path())) + "/" + os.path.basename(fir.lib_path())}
st = torch.cuda.Stream()
for n, cases in ((100_000, (("top1_128", 128, 1, 0, 200), ("top1_4096", 4096, 1, 0, 50), ("top5_4096", 4096, 5, 0, 30))),
                 (1_000_000, (("top1_32768_int8", 32768, 1, -1, 5), ("top1_32768_fp16", 32768, 1, 0, 5), ("few_8", 8, 0, 0, 50)))):
    x = unit_rows(n, 512, 5)
    torch.cuda.synchronize()                            # (the library's streams do not wait for torch's: the rows must be there before they are tiled)
    g = fir.Gallery(dev_ptr=x.data_ptr(), n=n, d=512, metric=0, device=0)
    m = fir.GemmSearch(g, fir.GemmSearch.F16)
    for name, qb, k, int8, reps in cases:
        # perturbed copies of gallery rows (bench.py's planted queries): every query has a near row, every list certifies
        g7 = torch.Generator(device=dev)
        g7.manual_seed(7)
        q = (x[(torch.arange(qb, device=dev) * 977 + 11) % n] + (torch.rand((qb, 512), generator=g7, device=dev) - 0.5) * 0.05 * x.mean()).clamp_min(0)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
        keys = torch.empty(qb * max(k, 1), device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        set_int8(m._h, int8)
        with torch.cuda.stream(st):
            if k == 0:
                call = lambda: m.search_few_keys_dev(q.data_ptr(), qb, keys.data_ptr(), stream=st.cuda_stream)        # noqa: E731
            elif k == 1:
                call = lambda: m.search_top1_keys_dev(q.data_ptr(), qb, keys.data_ptr(), stream=st.cuda_stream)       # noqa: E731
            else:
                call = lambda: m.search_topk_keys_dev(q.data_ptr(), qb, k, keys.data_ptr(), stream=st.cuda_stream)    # noqa: E731
            out[f"{n // 1000}k_{name}_ms"] = ms_per_call(call, reps)
    m.close()
    g.close()
    del x
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
