"""fir_twd_conventional on large batches: type 0 (posteriors), threshold 0.24, reduced_features_count 64, host pointers, timed
around the call (it returns with the verdicts in host memory).

    galleries: (a) 230 400 x 256, 7 680 identities of 30 images -- the reference's 30-per-class shape at the largest class count the
                   classifier accepts; (b) 1 000 000 x 256, 7 680 identities (about 130 images each).
               An image is centre * (1 + 0.3 noise), normalised, as in tools/class_rank_gemm_bench.py, then multiplied by --scale
               (a power of two: with unit rows every posterior ratio sits near 0.2 and every query is unreliable).
               "class-major": the images of an identity are consecutive rows; "permuted": the same rows in random order.
    batches:   128, 1 024, 4 096 and 32 768 queries per call (images of random identities drawn the same way)
    forms:     "routed"  fir_gallery_set_large_batch_mfma(g, 64): the matrix-core batch form
               "staged"  fir_gallery_set_large_batch_mfma(g, 0): the launch-per-stage form
               "auto"    fir_gallery_set_large_batch_mfma(g, -1): whatever the library chooses by itself
    per case one warm-up call, then the median of --reps timed calls, and the six counters of fir_twd_last_mfma where the library
    has them. The library is loaded with ctypes alone, so --lib can name ANY build of libfir_amd.so -- the parent commit's, which
    has neither the form nor the counters, included: run once per library and compare the tables.

    python tools/twd_batch_probe.py [--lib path/to/libfir_amd.so] [--forms routed,staged,auto] [--shapes a,b] [--batches 128,1024,4096,32768]
                                    [--reps 3] [--scale 4] [--max-staged 32768]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "fast-image-recognition_amd", "libfir_amd.so"))
ap.add_argument("--forms", default="routed,staged")
ap.add_argument("--shapes", default="a,b")
ap.add_argument("--batches", default="128,1024,4096,32768")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--scale", type=float, default=4.0)
ap.add_argument("--max-staged", type=int, default=32768, help="largest batch the staged form is timed at (it takes seconds per thousand queries)")
args = ap.parse_args()

L = C.CDLL(args.lib)
L.fir_last_error.restype = C.c_char_p
vp = C.c_void_p
L.fir_gallery_create.argtypes = [vp, C.c_int64, C.c_int32, vp, C.c_int32, C.c_int32, C.POINTER(vp)]
L.fir_gallery_destroy.argtypes = [vp]
L.fir_gallery_set_large_batch_mfma.argtypes = [vp, C.c_int32]
L.fir_twd_conventional.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, vp, vp]
HAS_COUNTERS = hasattr(L, "fir_twd_last_mfma")
if HAS_COUNTERS:
    L.fir_twd_last_mfma.argtypes = [vp, vp]


def ok(rc):
    if rc != 0:
        raise RuntimeError(f"error {rc}: {L.fir_last_error().decode()}")


D, NC, TYPE, TH, RED = 256, 7680, 0, 0.24, 64
SHAPES = {"a": 230400, "b": 1000000}
batches = [int(b) for b in args.batches.split(",")]
rng = np.random.default_rng(5)
centres = rng.random((NC, D), dtype=np.float32)


def images(who):
    x = centres[who] * (1 + np.float32(0.3) * (rng.random((who.size, D), dtype=np.float32) - np.float32(0.5)))
    x /= np.sqrt((x * x).sum(axis=1, dtype=np.float32))[:, None]
    return np.ascontiguousarray(x * np.float32(args.scale), np.float32)


queries = images(rng.integers(0, NC, max(batches)))
print(f"# {os.path.relpath(args.lib, ROOT) if args.lib.startswith(ROOT) else args.lib}: type {TYPE}, threshold {TH}, reduced {RED}, {NC} classes, d = {D}, "
      f"scale {args.scale}, reps {args.reps}, counters {'yes' if HAS_COUNTERS else 'no (a library without the batch form)'}")
print("# shape labelling    form     queries   ms/call (median)   queries/s  reliable | took  reliable  stage2  band  uncertified  class-scan")
for sh in args.shapes.split(","):
    n = SHAPES[sh]
    labels_major = (np.arange(n, dtype=np.int64) * NC // n).astype(np.int32)
    rows_major = images(labels_major)
    perm = rng.permutation(n)
    for name in ("class-major", "permuted"):
        rows = rows_major if name == "class-major" else np.ascontiguousarray(rows_major[perm])
        labels = labels_major if name == "class-major" else np.ascontiguousarray(labels_major[perm])
        g = vp()
        ok(L.fir_gallery_create(rows.ctypes.data_as(vp), n, D, labels.ctypes.data_as(vp), 0, 0, C.byref(g)))
        verdicts = {}
        for form in args.forms.split(","):
            ok(L.fir_gallery_set_large_batch_mfma(g, {"routed": 64, "staged": 0, "auto": -1}[form]))
            for qb in batches:
                if form == "staged" and qb > args.max_staged:
                    continue
                q = queries[:qb]
                cls = np.empty(qb, np.int32)
                unrel = np.empty(qb, np.int32)
                call = lambda: ok(L.fir_twd_conventional(g, q.ctypes.data_as(vp), qb, NC, TYPE, TH, RED, cls.ctypes.data_as(vp), unrel.ctypes.data_as(vp)))
                call()                                                # warm-up: scratch, the fp16 copies, kernel loading
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    ts.append(time.perf_counter() - t0)
                cnt = (C.c_int64 * 6)()
                if HAS_COUNTERS:
                    ok(L.fir_twd_last_mfma(g, cnt))
                med = float(np.median(ts))
                print(f"  {sh}     {name:12s} {form:7s} {qb:8d} {med * 1e3:12.2f} ({min(ts) * 1e3:.2f}..{max(ts) * 1e3:.2f}) {qb / med:10.0f} {int((unrel == 0).sum()):9d} | "
                      + " ".join(f"{int(c):7d}" for c in cnt), flush=True)
                key = (qb,)
                if key in verdicts:                                   # the forms must agree
                    assert np.array_equal(verdicts[key][0], cls) and np.array_equal(verdicts[key][1], unrel), (sh, name, form, qb)
                verdicts[key] = (cls.copy(), unrel.copy())
        ok(L.fir_gallery_destroy(g))
sys.stdout.flush()
