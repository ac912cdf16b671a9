"""Where the int8 nomination pass (fir_gallery_set_int8_nomination) pays: the two constants of the automatic rule.

  call size   queries per call against n x d, int8 pass on (mode 1) and off (mode 0), the matrix cores chosen by the library
  R / G       the same at one call size on galleries where one row in a thousand carries one outlier coordinate of growing
              size: it inflates max|c_g|, hence the grid step and R, the largest quantisation residual of a row (G: the largest
              centred norm); R and G are recomputed here as fir_gemm_i8.h defines them

Prints one line per case: q/s with and without the pass, their ratio, second-pass and exact-scan queries of the int8 calls.
Identical keys are asserted. Usage: python tools/int8_nomination_sweep.py [--rows 1000000] [--dim 512] [--reps 3] [--outliers 0.05,0.1,...] [--no-call-sizes]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def r_over_g(rows):
    mu = rows.mean(dim=0, dtype=torch.float64).float()
    g2, r2, mx = 0.0, 0.0, 0.0
    for i in range(0, rows.shape[0], 131072):
        c = rows[i:i + 131072] - mu
        mx = max(mx, float(c.abs().max()))
    s = 127.0 / mx
    for i in range(0, rows.shape[0], 131072):
        c = rows[i:i + 131072] - mu
        res = (torch.round(c * s).clamp(-127, 127).double() / s - c.double())
        r2 = max(r2, float((res * res).sum(dim=1).max()))
        g2 = max(g2, float((c.double() * c.double()).sum(dim=1).max()))
    return r2 ** 0.5, g2 ** 0.5


def rate(fir, g, q, qb, keys, mode, reps):
    g.set_int8_nomination(mode)
    g.search_top1_keys_dev(q.data_ptr(), qb, keys.data_ptr())
    torch.cuda.synchronize()
    st0 = g.mfma_stats()
    t0 = time.perf_counter()
    for _ in range(reps):
        g.search_top1_keys_dev(q.data_ptr(), qb, keys.data_ptr())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st1 = g.mfma_stats()
    return qb * reps / dt, st1["second_pass_queries"] - st0["second_pass_queries"], st1["fallback_queries"] - st0["fallback_queries"], g.last_dispatch()["kernel"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--outlier-batch", type=int, default=32768)
    ap.add_argument("--outliers", default="0.05,0.1,0.15,0.25,0.5,1.0", help="sizes of the outlier coordinate, ascending")
    ap.add_argument("--no-call-sizes", action="store_true")
    args = ap.parse_args()
    fir = ge.load_package()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d = args.rows, args.dim
    rows = torch.rand((n, d), generator=gen, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    qmax = 131072
    q = torch.rand((qmax, d), generator=gen, device=dev)
    q[1::2] = (rows[(torch.arange(qmax // 2, device=dev) * 977 + 11) % n] + 0.0025 * (torch.rand((qmax // 2, d), generator=gen, device=dev) - 0.5)).clamp_min(0)
    q /= q.norm(dim=1, keepdim=True)
    q = q.contiguous()
    keys = torch.empty(qmax, dtype=torch.int64, device=dev)
    keys0 = torch.empty(qmax, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def case(tag, qb):
        with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g:
            r0, _, _, k0 = rate(fir, g, q, qb, keys0, 0, args.reps)
            r1, sp, fb, k1 = rate(fir, g, q, qb, keys, 1, args.reps)
            assert torch.equal(keys[:qb], keys0[:qb])
            print(f"{tag}: {qb} queries/call  fp16 {r0 / 1e6:.3f} M q/s  int8 {r1 / 1e6:.3f} M q/s  x{r1 / r0:.3f}  second pass {sp}  exact scan {fb}  [{k1}]", flush=True)

    R, G = r_over_g(rows)
    print(f"gallery {n} x {d}: R = {R:.5f}, G = {G:.4f}, R / G = {R / G:.5f}", flush=True)
    for qb in (() if args.no_call_sizes else (512, 2048, 8192, 32768, 131072)):
        case("call size", qb)
    for a in [float(x) for x in args.outliers.split(",") if x]:
        rows[::1000, 7] = a
        torch.cuda.synchronize()
        R, G = r_over_g(rows)
        case(f"outlier {a} (R = {R:.5f}, G = {G:.4f}, R / G = {R / G:.5f})", args.outlier_batch)


if __name__ == "__main__":
    main()
