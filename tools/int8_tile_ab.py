"""The int8 pass's 256-query tile against its 128-query tile, on ONE matrix-core state: fir_gemm_set_int8_tile_ (fir_internal.h)
switches between calls, so both forms see the same gallery copy, the same queries and the same box. Data as
tools/int8_nomination_sweep.py's (uniform unit rows, half fresh and half planted queries). Per call size: M q/s of each form
(alternating, `--reps` calls timed after a warm-up, `--rounds` times), identical keys asserted, the counters of the timed calls.
With FIR_AMD_LIB pointing at the audit build and FIR_GEMM_DEBUG_COUNTS=1 the library prints the appended rows per query of each
call's last super-batch as well.
Usage: python tools/int8_tile_ab.py [--rows 1000000] [--dim 512] [--sizes 512,2048,8192,32768,131072] [--reps 3] [--rounds 2]"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--sizes", default="512,2048,8192,32768,131072")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    fir = ge.load_package()
    lib = C.CDLL(fir.lib_path())
    for name in ("fir_gemm_set_int8_", "fir_gemm_set_int8_tile_"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int32]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d = args.rows, args.dim
    sizes = [int(x) for x in args.sizes.split(",") if x]
    modes = [0, 1]                                   # fir_gemm_set_int8_tile_: never / whenever the shape allows
    qmax = max(sizes)
    rows = torch.rand((n, d), generator=gen, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    q = torch.rand((qmax, d), generator=gen, device=dev)
    q[1::2] = (rows[(torch.arange(qmax // 2, device=dev) * 977 + 11) % n] + 0.0025 * (torch.rand((qmax // 2, d), generator=gen, device=dev) - 0.5)).clamp_min(0)
    q /= q.norm(dim=1, keepdim=True)
    q = q.contiguous()
    keys = [torch.empty(qmax, dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            lib.fir_gemm_set_int8_(m._h, 1)
            for qb in sizes:
                best, names = [0.0, 0.0], ["", ""]
                st0 = m.stats()
                for _ in range(args.rounds):
                    for tile in (0, 1):
                        lib.fir_gemm_set_int8_tile_(m._h, modes[tile])
                        m.search_top1_keys_dev(q.data_ptr(), qb, keys[tile].data_ptr())
                        torch.cuda.synchronize()
                        names[tile] = g.last_dispatch()["kernel"]
                        t0 = time.perf_counter()
                        for _ in range(args.reps):
                            m.search_top1_keys_dev(q.data_ptr(), qb, keys[tile].data_ptr())
                        torch.cuda.synchronize()
                        best[tile] = max(best[tile], qb * args.reps / (time.perf_counter() - t0))
                st1 = m.stats()
                assert torch.equal(keys[0][:qb], keys[1][:qb])
                print(f"{n} x {d}, {qb} queries/call: 128-query tile {best[0] / 1e6:.3f} M q/s  256-query tile {best[1] / 1e6:.3f} M q/s  x{best[1] / best[0]:.3f}  "
                      f"second pass {st1['second_pass_queries'] - st0['second_pass_queries']}  exact scan {st1['fallback_queries'] - st0['fallback_queries']}  "
                      f"[{names[0]} | {names[1]}]", flush=True)


if __name__ == "__main__":
    main()
