"""Times of the device-side PCA primitives (fir_gallery_feature_stats, fir_gallery_scatter, fir_gallery_create_projected) -- one
GPU, whole calls on the host clock, medians of three alternating rounds (every variant once per round, round after round), one
warm-up of every variant first.

  shapes      100 000 x 512 -> 64 and -> 256, 1M x 512 -> 256 (--big adds 1M x 1536 -> 256)
  stats       fir_gallery_feature_stats, NULL mask; GB/s against the tiled bytes read once
  scatter     fir_gallery_scatter, NULL mask and NULL centre (column sums included); TFLOP/s against 2 n d^2 / 2
  project     fir_gallery_create_projected (+ destroy); TFLOP/s against 2 n d p, to be read against the 59 TFLOP/s measured roof of
              v_mfma_f64_16x16x4_f64 (README), and a device-to-device hipMemcpyAsync of the output's bytes + a synchronisation
  host route  what a caller had before: fir_gallery_read_rows, numpy float64 on the CPUs (column statistics; x^T x about the mean;
              (x - mean) W^T rounded to float32), fir_gallery_create of the result -- timed once per shape, not per round

The device results are compared with the host route's before anything is timed (scatter to 1e-9 relative of its largest entry,
projection to 1e-5 of the largest output). Every shape runs in a child process of its own under its own time limit, one at a time;
the first one that fails or runs out of time ends the run. The lines go to stdout and to --out (default profiles/projection.txt).

    python tools/projection_probe.py [--rounds 3] [--limit 500] [--small] [--big] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "projection.txt")


def child(cfg):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    fir = ge.load_package()
    dev = torch.device("cuda", 0)
    n, d, p, rounds = cfg["n"], cfg["d"], cfg["p"], cfg["rounds"]
    gen = torch.Generator(device=dev).manual_seed(29 + n + d)
    x = torch.rand((n, d), generator=gen, device=dev)
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    torch.cuda.synchronize()
    tag = f"{n:>8d} x {d} -> {p}"
    lines = []

    def clock(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0) * 1e3, out

    def median_rounds(variants):
        for _, call in variants:
            call()
        ts = {name: [] for name, _ in variants}
        for _ in range(rounds):
            for name, call in variants:
                ts[name].append(clock(call)[0])
        return {name: float(np.median(v)) for name, v in ts.items()}

    with fir.Gallery(dev_ptr=x.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        del x
        # the host route, once: read back, float64 on the CPUs, upload again
        t_read, xh = clock(lambda: g.read_rows())
        t_hstats, hs = clock(lambda: (xh.min(axis=0), xh.max(axis=0), xh.mean(axis=0, dtype=np.float64), xh.std(axis=0, dtype=np.float64, ddof=1)))
        mean = hs[2]

        def host_scatter():
            z = xh.astype(np.float64) - mean
            return z.T @ z
        t_hscat, s_host = clock(host_scatter)
        s_dev, mean_dev, count = g.scatter()
        assert count == n and np.abs(mean_dev - mean).max() < 1e-12
        assert np.abs(s_dev - s_host).max() <= 1e-9 * np.abs(s_host).max(), float(np.abs(s_dev - s_host).max())
        t_eig, (vals, vecs) = clock(lambda: np.linalg.eigh(s_dev))
        basis = vecs[:, ::-1][:, :p].T.copy()

        def host_project():
            return ((xh.astype(np.float64) - mean) @ basis.T).astype(np.float32)
        t_hproj, y_host = clock(host_project)

        def host_create():
            fir.Gallery(y_host, None, 0, 0).close()
        t_hcreate, _ = clock(host_create)
        with fir.Projection(basis, mean) as proj:
            with g.projected(proj) as h:
                y_dev = h.read_rows()
            assert np.abs(y_dev - y_host).max() <= 1e-5 * np.abs(y_host).max(), float(np.abs(y_dev - y_host).max())
            out_bytes = n * ((p + 3) // 4) * 16
            a = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
            b = torch.empty(out_bytes, dtype=torch.uint8, device=dev)

            def d2d():
                b.copy_(a)
                torch.cuda.synchronize()
            ts = median_rounds([("stats", lambda: g.feature_stats()), ("scatter", lambda: g.scatter()),
                                ("project", lambda: g.projected(proj).close()), ("d2d", d2d)])
        tiled = ((n + 63) // 64) * 64 * ((d + 3) // 4) * 16
        lines.append(f"{tag}  feature_stats   {ts['stats']:9.2f} ms  {tiled / ts['stats'] / 1e6:8.1f} GB/s of the tiled rows | host route: "
                     f"read_rows {t_read:.0f} ms + numpy {t_hstats:.0f} ms")
        lines.append(f"{tag}  scatter         {ts['scatter']:9.2f} ms  {n * d * d / ts['scatter'] / 1e9:8.2f} TFLOP/s of n d^2 | host route: "
                     f"read_rows {t_read:.0f} ms + numpy {t_hscat:.0f} ms")
        lines.append(f"{tag}  create_projected{ts['project']:9.2f} ms  {2.0 * n * d * p / ts['project'] / 1e9:8.2f} TFLOP/s of 2 n d p (roof 59) | "
                     f"d2d copy of the output {ts['d2d']:.2f} ms | host route: read_rows {t_read:.0f} ms + numpy {t_hproj:.0f} ms + create {t_hcreate:.0f} ms")
        lines.append(f"{tag}  numpy.linalg.eigh of the {d} x {d} scatter matrix on the host: {t_eig:.0f} ms")
    print(json.dumps(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--small", action="store_true", help="100 000-row shapes only")
    ap.add_argument("--big", action="store_true", help="add 1M x 1536 -> 256")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(json.loads(args.child))
        return 0
    shapes = [(100_000, 512, 64), (100_000, 512, 256)]
    if not args.small:
        shapes.append((1_000_000, 512, 256))
    if args.big:
        shapes.append((1_000_000, 1536, 256))
    out = ["device-side PCA primitives: whole calls, host clock, medians of %d alternating rounds (tools/projection_probe.py)" % args.rounds]
    for n, d, p in shapes:
        cfg = json.dumps({"n": n, "d": d, "p": p, "rounds": args.rounds})
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg], capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out.append(f"{n} x {d} -> {p}: no result inside {args.limit} s; the run ends here")
            break
        if r.returncode != 0:
            out.append(f"{n} x {d} -> {p}: failed ({r.returncode}); the run ends here\n{r.stderr[-2000:]}")
            break
        out += json.loads(r.stdout.strip().split("\n")[-1])
        print("\n".join(out[-4:]), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
