"""Times of the device-side gallery subsets (fir_gallery_create_subset_dev, a search on the new handle and
fir_keys_to_origin_dev) -- one GPU, L2, 512 features, whole calls on the host clock, medians of three alternating rounds (every
variant once per round, round after round), one warm-up of every variant first.

  galleries   100 000 x 512 and 1M x 512
  masks       random half, clustered 1/8 (runs of 16 whole tiles), scattered 1/64 (a seeded random row subset)
  (a) create  fir_gallery_create_subset_dev (device mask; the call synchronises) against
                - a device-to-device hipMemcpyAsync of the same number of row bytes + a synchronisation: the bandwidth yardstick
                - what a caller could do before: compact the caller's array on the host, then fir_gallery_create
  (b) split   one whole split: queries up, create_subset_dev, fir_search_top1_keys_dev on the new handle (default routing, as a caller
              gets it), fir_keys_to_origin_dev, keys back, destroy -- against fir_search_top1_masked of the same host batch on the
              full handle (the only form there was); 128 / 1 024 / 8 192 queries
  (c) reuse   the same without create and destroy: a second batch on a subset handle that exists

The mapped keys of (b) are compared with the masked call's answers before anything is timed. Every gallery size runs in a child
process of its own under its own time limit, one at a time; the first one that fails or runs out of time ends the run. The lines go
to stdout and to --out (default profiles/gallery_subset.txt).

    python tools/subset_probe.py [--rounds 3] [--limit 500] [--small] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "gallery_subset.txt")
RUN_TILES = 16


def make_mask(np, n, name, seed):
    if name == "clustered 1/8":
        return ((np.arange(n) // 64) // RUN_TILES) % 8 == 0
    rng = np.random.default_rng(seed)
    return rng.random(n) < (0.5 if name == "random 1/2" else 1.0 / 64)


def child(cfg):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    fir = ge.load_package()
    dev = torch.device("cuda", 0)
    n, d, rounds = cfg["n"], cfg["d"], cfg["rounds"]
    gen = torch.Generator(device=dev).manual_seed(11 + n)
    x = torch.rand((n, d), generator=gen, device=dev)
    x = (x / x.norm(dim=1, keepdim=True)).contiguous()
    qmax = max(cfg["qbs"])
    pick = torch.randint(0, n, (qmax,), generator=gen, device=dev)
    q = x[pick] + 0.02 * torch.rand((qmax, d), generator=gen, device=dev) / d ** 0.5
    qh = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    xh = x.cpu().numpy()
    torch.cuda.synchronize()
    tag = f"{n:>8d} x {d}"
    masks = [(name, make_mask(np, n, name, 17 + i)) for i, name in enumerate(("random 1/2", "clustered 1/8", "scattered 1/64"))]

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
        qd = torch.empty((qmax, d), dtype=torch.float32, device=dev)
        kd = torch.empty(qmax, dtype=torch.int64, device=dev)
        for name, take in masks:
            words = fir.pack_row_mask(take)
            wd = torch.from_numpy(words.view(np.int64)).to(dev)
            sel = np.flatnonzero(take)
            m = sel.shape[0]
            dst = torch.empty((m, d), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()

            def create():
                g.subset(mask_ptr=wd.data_ptr()).close()

            def memcpy():
                dst.copy_(x[:m])                                   # contiguous, same type, same device: one hipMemcpyAsync
                torch.cuda.synchronize()

            def host_way():
                fir.Gallery(np.ascontiguousarray(xh[sel]), None, 0, 0).close()

            med = median_rounds([("create", create), ("memcpy", memcpy), ("host", host_way)])
            sub = g.subset(mask_ptr=wd.data_ptr())
            t_close = clock(sub.close)[0]
            gbs = 2.0 * m * d * 4 / (med["create"] * 1e-3) / 1e9
            print(f"(a) {tag} mask {name:<14s} ({m:7d} rows): create_subset_dev {med['create']:9.3f} ms ({gbs:6.0f} GB/s read + written; destroy {t_close:6.3f} ms)   "
                  f"d2d memcpy of the row bytes {med['memcpy']:9.3f} ms ({med['create'] / med['memcpy']:5.2f} x)   host compaction + fir_gallery_create "
                  f"{med['host']:9.1f} ms ({med['host'] / med['create']:6.1f} x)", flush=True)

            for qb in cfg["qbs"]:
                qq = qh[:qb]

                def batch(sub_):
                    qd[:qb].copy_(torch.from_numpy(qq))
                    torch.cuda.synchronize()
                    sub_.search_top1_keys_dev(qd.data_ptr(), qb, kd.data_ptr())
                    sub_.keys_to_origin_dev(kd.data_ptr(), qb)
                    sub_.sync()
                    return kd[:qb].cpu().numpy().view(np.uint64)

                def split():
                    with g.subset(mask_ptr=wd.data_ptr()) as s:
                        return batch(s)

                def masked():
                    return g.search_top1_masked(qq, words)

                idx, dist = masked()
                got = split()
                want = np.where(idx < 0, np.uint64(fir.capi.KEY_NONE), np.array([fir.key_pack(a, b) for a, b in zip(dist, idx)], np.uint64))
                assert np.array_equal(got, want), "the mapped keys of the split are not the masked call's"
                with g.subset(mask_ptr=wd.data_ptr()) as s:
                    batch(s)
                    path = s.last_dispatch()["path"]
                    med = median_rounds([("split", split), ("masked", masked), ("reuse", lambda: batch(s))])
                print(f"(b) {tag} mask {name:<14s} qb={qb:5d}: whole split (create + top-1 [{path}] + map + destroy) {med['split']:9.3f} ms   fir_search_top1_masked "
                      f"{med['masked']:9.3f} ms   masked / split {med['masked'] / med['split']:6.2f}", flush=True)
                print(f"(c) {tag} mask {name:<14s} qb={qb:5d}: a second batch on the same subset handle {med['reuse']:9.3f} ms   masked / reuse "
                      f"{med['masked'] / med['reuse']:6.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=500, help="seconds per gallery size")
    ap.add_argument("--small", action="store_true", help="100 000 rows only")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        child(json.loads(args.one))
        return 0
    sizes = (100_000,) if args.small else (100_000, 1_000_000)
    cfgs = [dict(n=n, d=512, qbs=[128, 1024, 8192], rounds=args.rounds) for n in sizes]
    lines = ["fir_gallery_create_subset_dev / fir_keys_to_origin_dev -- tools/subset_probe.py, one GPU, L2, 512 features",
             "whole calls on the host clock, medians of the alternating rounds, one warm-up of every variant first",
             "(a) create_subset_dev against a d2d memcpy of the same row bytes and against host compaction + fir_gallery_create",
             "(b) one whole split (queries up, create, routed top-1, key map, keys back, destroy) against fir_search_top1_masked of the same batch",
             "(c) the same batch on a subset handle that already exists"]
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1] if rc else f"wrote {args.out}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
