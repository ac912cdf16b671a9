"""Times of the masked searches (fir_search_top1_masked, fir_search_knn_masked at k = 64) -- one GPU, L2, 512 features, whole
host-pointer calls on the host clock, medians of three alternating rounds (every variant once per round, round after round).

  galleries   100 000 x 512 and 1M x 512; 8 / 128 / 1 024 queries
  masks       densities 1, 1/2, 1/8, 1/64 in two layouts: clustered (runs of 16 whole tiles set, as a class filter on class-major labels
              produces: the scan skips every other tile) and scattered (a seeded random row subset: nearly every tile keeps a row)
  against     (1) the same calls unmasked in the forms the masked ones are built from: fir_search_top1_other_class with a class no row
                  carries (the generic exact top-1 scan with one more compare) and fir_search_knn (store + select), both with
                  set_large_batch_mfma(0) so that neither is routed to the matrix cores
              (2) what a caller without masks does today: fir_gallery_create over the compacted rows, then the unmasked call (the two
                  parts timed apart, one round: the upload dominates)

Two things the output states plainly: what the all-ones mask costs over the unmasked generic scan, and whether clustered 1/8 and 1/64
masks run well below the all-ones time (if they do not, the tile skip is not working).

Every gallery size runs in a child process of its own under its own time limit, one at a time; the first one that fails or runs out
of time ends the run. The lines go to stdout and to profiles/masked_search.txt.

    python tools/masked_search_probe.py [--rounds 3] [--limit 500] [--small]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "masked_search.txt")
K = 64
RUN_TILES = 16


def make_mask(np, n, density, layout, seed):
    if density == 1:
        return np.ones(n, bool)
    if layout == "clustered":
        tile = np.arange(n) // 64
        return (tile // RUN_TILES) % density == 0            # one run of RUN_TILES tiles in every `density` runs
    rng = np.random.default_rng(seed)
    return rng.random(n) < 1.0 / density


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
    cls = (torch.arange(n, device=dev, dtype=torch.int32) // 10).contiguous()
    qmax = max(cfg["qbs"])
    pick = torch.randint(0, n, (qmax,), generator=gen, device=dev)
    q = x[pick] + 0.02 * torch.rand((qmax, d), generator=gen, device=dev) / d ** 0.5
    qh = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    xh = x.cpu().numpy()
    torch.cuda.synchronize()
    tag = f"{n:>8d} x {d}"
    masks = [("1", "-", make_mask(np, n, 1, "-", 0))]
    for density in (2, 8, 64):
        for layout in ("clustered", "scattered"):
            masks.append((f"1/{density}", layout, make_mask(np, n, density, layout, 13 + density)))

    def clock(call):
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0) * 1e3, out

    with fir.Gallery(dev_ptr=x.data_ptr(), n=n, d=d, metric=0, device=0, dev_class_ptr=cls.data_ptr()) as g:
        g.set_large_batch_mfma(0)
        packed = [fir.pack_row_mask(m) for _, _, m in masks]
        for qb in cfg["qbs"]:
            qq = qh[:qb]
            variants = [("top1 unmasked generic scan", lambda: g.search_top1_other_class(qq, 1 << 30)), ("knn unmasked store+select", lambda: g.search_knn(qq, K))]
            for (dens, layout, _), words in zip(masks, packed):
                variants.append((f"top1 masked {dens} {layout}", lambda w=words: g.search_top1_masked(qq, w)))
                variants.append((f"knn masked {dens} {layout}", lambda w=words: g.search_knn_masked(qq, w, K)))
            for _, call in variants:                          # one warm-up each: scratch grows here, not in a timed call
                call()
            ts = {name: [] for name, _ in variants}
            for _ in range(rounds):
                for name, call in variants:
                    ts[name].append(clock(call)[0])
            med = {name: float(np.median(v)) for name, v in ts.items()}
            kern = {}
            g.search_top1_masked(qq, packed[0])
            kern["masked"] = g.last_dispatch()["kernel"]
            g.search_top1_other_class(qq, 1 << 30)
            kern["unmasked"] = g.last_dispatch()["kernel"]
            for kind, base in (("top1", "top1 unmasked generic scan"), ("knn", "knn unmasked store+select")):
                ones = med[f"{kind} masked 1 -"]
                print(f"(1) {tag} qb={qb:5d} {kind:4s}: unmasked {med[base]:9.3f} ms   all-ones mask {ones:9.3f} ms   all-ones / unmasked {ones / med[base]:5.2f}"
                      + (f"   ({kern['unmasked']} | {kern['masked']})" if kind == "top1" else ""), flush=True)
                for dens, layout, _ in masks[1:]:
                    t = med[f"{kind} masked {dens} {layout}"]
                    print(f"(1) {tag} qb={qb:5d} {kind:4s}: mask {dens:>4s} {layout:<9s} {t:9.3f} ms   / all-ones {t / ones:5.2f}   / unmasked {t / med[base]:5.2f}", flush=True)
        # (2) the alternative today: a second handle over the compacted rows, then the unmasked call (default routing, as a caller gets it)
        qb = cfg["qbs"][-1]
        qq = qh[:qb]
        for (dens, layout, m), words in zip(masks[1:], packed[1:]):
            sel = np.flatnonzero(m)
            t_pack, sub = clock(lambda: np.ascontiguousarray(xh[sel]))
            t_up, h = clock(lambda: fir.Gallery(sub, None, 0, 0))
            with h:
                h.search_top1(qq)
                t_c1 = clock(lambda: h.search_top1(qq))[0]
                t_ck = clock(lambda: h.search_knn(qq, K))[0]
            t_m1 = clock(lambda: g.search_top1_masked(qq, words))[0]
            t_mk = clock(lambda: g.search_knn_masked(qq, words, K))[0]
            print(f"(2) {tag} qb={qb:5d} mask {dens:>4s} {layout:<9s} ({sel.shape[0]:7d} rows): compact on the host {t_pack:8.1f} ms + create {t_up:8.1f} ms, then top1 "
                  f"{t_c1:8.3f} ms / knn {t_ck:8.3f} ms   masked on the full handle: top1 {t_m1:8.3f} ms / knn {t_mk:8.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=500, help="seconds per gallery size")
    ap.add_argument("--small", action="store_true", help="100 000 rows only")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        child(json.loads(args.one))
        return 0
    sizes = (100_000,) if args.small else (100_000, 1_000_000)
    cfgs = [dict(n=n, d=512, qbs=[8, 128, 1024], rounds=args.rounds) for n in sizes]
    lines = ["fir_search_top1_masked / fir_search_knn_masked (k = 64) -- tools/masked_search_probe.py, one GPU, L2, 512 features",
             "whole host-pointer calls on the host clock, medians of the alternating rounds; set_large_batch_mfma(0) on the full handle",
             "(1) masked calls against the unmasked generic top-1 scan (fir_search_top1_other_class, absent class) and store + select (fir_search_knn)",
             "(2) the alternative today: compact the rows on the host + fir_gallery_create + the unmasked call (one round), next to the masked call"]
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
