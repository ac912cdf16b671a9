"""fir_search_radius, both forms, against the calls that answered the same question before it: whole host-pointer calls on one
gallery in one process, each timed on the host clock around the (synchronous) call.

    gallery: --rows x --dim uniform [0, 1) rows, normalised (tests/synth.py's distribution), queries drawn the same way
    forms:   radius/1  fir_search_radius, store + count + select (behind a threshold no call reaches)
             radius/2  fir_search_radius through the matrix cores (fir_gallery_set_large_batch_mfma(g, 1))
             knn/1     fir_search_knn(k = max_results), store + select: the reference point of radius/1
             knn/2     fir_search_knn(k = max_results) through the matrix cores: the reference point of radius/2
    radii:   nextafter of the K-th distance fir_search_knn reports, at max_results = K; "K = 1000 / 256": the radius of K = 1000 with
             max_results = 256 (the count exceeds max_results); "overflow": radius = +inf with max_results = 16 -- every list
             overflows and every query of radius/2 falls back to radius/1: what a useless pass costs
    per line: one warm-up call of each form, then --reps timed calls of each, ALTERNATING; ms per call as min..median..max, the ratios
             of the medians, and the queries radius/2 left to radius/1 in all its timed calls (fir_gallery_mfma_stats_ex). Counts,
             idx and distance bits of the two radius forms are compared at every timed call.
    shares:  radius/1 with fir_profile_enable: the library's two event pairs per tile of 8 queries -- the store pass, then count +
             select + sort -- summed over the call, for the radius of K = 16 at max_results 0, 16 and 1024.

    python tools/radius_search_probe.py [--rows 1000000] [--dim 512] [--ks 1,9,64,256] [--batches 128,1024,8192] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--ks", default="1,9,64,256")
ap.add_argument("--batches", default="128,1024,8192")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

fir = ge.load_package()
dev = torch.device("cuda", 0)
n, d = args.rows, args.dim
ks = [int(k) for k in args.ks.split(",")]
batches = [int(b) for b in args.batches.split(",")]
NEVER = 1 << 30        # a caller's threshold no call reaches (threshold 0 is the same form but frees the fp16 copy)
INF = np.float32(np.inf)


def unit_rows(count, gen):
    x = torch.rand((count, d), generator=gen, device=dev)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


gen = torch.Generator(device=dev).manual_seed(13)
h_rows = unit_rows(n, gen).cpu().numpy()
h_q = unit_rows(max(batches), gen).cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def span(ts):
    return f"{min(ts):8.2f}..{np.median(ts):8.2f}..{max(ts):8.2f}"


print(f"# {n} x {d}, reps = {args.reps}; device: {fir.device_info(0)}")
print("# ms per whole host-pointer call, min..median..max of the timed calls")
print("#   case      queries | radius/1                    | knn/1                       | radius/2                    | knn/2                       |"
      " r1/k1  k2/r2  r1/r2 | radius/2 queries left to radius/1 | mean count")
with fir.Gallery(h_rows, None, 0, 0) as g:
    def line(label, qb, radius, m, knn_k):
        q = h_q[:qb]

        def rad(threshold):
            g.set_large_batch_mfma(threshold)
            return g.search_radius(q, radius, m)

        def knn(threshold):
            g.set_large_batch_mfma(threshold)
            return g.search_knn(q, knn_k)

        forms = (("r1", lambda: rad(NEVER)), ("k1", lambda: knn(NEVER)), ("r2", lambda: rad(1)), ("k2", lambda: knn(1)))
        first = {}
        for name, fn in forms:                                          # warm-up: scratch, the fp16 copy, kernel loading
            first[name] = fn()
            if name in ("r2", "k2"):
                assert g.last_dispatch()["path"] == "mfma", (name, g.last_dispatch())
        times = {name: [] for name, _ in forms}
        left = 0
        for _ in range(args.reps):
            for name, fn in forms:
                before = g.mfma_stats()["fallback_queries"]
                out, t = timed(fn)
                times[name].append(t)
                if name == "r2":
                    left += g.mfma_stats()["fallback_queries"] - before
                    c1, i1, d1 = first["r1"]
                    assert np.array_equal(out[0], c1) and np.array_equal(out[1], i1) and np.array_equal(out[2].view(np.uint32), d1.view(np.uint32)), (label, qb)
        med = {name: np.median(ts) for name, ts in times.items()}
        print(f"{label:>12s} {qb:8d} | {span(times['r1'])} | {span(times['k1'])} | {span(times['r2'])} | {span(times['k2'])} | "
              f"{med['r1'] / med['k1']:5.2f}  {med['k2'] / med['r2']:5.2f}  {med['r1'] / med['r2']:5.2f} | {left:8d} of {args.reps * qb:8d} | "
              f"{first['r1'][0].mean():.1f}", flush=True)

    g.set_large_batch_mfma(NEVER)
    kth = {}
    for k in sorted(set(ks) | {16, 1000}):                              # the K-th distance fir_search_knn reports, for every query
        kth[k] = np.nextafter(g.search_knn(h_q, k)[1][:, k - 1], INF)
    for k in ks:
        for qb in batches:
            line(f"K = {k}", qb, kth[k][:qb], k, k)
    for qb in batches:
        line("K = 1000/256", qb, kth[1000][:qb], 256, 256)
    for qb in batches:
        line("overflow", qb, INF, 16, 16)

    print("# radius/1, the library's event pairs (fir_profile_enable), radius of K = 16: ms summed over the call's tiles of 8 queries")
    print("#   max_results  queries   store pass   count + select + sort   share of the second")
    g.set_large_batch_mfma(NEVER)
    qb = min(batches)
    for m in (0, 16, 1024):
        g.search_radius(h_q[:qb], kth[16][:qb], m)
        g.profile_enable(True)
        g.profile_read()
        g.search_radius(h_q[:qb], kth[16][:qb], m)
        ms, _ = g.profile_read()
        g.profile_enable(False)
        store, sel = float(ms[0::2].sum()), float(ms[1::2].sum())
        print(f"{m:14d} {qb:8d} {store:12.3f} {sel:23.3f} {sel / (store + sel):21.3f}   # {ms.shape[0]} durations", flush=True)
