"""Times of the in-place gallery updates (fir_gallery_append / _set_rows / _remove_rows) -- one GPU, L2, 512 features, f32, labelled
galleries of 100 000 and 1 000 000 rows. Whole host-pointer calls on the host clock (each ends in a synchronisation), after one
warm-up round; the forms that are compared alternate inside one run, and every line gives min / median / max of --reps rounds.

  (a) append of 64 / 4 096 / 65 536 rows to a handle with room reserved, against what a caller had to do before: fir_gallery_destroy
      plus fir_gallery_create over n + m rows (unchanged code); and the same appends when they have to grow the buffers
  (b) fir_gallery_set_rows and fir_gallery_remove_rows of 64 and 4 096 rows
  (c) the first routed top-1 batch of 1 024 queries after a mutation (the matrix-core state and its copies are rebuilt), against a
      steady-state routed batch and the first routed batch on a fresh handle (the process has loaded its kernels on another handle
      before)

Every configuration runs in a child process of its own under its own time limit, one at a time; the first one that fails or runs
out of time ends the run. The lines go to stdout and to profiles/gallery_update.txt.

    python tools/gallery_update_probe.py [--reps 3] [--limit 420] [--small]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "gallery_update.txt")


def spread(ts):
    ts = sorted(ts)
    return f"{ts[0] * 1e3:10.3f} / {ts[len(ts) // 2] * 1e3:10.3f} / {ts[-1] * 1e3:10.3f} ms"


def clock(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def child(cfg):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    fir = ge.load_package()
    dev = torch.device("cuda", 0)
    n, d, part, reps = cfg["n"], cfg["d"], cfg["part"], cfg["reps"]
    extra = 65536
    gen = torch.Generator(device=dev).manual_seed(11 + n)
    x = torch.rand((n + extra, d), generator=gen, device=dev)
    rows = (x / x.norm(dim=1, keepdim=True)).cpu().numpy()
    del x
    torch.cuda.empty_cache()
    labels = (np.arange(n + extra, dtype=np.int32) // 10).astype(np.int32)
    tag = f"{n:>8d} x {d}"
    if part == "a":
        for m in cfg["ms"]:
            ta, tc, tg = [], [], []
            g = fir.Gallery(rows[:n], labels[:n], 0, 0)
            g.reserve(n + m)
            for r in range(reps + 1):
                t = clock(lambda: g.append(rows[n:n + m], labels[n:n + m]))
                assert g.n == n + m
                g.remove_rows(np.arange(n, n + m, dtype=np.int32))            # (the tail: nothing moves)
                h = fir.Gallery(rows[:n], labels[:n], 0, 0)                     # (what the caller held before)

                def recreate():
                    nonlocal h
                    h.close()
                    h = fir.Gallery(rows[:n + m], labels[:n + m], 0, 0)

                t2 = clock(recreate)
                h.close()
                if r >= 1:
                    ta.append(t)
                    tc.append(t2)
            g.close()
            for r in range(reps):                                             # a handle with no room: the append grows the buffers
                g = fir.Gallery(rows[:n], labels[:n], 0, 0)
                tg.append(clock(lambda: g.append(rows[n:n + m], labels[n:n + m])))
                g.close()
            med = lambda ts: sorted(ts)[len(ts) // 2]
            print(f"(a) {tag} append m={m:6d}: room reserved {spread(ta)}   destroy + create of n + m rows {spread(tc)}   (median ratio {med(tc) / med(ta):8.1f})   "
                  f"append that grows {spread(tg)}", flush=True)
    elif part == "b":
        rng = np.random.default_rng(5)
        with fir.Gallery(rows[:n], labels[:n], 0, 0) as g:
            g.reserve(n + 4096)
            for m in cfg["ms"]:
                ts, tr = [], []
                for r in range(reps + 1):
                    idx = rng.choice(n, m, replace=False).astype(np.int32)
                    t = clock(lambda: g.set_rows(idx, rows[n:n + m], labels[n:n + m]))
                    t2 = clock(lambda: g.remove_rows(idx))
                    g.append(rows[n:n + m], labels[n:n + m])
                    if r >= 1:
                        ts.append(t)
                        tr.append(t2)
                print(f"(b) {tag} m={m:6d}: set_rows {spread(ts)}   remove_rows {spread(tr)}", flush=True)
    else:
        qb = 1024
        q = rows[n:n + qb].copy()
        with fir.Gallery(rows[:4099], labels[:4099], 0, 0) as w:          # the process loads the matrix-core kernels here
            w.set_large_batch_mfma(1)
            w.search_top1(q)
        fresh, steady, after = [], [], []
        for r in range(reps):
            with fir.Gallery(rows[:n], labels[:n], 0, 0) as g:
                fresh.append(clock(lambda: g.search_top1(q)))
                assert g.last_dispatch()["path"] == "mfma", g.last_dispatch()
                g.search_top1(q)
                steady.append(clock(lambda: g.search_top1(q)))
                g.set_rows(np.arange(64, dtype=np.int32) * 97, rows[n:n + 64])
                after.append(clock(lambda: g.search_top1(q)))
                assert g.last_dispatch()["path"] == "mfma", g.last_dispatch()
                steady.append(clock(lambda: g.search_top1(q)))
        print(f"(c) {tag} routed top-1, {qb} queries: steady state {spread(steady)}   first call on a fresh handle {spread(fresh)}   "
              f"first call after a mutation {spread(after)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds per configuration")
    ap.add_argument("--small", action="store_true", help="100 000 rows only")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        child(json.loads(args.one))
        return 0
    cfgs = []
    for n in (100_000,) if args.small else (100_000, 1_000_000):
        cfgs.append(dict(part="a", n=n, d=512, ms=[64, 4096, 65536], reps=args.reps))
        cfgs.append(dict(part="b", n=n, d=512, ms=[64, 4096], reps=args.reps))
        cfgs.append(dict(part="c", n=n, d=512, reps=args.reps))
    lines = ["fir_gallery_append / _set_rows / _remove_rows -- tools/gallery_update_probe.py, one GPU, L2, 512 features, f32, labelled (10 rows per class)",
             f"whole host-pointer calls on the host clock, min / median / max of {args.reps} rounds after one warm-up round, the compared forms alternating in one run",
             "(a) append with room reserved against destroy + create of n + m rows; the same append when it has to grow the buffers (fresh handle each time)",
             "(b) set_rows / remove_rows of m random rows",
             "(c) routed top-1 batches of 1 024 queries: steady state, the first on a fresh handle, the first after a mutation (state and copies rebuilt)"]
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
