#!/usr/bin/env python3
"""A fixed list of TWD calls whose kernel launches can be counted from outside: both classifiers, conventional types 0
and 1, 1 / 8 / 9 queries per call, FIR_TWD_FUSED = 0 / 1 / 2, against a single-segment gallery (3 000 x 256, 37 classes) and
one that is multi-segment in both classifiers (20 001 x 256, 40 classes). No existing test can tell which form of a driver ran;
the table of kernel name -> launches of a kernel trace of this script can (profiles/small_call_plumbing_ab.txt).
usage: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/twd_launches.py     (FIR_AMD_LIB selects the build)"""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library: both bring a HIP runtime, torch's has to initialise first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import golden_cases as gc  # noqa: E402


def main():
    fir = ge.load_package()
    digest = []
    for seed, n, ncls in ((31, 3000, 37), (32, 20001, 40)):
        rows, cls, q, _ = gc.twd_case(seed=seed, n=n, d=256, n_classes=ncls)
        with fir.Gallery(rows, cls, gc.L2, 0) as g:
            for mode in ("0", "1", "2"):
                os.environ["FIR_TWD_FUSED"] = mode       # read by the library once per call
                for qb in (1, 8, 9):
                    for typ, th in ((0, 0.24), (1, 0.003)):
                        c, u = g.twd_conventional(q[:qb], ncls, typ, th, 64)
                        digest.append(int(c.sum()) * 131 + int(u.sum()))
                    c, u, k = g.twd_proposed(q[:qb], 32, 0.7)
                    digest.append(int(c.sum()) * 131 + int(u.sum()) * 17 + int(k.sum()))
    del os.environ["FIR_TWD_FUSED"]
    print("twd_launches: 54 calls, verdict digest", " ".join(str(v) for v in digest), flush=True)


if __name__ == "__main__":
    main()
