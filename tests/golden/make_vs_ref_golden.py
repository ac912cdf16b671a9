#!/usr/bin/env python3
"""Generate tests/golden/oracle_vs_ref.npz: the REAL reference code's results (oracle/_ref, built by oracle/build_ref.sh)
for the cases of tests/test_oracle_vs_ref.py -- outputs plus the reference's own shuffled splits, no reference source.

Run where oracle/_ref is built:   python tests/golden/make_vs_ref_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib  # noqa: E402
import test_oracle_vs_ref as t  # noqa: E402


def main():
    if not oracle_lib.have_ref():
        raise SystemExit("oracle/_ref is not built")
    out = os.path.join(HERE, "oracle_vs_ref.npz")
    np.savez_compressed(out, **t.all_recorded())
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
