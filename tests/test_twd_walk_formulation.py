"""tests/twd_walk.py against the oracle, on the CPU: the walk over the oracle's own distance tables (oracle.all_distances over
every sub-range) gives oracle.twd_proposed / oracle.twd_conventional, integer for integer -- all three metrics, reduced
feature counts 8 to 128, the three conventional types, a gallery of 70 rows and one of 3000, 19 queries each. This is what
lets tests/test_gpu_subrange_scans.py grade a device verdict as walk(device tables)."""
import functools

import numpy as np
import pytest

import golden_cases as gc
import twd_walk

REDUCED = (8, 16, 32, 64, 128)
NQ = 19
PROP_TH = (0.7, 0.95, 0.3, 1.5)
CONV = gc.TWD_CONVENTIONAL + [(1, 0.0), (2, 0.5), (0, 0.9), (0, 0.21)]     # 0.21: inside the spread of these cases' posterior ratios
SHAPES = ((70, 7), (3000, 37))


@functools.lru_cache(maxsize=None)
def _case(n, ncls, metric):
    return twd_walk.case(31 + n % 97 + metric, n, ncls, metric, NQ)


def chunk_tables(oracle, rows, qv, step, metric):
    return np.stack([oracle.all_distances(rows, qv, lo, lo + step, metric) for lo in range(0, twd_walk.LAST_FEATURE, step)])


@pytest.mark.parametrize("n,ncls", SHAPES)
@pytest.mark.parametrize("metric", (gc.L2, gc.CHI2, gc.KL))
def test_proposed_walk_equals_the_oracle(oracle, metric, n, ncls):
    rows, cls, q = _case(n, ncls, metric)
    outcomes = set()
    for reduced in REDUCED:
        for qi in range(NQ):
            sub = chunk_tables(oracle, rows, q[qi], reduced, metric)
            for th in PROP_TH:
                exp = oracle.twd_proposed(rows, cls, q[qi], reduced, th, metric)
                assert twd_walk.proposed(sub, cls, th) == exp, (reduced, qi, th)
                outcomes.add((exp[1], exp[2] == 1, exp[2] == twd_walk.LAST_FEATURE // reduced))
    # the cases stop after one chunk, after a few and never
    assert {(0, True, False), (1, False, False), (1, False, True)} <= outcomes, outcomes


@pytest.mark.parametrize("n,ncls", SHAPES)
@pytest.mark.parametrize("metric", (gc.L2, gc.CHI2, gc.KL))
def test_conventional_walk_equals_the_oracle(oracle, metric, n, ncls):
    rows, cls, q = _case(n, ncls, metric)
    outcomes = set()
    for reduced in REDUCED:
        for qi in range(NQ):
            d1 = oracle.all_distances(rows, q[qi], 0, reduced, metric)
            d2 = oracle.all_distances(rows, q[qi], reduced, twd_walk.LAST_FEATURE, metric)
            for typ, th in CONV:
                exp = oracle.twd_conventional(rows, cls, q[qi], ncls, typ, th, reduced, metric)
                got = twd_walk.conventional(d1, d2, cls, ncls, typ, th, reduced)
                assert got[:2] == exp, (reduced, qi, typ, th)
                assert (got[2] is None) == (typ != 0)
                outcomes.add((typ, exp[1]))
    assert outcomes == {(t, u) for t in (0, 1, 2) for u in (0, 1)}, outcomes


def test_walk_edges(oracle):
    """What the synthetic galleries never hold: NaN rows (never the best row, never pruned), equal sums (the first row wins),
    nothing below 100000 (class -1), fewer classes than the five posteriors summed."""
    n, ncls = 70, 3
    rows, cls, q = _case(70, 7, gc.L2)
    rows, cls = rows.copy(), (np.arange(n) % ncls).astype(np.int32)
    rows[5] = np.nan
    rows[40, 200] = np.nan
    rows[33] = rows[9]
    cls[33] = (cls[9] + 1) % ncls
    qq = np.stack([q[0], rows[9], rows[9] * np.float32(1.001), q[NQ - 1]])
    far = np.full((n, 256), 3.0e4, np.float32)
    for rr, queries in ((rows, qq), (far, np.zeros((1, 256), np.float32))):
        for qv in queries:
            for reduced in (32, 64):
                sub = chunk_tables(oracle, rr, qv, reduced, gc.L2)
                for th in PROP_TH if rr is rows else ():          # (with no row below 100000 the oracle reads class_no[-1])
                    assert twd_walk.proposed(sub, cls, th) == oracle.twd_proposed(rr, cls, qv, reduced, th), (reduced, th)
                d1 = oracle.all_distances(rr, qv, 0, reduced, gc.L2)
                d2 = oracle.all_distances(rr, qv, reduced, 256, gc.L2)
                for typ, th in CONV:
                    assert twd_walk.conventional(d1, d2, cls, ncls, typ, th, reduced)[:2] == oracle.twd_conventional(rr, cls, qv, ncls, typ, th, reduced)
    assert twd_walk.proposed(chunk_tables(oracle, far, np.zeros(256, np.float32), 32, gc.L2), cls, 0.7) == (-1, 0, 1)
