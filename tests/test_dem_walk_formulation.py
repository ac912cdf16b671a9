"""The order-free form of DirectedEnumeration::recognize that fir_dem_recognize computes on the device (include/fir_amd.h;
restated in tests/dem_walk.py) against the oracle's literal walk, on small random cases built to have ties: integer-valued
features and table entries (equal likelihoods, equal distances), pivots at positions below the number of pivots (the
two-write quirk of ann.cpp:431-432: likelihood_indices holds a row twice), every count to check from "pivots only" to
the whole gallery, thresholds that never, sometimes and always fire. And the property the tie flag stands for: with
tie == 0 the walk that takes equal likelihoods in DESCENDING position order gives the same answer."""
import numpy as np

import dem_walk


def bits(x):
    return int(np.float32(x).view(np.uint32))


def _cases(n_cases=250):
    rng = np.random.default_rng(20240607)
    for c in range(n_cases):
        n = int(rng.integers(8, 201))
        d = int(rng.integers(1, 4))
        used = int(rng.integers(1, 6))
        rows = rng.integers(0, 4, (n, d)).astype(np.float32)
        q = rng.integers(0, 4, d).astype(np.float32)
        piv = rng.permutation(n)[:used].astype(np.int32)
        if c % 2 and used > 1:
            piv[1] = 0 if piv[0] != 0 else 1                     # a pivot below `used`: the index array loses a row
            piv = np.array(list(dict.fromkeys(piv.tolist())), np.int32)
        table = rng.integers(-1, 4, (piv.size, n)).astype(np.float32)
        if c % 3 == 0:                                           # no equal likelihoods but the quirk's
            table = rng.random((piv.size, n), dtype=np.float32)
        yield n, d, rows, q, piv, table


def test_formulation_equals_the_walk_and_the_flag_covers_every_tie(oracle):
    checked = flagged = exits = quirks = plain = 0
    for n, d, rows, q, piv, table in _cases():
        used = piv.size
        dist = oracle.all_distances(rows, q, 0, d, 0)
        pd = dist[piv]
        order = dem_walk.order_after_pivots(n, piv)
        quirks += len(set(order.tolist())) < n
        lik = dem_walk.likelihoods(n, piv, table, pd)
        *_, elik = oracle.dem_recognize(rows, piv, table, 0.0, used, q, 0, want_lik=True)
        assert np.array_equal(lik.view(np.uint32), elik.view(np.uint32))
        for M in sorted({used, used + 1, (used + n) // 2, n}):
            for thr in (0.0, float(np.median(dist)), 1e9):
                want = oracle.dem_recognize(rows, piv, table, thr, M, q, 0)
                row, best, found, calc, tie = dem_walk.formulation(pd, piv, order, lik, dist, M, thr)
                assert (row, bits(best), found, calc) == (want[0], bits(want[1]), want[2], want[3]), (n, used, M, thr)
                asc = dem_walk.sequential_walk(pd, piv, order, lik, dist, M, thr)
                assert (asc[0], bits(asc[1]), asc[2], asc[3]) == (want[0], bits(want[1]), want[2], want[3])
                if tie == 0:
                    desc = dem_walk.sequential_walk(pd, piv, order, lik, dist, M, thr, descending=True)
                    assert (desc[0], bits(desc[1]), desc[2], desc[3]) == (row, bits(best), found, calc), (n, used, M, thr)
                checked += 1
                flagged += tie
                exits += found
                plain += tie == 0 and M > used and calc > used
    # the cases do what they were built for: ties, early exits and the quirk all occur, and not every case is flagged
    assert checked > 2000 and flagged > 100 and plain > 100 and 0 < exits < checked and quirks > 20, (checked, flagged, plain, exits, quirks)
