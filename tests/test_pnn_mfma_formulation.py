"""The three-term form of the matrix-core PNN (csrc/fir_cls_pnn_mfma.h) in float64 numpy against the oracle's PNN:

    S = |q-avg|^2 + |g-avg|^2 - 2 (q-avg).(g-avg)     instead of     sum_k ((g-avg) - (q-avg))^2

Every class score stays within E(q) + 2^-40 relative of the oracle's (pnn_mfma_cases.score_bound: the formula k_cls_pnn_band
evaluates on the device), and on the five larger shapes no query falls inside the band that sends a query back to the scan -- so a
fallback count above a handful on the GPU (test_gpu_pnn_mfma.py) means a broken kernel, not a cautious band."""
import numpy as np
import pytest

import pnn_mfma_cases as pc


def check(oracle, tr, tcls, avg, ncls, q):
    got = pc.three_term_scores(tr, tcls, avg, ncls, q)
    want = np.array([oracle.pnn_predict(tr, tcls, avg, ncls, qi)[1] for qi in q])
    bound = pc.score_bound(tr, avg, q)
    pc.assert_scores_within(got, want, bound, "three-term form against the oracle")
    return got, want, bound


@pytest.mark.parametrize("seed,n,d,ncls", pc.LARGER_SHAPES)
def test_the_form_stays_inside_its_bound_and_the_band_is_empty(oracle, seed, n, d, ncls):
    tr, tcls, avg, q = pc.larger_case(seed, n, d, ncls)
    assert q.shape[0] == 160
    got, want, bound = check(oracle, tr, tcls, avg, ncls, q)
    assert pc.in_band(got, bound).sum() == 0
    assert np.array_equal(got.argmax(1), want.argmax(1))


@pytest.mark.parametrize("seed,n,d,ncls,frac", [s for s in pc.EDGE_SHAPES if s[2] in (1, 3)])
def test_the_bound_holds_where_the_denominator_is_smallest(oracle, seed, n, d, ncls, frac):
    """d = 3 and d = 1: the denominator 2 d var is at its smallest, E(q) at its largest (1.8e-11 at d = 3)."""
    tr, tcls, avg, q = pc.edge_case(oracle, seed, n, d, ncls, frac)
    got, want, bound = check(oracle, tr, tcls, avg, ncls, q)
    settled = ~pc.in_band(got, bound)
    assert np.array_equal(got.argmax(1)[settled], want.argmax(1)[settled])       # outside the band the classes are the oracle's


def test_the_bound_formula():
    """Pinned numbers: unit-norm-like rows at d = 512 and the reference's var give 2.0e-12 + 2^-40; d > 2000 divides var by 10."""
    tr = np.zeros((2, 512)); tr[0, 0] = 0.6; tr[1, 1] = 0.8
    avg = np.zeros(512)
    q = np.zeros((1, 512)); q[0, 2] = 0.6
    e = pc.score_bound(tr, avg, q)[0] - pc.SLACK
    assert e == pytest.approx(2 * 2.0 ** -53 * 514 * (0.36 + 0.64) / (2 * 512 * 2e-5), rel=1e-12)
    assert pc.default_var(2100) == pytest.approx(2e-6) and pc.default_var(2000) == 2e-5
    sc = np.array([[1.0, 1.0 - 1e-13, 0.0], [1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [np.nan, 0.5, 0.1]])
    assert pc.in_band(sc, np.full(4, 1e-12)).tolist() == [True, False, True, True]
