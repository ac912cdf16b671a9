"""Shared by test_gpu_pnn_mfma.py and test_pnn_mfma_formulation.py: the shapes, the splits and the bound of the matrix-core PNN
(csrc/fir_cls_pnn_mfma.h, include/fir_amd.h at fir_cls_pnn_predict).

A routed call computes S = |q-avg|^2 + |g-avg|^2 - 2 (q-avg).(g-avg) where the scan sums ((g-avg) - (q-avg))^2. First order and in
any summation order |dS| <= 2 u (d+2) (|q-avg|^2 + |g-avg|^2), u = 2^-53; a class score sum_t exp(-S / (2 d var)) / nt inherits it
divided by the denominator:

    E(q) = 2 * 2^-53 * (d + 2) * (|q-avg|^2 + max_t |g_t-avg|^2) / (2 d var)

and 2^-40 on top covers exp and the order of the class sums. A query is settled when its two largest scores s1 >= s2 satisfy
s2 (1 + B) < s1 (1 - B) with B = 2 (E(q) + 2^-40); the others (and NaN / all-zero score rows) are the scan's."""
import numpy as np

import golden_cases as gc

U = 2.0 ** -53
SLACK = 2.0 ** -40

# (seed, n, d, classes, train fraction): split as test_gpu_cls.test_matches_oracle_on_fresh_data makes it
EDGE_SHAPES = [(5, 200, 3, 4, .7), (7, 135, 1, 3, .5), (8, 129, 33, 2, .5), (9, 6000, 31, 40, .9), (11, 300, 640, 7, .43), (6, 130, 2100, 5, .5)]
# the 16-queries-per-read kernel (640 < d <= 1280: d = 1280 fills the LDS exactly) and the first row length that is not taken; 700 rows
# at .8 are nine tiles, more than one workgroup's eight waves
LDS_BOUNDARY_SHAPES = [(41, 700, 641, 6, .8), (42, 700, 1280, 6, .8), (43, 700, 1281, 6, .8)]
# (seed, n, d, classes): train mask default_rng(seed).random(n) < 0.8, class-sorted (stable), avg = the training mean
LARGER_SHAPES = [(21, 2400, 96, 12), (22, 3000, 512, 25), (23, 1500, 36, 7), (24, 4000, 257, 101), (25, 1200, 2100, 5)]


def default_var(d):
    """classification.cpp:190-193"""
    return 0.00002 / 10 if d > 2000 else 0.00002


def edge_case(oracle, seed, n, d, ncls, frac):
    x, lab, _ = gc.cls_case(seed=seed, n=n, d=d, n_classes=ncls)
    is_train = np.random.default_rng(seed).random(n) < frac
    order = np.argsort(lab[is_train], kind="stable")
    tr, tcls = x[is_train][order], lab[is_train][order]
    _, _, avg, _ = oracle.train_stats(tr)
    return tr, tcls, avg, x[~is_train][:23]


def larger_case(seed, n, d, ncls):
    x, lab, _ = gc.cls_case(seed=seed, n=n, d=d, n_classes=ncls)
    is_train = np.random.default_rng(seed).random(n) < 0.8
    order = np.argsort(lab[is_train], kind="stable")
    tr, tcls = x[is_train][order], lab[is_train][order]
    return tr, tcls, tr.mean(0), x[~is_train][:160]


def score_bound(tr, avg, q):
    """E(q) + 2^-40 per query, shape [len(q)]."""
    d = tr.shape[1]
    ng_max = (((tr - avg) ** 2).sum(1)).max()
    nq = ((np.atleast_2d(q) - avg) ** 2).sum(1)
    return 2.0 * U * (d + 2) * (nq + ng_max) / (2.0 * d * default_var(d)) + SLACK


def assert_scores_within(got, want, bound, what):
    """|got - want| <= bound[q] * |want| + 1e-300, row by row."""
    err = np.abs(got - want)
    lim = bound[:, None] * np.abs(want) + 1e-300
    bad = np.argwhere(~(err <= lim))
    assert bad.size == 0, (what, bad[:5], err[tuple(bad[0])], lim[tuple(bad[0])])


def three_term_scores(tr, tcls, avg, ncls, q):
    """The form in float64 numpy: scores [len(q), ncls]."""
    d = tr.shape[1]
    gc_, qc = tr - avg, np.atleast_2d(q) - avg
    s = ((qc * qc).sum(1)[:, None] + (gc_ * gc_).sum(1)[None, :]) - 2.0 * (qc @ gc_.T)
    e = np.exp(-s / (2.0 * d * default_var(d)))
    out = np.zeros((qc.shape[0], ncls))
    for c in range(ncls):
        out[:, c] = e[:, tcls == c].sum(1) / tr.shape[0]
    return out


def in_band(scores, bound):
    """True per query when the scan has to answer: NaN, all zero, or the two largest scores closer than the form's error."""
    top = np.sort(scores, axis=1)
    s1 = top[:, -1]
    s2 = top[:, -2] if scores.shape[1] > 1 else np.zeros_like(s1)
    b = 2.0 * bound
    with np.errstate(invalid="ignore"):
        settled = ~np.isnan(scores).any(1) & (s1 > 0) & (s2 * (1 + b) < s1 * (1 - b))
    return ~settled
