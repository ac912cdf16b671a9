"""projection_ref's bounds hold for float64 sums taken in another order, and its end-to-end case grades (nearly) every query.
No GPU: numpy only."""
import numpy as np

import projection_ref as pr

F32, F64 = np.float32, np.float64


def data(seed, n, d):
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.integers(-20, 11, size=(n, d))                    # values spanning 2^-20 .. 2^10
    return (rng.standard_normal((n, d)) * scale + 0.25 * scale).astype(F32)


def chunked_shuffled_sum(terms, rng, chunk=64):
    """float64 sum of terms[m, ...] along axis 0 in a shuffled order, chunk partials first, partials folded in order."""
    t = terms[rng.permutation(terms.shape[0])]
    acc = np.zeros(t.shape[1:], F64)
    for c0 in range(0, t.shape[0], chunk):
        part = np.zeros(t.shape[1:], F64)
        for row in t[c0:c0 + chunk]:
            part = part + row
        acc = acc + part
    return acc


def test_a_shuffled_chunked_float64_order_stays_inside_the_projection_bound():
    rng = np.random.default_rng(1)
    n, d, p = 40, 130, 17
    rows = data(2, n, d)
    basis = rng.standard_normal((p, d))
    center = rows.astype(F64).mean(axis=0)
    exact, bound = pr.project(rows, basis, center)
    bias = np.zeros(p, F64)
    for f in range(d):
        bias = bias + center[f] * basis[:, f]
    terms = rows.astype(F64).T[:, :, None] * basis.T[:, None, :]         # [d][n][p], each product rounded once
    got = (chunked_shuffled_sum(terms, rng, 16) - bias[None, :]).astype(F32)
    ok, worst = pr.within(got, exact, bound)
    assert ok, worst


def test_a_shuffled_chunked_float64_order_stays_inside_the_scatter_and_sum_bounds():
    rng = np.random.default_rng(3)
    n, d = 700, 9
    rows = data(4, n, d)
    take = rng.random(n) < 0.6
    m, s, sq, sabs = pr.column_sums(rows, take)
    x = rows[take].astype(F64)
    ok, worst = pr.within(chunked_shuffled_sum(x, rng), s, pr.sums_bound(sabs, m))
    assert ok, worst
    ok, worst = pr.within(chunked_shuffled_sum(x * x, rng), sq, pr.sums_bound(sq.astype(F64), m))
    assert ok, worst
    center = (s / m).astype(F64)
    exact, bound = pr.scatter(rows, take, center)
    z = x - center
    got = chunked_shuffled_sum(z[:, :, None] * z[:, None, :], rng)
    ok, worst = pr.within(got, exact, bound)
    assert ok, worst


def test_the_std_formula_is_the_literal_one():
    rows = data(5, 50, 3)
    m, s, sq, _ = pr.column_sums(rows)
    avg, sd = pr.std_formula(s.astype(F64), sq.astype(F64), m)
    assert np.allclose(avg, rows.astype(F64).mean(axis=0), rtol=1e-12)
    assert np.allclose(sd, rows.astype(F64).std(axis=0, ddof=1), rtol=1e-6)
    with np.errstate(all="ignore"):
        _, sd1 = pr.std_formula(s.astype(F64), sq.astype(F64), 1)        # count 1: 0 / 0 or x / 0, whatever the formula yields
    assert not np.any(np.isfinite(sd1))


def test_the_end_to_end_inputs_leave_at_most_five_percent_ungraded():
    rows, q, take = pr.e2e_data()
    assert rows.shape == (pr.E2E_N, pr.E2E_D) and 300 < take.sum() < 400
    assert np.allclose(np.linalg.norm(rows.astype(F64), axis=1), 1.0, atol=1e-6)
    basis, mean, top1, graded = pr.e2e_float64(rows, q, take)
    assert basis.shape == (pr.E2E_P, pr.E2E_D)
    assert np.mean(~graded) <= 0.05, np.mean(~graded)
    assert np.mean(top1 == np.arange(pr.E2E_N)) > 0.5                     # the noise is small enough for the case to mean something
