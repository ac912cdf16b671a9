"""numpy restatement of the linear projection / PCA calls (include/fir_amd.h) and the bounds the GPU tests hold them to.

"Exact" below is numpy longdouble (64-bit mantissa on x86) over exactly widened float32 inputs; the sums the tests compare are at
most a few thousand terms long, so the reference's own rounding is below 2^-52 of the sum of magnitudes -- the factor 2 in 2^-52
(instead of the unit roundoff 2^-53) of every bound covers it.

Bounds, first order, for float64 accumulation of m terms in ANY order (Higham, Accuracy and Stability, section 4.2: (m - 1) u sum|t|)
plus the roundings of forming the terms:
  projection  |y_dev - y| <= ulp32(y) / 2 + (d + 3) 2^-52 sum_f (|x_f| + |c_f|) |W_kf|
              (d products, d - 1 additions, the bias' own d-term sum, one subtraction; one rounding to float32 at the end)
  scatter     |S_dev - S| <= (m + 6) 2^-52 sum_j |x_ja - c_a| |x_jb - c_b|,  m = selected rows
              (each factor rounded once when centred, each product once, m - 1 additions)
  sums        |sum_dev - sum| <= (m + 2) 2^-52 sum |x|   (the same with x^2 for the sum of squares: the squares are exact)
"""
import numpy as np

LD = np.longdouble
F32, F64 = np.float32, np.float64
U = 2.0 ** -52
FLT_MAX = float(np.finfo(np.float32).max)


def selected(take, n):
    return np.ones(n, bool) if take is None else np.asarray(take, bool)


def column_sums(rows, take=None):
    """(count, sum, sum of squares, sum |x|) over the selected rows, longdouble."""
    x = rows[selected(take, rows.shape[0])].astype(LD)
    return x.shape[0], x.sum(axis=0), (x * x).sum(axis=0), np.abs(x).sum(axis=0)


def min_max(rows, take=None):
    """Exact: the reference starts at FLT_MAX / -FLT_MAX and compares with < and >."""
    x = rows[selected(take, rows.shape[0])]
    d = rows.shape[1]
    if x.shape[0] == 0:
        return np.full(d, FLT_MAX, F64), np.full(d, -FLT_MAX, F64)
    return np.minimum(x.min(axis=0).astype(F64), FLT_MAX), np.maximum(x.max(axis=0).astype(F64), -FLT_MAX)


def std_formula(sum_x, sum_sq, count):
    """split_train_test's literal formula in IEEE double (classification.cpp:969-989) from the two sums."""
    with np.errstate(all="ignore"):
        cnt = F64(count)
        avg = np.asarray(sum_x, F64) / cnt
        return avg, np.sqrt((np.asarray(sum_sq, F64) - avg * avg * cnt) / (cnt - F64(1.0)))


def sums_bound(abs_sum, m):
    return (m + 2) * U * np.asarray(abs_sum, F64)


def scatter(rows, take, center):
    """(S, B): the exact scatter matrix about `center` (float64[d], as the device receives it) over the selected rows, and the
    bound on |S_dev - S| element by element."""
    sel = selected(take, rows.shape[0])
    z = rows[sel].astype(LD) - np.asarray(center, F64).astype(LD)
    s = z.T @ z
    b = (int(sel.sum()) + 6) * U * (np.abs(z).T @ np.abs(z)).astype(F64)
    return s, b


def project(rows, basis, center=None):
    """(y, B): y[j][k] = sum_f x_jf W_kf - sum_f c_f W_kf exactly (longdouble), and the bound on |y_dev - y| including the final
    rounding to float32."""
    x = rows.astype(LD)
    w = np.asarray(basis, F64).astype(LD)
    d = w.shape[1]
    c = np.zeros(d, LD) if center is None else np.asarray(center, F64).astype(LD)
    y = x @ w.T - (w @ c)[None, :]
    mag = ((np.abs(x) + np.abs(c)[None, :]) @ np.abs(w).T).astype(F64)
    y64 = y.astype(F64)
    ulp32 = np.ldexp(1.0, np.maximum(np.frexp(np.abs(y64))[1] - 24, -149))       # of the binade y lies in: |y| = m 2^e, m in [0.5, 1)
    return y, ulp32 / 2 + (d + 3) * U * mag


def within(got, exact, bound):
    """Every |got - exact| <= bound; returns the worst ratio for the message."""
    err = np.abs(np.asarray(got, F64).astype(LD) - exact).astype(F64)
    ok = err <= bound
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return bool(np.all(ok)), float(np.max(ratio)) if ratio.size else 0.0


# ---- the end-to-end case: 700 x 48, low rank plus noise, L2-normalised rows, half the rows as the training mask, p = 12 --------------
E2E_N, E2E_D, E2E_P, E2E_RANK, E2E_GAP = 700, 48, 12, 10, 2.0 ** -18


def e2e_data(seed=20261):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((E2E_N, E2E_RANK)) @ rng.standard_normal((E2E_RANK, E2E_D)) + 0.7
    rows = base + 0.05 * rng.standard_normal((E2E_N, E2E_D))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows = rows.astype(F32)
    q = rows.astype(F64) + 0.02 * rng.standard_normal((E2E_N, E2E_D)) / np.sqrt(E2E_D)
    take = rng.random(E2E_N) < 0.5
    return rows, q.astype(F32), take


def e2e_float64(rows, queries, take):
    """The float64 pipeline: covariance of the training rows, numpy.linalg.eigh, the leading p components, squared L2 distances of
    the projected queries to the projected rows. Returns (basis [p][d], mean, top-1 row per query, graded[q]): a query is graded
    when its two best float64 distances differ by more than 2^-18 relative."""
    x = rows[take].astype(F64)
    mean = x.mean(axis=0)
    z = x - mean
    vals, vecs = np.linalg.eigh(z.T @ z)
    basis = vecs[:, ::-1][:, :E2E_P].T.copy()
    return (basis, mean) + e2e_grade(rows, queries, basis, mean)


def e2e_grade(rows, queries, basis, mean):
    yg = (rows.astype(F64) - mean) @ basis.T
    yq = (queries.astype(F64) - mean) @ basis.T
    dist = ((yq[:, None, :] - yg[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]
    d1 = np.take_along_axis(dist, order[:, :1], 1)[:, 0]
    d2 = np.take_along_axis(dist, order[:, 1:2], 1)[:, 0]
    graded = (d2 - d1) > E2E_GAP * d2
    return order[:, 0], graded
