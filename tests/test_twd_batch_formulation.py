"""The second-stage certificate of fir_twd_conventional's matrix-core batch form (csrc/fir_twd_batch.h), in
numpy float32 with every sum taken feature by feature as the kernels and the reference take it:

    d_256 = (sum_{f < 256} (q_f - g_f)^2) / 256                                    the distance the eight nominated rows are ranked by
    v     = ((double)d1 * r + (float)(d2 * (256 - r))) / 256                       ImageTesting.cpp:173-174, d1 over [0, r), d2 over [r, 256)

Whenever  d_256(8th nearest row) * (1 - 2^-14) - 256 * 2^-149 > v_best  holds, the first minimum of v over ALL rows is the first
minimum over the 8 nearest rows by (d_256, row); and the inequality holds on every plain query -- including rows one ulp away from
the nearest row in a few features -- and fails, as it must, where duplicates fill the eight."""
import numpy as np
import pytest

import synth

CERT_REL = 2.0 ** -14          # kMfmaCertRel
CERT_ABS = 256.0 * 2.0 ** -149  # kMfmaCertAbs
N, D, QB = 3000, 256, 40


def seq_sum_sq(q, rows, lo, hi):
    """sum_{f in [lo, hi)} (q_f - g_f)^2 in float32, one rounding per operation, in feature order -- for every row at once."""
    acc = np.zeros(rows.shape[0], np.float32)
    for f in range(lo, hi):
        df = (q[f] - rows[:, f]).astype(np.float32)
        acc = (acc + (df * df).astype(np.float32)).astype(np.float32)
    return acc


def d256_and_v(q, rows, r):
    d256 = (seq_sum_sq(q, rows, 0, 256) / np.float32(256)).astype(np.float32)
    d1 = (seq_sum_sq(q, rows, 0, r) / np.float32(r)).astype(np.float32)
    d2 = (seq_sum_sq(q, rows, r, 256) / np.float32(256 - r)).astype(np.float32)
    tail = (d2 * np.float32(256 - r)).astype(np.float32)
    v = (d1.astype(np.float64) * r + tail.astype(np.float64)) / 256
    return d256, v


def first_min(values, candidates=None):
    """The reference's loop: strict '<' from 100000 over rows in ascending order; -1 when nothing qualifies."""
    idx = np.arange(values.size) if candidates is None else np.sort(candidates)
    best, where = 100000.0, -1
    for i in idx:
        if values[i] < best:
            best, where = values[i], int(i)
    return where


def nominate(d256):
    """The 8 nearest rows by (d_256, row) among the rows below 100000 -- fir_search_topk's keys."""
    order = np.lexsort((np.arange(d256.size), d256))
    order = order[d256[order] < np.float32(100000.0)]
    return order[:8]


def certified(d256, v, eight):
    if eight.size < 8:
        return False
    vb = first_min(v, eight)
    return vb >= 0 and float(d256[eight[7]]) * (1.0 - CERT_REL) - CERT_ABS > v[vb]


@pytest.fixture(scope="module")
def data():
    rows = (synth.make_gallery(91, N, D, 0) * np.float32(4)).astype(np.float32)
    q, pick = synth.make_queries(91, rows, QB, 0, noise=0.4)
    q = q.astype(np.float32)
    return rows, q, pick


@pytest.mark.parametrize("r", [64, 128, 240])
def test_the_certificate_holds_on_plain_queries_and_implies_the_full_scans_answer(data, r):
    rows, q, _ = data
    held = 0
    for qi in q:
        d256, v = d256_and_v(qi, rows, r)
        eight = nominate(d256)
        assert certified(d256, v, eight)
        assert first_min(v, eight) == first_min(v)
        held += 1
    assert held == QB


@pytest.mark.parametrize("r", [64, 128])
def test_rows_one_ulp_from_the_nearest_row_and_exact_duplicates(data, r):
    rows, q, _ = data
    rows = rows.copy()
    rng = np.random.default_rng(3)
    some_certified = some_not = 0
    for k, qi in enumerate(q[:12]):
        d256, _ = d256_and_v(qi, rows, r)
        near = int(nominate(d256)[0])
        g = rows.copy()
        # up to seven rows that differ from the nearest row by one ulp in a few features: d_256 and v may order them differently
        for j in range(1 + k % 7):
            twin = g[near].copy()
            for f in rng.integers(0, 256, 3):
                twin[f] = np.nextafter(twin[f], np.float32(8), dtype=np.float32)
            g[(near + 97 * (j + 1)) % N] = twin
        if k % 3 == 2:                                       # exact duplicates, scattered: with 12 of them the eight are all ties
            for j in range(12):
                g[(near + 211 * (j + 1)) % N] = g[near]
        d256, v = d256_and_v(qi, g, r)
        eight = nominate(d256)
        if certified(d256, v, eight):
            some_certified += 1
            assert first_min(v, eight) == first_min(v), k
        else:
            some_not += 1
        if k % 3 == 2:
            assert not certified(d256, v, eight), k         # a tie with the 8th row never certifies
        elif k % 7 < 6:
            assert certified(d256, v, eight), k             # fewer than 8 near-twins: the 8th row is an ordinary one, percent away
    assert some_certified and some_not


def test_hostile_rows_never_certify_a_wrong_row(data):
    rows, q, _ = data
    g = rows.copy()
    g[5] = np.nan
    g[700, 3] = np.inf
    g[9] = np.float32(3.0e4)                               # squared distances above the 100000 start value
    for qi in q[:6]:
        with np.errstate(invalid="ignore", over="ignore"):
            d256, v = d256_and_v(qi, g, 64)
        eight = nominate(d256)
        assert not np.isin(eight, [5, 700, 9]).any()
        if certified(d256, v, eight):
            assert first_min(v, eight) == first_min(v)
    tiny = g[:5].copy()                                    # fewer than 8 rows: no certificate
    d256, v = d256_and_v(q[0], tiny, 64)
    assert not certified(d256, v, nominate(d256))
