"""The host side of the float64 classifier (csrc/fir_cls.hip), branch by branch: which form of the distance scan a call over a
training set streamed from HBM takes and that every form gives the same bits; the three ways a class comes back to the caller
(ticket, pinned slots, staged copy); the sequential PNN's other kernels; one handle's scratch shared by every entry point; and
what a profiled call of the two matrix-core forms leaves behind. Shapes are the smallest that reach each branch."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCHES = (1, 8, 9, 24, 37, 64)
F4 = "fir::k_cls_scan_lds<2, 4, 512, 2, 2>"       # four tiles of eight queries per read of the rows
F2 = "fir::k_cls_scan_lds<4, 2, 256, 2, 2>"       # two
F1 = "fir::k_cls_scan_lds<8, 1>"                  # one
# (timed launches, last kernel) by the rule in cls_scan: a call of ceil(nq / 8) tiles is cut into groups of 4, 2, 1 tiles -- four only
# while 4 x (2 dp2 + 1) x 64 bytes of LDS fit 150 KiB (d = 512: 131 328; d = 640: 164 096, two tiles at most) --, one launch per form
# and at most 64 tiles; tiles: 1, 1, 2, 3, 5, 8.
LAUNCHES = {
    512: {1: (1, F1), 8: (1, F1), 9: (1, F2), 24: (2, F1), 37: (2, F1), 64: (1, F4)},
    513: {1: (1, F1), 8: (1, F1), 9: (1, F2), 24: (2, F1), 37: (2, F1), 64: (1, F4)},
    640: {1: (1, F1), 8: (1, F1), 9: (1, F2), 24: (2, F1), 37: (2, F1), 64: (1, F2)},
}


def clustered(n, d, ncls, seed, nq, tcls=None):
    """Class-major float64 rows, class centres + noise: the PNN scores of the right class are not denormal, a query's nearest rows are its class's."""
    rng = np.random.default_rng(seed)
    centres = rng.random((ncls, d))
    if tcls is None:
        tcls = np.sort(rng.integers(0, ncls, n)).astype(np.int32)
    tr = centres[tcls] + 0.004 * rng.standard_normal((n, d))
    q = centres[rng.integers(0, ncls, nq)] + 0.004 * rng.standard_normal((nq, d))
    return tr, tcls, q


def hbm_rows(d):
    """The fewest tiles of 64 rows the library streams from HBM (tiles * 64 * dp2 * 16 > 2^28), the last tile partly empty."""
    dp2 = (d + 1) // 2
    return ((1 << 28) // (64 * dp2 * 16) + 1) * 64 - 17


@functools.lru_cache(maxsize=1)
def hbm_data(d):
    tr, tcls, q = clustered(hbm_rows(d), d, 7, 100 + d, 64)
    tr[5] = tr[4]                                   # two rows of class 0 at equal distance from everything
    q[0] = tr[4]
    return tr, tcls, tr.mean(0), q


def same_bits(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(u, v) for u, v in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- scan forms over a training set streamed from HBM ----

@pytest.fixture(scope="module", params=[512, 640, 1024, 513])
def hbm_set(request, fir):
    d = request.param
    tr, tcls, avg, q = hbm_data(d)
    dp2 = (d + 1) // 2
    tiles = (tr.shape[0] + 63) // 64
    assert tiles * 64 * dp2 * 16 > 1 << 28 >= (tiles - 1) * 64 * dp2 * 16
    with fir.ClsModel(tr, tcls, 7, avg, 0) as m:
        yield d, tr, tcls, avg, q, m, m.distance_sums(q)


@pytest.mark.parametrize("one_tile", [False, True])
def test_every_scan_form_gives_the_same_bits(hbm_set, monkeypatch, one_tile):
    """1, 8, 9, 24, 37 and 64 queries: the sums of q[:nq] are the first nq of the 64-query call's, bit for bit; the timed launches
    and the last kernel are what the rule gives (d = 1024: the query tile exceeds 64 KiB, k_cls_scan<8> runs, which is not timed).
    FIR_CLS_ONE_TILE=1: the same bits from one launch of the one-tile form per 64 tiles."""
    d, tr, tcls, avg, q, m, full = hbm_set
    if one_tile:
        monkeypatch.setenv("FIR_CLS_ONE_TILE", "1")
    m.profile_enable(True)
    try:
        for nq in BATCHES:
            part = m.distance_sums(q[:nq])
            ms, _, name = m.profile_read()
            assert same_bits(part, full[:nq]), (d, nq)
            if d in LAUNCHES:
                assert (len(ms), name) == ((1, F1) if one_tile else LAUNCHES[d][nq]), (d, nq)
            else:
                assert len(ms) == 0 and "k_cls_scan_lds" not in name, (d, nq, name)
    finally:
        m.profile_enable(False)


def test_scan_sums_are_the_oracles_bits(hbm_set, oracle):
    d, tr, tcls, avg, q, m, full = hbm_set
    for i in (3, 63):
        _, dist = oracle.knn_predict(tr, tcls, avg, 7, q[i], 1)             # mean distances (sum / d)
        assert same_bits(full[i] / d, dist), (d, i)


# ---- how the classes come back: ticket, pinned slots, staged copy ----

def ask(m, q):
    """every class-returning entry point for q: (pnn class, pnn scores, knn-1, knn-3, seq class, seq chunks)"""
    return m.pnn_predict(q) + (m.knn_predict(q, 1), m.knn_predict(q, 3)) + m.pnn_predict_seq(q)


PIN_QUERY_BYTES, PIN_SLOTS = 256 * 1024, 2048       # the library's pinned staging: bytes of queries, result slots per array


def pinned_queries(d):
    """The largest call whose queries and classes go through the pin (cls_small: qb * d * 8 <= 256 KiB and qb <= 2048)."""
    return min(PIN_SLOTS, PIN_QUERY_BYTES // (d * 8))


@pytest.fixture(scope="module", params=[(300, 33), (300, 16), (130, 2100)], ids=["d33", "d16", "d2100"])
def delivery_set(request, fir):
    n, d = request.param
    nq = max(2049, pinned_queries(d) + 1) if d < 2100 else pinned_queries(d) + 1
    tr, tcls, q = clustered(n, d, 5, d, nq)
    avg = tr.mean(0)
    with fir.ClsModel(tr, tcls, 5, avg, 0) as m:
        singles = [ask(m, q[i:i + 1]) for i in range(nq)]
        one_by_one = tuple(np.concatenate([s[j] for s in singles]) for j in range(6))
        yield d, tr, tcls, avg, q, m, one_by_one


def test_batches_are_delivered_like_single_queries(delivery_set, oracle):
    """1 query (the ticket), 2 (the pinned slots), the last batch in the pin and the first beyond it -- 992 / 993 at d = 33 (the
    query bytes run out), 2048 / 2049 at d = 16 (the result slots do: classes and chunk counts fill both halves), 15 / 16 at
    d = 2100 --, and 2048 / 2049 staged at d = 33. Every result equals the same queries asked one at a time."""
    d, tr, tcls, avg, q, m, one = delivery_set
    edge = pinned_queries(d)
    assert edge == {33: 992, 16: 2048, 2100: 15}[d]
    for nq in sorted({1, 2, edge, edge + 1, q.shape[0] - 1, q.shape[0]}):
        got = ask(m, q[:nq])
        for j, what in enumerate(("pnn class", "pnn scores", "knn-1", "knn-3", "seq class", "seq chunks")):
            assert same_bits(got[j], one[j][:nq]), (d, nq, what)
    for i in (0, 1, 7, q.shape[0] - 2, q.shape[0] - 1):
        ec, es = oracle.pnn_predict(tr, tcls, avg, 5, q[i])
        assert one[0][i] == ec
        np.testing.assert_allclose(one[1][i], es, rtol=1e-12, atol=1e-300)
        assert one[2][i] == oracle.knn_predict(tr, tcls, avg, 5, q[i], 1)[0]
        assert one[3][i] == oracle.knn_predict(tr, tcls, avg, 5, q[i], 3)[0]
        assert (one[4][i], one[5][i]) == oracle.pnn_predict_seq(tr, tcls, avg, 5, q[i])


def test_one_query_without_scores(delivery_set, fir):
    """fir_cls_pnn_predict(scores = NULL) for one query is the call that takes the ticket path: the class of the call with scores."""
    d, tr, tcls, avg, q, m, one = delivery_set
    best = np.full(1, -7, np.int32)
    vp = ctypes.c_void_p
    for i in (0, 1, 2):
        qi = np.ascontiguousarray(q[i:i + 1])
        rc = fir.lib().fir_cls_pnn_predict(m._h, qi.ctypes.data_as(vp), 1, 0.0, None, best.ctypes.data_as(vp))
        assert rc == 0 and best[0] == one[0][i], (rc, i)


# ---- the sequential PNN's other kernels ----

@pytest.mark.parametrize("case", ["rows", "classes"])
def test_sequential_pnn_beyond_the_parallel_table(fir, oracle, case):
    """More than 65 536 rows: k_cls_pnn_seq instead of the per-(class, chunk) table. 400 classes x 20 chunks x 8 bytes > 48 KiB: the
    walk's table stays out of LDS. (class, chunks) = the oracle's, one and five queries per call."""
    if case == "rows":
        n, d, ncls = 65536 + 67, 33, 3
        tr, tcls, q = clustered(n, d, ncls, 7, 5)
    else:
        n, d, ncls = 800, 640, 400
        tr, tcls, q = clustered(n, d, ncls, 8, 5, tcls=np.repeat(np.arange(400, dtype=np.int32), 2))
        assert (d + 31) // 32 * ncls * 8 > 48 * 1024
    avg = tr.mean(0)
    want = [oracle.pnn_predict_seq(tr, tcls, avg, ncls, qi) for qi in q]
    with fir.ClsModel(tr, tcls, ncls, avg, 0) as m:
        best5, chunks5 = m.pnn_predict_seq(q)
        singles = [m.pnn_predict_seq(q[i:i + 1]) for i in range(5)]
    assert [(int(b), int(c)) for b, c in zip(best5, chunks5)] == want
    assert [(int(b[0]), int(c[0])) for b, c in singles] == want


# ---- one handle's scratch under every entry point ----

SEQUENCE = (
    lambda m, q: m.knn_class_nearest(q[:50], 8),
    lambda m, q: m.pnn_predict(q[:3]),
    lambda m, q: m.pnn_predict_seq(q[:40]),
    lambda m, q: m.knn_predict(q[:200], 3),
    lambda m, q: m.distance_sums(q[:5]),
    lambda m, q: m.pnn_predict(q[:300]),
    lambda m, q: m.kmedoids(2),
    lambda m, q: m.knn_predict(q[:1], 1),
)


def test_scratch_is_reused_across_entry_points(fir):
    """`scores` serves three layouts and `sums` two: the calls in a row on one handle, exact and then with both matrix-core forms on
    from 16 queries, each give the bits of the same call on a fresh handle."""
    tr, tcls, q = clustered(3000, 96, 11, 96, 300)
    avg = tr.mean(0)

    def settle(m, routed):
        m.set_pnn_mfma(16 if routed else 0)
        m.set_knn_mfma(16 if routed else 0)

    with fir.ClsModel(tr, tcls, 11, avg, 0) as m:
        for routed in (False, True):
            settle(m, routed)
            for step, call in enumerate(SEQUENCE):
                got = call(m, q)
                with fir.ClsModel(tr, tcls, 11, avg, 0) as fresh:
                    settle(fresh, routed)
                    want = call(fresh, q)
                assert same_bits(got, want), (routed, step)
        assert m.pnn_stats()["matrix_core_queries"] == 300 and m.knn_stats()["matrix_core_queries"] == 200


# ---- what a profiled call of the two matrix-core forms leaves behind ----

def test_profile_record_of_the_matrix_core_forms(fir):
    """A routed PNN batch and a routed kNN-3 batch of 32 queries over a d = 512 set just over the 256 MiB, each query next to three
    rows of one class. One query of each batch is answered by the exact scan after all (PNN: its scores all underflow; kNN-3: its
    two nearest rows are equal, and equal distances are not the matrix-core form's to order). The PNN form leaves three event pairs
    and its own pass as the dispatch -- the scan of the query it hands on is not bracketed; the kNN form leaves its pass's pair plus
    one per scan launch of the queries handed on (one query: one launch), and restores the pass as the dispatch."""
    nt, d, qb = hbm_rows(512), 512, 32
    rng = np.random.default_rng(5)
    tr = rng.random((nt, d))                          # (uniform rows: a query next to one row has no second row anywhere near)
    tcls = np.sort(rng.integers(0, 7, nt)).astype(np.int32)
    near = np.arange(qb) * 1000 + 7                   # rows r, r + 1, r + 2 of one class close together: kNN-3 settles inside them
    assert np.array_equal(tcls[near], tcls[near + 2])
    tr[near + 1] = tr[near] + 1e-3 * rng.standard_normal((qb, d))
    tr[near + 2] = tr[near] + 2e-3 * rng.standard_normal((qb, d))
    tr[near[0] + 1] = tr[near[0]]                     # ... but for the first query: its two nearest rows are equal
    avg = tr.mean(0)
    q = tr[near] + 1e-4 * rng.standard_normal((qb, d))
    qp = q.copy()
    qp[1] *= 4.0
    with fir.ClsModel(tr, tcls, 7, avg, 0) as m:
        m.set_pnn_mfma(16)
        m.set_knn_mfma(16)
        m.profile_enable(True)
        pnn_cls, _ = m.pnn_predict(qp)
        pnn_disp, pnn_pairs, pnn_st = m.last_dispatch(), len(m.profile_read()[0]), m.pnn_stats()
        knn_cls = m.knn_predict(q, 3)
        knn_disp, knn_pairs, knn_st = m.last_dispatch(), len(m.profile_read()[0]), m.knn_stats()
        m.profile_enable(False)
        m.set_pnn_mfma(0)
        m.set_knn_mfma(0)
        assert same_bits(pnn_cls, m.pnn_predict(qp)[0]) and same_bits(knn_cls, m.knn_predict(q, 3))
    assert pnn_st == {"matrix_core_queries": qb, "exact_scan_queries_of_them": 1}
    assert knn_st == {"matrix_core_queries": qb, "exact_scan_queries_of_them": 1}
    # Recorded from this test on commit 95cdacc, the last one before the host side became stages (one MI355X). The PNN's bytes: one read
    # of the 1025 tiles and the row norms, 32 queries' operands in LDS, the sums written; its flops 2 nt d qb. The kNN's flops: 2 nt d 128.
    assert (nt, pnn_pairs, knn_pairs) == (65583, 3, 2)
    assert pnn_disp == {"kernel": "fir::k_cls_pnn_mfma<2>", "bytes_per_launch": 286142584.0, "flops_per_launch": 2149023744.0}
    assert knn_disp == {"kernel": "fir::k_gemm_proxy_f16x<4, 0, 0>", "bytes_per_launch": 0.0, "flops_per_launch": 8596094976.0}
