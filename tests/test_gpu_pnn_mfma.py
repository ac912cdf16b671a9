"""PNN batches on the float64 matrix cores (fir_cls_set_pnn_mfma, csrc/fir_cls_pnn_mfma.h) against the scan of the same handle and
against the oracle: the scan's classes for every query, every class score within E(q) + 2^-40 relative (pnn_mfma_cases.score_bound),
queries inside the band answered by the scan bit for bit, and the bookkeeping of fir_cls_pnn_stats / fir_cls_last_dispatch."""
import ctypes

import numpy as np
import pytest

import golden_cases as gc
import pnn_mfma_cases as pc

pytestmark = pytest.mark.gpu

FIR_ERR_ARG = -1          # include/fir_amd.h


def takes_the_form(d):
    """include/fir_amd.h at fir_cls_pnn_predict: 16 queries of up to 1280 features fit the LDS; longer rows stay with the scan."""
    return d <= 1280


def routed_against_scan(fir, oracle, tr, tcls, avg, ncls, q):
    """scan and routed answers of one handle for q, checked as the header promises; returns the rise of the two counters."""
    d = tr.shape[1]
    with fir.ClsModel(tr, tcls, ncls, avg, 0) as m:
        scan_cls, scan_sc = m.pnn_predict(q)
        assert m.pnn_stats() == {"matrix_core_queries": 0, "exact_scan_queries_of_them": 0}      # a fresh handle routes nothing
        m.set_pnn_mfma(1)
        m.profile_enable(True)
        s0 = m.pnn_stats()
        mm_cls, mm_sc = m.pnn_predict(q)
        s1 = m.pnn_stats()
        disp = m.last_dispatch()
        m.profile_read()
    rose = {k: s1[k] - s0[k] for k in s0}
    print(f"d={d} nt={tr.shape[0]} qb={q.shape[0]} rose={rose} kernel={disp['kernel']} "
          f"max rel diff to scan={np.max(np.abs(mm_sc - scan_sc) / np.maximum(np.abs(scan_sc), 1e-300)):.3e}")
    assert np.array_equal(mm_cls, scan_cls)
    bound = pc.score_bound(tr, avg, q)
    pc.assert_scores_within(mm_sc, scan_sc, bound, "routed against the scan")
    want = np.array([oracle.pnn_predict(tr, tcls, avg, ncls, qi)[1] for qi in q])
    pc.assert_scores_within(mm_sc, want, bound, "routed against the oracle")
    if takes_the_form(d):
        assert rose["matrix_core_queries"] == q.shape[0]
        assert f"k_cls_pnn_mfma<{2 if d <= 640 else 1}>" in disp["kernel"]          # 32 queries per read of the rows up to d = 640, 16 beyond
        assert disp["flops_per_launch"] == 2.0 * tr.shape[0] * d * q.shape[0] and disp["bytes_per_launch"] > 0
    else:
        assert rose == {"matrix_core_queries": 0, "exact_scan_queries_of_them": 0}
        assert "k_cls_pnn_mfma" not in disp["kernel"]
        assert np.array_equal(mm_sc.view(np.uint64), scan_sc.view(np.uint64))
    return rose


@pytest.mark.parametrize("nq", [23, 1, 17])
@pytest.mark.parametrize("seed,n,d,ncls,frac", pc.EDGE_SHAPES)
def test_edge_shapes(fir, oracle, seed, n, d, ncls, frac, nq):
    """d = 1, odd d, dp2 no multiple of 4, a partly empty last tile, class boundaries inside a 16-row block, qb no multiple of 16,
    d = 640 (32 queries fill the LDS exactly), d = 2100 (not taken: the scan answers and nothing is counted)."""
    tr, tcls, avg, q = pc.edge_case(oracle, seed, n, d, ncls, frac)
    routed_against_scan(fir, oracle, tr, tcls, avg, ncls, q[:nq])


@pytest.mark.parametrize("nq", [23, 1, 17])
@pytest.mark.parametrize("seed,n,d,ncls,frac", pc.LDS_BOUNDARY_SHAPES)
def test_sixteen_queries_per_read_and_the_first_shape_not_taken(fir, oracle, seed, n, d, ncls, frac, nq):
    """d = 641 and d = 1280 run k_cls_pnn_mfma<1> (asserted by name in routed_against_scan), d = 1281 keeps the scan, uncounted."""
    tr, tcls, avg, q = pc.edge_case(oracle, seed, n, d, ncls, frac)
    assert tr.shape[0] > 512 and q.shape[0] >= nq
    routed_against_scan(fir, oracle, tr, tcls, avg, ncls, q[:nq])


def test_fewer_than_sixteen_rows_and_an_empty_class(fir, oracle):
    """nt < 16 (one 16-row block, mostly padding) with class 2 of 4 empty, then the same classes over 150 rows."""
    x, lab, ncls = gc.cls_case(seed=5, n=200, d=3, n_classes=4)
    keep = lab != 2
    for rows in (13, 150):
        xs, ls = x[keep][:rows], lab[keep][:rows]
        order = np.argsort(ls, kind="stable")
        tr, tcls = xs[order], ls[order]
        routed_against_scan(fir, oracle, tr, tcls, tr.mean(0), ncls, x[~keep][:19])


@pytest.mark.parametrize("seed,n,d,ncls", pc.LARGER_SHAPES)
def test_larger_shapes_with_a_cap_on_the_fallback(fir, oracle, seed, n, d, ncls):
    """160 queries. The float64 emulation of the form (test_pnn_mfma_formulation.py) puts none of them inside the band, so more than
    10 answered by the scan would mean the fallback is hiding a broken kernel."""
    tr, tcls, avg, q = pc.larger_case(seed, n, d, ncls)
    assert q.shape[0] == 160
    rose = routed_against_scan(fir, oracle, tr, tcls, avg, ncls, q)
    assert rose["exact_scan_queries_of_them"] <= 10


def test_the_band_sends_ties_to_the_scan(fir, oracle):
    """Class 1 is a copy of class 0 but for 2^-45 in one feature of one row: their scores differ by less than the form's error, so
    the scan has to answer; four queries scaled by 4.0 underflow every score to 0 -- the scan's too. All 20: the scan's bits."""
    x, lab, ncls = gc.cls_case(seed=31, n=960, d=36, n_classes=6)
    is_train = np.random.default_rng(31).random(960) < 0.8
    c0 = x[is_train & (lab == 0)]
    twin = c0.copy()
    twin[0, 0] += 2.0 ** -45
    rest = [x[is_train & (lab == c)] for c in range(2, ncls)]
    tr = np.concatenate([c0, twin] + rest)
    tcls = np.concatenate([np.full(len(c0), 0), np.full(len(twin), 1)] + [np.full(len(r), c + 2) for c, r in enumerate(rest)]).astype(np.int32)
    _, _, avg, _ = oracle.train_stats(tr)
    # 16 test rows of class 0 with the twins on top (a row another class wins by a clear margin is settled, rightly): by the oracle
    q0 = np.array([qi for qi in x[~is_train & (lab == 0)] if set(np.argsort(oracle.pnn_predict(tr, tcls, avg, ncls, qi)[1])[-2:]) == {0, 1}][:16])
    assert len(q0) == 16, f"only {len(q0)} class-0 test rows have the twin classes on top: the split no longer gives 16"
    q = np.concatenate([q0, 4.0 * x[~is_train][:4]])
    assert q.shape[0] == 20
    with fir.ClsModel(tr, tcls, ncls, avg, 0) as m:
        scan_cls, scan_sc = m.pnn_predict(q)
        m.set_pnn_mfma(1)
        mm_cls, mm_sc = m.pnn_predict(q)
        st = m.pnn_stats()
    assert np.all(scan_sc[16:] == 0) and np.all(scan_sc[:16].max(1) > 0)
    assert st == {"matrix_core_queries": 20, "exact_scan_queries_of_them": 20}
    assert np.array_equal(mm_cls, scan_cls)
    assert np.array_equal(mm_sc.view(np.uint64), scan_sc.view(np.uint64))


def test_batching_and_the_setter(fir, oracle):
    """200 000 x 4: 700 queries are two internal batches (the distance table is capped at 1 GiB), both routed."""
    rng = np.random.default_rng(12)
    nt, d, ncls = 200_000, 4, 5
    x = rng.random((nt, d))
    lab = np.sort(rng.integers(0, ncls, nt)).astype(np.int32)
    x += lab[:, None] * 0.15
    q = rng.random((700, d)) + rng.integers(0, ncls, 700)[:, None] * 0.15
    avg = x.mean(0)
    L = fir.lib()
    assert L.fir_cls_set_pnn_mfma(None, 1) == FIR_ERR_ARG
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert L.fir_cls_pnn_stats(None, ctypes.byref(a), ctypes.byref(b)) == FIR_ERR_ARG
    with fir.ClsModel(x, lab, ncls, avg, 0) as m:
        scan_cls, scan_sc = m.pnn_predict(q)
        knn, seq, sums = m.knn_predict(q[:40], 3), m.pnn_predict_seq(q[:40]), m.distance_sums(q[:5])
        m.set_pnn_mfma(1)
        mm_cls, mm_sc = m.pnn_predict(q)
        assert m.pnn_stats()["matrix_core_queries"] == 700
        parts = [m.pnn_predict(q[:300]), m.pnn_predict(q[300:])]
        assert m.pnn_stats()["matrix_core_queries"] == 1400
        assert np.array_equal(mm_cls, scan_cls)
        assert np.array_equal(mm_cls, np.concatenate([p[0] for p in parts]))
        assert np.array_equal(mm_sc.view(np.uint64), np.concatenate([p[1] for p in parts]).view(np.uint64))
        # the other entry points keep the scan whatever is set
        assert np.array_equal(m.knn_predict(q[:40], 3), knn)
        assert all(np.array_equal(u, v) for u, v in zip(m.pnn_predict_seq(q[:40]), seq))
        assert np.array_equal(m.distance_sums(q[:5]).view(np.uint64), sums.view(np.uint64))
        before = m.pnn_stats()
        m.set_pnn_mfma(0)
        back_cls, back_sc = m.pnn_predict(q)
        assert m.pnn_stats() == before
        assert np.array_equal(back_cls, scan_cls) and np.array_equal(back_sc.view(np.uint64), scan_sc.view(np.uint64))
        assert np.array_equal(m.knn_predict(q[:40], 3), knn)
        assert all(np.array_equal(u, v) for u, v in zip(m.pnn_predict_seq(q[:40]), seq))
        assert np.array_equal(m.distance_sums(q[:5]).view(np.uint64), sums.view(np.uint64))
        m.set_pnn_mfma(64)
        m.pnn_predict(q[:63])
        assert m.pnn_stats() == before
        m.pnn_predict(q[:64])
        assert m.pnn_stats()["matrix_core_queries"] == before["matrix_core_queries"] + 64
        m.set_pnn_mfma(-1)                                   # the automatic choice: never, in this version
        m.pnn_predict(q[:64])
        assert m.pnn_stats()["matrix_core_queries"] == before["matrix_core_queries"] + 64


def test_a_routed_call_repeats_bit_for_bit(fir, oracle):
    tr, tcls, avg, q = pc.larger_case(*pc.LARGER_SHAPES[3])
    with fir.ClsModel(tr, tcls, 101, avg, 0) as m:
        m.set_pnn_mfma(1)
        first = m.pnn_predict(q)
        second = m.pnn_predict(q)
        m.set_pnn_mfma(0)                                    # frees the row norms: they are made again, the same bits
        m.set_pnn_mfma(1)
        third = m.pnn_predict(q)
    for other in (second, third):
        assert np.array_equal(first[0], other[0])
        assert np.array_equal(first[1].view(np.uint64), other[1].view(np.uint64))
