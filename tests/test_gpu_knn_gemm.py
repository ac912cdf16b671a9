"""fir_gemm_search_knn_keys_dev: the K nearest rows for K up to 256 through the matrix cores must be, bit for bit, the keys of the
store + select form (fir_search_knn_keys_dev) on the same handle, and for a few queries what the oracle's distance vector gives
(knn_gemm_ref.expected). On plain data nothing may hide behind the exact form: the state's fallback_queries counter is checked
wherever tests/test_knn_gemm_formulation.py has shown, without a GPU, that the bound from the row sample has to hold."""
import numpy as np
import pytest
import torch

import knn_gemm_ref as ref
import synth

pytestmark = pytest.mark.gpu

L2 = 0
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FIR_ERR_ARG = -1
DEV = torch.device("cuda", 0)
GUARD = 0x5A5A5A5A


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gemm_keys(m, tq, qb, k, stream=None):
    out = torch.full((qb * k + 4,), GUARD, dtype=torch.int64, device=DEV)
    m.search_knn_keys_dev(tq.data_ptr(), qb, k, out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert torch.all(out[qb * k:] == GUARD)                                   # nothing past the end
    return out[:qb * k].cpu().numpy().view(np.uint64).reshape(qb, k)


def scan_keys(g, tq, qb, k, end=0):
    out = torch.full((qb * k + 4,), GUARD, dtype=torch.int64, device=DEV)
    g.search_knn_keys_dev(tq.data_ptr(), qb, k, out.data_ptr(), 0, end)
    g.sync()
    assert torch.all(out[qb * k:] == GUARD)
    return out[:qb * k].cpu().numpy().view(np.uint64).reshape(qb, k)


def both(fir, g, q, k, end=0, pkg_gemm=None):
    """(keys of the store + select form, keys of the matrix-core form, the state's stats), over features [0, end)."""
    qb = q.shape[0]
    tq = torch.from_numpy(np.array(q, np.float32)).to(DEV)
    scan = scan_keys(g, tq, qb, k, end)
    with (pkg_gemm or fir).GemmSearch(g, 2, end) as m:
        gemm = gemm_keys(m, tq, qb, k)
        st = m.stats()
    return scan, gemm, st


def same(scan, gemm):
    assert np.array_equal(gemm, scan), np.nonzero((gemm != scan).any(axis=1))[0][:8]


def no_exact_form(st):
    assert st["fallback_queries"] == 0 and st["second_pass_queries"] == 0, st


@pytest.mark.parametrize("n,d,qb,k", ref.SHAPES)
def test_equals_store_and_select_and_the_oracle(fir, oracle, n, d, qb, k):
    rows, q = ref.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k)
        if n == 66000:
            assert "f16x<1," in g.last_dispatch()["kernel"] and g.last_dispatch()["path"] == "mfma", g.last_dispatch()
    same(scan, gemm)
    no_exact_form(st)
    # the oracle, for a few queries (its distance vector is one gallery pass on the host per query)
    for i in sorted({0, qb // 2, qb - 1}):
        assert np.array_equal(gemm[i], ref.expected(oracle.all_distances(rows, q[i], 0, d, L2), k)), i


def test_prefix_property_and_agreement_with_k_up_to_8(fir):
    n, d, qb = 3000, 64, 130
    rows, q = ref.case(n + d, n, d, qb)
    tq = torch.from_numpy(q.copy()).to(DEV)
    with fir.Gallery(rows, None, L2, 0) as g, fir.GemmSearch(g, 2) as m:
        k64 = gemm_keys(m, tq, qb, 64)
        k9 = gemm_keys(m, tq, qb, 9)
        assert m.stats()["fallback_queries"] == 0
        assert np.array_equal(k64[:, :9], k9)
        for k in (1, 5, 8):
            kk = gemm_keys(m, tq, qb, k)                                        # the top-1 / top-K forms as they are
            assert np.array_equal(kk, k64[:, :k]), k
            exp = torch.zeros(qb * k, dtype=torch.int64, device=DEV)
            if k == 1:
                m.search_top1_keys_dev(tq.data_ptr(), qb, exp.data_ptr())
            else:
                m.search_topk_keys_dev(tq.data_ptr(), qb, k, exp.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(kk, exp.cpu().numpy().view(np.uint64).reshape(qb, k))


def test_feature_prefix_state(fir, oracle):
    n, d, end, qb, k = 3000, 512, 64, 70, 33
    rows, q = ref.case(11, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k, end)
    same(scan, gemm)
    no_exact_form(st)
    for i in (0, qb - 1):
        assert np.array_equal(gemm[i], ref.expected(oracle.all_distances(rows, q[i], 0, end, L2), k))


@pytest.mark.parametrize("k", [50, 250])
def test_cuts_inside_runs_of_equal_distances(fir, k):
    """200 copies of one row: K = 50 cuts the run, K = 250 asks for more rows than there are. The lower rows come first."""
    n, d, qb = 200, 64, 9
    rows = np.tile(synth.make_gallery(5, 1, d, L2), (n, 1)).astype(np.float32)
    q, _ = synth.make_queries(5, synth.make_gallery(6, 100, d, L2), qb, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k)
    same(scan, gemm)
    no_exact_form(st)
    idx, dist = fir.keys_unpack(gemm)
    m = min(k, n)
    assert np.array_equal(idx[:, :m], np.tile(np.arange(m, dtype=np.int32), (qb, 1))) and np.all(idx[:, m:] == -1)
    assert np.all(bits(dist[:, :m]) == bits(dist[:, :1]))


def test_more_candidates_than_a_list_holds(fir):
    """6000 identical rows: every row is at the bound, every list overflows, the store + select form answers every query."""
    n, d, qb, k = 6000, 64, 66, 16
    rows = np.tile(synth.make_gallery(5, 1, d, L2), (n, 1)).astype(np.float32)
    q, _ = synth.make_queries(5, synth.make_gallery(6, 100, d, L2), qb, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k)
    same(scan, gemm)
    assert np.array_equal(fir.keys_unpack(gemm)[0], np.tile(np.arange(k, dtype=np.int32), (qb, 1)))
    assert st["fallback_queries"] == qb, st


def test_hostile_values(fir):
    n, d, k = 3000, 64, 33
    rows = synth.make_gallery(23, n, d, L2).copy()
    q, _ = synth.make_queries(23, rows, 70, L2)
    q = q.copy()
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k)
        same(scan, gemm)
        no_exact_form(st)
        # hostile queries: NaN (every slot unused), scaled far out of fp16's range either way
        q[1, 7] = np.nan
        q[2] *= np.float32(1e19)
        q[3] *= np.float32(1e-20)
        scan, gemm, _ = both(fir, g, q, k)
        same(scan, gemm)
        assert np.all(gemm[1] == KEY_NONE)
    rows[100] = 1.0e4                                           # mean squared distance to a unit query ~1e8 >= 100000: never returned
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, _ = both(fir, g, q, k)
    same(scan, gemm)
    assert not np.isin(fir.keys_unpack(gemm[[0, 4, 5]])[0], [100]).any()
    rows[77] = np.nan                                           # a NaN row
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, _ = both(fir, g, q, k)
    same(scan, gemm)
    assert not np.isin(fir.keys_unpack(gemm)[0], [77, 100]).any()


@pytest.mark.parametrize("spread", [0.3, 0.005])
def test_clustered_class_major_identities(fir, spread):
    """150 identities x 40 images, class-major, K = 64: a leading sample would know nothing of the later identities; the spread runs do."""
    rows, q = ref.clustered(spread)
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, 64)
    same(scan, gemm)
    if spread == 0.3:
        no_exact_form(st)


def test_row_offset_shows_in_the_low_word(fir):
    n, d, qb, k = 3000, 64, 40, 33
    rows, q = ref.case(n + d, n, d, 130)
    q = q[:qb]
    tq = torch.from_numpy(q.copy()).to(DEV)
    with fir.Gallery(rows, None, L2, 0) as g:
        with fir.GemmSearch(g, 2) as m:
            base = gemm_keys(m, tq, qb, k)
        g.set_row_offset(1 << 20)
        scan, gemm, st = both(fir, g, q, k)
    same(scan, gemm)
    no_exact_form(st)
    assert np.array_equal(gemm, base + np.uint64(1 << 20))


def test_two_calls_give_the_same_bytes(fir):
    n, d, qb, k = 5000, 512, 70, 33
    rows, q = ref.case(n + d, n, d, qb)
    tq = torch.from_numpy(q.copy()).to(DEV)
    with fir.Gallery(rows, None, L2, 0) as g, fir.GemmSearch(g, 2) as m:
        a = gemm_keys(m, tq, qb, k)
        b = gemm_keys(m, tq, qb, 256)
        c = gemm_keys(m, tq, qb, k)
    assert np.array_equal(a, c) and np.array_equal(b[:, :k], a)


def test_host_form_routing(fir):
    n, d, qb, k = 3000, 64, 130, 33
    rows, q = ref.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        def knn(queries):
            g.search_top1(queries[:3])                                        # leaves a scan record: an unrouted knn call does not touch it
            assert g.last_dispatch()["path"] == "scan"
            return g.search_knn(queries, k), g.last_dispatch()

        plain, ld = knn(q)                                                    # no threshold: n < 65536 stays with store + select
        assert ld["path"] == "scan", ld
        g.set_large_batch_mfma(64)
        routed, ld = knn(q)
        assert ld["path"] == "mfma" and "k_gemm_proxy_f16x<1," in ld["kernel"], ld
        assert g.mfma_stats()["fallback_queries"] == 0
        few, ld = knn(q[:63])                                                 # below the caller's threshold
        assert ld["path"] == "scan", ld
        g.set_large_batch_mfma(0)
        off, ld = knn(q)
        assert ld["path"] == "scan", ld
    for other in (routed, off):
        assert np.array_equal(plain[0], other[0]) and np.array_equal(bits(plain[1]), bits(other[1]))
    assert np.array_equal(plain[0][:63], few[0]) and np.array_equal(bits(plain[1][:63]), bits(few[1]))


def test_large_batches_over_large_galleries_are_routed_by_default(fir):
    """The automatic rule (profiles/knn_matrix_cores.txt): 8 < K <= 256 from 128 queries over 65 536 rows on; K <= 8, fewer queries and
    K > 256 keep store + select. The same keys either way."""
    n, d, qb, k = 66000, 128, 200, 64
    rows, q = ref.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        def knn(queries, kk):
            g.search_top1(queries[:1])                                        # one query: the scan; its record stays unless the call is routed
            assert g.last_dispatch()["path"] == "scan"
            return g.search_knn(queries, kk), g.last_dispatch()["path"]

        routed, path = knn(q, k)
        assert path == "mfma" and g.mfma_stats()["fallback_queries"] == 0
        for queries, kk in ((q[:127], k), (q, 8), (q, 257)):
            got, path = knn(queries, kk)
            assert path == "scan", (queries.shape[0], kk)
            m = min(k, kk)
            assert np.array_equal(got[0][:, :m], routed[0][:queries.shape[0], :m]) and np.array_equal(bits(got[1][:, :m]), bits(routed[1][:queries.shape[0], :m]))
        g.set_large_batch_mfma(0)
        plain, path = knn(q, k)
        assert path == "scan"
    assert np.array_equal(plain[0], routed[0]) and np.array_equal(bits(plain[1]), bits(routed[1]))


def test_long_rows_direct_and_routed_by_default(fir):
    """2 048 features: the re-rank stages nine rows of 8 KiB in LDS (more than 64 KiB: the kernel has to opt in) and the pass streams its
    query slabs. The direct call, and fir_search_knn routing 128 queries over 65 536 rows by itself: the keys of store + select.
    (No list is near its capacity on this data: in float64, 170-370 of the 65 536 rows lie below D_s d - |q|^2 + 2.5 E d.)"""
    n, d, qb, k = 65536, 2048, 128, 9
    rng = np.random.default_rng(29)

    def unit(x):
        x /= np.sqrt((x * x).sum(axis=1, dtype=np.float32))[:, None]
        return x

    rows = unit(rng.random((n, d), dtype=np.float32))
    q = unit(rng.random((qb, d), dtype=np.float32))
    q[1::2] = unit(rows[rng.integers(0, n, qb // 2)] * (1 + np.float32(0.05) * (rng.random((qb // 2, d), dtype=np.float32) - np.float32(0.5))))
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k)
        same(scan, gemm)
        no_exact_form(st)
        g.search_top1(q[:1])
        assert g.last_dispatch()["path"] == "scan"
        idx, dist = g.search_knn(q, k)
        assert g.last_dispatch()["path"] == "mfma" and g.mfma_stats()["fallback_queries"] == 0, g.last_dispatch()
    si, sd = fir.keys_unpack(scan)
    assert np.array_equal(idx, si) and np.array_equal(bits(dist), bits(sd))


def device_sample_bound(fir, g, q, k, end=0, div=ref.SAMPLE_DIV):
    """D_s as the library's internal fir_knn_sample_bound_dev_ writes it (not part of the public ABI): float32 [qb]"""
    import ctypes as C

    fn = fir.lib().fir_knn_sample_bound_dev_
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    tq = torch.from_numpy(np.array(q, np.float32)).to(DEV)
    out = torch.full((q.shape[0] + 4,), -7.0, dtype=torch.float32, device=DEV)
    assert fn(g._h, tq.data_ptr(), q.shape[0], end, k, div, out.data_ptr(), None) == 0
    g.sync()
    assert torch.all(out[q.shape[0]:] == -7.0)
    return out[:q.shape[0]].cpu().numpy()


def expected_sample_bound(oracle, rows, q, k, d):
    """the K-th smallest oracle distance over the restatement's sample rows (knn_gemm_ref.sample_rows), 100000 with fewer than K below it"""
    s = np.ascontiguousarray(rows[ref.sample_rows(rows.shape[0], k)])
    out = np.full(q.shape[0], ref.NOT_FOUND, np.float32)
    for i in range(q.shape[0]):
        dist = oracle.all_distances(s, q[i], 0, d, L2)
        dist = np.sort(dist[dist < ref.NOT_FOUND])
        if dist.shape[0] >= k:
            out[i] = dist[k - 1]
    return out


@pytest.mark.parametrize("n,d,qb,k", [
    (66000, 128, 24, 64),        # 16 runs of 32 tiles spread over 1 032: a leading or otherwise placed sample gives other bits; three query tiles
    (3000, 64, 600, 9),          # more queries than one launch's 64 tiles: two groups
    (333, 100, 10, 256),         # the sample is the gallery, its last tile part full
    (200, 64, 9, 250),           # fewer rows than K: no bound
])
def test_the_sample_bound_is_the_kth_distance_over_the_spread_runs(fir, oracle, n, d, qb, k):
    rows, q = ref.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        got = device_sample_bound(fir, g, q, k)
    want = expected_sample_bound(oracle, rows, q, k, d)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:8]
    if n == 66000:          # ... and the spread is what it is about: the leading 32 768 rows give another bound
        lead = np.sort(oracle.all_distances(np.ascontiguousarray(rows[:32768]), q[0], 0, d, L2))[k - 1]
        assert lead != want[0]
    if k > n:
        assert np.all(got == ref.NOT_FOUND)


def test_more_queries_than_one_launch_group(fir):
    """600 queries: the sample bound runs in two groups (64 tiles of 8 per launch), the re-rank over 600 lists."""
    n, d, qb, k = 3000, 64, 600, 33
    rows, q = ref.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, k)
    same(scan, gemm)
    no_exact_form(st)


def test_on_a_callers_stream_after_a_call_on_another(fir):
    n, d, qb, k = 3000, 64, 130, 33
    rows, q = ref.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        hi, hd = g.search_knn(q, k)
        dq = torch.from_numpy(q.copy()).to(DEV)
        s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        k1 = torch.zeros(qb, dtype=torch.int64, device=DEV)
        keys = torch.full((qb * k + 8,), GUARD, dtype=torch.int64, device=DEV)
        with fir.GemmSearch(g, 2) as m:
            torch.cuda.synchronize()
            m.search_top1_keys_dev(dq.data_ptr(), qb, k1.data_ptr(), stream=s1.cuda_stream)          # no host synchronisation in between
            m.search_knn_keys_dev(dq.data_ptr(), qb, k, keys.data_ptr(), stream=s2.cuda_stream)
            s2.synchronize()
            s1.synchronize()
    assert torch.all(keys[qb * k:] == GUARD)
    di, dd = fir.keys_unpack(keys[:qb * k].cpu().numpy().view(np.uint64).reshape(qb, k))
    assert np.array_equal(di, hi) and np.array_equal(bits(dd), bits(hd))
    assert np.array_equal(fir.keys_unpack(k1.cpu().numpy().view(np.uint64))[0], hi[:, 0])


def test_errors_and_empty_inputs(fir):
    d = 64
    rows = synth.make_gallery(1, 300, d, L2)
    tq = torch.from_numpy(rows[:4].copy()).to(DEV)
    keys = torch.zeros(4 * 257, dtype=torch.int64, device=DEV)

    def fails(m, *a):
        with pytest.raises(fir.FirError) as e:
            m.search_knn_keys_dev(*a)
        assert e.value.code == FIR_ERR_ARG
        return str(e.value)

    with fir.Gallery(rows, None, L2, 0) as g:
        with fir.GemmSearch(g, 2) as m:
            assert "k=0 outside [1,256]" in fails(m, tq.data_ptr(), 4, 0, keys.data_ptr())
            assert "k=257 outside [1,256]" in fails(m, tq.data_ptr(), 4, 257, keys.data_ptr())
            assert "NULL" in fails(m, tq.data_ptr(), 4, 9, None)
            assert "NULL" in fails(m, None, 4, 9, keys.data_ptr())
            assert "NULL" in fails(m, None, -1, 0, None)                                     # NULL before qb < 0 before k
            assert "qb < 0" in fails(m, tq.data_ptr(), -1, 0, keys.data_ptr())
            assert "k=0" in fails(m, None, 0, 0, keys.data_ptr())                            # k before "nothing to do"
            m.search_knn_keys_dev(None, 0, 9, keys.data_ptr())                               # qb = 0
            m.search_knn_keys_dev(None, 0, 5, keys.data_ptr())
        with fir.GemmSearch(g, fir.GemmSearch.BF16_SPLIT) as m:
            assert "FIR_GEMM_F16" in fails(m, tq.data_ptr(), 4, 9, keys.data_ptr())
    with fir.Gallery(np.zeros((0, d), np.float32), None, L2, 0) as g, fir.GemmSearch(g, 2) as m:
        for k in (5, 9, 256):
            keys.fill_(0)
            m.search_knn_keys_dev(tq.data_ptr(), 4, k, keys.data_ptr())                     # empty gallery: unused slots
            torch.cuda.synchronize()
            assert torch.all(keys[:4 * k] == -1) and torch.all(keys[4 * k:] == 0)


def test_the_certificate_bound_is_needed_and_a_shrunken_one_is_caught(fir, fir_audit, monkeypatch):
    """The coherent-rounding near-tie of test_gpu_gemm.py with nine copies of its row B, K = 9: the query is row A (distance exactly
    0), the nine B rows lie 2e-9 / d away, but their fp16 proxies are LOWER than A's by 0.77 of the rounding window -- the nine
    smallest proxies are the B rows', A is the tenth, and the true answer is A and the eight B rows of lowest index. With the bound
    as derived A is appended and re-ranked and the keys are the scan's; the audit library with the certificate's E shrunk to a
    quarter leaves A out and certifies the nine B rows."""
    from test_gpu_gemm import _coherent_rounding_fixture

    rows, q, ia, ib = _coherent_rounding_fixture()
    rows = rows.copy()
    rows[ib + 1:ib + 9] = rows[ib]
    k = 9
    got = {}
    for lib_name, pkg in (("audit", fir_audit), ("shipped", fir)):
        with pkg.Gallery(rows, None, L2, 0) as g:
            for scale in ("1", "0.25", None):
                if scale is None:
                    monkeypatch.delenv("FIR_GEMM_EREL_SCALE")
                else:
                    monkeypatch.setenv("FIR_GEMM_EREL_SCALE", scale)
                scan, gemm, st = both(pkg, g, q, k)
                got[lib_name, scale] = (gemm, st["fallback_queries"])
                idx, dist = pkg.keys_unpack(scan)
                assert idx[0].tolist() == [ia] + list(range(ib, ib + 8)) and dist[0, 0] == 0.0 and dist[0, 1] > 0.0
    for key in (("audit", "1"), ("audit", None), ("shipped", "1"), ("shipped", "0.25"), ("shipped", None)):
        gemm, fb = got[key]
        same(scan, gemm)
        assert fb <= 2, (key, fb)
    gemm, fb = got["audit", "0.25"]
    idx, dist = fir.keys_unpack(gemm)
    # row A missing, certified (no exact form for it): the shrunken bound is unsound and it shows
    assert idx[0].tolist() == list(range(ib, ib + 9)) and dist[0, 0] > 0.0 and fb <= 2, (idx[0], dist[0], fb)
    assert not np.array_equal(gemm, scan)
