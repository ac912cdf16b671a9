"""fir_gemm_search_radius_keys_dev: every row within a per-query radius through the matrix cores must give, bit for bit, the counts
and keys of the store + count + select form (fir_search_radius_keys_dev) on the same handle, and for a few queries what the
oracle's distance vector gives under radius_ref.expected. The radii come from fir_range_distances on the same handle, sorted on
the host. On plain data nothing may hide behind the exact form: the state's fallback_queries counter is checked wherever
tests/test_radius_formulation.py has shown, without a GPU, that the bound made of the radius has to hold."""
import numpy as np
import pytest
import torch

import knn_gemm_ref as kg
import knn_select_ref as ks
import radius_ref as ref
import synth
from test_radius_formulation import SHAPES

pytestmark = pytest.mark.gpu

L2 = 0
F32 = np.float32
INF = F32(np.inf)
FIR_ERR_ARG = -1
DEV = torch.device("cuda", 0)
GUARD = 0x5A5A5A5A5A5A5A5A
GUARD32 = 0x5A5A5A5A
K_LIST_CAP = 4096


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def call(fn, tq, tr, qb, m, *tail, **kw):
    """(count, keys) of one device-pointer radius call; guard words behind both outputs"""
    keys = torch.full((qb * m + 4,), GUARD, dtype=torch.int64, device=DEV)
    count = torch.full((qb + 4,), GUARD32, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    fn(tq.data_ptr(), qb, tr.data_ptr(), m, count.data_ptr(), keys.data_ptr() if m else None, *tail, **kw)
    torch.cuda.synchronize()
    assert torch.all(keys[qb * m:] == GUARD) and torch.all(count[qb:] == GUARD32)      # nothing past the end
    return count[:qb].cpu().numpy(), keys[:qb * m].cpu().numpy().view(np.uint64).reshape(qb, m)


def both(fir, g, q, radius, m, end=0, state=None):
    """(count, keys) of the store + count + select form, of the matrix-core form, and the state's stats, over features [0, end)."""
    qb = q.shape[0]
    tq = torch.from_numpy(np.array(q, np.float32)).to(DEV)
    tr = torch.from_numpy(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (qb,)).copy()).to(DEV)
    scan = call(g.search_radius_keys_dev, tq, tr, qb, m, 0, end)
    if state is not None:
        return scan, call(state.search_radius_keys_dev, tq, tr, qb, m), state.stats()
    with fir.GemmSearch(g, 2, end) as s:
        gemm = call(s.search_radius_keys_dev, tq, tr, qb, m)
        st = s.stats()
    return scan, gemm, st


def same(scan, gemm):
    assert np.array_equal(gemm[0], scan[0]), np.nonzero(gemm[0] != scan[0])[0][:8]
    assert np.array_equal(gemm[1], scan[1]), np.nonzero((gemm[1] != scan[1]).any(axis=1))[0][:8]


def no_exact_form(st):
    assert st["fallback_queries"] == 0 and st["second_pass_queries"] == 0, st


def at_rank(dist, r):
    """[qb] the exact bits of each query's r-th smallest qualifying distance"""
    return np.array([np.sort(row[ks.qualifies(row)])[r - 1] for row in dist], F32)


@pytest.mark.parametrize("n,d,end,qb,ranks", SHAPES)
def test_equals_store_count_select_and_the_oracle(fir, oracle, n, d, end, qb, ranks):
    rows, q = kg.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g, fir.GemmSearch(g, 2, end) as s:
        dist = g.range_distances(q, 0, end)
        fallbacks = 0
        for r in ranks:
            m = min(r, 256)
            radius = np.nextafter(at_rank(dist, r), INF)
            scan, gemm, st = both(fir, g, q, radius, m, end, state=s)
            same(scan, gemm)
            assert st["fallback_queries"] == fallbacks and st["second_pass_queries"] == 0, (r, st)
            assert np.all(gemm[0] >= r)
            # the oracle, for a few queries (its distance vector is one gallery pass on the host per query)
            for i in sorted({0, qb // 2, qb - 1}):
                want_c, want_k = ref.expected(oracle.all_distances(rows, q[i], 0, end or d, L2), radius[i], m)
                assert gemm[0][i] == want_c and np.array_equal(gemm[1][i], want_k), (r, i)
        if n == 66000:
            assert "f16x<1," in g.last_dispatch()["kernel"] and g.last_dispatch()["path"] == "mfma", g.last_dispatch()


@pytest.mark.parametrize("r", [1, 33, 256])
def test_the_smallest_margin_the_rth_row_is_out_at_its_own_distance_and_in_one_ulp_above(fir, r):
    n, d, qb = 3000, 64, 130
    rows, q = kg.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g, fir.GemmSearch(g, 2) as s:
        dist = g.range_distances(q)
        at = at_rank(dist, r)
        j = np.array([np.flatnonzero(dist[i].view(np.uint32) == at[i].view(np.uint32))[0] for i in range(qb)])
        for radius, inside in ((at, False), (np.nextafter(at, INF), True)):
            scan, gemm, st = both(fir, g, q, radius, 256, state=s)
            same(scan, gemm)
            no_exact_form(st)
            want_c, want_k = ref.expected_batch(dist, radius, 256)
            assert np.array_equal(gemm[0], want_c) and np.array_equal(gemm[1], want_k)
            listed = (ks.unpack(gemm[1])[0] == j[:, None]).any(axis=1)
            assert np.all(listed == inside), (r, inside)
            assert np.all(gemm[0] >= r) if inside else np.all(gemm[0] < r)


@pytest.mark.parametrize("n", [K_LIST_CAP, K_LIST_CAP + 1, 6000])
def test_identical_rows_at_the_list_capacity(fir, n):
    """Every row is one vector and the radius lies just above its distance: 4096 rows fill a list exactly and are certified, one row
    more overflows every list and the store + count + select form answers every query; 6000: the same, far past the seam."""
    d, qb, m = 64, 9, 16
    rows = np.tile(synth.make_gallery(5, 1, d, L2), (n, 1)).astype(np.float32)
    q, _ = synth.make_queries(5, synth.make_gallery(6, 100, d, L2), qb, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        assert np.all(bits(dist) == bits(dist[:, :1]))
        scan, gemm, st = both(fir, g, q, np.nextafter(dist[:, 0], INF), m)
        same(scan, gemm)
        assert np.all(gemm[0] == n)
        assert np.array_equal(ks.unpack(gemm[1])[0], np.tile(np.arange(m, dtype=np.int32), (qb, 1)))
        assert st["fallback_queries"] == (0 if n <= K_LIST_CAP else qb), st
        scan, gemm, st = both(fir, g, q, dist[:, 0].copy(), m)                 # the rows' own distance: nothing is inside
        same(scan, gemm)
        assert np.all(gemm[0] == 0) and np.all(gemm[1] == ref.KEY_NONE)


def test_an_infinite_radius_over_more_rows_than_a_list_holds_falls_back_and_equals_knn(fir):
    n, d, qb, m = 5000, 512, 70, 33
    rows, q = kg.case(n + d, n, d, qb)
    tq = torch.from_numpy(q.copy()).to(DEV)
    with fir.Gallery(rows, None, L2, 0) as g:
        knn = torch.zeros(qb * m, dtype=torch.int64, device=DEV)
        g.search_knn_keys_dev(tq.data_ptr(), qb, m, knn.data_ptr())
        g.sync()
        scan, gemm, st = both(fir, g, q, INF, m)
    same(scan, gemm)
    assert st["fallback_queries"] == qb, st
    assert np.all(gemm[0] == n) and np.array_equal(gemm[1], knn.cpu().numpy().view(np.uint64).reshape(qb, m))


def test_count_only_and_hostile_values(fir):
    n, d = 3000, 64
    rows = synth.make_gallery(23, n, d, L2).copy()
    q, _ = synth.make_queries(23, rows, 70, L2)
    q = q.copy()
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        radius = np.nextafter(at_rank(dist, 33), INF)
        for m in (0, 33):
            scan, gemm, st = both(fir, g, q, radius, m)
            same(scan, gemm)
            no_exact_form(st)
            assert np.all(gemm[0] >= 33) and gemm[1].shape == (70, m)
        # hostile radii: NaN, zero, negative, -inf qualify nothing; +inf and the cut-off take every row fir_search_knn considers
        radius[:8] = [np.nan, 0.0, -0.0, -1.0, -np.inf, np.inf, 100000.0, 3e38]
        scan, gemm, _ = both(fir, g, q, radius, 33)
        same(scan, gemm)
        assert np.all(gemm[0][:5] == 0) and np.all(gemm[0][5:8] == n)
        # hostile queries: NaN (nothing qualifies), scaled far out of fp16's range either way
        q[1, 7] = np.nan
        q[2] *= np.float32(1e19)
        q[3] *= np.float32(1e-20)
        radius = np.nextafter(at_rank(dist, 33), INF)
        radius[2] = INF
        scan, gemm, _ = both(fir, g, q, radius, 33)
        same(scan, gemm)
        assert gemm[0][1] == 0 and np.all(gemm[1][1] == ref.KEY_NONE)
    rows[100] = 1.0e4                                           # mean squared distance to a unit query ~1e8 >= 100000: never inside
    rows[77] = np.nan                                           # a NaN row
    with fir.Gallery(rows, None, L2, 0) as g:
        for rad in (radius, INF):
            scan, gemm, _ = both(fir, g, q, rad, 33)
            same(scan, gemm)
            assert not np.isin(ks.unpack(gemm[1])[0], [77, 100]).any() and np.all(gemm[0] <= n - 2)


def test_long_rows(fir):
    """2 048 features: the re-rank stages nine rows of 8 KiB in LDS (more than 64 KiB: the kernel has to opt in) and the pass streams
    its query slabs; the shape of test_gpu_knn_gemm.py::test_long_rows_direct_and_routed_by_default, radius at rank 9."""
    n, d, qb, r = 65536, 2048, 128, 9
    rng = np.random.default_rng(29)

    def unit(x):
        x /= np.sqrt((x * x).sum(axis=1, dtype=np.float32))[:, None]
        return x

    rows = unit(rng.random((n, d), dtype=np.float32))
    q = unit(rng.random((qb, d), dtype=np.float32))
    q[1::2] = unit(rows[rng.integers(0, n, qb // 2)] * (1 + np.float32(0.05) * (rng.random((qb // 2, d), dtype=np.float32) - np.float32(0.5))))
    with fir.Gallery(rows, None, L2, 0) as g:
        radius = np.nextafter(at_rank(g.range_distances(q), r), INF)
        scan, gemm, st = both(fir, g, q, radius, r)
    same(scan, gemm)
    no_exact_form(st)
    assert np.all(gemm[0] >= r)


def test_more_queries_than_one_super_batch(fir):
    """8 192 + 70 queries: two sets of launches, the second one's radii, counts and keys at their offsets."""
    n, d, qb0, r = 3000, 64, 130, 9
    rows, q = kg.case(n + d, n, d, qb0)
    reps = (8192 + 70 + qb0 - 1) // qb0
    with fir.Gallery(rows, None, L2, 0) as g:
        radius = np.nextafter(at_rank(g.range_distances(q), r), INF)
        scan, gemm, st = both(fir, g, q, radius, r)
        same(scan, gemm)
        big_q, big_r = np.tile(q, (reps, 1))[:8192 + 70], np.tile(radius, reps)[:8192 + 70]
        qb = big_q.shape[0]
        tq, tr = torch.from_numpy(big_q).to(DEV), torch.from_numpy(big_r).to(DEV)
        with fir.GemmSearch(g, 2) as s:
            count, keys = call(s.search_radius_keys_dev, tq, tr, qb, r)
            no_exact_form(s.stats())
    assert np.array_equal(count, np.tile(scan[0], reps)[:qb]) and np.array_equal(keys, np.tile(scan[1], (reps, 1))[:qb])


def test_host_form_routing(fir):
    n, d, qb, r = 3000, 64, 130, 33
    rows, q = kg.case(n + d, n, d, qb)
    with fir.Gallery(rows, None, L2, 0) as g:
        radius = np.nextafter(at_rank(g.range_distances(q), r), INF)

        def search(queries, rad, m=r):
            g.search_top1(queries[:3])                                        # leaves a scan record: an unrouted radius call does not touch it
            assert g.last_dispatch()["path"] == "scan"
            return g.search_radius(queries, rad, m), g.last_dispatch()

        plain, ld = search(q, radius)                                         # no threshold: never routed by itself
        assert ld["path"] == "scan", ld
        g.set_large_batch_mfma(64)
        routed, ld = search(q, radius)
        assert ld["path"] == "mfma" and "k_gemm_proxy_f16x<1," in ld["kernel"], ld
        assert g.mfma_stats()["fallback_queries"] == 0
        counted, ld = search(q, radius, 0)
        assert ld["path"] == "mfma" and counted[1] is None and np.array_equal(counted[0], plain[0])
        few, ld = search(q[:63], radius[:63])                                 # below the caller's threshold
        assert ld["path"] == "scan", ld
        wide, ld = search(q, radius, 257)                                     # more than the matrix-core form returns
        assert ld["path"] == "scan", ld
        g.set_large_batch_mfma(0)
        off, ld = search(q, radius)
        assert ld["path"] == "scan", ld
    assert np.all(plain[0] >= r)
    for other in (routed, off):
        assert np.array_equal(plain[0], other[0]) and np.array_equal(plain[1], other[1]) and np.array_equal(bits(plain[2]), bits(other[2]))
    assert np.array_equal(plain[0][:63], few[0]) and np.array_equal(plain[1][:63], few[1]) and np.array_equal(bits(plain[2][:63]), bits(few[2]))
    assert np.array_equal(plain[0], wide[0]) and np.array_equal(plain[1], wide[1][:, :r])


def test_errors_and_empty_inputs(fir):
    d = 64
    rows = synth.make_gallery(1, 300, d, L2)
    tq = torch.from_numpy(rows[:4].copy()).to(DEV)
    tr = torch.ones(4, dtype=torch.float32, device=DEV)
    keys = torch.zeros(4 * 257, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)

    def fails(m, *a):
        with pytest.raises(fir.FirError) as e:
            m.search_radius_keys_dev(*a)
        assert e.value.code == FIR_ERR_ARG
        return str(e.value)

    with fir.Gallery(rows, None, L2, 0) as g:
        with fir.GemmSearch(g, 2) as m:
            assert "max_results=-1 outside [0,256]" in fails(m, tq.data_ptr(), 4, tr.data_ptr(), -1, cnt.data_ptr(), keys.data_ptr())
            assert "max_results=257 outside [0,256]" in fails(m, tq.data_ptr(), 4, tr.data_ptr(), 257, cnt.data_ptr(), keys.data_ptr())
            assert "NULL" in fails(m, tq.data_ptr(), 4, tr.data_ptr(), 9, cnt.data_ptr(), None)
            assert "NULL" in fails(m, tq.data_ptr(), 4, tr.data_ptr(), 0, cnt.data_ptr(), keys.data_ptr())      # count-only: no keys
            assert "NULL" in fails(m, tq.data_ptr(), 4, tr.data_ptr(), 9, None, keys.data_ptr())
            assert "NULL" in fails(m, tq.data_ptr(), 4, None, 9, cnt.data_ptr(), keys.data_ptr())
            assert "NULL" in fails(m, None, 4, tr.data_ptr(), 9, cnt.data_ptr(), keys.data_ptr())
            assert "NULL" in fails(m, None, -1, None, 300, None, None)                                          # NULL before qb < 0 before max_results
            assert "qb < 0" in fails(m, tq.data_ptr(), -1, tr.data_ptr(), 300, cnt.data_ptr(), keys.data_ptr())
            assert "max_results=300" in fails(m, None, 0, None, 300, cnt.data_ptr(), keys.data_ptr())           # max_results before "nothing to do"
            m.search_radius_keys_dev(None, 0, None, 9, cnt.data_ptr(), keys.data_ptr())                         # qb = 0
            m.search_radius_keys_dev(None, 0, None, 0, cnt.data_ptr(), None)
        with fir.GemmSearch(g, fir.GemmSearch.BF16_SPLIT) as m:
            assert "FIR_GEMM_F16" in fails(m, tq.data_ptr(), 4, tr.data_ptr(), 9, cnt.data_ptr(), keys.data_ptr())
    with fir.Gallery(np.zeros((0, d), np.float32), None, L2, 0) as g, fir.GemmSearch(g, 2) as m:
        for k in (0, 9, 256):
            keys.fill_(0)
            cnt.fill_(7)
            m.search_radius_keys_dev(tq.data_ptr(), 4, tr.data_ptr(), k, cnt.data_ptr(), keys.data_ptr() if k else None)      # empty gallery
            torch.cuda.synchronize()
            assert torch.all(keys[:4 * k] == -1) and torch.all(keys[4 * k:] == 0) and torch.all(cnt == 0)
