"""fir_gemm_search_top_classes_keys_dev: the K nearest DISTINCT classes through the matrix cores must be, bit for bit, what the exact
class-minimum scan (fir_search_top_classes_keys_dev) gives on the same gallery, and what the oracle's distance vector gives after
the per-class reduction of test_gpu_class_rank.py. On plain data nothing may hide behind the exact form: the state's
fallback_queries counter is checked wherever the bound from the row sample has to hold."""
import functools

import numpy as np
import pytest
import torch

import synth
from test_gpu_class_rank import bits, check, expected

pytestmark = pytest.mark.gpu

L2 = 0
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FIR_ERR_ARG, FIR_ERR_STATE = -1, -5
DEV = torch.device("cuda", 0)


def both(fir, g, q, nc, k, end=0, pkg_gemm=None):
    """((keys, classes) of the scan form, (keys, classes) of the matrix-core form, the state's stats), over features [0, end)."""
    qb = q.shape[0]
    tq = torch.from_numpy(np.array(q, np.float32)).to(DEV)
    out = []
    for _ in range(2):
        out.append((torch.full((qb * k + 4,), 0x5A5A5A5A, dtype=torch.int64, device=DEV), torch.full((qb * k + 4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)))
    g.search_top_classes_keys_dev(tq.data_ptr(), qb, nc, k, out[0][0].data_ptr(), out[0][1].data_ptr(), 0, end)
    g.sync()
    with (pkg_gemm or fir).GemmSearch(g, 2, end) as m:
        m.search_top_classes_keys_dev(tq.data_ptr(), qb, nc, k, out[1][0].data_ptr(), out[1][1].data_ptr())
        torch.cuda.synchronize()
        st = m.stats()
    res = []
    for keys, cls in out:
        assert torch.all(keys[qb * k:] == 0x5A5A5A5A) and torch.all(cls[qb * k:] == 0x5A5A5A5A)          # nothing past the end
        res.append((keys[:qb * k].cpu().numpy().view(np.uint64).reshape(qb, k), cls[:qb * k].cpu().numpy().reshape(qb, k)))
    return res[0], res[1], st


def same(scan, gemm):
    assert np.array_equal(gemm[0], scan[0]), np.nonzero((gemm[0] != scan[0]).any(axis=1))[0][:8]
    assert np.array_equal(gemm[1], scan[1]), np.nonzero((gemm[1] != scan[1]).any(axis=1))[0][:8]


def class_major_even(n, nc):
    return (np.arange(n, dtype=np.int64) * nc // n).astype(np.int32)


LABELLINGS = {
    "interleaved": lambda n, nc: synth.make_labels(n, nc),
    "class_major": class_major_even,
    "one_per_row": lambda n, nc: np.arange(n, dtype=np.int32),
}


@functools.lru_cache(maxsize=None)
def case(seed, n, d, qb):
    rows = synth.make_gallery(seed, n, d, L2)
    q, _ = synth.make_queries(seed, rows, qb, L2)
    for a in (rows, q):
        a.setflags(write=False)
    return rows, q


@pytest.mark.parametrize("n,d,qb,nc,k,labelling", [
    (3000, 64, 130, 37, 5, "interleaved"),
    (5000, 512, 70, 500, 5, "class_major"),
    (333, 100, 130, 10, 8, "interleaved"),
    (2000, 520, 33, 2000, 32, "one_per_row"),
    (7, 64, 3, 3, 5, "interleaved"),                      # fewer classes than k: unused slots
    (66000, 128, 200, 1000, 5, "interleaved"),            # crosses 65 536 rows; the sample bound decides what is appended (n > list capacity)
])
def test_equals_the_scan_and_the_oracle(fir, oracle, n, d, qb, nc, k, labelling):
    rows, q = case(n + d, n, d, qb)
    labels = LABELLINGS[labelling](n, nc)
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, nc, k)
        assert "f16x<1," in g.last_dispatch()["kernel"] and g.last_dispatch()["path"] == "mfma", g.last_dispatch()
    same(scan, gemm)
    assert st["fallback_queries"] == 0 and st["second_pass_queries"] == 0, st
    if n == 7:
        assert np.all(gemm[0][:, 3:] == KEY_NONE) and np.all(gemm[1][:, 3:] == -1) and np.all(gemm[1][:, :3] >= 0)
    # the oracle, for a few queries (its distance vector is one gallery pass on the host per query)
    pick = sorted({0, qb // 2, qb - 1})
    dist = np.stack([oracle.all_distances(rows, q[i], 0, d, L2) for i in pick])
    idx, dd = fir.keys_unpack(gemm[0][pick])
    check((gemm[1][pick], idx, dd), expected(dist, labels, nc, k))


def test_feature_prefix_state(fir, oracle):
    n, d, end, qb, nc, k = 3000, 512, 64, 70, 37, 5
    rows, q = case(11, n, d, qb)
    labels = synth.make_labels(n, nc)
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, nc, k, end)
    same(scan, gemm)
    assert st["fallback_queries"] == 0, st
    dist = np.stack([oracle.all_distances(rows, q[i], 0, end, L2) for i in (0, qb - 1)])
    idx, dd = fir.keys_unpack(gemm[0][[0, qb - 1]])
    check((gemm[1][[0, qb - 1]], idx, dd), expected(dist, labels, nc, k))


@pytest.mark.parametrize("spread", [0.3, 0.005])
def test_clustered_identities(fir, spread):
    """150 identities x 40 images, class-major: the five nearest ROWS of a query are one identity, the answer is five identities."""
    rng = np.random.default_rng(17)
    ids, per, d, qb, k = 150, 40, 256, 130, 5
    centres = rng.random((ids, d), dtype=np.float32)
    rows = synth.normalise(np.repeat(centres, per, axis=0) * (1 + spread * (rng.random((ids * per, d), dtype=np.float32) - 0.5)), 0)
    who = rng.integers(0, ids, qb)
    q = synth.normalise(centres[who] * (1 + spread * (rng.random((qb, d), dtype=np.float32) - 0.5)), 0)
    labels = np.repeat(np.arange(ids, dtype=np.int32), per)
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, ids, k)
        ti, _ = g.search_topk(q, k)
    same(scan, gemm)
    assert np.all(ti // per == who[:, None])                                   # the nearest five rows: one class
    assert np.array_equal(gemm[1][:, 0], who.astype(np.int32))
    assert all(len(set(r)) == k and min(r) >= 0 for r in gemm[1].tolist())     # five distinct classes
    if spread == 0.3:
        assert st["fallback_queries"] == 0, st


def test_ties_across_and_within_classes(fir):
    n, d = 200, 32
    rows = synth.make_gallery(41, n, d, L2).copy()
    labels = synth.make_labels(n, 10).copy()
    rows[150] = rows[20]                       # the same row in two classes (4 and 7)
    labels[20], labels[150] = 4, 7
    rows[133] = rows[61]                       # a duplicate inside one class
    labels[61], labels[133] = 2, 2
    q = np.stack([rows[20], rows[61], rows[150]]).astype(np.float32)
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, _ = both(fir, g, q, 10, 3)
    same(scan, gemm)
    idx, _ = fir.keys_unpack(gemm[0])
    cls = gemm[1]
    assert (cls[0, 0], idx[0, 0], cls[0, 1], idx[0, 1]) == (4, 20, 7, 150)
    assert (cls[1, 0], idx[1, 0]) == (2, 61) and 133 not in idx[1]


def test_more_candidates_than_a_list_holds(fir):
    """6000 identical rows in 10 classes: every row is at the bound, every list overflows, the exact form answers every query."""
    n, d, qb, nc, k = 6000, 64, 66, 10, 5
    rows = np.tile(synth.make_gallery(5, 1, d, L2), (n, 1)).astype(np.float32)
    labels = synth.make_labels(n, nc)
    q, _ = synth.make_queries(5, synth.make_gallery(6, 100, d, L2), qb, L2)
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, nc, k)
    same(scan, gemm)
    assert np.array_equal(gemm[1], np.tile(np.arange(k, dtype=np.int32), (qb, 1)))       # ties: the lower row's class first
    assert st["fallback_queries"] == qb, st


def test_hostile_values(fir):
    n, d, nc, k = 3000, 64, 37, 5
    rows = synth.make_gallery(23, n, d, L2).copy()
    labels = synth.make_labels(n, nc).copy()
    q, _ = synth.make_queries(23, rows, 70, L2)
    q = q.copy()
    labels[[3, 64, 200]] = -1                                   # labels outside [0, num_classes)
    labels[[5, 127]] = nc + 3
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, st = both(fir, g, q, nc, k)
        same(scan, gemm)
        assert st["fallback_queries"] == 0, st
        idx, _ = fir.keys_unpack(gemm[0])
        assert not np.isin(idx, [3, 64, 200, 5, 127]).any()
        # hostile queries: NaN (every slot unused), scaled far out of fp16's range either way
        q[1, 7] = np.nan
        q[2] *= np.float32(1e19)
        q[3] *= np.float32(1e-20)
        scan, gemm, _ = both(fir, g, q, nc, k)
        same(scan, gemm)
        assert np.all(gemm[0][1] == KEY_NONE) and np.all(gemm[1][1] == -1)
    rows[100] = 1.0e4                                           # mean squared distance to a unit query ~1e8 >= 100000
    labels[100] = nc                                            # alone in its class: the class must come back absent
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, _ = both(fir, g, q, nc + 1, k)
        same(scan, gemm)
        assert not np.isin(gemm[1], [nc]).any()
    rows[77] = np.nan                                           # a NaN row
    with fir.Gallery(rows, labels, L2, 0) as g:
        scan, gemm, _ = both(fir, g, q, nc + 1, k)
    same(scan, gemm)
    assert not np.isin(fir.keys_unpack(gemm[0])[0], [77, 100]).any()


def test_errors_and_empty_inputs(fir):
    d = 64
    rows = synth.make_gallery(1, 300, d, L2)
    tq = torch.from_numpy(rows[:4].copy()).to(DEV)
    keys = torch.zeros(4 * 33, dtype=torch.int64, device=DEV)
    cls = torch.zeros(4 * 33, dtype=torch.int32, device=DEV)

    def code(m, *a):
        with pytest.raises(fir.FirError) as e:
            m.search_top_classes_keys_dev(*a)
        return e.value.code

    with fir.Gallery(rows, None, L2, 0) as g, fir.GemmSearch(g, 2) as m:
        assert code(m, tq.data_ptr(), 4, 10, 3, keys.data_ptr(), cls.data_ptr()) == FIR_ERR_STATE          # no labels
    with fir.Gallery(rows, synth.make_labels(300, 10), L2, 0) as g:
        with fir.GemmSearch(g, 2) as m:
            for nc, k in ((10, 0), (10, 33), (0, 3), ((1 << 24) + 1, 3)):
                assert code(m, tq.data_ptr(), 4, nc, k, keys.data_ptr(), cls.data_ptr()) == FIR_ERR_ARG
            assert code(m, tq.data_ptr(), 4, 10, 3, None, None) == FIR_ERR_ARG
            m.search_top_classes_keys_dev(None, 0, 10, 3, None, None)                                       # qb = 0
            # one output NULL
            m.search_top_classes_keys_dev(tq.data_ptr(), 4, 10, 3, keys.data_ptr(), None)
            m.search_top_classes_keys_dev(tq.data_ptr(), 4, 10, 3, None, cls.data_ptr())
            torch.cuda.synchronize()
            k2 = torch.zeros(12, dtype=torch.int64, device=DEV)
            c2 = torch.zeros(12, dtype=torch.int32, device=DEV)
            g.search_top_classes_keys_dev(tq.data_ptr(), 4, 10, 3, k2.data_ptr(), c2.data_ptr())
            g.sync()
            assert torch.equal(keys[:12], k2) and torch.equal(cls[:12], c2)
        with fir.GemmSearch(g, fir.GemmSearch.BF16_SPLIT) as m:
            assert code(m, tq.data_ptr(), 4, 10, 3, keys.data_ptr(), cls.data_ptr()) == FIR_ERR_ARG
    with fir.Gallery(np.zeros((0, d), np.float32), np.zeros(0, np.int32), L2, 0) as g, fir.GemmSearch(g, 2) as m:
        m.search_top_classes_keys_dev(tq.data_ptr(), 4, 10, 3, keys.data_ptr(), cls.data_ptr())           # empty gallery: unused slots
        torch.cuda.synchronize()
        assert torch.all(keys[:12] == -1) and torch.all(cls[:12] == -1)


def test_row_shards_merge_to_the_unsplit_answer(fir):
    n, d, qb, nc, k = 4000, 64, 70, 100, 8
    rows, q = case(31, n, d, qb)
    labels = class_major_even(n, nc)
    tq = torch.from_numpy(q.copy()).to(DEV)

    def keys_of(r, lab, offset, gemm):
        keys = torch.zeros((qb, k), dtype=torch.int64, device=DEV)
        cls = torch.zeros((qb, k), dtype=torch.int32, device=DEV)
        with fir.Gallery(r, lab, L2, 0) as g:
            g.set_row_offset(offset)
            if gemm:
                with fir.GemmSearch(g, 2) as m:
                    m.search_top_classes_keys_dev(tq.data_ptr(), qb, nc, k, keys.data_ptr(), cls.data_ptr())
                    torch.cuda.synchronize()
                    assert m.stats()["fallback_queries"] == 0
            else:
                g.search_top_classes_keys_dev(tq.data_ptr(), qb, nc, k, keys.data_ptr(), cls.data_ptr())
                g.sync()
        return keys.cpu().numpy().view(np.uint64), cls.cpu().numpy()

    whole = keys_of(rows, labels, 0, False)
    parts = [keys_of(rows[a:b], labels[a:b], a, True) for a, b in ((0, 2000), (2000, n))]
    mk, mc = fir.class_keys_merge(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), k)
    assert np.array_equal(mk, whole[0]) and np.array_equal(mc, whole[1])
    assert fir.keys_unpack(parts[1][0])[0].min() >= 2000                          # keys carry the row offset


def test_host_form_routing(fir):
    n, d, qb, nc, k = 3000, 64, 130, 37, 5
    rows, q = case(n + d, n, d, qb)
    labels = synth.make_labels(n, nc)
    with fir.Gallery(rows, labels, L2, 0) as g:
        plain = g.search_top_classes(q, nc, k)                                     # no threshold: n < 65536 stays on the scan
        assert "fir::k_scan<8, 0, 8, 5, " in g.last_dispatch()["kernel"] and g.last_dispatch()["path"] == "scan"
        g.set_large_batch_mfma(64)
        routed = g.search_top_classes(q, nc, k)
        ld = g.last_dispatch()
        assert ld["path"] == "mfma" and "k_gemm_proxy_f16x<1," in ld["kernel"], ld
        assert g.mfma_stats()["fallback_queries"] == 0
        few = g.search_top_classes(q[:63], nc, k)                                  # below the caller's threshold
        assert "fir::k_scan<8, 0, 8, 5, " in g.last_dispatch()["kernel"]
        g.set_large_batch_mfma(0)
        off = g.search_top_classes(q, nc, k)
        assert "fir::k_scan<8, 0, 8, 5, " in g.last_dispatch()["kernel"] and g.last_dispatch()["path"] == "scan"
    for a, b, c in zip(plain, routed, off):
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(c) if c.dtype == np.float32 else c)
    assert all(np.array_equal(a[:63], b) for a, b in zip(plain[:2], few[:2]))


def test_on_a_callers_stream_after_a_call_on_another(fir):
    n, d, qb, nc, k = 3000, 64, 130, 37, 5
    rows, q = case(n + d, n, d, qb)
    labels = synth.make_labels(n, nc)
    with fir.Gallery(rows, labels, L2, 0) as g:
        hc, hi, hd = g.search_top_classes(q, nc, k)
        dq = torch.from_numpy(q.copy()).to(DEV)
        s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        k1 = torch.zeros(qb, dtype=torch.int64, device=DEV)
        keys = torch.full((qb * k + 8,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
        cls = torch.full((qb * k + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        with fir.GemmSearch(g, 2) as m:
            torch.cuda.synchronize()
            m.search_top1_keys_dev(dq.data_ptr(), qb, k1.data_ptr(), stream=s1.cuda_stream)          # no host synchronisation in between
            m.search_top_classes_keys_dev(dq.data_ptr(), qb, nc, k, keys.data_ptr(), cls.data_ptr(), stream=s2.cuda_stream)
            s2.synchronize()
            s1.synchronize()
    assert torch.all(keys[qb * k:] == 0x5A5A5A5A) and torch.all(cls[qb * k:] == 0x5A5A5A5A)
    di, dd = fir.keys_unpack(keys[:qb * k].cpu().numpy().view(np.uint64).reshape(qb, k))
    assert np.array_equal(di, hi) and np.array_equal(bits(dd), bits(hd))
    assert np.array_equal(cls[:qb * k].cpu().numpy().reshape(qb, k), hc)
    assert np.array_equal(fir.keys_unpack(k1.cpu().numpy().view(np.uint64))[0], hi[:, 0])


def test_the_certificate_bound_is_needed_and_a_shrunken_one_is_caught(fir, fir_audit, monkeypatch):
    """The coherent-rounding near-tie of test_gpu_gemm.py with its two rows in different classes, k = 1: row A is the query itself,
    row B's fp16 proxy is lower by most of the rounding window. With the bound as derived both are appended and re-ranked and A's
    class wins; the audit library with the certificate's E shrunk to a quarter appends only B and certifies the wrong class."""
    from test_gpu_gemm import _coherent_rounding_fixture

    rows, q, ia, ib = _coherent_rounding_fixture()
    labels = synth.make_labels(rows.shape[0], 50).copy()
    labels[ia], labels[ib] = 50, 51
    got = {}
    for lib_name, pkg in (("audit", fir_audit), ("shipped", fir)):
        with pkg.Gallery(rows, labels, L2, 0) as g:
            for scale in ("1", "0.25", None):
                if scale is None:
                    monkeypatch.delenv("FIR_GEMM_EREL_SCALE")
                else:
                    monkeypatch.setenv("FIR_GEMM_EREL_SCALE", scale)
                scan, gemm, st = both(pkg, g, q, 52, 1)
                got[lib_name, scale] = (gemm, st["fallback_queries"])
                assert scan[1][0, 0] == 50 and pkg.keys_unpack(scan[0])[0][0, 0] == ia and pkg.keys_unpack(scan[0])[1][0, 0] == 0.0
    for key in (("audit", "1"), ("audit", None), ("shipped", "1"), ("shipped", "0.25"), ("shipped", None)):
        gemm, fb = got[key]
        same(scan, gemm)
        assert fb <= 2, (key, fb)
    gemm, fb = got["audit", "0.25"]
    idx, dist = fir.keys_unpack(gemm[0])
    # the wrong class, certified (no exact scan for it): the shrunken bound is unsound and it shows
    assert gemm[1][0, 0] == 51 and idx[0, 0] == ib and dist[0, 0] > 0.0 and fb <= 2, (gemm[1][0], idx[0], dist[0], fb)
