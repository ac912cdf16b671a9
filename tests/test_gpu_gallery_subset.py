"""Device-side gallery subsets (include/fir_amd.h, "device-side subsets of a gallery"): the row list of a mask, the tiled -> tiled
gather behind fir_gallery_create_subset / _from_rows, the row-major gather, the origin rows and the key map. Nothing has a
tolerance -- rows, labels, counts, classes and keys are compared for equality. The searches over a subset handle, mapped back with
fir_keys_to_origin_dev, must equal BOTH the _masked call of the same name on the source and masked_ref over the source's
fir_range_distances (the restatement tests/test_masked_formulation.py pins to the oracle).
SEG_ROWS is fir_kernels.h's kMaskSegRows: the rows of one segment of the mask scan (64 mask words, one wave)."""
import ctypes as C

import numpy as np
import pytest
import torch

import masked_ref as ref
import subset_ref as sr
import synth
from test_gpu_knn_select import host_keys
from test_gpu_masked_search import DevBuf, dev_mask, kth_radii, masks_of, permuted, random_half, with_garbage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
L2, CHI2, KL = 0, 1, 2
ERR_ARG, ERR_STATE = -1, -5
F32, I32, U64 = np.float32, np.int32, np.uint64
NONE = ref.KEY_NONE
POISON = 0x5A5A5A5A5A5A5A5A
SEG_ROWS = 64 * 64
SEAM_N = 2 * SEG_ROWS + 70                                          # crosses two seams of the scan, the last segment part-full
NS = (1, 63, 64, 65, 130, 300)
DS = (1, 5, 64, 130)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def padding_words(fir, g):
    fn = fir.lib().fir_gallery_padding_words_
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    w = C.c_int64(-1)
    assert fn(g._h, C.byref(w)) == 0
    return w.value


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, I32)).to(DEV)


def to_origin(sub, keys, stream=None):
    """Keys of a call on the subset handle through fir_keys_to_origin_dev, a canary word behind them."""
    keys = np.ascontiguousarray(keys, U64)
    buf = DevBuf(keys.size)
    buf.t[:keys.size] = torch.from_numpy(keys.reshape(-1).view(np.int64)).to(DEV)
    torch.cuda.synchronize()
    sub.keys_to_origin_dev(buf.ptr(), keys.size, stream=stream)
    sub.sync()
    return buf.read().reshape(keys.shape)


def check_handle(fir, sub, rows, labels, sel, tag):
    """Layout, labels and origin of a subset handle against the numpy gather."""
    sel = np.asarray(sel, np.int64)
    assert sub.n == sel.shape[0] and sub.d == rows.shape[1], tag
    if labels is None:
        got = sub.read_rows()
        assert same(got, rows[sel]), tag
    else:
        got, gl = sub.read_rows(with_classes=True)
        assert same(got, rows[sel]) and same(gl, labels[sel].astype(I32)), tag
    assert padding_words(fir, sub) == 0, tag
    assert same(sub.origin_rows(), sel.astype(I32)), tag
    if sel.shape[0] > 2:
        assert same(sub.origin_rows(1, sel.shape[0] - 2), sel[1:-1].astype(I32)), tag


# ---- mask -> row list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS + (SEAM_N,))
def test_rows_of_mask_host_and_device_forms(fir, n):
    rows = synth.make_gallery(601, n, 4, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        for name, take in masks_of(n, 602 + n).items():
            want = np.flatnonzero(take).astype(I32)
            count = want.shape[0]
            for arg in (take, with_garbage(take)):
                c, got = g.rows_of_mask(arg)
                assert c == count and same(got, want), (n, name)
            assert same(want, sr.rows_of_mask(ref.pack_bits(take), n))
            for cap in sorted({0, max(count - 1, 0), count, count + 3}):                       # below, at and above the count; 0 = count only
                c, got = g.rows_of_mask(take, cap)
                assert c == count and same(got, want[:cap]), (n, name, cap)
            # the device form: canaries behind the rows, the count as one int64, two calls the same bytes
            mt = torch.from_numpy(with_garbage(take).view(np.int64)).to(DEV)
            for cap in sorted({max(count - 1, 0), count + 3}):
                outs = []
                for _ in range(2):
                    rbuf, cbuf = DevBuf(cap, torch.int32), DevBuf(1)
                    g.rows_of_mask_dev(mt.data_ptr(), rbuf.ptr() if cap else None, cap, cbuf.ptr())
                    g.sync()
                    r = rbuf.read()
                    assert int(cbuf.read()[0]) == count, (n, name, cap)
                    assert same(r[:min(cap, count)], want[:cap]) and np.all(r[min(cap, count):] == 0x5A5A5A5A), (n, name, cap)
                    outs.append(r.tobytes())
                assert outs[0] == outs[1]
        st = torch.cuda.Stream()                                                            # a caller's stream, the count-only call
        cbuf, ot = DevBuf(1), dev_mask(fir, np.ones(n, bool))
        g.rows_of_mask_dev(ot.data_ptr(), None, 0, cbuf.ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert int(cbuf.read()[0]) == n


# ---- layout, labels, origin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
def test_mask_subsets_hold_the_selected_rows_and_labels(fir, d):
    for n in NS:
        rows = synth.make_gallery(611 + n, n, d, L2)
        labels = permuted(n, 7, 612 + n) - 2
        with fir.Gallery(rows, labels, L2, 0) as g, fir.Gallery(rows, None, L2, 0) as plain:
            for name, take in masks_of(n, 613 + n).items():
                sel = np.flatnonzero(take)
                for arg in (take, with_garbage(take)):
                    with g.subset(arg) as sub:
                        check_handle(fir, sub, rows, labels, sel, (n, d, name))
                mt = dev_mask(fir, take)
                with g.subset(mask_ptr=mt.data_ptr()) as sub:                              # the device form
                    check_handle(fir, sub, rows, labels, sel, (n, d, name, "dev"))
                with plain.subset(take) as sub:                                            # an unlabelled source: an unlabelled subset
                    check_handle(fir, sub, rows, None, sel, (n, d, name, "unlabelled"))
                    if sel.shape[0]:
                        with pytest.raises(fir.FirError) as e:
                            sub.read_rows(with_classes=True)
                        assert e.value.code == ERR_STATE


def test_a_subset_across_the_seams_of_the_scan(fir):
    n, d = SEAM_N, 4
    rows = synth.make_gallery(621, n, d, L2)
    labels = permuted(n, 50, 622)
    with fir.Gallery(rows, labels, L2, 0) as g:
        for name in ("half", "zero words", "ones", "last"):
            take = masks_of(n, 623)[name]
            with g.subset(with_garbage(take)) as sub:
                check_handle(fir, sub, rows, labels, np.flatnonzero(take), name)


@pytest.mark.parametrize("d", DS)
def test_row_lists_any_order_with_repeats(fir, d):
    n = 130
    rows = synth.make_gallery(631, n, d, L2)
    labels = permuted(n, 9, 632)
    rng = np.random.default_rng(633 + d)
    lists = {"reversed": np.arange(n)[::-1], "repeats": np.array([5, 5, 129, 0, 5, 64, 63, 0]), "longer than n": rng.integers(0, n, 3 * n + 7)}
    for m in (63, 64, 65):
        lists[f"m={m}"] = rng.integers(0, n, m)
    with fir.Gallery(rows, labels, L2, 0) as g, fir.Gallery(rows, None, L2, 0) as plain:
        for name, sel in lists.items():
            with g.from_rows(sel) as sub:
                check_handle(fir, sub, rows, labels, sel, (d, name))
            st = dev_i32(sel)
            with g.from_rows(rows_ptr=st.data_ptr(), m=sel.shape[0]) as sub:
                check_handle(fir, sub, rows, labels, sel, (d, name, "dev"))
            with plain.from_rows(sel) as sub:
                check_handle(fir, sub, rows, None, sel, (d, name, "unlabelled"))
        # the device list form cannot fail late: a bad index is a row of zeros with label -1 and origin -1
        bad = np.array([3, -1, n, 7, 1 << 30], I32)
        bt = dev_i32(bad)
        with g.from_rows(rows_ptr=bt.data_ptr(), m=5) as sub:
            got, gl = sub.read_rows(with_classes=True)
            ok = np.array([True, False, False, True, False])
            assert same(got[ok], rows[[3, 7]]) and np.all(got[~ok] == 0) and gl.tolist() == [labels[3], -1, -1, labels[7], -1]
            assert sub.origin_rows().tolist() == [3, -1, -1, 7, -1] and padding_words(fir, sub) == 0
            keys = np.array([1 << 32 | 0, 1 << 32 | 1, 1 << 32 | 3, 1 << 32 | 5, int(NONE)], U64)
            assert to_origin(sub, keys).tolist() == [1 << 32 | 3, int(NONE), 1 << 32 | 7, int(NONE), int(NONE)]     # a zero row and a row past m map to none


@pytest.mark.parametrize("bad_value", (np.nan, -0.25))
def test_the_plain_range_flag_is_recomputed_from_the_gathered_values(fir, bad_value):
    n, d = 130, 64
    rows = synth.make_gallery(641, n, d, CHI2)
    rows[77, 13] = F32(bad_value)
    q, _ = synth.make_queries(642, rows, 9, CHI2)
    with fir.Gallery(rows, None, CHI2, 0) as g:
        assert g.value_range()[0] is False
        without = np.ones(n, bool)
        without[77] = False
        with g.subset(without) as sub, fir.Gallery(rows[without], None, CHI2, 0) as fresh:
            assert sub.value_range()[0] is True and fresh.value_range()[0] is True
            for a, b in zip(sub.search_top1(q), fresh.search_top1(q)):
                assert a.tobytes() == b.tobytes()
        with g.subset(~without | (np.arange(n) < 3)) as sub:
            assert sub.value_range()[0] is False
        with g.from_rows([76, 78]) as sub:
            assert sub.value_range()[0] is True
        with g.from_rows([76, 77, 77]) as sub:
            assert sub.value_range()[0] is False


# ---- searches over the subset handle, mapped back ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_searches_mapped_back_equal_the_masked_calls_and_the_restatement(fir, metric):
    n, d, qb, nc = 300, 64, 17, 12
    rows = synth.make_gallery(651, n, d, metric)
    rows[55] = rows[40]                                                        # equal distances: rows 40, 55 and 250 tie for every query
    rows[250] = rows[40]
    labels = permuted(n, nc, 652)
    q, _ = synth.make_queries(653, rows, qb, metric)
    q[0] = rows[40]
    excl = permuted(qb, nc, 654)
    with fir.Gallery(rows, labels, metric, 0) as g:
        for off in (0, 1000):
            g.set_row_offset(off)
            for name in ("half", "zero words", "one bit", "ones"):
                take = masks_of(n, 655)[name].copy()
                if name != "one bit":
                    take[[55, 250]] = True
                    take[40] = name == "ones"
                with g.subset(take) as sub:
                    for start, end in ((0, 0), (3, 61)):
                        dist = g.range_distances(q, start, end)
                        tag = (metric, off, name, start, end)
                        got = to_origin(sub, host_keys(*sub.search_top1(q, start, end)))
                        assert np.array_equal(got, host_keys(*g.search_top1_masked(q, take, start, end))), ("top1 masked",) + tag
                        assert np.array_equal(got, ref.top1_keys(dist, take, off)), ("top1 ref",) + tag
                        for k in (1, 9):
                            got = to_origin(sub, host_keys(*sub.search_knn(q, k, start, end)))
                            assert np.array_equal(got, host_keys(*g.search_knn_masked(q, take, k, start, end))), ("knn masked", k) + tag
                            assert np.array_equal(got, ref.knn_keys(dist, take, k, off)), ("knn ref", k) + tag
                        radii = kth_radii(dist, take, 5)
                        cnt, idx, dd = sub.search_radius(q, radii, 8, start, end)
                        mc, mi, md = g.search_radius_masked(q, take, radii, 8, start, end)
                        wc, wk = ref.radius_keys(dist, take, radii, 8, off)
                        got = to_origin(sub, host_keys(idx, dd))
                        assert np.array_equal(cnt, mc) and np.array_equal(cnt, wc), ("radius counts",) + tag
                        assert np.array_equal(got, host_keys(mi, md)) and np.array_equal(got, wk), ("radius keys",) + tag
                        cls, idx, dd = sub.search_top_classes(q, nc, 5, start, end)
                        mcls, mi, md = g.search_top_classes_masked(q, take, nc, 5, start, end)
                        kc, cc = ref.class_keys(dist, take, labels, nc, 5, off)
                        got = to_origin(sub, host_keys(idx, dd))
                        assert np.array_equal(got, host_keys(mi, md)) and np.array_equal(cls, mcls), ("classes masked",) + tag
                        assert np.array_equal(got, kc) and np.array_equal(cls, cc), ("classes ref",) + tag
                        # other-class: the source has no masked form of it; the mask AND "class differs" composes it, query by query
                        got = to_origin(sub, host_keys(*sub.search_top1_other_class(q, excl, start, end)))
                        for i in range(qb):
                            both = take & (labels != excl[i])
                            assert got[i] == ref.top1_keys(dist[i:i + 1], both, off)[0], ("other class ref", i) + tag
                            if i < 5:
                                assert got[i] == host_keys(*g.search_top1_masked(q[i:i + 1], both, start, end))[0], ("other class masked", i) + tag
                    if name == "half" and off == 0:
                        two = to_origin(sub, host_keys(*sub.search_knn(q[:1], 2)))[0]       # the copies of the query's own row, lowest first
                        assert (two & np.uint64(0xFFFFFFFF)).tolist() == [55, 250]
        g.set_row_offset(0)


def test_the_subsets_own_row_offset_and_the_sources_offset_at_creation(fir):
    n, d, qb = 300, 16, 9
    rows = synth.make_gallery(661, n, d, L2)
    q, _ = synth.make_queries(662, rows, qb, L2)
    take = random_half(n, 663)
    with fir.Gallery(rows, None, L2, 0) as g:
        g.set_row_offset(1000)
        with g.subset(take) as sub:
            g.set_row_offset(5)                                                # afterwards: the subset keeps 1000
            sub.set_row_offset(77)                                             # its own offset is taken out of the keys it is given
            idx, dist = sub.search_knn(q, 9)
            assert idx.min() >= 77
            got = to_origin(sub, host_keys(idx, dist))
            g.set_row_offset(1000)
            assert np.array_equal(got, host_keys(*g.search_knn_masked(q, take, 9)))
            low = np.array([1 << 32 | 76, 1 << 32 | (77 + sub.n), 1 << 32 | 77], U64)     # below and past the handle's rows: none
            assert to_origin(sub, low).tolist() == [int(NONE), int(NONE), 1 << 32 | (int(np.flatnonzero(take)[0]) + 1000)]


def test_routed_forms_at_the_smallest_gated_shape(fir):
    """300 x 64, L2, a caller's threshold of one query, 130 queries: the subset handle takes the matrix cores, which no masked call can."""
    n, d, qb, nc = 300, 64, 130, 12
    rows = synth.make_gallery(671, n, d, L2)
    labels = permuted(n, nc, 672)
    q, _ = synth.make_queries(673, rows, qb, L2)
    take = masks_of(n, 674)["zero words"]
    with fir.Gallery(rows, labels, L2, 0) as g, g.subset(take) as sub:
        sub.set_large_batch_mfma(1)
        got = to_origin(sub, host_keys(*sub.search_top1(q)))
        assert sub.last_dispatch()["path"] == "mfma", sub.last_dispatch()
        assert np.array_equal(got, host_keys(*g.search_top1_masked(q, take)))
        assert g.last_dispatch()["path"] == "scan"
        passes = sub.mfma_stats()["passes"]
        assert passes > 0
        got = to_origin(sub, host_keys(*sub.search_knn(q, 9)))
        assert sub.mfma_stats()["passes"] > passes
        assert np.array_equal(got, host_keys(*g.search_knn_masked(q, take, 9)))
        passes = sub.mfma_stats()["passes"]
        cls, idx, dd = sub.search_top_classes(q, nc, 2)
        assert sub.mfma_stats()["passes"] > passes
        mcls, mi, md = g.search_top_classes_masked(q, take, nc, 2)
        assert np.array_equal(to_origin(sub, host_keys(idx, dd)), host_keys(mi, md)) and np.array_equal(cls, mcls)


# ---- the row-major gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
def test_gather_rows_dev(fir, d):
    n = 130
    rows = synth.make_gallery(681, n, d, L2)
    labels = permuted(n, 9, 682) + 100
    sel = np.array([129, 0, 64, 64, 63, -1, n, 5, 5, 5, 1 << 30, 128], I32)
    ok = (sel >= 0) & (sel < n)
    want = np.where(ok[:, None], rows[np.where(ok, sel, 0)], F32(0))
    it = dev_i32(sel)
    with fir.Gallery(rows, labels, L2, 0) as g, fir.Gallery(rows, None, L2, 0) as plain:
        for stream in (None, torch.cuda.Stream()):
            out = torch.full((sel.shape[0] * d + 8,), 7.5, dtype=torch.float32, device=DEV)
            cls = DevBuf(sel.shape[0], torch.int32)
            torch.cuda.synchronize()
            g.gather_rows_dev(it.data_ptr(), sel.shape[0], out.data_ptr(), cls.ptr(), stream=stream.cuda_stream if stream else None)
            g.sync()
            if stream:
                stream.synchronize()
            o = out.cpu().numpy()
            assert np.all(o[sel.shape[0] * d:] == F32(7.5))
            assert same(o[:sel.shape[0] * d].reshape(-1, d), want.astype(F32))
            assert cls.read().tolist() == np.where(ok, labels[np.where(ok, sel, 0)], -1).tolist()
        out = torch.zeros(sel.shape[0] * d, dtype=torch.float32, device=DEV)
        plain.gather_rows_dev(it.data_ptr(), sel.shape[0], out.data_ptr())                 # no labels asked for: fine without them
        plain.sync()
        assert same(out.cpu().numpy().reshape(-1, d), want.astype(F32))
        with pytest.raises(fir.FirError) as e:
            plain.gather_rows_dev(it.data_ptr(), sel.shape[0], out.data_ptr(), DevBuf(12, torch.int32).ptr())
        assert e.value.code == ERR_STATE


def test_a_whole_split_without_leaving_the_device(fir):
    """gallery = the subset of `take`, queries = the gathered complement, keys mapped: fir_search_top1_masked of the same split."""
    n, d = 300, 64
    rows = synth.make_gallery(691, n, d, L2)
    rows[202] = rows[3]
    take = np.arange(n) % 3 != 0
    st = torch.cuda.Stream()
    with fir.Gallery(rows, None, L2, 0) as g:
        want = host_keys(*g.search_top1_masked(rows[~take], take))
        inv, m = dev_mask(fir, ~take), int((~take).sum())
        idx, cnt, qs, keys = DevBuf(m, torch.int32), DevBuf(1), torch.zeros(m * d, dtype=torch.float32, device=DEV), DevBuf(m)
        torch.cuda.synchronize()
        tk = dev_mask(fir, take)
        with g.subset(mask_ptr=tk.data_ptr(), stream=st.cuda_stream) as sub:
            g.rows_of_mask_dev(inv.data_ptr(), idx.ptr(), m, cnt.ptr(), stream=st.cuda_stream)
            g.gather_rows_dev(idx.ptr(), m, qs.data_ptr(), stream=st.cuda_stream)
            sub.search_top1_keys_dev(qs.data_ptr(), m, keys.ptr(), stream=st.cuda_stream)
            sub.keys_to_origin_dev(keys.ptr(), m, stream=st.cuda_stream)
            st.synchronize()
            assert int(cnt.read()[0]) == m and same(idx.read(), np.flatnonzero(~take).astype(I32))
            got = keys.read()
        assert np.array_equal(got, want)
        assert int(got[1] & np.uint64(0xFFFFFFFF)) == 202                                   # test row 3's copy


# ---- order and lifetime ----------------------------------------------------------------------------------------------------------------
def test_creation_is_a_call_on_the_source_and_the_subset_stands_alone(fir):
    n, d, extra, qb = 200, 64, 70, 9
    rows = synth.make_gallery(701, n + extra, d, L2)
    labels = permuted(n + extra, 6, 702)
    q, _ = synth.make_queries(703, rows, qb, L2)
    take = random_half(n + extra, 704)
    take[n:] = True
    sel = np.flatnonzero(take)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    rt, lt, mt = torch.from_numpy(rows[n:]).to(DEV), dev_i32(labels[n:]), dev_mask(fir, take)
    torch.cuda.synchronize()
    g = fir.Gallery(rows[:n], labels[:n], L2, 0)
    g.reserve(n + extra)
    g.append_dev(rt.data_ptr(), extra, lt.data_ptr(), stream=s1.cuda_stream)             # queued on one stream ...
    sub = g.subset(mask_ptr=mt.data_ptr(), stream=s2.cuda_stream)                          # ... seen by the creation on another
    check_handle(fir, sub, rows, labels, sel, "after append_dev")
    before = sub.search_knn(q, 9)
    with fir.Gallery(rows[sel], labels[sel], L2, 0) as fresh:
        for a, b in zip(before, fresh.search_knn(q, 9)):
            assert a.tobytes() == b.tobytes()
    mem = sub.memory_bytes()
    assert mem["scratch"] >= 4 * sel.shape[0]                                             # the row list, 4 bytes per row
    g.set_rows([int(sel[0]), int(sel[-1])], rows[:2] * F32(3.0))                          # the source changes, shrinks, goes away
    g.remove_rows(sel[:20])
    for a, b in zip(before, sub.search_knn(q, 9)):
        assert a.tobytes() == b.tobytes()
    g.close()
    for a, b in zip(before, sub.search_knn(q, 9)):
        assert a.tobytes() == b.tobytes()
    assert same(sub.origin_rows(), sel.astype(I32))
    # an in-place update of the subset itself ends the map
    sub.append(rows[:1], labels[:1])
    keys = DevBuf(1)
    for call in (lambda: sub.origin_rows(0, 1), lambda: sub.keys_to_origin_dev(keys.ptr(), 1)):
        with pytest.raises(fir.FirError) as e:
            call()
        assert e.value.code == ERR_STATE and "changed in place" in str(e.value)
    sub.sync()
    assert keys.read()[0] == np.uint64(POISON)
    sub.close()


def test_errors_and_empty_subsets(fir):
    n, d = 100, 16
    rows = synth.make_gallery(711, n, d, L2)
    labels = permuted(n, 5, 712)
    L = fir.lib()
    p = lambda a: a.ctypes.data_as(fir.capi._vp)
    vp = fir.capi._vp
    mask = fir.pack_row_mask(np.arange(n) % 2 == 0)
    lst = np.array([1, 2, 3], I32)
    out_rows, cnt = np.full(8, 77, I32), C.c_int64(-7)

    def err(rc, code, text):
        assert rc == code and text in L.fir_last_error().decode(), (rc, L.fir_last_error())

    with fir.Gallery(rows, labels, L2, 0) as g:
        h, new = g._h, vp()
        mem0 = g.memory_bytes()
        err(L.fir_gallery_create_subset(None, p(mask), C.byref(new)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_create_subset(h, None, C.byref(new)), ERR_ARG, "NULL argument")             # a NULL mask with n > 0
        err(L.fir_gallery_create_subset(h, p(mask), None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_create_subset_dev(h, None, None, C.byref(new)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_create_from_rows(h, None, 3, C.byref(new)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_create_from_rows(h, p(lst), 3, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_create_from_rows(h, p(lst), -1, C.byref(new)), ERR_ARG, "m < 0")
        err(L.fir_gallery_create_from_rows_dev(h, None, 3, None, C.byref(new)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_create_from_rows_dev(h, p(lst), -1, None, C.byref(new)), ERR_ARG, "m < 0")
        err(L.fir_gallery_create_from_rows(h, p(np.array([1, n, 3], I32)), 3, C.byref(new)), ERR_ARG, f"row index {n} (entry 1 of the list) outside [0,{n})")
        err(L.fir_gallery_create_from_rows(h, p(np.array([1, 2, -4], I32)), 3, C.byref(new)), ERR_ARG, "row index -4")
        assert not new.value and g.memory_bytes() == mem0                                            # nothing was allocated
        err(L.fir_gallery_rows_of_mask(h, None, p(out_rows), 8, C.byref(cnt)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_rows_of_mask(h, p(mask), None, 8, C.byref(cnt)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_rows_of_mask(h, p(mask), p(out_rows), 8, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_rows_of_mask(h, p(mask), p(out_rows), -1, C.byref(cnt)), ERR_ARG, "cap < 0")
        err(L.fir_gallery_rows_of_mask_dev(h, p(mask), None, 0, None, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_gather_rows_dev(h, None, 3, p(rows), None, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_gather_rows_dev(h, p(lst), 3, None, None, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_gather_rows_dev(h, p(lst), -1, p(rows), None, None), ERR_ARG, "m < 0")
        assert np.all(out_rows == 77) and cnt.value == -7
        # an ordinary handle has no origin
        err(L.fir_gallery_origin_rows(h, 0, 1, p(out_rows)), ERR_STATE, "no origin rows")
        err(L.fir_keys_to_origin_dev(h, p(mask), 1, None), ERR_STATE, "no origin rows")
        err(L.fir_keys_to_origin_dev(None, p(mask), 1, None), ERR_ARG, "NULL argument")
        with g.subset(np.arange(n) < 10) as sub:
            err(L.fir_gallery_origin_rows(sub._h, 5, 6, p(out_rows)), ERR_ARG, "outside [0,10)")
            err(L.fir_gallery_origin_rows(sub._h, 0, -1, p(out_rows)), ERR_ARG, "m < 0")
            err(L.fir_keys_to_origin_dev(sub._h, None, 1, None), ERR_ARG, "NULL argument")
            err(L.fir_keys_to_origin_dev(sub._h, p(mask), -1, None), ERR_ARG, "count < 0")
            assert sub.origin_rows(10, 0).shape == (0,)
        # empty subsets answer like an empty gallery
        q = rows[:3]
        zt = dev_mask(fir, np.zeros(n, bool))
        for sub in (g.subset(np.zeros(n, bool)), g.from_rows([]), g.from_rows(rows_ptr=0, m=0), g.subset(mask_ptr=zt.data_ptr())):
            with sub, fir.Gallery(np.zeros((0, d), F32), None, L2, 0) as empty:
                assert sub.n == 0 and sub.origin_rows().shape == (0,)
                for a, b in zip(sub.search_top1(q) + sub.search_knn(q, 4) + sub.search_radius(q, np.inf, 2), empty.search_top1(q) + empty.search_knn(q, 4) + empty.search_radius(q, np.inf, 2)):
                    assert a.tobytes() == b.tobytes()
                assert np.all(sub.search_top1(q)[0] == -1)
                keys = DevBuf(2)
                sub.keys_to_origin_dev(keys.ptr(), 2)                                       # any row is outside an empty handle's rows
                sub.sync()
                assert np.all(keys.read() == NONE)
    with fir.Gallery(np.zeros((0, d), F32), None, L2, 0) as empty:                             # an empty source: the mask is not read
        c, r = empty.rows_of_mask(None)
        assert c == 0 and r.shape == (0,)
        with empty.subset(mask_ptr=0) as sub:
            assert sub.n == 0
