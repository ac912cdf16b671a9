"""Linear projection / PCA on the device (include/fir_amd.h, "linear projection / PCA"): fir_gallery_feature_stats,
fir_gallery_scatter, fir_projection and fir_gallery_create_projected against tests/projection_ref.py.

Exact where the contract is exact (counts, min / max, symmetry, repeatability, identity / selection bases, the equality of the
row-major and the tiled path, the layout invariant, labels, offsets, every search on a projected handle against a handle created
afresh over its rows); inside projection_ref's derived bounds where float64 sums are taken in the device's order.

SEG_ROWS is fir_projection.h's kPjSegMinTiles * 64: the rows of one row segment of the column-sum and scatter kernels at these sizes.
SEAM_N crosses three seams and leaves the last segment part-full, its last tile too. STRIDE_N has more tiles than the projection
kernel's largest grid takes in one step (8 workgroups a compute unit, 4 tiles each), so its waves come round a second time."""
import ctypes as C

import numpy as np
import pytest
import torch

import projection_ref as pr
import synth
from test_gpu_masked_search import masks_of, permuted, with_garbage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
L2, CHI2 = 0, 1
ERR_ARG = -1
F32, F64, I32 = np.float32, np.float64, np.int32
NS = (1, 63, 64, 65, 130, 300)
DS = (1, 3, 4, 5, 64, 68, 130)
SEG_ROWS = 8 * 64
SEAM_N, SEAM_D = 3 * SEG_ROWS + 100, 8


def ps_of(d):
    return sorted({1, 3, 4, 5, 16, 17, 64, d, d + 3})


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_values(a, b):
    """The same bytes wherever either is a number; NaN where the other is NaN (count 0 or 1: a NaN's payload is no contract)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and same(np.where(na, 0.0, a), np.where(nb, 0.0, b))


def padding_words(fir, g):
    fn = fir.lib().fir_gallery_padding_words_
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    w = C.c_int64(-1)
    assert fn(g._h, C.byref(w)) == 0
    return w.value


def device_sums(fir, g, mask):
    fn = fir.lib().fir_gallery_feature_sums_
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 4
    m, pm = g._mask(mask)
    s, q = np.empty(g.d, F64), np.empty(g.d, F64)
    assert fn(g._h, pm, s.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)) == 0
    return s, q


def wide_rows(seed, n, d):
    """float32 values spanning 2^-20 .. 2^10 with a non-zero mean: a padding row left un-gated after centring would show."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.integers(-20, 11, size=(n, d))
    return (rng.standard_normal((n, d)) * scale + 0.75 * scale).astype(F32)


def the_masks(n, seed):
    """name -> bool[n] or packed words: None, all ones, empty, one row, only the last row, a whole tile cleared, garbage past n."""
    m = masks_of(n, seed)
    out = {"null": None, "ones": m["ones"], "zeros": m["zeros"], "one bit": m["one bit"], "last": m["last"], "zero words": m["zero words"],
           "half": m["half"], "garbage": with_garbage(m["half"])}
    return out, {"null": m["ones"], "garbage": m["half"]}


def shapes():
    return [(n, d) for d in DS for n in NS] + [(SEAM_N, SEAM_D)]


# ---- feature statistics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS + (SEAM_D,))
def test_feature_stats(fir, d):
    for n in ((SEAM_N,) if d == SEAM_D else NS):
        rows = wide_rows(700 + n + d, n, d)
        with fir.Gallery(rows, None, L2, 0) as g:
            masks, alias = the_masks(n, 701 + n)
            outs = {}
            for name, mask in masks.items():
                take = alias.get(name, mask)
                tag = (n, d, name)
                got = g.feature_stats(mask)
                again = g.feature_stats(mask)
                assert got[0] == again[0] and all(same(a, b) for a, b in zip(got[1:], again[1:])), tag      # the same bytes twice
                outs[name] = got
                m, s, sq, sabs = pr.column_sums(rows, take)
                lo, hi = pr.min_max(rows, take)
                assert got[0] == m, tag
                assert same(got[1], lo) and same(got[2], hi), tag
                ds, dq = device_sums(fir, g, mask)
                ok, worst = pr.within(ds, s, pr.sums_bound(sabs, m))
                assert ok, (tag, "sum", worst)
                ok, worst = pr.within(dq, sq, pr.sums_bound(sq.astype(F64), m))
                assert ok, (tag, "sum of squares", worst)
                avg, sd = pr.std_formula(ds, dq, m)                                              # the literal formula from the device's sums
                assert same_values(got[3], avg) and same_values(got[4], sd), tag
                if m > 1:
                    assert np.all(np.isfinite(got[3])), tag
            assert all(same(a, b) for a, b in zip(outs["null"][1:], outs["ones"][1:]))           # all ones = NULL, garbage bits change nothing
            assert all(same(a, b) for a, b in zip(outs["half"][1:], outs["garbage"][1:]))


# ---- scatter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS + (SEAM_D,))
def test_scatter(fir, d):
    for n in ((SEAM_N,) if d == SEAM_D else NS):
        rows = wide_rows(720 + n + d, n, d)
        own = np.random.default_rng(721 + n).standard_normal(d) * 0.5 + 0.25                    # a caller's centre
        with fir.Gallery(rows, None, L2, 0) as g:
            masks, alias = the_masks(n, 722 + n)
            outs = {}
            for name, mask in masks.items():
                take = alias.get(name, mask)
                tag = (n, d, name)
                s, mean, count = g.scatter(mask)
                s2, mean2, count2 = g.scatter(mask)
                assert count == count2 and same(s, s2) and same(mean, mean2), tag
                assert same(s, s.T.copy()), tag                                                  # symmetric bit for bit
                outs[name] = (s, mean)
                m = int(np.asarray(take).sum())
                assert count == m, tag
                if m > 0:
                    ds, _ = device_sums(fir, g, mask)
                    assert same(mean, ds / F64(m)), tag                                          # the mean of the column-sum kernel
                else:
                    assert same(mean, np.zeros(d)), tag
                exact, bound = pr.scatter(rows, take, mean)
                ok, worst = pr.within(s, exact, bound)
                assert ok, (tag, "null centre", worst)
                so, co, cnt = g.scatter(mask, own)
                assert cnt == m and same(co, own) and same(so, so.T.copy()), tag
                exact, bound = pr.scatter(rows, take, own)
                ok, worst = pr.within(so, exact, bound)
                assert ok, (tag, "own centre", worst)
            assert same(outs["null"][0], outs["ones"][0]) and same(outs["null"][1], outs["ones"][1])
            assert same(outs["half"][0], outs["garbage"][0])


# ---- projection: exact cases ----------------------------------------------------------------------------------------------------------
def apply_dev(proj, rows, stream=None):
    t = torch.from_numpy(np.ascontiguousarray(rows, F32)).to(DEV)
    out = torch.full((rows.shape[0] * proj.p + 8,), 7.5, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    proj.apply_dev(t.data_ptr(), rows.shape[0], out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[rows.shape[0] * proj.p:] == 7.5)                                             # nothing written past the end
    return o[:rows.shape[0] * proj.p].reshape(rows.shape[0], proj.p).copy()


def check_projected(fir, g, proj, rows, labels, tag):
    """Layout, labels, offset and the equality of the three paths; returns the projected rows."""
    with g.projected(proj) as h:
        assert (h.n, h.d) == (g.n, proj.p), tag
        got, gl = h.read_rows(with_classes=True)
        assert same(gl, labels), tag
        assert padding_words(fir, h) == 0, tag
        again = g.projected(proj)
        assert same(again.read_rows(), got), tag
        again.close()
    src = g.read_rows()
    assert same(src, rows), tag
    assert same(proj.apply(src), got), tag                                                       # the row-major path: the same bits
    assert same(apply_dev(proj, src), got), tag
    return got


@pytest.mark.parametrize("d", DS)
def test_identity_selection_and_centred_bases_are_exact(fir, d):
    rng = np.random.default_rng(740 + d)
    for n in NS:
        rows = wide_rows(741 + n + d, n, d)
        labels = permuted(n, 7, 742 + n) - 2
        with fir.Gallery(rows, labels, L2, 0) as g:
            with fir.Projection(np.eye(d)) as ident:
                assert same(check_projected(fir, g, ident, rows, labels, (n, d, "identity")), rows)
            for p in ps_of(d):
                sel = rng.integers(0, d, p)                                                      # selection (p <= d: a permutation prefix), repeats past d
                if p <= d:
                    sel = rng.permutation(d)[:p]
                basis = np.zeros((p, d))
                basis[np.arange(p), sel] = 1.0
                with fir.Projection(basis) as proj:
                    assert proj.info() == (p, d, 0)
                    assert same(check_projected(fir, g, proj, rows, labels, (n, d, p, "selection")), rows[:, sel]), (n, d, p)
            c = rng.standard_normal(d) * 3.0
            with fir.Projection(np.eye(d), c) as cen:
                want = (rows.astype(F64) - c[None, :]).astype(F32)
                assert same(check_projected(fir, g, cen, rows, labels, (n, d, "centred identity")), want), (n, d)


def test_row_offset_labels_and_independence_of_the_source(fir):
    n, d, p = 130, 5, 3
    rows = wide_rows(750, n, d)
    labels = permuted(n, 9, 751)
    basis = np.random.default_rng(752).standard_normal((p, d))
    g = fir.Gallery(rows, labels, L2, 0)
    g.set_row_offset(1000)
    with fir.Projection(basis) as proj:
        h = g.projected(proj)
        plain = fir.Gallery(rows, None, L2, 0).projected(proj)                                   # a source without labels: none carried
        with pytest.raises(fir.FirError):
            plain.read_rows(with_classes=True)
        plain.close()
    got = h.read_rows()
    g.set_rows(np.arange(n, dtype=I32), np.zeros((n, d), F32))                                   # the source changes, then goes
    g.close()
    assert same(h.read_rows(), got)
    idx, dist = h.search_top1(got[:17])
    assert same(idx, (np.arange(17) + 1000).astype(I32)) and np.all(dist == 0)                   # the offset was carried; itself at distance 0
    with pytest.raises(fir.FirError):
        h.origin_rows()                                                                          # no origin list
    h.close()


def test_more_tiles_than_one_grid_step(fir):
    cus = fir.device_info(0)["cus"]
    n, d = cus * 8 * 4 * 64 + 5 * 64 + 3, 8
    rng = np.random.default_rng(760)
    rows = rng.standard_normal((n, d)).astype(F32)
    sel = rng.permutation(d)[:4]
    basis = np.zeros((4, d))
    basis[np.arange(4), sel] = 1.0
    with fir.Gallery(rows, None, L2, 0) as g, fir.Projection(basis) as proj, g.projected(proj) as h:
        assert same(h.read_rows(), rows[:, sel])
        assert padding_words(fir, h) == 0
        assert same(proj.apply(rows), rows[:, sel])
    # the row-major form in several slabs: 64 MiB of tiled input and output a slab, 10880 rows at 1536 -> 4 features
    m, d = 10880 + 70, 1536
    rows = rng.standard_normal((m, d)).astype(F32)
    sel = rng.permutation(d)[:4]
    basis = np.zeros((4, d))
    basis[np.arange(4), sel] = 1.0
    with fir.Projection(basis) as proj:
        assert same(proj.apply(rows), rows[:, sel])
        assert same(apply_dev(proj, rows), rows[:, sel])


# ---- projection: inside the bound -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS + (SEAM_D,))
def test_random_bases_stay_inside_the_bound(fir, d):
    rng = np.random.default_rng(770 + d)
    for n in ((SEAM_N,) if d == SEAM_D else NS):
        rows = wide_rows(771 + n + d, n, d)
        labels = permuted(n, 5, 772 + n)
        center = rows.astype(F64).mean(axis=0)
        with fir.Gallery(rows, labels, L2, 0) as g:
            for p in ps_of(d):
                basis = rng.standard_normal((p, d)) * 2.0 ** rng.integers(-3, 4, size=(p, 1))
                for c in (None, center):
                    with fir.Projection(basis, c) as proj:
                        got = check_projected(fir, g, proj, rows, labels, (n, d, p))
                    exact, bound = pr.project(rows, basis, c)
                    ok, worst = pr.within(got, exact, bound)
                    assert ok, (n, d, p, c is not None, worst)


# ---- a projected handle answers like a handle created over its rows --------------------------------------------------------------------
def all_searches(g, q, nc):
    out = [g.search_top1(q), g.search_topk(q, 5), g.search_knn(q, 9), g.search_top_classes(q, nc, 3)]
    kd = out[2][1][:, 4]
    out.append(g.search_radius(q, np.nextafter(kd, F32(np.inf)), 8))
    return [np.ascontiguousarray(a) for t in out for a in t]


@pytest.mark.parametrize("metric", (L2, CHI2))
def test_searches_equal_a_fresh_handle(fir, metric):
    rng = np.random.default_rng(780 + metric)
    nc = 11
    for n, d, p, qb in ((300, 68, 17, 9), (130, 5, 8, 33), (300, 130, 64, 130)):
        rows = synth.make_gallery(781 + n, n, d, metric)
        labels = permuted(n, nc, 782 + n)
        basis = np.abs(rng.standard_normal((p, d))) / d                                           # non-negative features stay non-negative
        with fir.Gallery(rows, labels, metric, 0) as g, fir.Projection(basis) as proj, g.projected(proj) as h:
            y = h.read_rows()
            q = proj.apply(synth.make_queries(783 + n, rows, qb, metric)[0])
            q[::3] = y[(np.arange(q[::3].shape[0]) * 7) % n]                                      # some queries are gallery rows themselves
            with fir.Gallery(y, labels, metric, 0) as fresh:
                assert h.value_range()[0] == fresh.value_range()[0]
                for a, b in zip(all_searches(h, q, nc), all_searches(fresh, q, nc)):
                    assert same(a, b), (metric, n, d, p)
                idx, dist = h.search_top1(q[::3])
                assert np.all(dist == 0) and same(y[idx], q[::3])                                 # a projected row finds itself (or its twin) at 0
                if metric == L2 and qb >= 130:                                                    # the routed forms, a caller's threshold of one query
                    h.set_large_batch_mfma(1)
                    fresh.set_large_batch_mfma(1)
                    for a, b in zip(all_searches(h, q, nc), all_searches(fresh, q, nc)):
                        assert same(a, b), ("routed", n, d, p)
                    assert h.mfma_stats()["passes"] > 0


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_pca_top1_matches_the_float64_pipeline(fir):
    rows, q, take = pr.e2e_data()
    basis64, mean64, top64, graded64 = pr.e2e_float64(rows, q, take)
    with fir.Gallery(rows, None, L2, 0) as g:
        s, mean, count = g.scatter(take)
        assert count == int(take.sum())
        vals, vecs = np.linalg.eigh(s)
        basis = vecs[:, ::-1][:, :pr.E2E_P].T.copy()
        with fir.Projection(basis, mean) as proj, g.projected(proj) as h:
            idx, _ = h.search_top1(proj.apply(q))
    # graded against the float64 pipeline run on the device's own basis (an eigenvector's sign or a rotation inside a near-degenerate
    # pair changes no distance; grading on the same basis keeps that out of the comparison) and against the all-numpy pipeline's gaps
    top, graded = pr.e2e_grade(rows, q, basis, mean)
    graded &= graded64
    print("graded", graded.mean(), "agree", np.mean(idx[graded] == top[graded]))
    assert np.mean(~graded) <= 0.05
    assert np.array_equal(idx[graded], top[graded])
    assert np.array_equal(top[graded], top64[graded])


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors(fir):
    L = fir.lib()
    rows = wide_rows(790, 70, 6)
    vp = C.c_void_p
    buf = np.zeros(64 * 64, F64)
    pb = buf.ctypes.data_as(vp)
    cnt = C.c_int64()

    def fails(rc, text):
        assert rc == ERR_ARG, rc
        assert text in L.fir_last_error().decode(), L.fir_last_error()

    with fir.Gallery(rows, None, L2, 0) as g, fir.Gallery(np.zeros((0, 6), F32), None, L2, 0) as empty:
        before = g.memory_bytes()
        fails(L.fir_gallery_feature_stats(None, None, C.byref(cnt), pb, pb, pb, pb), "NULL")
        fails(L.fir_gallery_scatter(None, None, None, pb, None, C.byref(cnt)), "NULL")
        fails(L.fir_gallery_scatter(g._h, None, None, None, None, C.byref(cnt)), "NULL")
        fails(L.fir_gallery_feature_stats(empty._h, None, C.byref(cnt), pb, pb, pb, pb), "empty")
        fails(L.fir_gallery_scatter(empty._h, None, None, pb, None, C.byref(cnt)), "empty")
        h = vp()
        fails(L.fir_projection_create(None, 2, 6, None, 0, C.byref(h)), "NULL")
        fails(L.fir_projection_create(pb, 2, 6, None, 0, None), "NULL")
        fails(L.fir_projection_create(pb, 0, 6, None, 0, C.byref(h)), "p=0")
        fails(L.fir_projection_create(pb, 4097, 6, None, 0, C.byref(h)), "p=4097")
        fails(L.fir_projection_create(pb, 2, 0, None, 0, C.byref(h)), "d=0")
        assert not h.value
        fails(L.fir_projection_info(None, None, None, None), "NULL")
        with fir.Projection(np.ones((2, 5))) as wrong, fir.Projection(np.ones((2, 6))) as right:
            fails(L.fir_gallery_create_projected(g._h, wrong._h, C.byref(h)), "5 features")
            fails(L.fir_gallery_create_projected(empty._h, right._h, C.byref(h)), "empty")
            fails(L.fir_gallery_create_projected(g._h, None, C.byref(h)), "NULL")
            fails(L.fir_gallery_create_projected(g._h, right._h, None), "NULL")
            fails(L.fir_projection_apply(right._h, None, 3, pb), "NULL")
            fails(L.fir_projection_apply(right._h, pb, -1, pb), "m < 0")
            fails(L.fir_projection_apply_dev(right._h, None, 3, pb, None), "NULL")
            assert not h.value
            if fir.device_count() > 1:
                with fir.Projection(np.ones((2, 6)), None, 1) as other:
                    fails(L.fir_gallery_create_projected(g._h, other._h, C.byref(h)), "device")
        assert g.memory_bytes() == before                                                         # nothing was allocated on the way
        big = fir.Gallery(np.zeros((3, 4097), F32), None, L2, 0)
        fails(L.fir_gallery_scatter(big._h, None, None, pb, None, C.byref(cnt)), "4096")
        big.close()
