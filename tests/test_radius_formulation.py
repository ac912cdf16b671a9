"""The matrix-core form of fir_search_radius (csrc/fir_gemm_knn.h: k_gemm_rerank_radius), checked without a GPU on the float64
emulation of the fp16 proxies (gemm_f16_form.Form) with knn_gemm_ref.tau_of, the restatement of k_gemm_tau_class: the query's radius
is the bound, no row sample. Over every shape tests/test_gpu_radius_gemm.py runs through the matrix cores, with the radius at
nextafter of the r-th smallest reference distance,
  every row inside the radius (float32's rounding of the reference distance allowed for, as knn_gemm_ref.formulation does) has a
      proxy below tau: it is appended,
  no list exceeds 4096 entries, and
  the certificate's lower bound (|q|^2 + tau) / d - E lies above the radius,
so the device test's "no query went to the store + count + select form" is a condition the formulation alone can satisfy.
radius_ref.expected, the contract both device tests grade against, is checked here against a brute-force filter on hand-made rows."""
import numpy as np
import pytest

import gemm_f16_form as gf
import knn_gemm_ref as kg
import knn_select_ref as ks
import radius_ref as ref

F32 = np.float32
INF = F32(np.inf)

# (n, d_row, end, qb, ranks): tests/test_gpu_radius_gemm.py runs the same list
SHAPES = [
    (3000, 64, 0, 130, (1, 9, 256, 1000)),
    (5000, 512, 0, 70, (1, 33, 256)),
    (333, 100, 0, 40, (1, 256, 333)),
    (3000, 512, 64, 70, (1, 33)),            # a feature prefix
    (66000, 128, 0, 200, (1, 64, 256, 1000)),
]


def radius_at_rank(rows, q, r, end=0):
    """[qb] float32: nextafter of the exact r-th smallest reference distance over ALL rows (knn_gemm_ref.sample_bound with the sample
    divisor 1: the sample is the gallery)."""
    at = kg.sample_bound(rows, q, r, end, div=1)
    assert (at < kg.NOT_FOUND).all()
    return np.nextafter(at, INF)


def formulation(rows, q, radius, end=0, chunk=32):
    form = gf.Form(rows, 2, end)
    q = np.asarray(q, F32)
    out = {"count": [], "inside": [], "listed_all": [], "margin": []}
    for c0 in range(0, q.shape[0], chunk):
        p_emu, p_true, _, qn = form.emulate(q[c0:c0 + chunk])
        r = radius[c0:c0 + chunk]
        tau = kg.tau_of(form.e_rel, r, form.d, qn.astype(F32), form.gmax).astype(np.float64)
        dist = (qn[:, None] + p_true) / form.d
        near = dist <= r.astype(np.float64)[:, None] * (1.0 + 2.0 * (form.d + 3) * gf.U)
        listed = p_emu < tau[:, None]
        ed = gf.e_d_of(form.e_rel, qn.astype(F32), form.gmax).astype(np.float64)
        lower = (qn.astype(F32).astype(np.float64) + tau) / form.d - ed / form.d
        out["count"].append(listed.sum(axis=1))
        out["inside"].append(near.sum(axis=1))
        out["listed_all"].append((~near | listed).all(axis=1))
        out["margin"].append(np.where(listed.all(axis=1), np.inf, lower - r.astype(np.float64)))      # every row re-ranked: certified
    return {k: np.concatenate(v) for k, v in out.items()}


@pytest.mark.parametrize("n,d,end,qb,ranks", SHAPES)
def test_the_device_shapes_need_no_exact_form(n, d, end, qb, ranks):
    rows, q = kg.case(n + d, n, d, qb)
    most = 0
    for r in ranks:
        f = formulation(rows, q, radius_at_rank(rows, q, r, end), end)
        assert f["listed_all"].all(), (n, d, end, r, np.flatnonzero(~f["listed_all"])[:8])
        assert f["count"].max() <= gf.K_LIST_CAP, (n, d, end, r, int(f["count"].max()))
        assert (f["margin"] > 0).all(), (n, d, end, r, float(f["margin"].min()))
        assert (f["inside"] >= r).all() and (f["count"] >= f["inside"]).all()
        most = max(most, int(f["count"].max()))
    print("radius formulation", (n, d, end, qb), "ranks", ranks, "most rows below tau", most)


def brute(dist_row, radius, max_results, row_offset):
    """the contract, element by element in Python floats made of float32 values"""
    keys = []
    for i, v in enumerate(np.asarray(dist_row, F32)):
        if v < F32(radius) and v < F32(100000.0):                  # (both False for NaN)
            keys.append((int(ks.orderable(np.array([v], F32))[0]) << 32) | ((i + row_offset) & 0xFFFFFFFF))
    keys.sort()
    out = keys[:max_results] + [int(ref.KEY_NONE)] * (max_results - min(len(keys), max_results))
    return len(keys), np.array(out, np.uint64)


def test_expected_is_the_contract_on_hand_made_rows():
    row = np.array([3.0, 1.0, 1.0, np.nan, 100000.0, 0.5, -0.0, 0.0, 99999.99, np.inf, 1.0, -1.5, 2.0e5], F32)
    radii = [0.0, -0.0, -1.0, -2.0, np.nan, 0.5, np.nextafter(F32(0.5), INF), 1.0, np.nextafter(F32(1.0), INF), 3.0, 99999.99, 100000.0,
             1.0e5 + 1, 3.0e38, np.inf, -np.inf, np.nextafter(F32(0.0), INF)]
    for radius in radii:
        for m in (0, 1, 2, 3, 5, 13, 20):
            for off in (0, 10, 1 << 20):
                c, k = ref.expected(row, radius, m, off)
                bc, bk = brute(row, radius, m, off)
                assert c == bc and np.array_equal(k, bk), (radius, m, off)
    # a few by hand: ties go by row, -0.0 is +0.0, the compare is strict, NaN and the cut-off never qualify
    c, k = ref.expected(row, 1.0, 5, 10)
    assert c == 4 and ks.unpack(k)[0].tolist() == [21, 16, 17, 15, -1]
    c, k = ref.expected(row, np.nextafter(F32(1.0), INF), 5, 0)
    assert c == 7 and ks.unpack(k)[0].tolist() == [11, 6, 7, 5, 1]
    assert ks.unpack(k)[1].tolist() == [-1.5, 0.0, 0.0, 0.5, 1.0]
    c, k = ref.expected(row, np.inf, 13, 0)
    assert c == 9 and np.array_equal(k, ks.expected_keys(row, 13))                  # an infinite radius: fir_search_knn's keys
    assert ref.expected(row, np.nan, 3, 0)[0] == 0 and ref.expected(row, 0.0, 3, 0)[0] == 1      # (-1.5 < 0)
    c, k = ref.expected(np.zeros(0, F32), np.inf, 2, 0)
    assert c == 0 and np.all(k == ref.KEY_NONE)
    cb, kb = ref.expected_batch(np.stack([row, row]), [1.0, np.inf], 3)
    assert cb.tolist() == [4, 9] and np.array_equal(kb[0], ref.expected(row, 1.0, 3)[1])


def test_bound_and_declared_symbols():
    import os
    import re

    import __graft_entry__ as ge

    pkg = ge.load_package()
    sigs = {name: args for name, _, args in pkg.capi.SYMBOLS}
    for name, nargs in (("fir_search_radius", 10), ("fir_search_radius_keys_dev", 10), ("fir_gemm_search_radius_keys_dev", 8), ("fir_sharded_search_radius", 10)):
        assert name in sigs and len(sigs[name]) == nargs, name
        assert hasattr(pkg.lib(), name)
    for cls, meth in ((pkg.Gallery, "search_radius"), (pkg.Gallery, "search_radius_keys_dev"), (pkg.GemmSearch, "search_radius_keys_dev"),
                      (pkg.ShardedGallery, "search_radius")):
        assert callable(getattr(cls, meth))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fir_amd.h")).read()
    for name in ("fir_search_radius", "fir_search_radius_keys_dev", "fir_gemm_search_radius_keys_dev", "fir_sharded_search_radius"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
