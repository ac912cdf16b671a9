"""fir_dem_recognize: DirectedEnumeration::recognize (qt_cpp/ann.cpp:416-507, PIVOT build) for a batch of queries in one
call, on the device -- against the REAL reference's outputs (tests/golden), against the oracle's walk on fresh data, and
the tie flag against the numpy restatement of the formulation (tests/dem_walk.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import dem_walk
import golden_cases as gc
import synth

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz"))
ERR_ARG = -1                     # FIR_ERR_ARG, include/fir_amd.h
SELECT_ONE_GROUP_ROWS = 8192     # kSelOneGroupRows, csrc/fir_dem.hip: more candidate positions (n - used) than this and
                                 # several workgroups share a query's select passes
GATHER_DIV = 8                   # kGatherDiv, csrc/fir_dem.hip: candidate distances by gather while Mc < n // GATHER_DIV


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def as_tuples(row, dist, found, calc):
    return list(zip(np.asarray(row).tolist(), bits(dist).tolist(), np.asarray(found).tolist(), np.asarray(calc).tolist()))


def oracle_tuples(oracle, rows, piv, table, thr, m, queries, metric):
    out = [oracle.dem_recognize(rows, piv, table, thr, m, q, metric) for q in queries]
    return as_tuples(*zip(*out))


def restated_ties(g, dem, queries, thr, m):
    """The tie flag per query as tests/dem_walk.py works it out from the device's own pieces."""
    piv, _, _, order = dem.get(want_table=False)
    pd, lik = dem.likelihoods(queries)
    dist = g.range_distances(queries)
    return [dem_walk.formulation(pd[i], piv[: dem.n_used], order, lik[i], dist[i], m, thr)[4] for i in range(len(queries))]


def test_reference_outputs_reproduced_in_one_call(fir, oracle):
    rows, cls, queries = gc.dem_case()
    gp, gt, gth = GOLD["dem/pivots"], GOLD["dem/table"], float(GOLD["dem/threshold"])
    n = len(rows)
    # the reference's inputs themselves: how many (query, count) pairs hang on the order of equal likelihoods?
    order = dem_walk.order_after_pivots(n, gp)
    cpu_ties = {}
    for m in gc.DEM_IMAGE_COUNTS:
        for i, q in enumerate(queries):
            *_, lik = oracle.dem_recognize(rows, gp, gt, 0.0, gp.size, q, gc.L2, want_lik=True)
            dist = oracle.all_distances(rows, q, 0, rows.shape[1], gc.L2)
            cpu_ties[m, i] = dem_walk.formulation(dist[gp], gp, order, lik, dist, m, gth)[4]
    assert sum(cpu_ties.values()) * 10 <= len(cpu_ties), cpu_ties
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, int(gp[0]), gp.size)
        for m in gc.DEM_IMAGE_COUNTS:
            row, dist, found, calc, tie = dem.recognize(queries, gth, m)
            got = as_tuples(row, dist, found, calc)
            want = as_tuples(*(GOLD[f"dem/recognize/{m}/{k}"] for k in ("row", "dist", "found", "calc")))
            under_oracle = oracle_tuples(oracle, rows, gp, gt, gth, m, queries, gc.L2)
            excused = 0
            for i in range(len(queries)):
                assert tie[i] == cpu_ties[m, i], (m, i)
                if tie[i]:                                   # the reference's partial_sort was free to differ: the oracle's rule
                    excused += 1
                    assert got[i] == under_oracle[i], (m, i)
                else:
                    assert got[i] == want[i], (m, i)
            assert excused * 10 <= len(queries), (m, tie)
        dem.close()


FRESH = [(31, 2000, 512, 40, 30, gc.L2), (32, 777, 100, 7, 40, gc.L2), (33, 1500, 256, 30, 12, gc.CHI2), (34, 64, 33, 4, 5, gc.L2)]


@functools.lru_cache(maxsize=None)
def fresh_case(oracle, seed, n, d, ncls, npiv, metric):
    rows = synth.make_gallery(seed, n, d, metric)
    cls = synth.make_labels(n, ncls)
    q, _ = synth.make_queries(seed, rows, 11, metric)        # one full internal batch of 8 and a ragged one
    first = (seed * 7919) % n
    piv, table, mo = oracle.dem_pivot_table(rows, cls, first, npiv, metric)
    used = min(npiv, 32)
    return rows, cls, q, first, piv[:used], table[:used], float(oracle.get_threshold(mo, 0.01))


@pytest.mark.parametrize("seed,n,d,ncls,npiv,metric", FRESH)
def test_matches_oracle_on_fresh_data(fir, oracle, seed, n, d, ncls, npiv, metric):
    rows, cls, q, first, piv, table, mixed = fresh_case(oracle, seed, n, d, ncls, npiv, metric)
    used = len(piv)
    with fir.Gallery(rows, cls, metric, 0) as g:
        dem = fir.Dem(g, first, npiv)
        assert dem.n_used == used
        for m in (used, used + 1, n // 20, n // 2, n):         # gather and dense candidate distances, and no candidates at all
            for thr in (0.0, mixed, 1e9):                      # the full walk, a mix, the first pivot
                row, dist, found, calc, tie = dem.recognize(q, thr, m)
                assert as_tuples(row, dist, found, calc) == oracle_tuples(oracle, rows, piv, table, thr, m, q, metric), (m, thr)
                if thr == 1e9:
                    assert found.all() and (calc == 1).all() and not tie.any()
        dem.close()


@pytest.mark.parametrize("mixed_thr", [False, True])
def test_one_handle_whose_calls_grow_and_shrink(fir, oracle, mixed_thr):
    """One handle, calls of changing size: the host-pointer form's query / result buffers and the candidate scratch grow,
    the candidate distances go from gather (Mc < n // GATHER_DIV) to dense and back, fir_dem_likelihoods runs in between,
    and the last call has no candidates. Every answer is the oracle's walk and, bit for bit, a fresh handle's."""
    n, npiv = 300, 5
    rows, cls, q, first, piv, table, mixed = fresh_case(oracle, 35, n, 64, 10, npiv, gc.L2)
    thr = mixed if mixed_thr else 0.0
    used = len(piv)
    assert used == npiv and 30 < n // GATHER_DIV                # 3 and 30 candidates are gathered, n - used are not

    def fresh(call):
        d = fir.Dem(g, first, npiv)
        try:
            return call(d)
        finally:
            d.close()

    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, first, npiv)
        try:
            for step, (qb, m) in enumerate([(1, used + 3), (11, used + 30), (3, n), (11, used + 3), (2, used)]):
                if step == 2:
                    got, want = dem.likelihoods(q), fresh(lambda d: d.likelihoods(q))
                    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
                got = dem.recognize(q[:qb], thr, m)
                assert as_tuples(*got[:4]) == oracle_tuples(oracle, rows, piv, table, thr, m, q[:qb], gc.L2), (qb, m)
                want = fresh(lambda d: d.recognize(q[:qb], thr, m))
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want)), (qb, m)
        finally:
            dem.close()


def test_index_quirk_and_its_equal_likelihoods(fir, oracle):
    """ann.cpp:431-432 leaves a row twice in the index array (tests/test_gpu_dem.py builds the same case): the two positions
    have one likelihood and one distance. The answers are the position-order walk's, the flag the restatement's."""
    n, d = 300, 64
    rows = synth.make_gallery(41, n, d, gc.L2)
    rows[0] = 0
    rows[0, 0] = 1
    cls = synth.make_labels(n, 10)
    q, _ = synth.make_queries(41, rows, 4, gc.L2)
    piv, table, _ = oracle.dem_pivot_table(rows, cls, 7, 5, gc.L2)
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, 7, 5)
        order = dem.get(want_table=False)[3]
        assert len(set(order.tolist())) < n
        for m in (n, n // 2):
            row, dist, found, calc, tie = dem.recognize(q, 0.0, m)
            assert as_tuples(row, dist, found, calc) == oracle_tuples(oracle, rows, piv, table, 0.0, m, q, gc.L2)
            assert tie.tolist() == restated_ties(g, dem, q, 0.0, m), m
        dem.close()


def test_ties_on_purpose(fir, oracle):
    """16 copies of one row, queries equal to it: the copies have likelihood 0, come first, and the count to check cuts
    through them. Every answer hangs on their order (tie = 1) and is the position-order walk's."""
    n, d = 400, 48
    rows = synth.make_gallery(43, n, d, gc.L2)
    group = np.arange(100, 340, 15)
    assert group.size == 16
    rows[group] = rows[group[0]]
    cls = synth.make_labels(n, 8)
    q = np.tile(rows[group[0]], (3, 1))
    piv, table, _ = oracle.dem_pivot_table(rows, cls, 5, 6, gc.L2)
    assert not set(piv.tolist()) & set(group.tolist())
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, 5, 6)
        for thr in (0.0, 1e-6):                                # the full walk; the exit at the first copy
            m = dem.n_used + 8
            row, dist, found, calc, tie = dem.recognize(q, thr, m)
            assert tie.tolist() == [1, 1, 1]
            assert as_tuples(row, dist, found, calc) == oracle_tuples(oracle, rows, piv, table, thr, m, q, gc.L2)
            assert (row == group[0]).all() and (dist == 0).all() and (calc == (m if thr == 0 else dem.n_used + 1)).all()
            assert tie.tolist() == restated_ties(g, dem, q, thr, m)
        dem.close()


@pytest.mark.parametrize("cnt", [SELECT_ONE_GROUP_ROWS, SELECT_ONE_GROUP_ROWS + 1])
def test_form_boundaries(fir, oracle, cnt):
    """The largest gallery one workgroup per query selects from and the smallest that several share, with the count to
    check on both sides of the gather / dense crossover, and one that cuts through a group of equal likelihoods."""
    npiv, d = 5, 32
    n = cnt + npiv
    rows = synth.make_gallery(47, n, d, gc.L2)
    rows[1000:1040] = rows[1000]
    cls = synth.make_labels(n, 50)
    q, _ = synth.make_queries(47, rows, 9, gc.L2)
    q[0] = rows[1000]
    piv, table, mo = oracle.dem_pivot_table(rows, cls, 11, npiv, gc.L2)
    mixed = float(oracle.get_threshold(mo, 0.01))
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, 11, npiv)
        assert dem.n_used == npiv and dem.n - dem.n_used == cnt
        for m in (npiv + n // GATHER_DIV - 1, npiv + n // GATHER_DIV, npiv + 20):
            for thr in (0.0, mixed):
                row, dist, found, calc, tie = dem.recognize(q, thr, m)
                assert as_tuples(row, dist, found, calc) == oracle_tuples(oracle, rows, piv, table, thr, m, q, gc.L2), (m, thr)
                assert tie.tolist() == restated_ties(g, dem, q, thr, m), (m, thr)
        assert dem.recognize(q, 0.0, npiv + 20)[4][0] == 1       # query 0 = the 40 equal rows, 20 of them checked
        dem.close()


def test_device_pointers_back_to_back_on_another_stream(fir, oracle):
    import torch

    rows, cls, q, first, piv, table, mixed = fresh_case(oracle, *FRESH[0])
    n, qb = len(rows), len(q)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(q).to(dev)
    out = [{k: torch.full((qb,), -7, dtype=torch.float32 if k == "dist" else torch.int32, device=dev)
            for k in ("row", "dist", "found", "calc", "tie")} for _ in range(2)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()                                   # (the library's streams do not wait for torch's)
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, first, 30)
        counts = (n // 20, n)
        for o, m in zip(out, counts):                          # gather then dense, no host synchronisation in between
            dem.recognize_dev(dq.data_ptr(), qb, mixed, m, *(o[k].data_ptr() for k in ("row", "dist", "found", "calc", "tie")),
                              stream=st.cuda_stream)
        g.sync()
        for o, m in zip(out, counts):
            host = dem.recognize(q, mixed, m)
            for k, h in zip(("row", "dist", "found", "calc", "tie"), host):
                assert np.array_equal(o[k].cpu().numpy().view(np.uint32), h.view(np.uint32)), (m, k)
            assert as_tuples(*host[:4]) == oracle_tuples(oracle, rows, piv, table, mixed, m, q, gc.L2)
        # outputs that are not asked for
        only = torch.full((qb,), -7, dtype=torch.int32, device=dev)
        dem.recognize_dev(dq.data_ptr(), qb, mixed, n, only.data_ptr(), None, None, None, None, stream=st.cuda_stream)
        g.sync()
        assert np.array_equal(only.cpu().numpy(), dem.recognize(q, mixed, n)[0])
        dem.close()


def test_argument_errors(fir):
    rows, cls, q, ncls = gc.twd_case(seed=7, n=70, d=256, n_classes=5)
    L = fir.lib()
    vp = ctypes.c_void_p
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        dem = fir.Dem(g, 3, 5)
        qq = np.ascontiguousarray(q[:2], np.float32)
        pq = qq.ctypes.data_as(vp)
        row = np.empty(2, np.int32)
        pr = row.ctypes.data_as(vp)
        bad = [
            (L.fir_dem_recognize, (None, pq, 2, 0.5, 0, pr, None, None, None, None)),
            (L.fir_dem_recognize, (dem._h, pq, 0, 0.5, 0, pr, None, None, None, None)),
            (L.fir_dem_recognize, (dem._h, pq, -3, 0.5, 0, pr, None, None, None, None)),
            (L.fir_dem_recognize, (dem._h, None, 2, 0.5, 0, pr, None, None, None, None)),
            (L.fir_dem_recognize, (dem._h, pq, 2, 0.5, 0, None, None, None, None, None)),
            (L.fir_dem_recognize_dev, (None, pq, 2, 0.5, 0, pr, None, None, None, None, None)),
            (L.fir_dem_recognize_dev, (dem._h, pq, 0, 0.5, 0, pr, None, None, None, None, None)),
            (L.fir_dem_recognize_dev, (dem._h, None, 2, 0.5, 0, pr, None, None, None, None, None)),
            (L.fir_dem_recognize_dev, (dem._h, pq, 2, 0.5, 0, None, None, None, None, None, None)),
        ]
        for fn, args in bad:
            assert fn(*args) == ERR_ARG, args
            assert L.fir_last_error().decode().startswith("fir_dem_recognize: "), args
        first = dem.recognize(qq, 0.5, 0)                      # a valid call still works
        nan_thr = dem.recognize(qq, float("nan"), 0)           # never below a NaN threshold
        assert not nan_thr[2].any() and (nan_thr[3] == 70).all()
        assert all(np.array_equal(a, b) for a, b in zip(first, dem.recognize(qq, 0.5, 0)))
        dem.close()
