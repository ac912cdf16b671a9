"""fir_search_top_classes: the k nearest DISTINCT classes of each query (ConventionalTWDClassifier::recognize keeps the best row of
every class and then the best classes, ImageTesting.cpp:118-122, 141-149). The expected lists are built here from the oracle's
distance vector (oracle.all_distances): per class the first minimum among the rows with dist < 100000, then the k smallest by
(distance, row) -- never from the library's own output. L2 and chi-square must match exactly: classes, rows and distance bits."""
import functools

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

L2, CHI2, KL = 0, 1, 2
NOT_FOUND = np.float32(100000.0)
KEY_NONE = 0xFFFFFFFFFFFFFFFF
FIR_ERR_ARG, FIR_ERR_STATE = -1, -5
SHAPES = [(257, 64), (1000, 256), (65, 100), (1, 7)]
NQ = 9


def bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)


def interleaved(n):
    return synth.make_labels(n, 37), 37                        # i % 37: no two neighbours share a label


def class_major(n, seed=5):
    """Blocks of equal labels of uneven lengths (1 to 150 rows) that cross the 64-row tile edges."""
    rng = np.random.default_rng(seed)
    labels = np.empty(n, np.int32)
    i = c = 0
    while i < n:
        m = int(rng.integers(1, 151))
        labels[i:i + m] = c
        i += m
        c += 1
    return labels, c


LABELS = {"interleaved": interleaved, "class_major": class_major}


@functools.lru_cache(maxsize=None)
def case(orc, n, d, metric, nq=NQ, start=0, end=0):
    """(rows, queries, oracle distances [nq, n]) of one shape, computed once and shared (read-only) by the tests that use it.
    orc: the session's `oracle` fixture."""
    rows = synth.make_gallery(1000 + n + d, n, d, metric)
    q, _ = synth.make_queries(n + d, rows, nq, metric)
    dist = np.stack([orc.all_distances(rows, q[i], start, end or d, metric) for i in range(nq)])
    for a in (rows, q, dist):
        a.setflags(write=False)
    return rows, q, dist


def expected(dist, labels, num_classes, k):
    """dist [nq, n] -> (classes, rows, distances), each [nq, k], padded with -1 / -1 / 100000."""
    nq, n = dist.shape
    cls = np.full((nq, k), -1, np.int32)
    idx = np.full((nq, k), -1, np.int32)
    dd = np.full((nq, k), NOT_FOUND, np.float32)
    for q in range(nq):
        ok = (labels >= 0) & (labels < num_classes) & (dist[q] < NOT_FOUND)            # NaN: the comparison is false
        r = np.nonzero(ok)[0]
        r = r[np.lexsort((r, dist[q][r]))]                                            # ascending (distance, row)
        _, first = np.unique(labels[r], return_index=True)                            # every class's first = its nearest row, lowest index
        w = r[np.sort(first)][:k]                                                     # the class minima in (distance, row) order
        cls[q, :w.size], idx[q, :w.size], dd[q, :w.size] = labels[w], w, dist[q][w]
    return cls, idx, dd


def check(got, exp):
    for g, e, what in zip(got, exp, ("classes", "rows", "distances")):
        if what == "distances":
            assert np.array_equal(bits(g), bits(e)), (what, g, e)
        else:
            assert np.array_equal(g, e), (what, g, e)


@pytest.mark.parametrize("metric", [L2, CHI2])
@pytest.mark.parametrize("labelling", sorted(LABELS))
@pytest.mark.parametrize("n,d", SHAPES)
def test_matches_the_oracle_and_the_top1_search(fir, oracle, n, d, labelling, metric):
    rows, q, dist = case(oracle, n, d, metric)
    labels, nc = LABELS[labelling](n)
    with fir.Gallery(rows, labels, metric, 0) as g:
        for k in (1, 5, 8, 32):
            got = g.search_top_classes(q, nc, k)
            assert [a.shape for a in got] == [(NQ, k)] * 3
            check(got, expected(dist, labels, nc, k))
            # the report names the scan with the class-minimum epilogue (5), 8 queries per tile
            assert f"fir::k_scan<8, {metric}, 8, 5, " in g.last_dispatch()["kernel"]
        i1, d1 = g.search_top1(q)
    assert np.array_equal(got[1][:, 0], i1) and np.array_equal(bits(got[2][:, 0]), bits(d1))


@pytest.mark.parametrize("metric", [L2, CHI2])
@pytest.mark.parametrize("n,d,start,end", [(65, 100, 3, 97), (1000, 256, 64, 256)])
def test_feature_ranges(fir, oracle, n, d, start, end, metric):
    rows, q, dist = case(oracle, n, d, metric, NQ, start, end)
    labels, nc = interleaved(n)
    with fir.Gallery(rows, labels, metric, 0) as g:
        check(g.search_top_classes(q, nc, 5, start, end), expected(dist, labels, nc, 5))


def test_larger_gallery_many_workgroups_and_the_sample_bound(fir, oracle):
    """20000 rows = 313 tiles: many workgroups lower the same table entries, the bound from the row sample is in force, and
    17 queries are three tiles of 8 with one part full."""
    n, d, nc, nq = 20000, 32, 5000, 17
    rows, q, dist = case(oracle, n, d, L2, nq)
    labels = np.random.default_rng(77).permutation(np.arange(n, dtype=np.int32) % nc).astype(np.int32)
    with fir.Gallery(rows, labels, L2, 0) as g:
        for k in (1, 10):
            check(g.search_top_classes(q, nc, k), expected(dist, labels, nc, k))


def test_select_with_every_class_in_one_stride(fir, oracle):
    """The select kernel gathers its candidates from per-thread (stride 256) minima; 1101 classes that are all multiples of 256
    sit in one thread's stride, more of them than the gathered list holds: its other path answers."""
    n, d, k = 1101, 8, 5
    rows = synth.make_gallery(3, n, d, L2)
    q, _ = synth.make_queries(3, rows, 3, L2)
    labels = (np.arange(n, dtype=np.int32) * 256).astype(np.int32)
    dist = np.stack([oracle.all_distances(rows, q[i], 0, d, L2) for i in range(3)])
    with fir.Gallery(rows, labels, L2, 0) as g:
        check(g.search_top_classes(q, 256 * n, k), expected(dist, labels, 256 * n, k))
        check(g.search_top_classes(q, 256 * n, 1), expected(dist, labels, 256 * n, 1))


@pytest.mark.parametrize("metric", [L2, CHI2])
def test_one_class_per_row_is_the_row_search(fir, oracle, metric):
    n, d = 257, 64
    rows, q, dist = case(oracle, n, d, metric)
    labels = np.arange(n, dtype=np.int32)
    with fir.Gallery(rows, labels, metric, 0) as g:
        for k in (1, 3, 8):
            cls, idx, dd = g.search_top_classes(q, n, k)
            ti, td = g.search_topk(q, k)
            assert np.array_equal(idx, ti) and np.array_equal(cls, ti) and np.array_equal(bits(dd), bits(td))
            check((cls, idx, dd), expected(dist, labels, n, k))


def test_padding_and_labels_outside_the_class_range(fir, oracle):
    n, d = 257, 64
    rows, q, dist = case(oracle, n, d, L2)
    labels = (np.arange(n, dtype=np.int32) % 3).astype(np.int32)
    with fir.Gallery(rows, labels, L2, 0) as g:
        cls, idx, dd = g.search_top_classes(q, 10, 8)            # three classes present, eight asked for
    check((cls, idx, dd), expected(dist, labels, 10, 8))
    assert np.all(cls[:, 3:] == -1) and np.all(idx[:, 3:] == -1) and np.all(dd[:, 3:] == NOT_FOUND) and np.all(cls[:, :3] >= 0)
    # a few rows labelled -1 and num_classes + 3, the overall nearest row of query 1 among them: they take no part
    nc = 37
    labels = synth.make_labels(n, nc).copy()
    nearest = int(np.argmin(dist[1]))
    labels[[nearest, 64, 200]] = -1
    labels[[3, 127]] = nc + 3
    with fir.Gallery(rows, labels, L2, 0) as g:
        got = g.search_top_classes(q, nc, 5)
    check(got, expected(dist, labels, nc, 5))
    assert not np.isin(got[1], [nearest, 64, 200, 3, 127]).any()


def test_ties_across_and_within_classes(fir, oracle):
    n, d = 200, 32
    rows = synth.make_gallery(41, n, d, L2).copy()
    labels = synth.make_labels(n, 10).copy()
    rows[150] = rows[20]                       # the same row in two classes (4 and 7)
    labels[20], labels[150] = 4, 7
    rows[133] = rows[61]                       # a duplicate inside one class
    labels[61], labels[133] = 2, 2
    q = np.stack([rows[20], rows[61], rows[150]]).astype(np.float32)
    dist = np.stack([oracle.all_distances(rows, q[i], 0, d, L2) for i in range(3)])
    with fir.Gallery(rows, labels, L2, 0) as g:
        cls, idx, dd = g.search_top_classes(q, 10, 3)
    check((cls, idx, dd), expected(dist, labels, 10, 3))
    assert (cls[0, 0], idx[0, 0], cls[0, 1], idx[0, 1]) == (4, 20, 7, 150)      # equal distances: the lower row's class first
    assert (cls[2, 0], idx[2, 0], cls[2, 1], idx[2, 1]) == (4, 20, 7, 150)
    assert (cls[1, 0], idx[1, 0]) == (2, 61) and 133 not in idx[1]              # within a class: the first row


def test_rows_that_do_not_qualify_are_never_reported(fir, oracle):
    n, d = 300, 32
    rows = synth.make_gallery(23, n, d, L2).copy()
    rows[5, 3] = np.nan
    rows[77] = np.nan
    rows[100] = 1.0e4                          # mean squared distance to a unit query ~1e8 >= 100000
    labels = (np.arange(n, dtype=np.int32) % 10).astype(np.int32)
    labels[[5, 77, 100]] = [10, 11, 12]        # each alone in its class: those classes must come back absent
    q, _ = synth.make_queries(23, rows, 4, L2)
    dist = np.stack([oracle.all_distances(rows, q[i], 0, d, L2) for i in range(4)])
    assert np.all(np.isnan(dist[:, [5, 77]])) and np.all(dist[:, 100] >= NOT_FOUND)
    with fir.Gallery(rows, labels, L2, 0) as g:
        cls, idx, dd = g.search_top_classes(q, 13, 13)
    check((cls, idx, dd), expected(dist, labels, 13, 13))
    assert np.all(cls[:, :10] >= 0) and np.all(cls[:, 10:] == -1) and not np.isin(idx, [5, 77, 100]).any()
    assert not np.isin(cls, [10, 11, 12]).any()


def test_a_second_call_sees_nothing_of_the_first(fir, oracle):
    n, d = 1000, 256
    rows, q, dist = case(oracle, n, d, L2)
    labels, nc = interleaved(n)
    with fir.Gallery(rows, labels, L2, 0) as g:
        check(g.search_top_classes(q, 37, 8), expected(dist, labels, 37, 8))
        q2 = np.ascontiguousarray(q[::-1][:4])                   # other queries, fewer classes (labels 5..36 now outside), other k
        check(g.search_top_classes(q2, 5, 3), expected(dist[::-1][:4], labels, 5, 3))
        check(g.search_top_classes(q, 37, 8), expected(dist, labels, 37, 8))


def test_empty_inputs_and_errors(fir):
    d = 16
    with fir.Gallery(np.zeros((0, d), np.float32), np.zeros(0, np.int32), L2, 0) as g:
        cls, idx, dd = g.search_top_classes(np.ones((2, d), np.float32), 4, 3)
        assert np.all(cls == -1) and np.all(idx == -1) and np.all(dd == NOT_FOUND) and cls.shape == (2, 3)
    rows = np.ones((10, d), np.float32)
    with fir.Gallery(rows, np.arange(10, dtype=np.int32), L2, 0) as g:
        cls, idx, dd = g.search_top_classes(np.zeros((0, d), np.float32), 10, 3)
        assert cls.shape == (0, 3) and idx.shape == (0, 3) and dd.shape == (0, 3)
        for nc, k in ((10, 0), (10, 33), (0, 3), ((1 << 24) + 1, 3)):
            with pytest.raises(fir.FirError) as e:
                g.search_top_classes(np.zeros((2, d), np.float32), nc, k)
            assert e.value.code == FIR_ERR_ARG
        with pytest.raises(fir.FirError) as e:
            g.search_top_classes(np.zeros((2, d), np.float32), 10, 3, 8, 4)
        assert e.value.code == FIR_ERR_ARG
    with fir.Gallery(rows, None, L2, 0) as g:
        with pytest.raises(fir.FirError) as e:
            g.search_top_classes(np.zeros((2, d), np.float32), 10, 3)
        assert e.value.code == FIR_ERR_STATE


def test_device_form_on_a_callers_stream_after_a_call_on_another(fir, oracle):
    n, d, k = 1000, 256, 5
    rows, q, dist = case(oracle, n, d, L2)
    labels, nc = interleaved(n)
    dev = torch.device("cuda", 0)
    with fir.Gallery(rows, labels, L2, 0) as g:
        hc, hi, hd = g.search_top_classes(q, nc, k)
        dq = torch.from_numpy(q).to(dev)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        k1 = torch.zeros(NQ, dtype=torch.int64, device=dev)
        keys = torch.full((NQ * k + 8,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        cls = torch.full((NQ * k + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g.search_top1_keys_dev(dq.data_ptr(), NQ, k1.data_ptr(), stream=s1.cuda_stream)         # no host synchronisation in between
        g.search_top_classes_keys_dev(dq.data_ptr(), NQ, nc, k, keys.data_ptr(), cls.data_ptr(), stream=s2.cuda_stream)
        s2.synchronize()
        s1.synchronize()
    assert torch.all(keys[NQ * k:] == 0x5A5A5A5A) and torch.all(cls[NQ * k:] == 0x5A5A5A5A)      # nothing past the end
    di, dd = fir.keys_unpack(keys[:NQ * k].cpu().numpy().view(np.uint64).reshape(NQ, k))
    assert np.array_equal(di, hi) and np.array_equal(bits(dd), bits(hd))
    assert np.array_equal(cls[:NQ * k].cpu().numpy().reshape(NQ, k), hc)
    check((hc, hi, hd), expected(dist, labels, nc, k))
    assert np.array_equal(fir.keys_unpack(k1.cpu().numpy().view(np.uint64))[0], hi[:, 0])


def test_row_shards_merge_to_the_unsplit_answer(fir, oracle):
    n, d, k = 1000, 256, 8
    rows, q, dist = case(oracle, n, d, L2)
    labels, nc = class_major(n)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(q).to(dev)

    def keys_of(r, lab, offset):
        keys = torch.zeros((NQ, k), dtype=torch.int64, device=dev)
        cls = torch.zeros((NQ, k), dtype=torch.int32, device=dev)
        with fir.Gallery(r, lab, L2, 0) as g:
            g.set_row_offset(offset)
            g.search_top_classes_keys_dev(dq.data_ptr(), NQ, nc, k, keys.data_ptr(), cls.data_ptr())
            g.sync()
        return keys.cpu().numpy().view(np.uint64), cls.cpu().numpy()

    whole = keys_of(rows, labels, 0)
    cuts = [0, 300, 333, n]                                   # the class blocks straddle the cuts
    parts = [keys_of(rows[a:b], labels[a:b], a) for a, b in zip(cuts[:-1], cuts[1:])]
    mk, mc = fir.class_keys_merge(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), k)
    assert np.array_equal(mk, whole[0]) and np.array_equal(mc, whole[1])
    idx, dd = fir.keys_unpack(mk)
    check((mc, idx, dd), expected(dist, labels, nc, k))


@pytest.mark.parametrize("n,d,nc", [(257, 64, 10), (1000, 256, 37)])
def test_kl_within_the_repository_bar(fir, oracle, n, d, nc):
    """KL is not bit-exact here (test_gpu_parity.py: 1e-5 relative). Every reported distance is within 1e-5 relative of the oracle's
    class minimum at that rank and the reported row belongs to the reported class; the class must be the oracle's wherever the
    oracle's class minima at the neighbouring ranks differ by more than 2e-5 relative. Slots left out for that reason are counted:
    more than 1 in 20 fails. (With the oracle's float32 distances both inputs leave out 0 of 72.)"""
    k = 8
    rows, q, dist = case(oracle, n, d, KL)
    labels = ((np.arange(n, dtype=np.int64) * 7919) % nc).astype(np.int32)
    ecls, eidx, edd = expected(dist, labels, nc, k + 1)                                  # one rank further: the neighbour of the last slot
    with fir.Gallery(rows, labels, KL, 0) as g:
        cls, idx, dd = g.search_top_classes(q, nc, k)
    assert np.all(idx >= 0) and np.array_equal(labels[idx], cls)
    e = edd[:, :k].astype(np.float64)
    rel = np.abs(dd.astype(np.float64) - e) / np.abs(e)
    print("KL: largest relative distance error", rel.max())
    assert np.all(rel <= 1e-5), rel.max()
    left_out = 0
    for qi in range(NQ):
        for r in range(k):
            near = [edd[qi, j] for j in (r - 1, r + 1) if 0 <= j < k + 1 and eidx[qi, j] >= 0]
            if any(abs(float(x) - float(edd[qi, r])) <= 2e-5 * abs(float(edd[qi, r])) for x in near):
                left_out += 1
                continue
            assert cls[qi, r] == ecls[qi, r], (qi, r, cls[qi], ecls[qi])
    print("KL: slots left out", left_out, "of", NQ * k)
    assert left_out * 20 <= NQ * k, left_out
