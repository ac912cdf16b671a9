"""fir_search_top1_other_class, the gallery self-join and the false-accept threshold without a GPU: other_class_ref, the numpy
restatement the device tests grade against, pinned to the oracle -- oracle.all_distances for the distance bits (three metrics),
oracle.get_threshold for the threshold bits -- and to the reference's own way of writing each step (a running strict minimum; sort a
row's distances and take the first entry of another class). The lemma of the routed form (the nearest row of another class is among
the two nearest distinct classes) is checked on data with duplicated rows within and across classes, one-class galleries, and an
excluded class that is absent, ranked first, or ranked second."""
import numpy as np
import pytest

import knn_select_ref as ks
import other_class_ref as ref
import synth

F32 = np.float32
I32 = np.int32


def matrix(oracle, rows, queries, start, end, metric):
    return np.stack([oracle.all_distances(rows, q, start, end, metric) for q in queries])


def case(seed, n, d, metric, classes):
    rows = synth.make_gallery(seed, n, d, metric)
    # duplicated rows inside a class and across classes
    if n > 12:
        rows[7] = rows[2]
        rows[n - 1] = rows[2]
        rows[11] = rows[5]
    labels = (synth.splitmix64(np.arange(n, dtype=np.uint64), seed + 1) % np.uint64(classes)).astype(I32)
    if n > 12:
        labels[7] = labels[2]                      # the copy at row 7 shares row 2's class ...
        labels[n - 1] = (labels[2] + 1) % classes  # ... the one at the last row does not (one class: it does)
    return rows, labels


@pytest.mark.parametrize("metric", (0, 1, 2))
def test_masked_first_minimum_keys_against_the_reference_loop(oracle, metric):
    n, d = 90, 24
    rows, labels = case(31 + metric, n, d, metric, 5)
    q, _ = synth.make_queries(33, rows, 9, metric)
    q[1] = rows[2]                                 # exact duplicates: rows 2, 7 (same class) and n - 1 (another)
    for start, end in ((0, d), (3, 17), (4, 5)):
        dist = matrix(oracle, rows, q, start, end, metric)
        for exclude in (labels[2], (labels[2] + 1) % 5, 77, -1):
            keys = ref.expected_keys(dist, labels, exclude)
            for i in range(q.shape[0]):
                bi, bd = ref.first_minimum(dist[i], labels, exclude)
                idx, dd = ks.unpack(keys[i:i + 1])
                assert idx[0] == bi and dd.view(np.uint32)[0] == F32(bd).view(np.uint32), (metric, start, end, exclude, i)
        # the query that is row 2 itself: own class excluded -> the copy in the other class; that class excluded -> row 2, the lowest
        assert ks.unpack(ref.expected_keys(dist[1:2], labels, labels[2]))[0][0] == n - 1
        assert ks.unpack(ref.expected_keys(dist[1:2], labels, labels[n - 1]))[0][0] == 2
        # an exclusion no row carries: plain top-1
        assert np.array_equal(ref.expected_keys(dist, labels, 77), np.array([ks.expected_keys(r, 1)[0] for r in dist]))


def test_hand_made_rows_nan_cutoff_offsets_and_extreme_labels():
    row = np.array([3.0, 1.0, 1.0, np.nan, 100000.0, 0.5, -0.0, 0.0, 2.0e5], F32)
    labels = np.array([0, 1, 2, 3, 4, np.iinfo(I32).min, np.iinfo(I32).max, -1, 9], I32)
    want = {0: 6, 1: 6, np.iinfo(I32).max: 7, -1: 6, np.iinfo(I32).min: 6, 12345: 6}
    for ex, idx in want.items():
        for off in (0, 1 << 20):
            k = ref.expected_keys(row, labels, ex, off)
            assert ks.unpack(k)[0][0] == idx + off, (ex, off)
    # -0.0 packs as +0.0: rows 6 and 7 tie and the lower row wins unless it is excluded
    assert ks.unpack(ref.expected_keys(row, labels, np.iinfo(I32).max))[1].view(np.uint32)[0] == 0
    # NaN, the cut-off and anything above never qualify: alone they give FIR_KEY_NONE
    assert ref.expected_keys(row[[3, 4, 8]], labels[[3, 4, 8]], 0)[0] == ref.KEY_NONE
    # everything excluded
    assert ref.expected_keys(np.ones(4, F32), np.full(4, 5, I32), 5)[0] == ref.KEY_NONE
    assert ref.expected_keys(np.zeros((2, 0), F32), np.zeros(0, I32), 5).tolist() == [ref.KEY_NONE] * 2
    # one exclusion per query
    k = ref.expected_keys(np.stack([row, row]), labels, [np.iinfo(I32).max, 0])
    assert ks.unpack(k)[0].tolist() == [7, 6]


@pytest.mark.parametrize("metric", (0, 1, 2))
def test_self_join_statistic_is_the_references_sort_and_scan(oracle, metric):
    n, d = 120, 16
    rows, labels = case(51 + metric, n, d, metric, 7)
    dist = matrix(oracle, rows, rows, 0, d, metric)                       # dist[i, j] = feature_distance(row i, row j): row i is the query
    keys = ref.self_join_keys(dist, labels)
    assert (keys != ref.KEY_NONE).all()
    idx, dd = ks.unpack(keys)
    assert (labels[idx] != labels).all() and (idx != np.arange(n)).all()
    want = ref.other_class_dists_reference_way(dist, labels)
    assert np.array_equal(dd.view(np.uint32), (want + F32(0.0)).view(np.uint32))
    if metric != 2:
        # L2 and chi-square: the reference's argument order, distance(row j, row i), gives the same bits
        assert np.array_equal(dist.view(np.uint32), np.ascontiguousarray(dist.T).view(np.uint32))
    # a window of rows, as fir_gallery_other_class_keys_dev(row0 = 60, m = 50) sees it
    assert np.array_equal(ref.self_join_keys(dist[60:110], labels, row0=60), keys[60:110])
    # one class: nobody has a row of another class
    assert (ref.self_join_keys(dist, np.full(n, 3, I32)) == ref.KEY_NONE).all()
    assert ref.other_class_dists_reference_way(dist, np.full(n, 3, I32)).shape == (0,)


def test_threshold_bits_are_get_thresholds(oracle):
    n, d = 300, 16
    rows, labels = case(61, n, d, 0, 11)
    labels[labels == 4] = 3
    dist = matrix(oracle, rows, rows, 0, d, 0)
    dists = ref.keys_to_dists(ref.self_join_keys(dist, labels))
    assert dists.shape[0] == n
    for rate in (0.0, 0.01, 0.05, 0.5, 0.999):
        thr, lo, hi, size, ind = ref.threshold(dists, rate)
        assert size == n and ind == int(F32(n) * F32(rate))
        assert F32(thr).view(np.uint32) == oracle.get_threshold(dists, rate).view(np.uint32), rate
        assert lo == dists.min() and hi == dists.max() and lo <= thr <= hi
    assert ref.threshold(dists, 0.0)[0] == dists.min()
    # the float product: 10 * 0.7f = 6.99999988 rounds to 7.0f (the double product of the same two numbers truncates to 6)
    assert ref.threshold(np.arange(10, dtype=F32), 0.7)[4] == 7 and int(10.0 * float(F32(0.7))) == 6
    assert F32(7.0).view(np.uint32) == oracle.get_threshold(np.arange(10, dtype=F32), 0.7).view(np.uint32)
    # a rate of 1.0 indexes past the end, NaN and negative rates index nowhere, an empty statistic has no threshold
    assert ref.threshold(dists, 1.0)[0] is None and ref.threshold(dists, 1.0)[4] == n
    assert ref.threshold(dists, np.nan)[0] is None and ref.threshold(dists, -0.5)[0] is None
    assert ref.threshold(np.zeros(0, F32), 0.5) == (None, None, None, 0, None)
    # rows without a row of another class are not counted
    keys = np.array([ref.KEY_NONE, ks.all_keys(np.array([2.0], F32))[0], ref.KEY_NONE, ks.all_keys(np.array([1.0], F32))[0]], np.uint64)
    assert ref.keys_to_dists(keys).tolist() == [2.0, 1.0]


@pytest.mark.parametrize("classes", (1, 2, 9))
def test_lemma_nearest_other_class_row_is_among_the_two_nearest_classes(oracle, classes):
    n, d = 150, 12
    rows, labels = case(71 + classes, n, d, 0, classes)
    q, _ = synth.make_queries(73, rows, 12, 0)
    q[0] = rows[2]
    q[1] = rows[5]
    dist = matrix(oracle, rows, q, 0, d, 0)
    dist[3, 10:20] = np.nan
    dist[4, :] = F32(100000.0)                                             # a query nothing qualifies for
    for off in (0, 1 << 20):
        two = [ref.two_nearest_classes(r, labels, classes, off) for r in dist]
        keys2 = np.stack([k for k, _ in two])
        cls2 = np.stack([c for _, c in two])
        first, second = cls2[:, 0].copy(), cls2[:, 1].copy()
        for name, exclude in (("absent", np.full(12, classes + 5, I32)), ("first", first), ("second", second),
                              ("own class of a gallery row", np.resize(labels[:12], 12))):
            got = ref.pick_of_two(keys2, cls2, exclude)
            want = ref.expected_keys(dist, labels, exclude, off)
            assert np.array_equal(got, want), (classes, off, name)
        # absent: rank 1; rank 1 excluded: rank 2 (FIR_KEY_NONE in a one-class gallery)
        assert np.array_equal(ref.pick_of_two(keys2, cls2, np.full(12, classes + 5, I32)), keys2[:, 0])
        assert np.array_equal(ref.pick_of_two(keys2, cls2, first)[first >= 0], keys2[first >= 0, 1])
        assert ref.pick_of_two(keys2, cls2, first)[4] == ref.KEY_NONE
        if classes == 1:
            assert (keys2[:, 1] == ref.KEY_NONE).all()


def test_bound_and_declared_symbols():
    import os
    import re

    import __graft_entry__ as ge

    pkg = ge.load_package()
    sigs = {name: args for name, _, args in pkg.capi.SYMBOLS}
    names = (("fir_search_top1_other_class", 8), ("fir_search_top1_other_class_keys_dev", 8), ("fir_gallery_other_class_keys_dev", 7),
             ("fir_gallery_other_class", 5), ("fir_gallery_far_threshold", 8), ("fir_sharded_search_top1_other_class", 8))
    for name, nargs in names:
        assert name in sigs and len(sigs[name]) == nargs, name
        assert hasattr(pkg.lib(), name)
    for cls, meth in ((pkg.Gallery, "search_top1_other_class"), (pkg.Gallery, "search_top1_other_class_keys_dev"), (pkg.Gallery, "other_class"),
                      (pkg.Gallery, "other_class_keys_dev"), (pkg.Gallery, "far_threshold"), (pkg.ShardedGallery, "search_top1_other_class")):
        assert callable(getattr(cls, meth))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fir_amd.h")).read()
    for name, _ in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
