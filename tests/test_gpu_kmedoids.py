"""fir_cls_kmedoids on the device: PNNwithClusteringClassifier::train (classification.cpp:320-388) for every class of a handle.
Medoids, counts and padding equal the oracle's 100-step algorithm class by class; the steps computed equal those of the
numpy restatement of the table formulation (tests/kmedoids_ref.py); the medoid model reproduces the REAL reference's
recorded predictions (tests/golden)."""
import os

import numpy as np
import pytest

import golden_cases as gc
import kmedoids_ref as kr
from test_kmedoids_formulation import CASES, VARIANTS, extra_inputs, variant

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz"))
FIR_ERR_ARG, FIR_ERR_NOMEM = -1, -3
SIZES = [3, 5, 6, 30, 0, 63, 64, 65, 130, 1]          # class boundaries in the middle of 64-row tiles, an empty class


def by_sizes(x, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cls = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return x[: off[-1]], cls, off


def oracle_train(oracle, rows, off, k):
    nc = len(off) - 1
    out = np.full((nc, k), -1, np.int32)
    count = np.zeros(nc, np.int32)
    for i in range(nc):
        if off[i + 1] > off[i]:
            med = oracle.pnn_cluster_class(rows[off[i]:off[i + 1]], k)
            count[i] = med.size
            out[i, : med.size] = off[i] + med
    return out, count


def model(fir, rows, cls, nc, avg=None):
    return fir.ClsModel(rows, cls, nc, np.zeros(rows.shape[1]) if avg is None else avg, 0)


def one_class(fir, rows, k, steps=0):
    with model(fir, rows, np.zeros(rows.shape[0], np.int32), 1) as m:
        got, count, run = m.kmedoids(k, steps)
    return got[0], int(count[0]), int(run[0])


@pytest.mark.parametrize("d", [96, 7, 512])
def test_mixed_class_sizes_equal_the_oracle_class_by_class(fir, oracle, d):
    x, _, _ = gc.cls_case(11, sum(SIZES), d, n_classes=3)
    rows, cls, off = by_sizes(x, SIZES)
    tables = [kr.pair_table(rows[off[i]:off[i + 1]]) for i in range(len(SIZES))]
    with model(fir, rows, cls, len(SIZES)) as m:
        for k in (1, 2, 5, 16):
            got, count, run = m.kmedoids(k)
            want, want_count = oracle_train(oracle, rows, off, k)
            assert np.array_equal(got, want), k
            assert np.array_equal(count, want_count), k
            assert np.array_equal(run, [kr.cluster_table(t, k)[1] for t in tables]), k
            assert np.all(run[np.array(SIZES) <= k] == 0) and np.all(run[np.array(SIZES) > k] >= 1)


@pytest.mark.parametrize("name", VARIANTS[1:])
def test_duplicate_and_nan_rows_equal_the_oracle(fir, oracle, name):
    inputs = [(variant(gc.cls_case(seed, n, d, n_classes=3)[0], name), k) for seed, n, d, k in CASES]
    if name == VARIANTS[1]:
        inputs.append(extra_inputs()[1][1:])                                       # exact ties
    for r, k in inputs:
        want = oracle.pnn_cluster_class(r, k)
        got, count, run = one_class(fir, r, k)
        assert count == want.size and np.array_equal(got[:count], want) and np.all(got[count:] == -1), (name, r.shape, k)
        assert run == kr.cluster_class(r, k)[1]


def test_the_step_bound_is_honoured(fir):
    _, a, k = extra_inputs()[0]
    table = kr.pair_table(a)
    with model(fir, a, np.zeros(a.shape[0], np.int32), 1) as m:
        for steps in range(1, 8):
            got, count, run = m.kmedoids(k, steps)
            want, _ = kr.cluster_table(table, k, steps, early=False)               # exactly that many steps
            assert np.array_equal(got[0, : count[0]], want) and np.all(got[0, count[0]:] == -1), steps
            assert run[0] == kr.cluster_table(table, k, steps)[1] == min(steps, 6), steps


def test_a_class_larger_than_the_workgroup(fir, oracle):
    sizes = [30, 1500, 30]
    x, _, _ = gc.cls_case(12, sum(sizes), 16, n_classes=3)
    rows, cls, off = by_sizes(x, sizes)
    with model(fir, rows, cls, 3) as m:
        got, count, run = m.kmedoids(4)
    want, want_count = oracle_train(oracle, rows, off, 4)
    assert np.array_equal(got, want) and np.array_equal(count, want_count)
    assert np.all(run >= 1) and np.all(run <= 100)


def test_scratch_bound_splits_the_classes_into_groups(fir, oracle):
    x, _, _ = gc.cls_case(11, sum(SIZES), 96, n_classes=3)
    rows, cls, off = by_sizes(x, SIZES)
    want, want_count = oracle_train(oracle, rows, off, 5)
    with model(fir, rows, cls, len(SIZES)) as m:
        free = m.kmedoids(5)
        tight = m.kmedoids(5, 0, 130 * 130 * 8)                                    # the 130-row table fits, and only alone
        with pytest.raises(fir.FirError) as e:
            m.kmedoids(5, 0, 100000)
        assert e.value.code == FIR_ERR_NOMEM
        again = m.kmedoids(5)
    for got in (free, tight, again):
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want_count)
        assert np.array_equal(got[2], free[2])


def test_a_handle_with_a_mean_clusters_the_centred_rows(fir):
    x, _, _ = gc.cls_case(13, 100, 33, n_classes=3)
    rows, cls, off = by_sizes(x, [40, 60])
    avg = rows.mean(axis=0)
    with model(fir, rows, cls, 2, avg) as m:
        got = m.kmedoids(5)
        sums = m.distance_sums(rows)
    centred = rows - avg
    want = kr.cluster_train(centred, off, 5)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    for i in range(2):
        t = kr.pair_table(centred[off[i]:off[i + 1]])
        dev = sums[off[i]:off[i + 1], off[i]:off[i + 1]] / np.float64(33)
        assert np.array_equal(t.view(np.uint64), dev.view(np.uint64))


@pytest.mark.parametrize("k", [5, 2])
def test_medoid_model_reproduces_the_reference_predictions(fir, k):
    x, _, ncls = gc.cls_case()
    train, tcls, test = GOLD["cls/train"], GOLD["cls/train_class"], GOLD["cls/test"]
    tr = x[train]
    with model(fir, tr, tcls, ncls) as m:
        rows, count, _ = m.kmedoids(k)
    keep = np.concatenate([rows[i, : count[i]] for i in range(ncls)])
    with fir.ClsModel(tr[keep], tcls[keep], ncls, GOLD["cls/avg"], 0) as med:
        med.set_total_training_size(len(train))
        best, _ = med.pnn_predict(x[test])
    assert np.array_equal(best, GOLD[f"cls/pnn_clust{k}"])


def test_bad_arguments(fir):
    import ctypes as C

    x, _, _ = gc.cls_case(14, 40, 8, n_classes=3)
    with model(fir, x, np.zeros(40, np.int32), 1) as m:
        for k, steps in ((0, 0), (257, 0), (5, -1)):
            with pytest.raises(fir.FirError) as e:
                m.kmedoids(k, steps)
            assert e.value.code == FIR_ERR_ARG, (k, steps)
        with pytest.raises(fir.FirError) as e:
            m.kmedoids(5, 0, -1)
        assert e.value.code == FIR_ERR_ARG
        count = np.empty(1, np.int32)
        assert fir.capi.lib().fir_cls_kmedoids(m._h, 5, 0, 0, None, count.ctypes.data_as(C.c_void_p), None) == FIR_ERR_ARG
        rows, count, _ = m.kmedoids(5)
        assert count[0] == 5 and np.all(rows >= 0)
    big = np.zeros((32769, 2))
    with model(fir, big, np.zeros(32769, np.int32), 1) as m:
        with pytest.raises(fir.FirError) as e:
            m.kmedoids(5)
        assert e.value.code == FIR_ERR_ARG


def test_no_side_effects_on_the_handle(fir):
    x, lab, ncls = gc.cls_case(15, 300, 40, n_classes=4)
    order = np.argsort(lab, kind="stable")
    rows, cls = x[order], lab[order]
    q = x[::7] + 0.01
    with model(fir, rows, cls, ncls, rows.mean(axis=0)) as m:
        before, scores_before = m.pnn_predict(q)
        first = m.kmedoids(3)
        second = m.kmedoids(3)
        after, scores_after = m.pnn_predict(q)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert np.array_equal(before, after) and np.array_equal(scores_before.view(np.uint64), scores_after.view(np.uint64))
