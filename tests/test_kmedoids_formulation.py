"""The table formulation of PNNwithClusteringClassifier::train that fir_cls_kmedoids implements (tests/kmedoids_ref.py) is the
oracle's 100-step algorithm (oracle.c, classification.cpp:320-388): same medoids on plain, duplicate-row, NaN and tied
inputs; stopping at the fixed point changes nothing; and the library declares, exports and binds the entry point."""
import ctypes

import numpy as np
import pytest

import golden_cases as gc
import kmedoids_ref as kr

CASES = [(1, 6, 7, 5), (2, 30, 96, 5), (3, 30, 96, 2), (4, 65, 33, 5), (5, 130, 16, 8), (6, 200, 8, 3), (7, 150, 4, 16)]
VARIANTS = ("plain", "duplicate", "nan_medoid", "nan_tail_and_duplicate")


def variant(rows, name):
    r = np.array(rows, np.float64)
    n, d = r.shape
    if name == "duplicate":
        r[1] = r[0]                       # empties cluster 1
    elif name == "nan_medoid":
        r[0, 0] = np.nan
    elif name == "nan_tail_and_duplicate":
        r[n - 1, d - 1] = np.nan
        r[3] = r[2]
    return r


def extra_inputs():
    rng = np.random.default_rng(0)
    a = rng.random((300, 2))
    b = np.round(rng.random((120, 3)) * 4) / 4
    return [("six_steps", a, 12), ("exact_ties", b, 6)]


def all_inputs():
    out = []
    for seed, n, d, k in CASES:
        x, _, _ = gc.cls_case(seed, n, d, n_classes=3)
        for v in VARIANTS:
            out.append((f"{seed}-{n}x{d}-K{k}-{v}", variant(x, v), k))
    return out + extra_inputs()


@pytest.mark.parametrize("seed,n,d,k", CASES)
@pytest.mark.parametrize("name", VARIANTS)
def test_restatement_equals_the_oracle_at_100_steps(oracle, seed, n, d, k, name):
    x, _, _ = gc.cls_case(seed, n, d, n_classes=3)
    r = variant(x, name)
    want = oracle.pnn_cluster_class(r, k)
    got, run = kr.cluster_class(r, k)
    assert np.array_equal(got, want), (got, want)
    full, run_full = kr.cluster_class(r, k, early=False)
    assert np.array_equal(full, want) and run_full == (100 if n > k else 0)
    assert run <= run_full


def test_restatement_equals_the_oracle_on_a_six_step_input_and_on_exact_ties(oracle):
    (_, a, ka), (_, b, kb) = extra_inputs()
    got, run = kr.cluster_class(a, ka)
    assert np.array_equal(got, oracle.pnn_cluster_class(a, ka))
    assert run == 6
    t = kr.pair_table(b)
    upper = t[np.triu_indices(120, 1)]
    assert np.unique(upper).size < upper.size, "the rounded input should have exactly tied distances"
    got, _ = kr.cluster_class(b, kb)
    assert np.array_equal(got, oracle.pnn_cluster_class(b, kb))


def test_the_table_is_symmetric_bit_for_bit():
    x, _, _ = gc.cls_case(4, 65, 33, n_classes=3)
    t = kr.pair_table(variant(x, "nan_tail_and_duplicate"))
    assert np.array_equal(np.isnan(t), np.isnan(t.T))
    ok = ~np.isnan(t)
    assert np.array_equal(t[ok].view(np.uint64), t.T[ok].view(np.uint64))


@pytest.mark.parametrize("label,rows,k", [pytest.param(*c, id=c[0]) for c in all_inputs()])
def test_stopping_at_the_fixed_point_changes_nothing(label, rows, k):
    table = kr.pair_table(rows)
    for steps in range(1, 8):
        early, run = kr.cluster_table(table, k, steps, early=True)
        full, run_full = kr.cluster_table(table, k, steps, early=False)
        assert np.array_equal(early, full), steps
        assert run <= run_full == (steps if rows.shape[0] > k else 0)


def test_library_declares_exports_and_binds_fir_cls_kmedoids(fir):
    assert "fir_cls_kmedoids" in {s[0] for s in fir.capi.SYMBOLS}
    assert hasattr(ctypes.CDLL(fir.lib_path()), "fir_cls_kmedoids")
    assert hasattr(fir.ClsModel, "kmedoids")
