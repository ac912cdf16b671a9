"""fir_gallery_remove_plan -- fir_gallery_remove_rows' swap-remove rule as pure integer work on the host -- against the numpy
statement of the rule in gallery_update_ref.py. No GPU: the call touches no device."""
import numpy as np
import pytest

import gallery_update_ref as ref

SIZES = (1, 64, 65, 200)
KINDS = ("none", "one", "last", "tail", "head", "all", "third")


def removal_set(n, kind):
    rng = np.random.default_rng(1000 * n + KINDS.index(kind))
    if kind == "none":
        return np.empty(0, np.int32)
    if kind == "one":
        return np.array([n // 3], np.int32)
    if kind == "last":
        return np.array([n - 1], np.int32)
    if kind == "tail":                                   # only rows at or beyond n': nothing moves
        m = max(1, n // 4)
        return rng.permutation(np.arange(n - m, n)).astype(np.int32)
    if kind == "head":                                   # only rows below n' (where the set fits there): every one is a hole
        m = max(1, n // 4)
        return rng.permutation(np.arange(0, min(m, n))).astype(np.int32)
    if kind == "all":
        return rng.permutation(n).astype(np.int32)
    return rng.choice(n, size=max(1, n // 3), replace=False).astype(np.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_remove_plan_is_the_rule(fir, n, kind):
    idx = removal_set(n, kind)
    moved = fir.remove_plan(n, idx)
    assert moved.dtype == np.int32 and moved.shape == idx.shape
    assert np.array_equal(moved, ref.remove_plan(n, idx)), (n, kind, idx, moved)
    # the plan applied to arange(n): exactly the surviving rows, each once, the rows that were not moved in place
    n_new = n - idx.size
    after = np.arange(n_new, dtype=np.int64)
    for r, src in zip(idx.tolist(), moved.tolist()):
        if r < n_new:
            assert src >= n_new, "a hole is filled from the tail"
            after[r] = src
        else:
            assert src == -1
    survivors = np.setdiff1d(np.arange(n), idx)
    assert np.array_equal(np.sort(after), survivors)
    untouched = np.setdiff1d(np.arange(n_new), idx)
    assert np.array_equal(after[untouched], untouched)
    # holes ascending take survivors ascending
    holes = np.sort(idx[idx < n_new])
    assert np.all(np.diff(after[holes]) > 0)
    assert np.array_equal(after, ref.remove_order(n, idx))


@pytest.mark.parametrize("n", SIZES)
def test_remove_plan_refuses_bad_lists(fir, n):
    L = fir.lib()
    bad = [np.array([0, 0], np.int32), np.array([-1], np.int32), np.array([n], np.int32), np.array([n - 1, 0, n - 1], np.int32)]
    for idx in bad:
        with pytest.raises(fir.FirError) as e:
            fir.remove_plan(n, idx)
        assert e.value.code == -1, idx                   # FIR_ERR_ARG
        with pytest.raises(ValueError):
            ref.remove_plan(n, idx)
    out = np.zeros(1, np.int32)
    one = np.zeros(1, np.int32)
    assert L.fir_gallery_remove_plan(n, one.ctypes.data, -1, out.ctypes.data) == -1
    assert b"m < 0" in L.fir_last_error()
    assert L.fir_gallery_remove_plan(n, None, 1, out.ctypes.data) == -1
    assert L.fir_gallery_remove_plan(n, None, 0, None) == 0          # nothing to do
    assert L.fir_gallery_remove_plan(n, one.ctypes.data, 1, None) == 0   # moved_from may be NULL: the checks alone
