"""The restatement of the gallery subsets (subset_ref) against masked_ref, and fir_keys_map_rows -- pure host code like
fir_keys_unpack, so it runs without a device -- against the restatement. Equality everywhere."""
import numpy as np
import pytest

import masked_ref
import subset_ref as sr
import synth

I32, U64 = np.int32, np.uint64
ERR_ARG = -1
NONE = sr.KEY_NONE


def half(n, seed):
    return (synth.splitmix64(np.arange(n, dtype=np.uint64), seed) & np.uint64(1)).astype(bool)


def keys_over(m, count, seed):
    """count keys with pseudo-random distance bits and low words inside [0, m), a few FIR_KEY_NONE among them"""
    h = synth.splitmix64(np.arange(count, dtype=np.uint64), seed)
    keys = (h & sr.HIGH) | (h % np.uint64(m))
    keys[::7] = NONE
    return keys


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130, 300, 1000))
def test_rows_of_mask_is_flatnonzero_of_the_unpacked_bits(n):
    for seed in range(3):
        take = half(n, 10 * n + seed)
        words = masked_ref.pack_bits(take)
        assert np.array_equal(sr.rows_of_mask(words, n), np.flatnonzero(take).astype(I32))
        assert np.array_equal(sr.rows_of_mask(words, n), np.flatnonzero(masked_ref.unpack_bits(words, n)).astype(I32))
        if n % 64:                                                   # bits at or past n change nothing
            dirty = words.copy()
            dirty[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
            assert np.array_equal(sr.rows_of_mask(dirty, n), np.flatnonzero(take).astype(I32))
        count = int(take.sum())
        for cap in (0, max(count - 1, 0), count, count + 5):
            c, rows = sr.rows_of_mask_capped(words, n, cap)
            assert c == count and np.array_equal(rows, np.flatnonzero(take)[:cap].astype(I32))


@pytest.mark.parametrize("off", (0, 1000, (1 << 31) - 400))
def test_map_rows_is_map_back(off):
    n = 300
    take = half(n, 77)
    sel = np.flatnonzero(take)
    keys = keys_over(sel.shape[0], 500, 78).reshape(50, 10)
    got, bad = sr.map_rows(keys, sel, off)
    assert not bad and np.array_equal(got, masked_ref.map_back(keys, sel, off))
    assert np.array_equal(got == NONE, keys == NONE)


def test_keys_map_rows_through_the_library(fir):
    n = 300
    sel = np.flatnonzero(half(n, 81)).astype(I32)
    m = sel.shape[0]
    keys = keys_over(m, 400, 82)
    for add in (0, 1000, -3, -(1 << 20)):                            # a negative row_add wraps as uint32 does
        want, bad = sr.map_rows(keys, sel, add)
        assert not bad
        got = fir.keys_map_rows(keys, sel, add)
        assert got.dtype == U64 and np.array_equal(got, want), add
        assert np.array_equal(got == NONE, keys == NONE)             # FIR_KEY_NONE untouched, nothing else becomes it
    low = fir.keys_map_rows(np.array([5 << 32 | 0], U64), sel, -int(sel[0]) - 1)
    assert int(low[0]) == (5 << 32 | 0xFFFFFFFF)                     # (distance bits 5, row -1 as uint32: not FIR_KEY_NONE)
    # an increasing map keeps a sorted key list sorted, ties by row included
    srt = np.sort(keys[keys != NONE])
    srt[10:20] = (srt[10] & sr.HIGH) | np.arange(10, dtype=U64)      # ten keys of one distance, rows 0..9
    srt = np.sort(srt)
    out = fir.keys_map_rows(srt, sel, 1000)
    assert np.all(out[1:] >= out[:-1]) and np.array_equal(out, sr.map_rows(srt, sel, 1000)[0])
    # a repeated row in an arbitrary list: equal keys come out
    rep = np.array([4, 9, 4], I32)
    out = fir.keys_map_rows(np.array([7 << 32 | 0, 7 << 32 | 2], U64), rep, 0)
    assert out[0] == out[1] == U64(7 << 32 | 4)


def test_keys_map_rows_errors_leave_the_buffer_alone(fir):
    L = fir.lib()
    p = lambda a: a.ctypes.data_as(fir.capi._vp)
    row_map = np.array([3, 5, 8], I32)

    def err(rc, text):
        assert rc == ERR_ARG and text in L.fir_last_error().decode(), (rc, L.fir_last_error())

    keys = np.array([1 << 32 | 1, int(NONE), 2 << 32 | 3, 3 << 32 | 0], U64)          # the third key's low word == m
    before = keys.copy()
    err(L.fir_keys_map_rows(p(keys), 4, p(row_map), 3, 0), "row 3 outside [0,3)")
    assert np.array_equal(keys, before)                              # the keys before the offending one too
    keys[2] = U64(9 << 32 | 0xFFFFFFFF)                              # all ones in the low word only: a row, not FIR_KEY_NONE
    before = keys.copy()
    err(L.fir_keys_map_rows(p(keys), 4, p(row_map), 3, 0), "outside [0,3)")
    assert np.array_equal(keys, before)
    err(L.fir_keys_map_rows(None, 4, p(row_map), 3, 0), "NULL argument")
    err(L.fir_keys_map_rows(p(keys), 4, None, 3, 0), "NULL argument")
    err(L.fir_keys_map_rows(p(keys), -1, p(row_map), 3, 0), "count < 0")
    err(L.fir_keys_map_rows(p(keys), 4, p(row_map), -1, 0), "m < 0")
    assert L.fir_keys_map_rows(None, 0, None, 0, 0) == 0
    only_none = np.full(3, NONE, U64)
    assert L.fir_keys_map_rows(p(only_none), 3, None, 0, 0) == 0 and np.all(only_none == NONE)   # an empty subset maps no key
    with pytest.raises(fir.FirError):
        fir.keys_map_rows(np.array([1 << 32 | 3], U64), row_map, 0)
