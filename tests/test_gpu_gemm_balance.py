"""The fp16 top-1 pass hands its row blocks out at run time (k_gemm_proxy_f16x<3, 0, *>, `next_blk`): whichever wave asks
next takes the next block of the workgroup's row range. Whatever the order, every block is walked exactly once -- the keys of
the gallery's own dispatch are the exact scan's (set_large_batch_mfma(0)) on the same handle, bit for bit: short and clamped
last blocks, every number of units per row block, waves that get no block at all, frequent appends."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


def both_on_one_handle(fir, rows, q, threshold=-1):
    """(index, distance) through the matrix cores and through the exact scan, the same gallery handle; the matrix-core call's counters.
    threshold -1 = the automatic rule (below 65 536 rows it builds the matrix-core state for a gallery's fourth such call: the first three
    take the scan); a gallery that rule leaves to the scan altogether is given the caller's threshold instead."""
    with fir.Gallery(rows, None, 0, 0) as g:
        if threshold >= 0:
            g.set_large_batch_mfma(threshold)
        for _ in range(4):
            got = g.search_top1(q)
            disp = g.last_dispatch()
            if disp["path"] == "mfma":
                break
        st = g.mfma_stats()                            # (read once, behind the one matrix-core call)
        assert disp["path"] == "mfma" and "k_gemm_proxy_f16x<3, 0," in disp["kernel"], disp
        g.set_large_batch_mfma(0)
        want = g.search_top1(q)
        assert g.last_dispatch()["path"] == "scan"
    return got, want, st, disp


def assert_no_detours(st):
    """random data: every first certificate held -- no query took a second matrix-core pass, none the exact device scan (the
    keys alone cannot tell: either detour returns the right ones)"""
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


def assert_same_keys(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("d", [512, 384, 256])
@pytest.mark.parametrize("n", [8192 * 3 + 37, 40000])
def test_two_pairs_share_a_range(fir, n, d):
    """256 queries = two pairs in one launch (share = 2), 128 row ranges of a few row blocks each. 24 613 rows: no multiple of
    32 x 8, the last range ends in a short block and in blocks past the end (clamped loads, nothing appended). 384 features:
    three units per row block, the form whose two gallery buffers swap roles."""
    rows = synth.make_gallery(300 + d, n, d, 0)
    q, _ = synth.make_queries(300 + d, rows, 256, 0)
    rows[n - 1] = rows[11]                             # an exact tie between the first row block and the short last one: the lower row wins
    q[5] = rows[11]
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert ("<3, 0, 1>" in disp["kernel"]) == (d == 384), disp["kernel"]
    assert_same_keys(got, want)
    assert got[0][5] == 11
    assert_no_detours(st)


def test_sixteen_pairs_share_a_range(fir):
    """2 048 queries = sixteen pairs per launch, as the headline runs: 16 row ranges, ~80 row blocks per workgroup -- every wave
    comes back to the counter about ten times; the last range ends in a short block."""
    n, d = 40000 + 37, 512
    rows = synth.make_gallery(41, n, d, 0)
    q, _ = synth.make_queries(41, rows, 2048, 0)
    got, want, st, _ = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert_no_detours(st)


def test_fewer_row_blocks_than_waves(fir):
    """160 rows = five row blocks: one workgroup has work, three of its eight waves start past the end of the rows and the counter
    has nothing left when the others come back to it. (The automatic rule leaves a gallery this small to the scan: the test sets
    the caller's threshold.)"""
    n, d = 32 * 5, 512
    rows = synth.make_gallery(43, n, d, 0)
    q, _ = synth.make_queries(43, rows, 128, 0)
    got, want, st, _ = both_on_one_handle(fir, rows, q, threshold=128)
    assert_same_keys(got, want)
    assert_no_detours(st)


def test_class_ordered_near_duplicates_append_often(fir):
    """500 identities x 40 near-duplicate rows, class-ordered, 2 048 queries: hundreds of rows fall inside one rounding window of
    the nearest, appends are frequent, the staged appends overflow into the lists and are flushed at the workgroup's end -- and
    nothing is left to the exact device scan."""
    rng = np.random.default_rng(47)
    ident, per, d, qb = 500, 40, 512, 2048
    centres = rng.random((ident, d), dtype=np.float32)
    rows = np.repeat(centres, per, axis=0) * (1 + 1e-4 * (rng.random((ident * per, d), dtype=np.float32) - 0.5))
    rows = synth.normalise(rows.astype(np.float32), 0)
    who = rng.integers(0, ident, qb)
    q = synth.normalise((centres[who] * (1 + 1e-4 * (rng.random((qb, d), dtype=np.float32) - 0.5))).astype(np.float32), 0)
    got, want, st, _ = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert np.all(got[0] // per == who)
    assert st["fallback_queries"] == 0, st
