"""The fp16 matrix-core passes (k_gemm_proxy_f16x) peel the last unit of every row block: it loads the block's row norms
unconditionally, from a clamped address, and reads the bounds the next row block's first step checks against; the first
step checks the previous block's sums without asking whether anything is owed, and the rare path of that check lies out of
line. Whatever the unit sequence -- one unit that is first and last at once, two without a middle, an odd number, the
streamed ring, the sixteen-piece units of the few-block forms, the K-nearest form, the sample flow's two passes -- the keys are the exact scan's
(set_large_batch_mfma(0)) on the same handle, bit for bit. The shapes are the smallest at which each of these paths is
taken; galleries too small for the automatic rule get the caller's threshold (the number of queries of the call)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

N_SMALL = 32 * 70 + 5                                  # 70 full row blocks and a short one: a wave walks one block, one straddles
# 2 048 queries = sixteen pairs (eight where the query slabs are streamed) share a launch, so the chip's workgroups split into 16 (32) row
# ranges: over 20 037 rows = 626 full row blocks and a short one every wave walks several blocks in a row -- the first step's deferred
# checks, the last unit's early bound and the hand-out's ticket only exist from a wave's second block on
N_MULTI, QB_MULTI = 32 * 626 + 5, 2048


def both_on_one_handle(fir, rows, q, k=1):
    """(index, distance) through the matrix cores (threshold = this call's queries) and through the exact scan, the same
    gallery handle; the matrix-core call's counters and dispatch."""
    def search(g):
        return g.search_top1(q) if k == 1 else g.search_topk(q, k)
    with fir.Gallery(rows, None, 0, 0) as g:
        g.set_large_batch_mfma(q.shape[0])
        got = search(g)
        disp = g.last_dispatch()
        st = g.mfma_stats()
        assert disp["path"] == "mfma" and "k_gemm_proxy_f16x<" in disp["kernel"], disp
        g.set_large_batch_mfma(0)
        want = search(g)
        assert g.last_dispatch()["path"] == "scan"
    return got, want, st, disp["kernel"]


def assert_same_keys(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def assert_no_detours(st):
    """random data: every first certificate held -- no query took a second matrix-core pass, none the exact device scan (the
    keys alone cannot tell: either detour returns the right ones)"""
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


def gallery_and_queries(seed, n, d, qb):
    """Query 5 is row 11, which the LAST row is a copy of (a tie between the first row block and the last: the lower row wins);
    query 6 is the row before the last (the winner lies in the last block, short or not)."""
    rows = synth.make_gallery(seed, n, d, 0)
    q, _ = synth.make_queries(seed, rows, qb, 0)
    if n > 12:
        rows[n - 1] = rows[11]
        q[5] = rows[11]
        q[6] = rows[n - 2]
    return rows, q


def check_planted(got, n):
    if n > 12:
        assert got[0][5] == 11 and got[0][6] == n - 2


@pytest.mark.parametrize("d,units,odd", [(100, 1, 2), (256, 2, 0), (384, 3, 1), (512, 4, 0)])
def test_units_per_row_block(fir, d, units, odd):
    """One unit (first and last at once: a kernel form of its own, <*, 0, 2>), two (no middle), three (the odd form: the
    gallery buffers swap roles), four."""
    rows, q = gallery_and_queries(500 + d, N_MULTI, d, QB_MULTI)
    got, want, st, kern = both_on_one_handle(fir, rows, q)
    assert f"<3, 0, {odd}>" in kern, kern
    assert_same_keys(got, want)
    check_planted(got, N_MULTI)
    assert_no_detours(st)


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("d,odd", [(100, 2), (256, 0), (384, 1)])
def test_sample_flow_units_per_row_block(fir, monkeypatch, d, odd, k):
    """The smallest-proxy sample flow (FIR_GEMM_ADAPTIVE=0, read when the handle's matrix-core state is made): the sample pass
    <2, 0, odd> -- for k = 5 with its 64 subsets' minima -- gives the bound, the full pass <1, 0, odd> appends every row below it and
    is the kernel the call reports. One unit, an even number, an odd number: the epilogues of these two modes are not the ones
    <3, *> and <4, *> run."""
    monkeypatch.setenv("FIR_GEMM_ADAPTIVE", "0")
    rows, q = gallery_and_queries(500 + d, N_MULTI, d, QB_MULTI)
    got, want, st, kern = both_on_one_handle(fir, rows, q, k=k)
    assert f"<1, 0, {odd}>" in kern, kern
    assert_same_keys(got, want)
    if k == 1:
        check_planted(got, N_MULTI)
    assert_no_detours(st)


@pytest.mark.parametrize("d,odd", [(640, 1), (1280, 0)])
def test_streamed_units(fir, d, odd):
    """Rows longer than the resident tile: the query slabs go through the LDS ring, whose hand-written wait now has the two norm
    loads among the operations it leaves in flight. 640 features = five units (odd), 1280 = ten."""
    rows, q = gallery_and_queries(600 + d, N_MULTI, d, QB_MULTI)
    got, want, st, kern = both_on_one_handle(fir, rows, q)
    assert f"<3, 1, {odd}>" in kern, kern
    assert_same_keys(got, want)
    check_planted(got, N_MULTI)
    assert_no_detours(st)


@pytest.mark.parametrize("d", [100, 512, 1280])
@pytest.mark.parametrize("n", [32 * 5, 32 * 7 + 5, 20])
def test_few_row_blocks_and_clamped_norm_loads(fir, n, d):
    """One row range at most, a wave walks one block. 160 rows: fewer row blocks than waves -- three waves walk a block past
    the end, whose norm loads are clamped into the gallery's last 32 rows. 229 rows: the last block straddles the end. 20 rows: not one full block, and `gnorm` holds fewer
    than the 32 floats a last unit reads (the loads are pointed at the fp16 fragments instead; nothing of them is used)."""
    rows, q = gallery_and_queries(700 + d + n, n, d, 128)
    got, want, st, kern = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    check_planted(got, n)
    assert_no_detours(st)


def test_two_pairs_share_a_range(fir):
    """24 613 rows, 256 queries: two pairs in one launch (share = 2) walk 128 row ranges of a few blocks each; the last range
    ends in a short block and in blocks past the end."""
    n, d = 8192 * 3 + 37, 512
    rows, q = gallery_and_queries(811, n, d, 256)
    got, want, st, kern = both_on_one_handle(fir, rows, q)
    assert "<3, 0, 0>" in kern, kern
    assert_same_keys(got, want)
    check_planted(got, n)
    assert_no_detours(st)


@pytest.mark.parametrize("n,d,streamed", [(N_SMALL, 512, 0), (32 * 2187 + 5, 512, 0), (N_SMALL, 1280, 1)])
@pytest.mark.parametrize("qb,njb", [(16, 1), (32, 2)])
def test_few_block_forms(fir, qb, njb, n, d, streamed):
    """At most 16 / 32 queries: one / two live query blocks; the resident form's units are sixteen pieces. One pair per launch
    leaves the chip 256 row ranges: 69 989 rows are the fewest at which some waves walk a second block."""
    rows, q = gallery_and_queries(900 + d + qb, n, d, qb)
    got, want, st, kern = both_on_one_handle(fir, rows, q)
    assert f"<3, {streamed}, 0, 0, {njb}>" in kern, kern
    assert_same_keys(got, want)
    check_planted(got, n)
    assert_no_detours(st)


@pytest.mark.parametrize("d,streamed,odd", [(100, 0, 2), (512, 0, 0), (1280, 1, 0)])
def test_top5(fir, d, streamed, odd):
    """The K nearest rows with the bound found on the way (<4, *>): the same unit sequences, eight slots per query; 100 features
    are the one-unit form."""
    rows, q = gallery_and_queries(1000 + d, N_MULTI, d, QB_MULTI)
    rows[200:203] = rows[N_MULTI - 9]                   # four equal rows, three of them in one block, one in the last full block
    q[7] = rows[N_MULTI - 9]
    got, want, st, kern = both_on_one_handle(fir, rows, q, k=5)
    assert f"<4, {streamed}, {odd}>" in kern, kern
    assert_same_keys(got, want)
    assert list(got[0][7][:4]) == [200, 201, 202, N_MULTI - 9]
    assert_no_detours(st)


def test_class_ordered_near_duplicates_append_often(fir):
    """500 identities x 40 near-duplicate rows, class-ordered, 2 048 queries: hundreds of rows fall inside one rounding window of
    the nearest, so the check's rare path -- now out of line -- runs all the time, the staged appends overflow into the lists,
    and nothing is left to the exact device scan."""
    rng = np.random.default_rng(47)
    ident, per, d, qb = 500, 40, 512, 2048
    centres = rng.random((ident, d), dtype=np.float32)
    rows = np.repeat(centres, per, axis=0) * (1 + 1e-4 * (rng.random((ident * per, d), dtype=np.float32) - 0.5))
    rows = synth.normalise(rows.astype(np.float32), 0)
    who = rng.integers(0, ident, qb)
    q = synth.normalise((centres[who] * (1 + 1e-4 * (rng.random((qb, d), dtype=np.float32) - 0.5))).astype(np.float32), 0)
    got, want, st, kern = both_on_one_handle(fir, rows, q)
    assert "<3, 0, 0>" in kern, kern
    assert_same_keys(got, want)
    assert np.all(got[0] // per == who)
    assert st["fallback_queries"] == 0, st
