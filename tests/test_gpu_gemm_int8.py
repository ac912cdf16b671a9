"""The int8 nomination pass of large L2 top-1 batches (fir_gemm_i8.h, k_gemm_proxy_f16x<.., I8 = 1>): rows and queries minus the
gallery's column means, quantised to int8, nominated on the int8 matrix cores; the re-rank and its certificate are the fp16
flow's with the measured quantisation residuals in the windows. Every case switches the pass on with set_int8_nomination(1),
takes the exact scan (set_large_batch_mfma(0)) on the same handle as the yardstick -- index and distance bit for bit -- and
checks that last_dispatch names the int8 kernel. Shapes as in test_gpu_gemm_last_unit.py: the smallest at which each unit
sequence and each ragged end is walked. The lists and bounds the pass hands the re-rank, and its second-chance rounds, are held
against float64 in tests/test_gpu_gemm_int8_nominations.py."""
import numpy as np
import pytest

import synth
from test_gemm_int8_formulation import near_tie_fixture

pytestmark = pytest.mark.gpu

N_MULTI, QB_MULTI = 32 * 626 + 5, 2048                 # sixteen pairs share a launch: every wave walks several row blocks


def both_on_one_handle(fir, rows, q, labels=None):
    with fir.Gallery(rows, labels, 0, 0) as g:
        g.set_large_batch_mfma(q.shape[0])
        g.set_int8_nomination(1)
        got = g.search_top1(q)
        disp = g.last_dispatch()
        st = g.mfma_stats()
        assert disp["path"] == "mfma" and "k_gemm_proxy_i8x<" in disp["kernel"], disp
        g.set_large_batch_mfma(0)
        want = g.search_top1(q)
        assert g.last_dispatch()["path"] == "scan"
    return got, want, st, disp


def assert_same_keys(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def gallery_and_queries(seed, n, d, qb):
    """test_gpu_gemm_last_unit.py's plants: query 5 is row 11, which the LAST row is a copy of (the lower row wins the tie); query 6 is
    the row before the last (the winner lies in the last block, short or not)."""
    rows = synth.make_gallery(seed, n, d, 0)
    q, _ = synth.make_queries(seed, rows, qb, 0)
    if n > 12:
        rows[n - 1] = rows[11]
        q[5] = rows[11]
        q[6] = rows[n - 2]
    return rows, q


@pytest.mark.parametrize("d,odd", [(200, 2), (256, 2), (512, 0), (768, 1), (1024, 0)])
def test_unit_sequences(fir, d, odd):
    """Units of 256 features: padding inside the one unit (200), one, two, three (the odd form) and four. Random data: every first
    certificate holds, so a broken pass cannot hide behind the second pass or the exact device scan."""
    rows, q = gallery_and_queries(1500 + d, N_MULTI, d, QB_MULTI)
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert f"<3, {odd}>" in disp["kernel"], disp
    assert_same_keys(got, want)
    assert got[0][5] == 11 and got[0][6] == N_MULTI - 2
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st
    # int8 fragment bytes of one launch: the gallery's pieces once, sixteen pairs' tiles and keys
    dk8 = (d + 255) // 256 * 8
    assert disp["bytes_per_launch"] == ((N_MULTI + 31) // 32) * dk8 * 1024 + 16 * (4 * dk8 * 1024 + 1024), disp


@pytest.mark.parametrize("n,qb", [(32 * 7 + 5, 128), (20, 128), (8192 * 3 + 37, 300)])
def test_small_and_ragged_galleries(fir, n, qb):
    """229 rows: a short last block, waves past the end. 20 rows: not one full block. 24 613 rows x 300 queries: two pairs share a
    range and the third pair's tile is ragged."""
    rows, q = gallery_and_queries(1700 + n, n, 512, qb)
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert got[0][5] == 11 and got[0][6] == n - 2
    assert st["fallback_queries"] == 0, st


def test_class_ordered_near_duplicates(fir):
    """500 identities x 40 near-duplicate rows (test_gpu_gemm_last_unit.py's gallery): hundreds of rows inside a window; nothing is
    left to the exact device scan."""
    rng = np.random.default_rng(47)
    ident, per, d, qb = 500, 40, 512, 2048
    centres = rng.random((ident, d), dtype=np.float32)
    rows = np.repeat(centres, per, axis=0) * (1 + 1e-4 * (rng.random((ident * per, d), dtype=np.float32) - 0.5))
    rows = synth.normalise(rows.astype(np.float32), 0)
    who = rng.integers(0, ident, qb)
    q = synth.normalise((centres[who] * (1 + 1e-4 * (rng.random((qb, d), dtype=np.float32) - 0.5))).astype(np.float32), 0)
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert np.all(got[0] // per == who)
    assert st["fallback_queries"] == 0, st


def test_more_ties_than_a_list_holds_go_to_the_exact_scan(fir):
    """5 000 copies of one row: no list holds them, the exact device scan answers (the first copy wins)."""
    rows, q = gallery_and_queries(1900, 8192, 512, 128)
    rows[1000:6000] = rows[1000]
    q[9] = rows[1000]
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert got[0][9] == 1000
    assert st["fallback_queries"] >= 1, st


def test_bad_queries_and_rows(fir):
    """NaN, +-inf, 1e30, 1e-30 and zero queries; a zero row; then a constant gallery (packs zeros, R = 0). Keys are the exact scan's;
    the NaN query has no answer, as there."""
    rows, q = gallery_and_queries(2100, 4099, 512, 128)
    rows[77] = 0
    q[20, 3] = np.nan
    q[21, 5] = np.inf
    q[22, 7] = -np.inf
    q[23] *= np.float32(1e30)
    q[24] *= np.float32(1e-30)
    q[25] = 0
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert got[0][20] == -1
    const = np.full((2048, 512), np.float32(0.25), np.float32)
    got, want, st, disp = both_on_one_handle(fir, const, q)
    assert_same_keys(got, want)


@pytest.mark.parametrize("scale,turned_away", [(1e-11, False), (1e-16, True), (1e-17, True)])
def test_small_magnitudes(fir, scale, turned_away):
    """Rows AND queries of small magnitude: from about 1e-13 the product of the two scales leaves (1e-30, 1e30) -- from 1e-17 it is inf,
    1 / it is 0 and every proxy would be the row's norm -- and k_gemm_qprep_i8 leaves the query to the exact device scan; at 1e-11 the
    int8 pass answers. Keys are the exact scan's either way (tests/test_gemm_int8_formulation.py has the arithmetic)."""
    rows, q = gallery_and_queries(2200, 4099, 512, 128)
    rows = (rows * np.float32(scale)).astype(np.float32)
    q = (q * np.float32(scale)).astype(np.float32)
    got, want, st, disp = both_on_one_handle(fir, rows, q)
    assert_same_keys(got, want)
    assert got[0][5] == 11 and got[0][6] == 4099 - 2
    assert st["fallback_queries"] == (128 if turned_away else 0), st


def test_dispatch_and_memory(fir):
    """What takes the pass and what keeps fp16: mode 0, the K nearest rows, the nearest distinct classes, a few-query call, a feature
    prefix and rows longer than 1 024 features name fp16 kernels; the int8 copy is built by the first int8 call and reported with the fragments."""
    n, d, qb = 4099, 512, 256
    rows, q = gallery_and_queries(2300, n, d, qb)
    labels = synth.make_labels(n, 101)
    with fir.Gallery(rows, labels, 0, 0) as g:
        g.set_large_batch_mfma(1)
        g.set_int8_nomination(0)
        a = g.search_top1(q)
        assert "k_gemm_proxy_f16x<3, 0, 0>" in g.last_dispatch()["kernel"]
        before = g.memory_bytes()["fp16_fragments"]
        g.set_int8_nomination(1)
        g.search_topk(q, 5)
        assert "k_gemm_proxy_f16x<4" in g.last_dispatch()["kernel"]
        for kc in (1, 3):                                                       # the nearest distinct classes, the nearest one included
            g.search_top_classes(q, 101, kc)
            ld = g.last_dispatch()
            assert ld["path"] == "mfma" and "k_gemm_proxy_f16x<1," in ld["kernel"], ld
        g.search_top1(q[:32])
        assert "k_gemm_proxy_f16x<" in g.last_dispatch()["kernel"]          # a few-query call
        assert g.memory_bytes()["fp16_fragments"] == before                     # nothing has built the copy yet
        b = g.search_top1(q)
        assert "k_gemm_proxy_i8x<3, 0>" in g.last_dispatch()["kernel"]
        assert g.memory_bytes()["fp16_fragments"] == before + ((n + 31) // 32) * 16 * 1024
        assert_same_keys(a, b)
        g.search_top1(q, 0, 256)
        assert "k_gemm_proxy_f16x<" in g.last_dispatch()["kernel"]          # a prefix range
        g.set_int8_nomination(-1)
        g.search_top1(q)
        assert "k_gemm_proxy_f16x<" in g.last_dispatch()["kernel"]          # the rule: never under a caller's threshold
        g.set_int8_nomination(0)
        c = g.search_top1(q)
        assert "k_gemm_proxy_f16x<3, 0, 0>" in g.last_dispatch()["kernel"]
        assert_same_keys(a, c)
    rows, q = gallery_and_queries(2301, 2053, 1280, 128)
    with fir.Gallery(rows, None, 0, 0) as g:
        g.set_large_batch_mfma(128)
        g.set_int8_nomination(1)
        g.search_top1(q)
        assert "k_gemm_proxy_f16x<3, 1" in g.last_dispatch()["kernel"]


def test_automatic_rule_and_the_way_back_to_fp16(fir):
    """Automatic mode over >= 65 536 rows: a call of 2 048 queries takes the int8 pass, a smaller one fp16. 5 000 copies of one row
    and 256 queries that ask for it: more ties than a list holds, so more than one query in sixteen of the first int8 call needs a
    second pass -- the library learns that behind the call, and the gallery's later calls are fp16 again. Every call has the exact
    scan's keys."""
    n, d, qb = 70000, 64, 2048
    rows, q = gallery_and_queries(2500, n, d, qb)
    with fir.Gallery(rows, None, 0, 0) as g:
        g.search_top1(q[:512])
        assert "k_gemm_proxy_f16x<" in g.last_dispatch()["kernel"]              # below the rule's call size
        a = g.search_top1(q)
        assert "k_gemm_proxy_i8x<3, 2>" in g.last_dispatch()["kernel"], g.last_dispatch()
        b = g.search_top1(q)
        assert "k_gemm_proxy_i8x<3, 2>" in g.last_dispatch()["kernel"]           # nothing to go back for
        assert g.mfma_stats()["second_pass_queries"] == 0
        g.set_large_batch_mfma(0)
        want = g.search_top1(q)
    assert_same_keys(a, want)
    assert_same_keys(b, want)
    rows = rows.copy()
    q = q.copy()
    rows[1000:6000] = rows[1000]
    q[::8] = rows[1000]
    with fir.Gallery(rows, None, 0, 0) as g:
        a = g.search_top1(q)
        assert "k_gemm_proxy_i8x<" in g.last_dispatch()["kernel"]
        assert g.mfma_stats()["second_pass_queries"] >= qb // 8
        b = g.search_top1(q)                                                      # (the host-pointer call before it has finished: its counter has arrived)
        assert "k_gemm_proxy_f16x<" in g.last_dispatch()["kernel"] and "int8 nomination off" in g.last_dispatch()["kernel"], g.last_dispatch()
        c = g.search_top1(q)
        assert "k_gemm_proxy_f16x<" in g.last_dispatch()["kernel"]
        g.set_large_batch_mfma(0)
        want = g.search_top1(q)
    for got in (a, b, c):
        assert_same_keys(got, want)
    assert a[0][0] == 1000


def test_an_unsound_int8_bound_is_visible(fir, fir_audit, monkeypatch):
    """The suite can see an unsound bound: on the near-tie fixture (tests/test_gemm_int8_formulation.py) the audit build with
    FIR_GEMM_EREL_SCALE=0.25 -- the knob scales the whole bound, the absolute term included -- returns row B, certified (no exact
    device scan); with the bound as derived, and in the shipped library whatever the variable says, the reference's row A."""
    rows, q = near_tie_fixture()
    got = {}
    for lib_name, pkg in (("audit", fir_audit), ("shipped", fir)):
        for scale in ("1", "0.25"):
            monkeypatch.setenv("FIR_GEMM_EREL_SCALE", scale)
            with pkg.Gallery(rows, None, 0, 0) as g:
                g.set_large_batch_mfma(1)
                g.set_int8_nomination(1)
                idx, dist = g.search_top1(q)
                assert "k_gemm_proxy_i8x<" in g.last_dispatch()["kernel"]
                got[lib_name, scale] = (idx, dist, g.mfma_stats()["fallback_queries"])
                g.set_large_batch_mfma(0)
                want = g.search_top1(q)
            monkeypatch.delenv("FIR_GEMM_EREL_SCALE")
    assert want[0][0] == 0
    for key in (("audit", "1"), ("shipped", "1"), ("shipped", "0.25")):
        assert_same_keys(got[key][:2], want)
    idx, dist, fb = got["audit", "0.25"]
    assert idx[0] == 2 and dist[0] > want[1][0] and fb == 0, (idx[0], dist[0], fb)
