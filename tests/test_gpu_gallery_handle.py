"""The gallery handle's own bookkeeping (fir_capi.hip's host side), not its answers: what fir_gallery_memory_bytes reports against what the
calls must have allocated, which launches a profiled call times and records (the row samples of the candidate-list path and of the
class scan's bound are scans "on behalf of" a call), and which error a bad call reports first."""
import ctypes as C

import numpy as np
import pytest

import nomination_scan_ref as ref
import synth

pytestmark = pytest.mark.gpu

L2, CHI2 = 0, 1
FIR_OK, FIR_ERR_ARG, FIR_ERR_STATE = 0, -1, -5


def test_memory_report_follows_the_allocations(fir):
    """L2, 5 000 x 96 (79 tiles of 64 rows, 24 float4 chunks per row), no labels, never the matrix cores. A workspace asked for
    `need` elements holds max(need, 4096) of them; nothing that is large enough is touched.
      create        tiled = 79 tiles x 64 rows x 24 chunks x 16 bytes; scratch = 0
      top-1, 300    host queries of 115 200 bytes: the pinned path, no staging of queries. dkeys: 300 keys -> 4096 x 8 bytes;
                    qt (top1_dev): 300 x 96 + 64 floats, the 64 being the prefetch slack of the hand-scheduled kernel
      range, 4      dq: 4 x 96 floats -> 4096 x 4 bytes; dout: 4 x 5000 floats; qt is large enough
      top-3, 4      pinned path (12 keys, fewer than 8 queries), the register-list scan: dkeys and qt are large enough; part
                    (topk_dev): max_waves x min(queries per pass, 4) x k keys, and a gallery this small runs 16 queries per pass"""
    n, d = 5000, 96
    rows = synth.make_gallery(41, n, d, L2)
    q, _ = synth.make_queries(41, rows, 300, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        g.set_large_batch_mfma(0)
        m0 = g.memory_bytes()
        assert m0 == {"tiled": 79 * 64 * 24 * 16, "fp16_fragments": 0, "rowmajor_shadow": 0, "scratch": 0}, m0
        after_top1 = 4096 * 8 + (300 * 96 + 64) * 4
        after_range = after_top1 + max(4 * 96, 4096) * 4 + 4 * 5000 * 4
        for rep in range(2):                                   # the second round finds everything large enough
            g.search_top1(q)
            assert g.memory_bytes() == dict(m0, scratch=after_top1 if rep == 0 else after_range)
            g.range_distances(q[:4])
            assert g.memory_bytes() == dict(m0, scratch=after_range)
        tune = g.get_tuning()
        assert tune["queries_per_pass"] == 16
        part = max(tune["max_waves"] * min(tune["queries_per_pass"], 4) * 3, 4096) * 8
        g.search_topk(q[:4], 3)
        assert g.memory_bytes() == dict(m0, scratch=after_range + part)
        g.search_topk(q[:4], 3)
        g.search_top1(q)
        assert g.memory_bytes() == dict(m0, scratch=after_range + part)


def _timed(g):
    return len(g.profile_read()[0])


def test_row_samples_are_neither_timed_nor_recorded(fir, monkeypatch):
    """Chi-square, 65 600 x 32 in the plain range, 16 queries: the candidate-list path. Its row samples run with the handle's
    profiling off and unrecorded; the event pairs and the dispatch record belong to the append scan (k_nominate), one pair per
    recorded launch. The handle must not stay quiet: the next call, 3 queries through the exact scan, takes one pass of 2 queries and
    one of 1 -- two kernels, two event pairs, and a record that names the last of them (a record counts launches of ONE kernel)."""
    for name in ("FIR_CHI2_NOMINATION", "FIR_EXACT_SAMPLES", "FIR_NO_CHI2_NOMINATION"):
        monkeypatch.delenv(name, raising=False)
    rows, q = ref.make_case("pair_zero", 65600, 32, 16)
    with fir.Gallery(rows, None, CHI2, 0) as g:
        assert g.value_range()[0]
        g.profile_enable(True)
        g.search_top1(q)
        rec, timed = g.last_dispatch(), _timed(g)
        print("list path: timed", timed, "recorded", rec["launches"], rec["kernel"])
        assert "k_nominate" in rec["kernel"], rec
        assert timed == rec["launches"] >= 1, (timed, rec)
        monkeypatch.setenv("FIR_NO_CHI2_NOMINATION", "1")
        g.search_top1(q[:3])
        monkeypatch.delenv("FIR_NO_CHI2_NOMINATION")
        rec, timed = g.last_dispatch(), _timed(g)
        print("exact scan: timed", timed, "recorded", rec["launches"], rec["kernel"])
        assert "k_scan" in rec["kernel"] and rec["path"] == "scan", rec
        assert rec["launches"] >= 1 and timed == 2, (timed, rec)


def test_class_scan_sample_window_is_timed_and_recorded(fir):
    """L2, 20 000 x 32 (313 tiles), 5 000 classes, 17 queries, never the matrix cores: the class scan bounds itself from the leading
    eighth of the tiles, then scans the rest. Both windows are launches of the call itself: two event pairs, two recorded launches
    of the class-minimum scan. The top-1 call after it is recorded and timed as its own."""
    n, d, nc, nq = 20000, 32, 5000, 17
    rows = synth.make_gallery(1000 + n + d, n, d, L2)
    q, _ = synth.make_queries(n + d, rows, nq, L2)
    labels = np.random.default_rng(77).permutation(np.arange(n, dtype=np.int32) % nc).astype(np.int32)
    with fir.Gallery(rows, labels, L2, 0) as g:
        g.set_large_batch_mfma(0)
        g.profile_enable(True)
        g.search_top_classes(q, nc, 10)
        rec, timed = g.last_dispatch(), _timed(g)
        print("class scan: timed", timed, "recorded", rec["launches"], rec["kernel"])
        assert "fir::k_scan<8, 0, 8, 5, " in rec["kernel"], rec
        assert timed == rec["launches"] == 2, (timed, rec)
        g.search_top1(q)
        rec, timed = g.last_dispatch(), _timed(g)
        print("top-1 after it: timed", timed, "recorded", rec["launches"], rec["kernel"])
        assert "k_scan" in rec["kernel"] and "8, 5, " not in rec["kernel"] and rec["path"] == "scan", rec
        assert 1 <= rec["launches"] <= timed, (timed, rec)                # (several tile sizes: the record names the last one's kernel)


def test_first_error_of_a_bad_call(fir):
    """The code and the text of every single bad argument, written down from the library before its entry points shared one
    preamble, and which of two bad arguments is reported: qb < 0 before everything, k before the range, the missing labels
    before the range. qb == 0 is a successful call that touches no output (top_classes checks its other arguments first)."""
    L = fir.lib()
    n, d = 300, 16
    rows = synth.make_gallery(5, n, d, L2)
    q = np.ascontiguousarray(synth.make_queries(5, rows, 4, L2)[0], np.float32)
    idx, dist, cls = np.full(32, 7, np.int32), np.full(32, 7.0, np.float32), np.full(32, 7, np.int32)
    out = np.full(4 * n, 7.0, np.float32)
    pq, pi, pd, pc, po = (a.ctypes.data_as(C.c_void_p) for a in (q, idx, dist, cls, out))
    labels = synth.make_labels(n, 10)

    def err(rc_):
        return rc_, (L.fir_last_error().decode() if rc_ else "")

    def untouched():
        return (idx == 7).all() and (dist == 7.0).all() and (cls == 7).all() and (out == 7.0).all()

    QB, RANGE, K8, K32, NOLABELS = "qb < 0", "feature range [3,99) not inside [0,16)", "k=9 outside [1,8]", "k=33 outside [1,32]", \
        "gallery was created without class labels"
    with fir.Gallery(rows, labels, L2, 0) as g, fir.Gallery(rows, None, L2, 0) as bare:
        h, hb = g._h, bare._h
        top1 = lambda qb=4, a=0, b=0: err(L.fir_search_top1(h, pq, qb, a, b, pi, pd))
        topk = lambda qb=4, a=0, b=0, k=3: err(L.fir_search_topk(h, pq, qb, a, b, k, pi, pd))
        tcls = lambda qb=4, a=0, b=0, k=3, nc=10, hh=h: err(L.fir_search_top_classes(hh, pq, qb, a, b, nc, k, pc, pi, pd))
        rng = lambda qb=4, a=0, b=0: err(L.fir_range_distances(h, pq, qb, a, b, po))
        # one bad argument
        assert top1(qb=-1) == (FIR_ERR_ARG, QB) and top1(a=3, b=99) == (FIR_ERR_ARG, RANGE)
        assert topk(qb=-1) == (FIR_ERR_ARG, QB) and topk(a=3, b=99) == (FIR_ERR_ARG, RANGE) and topk(k=9) == (FIR_ERR_ARG, K8)
        assert topk(k=0) == (FIR_ERR_ARG, "k=0 outside [1,8]")
        assert tcls(qb=-1) == (FIR_ERR_ARG, QB) and tcls(a=3, b=99) == (FIR_ERR_ARG, RANGE) and tcls(k=33) == (FIR_ERR_ARG, K32)
        assert tcls(nc=0) == (FIR_ERR_ARG, "num_classes=0 outside [1,16777216]") and tcls(hh=hb) == (FIR_ERR_STATE, NOLABELS)
        assert rng(qb=-1) == (FIR_ERR_ARG, QB) and rng(a=3, b=99) == (FIR_ERR_ARG, RANGE)
        assert err(L.fir_search_top1(h, None, 4, 0, 0, pi, pd)) == (FIR_ERR_ARG, "NULL argument")
        # two: the first one checked is the one reported
        assert top1(qb=-1, a=3, b=99)[1] == QB and rng(qb=-1, a=3, b=99)[1] == QB
        assert topk(qb=-1, k=9)[1] == QB and topk(k=9, a=3, b=99)[1] == K8
        assert tcls(qb=-1, k=33)[1] == QB and tcls(k=33, hh=hb)[1] == K32 and tcls(a=3, b=99, hh=hb) == (FIR_ERR_STATE, NOLABELS)
        assert tcls(k=33, a=3, b=99)[1] == K32
        assert untouched()
        # nothing to do
        assert top1(qb=0) == (FIR_OK, "") and topk(qb=0) == (FIR_OK, "") and tcls(qb=0) == (FIR_OK, "") and rng(qb=0) == (FIR_OK, "")
        assert top1(qb=0, a=3, b=99)[0] == FIR_OK and topk(qb=0, a=3, b=99)[0] == FIR_OK and rng(qb=0, a=3, b=99)[0] == FIR_OK
        assert topk(qb=0, k=9) == (FIR_ERR_ARG, K8) and tcls(qb=0, a=3, b=99) == (FIR_ERR_ARG, RANGE)
        assert untouched()
        # and the handles still answer
        i1, _ = g.search_top1(q)
        ik, _ = g.search_topk(q, 3)
        assert np.array_equal(i1, ik[:, 0])
