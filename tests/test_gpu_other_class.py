"""fir_search_top1_other_class, the gallery self-join over it and fir_gallery_far_threshold on the device (include/fir_amd.h).
No expected value comes from the code under test: fir_range_distances on the same handle gives every row's distance bits (the
arithmetic the parity tests pin to the reference), other_class_ref masks them by class and takes the smallest packed key
(tests/test_other_class_formulation.py pins that to the oracle), and keys are compared as uint64 for equality -- no tolerance.
The threshold is oracle.get_threshold over those expected distances, bit for bit.
fir_gallery_set_tuning takes its wave count in whole workgroups of 4: "one and three" are 4 and 12 here."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import knn_select_ref as ks
import other_class_ref as ref
import scan_forms
import synth
from test_gpu_knn_select import host_keys

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, CHI2, KL = 0, 1, 2
ERR_ARG, ERR_STATE = -1, -5
F32, I32 = np.float32, np.int32
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
QBS = (1, 3, 8, 9, 17)
POISON = 0x5A5A5A5A5A5A5A5A


def runs_of_30(n):
    return (np.arange(n) // 30).astype(I32)


def permuted(n, classes, seed):
    return (synth.splitmix64(np.arange(n, dtype=np.uint64), seed) % np.uint64(classes)).astype(I32)


def exclusions(labels, qb, seed):
    """One excluded class per query: classes the gallery holds (so the mask bites), and every fifth one absent."""
    pick = (synth.splitmix64(np.arange(qb, dtype=np.uint64), seed) % np.uint64(labels.shape[0])).astype(np.int64)
    ex = labels[pick].copy()
    ex[4::5] = 1 << 30
    return ex


def want(g, q, labels, ex, start=0, end=0, off=0, dist=None):
    q = np.atleast_2d(q)
    if dist is None:
        dist = g.range_distances(q, start, end) if g.n else np.zeros((q.shape[0], 0), F32)
    return ref.expected_keys(dist, labels, ex, off)


def host_call(g, q, ex, start=0, end=0):
    qb = np.atleast_2d(q).shape[0]
    idx, dist = g.search_top1_other_class(q, ex, start, end)
    assert idx.shape == dist.shape == (qb,) and idx.dtype == np.int32 and dist.dtype == np.float32
    assert np.all(dist[idx < 0] == F32(100000.0))
    return host_keys(idx, dist)


class DevOut:
    """A poisoned key buffer with a tail of canary words, filled before anything else is queued."""

    def __init__(self, qb):
        self.qb = qb
        self.keys = torch.full((qb + 8,), POISON, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()

    def read(self):
        k = self.keys.cpu().numpy().view(np.uint64)
        assert np.all(k[self.qb:] == np.uint64(POISON))                       # nothing written past the end
        return k[: self.qb].copy()


def dev_call(g, qt, et, start=0, end=0, stream=None, out=None):
    if out is None:
        out = DevOut(qt.shape[0])
    g.search_top1_other_class_keys_dev(qt.data_ptr(), qt.shape[0], et.data_ptr(), out.keys.data_ptr(), start, end, stream=stream)
    if stream is None:
        g.sync()
    return out


def ranges_of(d):
    return [r for r in ((0, 0), (3, 61), (4, 5)) if r[1] <= d]


@pytest.mark.parametrize("d", (5, 64, 100))
@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_rows_ranges_metrics_and_batch_sizes(fir, metric, d):
    """The label guard at the tile edge (n around 64 and 128), masked chunks, part-full and several tiles per launch."""
    for n in (1, 63, 64, 65, 129, 1000):
        rows = synth.make_gallery(201 + n, n, d, metric)
        labels = runs_of_30(n) if n % 2 else permuted(n, 7, 203 + n)
        q, _ = synth.make_queries(205 + n, rows, max(QBS), metric)
        ex = exclusions(labels, max(QBS), 207 + n)
        with fir.Gallery(rows, labels, metric, 0) as g:
            for start, end in ranges_of(d):
                dist = g.range_distances(q, start, end)
                for qb in QBS:
                    got = host_call(g, q[:qb], ex[:qb], start, end)
                    assert np.array_equal(got, want(g, q[:qb], labels, ex[:qb], dist=dist[:qb])), (metric, n, d, start, end, qb)


@pytest.mark.parametrize("metric", (CHI2, KL))
def test_a_negative_gallery_value_takes_the_full_division_sequence(fir, metric):
    n, d, qb = 129, 64, 9
    rows = synth.make_gallery(211, n, d, metric)
    rows[77, 13] = F32(-0.001)
    labels = permuted(n, 5, 212)
    q, _ = synth.make_queries(213, rows, qb, metric)
    ex = exclusions(labels, qb, 214)
    with fir.Gallery(rows, labels, metric, 0) as g:
        assert g.value_range()[0] is False
        for start, end in ranges_of(d):
            assert np.array_equal(host_call(g, q, ex, start, end), want(g, q, labels, ex, start, end)), (metric, start, end)


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_every_instantiation_through_the_tuning(fir, metric):
    """queries_per_pass 1, 2, 4, 8 pick the tile (16 asks for the largest there is, 8); automatic wave counts, one workgroup and
    three: a wave then strides over several tiles. 17 queries: a launch of two tiles and a single query. 200 rows are few tiles (the
    one-query tile staged in LDS). Few means at most 4 * CUs tiles, so the gallery that is not few is sized from the device: one tile
    more than that and a part-full one, of short rows (65 637 x 64 on 256 CUs) -- there the one-query tile is the generic
    k_scan<1, m, 8, 6, 8, WPS, 0> (tests/scan_forms.py: OTHER_CLASS_GENERIC_ONE), and the test says so."""
    qb = 17
    many = (4 * fir.device_info()["cus"] + 1) * 64 + 37
    for n, d in ((200, 100), (many, 64)):
        rows = synth.make_gallery(221 + n, n, d, metric)
        labels = permuted(n, 11, 222)
        q, _ = synth.make_queries(223, rows, qb, metric)
        ex = exclusions(labels, qb, 224)
        with fir.Gallery(rows, labels, metric, 0) as g:
            expect = {r: want(g, q, labels, ex, *r) for r in ((0, 0), (3, 61))}
            seen = set()
            for qpp in (1, 2, 4, 8, 16):
                for waves in (0, 4, 12):
                    g.set_tuning(qpp, waves)
                    for r, e in expect.items():
                        assert np.array_equal(host_call(g, q, ex, *r), e), (metric, n, qpp, waves, r)
                        ld = g.last_dispatch()
                        assert ld["path"] == "scan" and ", 6, 8, " in ld["kernel"], ld
                        seen.add(ld["kernel"])
            g.set_tuning(-1, 0)
            assert np.array_equal(host_call(g, q[:1], ex[:1]), expect[0, 0][:1])
            seen.add(g.last_dispatch()["kernel"])
        if n == 200:
            assert any(k.startswith("fir::k_scan<1, %d, 16, 6, 8, " % metric) for k in seen), seen       # the few-tiles form
        else:
            assert scan_forms.OTHER_CLASS_GENERIC_ONE[metric] in seen, seen                                # the generic one-query form
            assert not any(k.startswith("fir::k_scan<1, %d, 16, 6, 8, " % metric) for k in seen), seen


def test_label_kinds(fir):
    n, d, qb = 1000, 64, 9
    rows = synth.make_gallery(231, n, d, L2)
    q, _ = synth.make_queries(232, rows, qb, L2)
    # all one class: every answer is -1 / 100000; another class excluded: plain top-1
    with fir.Gallery(rows, np.full(n, 7, I32), L2, 0) as g:
        idx, dist = g.search_top1_other_class(q, 7)
        assert np.all(idx == -1) and np.all(dist == F32(100000.0))
        i1, d1 = g.search_top1(q)
        assert np.array_equal(host_call(g, q, 8), host_keys(i1, d1))
    # negative and extreme labels are labels like any other, as exclusions too
    labels = permuted(n, 6, 233)
    labels[labels == 0] = -1
    labels[labels == 1] = I32_MIN
    labels[labels == 2] = I32_MAX
    with fir.Gallery(rows, labels, L2, 0) as g:
        dist = g.range_distances(q)
        for ex in (-1, I32_MIN, I32_MAX, 3, np.array([-1, I32_MIN, I32_MAX, 3, 4, 5, -2, 0, I32_MAX], I32)):
            got = host_call(g, q, ex)
            assert np.array_equal(got, want(g, q, labels, ex, dist=dist)), ex
            idx = ks.unpack(got)[0]
            assert np.all(labels[idx] != np.broadcast_to(np.asarray(ex, I32), (qb,)))
        # an exclusion no row carries: fir_search_top1_keys_dev's keys bit for bit
        qt = torch.from_numpy(q).to(DEV)
        et = torch.full((qb,), 12345, dtype=torch.int32, device=DEV)
        top1 = torch.full((qb,), POISON, dtype=torch.int64, device=DEV)
        g.search_top1_keys_dev(qt.data_ptr(), qb, top1.data_ptr())
        g.sync()
        assert np.array_equal(dev_call(g, qt, et).read(), top1.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_ties_nan_rows_cutoff_and_row_offset(fir, metric):
    n, d = 300, 64
    rows = synth.make_gallery(241, n, d, metric)
    labels = runs_of_30(n)
    q, _ = synth.make_queries(242, rows, 8, metric)
    # query 0 = row 40 (class 1), copied to row 55 (class 1) and to rows 100 and 250 (classes 3 and 8)
    rows[55] = rows[40]
    rows[100] = rows[40]
    rows[250] = rows[40]
    q[0] = rows[40]
    rows[101, 5] = np.nan                                                      # a NaN row: never an answer
    q[1] = rows[101]
    q[1, 5] = rows[102, 5]
    big = rows.copy()
    big[200:] *= F32(1.0e7)                                                    # rows scaled so that dist >= 100000 (L2), or simply far
    ex = np.array([1, 3, 6, 7, 9, 0, 1, 2], I32)
    for gal in (rows, big):
        with fir.Gallery(gal, labels, metric, 0) as g:
            for off in (0, 1 << 20):
                g.set_row_offset(off)
                dist = g.range_distances(q)
                got = host_call(g, q, ex)
                assert np.array_equal(got, want(g, q, labels, ex, off=off, dist=dist)), (metric, off)
                idx = ks.unpack(got)[0]
                if gal is rows:
                    assert idx[0] == 100 + off                                 # own class excluded: the LOWEST copy of another class
                    assert ks.unpack(host_call(g, q[:1], 3))[0][0] == 40 + off  # class 3 excluded: the lowest copy of all
                assert not np.any(idx == 101 + off)
            if gal is big and metric == L2:
                g.set_row_offset(0)
                assert np.all(g.range_distances(q[2:3])[0, 200:] >= F32(100000.0))
                assert np.all(g.search_top1_other_class(q, ex)[0] < 200)
    if metric == L2:
        # every row of another class at or beyond the cut-off: no answer, whatever lies inside the own class
        far = rows * F32(1.0e7)
        far[30:60] = rows[30:60]
        with fir.Gallery(far, labels, L2, 0) as g:
            idx, dd = g.search_top1_other_class(q[:1], 1)
            assert idx[0] == -1 and dd[0] == F32(100000.0)
            assert g.search_top1_other_class(q[:1], 2)[0][0] == 40


def test_device_call_streams_and_canaries(fir):
    n, d, qb = 1000, 100, 17
    rows = synth.make_gallery(251, n, d, L2)
    labels = permuted(n, 9, 252)
    q, _ = synth.make_queries(253, rows, 2 * qb, L2)
    ex = exclusions(labels, 2 * qb, 254)
    qt, et = torch.from_numpy(q).to(DEV), torch.from_numpy(ex).to(DEV)
    with fir.Gallery(rows, labels, L2, 0) as g:
        expect = want(g, q, labels, ex)
        expect_r = want(g, q, labels, ex, 3, 61)
        assert np.array_equal(dev_call(g, qt[:qb], et[:qb]).read(), expect[:qb])
        # a caller's stream
        st = torch.cuda.Stream()
        out = dev_call(g, qt[:qb], et[:qb], 3, 61, stream=st.cuda_stream)
        st.synchronize()
        assert np.array_equal(out.read(), expect_r[:qb])
        # two calls back to back on different streams: both use the handle's scratch, the second waits for the first
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1, o2 = DevOut(2 * qb), DevOut(qb)
        dev_call(g, qt, et, stream=s1.cuda_stream, out=o1)
        dev_call(g, qt[qb:], et[qb:], 3, 61, stream=s2.cuda_stream, out=o2)
        g.sync()
        s1.synchronize()
        s2.synchronize()
        assert np.array_equal(o1.read(), expect) and np.array_equal(o2.read(), expect_r[qb:])
        # qb == 0: nothing to do, nothing written
        o0 = DevOut(4)
        g.search_top1_other_class_keys_dev(qt.data_ptr(), 0, et.data_ptr(), o0.keys.data_ptr())
        g.sync()
        assert np.all(o0.read() == np.uint64(POISON))


def test_argument_errors(fir):
    n, d = 100, 16
    rows = synth.make_gallery(261, n, d, L2)
    q = rows[:3].copy()
    labels = runs_of_30(n)
    L = fir.lib()
    p = lambda a: a.ctypes.data_as(fir.capi._vp)
    ex, idx, dist = np.zeros(3, I32), np.zeros(3, I32), np.zeros(3, F32)

    def err(rc, code, text):
        assert rc == code and text in L.fir_last_error().decode(), (rc, L.fir_last_error())

    with fir.Gallery(rows, labels, L2, 0) as g:
        h = g._h
        err(L.fir_search_top1_other_class(None, p(q), 3, 0, 0, p(ex), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_other_class(h, None, 3, 0, 0, p(ex), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_other_class(h, p(q), 3, 0, 0, None, p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_other_class(h, p(q), 3, 0, 0, p(ex), None, p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_other_class(h, p(q), 3, 0, 0, p(ex), p(idx), None), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_other_class(h, p(q), -1, 0, 0, p(ex), p(idx), p(dist)), ERR_ARG, "qb < 0")
        err(L.fir_search_top1_other_class(h, p(q), 3, 5, 5, p(ex), p(idx), p(dist)), ERR_ARG, "feature range [5,5) not inside [0,16)")
        err(L.fir_search_top1_other_class(h, p(q), 0, 0, 17, p(ex), p(idx), p(dist)), ERR_ARG, "feature range [0,17)")   # the range before qb == 0
        assert L.fir_search_top1_other_class(h, None, 0, 0, 0, None, p(idx), p(dist)) == 0                                  # nothing to do
        err(L.fir_search_top1_other_class_keys_dev(h, p(q), 3, 0, 0, p(ex), None, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_other_class(h, 0, 0, None, p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_other_class_keys_dev(h, 90, 11, 0, 0, p(idx), None), ERR_ARG, "rows [90,101) not inside [0,100)")
        err(L.fir_gallery_other_class_keys_dev(h, -1, 2, 0, 0, p(idx), None), ERR_ARG, "not inside")
        assert L.fir_gallery_other_class_keys_dev(h, 100, 0, 0, 0, p(idx), None) == 0
        thr = np.zeros(1, F32)
        err(L.fir_gallery_far_threshold(h, 0, 0, 0.5, None, None, None, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_far_threshold(h, 0, 0, float("nan"), p(thr), None, None, None), ERR_ARG, "false_accept_rate")
        err(L.fir_gallery_far_threshold(h, 0, 0, -0.25, p(thr), None, None, None), ERR_ARG, "false_accept_rate")
        err(L.fir_gallery_far_threshold(h, 0, 0, 1.0, p(thr), None, None, None), ERR_ARG, "false_accept_rate")
        err(L.fir_gallery_far_threshold(h, 3, 3, 0.5, p(thr), None, None, None), ERR_ARG, "feature range")
    with fir.Gallery(rows, None, L2, 0) as g:                                   # no labels: FIR_ERR_STATE, before the range
        h = g._h
        qt = torch.from_numpy(q).to(DEV)
        et = torch.zeros(3, dtype=torch.int32, device=DEV)
        keys = torch.zeros(3, dtype=torch.int64, device=DEV)
        err(L.fir_search_top1_other_class(h, p(q), 3, 9, 9, p(ex), p(idx), p(dist)), ERR_STATE, "without class labels")
        err(L.fir_search_top1_other_class_keys_dev(h, qt.data_ptr(), 3, 0, 0, et.data_ptr(), keys.data_ptr(), None), ERR_STATE, "without class labels")
        err(L.fir_gallery_other_class(h, 0, 0, p(idx), p(dist)), ERR_STATE, "without class labels")
        err(L.fir_gallery_other_class_keys_dev(h, 0, 3, 0, 0, keys.data_ptr(), None), ERR_STATE, "without class labels")
        err(L.fir_gallery_far_threshold(h, 0, 0, 0.5, p(thr), None, None, None), ERR_STATE, "without class labels")


@pytest.mark.parametrize("d,rng", ((64, (0, 0)), (100, (0, 64))))
def test_routed_form_at_its_smallest_gated_shape(fir, d, rng):
    """Under a caller's threshold a host batch goes through the class form of the matrix cores and a pick: the scan form's keys, and
    the dispatch record says so. One label outside [0, 16777216) keeps the gallery on the scan."""
    n, qb = 4099, 130
    rows = synth.make_gallery(271 + d, n, d, L2)
    labels = permuted(n, 37, 272)
    rows[4000] = rows[12]
    q, _ = synth.make_queries(273, rows, qb, L2)
    q[1] = rows[12]
    ex = exclusions(labels, qb, 274)
    ex[1] = labels[12]
    with fir.Gallery(rows, labels, L2, 0) as g:
        expect = want(g, q, labels, ex, *rng)
        g.set_large_batch_mfma(0)
        scan = host_call(g, q, ex, *rng)
        assert g.last_dispatch()["path"] == "scan"
        g.set_large_batch_mfma(1)
        routed = host_call(g, q, ex, *rng)
        assert g.last_dispatch()["path"] == "mfma", g.last_dispatch()
        assert np.array_equal(scan, expect) and np.array_equal(routed, expect)
        # the device call always takes the scan form
        out = dev_call(g, torch.from_numpy(q).to(DEV), torch.from_numpy(ex).to(DEV), *rng)
        assert np.array_equal(out.read(), expect) and g.last_dispatch()["path"] == "scan"
    labels2 = labels.copy()
    labels2[2000] = -1
    with fir.Gallery(rows, labels2, L2, 0) as g:
        g.set_large_batch_mfma(1)
        got = host_call(g, q, ex, *rng)
        assert g.last_dispatch()["path"] == "scan", g.last_dispatch()
        assert np.array_equal(got, want(g, q, labels2, ex, *rng))


def test_automatic_routing_starts_at_128_queries_over_65536_rows(fir):
    n, d = 66000, 64
    rows = synth.make_gallery(275, n, d, L2)
    labels = permuted(n, 6600, 276)
    q, _ = synth.make_queries(277, rows, 130, L2)
    ex = exclusions(labels, 130, 278)
    with fir.Gallery(rows, labels, L2, 0) as g:
        expect = want(g, q, labels, ex)
        assert np.array_equal(host_call(g, q, ex), expect) and g.last_dispatch()["path"] == "mfma", g.last_dispatch()
        assert np.array_equal(host_call(g, q[:127], ex[:127]), expect[:127]) and g.last_dispatch()["path"] == "scan"
        assert np.array_equal(host_call(g, q, ex, 3, 61), want(g, q, labels, ex, 3, 61)) and g.last_dispatch()["path"] == "scan"
        g.set_large_batch_mfma(0)
        assert np.array_equal(host_call(g, q, ex), expect) and g.last_dispatch()["path"] == "scan"


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_self_join_against_the_reference_statistic(fir, metric):
    n, d = 1000, 64
    rows = synth.make_gallery(281, n, d, metric)
    rows[700] = rows[3]
    labels = runs_of_30(n)
    with fir.Gallery(rows, labels, metric, 0) as g:
        dist = g.range_distances(rows)                                        # dist[i, j]: row i is the query
        expect = ref.self_join_keys(dist, labels)
        idx, dd = g.other_class()
        assert np.array_equal(host_keys(idx, dd), expect), metric
        assert idx[3] == 700 and idx[700] == 3 and np.all(labels[idx] != labels)
        # a window on a caller's stream
        out = DevOut(70)
        st = torch.cuda.Stream()
        g.other_class_keys_dev(60, 70, out.keys.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert np.array_equal(out.read(), expect[60:130])
        g.set_row_offset(1 << 20)
        out = DevOut(70)
        g.other_class_keys_dev(60, 70, out.keys.data_ptr(), 3, 61)
        g.sync()
        assert np.array_equal(out.read(), ref.self_join_keys(g.range_distances(rows[60:130], 3, 61), labels, row0=60, row_offset=1 << 20))


def test_self_join_across_the_block_seam(fir):
    n, d = 8200, 16
    rows = synth.make_gallery(291, n, d, L2)
    labels = permuted(n, 40, 292)
    with fir.Gallery(rows, labels, L2, 0) as g:
        idx, dd = g.other_class()
        got = host_keys(idx, dd)
        for lo in range(0, n, 2050):                                          # the expected keys in four slabs of distances
            dist = g.range_distances(rows[lo:lo + 2050])
            assert np.array_equal(got[lo:lo + 2050], ref.self_join_keys(dist, labels, row0=lo)), lo


def test_threshold_is_get_thresholds(fir, oracle):
    n, d = 1000, 64
    rows = synth.make_gallery(301, n, d, L2)
    labels = runs_of_30(n)
    with fir.Gallery(rows, labels, L2, 0) as g:
        dists = ref.keys_to_dists(ref.self_join_keys(g.range_distances(rows), labels))
        assert dists.shape[0] == n
        for rate in (0.0, 0.01, 0.05, 0.5, 0.999):
            thr, lo, hi, cnt = g.far_threshold(rate)
            assert cnt == n and lo.view(np.uint32) == dists.min().view(np.uint32) and hi.view(np.uint32) == dists.max().view(np.uint32)
            assert thr.view(np.uint32) == oracle.get_threshold(dists, rate).view(np.uint32), rate
            assert thr.view(np.uint32) == F32(ref.threshold(dists, rate)[0]).view(np.uint32)
        for rate in (1.0, float("nan")):
            with pytest.raises(fir.FirError) as e:
                g.far_threshold(rate)
            assert e.value.code == ERR_ARG
    # a row without a row of another class below the cut-off is not counted: row 199, alone in its class and far from everything
    rows2 = rows[:200].copy()
    rows2[199] *= F32(1.0e7)
    labels2 = np.zeros(200, I32)
    labels2[150:] = 1
    labels2[199] = 2
    with fir.Gallery(rows2, labels2, L2, 0) as g:
        for rng in ((0, 0), (3, 61)):
            keys = ref.self_join_keys(g.range_distances(rows2, *rng), labels2)
            assert keys[199] == ref.KEY_NONE and (keys[:199] != ref.KEY_NONE).all()
            dists = ref.keys_to_dists(keys)
            thr, lo, hi, cnt = g.far_threshold(0.05, *rng)
            assert cnt == 199 and thr.view(np.uint32) == oracle.get_threshold(dists, 0.05).view(np.uint32)
            assert lo.view(np.uint32) == dists.min().view(np.uint32) and hi.view(np.uint32) == dists.max().view(np.uint32)
        idx, dd = g.other_class()
        assert idx[199] == -1 and dd[199] == F32(100000.0)
    with fir.Gallery(rows2, np.full(200, 4, I32), L2, 0) as g:                 # one class: nothing to count
        with pytest.raises(fir.FirError) as e:
            g.far_threshold(0.01)
        assert e.value.code == ERR_STATE


def test_sharded_handle_gives_the_unsharded_keys(fir):
    n, d, qb = 1000, 64, 17
    rows = synth.make_gallery(311, n, d, L2)
    labels = permuted(n, 9, 312)
    q, _ = synth.make_queries(313, rows, qb, L2)
    ex = exclusions(labels, qb, 314)
    with fir.Gallery(rows, labels, L2, 0) as g:
        expect = want(g, q, labels, ex)
        expect_r = want(g, q, labels, ex, 3, 61)
    with fir.ShardedGallery(rows, labels, fir.METRIC_L2, devices=[0], shards_per_device=3) as s:
        idx, dist = s.search_top1_other_class(q, ex)
        assert np.array_equal(host_keys(idx, dist), expect)
        idx, dist = s.search_top1_other_class(q, ex, 3, 61)
        assert np.array_equal(host_keys(idx, dist), expect_r)
    with fir.ShardedGallery(rows, None, fir.METRIC_L2, devices=[0], shards_per_device=3) as s:
        with pytest.raises(fir.FirError) as e:
            s.search_top1_other_class(q, ex)
        assert e.value.code == ERR_STATE


def test_shim_driver_threshold_is_the_oracles(tmp_path, oracle):
    """host/far_driver: fir::other_class_distances and fir::far_threshold over a feature file, against the oracle on the same file."""
    driver = os.path.join(ROOT, "fast-image-recognition_amd", "host", "far_driver")
    d, per, ncls = 64, 60, 5
    names, classes, feats = [], [], []
    centers = synth.uniform01(ncls * d, 5).reshape(ncls, d)
    for k in range(per * ncls):
        c = k % ncls
        names.append(f"/data/cls{c}/img{k}.jpg")
        classes.append(f"class_{c}")
        feats.append(0.6 * centers[c] + synth.uniform01(d, 1000 + k))
    path = str(tmp_path / "features.txt")
    synth.write_feature_file(path, names, classes, np.array(feats, F32))
    out = subprocess.run([driver, path, str(d), "0.05"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    rows, cls, nc = oracle.load_images(path, d, 0)
    assert got["images"] == rows.shape[0] == per * ncls == 300 and nc == ncls
    dist = np.stack([oracle.all_distances(rows, r, 0, d, 0) for r in rows])
    dists = ref.keys_to_dists(ref.self_join_keys(dist, cls))
    assert got["counted"] == dists.shape[0] == 300
    assert np.array_equal(np.array(got["dists"], F32).view(np.uint32), dists.view(np.uint32))
    assert F32(got["threshold"]).view(np.uint32) == oracle.get_threshold(dists, 0.05).view(np.uint32)
