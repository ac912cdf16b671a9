"""fir_twd_conventional's matrix-core batch form (type 0, L2; csrc/fir_twd_batch.h): class and reliable/unreliable verdict of every
query must be the oracle's (ConventionalTWDClassifier::recognize, ImageTesting.cpp:108-186) and those of the launch-per-stage form
the library had before -- the same call on a handle with set_large_batch_mfma(0) --, and fir_twd_last_mfma must say what the call
did: how many queries the form took, how many stage 1 found reliable, how many the matrix-core second stage answered, and how many
went back to the launch-per-stage form (threshold band, second stage not certified).

The synthetic rows are so close to each other that every posterior ratio sits near 0.2: rows and queries are multiplied by a power
of two (exact in float32), after which the thresholds 0.24 and 0.5 of golden_cases.TWD_CONVENTIONAL give both outcomes."""
import ctypes as C
import functools

import numpy as np
import pytest

import golden_cases as gc
import synth

pytestmark = pytest.mark.gpu

L2, CHI2 = gc.L2, gc.CHI2
FIR_ERR_ARG = -1
SENTINEL = 0x5A5A5A5A
# name -> (seed, n, d, classes, reduced_features_count, queries, scale)
SHAPES = {"3000x256": (13, 3000, 256, 37, 64, 130, 4), "4000x320": (31, 4000, 320, 101, 128, 150, 8)}


@functools.lru_cache(maxsize=None)
def shape(name):
    seed, n, d, ncls, red, qb, scale = SHAPES[name]
    rows, cls, _, _ = gc.twd_case(seed=seed, n=n, d=d, n_classes=ncls)
    q, _ = synth.make_queries(seed, rows, qb, L2, noise=0.4)
    rows, q = rows * np.float32(scale), q * np.float32(scale)
    for a in (rows, cls, q):
        a.setflags(write=False)
    return rows, cls, q, ncls, red


_EXPECTED = {}


def expected(oracle, name, typ, th, red=None):
    """The oracle's verdicts for one of SHAPES, computed once per (shape, type, threshold, reduced)."""
    rows, cls, q, ncls, red0 = shape(name)
    key = (name, typ, th, red or red0)
    if key not in _EXPECTED:
        e = [oracle.twd_conventional(rows, cls, qi, ncls, typ, th, red or red0) for qi in q]
        _EXPECTED[key] = ([x[0] for x in e], [x[1] for x in e])
    return _EXPECTED[key]


def call(g, q, ncls, typ, th, red):
    c, u = g.twd_conventional(q, ncls, typ, th, red)
    return list(c), list(u)


def today(fir, rows, cls, q, ncls, typ, th, red, metric=L2):
    """(verdicts, dispatch record) of the form the library had before: the same call with the matrix cores switched off."""
    with fir.Gallery(rows, cls, metric, 0) as g:
        g.set_large_batch_mfma(0)
        out = call(g, q, ncls, typ, th, red)
        assert g.twd_last_mfma()["queries"] == 0
        return out, g.twd_last_dispatch()


def raw_call(fir, g, q, ncls, typ, th, red, want_unreliable=True, class_out=True):
    """The C call itself with guard words behind both outputs: (rc, classes, unreliable or None)."""
    q = np.ascontiguousarray(q, np.float32)
    qb = q.shape[0]
    cls = np.full(qb + 8, SENTINEL, np.int32)
    unrel = np.full(qb + 8, SENTINEL, np.int32)
    rc = fir.lib().fir_twd_conventional(g._h, q.ctypes.data_as(C.c_void_p), qb, ncls, typ, th, red,
                                        cls.ctypes.data_as(C.c_void_p) if class_out else None,
                                        unrel.ctypes.data_as(C.c_void_p) if want_unreliable else None)
    assert np.all(cls[qb:] == SENTINEL) and np.all(unrel[qb:] == SENTINEL), "written past the outputs"
    if not want_unreliable:
        assert np.all(unrel == SENTINEL)
    return rc, list(cls[:qb]), list(unrel[:qb]) if want_unreliable else None


def routed_record(rep, staged_batches=0):
    assert rep["classifier"] == "conventional" and rep["planned_fused"] == 0 and rep["fused_launches"] == 0 and rep["kernel"] == "", rep
    assert rep["staged_batches"] == staged_batches, rep


@pytest.mark.parametrize("name", list(SHAPES))
def test_both_outcomes_equal_the_oracle_and_todays_form(fir, oracle, name):
    rows, cls, q, ncls, red = shape(name)
    qb = q.shape[0]
    with fir.Gallery(rows, cls, L2, 0) as g:
        g.set_large_batch_mfma(64)
        for th in (0.24, 0.5):                               # (d = 320: two prefix states, [0, 128) and [0, 256); two calls back to back)
            got = call(g, q, ncls, 0, th, red)
            mm = g.twd_last_mfma()
            exp = expected(oracle, name, 0, th)
            assert got == exp, th
            assert got == today(fir, rows, cls, q, ncls, 0, th, red)[0], th
            reliable = exp[1].count(0)
            assert 0 < reliable < qb
            assert mm == {"queries": qb, "reliable": reliable, "second_stage": qb - reliable, "band": 0, "uncertified": 0, "class_scan": 0}, (th, mm)
            routed_record(g.twd_last_dispatch())
        c1, u1 = call(g, q[5:6], ncls, 0, 0.24, red)          # one query: below the threshold, the one-launch or the staged form
        rep = g.twd_last_dispatch()
        assert g.twd_last_mfma()["queries"] == 0
        assert rep["fused_launches"] >= 1 if rep["planned_fused"] else rep["staged_batches"] == 1, rep
        exp = expected(oracle, name, 0, 0.24)
        assert (c1[0], u1[0]) == (exp[0][5], exp[1][5])


def test_beyond_65536_rows_and_the_list_capacity(fir, oracle):
    n, d, ncls, qb, red, th = 66000, 256, 1000, 200, 64, 0.24
    rows = synth.make_gallery(77, n, d, L2)
    q, _ = synth.make_queries(77, rows, qb, L2, noise=0.4)
    rows, q = rows * np.float32(4), q * np.float32(4)
    cls = synth.make_labels(n, ncls)
    with fir.Gallery(rows, cls, L2, 0) as g:
        g.set_large_batch_mfma(64)
        got = call(g, q, ncls, 0, th, red)
        mm = g.twd_last_mfma()
    with fir.Gallery(rows, cls, L2, 0) as g:                 # the automatic rule: >= 128 queries over >= 65 536 rows
        auto = call(g, q, ncls, 0, th, red)
        assert g.twd_last_mfma()["queries"] == qb
        few = call(g, q[:127], ncls, 0, th, red)
        assert g.twd_last_mfma()["queries"] == 0
    assert auto == got and few == (got[0][:127], got[1][:127])
    assert mm["queries"] == qb and mm["reliable"] + mm["second_stage"] + mm["band"] + mm["uncertified"] == qb, mm
    assert mm["reliable"] <= got[1].count(0) <= mm["reliable"] + mm["band"], mm
    assert got == today(fir, rows, cls, q, ncls, 0, th, red)[0]
    for i in (0, qb // 2, qb - 1):
        assert (got[0][i], got[1][i]) == oracle.twd_conventional(rows, cls, q[i], ncls, 0, th, red), i


@pytest.mark.parametrize("why", ["type 1", "type 2", "reduced 32", "reduced 50", "chi-square", "threshold 0", "no shadow copies", "label out of range",
                                 "automatic, 3000 rows"])
def test_calls_that_are_not_routed(fir, oracle, why):
    rows, cls, q, ncls, red = shape("3000x256")
    typ, th, metric = 0, 0.24, L2
    if why.startswith("type"):
        typ = int(why[-1])
        th = {1: 0.003, 2: 0.7}[typ]
    if why.startswith("reduced"):
        red = int(why.split()[1])
    if why == "chi-square":
        metric = CHI2
    if why == "label out of range":
        cls = cls.copy()
        cls[1500] = ncls + 3
    with fir.Gallery(rows, cls, metric, 0) as g:
        if not why.startswith("automatic"):
            g.set_large_batch_mfma(0 if why == "threshold 0" else 64)
        if why == "no shadow copies":
            g.set_shadow_copies(fir.SHADOW_NONE)
        got = call(g, q, ncls, typ, th, red)
        assert g.twd_last_mfma() == {"queries": 0, "reliable": 0, "second_stage": 0, "band": 0, "uncertified": 0, "class_scan": 0}
        rep = g.twd_last_dispatch()
    was, was_rep = today(fir, rows, cls, q, ncls, typ, th, red, metric)
    assert got == was and rep == was_rep, (rep, was_rep)
    if why != "label out of range":                          # (the oracle indexes its posteriors by label)
        e = [oracle.twd_conventional(rows, cls, qi, ncls, typ, th, red, metric) for qi in q]
        assert got == ([x[0] for x in e], [x[1] for x in e])


def test_duplicated_rows_are_not_certified_and_go_to_the_staged_form(fir, oracle):
    """Twelve copies of one row at scattered indices, in several classes: for a query next to them stage 1 sees classes whose
    nearest rows are bit-identical (max_probab <= 0.2: unreliable) and the eight nominated rows of stage 2 are all ties."""
    rows, cls, q, ncls, red = shape("3000x256")
    rows, q = rows.copy(), q.copy()
    copies = [17, 101, 333, 640, 900, 1203, 1500, 1777, 2048, 2222, 2600, 2999]
    for r in copies:
        rows[r] = rows[17]
    assert len({int(cls[r]) for r in copies}) >= 5
    q[3] = rows[17]
    q[10] = rows[17] * np.float32(1.001)
    q[77] = rows[17] * np.float32(0.999)
    th = 0.24
    e = [oracle.twd_conventional(rows, cls, qi, ncls, 0, th, red) for qi in q]
    exp = ([x[0] for x in e], [x[1] for x in e])
    # "those queries": the unreliable ones whose nearest row over [0, 256) is one of the copies
    those = [i for i, qi in enumerate(q) if exp[1][i] == 1 and int(np.argmin(oracle.all_distances(rows, qi, 0, 256, L2))) in copies]
    assert {3, 10, 77} <= set(those)
    with fir.Gallery(rows, cls, L2, 0) as g:
        g.set_large_batch_mfma(64)
        got = call(g, q, ncls, 0, th, red)
        mm = g.twd_last_mfma()
        routed_record(g.twd_last_dispatch(), staged_batches=1)
    assert got == exp
    assert [got[0][i] for i in (3, 10, 77)] == [int(cls[17])] * 3            # the first of the copies in row order
    assert mm["uncertified"] == len(those) and mm["band"] == 0 and mm["class_scan"] == 0, mm
    assert mm["queries"] == len(q) and mm["second_stage"] == exp[1].count(1) - len(those) and mm["reliable"] == exp[1].count(0), mm


def test_a_threshold_inside_the_band_goes_to_the_staged_form(fir, oracle):
    rows, cls, q, ncls, red = shape("3000x256")
    d1 = oracle.all_distances(rows, q[7], 0, red, L2).astype(np.float64)
    cmin = np.full(ncls, np.inf)
    np.minimum.at(cmin, cls, d1)
    top5 = np.sort(np.exp(-100.0 * cmin))[::-1][:5]
    th = float(np.exp(-100.0 * d1.min()) / top5.sum())           # query 7's max_probab, to a few 2^-53
    with fir.Gallery(rows, cls, L2, 0) as g:
        g.set_large_batch_mfma(64)
        got = call(g, q, ncls, 0, th, red)
        mm = g.twd_last_mfma()
        routed_record(g.twd_last_dispatch(), staged_batches=1)
    assert mm["band"] >= 1 and mm["queries"] == len(q), mm
    assert got == today(fir, rows, cls, q, ncls, 0, th, red)[0]


def test_hostile_values(fir):
    rows, cls, q, ncls, red = shape("3000x256")
    q = q.copy()                                                   # 130 queries: a ragged batch
    q[1, 7] = np.nan
    q[2, 5] = np.inf
    q[4] = 0
    rows2 = rows.copy()
    rows2[77] = np.nan
    rows2[1234, 40] = np.nan
    for rr in (rows, rows2):
        for th in (0.24, 0.5):
            was = today(fir, rr, cls, q, ncls, 0, th, red)[0]
            with fir.Gallery(rr, cls, L2, 0) as g:
                g.set_large_batch_mfma(64)
                rc, c, u = raw_call(fir, g, q, ncls, 0, th, red)
                assert rc == 0 and (c, u) == was, th
                assert g.twd_last_mfma()["queries"] == len(q)
                rc, c, u = raw_call(fir, g, q, ncls, 0, th, red, want_unreliable=False)
                assert rc == 0 and u is None and c == was[0], th


def test_row_offset_leaves_the_classes_unchanged(fir, oracle):
    rows, cls, q, ncls, red = shape("3000x256")
    with fir.Gallery(rows, cls, L2, 0) as g:
        g.set_row_offset(1000)
        g.set_large_batch_mfma(64)
        got = call(g, q, ncls, 0, 0.24, red)
        mm = g.twd_last_mfma()
    exp = expected(oracle, "3000x256", 0, 0.24)
    assert got == exp
    assert mm["queries"] == len(q) and mm["reliable"] == exp[1].count(0) and mm["second_stage"] == exp[1].count(1), mm


def test_argument_errors_come_first_and_read_as_before(fir):
    rows, cls, q, ncls, red = shape("3000x256")

    def message(g, *a):
        with pytest.raises(fir.FirError) as e:
            g.twd_conventional(*a)
        return e.value.code, str(e.value)

    bad = [(q, 4, 0, 0.24, red), (q, 7681, 0, 0.24, red), (q, ncls, 3, 0.24, red), (q, ncls, 0, 0.24, 0), (q, ncls, 0, 0.24, 256)]
    with fir.Gallery(rows, cls, L2, 0) as g, fir.Gallery(rows, cls, L2, 0) as g0:
        g.set_large_batch_mfma(64)
        g0.set_large_batch_mfma(0)
        for a in bad:
            assert message(g, *a) == message(g0, *a)
            assert message(g, *a)[0] == FIR_ERR_ARG
        assert raw_call(fir, g, q, ncls, 0, 0.24, red, class_out=False)[0] == FIR_ERR_ARG
        assert g.twd_last_mfma()["queries"] == 0 and g.twd_last_dispatch()["classifier"] is None      # nothing ran, nothing was recorded
        out = (C.c_int64 * 6)()
        assert fir.lib().fir_twd_last_mfma(None, out) == FIR_ERR_ARG
        assert fir.lib().fir_twd_last_mfma(g._h, None) == FIR_ERR_ARG
    with fir.Gallery(rows, None, L2, 0) as g:
        g.set_large_batch_mfma(64)
        with pytest.raises(fir.FirError):
            g.twd_conventional(q, ncls, 0, 0.24, red)                 # no labels
    with fir.Gallery(np.ascontiguousarray(rows[:, :128]), cls, L2, 0) as g:
        g.set_large_batch_mfma(64)
        with pytest.raises(fir.FirError):
            g.twd_conventional(np.ascontiguousarray(q[:, :128]), ncls, 0, 0.24, 64)      # d < 256
