"""The sub-range scans -- the twelve k_scan_subranges rows of kScanTable (csrc/fir_capi.hip), the only scan family whose numbers no
public call returns -- slot by slot against the oracle, and the three-way-decision calls they alone answer: every KL call.

The tables are read through the library's two internal entries, fir_subrange_distances_dev_ (the proposed classifier's chunks) and
fir_split_distances_dev_ (the conventional classifier's two stages), over torch device buffers with 64 canary words in front and
behind; fir_gallery_last_subrange_kernel_ names the kernel of the most recent one-pass launch, "" after the range-by-range branch.
Every slot out[(ci * qb + q) * n + row] is oracle.all_distances over sub-range ci: L2 and chi-square bit for bit (NaN where the
oracle has NaN), KL within the one tolerance of tests/kl_tolerance.py -- and bit for bit what fir_range_distances gives over the
same sub-range.

  a  every row by name: 1, 2, 3, 4, 5, 8 queries -> tiles of 1, 2, 4, 4, 8, 8; 9 and 11 queries are launches of 8 + 1 and 8 + 3
  b  gallery edges: 1, 63, 64, 65, 997 rows; a copy of a query, rows one ulp apart, NaN, a denormal, negative values, zeros
  c  feature ranges: one-pass steps and starts (a start that is a multiple of 4 and not of 32 included), their range-by-range twins
  d  the split form: both halves, each divided by its own feature count; one pass and two range passes
  e  more tiles than waves: a wave walks several tiles
  f  state: append across a tile seam, repeated calls, a caller's stream
  g  three-way decisions on KL galleries (always staged): verdicts == twd_walk over the DEVICE's tables (integers), tables within
     the KL tolerance of the oracle's; tests/test_twd_walk_formulation.py pins the walk to the oracle. L2 / chi-square staged once each."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scan_forms as sf
import synth
import twd_walk
from edge_gallery import NQ, edge_gallery
from kl_tolerance import bits, kl_bound
from scan_forms import CHI2, KL, L2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
METRICS = (L2, CHI2, KL)
PAD = 64
CANARY = 0x5A5A5A5A                     # as a float 1.5e16: no distance of these galleries
TILE_OF = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8}
SEEN, RAN = set(), set()


# ---- the internal entries -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _entries(path):
    lib = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    lib.fir_subrange_distances_dev_.restype = C.c_int
    lib.fir_subrange_distances_dev_.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    lib.fir_split_distances_dev_.restype = C.c_int
    lib.fir_split_distances_dev_.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.fir_gallery_last_subrange_kernel_.restype = C.c_char_p
    lib.fir_gallery_last_subrange_kernel_.argtypes = [vp]
    return lib


def last_kernel(fir, g):
    return _entries(fir.lib_path()).fir_gallery_last_subrange_kernel_(g._h).decode()


def _run(g, q, nsub, launch, stream=None):
    """One call into a poisoned buffer: [nsub, qb, n] float32 once the canaries on both sides are found untouched. stream: a torch
    stream -- the call is queued on it and the table is read by a copy on the same stream, with no other synchronisation."""
    q = np.array(q, F32)                                 # (a writable copy: torch takes no read-only arrays)
    qb, n = q.shape[0], g.n
    slots = nsub * qb * n
    qt = torch.from_numpy(q).to(DEV)
    buf = torch.full((PAD + slots + PAD,), CANARY, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    rc = launch(qt.data_ptr(), buf.data_ptr() + 4 * PAD, stream.cuda_stream if stream is not None else None)
    assert rc == 0, rc
    if stream is None:
        g.sync()
        host = buf.cpu().numpy()
    else:
        with torch.cuda.stream(stream):
            host = buf.cpu().numpy()
    assert np.all(host[:PAD] == CANARY), "written in front of the table"
    assert np.all(host[PAD + slots:] == CANARY), "written behind the table"
    table = host[PAD:PAD + slots]
    assert not np.any(table == CANARY), ("slots never written", np.flatnonzero(table == CANARY)[:5])
    return table.view(F32).reshape(nsub, qb, n).copy()


def subranges(fir, g, q, start, end, step, stream=None):
    lib = _entries(fir.lib_path())
    qb = len(q)
    return _run(g, q, (end - start) // step, lambda pq, po, st: lib.fir_subrange_distances_dev_(g._h, pq, qb, start, end, step, po, st), stream)


def split(fir, g, q, at, end, stream=None):
    lib = _entries(fir.lib_path())
    qb = len(q)
    return _run(g, q, 2, lambda pq, po, st: lib.fir_split_distances_dev_(g._h, pq, qb, at, end, po, st), stream)


# ---- the oracle's tables ---------------------------------------------------------------------------------------------------------------
_EXP = {}


def exp_row(oracle, key, rows, q, j, lo, hi, metric):
    """oracle.all_distances of query j over [lo, hi) (and its KL bound), computed once per gallery `key`"""
    k = (key, j, lo, hi)
    if k not in _EXP:
        e = oracle.all_distances(rows, q[j], lo, hi, metric)
        _EXP[k] = (e, kl_bound(q[j], rows, lo, hi) if metric == KL else None)
    return _EXP[k]


def check(oracle, key, rows, q, metric, got, ranges, what, qsel=None):
    """got[ci, j, row] against the oracle over ranges[ci], for the queries qsel (indices into q) in the order of the call"""
    qsel = list(range(got.shape[1])) if qsel is None else list(qsel)
    assert got.shape == (len(ranges), len(qsel), rows.shape[0]), (what, got.shape)
    worst = 0.0
    for ci, (lo, hi) in enumerate(ranges):
        for s, j in enumerate(qsel):
            exp, kb = exp_row(oracle, key, rows, q, j, lo, hi, metric)
            nan = np.isnan(exp)
            assert np.array_equal(np.isnan(got[ci, s]), nan), (what, ci, j, "NaN where the oracle has none, or the other way")
            if metric != KL:
                bad = np.flatnonzero((bits(got[ci, s]) != bits(exp)) & ~nan)
                assert bad.size == 0, (what, "sub-range", ci, (lo, hi), "query", j, "rows", bad[:5].tolist(), got[ci, s, bad[:3]], exp[bad[:3]])
            else:
                dev = np.abs(got[ci, s].astype(np.float64) - exp)
                lim = 1e-5 * np.abs(exp) + kb + 1e-12
                bad = np.flatnonzero(~(dev <= lim))
                assert bad.size == 0, (what, "sub-range", ci, (lo, hi), "query", j, "rows", bad[:5].tolist(), got[ci, s, bad[:3]], exp[bad[:3]])
                worst = max(worst, float((dev / lim).max(initial=0.0)))
    return worst


def steps_of(start, end, step):
    return [(lo, lo + step) for lo in range(start, end, step)]


def check_kl_is_range_distances(g, q, got, ranges, what):
    """KL: the sub-range kernel and the store pass of fir_range_distances run the same arithmetic -- equal bits."""
    for ci, (lo, hi) in enumerate(ranges):
        rd = g.range_distances(q, lo, hi)
        bad = np.argwhere(bits(got[ci]) != bits(rd))
        assert bad.size == 0, (what, (lo, hi), "KL bits differ from fir_range_distances at", bad[:5].tolist(), len(bad))


# ---- galleries ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges(metric, n, variant="edges"):
    """d = 100. 997 rows: the edge gallery of test_gpu_scan_forms.py (a copy of query 0 in five tiles, rows 300 / 620 one ulp apart,
    L2: NaN rows and rows beyond 100000; variant "nan row": a NaN value, a denormal and an all-NaN row). Fewer rows: the same plants
    at places that exist. Then, in every size: a gallery row whose features [32, 64) are zero -- a whole sub-range --, a query whose
    features [0, 40) are zero (both zero over [32, 40): the term is skipped), one negative gallery value and one negative query value."""
    d = 100
    if n >= 997:
        gal = edge_gallery(metric, n, d, NQ, variant)
        rows, q = gal.rows.copy(), gal.q.copy()
    else:
        rows = synth.make_gallery(9700 + 10 * n + metric, n, d, metric)
        q, _ = synth.make_queries(9800 + metric, rows, NQ, metric)
        q[0] = rows[n // 2]
        if n > 1:
            rows[n - 1] = rows[0]
            rows[n - 1, 5] = np.nextafter(rows[n - 1, 5], F32(1))
            rows[n - 1, 70] = np.nextafter(rows[n - 1, 70], F32(0))
        if metric == L2 or variant != "edges":
            rows[n // 3, 6] = np.nan
            rows[n // 3, 17] = F32(1e-41)
            if n >= 3:
                rows[2 * n // 3] = np.nan
    rows[n // 4, 32:64] = 0
    q[6, 0:40] = 0
    rows[3 * n // 4, 80] = -np.abs(rows[3 * n // 4, 80]) - F32(1e-3)
    q[7, 3] = -np.abs(q[7, 3]) - F32(1e-3)
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q, ("edges", metric, n, variant)


@functools.lru_cache(maxsize=None)
def plain(metric, n, d, nq=11):
    rows = synth.make_gallery(9900 + metric + d, n, d, metric)
    q, _ = synth.make_queries(9950 + metric + d, rows, nq, metric)
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q, ("plain", metric, n, d, nq)


# ---- a. every row by name ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_every_row_by_name(fir, oracle, metric):
    rows, q, key = edges(metric, 997)
    ranges = steps_of(0, 96, 32)
    worst = 0.0
    with fir.Gallery(rows, None, metric, 0) as g:
        for qb, tile in sorted(TILE_OF.items()) + [(9, 1), (11, 4)]:
            sel = list(range(NQ - qb, NQ)) if qb in (2, 4) else list(range(qb))         # (not always the first queries)
            got = subranges(fir, g, q[sel], 0, 96, 32)
            name = last_kernel(fir, g)
            assert name == sf.k_scan_subranges(tile, metric), (qb, name)
            worst = max(worst, check(oracle, key, rows, q, metric, got, ranges, (name, qb), sel))
            if metric == KL:
                check_kl_is_range_distances(g, q[sel], got, ranges, (name, qb))
            if qb <= 8:
                SEEN.add(name)
    # what the plants are for: the copies of query 0 are at distance 0 in every sub-range, the pair one ulp apart differs in two of the three
    for lo, hi in ranges:
        e0 = exp_row(oracle, key, rows, q, 0, lo, hi, metric)[0]
        assert np.all(e0[[133, 197, 389, 901, 995]] == 0)
    e3 = exp_row(oracle, key, rows, q, 3, 32, 64, metric)[0]
    assert bits(e3[300:301]) == bits(e3[620:621])            # (rows 300 and 620 differ at features 5 and 70 only)
    if metric == L2:
        assert np.isnan(exp_row(oracle, key, rows, q, 1, 0, 32, L2)[0][[450, 451]]).all()
    RAN.add(metric)
    print("sub-range rows of metric %d asserted by name; KL largest |got - oracle| / allowed = %.4f" % (metric, worst))


# ---- b. gallery edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 997))
@pytest.mark.parametrize("metric", METRICS)
def test_gallery_edges(fir, oracle, metric, n):
    """One row, a tile less one, a full tile, a tile and one row, 16 tiles with a part-full last one; 9 queries (8 + 1), three
    sub-ranges and the split form. chi-square / KL once more with the NaN plants (L2 holds them in its only variant)."""
    for variant in ("edges",) if metric == L2 else ("edges", "nan row"):
        rows, q, key = edges(metric, n, variant)
        with fir.Gallery(rows, None, metric, 0) as g:
            got = subranges(fir, g, q[:9], 0, 96, 32)
            assert last_kernel(fir, g) == sf.k_scan_subranges(1, metric)
            check(oracle, key, rows, q, metric, got, steps_of(0, 96, 32), ("edges", n, variant))
            got = split(fir, g, q[:9], 32, 96)
            assert last_kernel(fir, g) == sf.k_scan_subranges(1, metric)
            check(oracle, key, rows, q, metric, got, [(0, 32), (32, 96)], ("edges, split", n, variant))
        if variant == "nan row" and n >= 3:
            e = exp_row(oracle, key, rows, q, 2, 32, 64, metric)[0]
            assert e[960 if n >= 997 else 2 * n // 3] == 0                    # chi-square / KL skip every term of an all-NaN row
        if variant == "edges":
            e = exp_row(oracle, key, rows, q, 0, 0, 32, metric)[0]
            copy = 133 if n >= 997 else n // 2
            assert e[copy] == 0 or (metric == L2 and np.isnan(e[copy]))   # (L2, one row: the copy holds the NaN plant)


# ---- c. feature ranges ---------------------------------------------------------------------------------------------------------------------
ONE_PASS = [(256, 0, 256, 32), (256, 0, 256, 64), (256, 0, 256, 128), (256, 0, 256, 256), (100, 0, 96, 32), (257, 0, 256, 128),
            (300, 4, 260, 64), (300, 32, 288, 128), (1100, 0, 1024, 512)]
PER_RANGE = [(256, 0, 256, 8), (256, 0, 256, 16), (300, 2, 258, 32)]


@pytest.mark.parametrize("d,start,end,step", ONE_PASS + PER_RANGE, ids=lambda v: str(v))
@pytest.mark.parametrize("metric", METRICS)
def test_feature_ranges(fir, oracle, metric, d, start, end, step):
    """200 rows (three tiles and 8 rows), 5 queries (a tile of 8 with three padded). Steps that are multiples of 32 features from a
    start that is a multiple of 4 take one pass -- [4, 260) starts inside a load group of 8 chunks --; any other step or start goes
    range by range and reports no kernel."""
    rows, q, key = plain(metric, 200, d)
    one_pass = (d, start, end, step) in ONE_PASS
    ranges = steps_of(start, end, step)
    with fir.Gallery(rows, None, metric, 0) as g:
        got = subranges(fir, g, q[:5], start, end, step)
        name = last_kernel(fir, g)
        assert name == (sf.k_scan_subranges(8, metric) if one_pass else ""), (name, one_pass)
        check(oracle, key, rows, q, metric, got, ranges, (d, start, end, step))
        if metric == KL and one_pass:
            check_kl_is_range_distances(g, q[:5], got, ranges, (d, start, end, step))


# ---- d. the split form ----------------------------------------------------------------------------------------------------------------------
SPLITS = [(256, 64, 256, True), (256, 32, 256, True), (256, 128, 256, True), (256, 96, 256, True), (256, 224, 256, True), (300, 64, 192, True),
          (256, 48, 256, False), (256, 64, 250, False)]


@pytest.mark.parametrize("d,at,end,one_pass", SPLITS, ids=lambda v: str(v))
@pytest.mark.parametrize("metric", METRICS)
def test_split_form(fir, oracle, metric, d, at, end, one_pass):
    """[0, at) and [at, end): each half is the oracle's distance over its own range -- a mean over that half's own feature count.
    5 queries, then 11 (8 + 3)."""
    rows, q, key = plain(metric, 200, d)
    with fir.Gallery(rows, None, metric, 0) as g:
        for qb, tile in ((5, 8), (11, 4)):
            got = split(fir, g, q[:qb], at, end)
            name = last_kernel(fir, g)
            assert name == (sf.k_scan_subranges(tile, metric) if one_pass else ""), (name, one_pass)
            check(oracle, key, rows, q, metric, got, [(0, at), (at, end)], ("split", d, at, end, qb))


# ---- e. several tiles per wave -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (L2, CHI2))
def test_several_tiles_per_wave(fir, oracle, metric):
    """12 * cus + 5 tiles, the last one holding one row: the pass launches at most three waves per SIMD (12 * cus), so five waves walk
    a second tile. d = 64, two sub-ranges of 32, 3 queries (a tile of 4): every slot."""
    n = 64 * (12 * fir.device_info()["cus"] + 5) - 63
    rows, q, key = plain.__wrapped__(metric, n, 64, 3)          # (not kept: 50 MB)
    with fir.Gallery(rows, None, metric, 0) as g:
        got = subranges(fir, g, q, 0, 64, 32)
        assert last_kernel(fir, g) == sf.k_scan_subranges(4, metric)
        check(oracle, key, rows, q, metric, got, [(0, 32), (32, 64)], ("several tiles per wave", n))
    _EXP.clear()                                         # (the only large expected tables of the module)


# ---- f. state ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_state(fir, oracle, metric):
    """An append across a tile seam (60 -> 70 rows) answers as a fresh handle over the 70 rows; two calls give the same bytes; a call
    on a caller's stream followed by a read on that stream sees the whole table."""
    rows, q, key = plain(metric, 70, 100)
    ranges = steps_of(0, 96, 32)
    with fir.Gallery(rows[:60], None, metric, 0) as g:
        first = subranges(fir, g, q[:5], 0, 96, 32)
        assert first.shape == (3, 5, 60)
        g.append(rows[60:])
        assert g.n == 70
        grown = subranges(fir, g, q[:5], 0, 96, 32)
        grown_split = split(fir, g, q[:5], 32, 96)
    assert np.array_equal(bits(grown[:, :, :60]), bits(first))
    with fir.Gallery(rows, None, metric, 0) as g:
        fresh = subranges(fir, g, q[:5], 0, 96, 32)
        again = subranges(fir, g, q[:5], 0, 96, 32)
        fresh_split = split(fir, g, q[:5], 32, 96)
        st = torch.cuda.Stream()
        streamed = subranges(fir, g, q[:5], 0, 96, 32, stream=st)
        streamed_split = split(fir, g, q[:5], 32, 96, stream=st)
        st.synchronize()
    check(oracle, key, rows, q, metric, fresh, ranges, "fresh handle")
    check(oracle, key, rows, q, metric, fresh_split, [(0, 32), (32, 96)], "fresh handle, split")
    for name, a, b in (("after append", grown, fresh), ("second call", again, fresh), ("caller's stream", streamed, fresh),
                       ("after append, split", grown_split, fresh_split), ("caller's stream, split", streamed_split, fresh_split)):
        assert np.array_equal(bits(a), bits(b)), name


# ---- g. three-way decisions answered by the sub-range kernels ---------------------------------------------------------------------------------
TWD_NQ = (1, 5, 8, 19)
CONV_TH = [(0, 0.21), (0, 0.24), (1, 0.003), (1, 1e-5), (2, 0.7), (2, 0.999)]
PROP_TH = (0.7, 0.95, 0.3, 1.5)
MARGIN = 1e-9          # a thousand times the 1e-12 agreement DESIGN.md states for the device's exp


def staged(g, classifier):
    rep = g.twd_last_dispatch()
    assert (rep["classifier"], rep["planned_fused"], rep["fused_launches"], rep["kernel"]) == (classifier, 0, 0, "") and rep["staged_batches"] >= 1, rep


@functools.lru_cache(maxsize=None)
def twd_case(oracle, metric, n, ncls):
    """19 queries of twd_walk.case whose posterior test (type 0), walked over the ORACLE's tables, stays further than MARGIN from
    every threshold used here: a query that does not is replaced by the next one of the pool."""
    rows, cls, pool = twd_walk.case(71 + metric + n % 89, n, ncls, metric, 24)
    keep = []
    for j in range(len(pool)):
        ok = True
        for reduced in (64, 48):
            d1 = oracle.all_distances(rows, pool[j], 0, reduced, metric)
            d2 = oracle.all_distances(rows, pool[j], reduced, 256, metric)
            for typ, th in CONV_TH:
                if typ == 0:
                    ok = ok and twd_walk.conventional(d1, d2, cls, ncls, 0, th, reduced)[2] > MARGIN
        if ok:
            keep.append(j)
    assert len(keep) >= max(TWD_NQ), keep
    # the last three of the pool sit next to gallery rows: keep them in the batch
    keep = keep[:max(TWD_NQ) - 3] + keep[-3:]
    q = np.ascontiguousarray(pool[keep])
    return rows, cls, q, ("twd", metric, n)


def queries_of(q, nq):
    return q[len(q) - nq:] if nq < 8 else q[:nq]          # (the small batches hold the queries next to a row)


@pytest.mark.parametrize("n,ncls", [(70, 7), (3000, 37)])
@pytest.mark.parametrize("metric", METRICS)
def test_twd_proposed_through_the_subrange_tables(fir, oracle, monkeypatch, metric, n, ncls):
    """KL: every call is staged. L2 / chi-square: staged by FIR_TWD_FUSED=0, one batch size, tables bit-equal, verdicts the oracle's."""
    rows, cls, q, key = twd_case(oracle, metric, n, ncls)
    monkeypatch.setenv("FIR_TWD_FUSED", "1" if metric == KL else "0")
    outcomes = set()
    with fir.Gallery(rows, cls, metric, 0) as g:
        for reduced in (32, 64, 128, 16):
            for nq in TWD_NQ if metric == KL else (19,):
                qq = queries_of(q, nq)
                sel = list(range(len(q) - nq, len(q))) if nq < 8 else list(range(nq))
                sub = subranges(fir, g, qq, 0, 256, reduced)
                assert last_kernel(fir, g) == ("" if reduced == 16 else sf.k_scan_subranges({1: 1, 5: 8, 8: 8, 19: 4}[nq], metric))
                check(oracle, key, rows, q, metric, sub, steps_of(0, 256, reduced), ("proposed", reduced, nq), sel)
                for th in PROP_TH:
                    got = tuple(np.asarray(x).tolist() for x in g.twd_proposed(qq, reduced, th))
                    staged(g, "proposed")
                    walk = [twd_walk.proposed(sub[:, j], cls, th) for j in range(nq)]
                    assert got == ([w[0] for w in walk], [w[1] for w in walk], [w[2] for w in walk]), (reduced, nq, th)
                    if metric != KL:
                        exp = [oracle.twd_proposed(rows, cls, qv, reduced, th, metric) for qv in qq]
                        assert walk == exp, (reduced, nq, th)
                    outcomes |= {(w[1], w[2] == 1, w[2] == 256 // reduced) for w in walk}
    assert {(0, True, False), (1, False, True)} <= outcomes, outcomes          # stopped after one chunk; never


@pytest.mark.parametrize("n,ncls", [(70, 7), (3000, 37)])
@pytest.mark.parametrize("metric", METRICS)
def test_twd_conventional_through_the_split_tables(fir, oracle, monkeypatch, metric, n, ncls):
    rows, cls, q, key = twd_case(oracle, metric, n, ncls)
    monkeypatch.setenv("FIR_TWD_FUSED", "1" if metric == KL else "0")
    outcomes = set()
    with fir.Gallery(rows, cls, metric, 0) as g:
        for reduced in (64, 48):
            for nq in TWD_NQ if metric == KL else (19,):
                qq = queries_of(q, nq)
                sel = list(range(len(q) - nq, len(q))) if nq < 8 else list(range(nq))
                tab = split(fir, g, qq, reduced, 256)
                assert last_kernel(fir, g) == ("" if reduced == 48 else sf.k_scan_subranges({1: 1, 5: 8, 8: 8, 19: 4}[nq], metric))
                check(oracle, key, rows, q, metric, tab, [(0, reduced), (reduced, 256)], ("conventional", reduced, nq), sel)
                for typ, th in CONV_TH:
                    got = tuple(np.asarray(x).tolist() for x in g.twd_conventional(qq, ncls, typ, th, reduced))
                    staged(g, "conventional")
                    walk = [twd_walk.conventional(tab[0, j], tab[1, j], cls, ncls, typ, th, reduced) for j in range(nq)]
                    assert typ != 0 or all(w[2] > MARGIN for w in walk), (reduced, nq, th)
                    assert got == ([w[0] for w in walk], [w[1] for w in walk]), (reduced, nq, typ, th)
                    if typ == 0:
                        for s, j in enumerate(sel):
                            d1 = exp_row(oracle, key, rows, q, j, 0, reduced, metric)[0]
                            d2 = exp_row(oracle, key, rows, q, j, reduced, 256, metric)[0]
                            ow = twd_walk.conventional(d1, d2, cls, ncls, 0, th, reduced)
                            assert ow[2] > MARGIN, (reduced, j, th, ow)
                    if metric != KL:
                        exp = [oracle.twd_conventional(rows, cls, qv, ncls, typ, th, reduced, metric) for qv in qq]
                        assert [w[:2] for w in walk] == exp, (reduced, nq, typ, th)
                    outcomes |= {(typ, w[1]) for w in walk}
    assert outcomes == {(t, u) for t in (0, 1, 2) for u in (0, 1)}, outcomes


def test_every_subrange_row_was_seen():
    """After the module: the names asserted in part a are the twelve k_scan_subranges rows of the table. (Run alone, or with a part of
    test_every_row_by_name deselected, there is nothing to add up.)"""
    if len(RAN) < 3:
        return
    print("sub-range kernel names asserted (%d):" % len(SEEN))
    for name in sorted(SEEN):
        print("  " + name)
    assert SEEN == set(sf.SUBRANGE_ROWS), sorted(SEEN ^ set(sf.SUBRANGE_ROWS))
