"""Every top-1 / top-K / store row of kScanTable (csrc/fir_capi.hip) by name, at the tile, range and tie edges.
tests/scan_forms.py says how a public call reaches each row; here every case is pinned through fir_gallery_set_tuning, run over one
edge gallery and compared with the oracle (recognize_bf, topk, all_distances: the C restatement of the reference -- nothing expected
comes from the library), and the dispatch record must name the row. L2 and chi-square: index and distance bits equal. KL: the bound
of tests/kl_tolerance.py (the one test_gpu_fuzz.py uses), rows equal wherever the oracle's gap exceeds it -- and wherever the only
rows inside it are bitwise copies of each other over the range: copies tie exactly in any arithmetic and order by row.

The edge gallery (edge_gallery, d = 100 unless the row needs long rows; n = 997: 16 tiles, part-full last tile; n = 1061: 17 tiles;
"many": (4 * cus + 1) * 64 + 37 rows from the device's CU count, for the generic one-query rows):
  query 0   an exact copy of row 133 (tile 2, even), which is copied to rows 197 (+64: the same lane's next tile, the R = 2 pair of
            k_scan_l2_lds<2, 4, 3, false, 2>), 389 (+256: the same wave's next tile with 4 waves), 901 (+768: with 12 waves) and n - 2
            (the part-full last tile): the answer is 133 and top-K lists the copies ascending. (Row n - 1 cannot be a copy as well
            as the only answer of query 1; the copy of the last tile sits one row before it.)
  query 1   nearest row n - 1, the last row of the part-full last tile
  query 2   nearest row 0
  query 3   near rows 300 and 620: 620 is 300 with features 5 and 70 moved by one ulp (every range below holds one of them)
  query 4   row 451 with feature 6 replaced -- L2: row 450 is all NaN and row 451 holds one NaN at feature 6, so 451 answers only over
            (64, 100). Chi-square / KL skip a term whose sum is NaN, and a NaN leaves the plain range: their NaN plant goes to the
            "not plain" variant (test_division_twins). An all-NaN row has distance 0 to every query there: it takes every answer
            but query 0's and would hide the other plants, so it has a variant of its own, "nan row" (row 960, behind row 133)
  query 5   (L2) nearest row 210 before rows 200..231 were scaled by 1e7: their distance is >= 100000, they never qualify
fir_gallery_set_tuning counts waves in whole workgroups of 4: WAVES is automatic, one workgroup (a wave strides over every fourth
tile, tiles % waves != 0 at 17 tiles) and three."""
import numpy as np
import pytest
import torch

import scan_forms as sf
import synth
from edge_gallery import NQ, R0, Gal, edge_gallery, mix
from kl_tolerance import bits, kl_bound
from scan_forms import CHI2, KL, L2, STORE, TOP1, TOPK

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32
NOT_FOUND = F32(100000.0)
RANGES = ((0, 0), (3, 61), (5, 7), (0, 96), (0, 44), (64, 100))
WAVES = (0, 4, 12)
NQ_MANY = 6                  # "many": 17 (NQ) one-query passes over 26 MB add nothing to 6; the oracle's KL pass over them costs seconds
K = 8
SEEN, RAN = set(), set()


def many_rows(fir):
    return (4 * fir.device_info()["cus"] + 1) * 64 + 37


def span(rng, d):
    return rng[0], rng[1] or d


def ranges_of(case):
    if case.chunks == sf.WHOLE:
        return [r for r in RANGES if (r[0] | r[1]) % 4 == 0]
    if case.chunks == sf.RAGGED:
        return [r for r in RANGES if (r[0] | r[1]) % 4 != 0]
    return list(RANGES)


# ---- the oracle's values, computed once per (gallery, range) and shared -------------------------------------------------------------
_EXP = {}


def _cached(gal, rng, what, make):
    key = (gal.key, rng, what)
    if key not in _EXP:
        _EXP[key] = make()
    return _EXP[key]


def exp_top1(oracle, gal, rng):
    s, e = span(rng, gal.d)

    def make():
        out = [oracle.recognize_bf(gal.rows, qv, s, e, gal.metric) for qv in gal.q]
        return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], F32)
    return _cached(gal, rng, "top1", make)


def exp_topk(oracle, gal, rng, k):
    s, e = span(rng, gal.d)

    def make():
        out = [oracle.topk(gal.rows, qv, s, e, k, gal.metric) for qv in gal.q]
        return np.stack([o[0] for o in out]).astype(np.int64), np.stack([o[1] for o in out])
    return _cached(gal, rng, ("topk", k), make)


def exp_all(oracle, gal, rng):
    s, e = span(rng, gal.d)
    return _cached(gal, rng, "all", lambda: np.stack([oracle.all_distances(gal.rows, qv, s, e, gal.metric) for qv in gal.q]))


def kl_bound_all(gal, rng):
    s, e = span(rng, gal.d)
    return _cached(gal, rng, "kl bound", lambda: np.stack([kl_bound(qv, gal.rows, s, e) for qv in gal.q]))


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def kl_list(gal, j, rng, ki, kd, gidx, gdist, k, what):
    """KL, query j: the device's k slots against the oracle's k + 5 nearest (ki, kd)."""
    s, e = span(rng, gal.d)
    live = ki >= 0
    kb = np.zeros(len(ki))
    kb[live] = kl_bound(gal.q[j], gal.rows[ki[live]], s, e)
    for i in range(k):
        if ki[i] < 0:
            assert gidx[i] == -1 and gdist[i] == NOT_FOUND, (what, j, i)
            continue
        assert abs(float(gdist[i]) - float(kd[i])) <= 1e-5 * abs(float(kd[i])) + kb[i] + 1e-12, (what, j, i, gdist[i], kd[i])
        rivals = [m for m in range(len(ki)) if m != i and ki[m] >= 0 and not np.array_equal(gal.rows[ki[m], s:e], gal.rows[ki[i], s:e])]
        if all(abs(float(kd[m]) - float(kd[i])) > 2e-5 * abs(float(kd[i])) + 2 * max(kb[i], kb[m]) for m in rivals):
            assert gidx[i] == ki[i], (what, j, i, gidx[i], ki[i])


def check_top1(oracle, gal, rng, got, nq, what, off=0):
    idx, dist = got
    assert idx.shape == dist.shape == (nq,)
    ei, ed = exp_top1(oracle, gal, rng)
    local = np.where(idx >= 0, idx.astype(np.int64) - off, -1)
    if gal.metric != KL:
        assert np.array_equal(local, ei[:nq]), (what, local, ei[:nq])
        assert np.array_equal(bits(dist), bits(ed[:nq])), (what, dist, ed[:nq])
        return
    ki, kd = exp_topk(oracle, gal, rng, 1 + 5)              # (the rivals of recognize_bf's answer, for the gap)
    assert np.array_equal(ki[:, 0], ei) and np.array_equal(bits(kd[:, 0]), bits(ed))
    for j in range(nq):
        kl_list(gal, j, rng, ki[j], kd[j], local[j:j + 1], dist[j:j + 1], 1, what)


def check_topk(oracle, gal, rng, got, nq, k, what, off=0):
    idx, dist = got
    assert idx.shape == dist.shape == (nq, k)
    local = np.where(idx >= 0, idx.astype(np.int64) - off, -1)
    if gal.metric != KL:
        ki, kd = exp_topk(oracle, gal, rng, k)
        assert np.array_equal(local, ki[:nq]), (what, local, ki[:nq])
        assert np.array_equal(bits(dist), bits(kd[:nq])), (what, dist, kd[:nq])
        return
    ki, kd = exp_topk(oracle, gal, rng, k + 5)
    for j in range(nq):
        kl_list(gal, j, rng, ki[j], kd[j], local[j], dist[j], k, what)


def check_store(oracle, gal, rng, got, nq, what):
    assert got.shape == (nq, gal.n)
    exp = exp_all(oracle, gal, rng)[:nq]
    nan = np.isnan(exp)                                  # (L2 rows that hold a NaN; a NaN is a NaN whatever its payload)
    assert np.array_equal(np.isnan(got), nan), what
    if gal.metric != KL:
        assert np.array_equal(bits(got)[~nan], bits(exp)[~nan]), (what, np.argwhere(bits(got) != bits(exp))[:5])
        return
    ok = np.abs(got.astype(np.float64) - exp) <= 1e-5 * np.abs(exp) + kl_bound_all(gal, rng)[:nq] + 1e-12
    assert np.all(ok), (what, np.argwhere(~ok)[:5])


def top1_keys_dev(fir, g, q, rng):
    """fir_search_top1_keys_dev over torch's device memory. The host call of ONE L2 query over a small gallery publishes through a
    launch of its own that leaves the dispatch record alone; this entry point runs the same one-query tile through top1_dev."""
    qt = torch.from_numpy(np.array(q, np.float32)).to(DEV)
    keys = torch.zeros((q.shape[0],), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    g.search_top1_keys_dev(qt.data_ptr(), q.shape[0], keys.data_ptr(), *rng)
    g.sync()
    return fir.keys_unpack(keys.cpu().numpy().view(np.uint64))


def call(fir, g, entry, q, rng, k=K, record=False):
    if entry == TOP1:
        if record and q.shape[0] == 1:
            return top1_keys_dev(fir, g, q, rng)
        return g.search_top1(q, *rng)
    if entry == TOPK:
        return g.search_topk(q, k, *rng)
    return g.range_distances(q, *rng)


def check(oracle, gal, entry, rng, got, nq, what, k=K, off=0):
    if entry == TOP1:
        check_top1(oracle, gal, rng, got, nq, what, off)
    elif entry == TOPK:
        check_topk(oracle, gal, rng, got, nq, k, what, off)
    else:
        check_store(oracle, gal, rng, got, nq, what)


def spoil_record(g, entry, q):
    """A call of another epilogue first, so that the record read next cannot be what an earlier call of this case left."""
    if entry == TOP1:
        g.range_distances(q[:1])
    else:
        g.search_top1(q[:2])


def named_call(fir, g, case, q, rng, k=K):
    """The whole-tile call of a case: its result, after asserting that the dispatch record names the case's kernel."""
    spoil_record(g, case.entry, q)
    got = call(fir, g, case.entry, q[: case.batch], rng, k, record=True)
    ld = g.last_dispatch()
    assert ld["kernel"] == case.name and ld["path"] == "scan", (case, rng, ld)
    assert ld["queries_per_pass"] == case.batch, (case, ld)
    return got, ld


def galleries_of(fir, case, metric):
    if case.size == sf.MANY:
        return [edge_gallery(metric, many_rows(fir), case.d, NQ_MANY)]
    return [edge_gallery(metric, n, case.d) for n in (997, 1061)]


def cases_of(entry, metric):
    return [c for c in sf.CASES if c.entry == entry and c.metric == metric]


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
@pytest.mark.parametrize("entry", (TOP1, TOPK, STORE))
def test_every_case_at_the_edges(fir, oracle, entry, metric):
    for case in cases_of(entry, metric):
        for gal in galleries_of(fir, case, metric):
            nq = gal.q.shape[0]
            with fir.Gallery(gal.rows, None, metric, 0) as g:
                for rng in ranges_of(case):
                    for waves in WAVES:
                        what = (case.name, gal.n, rng, waves)
                        g.set_tuning(case.qpp, waves)
                        # several tiles in one launch plus a remainder
                        check(oracle, gal, entry, rng, call(fir, g, entry, gal.q, rng), nq, what)
                        # exactly one whole tile of the pinned size: the record names the row
                        got, ld = named_call(fir, g, case, gal.q, rng)
                        check(oracle, gal, entry, rng, got, case.batch, what)
                        if waves:
                            assert ld["grid"][0] == waves // 4, (what, ld)
                        SEEN.add(ld["kernel"])
                if metric != L2:
                    assert g.value_range()[0] is True           # the edge gallery is plain: the plain-range twins did these passes
            print("asserted %s: n = %d, d = %d, %d ranges" % (case.name, gal.n, gal.d, len(ranges_of(case))))
    # what the plants are for, whole range: the oracle itself answers 133, n - 1 and 0
    gal = edge_gallery(metric, 997)
    ei, _ = exp_top1(oracle, gal, (0, 0))
    assert ei[0] == R0 and ei[1] == gal.n - 1 and ei[2] == 0, ei[:3]
    ki, _ = exp_topk(oracle, gal, (0, 0), K)
    assert ki[0, :5].tolist() == [R0, R0 + 64, R0 + 256, R0 + 768, gal.n - 2]
    if metric == L2:
        assert not (200 <= ei[5] < 232) and np.all(exp_all(oracle, gal, (0, 0))[:, 200:232] >= NOT_FOUND)
    RAN.add((entry, metric))


@pytest.mark.parametrize("metric", (CHI2, KL))
@pytest.mark.parametrize("entry", (TOP1, TOPK, STORE))
def test_division_twins(fir, oracle, entry, metric):
    """The full-sequence and the plain-range kernel of a chi-square / KL row give the same bits. A negative query value in the tile
    sends the tile through the full sequence (which twin works is decided on the device, per transposed tile): the other queries of
    the tile must return the bytes of the plain run. One-query tiles hold nobody else: top-1 folds its tiles into one launch behind
    one transposition, so a second, poisoned tile rides along; a one-query top-K or store pass has no such company, its full-sequence
    kernel is checked by the second half -- a gallery with a denormal and a NaN is not plain, every pass takes the full sequence,
    and the oracle decides again; once more with an all-NaN row, which chi-square and KL put at distance 0 from everything."""
    ranges = ((0, 0), (3, 61))
    for case in cases_of(entry, metric):
        gal = galleries_of(fir, case, metric)[0]
        poison = -np.abs(gal.q[0])
        with fir.Gallery(gal.rows, None, metric, 0) as g:
            g.set_tuning(case.qpp, 0)
            for rng in ranges:
                plain, _ = named_call(fir, g, case, gal.q, rng)
                assert g.value_range() == (True, True)
                if case.batch == 1 and entry != TOP1:
                    continue
                shared = max(case.batch - 1, 1)
                batch = np.vstack([gal.q[:shared], poison[None, :]])
                spoil_record(g, entry, gal.q)
                mixed = call(fir, g, entry, batch, rng)
                assert g.value_range() == (True, False), (case, rng)
                ld = g.last_dispatch()
                assert ld["kernel"] == case.name and ld["path"] == "scan", (case, ld)
                for a, b in zip(plain if isinstance(plain, tuple) else (plain,), mixed if isinstance(mixed, tuple) else (mixed,)):
                    assert np.array_equal(a[:shared].view(np.uint32), b[:shared].view(np.uint32)), (case, rng)
        for variant in ("not plain", "nan row"):
            odd = edge_gallery(metric, gal.n, gal.d, gal.q.shape[0], variant)
            with fir.Gallery(odd.rows, None, metric, 0) as g:
                g.set_tuning(case.qpp, 0)
                for rng in ranges:
                    check(oracle, odd, entry, rng, call(fir, g, entry, odd.q, rng), odd.q.shape[0], (case.name, variant, rng))
                    got, _ = named_call(fir, g, case, odd.q, rng)
                    check(oracle, odd, entry, rng, got, case.batch, (case.name, variant, rng))
                    assert g.value_range()[0] is False
    ei, ed = exp_top1(oracle, edge_gallery(metric, 997, variant="nan row"), (0, 0))
    # (query 4 is row 451 but for the feature that is NaN there: distance 0 as well, and the lower row)
    assert ei[0] == R0 and ei[4] == 451 and np.all(np.delete(ei, [0, 4]) == 960) and np.all(ed == 0)


@pytest.mark.parametrize("entry", (TOP1, TOPK, STORE))
def test_nothing_qualifies(fir, oracle, entry):
    """130 L2 rows, all at distance >= 100000 from every query: every top-1 and top-K case answers -1 / 100000 in every slot (the
    keys no row ever wrote), the store cases the oracle's values."""
    n = 130
    rows = synth.make_gallery(9301, n, 100, L2) * F32(1.0e7)
    q, _ = synth.make_queries(9302, synth.make_gallery(9301, n, 100, L2), NQ, L2)
    gal = Gal(rows, q, L2, n, 100, "all far")
    with fir.Gallery(rows, None, L2, 0) as g:
        for case in cases_of(entry, L2):
            if case.d != 100:
                continue                                   # (the long rows of the scalar-operand kernel: test_lds_boundaries)
            for rng in [r for r in ranges_of(case) if r != (5, 7)]:
                assert np.all(exp_all(oracle, gal, rng) >= NOT_FOUND)
                for waves in WAVES:
                    g.set_tuning(case.qpp, waves)
                    for batch in (q, q[: case.batch]):
                        got = call(fir, g, entry, batch, rng)
                        check(oracle, gal, entry, rng, got, batch.shape[0], (case.name, rng, waves))
                        if entry != STORE:
                            assert np.all(got[0] == -1) and np.all(got[1] == NOT_FOUND), (case.name, rng, waves)


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_topk_depth(fir, oracle, metric):
    """K = 1, 5, 8 through every top-K row: the whole edge gallery; (L2) a gallery where three rows qualify -- fewer than K in every
    wave and in the merge, the rest of the list is -1 / 100000 --; and a gallery of 3 rows."""
    gals = [edge_gallery(metric, 997)]
    if metric == L2:
        rows = synth.make_gallery(9401, 997, 100, L2)
        q, _ = synth.make_queries(9402, rows, NQ, L2)
        keep = rows[[5, 500, 996]].copy()
        rows = rows * F32(1.0e7)
        rows[[5, 500, 996]] = keep
        gals.append(Gal(rows, q, L2, 997, 100, "three rows qualify"))
    rows = synth.make_gallery(9403, 3, 100, metric)
    gals.append(Gal(rows, synth.make_queries(9404, rows, NQ, metric)[0], metric, 3, 100, ("three rows", metric)))
    for gi, gal in enumerate(gals):
        with fir.Gallery(gal.rows, None, metric, 0) as g:
            for case in cases_of(TOPK, metric):
                for k in (1, 5, 8):
                    for waves in WAVES:
                        g.set_tuning(case.qpp, waves)
                        for rng in ((0, 0), (3, 61)):
                            what = (case.name, gi, k, waves, rng)
                            check_topk(oracle, gal, rng, g.search_topk(gal.q, k, *rng), NQ, k, what)
                            got, _ = named_call(fir, g, case, gal.q, rng, k)
                            check_topk(oracle, gal, rng, got, case.batch, k, what)
        if gal.key == "three rows qualify":
            ki, _ = exp_topk(oracle, gal, (0, 0), 8)
            assert np.all(np.sort(ki[:, :3], axis=1) == np.array([5, 500, 996])) and np.all(ki[:, 3:] == -1)


LDS_FORMS = (
    # d, queries_per_pass = batch, the kernel, its dynamic LDS: (dp4 + 1) * 16 * queries bytes, 0 for the scalar-operand kernel
    (1020, 16, sf.L2_LDS_16, 256 * 16 * 16),          # 65 536: the last d whose 16-query tile fits the default 64 KiB
    (1024, 16, sf.L2_LDS_8, 257 * 16 * 8),            # one chunk more: 16 asked for, 8 per pass
    (2300, 8, sf.L2_LDS_8, 576 * 16 * 8),             # 73 728: above 64 KiB, the launch opts in
    (4604, 8, sf.L2_LDS_8, 1152 * 16 * 8),            # 147 456 = 144 KiB, the largest tile
    (4608, 8, sf.L2_FAST_8, 0),
    (4800, 8, sf.L2_FAST_8, 0),
)


@pytest.mark.parametrize("form", LDS_FORMS, ids=lambda f: "d%d-p%d" % (f[0], f[1]))
def test_lds_boundaries(fir, oracle, form):
    """Which hand-scheduled L2 kernel a whole-chunk top-1 call takes is LDS arithmetic on the row length. 237 rows (4 tiles, the last
    part full), rows 5 and 69 equal (one lane, consecutive tiles) with query 0 their copy, query 1 nearest to the last row; the whole
    row, a prefix that ends inside it and a range that starts inside it (the LDS reads run one unit ahead of the features)."""
    d, qpp, name, lds = form
    n = 237
    rows = synth.make_gallery(9500 + d, n, d, L2)
    q, _ = synth.make_queries(9600 + d, rows, qpp + 1, L2)
    rows[69] = rows[5]
    q[0] = rows[5]
    q[1] = mix(rows[n - 1], rows[7], L2)
    gal = Gal(rows, q, L2, n, d, ("lds", d))
    with fir.Gallery(rows, None, L2, 0) as g:
        for rng in ((0, 0), (0, 96), (64, 0), (d - 40, d - 4)):
            for waves in (0, 4):
                g.set_tuning(qpp, waves)
                check_top1(oracle, gal, rng, g.search_top1(q, *rng), qpp + 1, (name, rng, waves))
                spoil_record(g, TOP1, q)
                got = g.search_top1(q[:qpp], *rng)
                ld = g.last_dispatch()
                assert ld["kernel"] == name and ld["path"] == "scan" and lds <= ld["lds_bytes"] < lds + 64, (form, rng, ld)    # (+ static LDS: none today)
                check_top1(oracle, gal, rng, got, qpp, (name, rng, waves))
    ei, _ = exp_top1(oracle, gal, (0, 0))
    assert ei[0] == 5 and ei[1] == n - 1
    print("asserted %s at d = %d (%d bytes of dynamic LDS)" % (name, d, lds))


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_row_offset(fir, oracle, metric):
    """fir_gallery_set_row_offset(1 << 20): every top-1 and top-K row adds it to the rows it reports and changes nothing else."""
    off = 1 << 20
    for case in cases_of(TOP1, metric) + cases_of(TOPK, metric):
        gal = galleries_of(fir, case, metric)[0]
        rng = ranges_of(case)[1] if case.chunks == sf.ANY else ranges_of(case)[0]
        with fir.Gallery(gal.rows, None, metric, 0) as g:
            g.set_tuning(case.qpp, 0)
            g.set_row_offset(off)
            check(oracle, gal, case.entry, rng, call(fir, g, case.entry, gal.q, rng), gal.q.shape[0], (case.name, "offset"), off=off)
            got, _ = named_call(fir, g, case, gal.q, rng)
            check(oracle, gal, case.entry, rng, got, case.batch, (case.name, "offset"), off=off)
            assert np.ravel(got[0])[0] == R0 + off


def test_every_table_name_was_seen():
    """After the module: the dispatch records asserted above are the table's rows, all of them. (Run alone, or with a part of
    test_every_case_at_the_edges deselected, there is nothing to add up.)"""
    if len(RAN) < 9:
        return
    print("kernel names asserted (%d):" % len(SEEN))
    for name in sorted(SEEN):
        print("  " + name)
    assert SEEN == {c.name for c in sf.CASES}, sorted(SEEN ^ {c.name for c in sf.CASES})
