"""Every instantiation of the one-launch three-way-decision kernels (csrc/fir_twd.hip, kFusedTable: L2 / chi-square x 1, 2, 4,
8, 16 tiles per wave, k_twd_conv_fused and k_twd_prop_fused of each) against the oracle, with the form that answered read from
fir_twd_last_dispatch after every call.

The natural dispatch gives a wave more than one tile only for galleries of hundreds of thousands of rows. FIR_TWD_GROUPS=N caps
the workgroups per query of a one-launch call, so a gallery of a few thousand rows takes the tiles-per-wave form a gallery of a
million rows gets; it changes no answer. With N = 3 a call gets T tiles per wave for 512 (T / 2) 3 < n <= 512 T 3 rows.

Every comparison is of integers (class, unreliable flag, chunks used): there are no tolerances. A test asserts the kernel,
the tiles per wave and the workgroups per query it is meant to reach, so a plan that lands elsewhere fails the test instead of
passing on another kernel. A one-launch call whose workgroups do not meet in time is re-answered by the staged kernels (the
answers are the same); the tests count those launches and require that each kernel they aim at answered at least once per case
and that fewer than one launch in twenty of the module gave up. Nothing here tries to cause one."""
import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

TILES = (1, 2, 4, 8, 16)
CONV_THRESHOLDS = gc.TWD_CONVENTIONAL + [(1, 0.0), (2, 0.5), (0, 0.9)]
# stops after one chunk, after a few, never (0.3), everything pruned (1.5)
PROP_THRESHOLDS = [(32, 0.7), (64, 0.95), (16, 0.3), (128, 0.7), (32, 1.5), (8, 0.9)]
ALL_KERNELS = {f"fir::k_twd_{which}_fused<{m}, {t}>" for which in ("conv", "prop") for m in (gc.L2, gc.CHI2) for t in TILES}

# kernel name -> {"launches", "gave_up", "n": gallery sizes that reached it}: one-launch calls of the whole module whose verdicts
# equalled the oracle's
LEDGER = {}


class Case:
    """The one-launch calls of one test case: which kernels they reached and how many of their launches gave up."""

    def __init__(self, fir, oracle, monkeypatch, groups=3):
        self.fir, self.oracle, self.mp = fir, oracle, monkeypatch
        self.seen = {}
        monkeypatch.setenv("FIR_TWD_GROUPS", str(groups))

    def _fused(self, g, n, call, classifier, kernel, T, G, nq):
        """`call` under the automatic dispatch: the report must name the row aimed at. Returns the verdicts as lists."""
        self.mp.setenv("FIR_TWD_FUSED", "1")
        got = tuple(np.asarray(x).tolist() for x in call())
        rep = g.twd_last_dispatch()
        assert (rep["classifier"], rep["planned_fused"], rep["kernel"], rep["tiles_per_wave"], rep["workgroups_per_query"], rep["queries_per_launch"]) == \
            (classifier, 1, kernel, T, G, nq), (n, rep)
        assert rep["fused_launches"] == 1 and rep["staged_batches"] == rep["fused_gave_up"] <= 1, (n, rep)
        e = self.seen.setdefault(kernel, {"launches": 0, "gave_up": 0, "n": set()})
        e["launches"] += rep["fused_launches"]
        e["gave_up"] += rep["fused_gave_up"]
        e["n"].add(n)
        return got

    def _staged(self, g, call, classifier, batches=1):
        self.mp.setenv("FIR_TWD_FUSED", "0")
        got = tuple(np.asarray(x).tolist() for x in call())
        rep = g.twd_last_dispatch()
        assert (rep["classifier"], rep["planned_fused"], rep["fused_launches"], rep["fused_gave_up"], rep["tiles_per_wave"], rep["kernel"]) == \
            (classifier, 0, 0, 0, 0, "") and rep["staged_batches"] == batches, rep
        return got

    def conventional(self, g, rows, cls, q1, ncls, typ, th, fc, metric, T, G, staged_too=True):
        """One query through k_twd_conv_fused<metric, T> (and the launch-per-stage form) against the oracle."""
        n = len(rows)
        exp = self.oracle.twd_conventional(rows, cls, q1, ncls, typ, th, fc, metric)
        exp = ([exp[0]], [exp[1]])
        got = self._fused(g, n, lambda: g.twd_conventional(q1, ncls, typ, th, fc), "conventional", f"fir::k_twd_conv_fused<{metric}, {T}>", T, G, 1)
        assert got == exp, ("fused", n, typ, th, fc)
        if staged_too:
            assert self._staged(g, lambda: g.twd_conventional(q1, ncls, typ, th, fc), "conventional") == exp, ("per-stage", n, typ, th, fc)

    def proposed(self, g, rows, cls, q, fc, th, metric, T, G, exp=None, staged_too=True):
        """len(q) <= 8 queries in one launch of k_twd_prop_fused<metric, T> (and the launch-per-chunk form) against the oracle."""
        n = len(rows)
        if exp is None:
            exp = [self.oracle.twd_proposed(rows, cls, qi, fc, th, metric) for qi in q]
        exp = ([e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp])
        got = self._fused(g, n, lambda: g.twd_proposed(q, fc, th), "proposed", f"fir::k_twd_prop_fused<{metric}, {T}>", T, G, len(q))
        assert got == exp, ("fused", n, len(q), fc, th)
        if staged_too:
            assert self._staged(g, lambda: g.twd_proposed(q, fc, th), "proposed") == exp, ("per-chunk", n, len(q), fc, th)

    def close(self, *kernels):
        """Each kernel the case aimed at answered at least one launch to the end; its counts join the module's."""
        assert set(kernels) <= set(self.seen), (kernels, sorted(self.seen))
        for k, e in self.seen.items():
            assert e["launches"] > e["gave_up"], f"{k}: {e['launches']} launches, all {e['gave_up']} gave up (n = {sorted(e['n'])})"
            t = LEDGER.setdefault(k, {"launches": 0, "gave_up": 0, "n": set()})
            t["launches"] += e["launches"]
            t["gave_up"] += e["gave_up"]
            t["n"] |= e["n"]


def conv_groups(n, T):
    return (-(-n // 64) + 8 * T - 1) // (8 * T)


def metric_case(seed, n, ncls, metric):
    rows, cls, q, _ = gc.twd_case(seed=seed, n=n, d=256, n_classes=ncls)
    if metric == gc.CHI2:
        rows = np.abs(rows) + np.float32(1e-3)
        q = np.abs(q) + np.float32(1e-3)
    # 8 queries, three of them next to a row
    q = np.concatenate([q[:5], q[5:8] * np.float32(0.05) + rows[[1, n // 2, n - 1]] * np.float32(0.95)])
    return rows, cls, q


# ---- a. every table row, both kernels ------------------------------------------------------------------------------------------
# (every slot of every wave full; the last tile holds one row; the last workgroup holds one row in one tile and its other waves
# and slots lie past the last tile)
SIZES = {"full": lambda T: 512 * T * 3, "one-row-tile": lambda T: 512 * T * 3 - 63, "one-row-workgroup": lambda T: 512 * T * 2 + 1}


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("metric", [gc.L2, gc.CHI2])
def test_every_fused_kernel_of_the_table_matches_the_oracle(fir, oracle, monkeypatch, metric, T, size):
    n = SIZES[size](T)
    ncls = 37 if metric == gc.L2 else 23
    rows, cls, q = metric_case(61 + T + 7 * metric, n, ncls, metric)
    case = Case(fir, oracle, monkeypatch)
    G = conv_groups(n, T)
    assert G == 3
    for labels in (np.sort(cls), cls):                                  # class-major (the reference's order) and interleaved
        with fir.Gallery(rows, labels, metric, 0) as g:
            for (typ, th) in CONV_THRESHOLDS:
                for qi in (0, 3, 5, 6, 7):                              # one query per call: several are fused only at T = 1
                    case.conventional(g, rows, labels, q[qi:qi + 1], ncls, typ, th, 64, metric, T, G)
    with fir.Gallery(rows, cls, metric, 0) as g:
        for (fc, th) in PROP_THRESHOLDS + ([(4, 0.9)] if n < 7000 else []):
            exp = [oracle.twd_proposed(rows, cls, qi, fc, th, metric) for qi in q]
            case.proposed(g, rows, cls, q, fc, th, metric, T, 3, exp)
            case.proposed(g, rows, cls, q[[0, 5, 7]], fc, th, metric, T, 3, [exp[0], exp[5], exp[7]])
            case.proposed(g, rows, cls, q[6:7], fc, th, metric, T, 3, exp[6:7])
        knobs = g.last_dispatch()["knobs"]
        assert "FIR_TWD_GROUPS" in knobs or knobs.endswith("..."), knobs      # whatever is honoured is reported
    case.close(f"fir::k_twd_conv_fused<{metric}, {T}>", f"fir::k_twd_prop_fused<{metric}, {T}>")


# ---- b. order and ties with several tiles per wave -------------------------------------------------------------------------------
def sharp_thresholds(d, k, best):
    """Thresholds of types 1 and 2 that tell secondBestDist = d[k - 1] from its neighbours in the walk, d[k - 2] and d[k] (all
    distinct, descending): from the oracle's distances, in double like the reliability test."""
    d = d.astype(np.float64)
    assert d[k - 2] > d[k - 1] > d[k] >= best > 0
    lo, hi = (d[k - 1] + d[k]) / 2, (d[k - 2] + d[k - 1]) / 2
    return [(1, lo - best), (1, hi - best), (2, best / lo), (2, best / hi)]


@pytest.mark.parametrize("T,n", [(4, 6000), (16, 24000)])
def test_conventional_fused_record_walk_across_slots_waves_and_workgroups(fir, oracle, monkeypatch, T, n):
    """secondBestDist is bestDist at the last class change of the record walk (ImageTesting.cpp:123-125). Rows in descending
    first-stage distance to a query: every row is a record. The last record of another class than the best row's is put in
    turn into another slot, wave and workgroup (workgroup b, wave w, slot i own tile (8 b + w) T + i), and the thresholds sit
    between the distances of that record and its two neighbours. Then: copies of a late row further up -- same lane in
    another slot, another wave, another workgroup -- which tie with a record and are none; NaN rows; nothing below 100000."""
    ncls = 9
    rows, cls, q, _ = gc.twd_case(seed=17 + T, n=n, d=256, n_classes=ncls)
    order = np.argsort(oracle.all_distances(rows, q[0], 0, 64, 0), kind="stable")[::-1].copy()
    rows, cls = rows[order], cls[order]
    q = q[:3].copy()
    d = oracle.all_distances(rows, q[0], 0, 64, 0)
    best, cstar = float(d[n - 1]), int(cls[n - 1])
    case = Case(fir, oracle, monkeypatch)
    G = conv_groups(n, T)
    assert G == 3

    def pos(b, w, i, lane):
        return ((b * 8 + w) * T + i) * 64 + lane

    usual = [(1, 1e-4), (1, 1e-6), (2, 0.9), (2, 0.9999), (0, 0.24)]
    for k in (pos(0, 0, 1, 0), pos(0, 3, T - 1, 63), pos(0, 7, T // 2, 31), pos(1, 0, 0, 0), pos(1, 4, 1, 5), pos(2, 2, T - 1, 17), n - 1):
        assert 2 <= k < n
        c2 = cls.copy()
        c2[k:] = cstar                                                    # the last class change of the walk is at row k ...
        c2[k - 1] = (cstar + 1) % ncls                                    # ... from this row's class: secondBestDist = d[k - 1]
        with fir.Gallery(rows, c2, gc.L2, 0) as g:
            for (typ, th) in sharp_thresholds(d, k, best):
                case.conventional(g, rows, c2, q[0:1], ncls, typ, th, 64, gc.L2, T, G, staged_too=False)
            for (typ, th) in usual:
                case.conventional(g, rows, c2, q[1:2], ncls, typ, th, 64, gc.L2, T, G, staged_too=False)
    # ties: the row at `src` (smaller than everything in front of it) copied to p[0] < p[1] < p[2] < p[3] < src. p[0] is a record,
    # the later copies and `src` tie with it and are none, whatever their classes; every other row from p[0] on has the class of
    # p[0], so secondBestDist stays d[p[0] - 1]
    p = [pos(0, 1, 0, 17), pos(0, 1, 2, 17), pos(0, 5, 1, 17), pos(1, 2, 1, 17)]
    src = pos(2, 3, 1, 17)
    assert p == sorted(p) and p[3] < src < n - 1
    r2, c2 = rows.copy(), cls.copy()
    c2[p[0]:] = cstar
    c2[p[0] - 1] = (cstar + 1) % ncls
    for i, r in enumerate(p):
        r2[r] = rows[src]
    c2[p[1]], c2[p[2]], c2[p[3]], c2[src] = (cstar + 2) % ncls, (cstar + 3) % ncls, (cstar + 1) % ncls, (cstar + 4) % ncls
    d2 = oracle.all_distances(r2, q[0], 0, 64, 0)
    q2 = np.stack([q[0], rows[src] * np.float32(0.999), q[2]])            # the second one: the copies are the best rows, the FIRST one's class decides
    nan = r2.copy()
    nan[7] = np.nan
    nan[pos(1, 6, T - 1, 40), 3] = np.nan
    nan[pos(0, 2, 1, 9), 200] = np.nan
    # the all-NaN row has the best row's class: its posterior exp(-100 NaN) must not replace that class's maximum (ImageTesting.cpp:120:
    # `probab > probabs[c]` is false). Type 0 thresholds on both sides of the oracle's ratio best / (sum of the 5 largest)
    c3 = c2.copy()
    c3[7] = cstar
    ok = ~np.isnan(oracle.all_distances(nan, q[0], 0, 64, 0))
    post = np.zeros(ncls)
    np.maximum.at(post, c3[ok], np.exp(-100.0 * oracle.all_distances(nan, q[0], 0, 64, 0)[ok].astype(np.float64)))
    ratio = np.exp(-100.0 * best) / np.sort(post)[::-1][:5].sum()
    for rr, cc, extra in ((r2, c2, []), (nan, c3, [(0, ratio * 0.998), (0, ratio * 1.002)])):
        with fir.Gallery(rr, cc, gc.L2, 0) as g:
            for (typ, th) in sharp_thresholds(d2, p[0], best) + [(1, 1e-3), (2, 0.99)] + usual + extra:
                for qi in range(3):
                    case.conventional(g, rr, cc, q2[qi:qi + 1], ncls, typ, th, 64, gc.L2, T, G)
    far = np.full((n, 256), 3.0e4, np.float32)
    fcls = (np.arange(n, dtype=np.int32) % 7).astype(np.int32)
    with fir.Gallery(far, fcls, gc.L2, 0) as g:
        for typ, th in ((0, 0.24), (1, 0.003), (2, 0.7)):
            case.conventional(g, far, fcls, np.zeros((1, 256), np.float32), 7, typ, th, 64, gc.L2, T, G)
    case.close(f"fir::k_twd_conv_fused<0, {T}>")


@pytest.mark.parametrize("T,n", [(4, 6000), (16, 24000)])
def test_proposed_fused_ties_and_nan_rows_with_several_tiles_per_wave(fir, oracle, monkeypatch, T, n):
    """Equal sums at rows of the same lane in different slots (rows r and r + 64 * 8 * G * i: a query's tiles are dealt round to
    its G * 8 waves), in another wave and in another workgroup: the FIRST row is the best one and its class decides. NaN rows are
    never the best and never pruned; a gallery in which nothing is below 100000 answers -1 after one chunk."""
    ncls = 50
    rows, cls, q, _ = gc.twd_case(seed=44 + T, n=n, d=256, n_classes=ncls)
    q = q[:4].copy()
    case = Case(fir, oracle, monkeypatch)
    G = 3
    r = 2 * 64 + 17                                                     # wave 2 of workgroup 0, slot 0
    copies = [r, r + 64 * 8 * G * 1, r + 64 * 8 * G * (T - 1), r + 64 * 3, r + 64 * 8 * 2 + 64 * 8 * G * 2]
    assert max(copies) < n
    dup = rows[r].copy()
    for i, c in enumerate(copies):
        rows[c] = dup
        cls[c] = (3, 4, 3, 5, 6)[i]
    q[0] = dup
    q[1] = dup * np.float32(1.001)
    nan = rows.copy()
    nan[5] = np.nan
    nan[r + 64 * 8 * G * 2 + 64, 40] = np.nan
    for rr in (rows, nan):
        with fir.Gallery(rr, cls, gc.L2, 0) as g:
            for (fc, th) in [(32, 0.7), (64, 0.999), (32, 1.0), (8, 0.95)]:
                case.proposed(g, rr, cls, q, fc, th, gc.L2, T, G)
                case.proposed(g, rr, cls, q[0:1], fc, th, gc.L2, T, G)
    far = np.full((n, 256), 3.0e4, np.float32)                           # every chunk distance is 9e8 > 100000
    fcls = (np.arange(n, dtype=np.int32) % 7).astype(np.int32)
    with fir.Gallery(far, fcls, gc.L2, 0) as g:
        case.proposed(g, far, fcls, np.zeros((2, 256), np.float32), 32, 0.7, gc.L2, T, G, exp=[(-1, 0, 1), (-1, 0, 1)])
    case.close(f"fir::k_twd_prop_fused<0, {T}>")


# ---- c. meetings released through the flag words (more than 16 workgroups per query) with two tiles per wave ---------------------
def test_flag_released_meetings_with_two_tiles_per_wave(fir, oracle, monkeypatch):
    n, ncls = 20417, 40
    rows, cls, q = metric_case(77, n, ncls, gc.L2)
    case = Case(fir, oracle, monkeypatch, groups=20)
    assert conv_groups(n, 2) == 20 and conv_groups(n, 1) > 20
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        for (typ, th) in CONV_THRESHOLDS:
            for qi in (0, 5, 6, 7):
                case.conventional(g, rows, cls, q[qi:qi + 1], ncls, typ, th, 64, gc.L2, 2, 20)
        for (fc, th) in PROP_THRESHOLDS:
            exp = [oracle.twd_proposed(rows, cls, qi, fc, th) for qi in q]
            case.proposed(g, rows, cls, q, fc, th, gc.L2, 2, 20, exp)
            case.proposed(g, rows, cls, q[[0, 5, 7]], fc, th, gc.L2, 2, 20, [exp[0], exp[5], exp[7]])
            case.proposed(g, rows, cls, q[6:7], fc, th, gc.L2, 2, 20, exp[6:7])
    case.close("fir::k_twd_conv_fused<0, 2>", "fir::k_twd_prop_fused<0, 2>")


# ---- d. reduced_features_count -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(3000, 2), (8193, 8)])
def test_reduced_features_counts_fused_and_staged(fir, oracle, monkeypatch, n, T):
    """Conventional: multiples of 4 take the generic eight-piece load groups of the one-launch kernel (ragged for 4, 100, 252), the
    others the launch-per-stage form with masked range edges. Proposed: 8 features per chunk is the smallest fused step (32 chunks);
    1 and 2 give 256 and 128 chunks, more than the one-launch kernel's 64, and are staged only."""
    ncls = 37
    rows, cls, q = metric_case(91 + T, n, ncls, gc.L2)
    case = Case(fir, oracle, monkeypatch)
    G = conv_groups(n, T)
    assert G == 3
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        for fc in (4, 16, 100, 128, 252):
            for (typ, th) in gc.TWD_CONVENTIONAL:
                for qi in (0, 6, 7):
                    case.conventional(g, rows, cls, q[qi:qi + 1], ncls, typ, th, fc, gc.L2, T, G)
        monkeypatch.setenv("FIR_TWD_FUSED", "1")
        for fc in (1, 50, 255):
            for (typ, th) in gc.TWD_CONVENTIONAL:
                for qi in (0, 6, 7):
                    c, u = g.twd_conventional(q[qi:qi + 1], ncls, typ, th, fc)
                    rep = g.twd_last_dispatch()
                    assert (rep["planned_fused"], rep["fused_launches"], rep["staged_batches"], rep["kernel"]) == (0, 0, 1, ""), (fc, rep)
                    assert (int(c[0]), int(u[0])) == oracle.twd_conventional(rows, cls, q[qi], ncls, typ, th, fc), (fc, typ, th, qi)
        for th in (0.7, 0.95, 0.3):
            case.proposed(g, rows, cls, q, 8, th, gc.L2, T, 3)
            case.proposed(g, rows, cls, q[6:7], 8, th, gc.L2, T, 3)
        if n == 3000:
            monkeypatch.setenv("FIR_TWD_FUSED", "1")
            for fc in (1, 2):
                for th in (0.7, 0.95, 0.3):
                    got = tuple(np.asarray(x).tolist() for x in g.twd_proposed(q[5:8], fc, th))
                    rep = g.twd_last_dispatch()
                    assert (rep["planned_fused"], rep["fused_launches"], rep["staged_batches"], rep["kernel"]) == (0, 0, 1, ""), (fc, rep)
                    exp = [oracle.twd_proposed(rows, cls, qi, fc, th) for qi in q[5:8]]
                    assert got == ([e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp]), (fc, th)
    case.close(f"fir::k_twd_conv_fused<0, {T}>", f"fir::k_twd_prop_fused<0, {T}>")


# ---- e. many calls in a row ------------------------------------------------------------------------------------------------------------
def test_many_alternating_calls_on_one_handle_with_eight_tiles_per_wave(fir, oracle, monkeypatch):
    """The two parity blocks of the proposed kernel's state alternate from call to call and each call clears the other one; the
    conventional kernel's deciding workgroup leaves its state words zero. 60 calls, conventional and proposed in turn, of 1 to 5
    queries (a conventional call of several queries is answered by the launch-per-stage form in between: the report says so)."""
    n, ncls, T = 12288, 30, 8
    rows, cls, q, _ = gc.twd_case(seed=52, n=n, d=256, n_classes=ncls)
    rng = np.random.default_rng(5)
    case = Case(fir, oracle, monkeypatch)
    with fir.Gallery(rows, cls, gc.L2, 0) as g:
        for it in range(60):
            k = it // 2
            nq = (1, 1, 3, 1, 2, 1, 5, 1, 4, 1)[k % 10] if it % 2 == 0 else 1 + k % 5
            qq = q[rng.integers(0, len(q), nq)] * np.float32(0.5) + rows[rng.integers(0, n, nq)] * np.float32(0.5)
            if it % 2 == 0:
                typ, th = gc.TWD_CONVENTIONAL[k % len(gc.TWD_CONVENTIONAL)]
                if nq == 1:
                    case.conventional(g, rows, cls, qq, ncls, typ, th, 64, gc.L2, T, 3, staged_too=False)
                else:
                    monkeypatch.setenv("FIR_TWD_FUSED", "1")
                    c, u = g.twd_conventional(qq, ncls, typ, th, 64)
                    rep = g.twd_last_dispatch()
                    assert (rep["classifier"], rep["planned_fused"], rep["fused_launches"], rep["staged_batches"]) == ("conventional", 0, 0, 1), (it, rep)
                    exp = [oracle.twd_conventional(rows, cls, qi, ncls, typ, th, 64) for qi in qq]
                    assert (list(c), list(u)) == ([e[0] for e in exp], [e[1] for e in exp]), (it, typ, th)
            else:
                fc = (8, 32, 64, 128)[k % 4]
                th = (0.7, 0.95, 0.4)[k % 3]
                case.proposed(g, rows, cls, qq, fc, th, gc.L2, T, 3, staged_too=False)
    case.close("fir::k_twd_conv_fused<0, 8>", "fir::k_twd_prop_fused<0, 8>")


# ---- every row answered; few launches gave up ---------------------------------------------------------------------------------------
def test_every_instantiation_answered_and_few_launches_gave_up(fir, oracle, monkeypatch):
    """One call per row of kFusedTable and kernel (on its own this test reaches all twenty), then over everything this module
    launched: the kernels that answered with the oracle's verdicts are the table's, and fewer than 1 launch in 20 gave up."""
    case = Case(fir, oracle, monkeypatch)
    for metric in (gc.L2, gc.CHI2):
        for T in TILES:
            n = 512 * T * 2 + 1
            rows, cls, q = metric_case(23 + T, n, 11, metric)
            with fir.Gallery(rows, cls, metric, 0) as g:
                case.conventional(g, rows, cls, q[6:7], 11, 1, 0.003, 64, metric, T, 3, staged_too=False)
                case.proposed(g, rows, cls, q[4:7], 32, 0.7, metric, T, 3, staged_too=False)
    case.close(*sorted(ALL_KERNELS))
    answered = {k for k, e in LEDGER.items() if e["launches"] > e["gave_up"]}
    table = "\n".join(f"{k}: n = {sorted(e['n'])}, {e['launches'] - e['gave_up']} launches answered, {e['gave_up']} gave up" for k, e in sorted(LEDGER.items()))
    print(table)
    assert answered == ALL_KERNELS, table
    launches, gave_up = sum(e["launches"] for e in LEDGER.values()), sum(e["gave_up"] for e in LEDGER.values())
    assert gave_up * 20 < launches, f"{gave_up} of {launches} one-launch calls gave up\n{table}"
