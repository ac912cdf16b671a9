"""The chi-square / KL nomination scans of the candidate-list path themselves -- k_nominate<6 | 7>, k_scan<8, 5 | 6 | 7, ...>, the
thresholds (k_topk_tau, k_query_sums_widen, k_query_entropy_widen) and the lists -- against float64 (nomination_scan_ref.py), not
just the final keys: the re-rank is sound against rounding, not against a nomination value further from the reference than the
bound the threshold was widened by, and the final keys cannot tell unless the winner sits within a few ulp of the threshold.

Everything is read through the library's internal fir_gallery_list_nominations_: the steps topk_lists_dev runs, stopped before the
re-rank rewrites the nomination values, without the dispatch gates, so a 4000-row gallery (62 tiles and one of 32 rows) goes
through the kernels of the 65 536-row path; all_rows = 1 puts the thresholds at +inf, and the lists then hold every row's value.

  A  values      |nomination value - float64 reference| <= B for every (query, row), input kind, feature range and batch size
  B  thresholds  sample keys, widened thresholds and lists of the normal mode, K = 1 and 5
  C  L2          the same read-out with the exact metric: listed values are range_distances' bits
  D  public      the smallest shape the dispatch gates admit (65 600 x 32, 16 queries): the exact scan's keys, k_nominate named

Largest |value - reference| / B measured on an MI355X: profiles/nomination_scan_bounds.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

import nomination_scan_ref as ref

pytestmark = pytest.mark.gpu

N, QB = 4000, 40
U24 = ref.U24
FORMS = {"chi2_harm": (ref.CHI2, ref.FORM_HARM, "2"), "chi2_approx": (ref.CHI2, ref.FORM_APPROX, "1"), "kl_ent": (ref.KL, ref.FORM_ENT, None)}
# (form, samples): kChi2Approx always takes the exact metric's samples
FORM_SAMPLES = [("chi2_harm", "nomination"), ("chi2_harm", "exact"), ("chi2_approx", "exact"), ("kl_ent", "nomination"), ("kl_ent", "exact")]


@functools.lru_cache(maxsize=2)
def _case(kind, d):
    rows, q = ref.make_case(kind, N, d, QB)
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q


@functools.lru_cache(maxsize=1)
def _terms(metric, kind, d):
    """every feature's float64 term of one dataset: shared by the forms, sample modes and ranges of tests A and B"""
    rows, q = _case(kind, d)
    t = ref.feature_terms(metric, q, rows, 0, d)
    t.setflags(write=False)
    return t


def _reference(metric, kind, d, a, b):
    return ref.distances(metric, None, None, a, b, terms=_terms(metric, kind, d))


def _knobs(monkeypatch, form, samples):
    for name in ("FIR_CHI2_NOMINATION", "FIR_EXACT_SAMPLES", "FIR_NO_CHI2_NOMINATION"):
        monkeypatch.delenv(name, raising=False)
    if FORMS[form][2]:
        monkeypatch.setenv("FIR_CHI2_NOMINATION", FORMS[form][2])
    if samples == "exact":
        monkeypatch.setenv("FIR_EXACT_SAMPLES", "1")


def read_out(fir, g, q, a, b, k, all_rows):
    """fir_gallery_list_nominations_: dict of metric, qpad, stride, group_tiles, counts, tau, sq [qpad], rowsum [n + 1],
    skeys [k, stride], lists [qpad, 4096], flag"""
    fn = C.CDLL(fir.lib_path()).fir_gallery_list_nominations_
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] * 8
    q = np.ascontiguousarray(q, np.float32)
    qb, qmax = q.shape[0], (q.shape[0] + 15) // 16 * 16
    info, flag = np.zeros(4, np.int32), np.full(1, -1, np.int32)
    counts, tau, sq = np.full(qmax, -1, np.int32), np.full(qmax, np.nan, np.float32), np.full(qmax, np.nan, np.float32)
    rowsum, skeys, lists = np.full(g.n + 1, np.nan, np.float32), np.zeros(k * qmax, np.uint64), np.zeros((qmax, ref.LIST_CAP), np.uint64)
    rc = fn(g._h, q.ctypes.data, qb, a, b, k, all_rows, info.ctypes.data, counts.ctypes.data, tau.ctypes.data, sq.ctypes.data, rowsum.ctypes.data,
            skeys.ctypes.data, lists.ctypes.data, flag.ctypes.data)
    assert rc == 0, rc
    qpad, stride = int(info[1]), int(info[2])
    assert qb <= qpad <= qmax and qb <= stride <= qpad
    return dict(metric=int(info[0]), qpad=qpad, stride=stride, group_tiles=int(info[3]), counts=counts[:qpad], tau=tau[:qpad], sq=sq[:qpad], rowsum=rowsum,
                skeys=skeys[:k * stride].reshape(k, stride), lists=lists[:qpad], flag=int(flag[0]))


def values_of_all_rows(ex, qb, n):
    """[qb, n] float32 from an all_rows read-out: every live query lists every row once, the padding lists nothing"""
    assert ex["flag"] == 0
    assert np.array_equal(ex["counts"][:qb], np.full(qb, n)) and not ex["counts"][qb:].any(), ex["counts"]
    assert np.all(np.isposinf(ex["tau"][:qb])) and np.all(np.isneginf(ex["tau"][qb:])), ex["tau"]
    keys = ex["lists"][:qb, :n]
    rows, vals = ref.key_rows(keys), ref.key_values(keys)
    assert np.array_equal(np.sort(rows, axis=1), np.broadcast_to(np.arange(n), (qb, n))), "a row listed twice or not at all"
    out = np.empty((qb, n), np.float32)
    np.put_along_axis(out, rows, vals, axis=1)
    return out


def ratio_of(form, B, got, want):
    lim = ref.allowed(form, B, want)
    dev = np.abs(got.astype(np.float64) - want)
    return np.where(lim > 0, dev / np.where(lim > 0, lim, 1.0), np.where(dev > 0, np.inf, 0.0))


def check_constants(form, ex, q, rows, a, b):
    """sq and rowsum against float64: nf 2^-24 relative for the float sums, 2^-24 for the entropies added up in double (plus what
    nf <= 128 double additions and the device's double log2 may differ by: 2^-45 of the sum of the terms' magnitudes)"""
    nf, qb, n = b - a, q.shape[0], rows.shape[0]
    if form == ref.FORM_APPROX:
        return
    sums_q, sums_r = ref.range_sums(q, a, b), ref.range_sums(rows, a, b)
    assert np.all(np.isfinite(ex["sq"][:qb])) and np.all(np.isfinite(ex["rowsum"]))
    assert abs(float(ex["rowsum"][n]) - sums_r.max()) <= nf * U24 * sums_r.max(), "largest row sum"
    if form == ref.FORM_HARM:
        assert np.all(np.abs(ex["sq"][:qb] - sums_q) <= nf * U24 * sums_q), "query sums"
        assert np.all(np.abs(ex["rowsum"][:n] - sums_r) <= nf * U24 * sums_r), "row sums"
    else:
        for got, x in ((ex["sq"][:qb], q), (ex["rowsum"][:n], rows)):
            e = ref.range_entropies(x, a, b)
            v = np.asarray(x, np.float64)[:, a:b]
            mag = (np.abs(np.where(v > 0, v * np.log2(np.where(v > 0, v, 1.0)), 0.0)) + v).sum(axis=1)
            assert np.all(np.abs(got - e) <= U24 * np.abs(e) + 2.0 ** -45 * mag + 2.0 ** -149), "entropies"


A_PARAMS = [(kind, d, form, samples) for kind in ref.KINDS for d in (96, 100) for form, samples in FORM_SAMPLES]


@pytest.mark.parametrize("kind,d,form,samples", A_PARAMS)
def test_every_rows_nomination_value_is_within_the_bound(fir, monkeypatch, kind, d, form, samples):
    """A: all_rows mode, 4000 rows (62 full tiles and a 32-row one), d = 96 and 100, batches of 40, 12 and 8 queries (an odd number of
    16-query reads, a tile and a half, one tile), every range of nomination_scan_ref.ranges and every input kind."""
    metric, fm, _ = FORMS[form]
    _knobs(monkeypatch, form, samples)
    rows, q = _case(kind, d)
    worst = worst_floor = 0.0
    with fir.Gallery(rows, None, metric, 0) as g:
        for a, b in ref.ranges(d):
            want = _reference(metric, kind, d, a, b)
            B = ref.bound(fm, q, rows, a, b)
            for nq in (QB, 12, 8) if samples == "nomination" or form == "chi2_approx" else (QB,):
                ex = read_out(fir, g, q[:nq], a, b, 1, 1)
                per_read = 8 if fm == ref.FORM_APPROX else 16            # (k_nominate takes two tiles of 8 queries per gallery read)
                assert ex["metric"] == fm and ex["qpad"] == (nq + per_read - 1) // per_read * per_read, (a, b, nq, ex["metric"], ex["qpad"])
                got = values_of_all_rows(ex, nq, N)
                assert np.all(np.isfinite(got)), (a, b, nq, "a NaN or inf nomination value")
                r = ratio_of(fm, B[:nq], got, want[:nq])
                floor_only = (B[:nq] <= ref.ENT_FLOOR) & (fm == ref.FORM_ENT)          # the query and every row 0 over the range
                worst = max(worst, float(r[~floor_only].max(initial=0.0)))
                worst_floor = max(worst_floor, float(r[floor_only].max(initial=0.0)))
                bad = np.argwhere(r > 1.0)
                assert bad.size == 0, (a, b, nq, "|value - reference| > B", float(r.max()), bad[:6].tolist())
                check_constants(fm, ex, q[:nq], rows, a, b)
    print(f"nomination_scan_ratio form={form} samples={samples} kind={kind} d={d} largest |value - float64| / B = {worst:.4f}"
          + (f" (all-zero ranges, B = 2^-93: {worst_floor:.4f})" if worst_floor else ""))


def _groups(ex, k):
    """group of every row (-1: not sampled): tile t of the first group_tiles * K tiles belongs to group t mod K"""
    tiles = np.arange(N) // ref.TILE_ROWS
    gt = ex["group_tiles"]
    return np.where(tiles < gt * k, tiles % k, -1)


@pytest.mark.parametrize("kind,form,samples", [(kind, form, samples) for kind in ref.KINDS for form, samples in FORM_SAMPLES])
def test_thresholds_and_lists(fir, monkeypatch, kind, form, samples):
    """B: normal mode over the 4000 x 96 gallery, K = 1 and 5, a whole-chunk and a ragged range. Every row's nomination value comes
    from an all_rows run of the same call, the exact distances from range_distances of the same handle."""
    metric, fm, _ = FORMS[form]
    d = 96
    rows, q = _case(kind, d)
    approx = samples == "nomination"
    with fir.Gallery(rows, None, metric, 0) as g:
        for a, b in ((0, 96), (5, 93)):
            nf = float(b - a)
            want = _reference(metric, kind, d, a, b)
            B = ref.bound(fm, q, rows, a, b)
            lim = ref.allowed(fm, B, want)
            monkeypatch.setenv("FIR_NO_CHI2_NOMINATION", "1")
            exact = g.range_distances(q, a, b)
            _knobs(monkeypatch, form, samples)
            allv = values_of_all_rows(read_out(fir, g, q, a, b, 1, 1), QB, N)
            for k in (1, 5):
                ex = read_out(fir, g, q, a, b, k, 0)
                tag = (a, b, k)
                assert ex["metric"] == fm and ex["flag"] == 0, tag
                cnt, tau = ex["counts"][:QB].astype(np.int64), ex["tau"][:QB]
                assert not ex["counts"][QB:].any() and np.all(np.isneginf(ex["tau"][QB:])), tag
                assert np.all(np.isfinite(tau)) and cnt.max() <= ref.LIST_CAP, tag
                assert int((want <= tau[:, None].astype(np.float64)).sum(axis=1).max()) < ref.LIST_CAP, tag
                # the samples
                assert ex["group_tiles"] == max(1, min(((N + 63) // 64) // k, (max(16384, N * k // 256) // k + 63) // 64)), tag
                grp = _groups(ex, k)
                srow, sval = ref.key_rows(ex["skeys"][:, :QB]), ref.key_values(ex["skeys"][:, :QB]).astype(np.float64)
                qi = np.broadcast_to(np.arange(QB)[None, :], srow.shape)
                assert np.all((srow >= 0) & (srow < N)), tag
                assert np.array_equal(grp[srow], np.broadcast_to(np.arange(k)[:, None], srow.shape)), (tag, "a sample key outside its group")
                assert np.all(np.abs(sval - want[qi, srow]) <= lim[qi, srow]), (tag, "a sample key further than B from its row's reference")
                for i in range(k):
                    m = np.where(grp[None, :] == i, want, np.inf)
                    jmin = m.argmin(axis=1)
                    assert np.all(sval[i] <= m[np.arange(QB), jmin] + lim[np.arange(QB), jmin]), (tag, i, "a sample above its group's smallest reference + B")
                # the threshold
                top = sval.max(axis=0)
                t64 = tau.astype(np.float64)
                if fm == ref.FORM_APPROX:
                    sc = ref.approx_tau_scale(nf)
                    lo, hi, slack = top * sc, top * (1 + 2 * (sc - 1)), 6 * U24 * np.abs(t64) * (1 + B)
                else:
                    w = (2.5 if approx else 1.5) * B
                    lo, hi, slack = top + w, top + 2 * w, 6 * U24 * (np.abs(t64) + B)
                assert np.all(t64 >= lo - slack), (tag, "tau below the widening owed", float(((lo - t64) / np.maximum(B, 1e-300)).max()))
                assert np.all(t64 <= hi + slack), (tag, "tau above twice the widening")
                # the lists
                for i in range(QB):
                    keys = ex["lists"][i, :cnt[i]]
                    lrow, lval = ref.key_rows(keys), ref.key_values(keys)
                    under = np.flatnonzero(allv[i] <= tau[i])
                    assert np.array_equal(np.sort(lrow), under), (tag, i, "the listed rows are not {row : value <= tau}", cnt[i], len(under))
                    assert np.array_equal(lval.view(np.uint32), allv[i, lrow].view(np.uint32)), (tag, i, "a listed value differs from the all_rows run")
                    listed = np.zeros(N, bool)
                    listed[lrow] = True
                    e64 = exact[i].astype(np.float64)
                    must = e64 * (1 + 1.5 * B[i]) <= t64[i] if fm == ref.FORM_APPROX else e64 <= t64[i] - 1.5 * B[i]
                    assert np.all(listed[must]), (tag, i, "a row with exact distance <= tau - 1.5 B is not listed")
                    best = np.lexsort((np.arange(N), exact[i]))[:k]
                    assert np.all(listed[best]), (tag, i, "one of the K nearest rows is not listed", best.tolist())


def test_l2_candidate_lists_hold_the_exact_distances(fir, monkeypatch):
    """C: metric 0 through the same read-out -- the hand-scheduled append kernel over a whole-chunk range, the generic one over a ragged
    range: the listed values are range_distances' bits, the listed rows exactly {d <= tau}, and tau is the largest sample."""
    import synth

    _knobs(monkeypatch, "kl_ent", "nomination")
    rows = synth.make_gallery(211, N, 96, 0)
    q, _ = synth.make_queries(211, rows, QB, 0)
    with fir.Gallery(rows, None, 0, 0) as g:
        for a, b in ((0, 96), (5, 93), (32, 64)):
            exact = g.range_distances(q, a, b)
            for k in (1, 5):
                ex = read_out(fir, g, q, a, b, k, 0)
                tag = (a, b, k)
                assert ex["metric"] == 0 and ex["flag"] == 0 and ex["qpad"] == QB, tag
                cnt, tau = ex["counts"][:QB], ex["tau"][:QB]
                sval = ref.key_values(ex["skeys"][:, :QB])
                srow = ref.key_rows(ex["skeys"][:, :QB])
                assert np.array_equal(sval.view(np.uint32), exact[np.arange(QB)[None, :], srow].view(np.uint32)), tag
                assert np.array_equal(tau.view(np.uint32), sval.max(axis=0).view(np.uint32)), tag
                assert cnt.min() >= k and cnt.max() <= ref.LIST_CAP, tag
                for i in range(QB):
                    keys = ex["lists"][i, :cnt[i]]
                    lrow, lval = ref.key_rows(keys), ref.key_values(keys)
                    assert np.array_equal(np.sort(lrow), np.flatnonzero(exact[i] <= tau[i])), (tag, i)
                    assert np.array_equal(lval.view(np.uint32), exact[i, lrow].view(np.uint32)), (tag, i)


def _same_keys(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("metric", [ref.CHI2, ref.KL])
def test_public_path_at_the_smallest_gated_shape(fir, monkeypatch, metric):
    """D: 65 600 x 32, 16 queries: features 0 on both sides, in one member and in both members of a harmonic pair -- top-1 and top-5
    keys are the exact scan's bit for bit and the nomination scan is what ran. Then a gallery with two rows of 2^16 throughout (row
    sum 2^16 d): the bound swallows every distance, every list overflows, and the exact scan answers with the same keys."""
    n, d, qb = 65600, 32, 16
    _knobs(monkeypatch, "kl_ent", "nomination")
    for kind, nominated in (("pair_zero", True), ("dominant_row", False)):
        rows, q = ref.make_case(kind, n, d, qb)
        assert not nominated or (not rows[:, :2].any() and not q[:, :2].any() and not rows[:, 4:6].any() and q[:, 4:6].any())
        assert nominated or float(rows.sum(axis=1, dtype=np.float64).max()) == 2.0 ** 16 * d
        with fir.Gallery(rows, None, metric, 0) as g:
            a1 = g.search_top1(q)
            name1 = g.last_dispatch()["kernel"]
            a5 = g.search_topk(q, 5)
            name5 = g.last_dispatch()["kernel"]
            monkeypatch.setenv("FIR_NO_CHI2_NOMINATION", "1")
            e1 = g.search_top1(q)
            e5 = g.search_topk(q, 5)
            monkeypatch.delenv("FIR_NO_CHI2_NOMINATION")
        assert _same_keys(a1, e1) and _same_keys(a5, e5), kind
        assert ("k_nominate" in name1) == nominated and ("k_nominate" in name5) == nominated, (kind, name1, name5)
