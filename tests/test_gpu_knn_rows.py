"""The float64 kNN matrix-core path (fir_gemm_f64.h behind fir_cls_knn_predict) row by row: what the nomination and
k_gemm_rerank_f64 hand the vote -- the K' nearest rows (K' = 1 for k = 1, else 8), their distances and the certificate -- read
through the library's internal fir_cls_knn_rows_ and graded against knn_rows_ref.py, the reference's float64 arithmetic in numpy
(pinned to the oracle by test_knn_rows_formulation.py). A class is a coarse witness: a wrong nearest row of the right class, a
wrong tie-break, a wrong distance and a certificate set wrongly are all invisible to it.

Per query, for K' = 1 and K' = 8
  soundness     every listed row is in [0, nt) and listed once, -1 slots trail with distance +inf, every listed distance has the
                reference's bits for that row, the list ascends by (distance, row); the nomination lists (fir_gemm_nominations_ on
                the handle's state, fir_cls_knn_state_) have counts >= 0 and name rows < nt, each once
  certificate   ok == 1: rows and distances are nearest(reference, K') exactly
  no hiding     every query with finite operands of ordinary magnitude comes back ok == 1. The cap on uncertified queries is 0 and
                derived, not measured: every training set here has nt <= 4096 = kListCap rows and a row is appended at most once per
                query, so no list overflows. Every proxy is within W = e_rel (|q'|^2 + max |g'|^2) of its row's true
                |g'|^2 - 2 q'.g' (e_rel = 8 d 2^-24 + 2^-10 (1 + 2^-4); fir_gemm_rerank.h) and the bound the pass ends with is a
                K'-th smallest proxy of some set of rows + 2.5 W (k_gemm_seed_T, k_gemm_adapt_final): at least 1.5 W above the true
                K'-th smallest (asserted from the state's tau). The re-rank takes every listed row up to 2 W above the K'-th
                smallest listed proxy; the smallest proxy it leaves out, or tau, is p_excl > (K'-th proxy) + 2 W, so the
                certificate's lower bound (|q'|^2 + p_excl) / d - W / d exceeds ((K'-th proxy) + |q'|^2 + W) / d >= the K'-th exact
                distance found. Fewer than K' rows: everything is listed and re-ranked.
The argument needs every float of the pass to be an ordinary number. FINDING of this test's scale sweep (case F): it was not
guarded. k_gemm_qprep_f16_f64 let every query through whose own scale exponent and the training set's were inside [-100, 100]
EACH, but qinv = 2^-(sh + gallery_exp) underflows to 0 from element magnitudes of about 2^-61 down (every proxy is then the row's
norm alone, whatever the query) and E = e_rel (|q'|^2 + max |g'|^2) / d goes denormal and then 0 a little earlier than the norms:
queries came back ok == 1 with a wrong nearest row. The preparation now also refuses |sh + gallery_exp| > 120 (qinv, the norms,
the window and E are then normal floats with room); such queries are uncertified and the exact scan answers them.

Cases: A row length (every 16-row kernel form from float64 rows: one unit, even, odd, streamed odd, streamed even; odd d, d no
multiple of 16), B row count (tiles of 32 and 64 rows, fewer rows than K'), C the K'-best merge of k_gemm_rerank_f64 (equal
distances at its seams: 8 slots, batches of 64 list entries; a family of rows one ulp apart), D the longest rows the path takes
(the re-rank's LDS query above 48 KiB) and the first length it refuses, E non-finite, huge and degenerate queries, F powers of
two from 2^-140 to 2^120. Then, through fir_cls_knn_predict alone: one row per class (the class IS the row) and the batch seams
at 8192 and 16384 queries."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import knn_rows_ref as ref
from test_gpu_cls_forms import clustered
from test_gpu_gemm_nominations import nominations

pytestmark = pytest.mark.gpu

F32 = np.float32
K_LIST_CAP = 4096
FIR_ERR_ARG = -1
NT, QB = 2999, 200                                   # rows: no multiple of 32 or 64; queries: one full pair of passes and a ragged one
A_DIMS = {1: (0, 2), 3: (0, 2), 33: (0, 2), 127: (0, 2), 129: (0, 0), 300: (0, 1), 513: (1, 1), 700: (1, 0)}     # d: (STREAMED, ODD)
COPIES = (1, 7, 8, 9, 64, 65, 200)
SCALES = (-140, -90, -78, -74, -72, -70, -66, -60, -40, 40, 60, 64, 90, 120)


class Data:
    def __init__(self, tr, tcls, ncls, avg, q, ref_d=None):
        self.tr, self.tcls, self.ncls, self.avg, self.q = tr, np.ascontiguousarray(tcls, np.int32), ncls, avg, q
        self.nt, self.d = tr.shape
        self.ref_d = ref.mean_distances(tr, avg, q) if ref_d is None else ref_d
        for a in (self.tr, self.tcls, self.avg, self.q, self.ref_d):
            a.setflags(write=False)

    def model(self, fir):
        return fir.ClsModel(self.tr, self.tcls, self.ncls, self.avg, 0)


def e_rel_of(d):
    """fir_gemm_knn_f64_'s e_rel, in float32 as the library forms it"""
    return F32(8.0) * F32(d) * F32(5.9604645e-8) + F32(9.765625e-4) * F32(1.0625)


class _State:
    def __init__(self, h):
        self._h = h


def _hooks(fir):
    lib = C.CDLL(fir.lib_path())
    rows_fn, state_fn = lib.fir_cls_knn_rows_, lib.fir_cls_knn_state_
    rows_fn.restype = C.c_int
    rows_fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    state_fn.restype = C.c_void_p
    state_fn.argtypes = [C.c_void_p]
    lib.fir_last_error.restype = C.c_char_p
    return lib, rows_fn, state_fn


def knn_rows(fir, m, q, kp):
    """fir_cls_knn_rows_: (rows[qb, kp], dist[qb, kp], ok[qb]) of the nominate + re-rank step; the kNN counters stay put"""
    lib, rows_fn, _ = _hooks(fir)
    q = np.ascontiguousarray(q, np.float64)
    qb = q.shape[0]
    rows, dist, ok = np.full((qb, kp), -7, np.int32), np.full((qb, kp), np.nan), np.full(qb, -7, np.int32)
    before = m.knn_stats()
    rc = rows_fn(m._h, q.ctypes.data, qb, kp, rows.ctypes.data, dist.ctypes.data, ok.ctypes.data)
    if rc:
        raise fir.FirError(rc, lib.fir_last_error().decode(errors="replace"))
    assert m.knn_stats() == before
    return rows, dist, ok


def knn_state(fir, m):
    """the handle's float64 nomination state as something nominations() takes (None: none yet)"""
    h = _hooks(fir)[2](m._h)
    return _State(h) if h else None


def check_sound(rows, dist, ok, ref_d, nt, label):
    assert np.all((ok == 0) | (ok == 1)), (label, np.unique(ok))
    valid = rows >= 0
    assert np.all(rows[valid] < nt) and np.all(rows[~valid] == -1), (label, "a row outside [0, nt)")
    assert np.all(valid[:, :-1] >= valid[:, 1:]), (label, "an empty slot in front of a row")
    assert np.all(np.isposinf(dist[~valid])), (label, "an empty slot with a distance")
    want = np.take_along_axis(ref_d, np.where(valid, rows, 0).astype(np.int64), axis=1)
    diff = valid & (dist.view(np.uint64) != want.view(np.uint64))
    assert not diff.any(), (label, "a distance that is not the reference's for its row", np.argwhere(diff)[:4].tolist(),
                            dist[diff][:4], want[diff][:4])
    both = valid[:, 1:]
    asc = (dist[:, :-1] < dist[:, 1:]) | ((dist[:, :-1] == dist[:, 1:]) & (rows[:, :-1] < rows[:, 1:]))
    assert np.all(asc[both]), (label, "not ascending by (distance, row), or a row twice", np.argwhere(both & ~asc)[:4].tolist())


def check_lists(ex, qb, nt, label):
    cnt = ex["counts"].astype(np.int64)
    assert len(cnt) == qb and np.all(cnt >= 0) and np.all(cnt <= nt), (label, "counts", int(cnt.min(initial=0)), int(cnt.max(initial=0)))
    L = ex["lists"]
    valid = np.arange(L.shape[1])[None, :] < np.minimum(cnt, K_LIST_CAP)[:, None]
    row = (L & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.all(row[valid] < nt), (label, "a listed row past the end", int(row[valid].max()))
    s = np.sort(np.where(valid, row, -1 - np.arange(L.shape[1])[None, :]), axis=1)
    assert np.all(s[:, 1:] != s[:, :-1]), (label, "a row listed twice")


def check_bound(ex, data, q, ref_d, kp, label):
    """tau >= (true K'-th smallest |g'|^2 - 2 q'.g') + 1.5 W, and the float norms the window is made of"""
    if data.nt < kp:
        return
    qn64 = ((q - data.avg) ** 2).sum(axis=1)
    gmax64 = ((data.tr - data.avg) ** 2).sum(axis=1).max()
    assert np.allclose(ex["qnorm"], qn64, rtol=2.0 ** -22, atol=0), label
    assert np.isclose(float(ex["gmax"]), gmax64, rtol=2.0 ** -22, atol=0), label
    kth = np.partition(ref_d, kp - 1, axis=1)[:, kp - 1] * data.d - qn64
    W = float(e_rel_of(data.d)) * (qn64 + gmax64)
    over = ex["tau"].astype(np.float64) - kth
    room = np.where(W > 0, over / np.where(W > 0, W, 1.0), np.where(over >= 0, np.inf, -np.inf))      # (one row, the query itself: W = 0)
    print(label, "K'", kp, "(tau - true K'-th proxy) / W: min %.3f" % room.min())
    # (the float32 roundings of T = (p + |q'|^2) + w and tau = T - |q'|^2: 4 u (|q'|^2 + |tau| + w) <= 12 u (|q'|^2 + max |g'|^2) < 1e-3 W)
    assert np.all(room >= 1.5 - 2e-3), (label, "a bound less than 1.5 W above the K'-th smallest proxy", float(room.min()))


def grade(fir, m, data, kp, label, q=None, ref_d=None, all_ok=True, bound=True):
    """one call of the hook, graded; returns (rows, dist, ok)"""
    q = data.q if q is None else q
    ref_d = data.ref_d if ref_d is None else ref_d
    rows, dist, ok = knn_rows(fir, m, q, kp)
    ex = nominations(fir, knn_state(fir, m))
    check_sound(rows, dist, ok, ref_d, data.nt, label)
    check_lists(ex, q.shape[0], data.nt, label)
    sel = ok == 1
    assert not np.isnan(ref_d[sel]).any(), (label, "a certified query with NaN distances")
    want_r, want_d = ref.nearest(ref_d[sel], kp)
    wrong = np.nonzero((rows[sel] != want_r).any(axis=1) | (dist[sel].view(np.uint64) != want_d.view(np.uint64)).any(axis=1))[0]
    print(label, "K'", kp, "queries", len(ok), "uncertified", int((~sel).sum()), "certified with other rows than the reference's", len(wrong),
          "longest list", int(ex["counts"].max(initial=0)))
    assert len(wrong) == 0, (label, "certified, but not the reference's nearest rows", np.nonzero(sel)[0][wrong][:8].tolist(),
                             rows[sel][wrong][:2].tolist(), want_r[wrong][:2].tolist())
    if all_ok:
        assert sel.all(), (label, "finite queries that were not certified", np.nonzero(~sel)[0][:8].tolist())
    if bound:
        check_bound(ex, data, q, ref_d, kp, label)
    return rows, dist, ok


# ---- A: row length ----

@functools.lru_cache(maxsize=None)
def set_a(kind, d):
    if kind == "clustered":
        tr, tcls, q = clustered(NT, d, 23, 700 + d, QB)               # about 130 rows of the query's class inside each window
    else:
        rng = np.random.default_rng(700 + d)
        tr = rng.random((NT, d))
        tcls = np.sort(rng.integers(0, 23, NT)).astype(np.int32)
        q = rng.random((QB, d))
        q[::2] = tr[rng.integers(0, NT, QB // 2)] + 0.01 * rng.standard_normal((QB // 2, d))
    return Data(tr, tcls, 23, tr.mean(0), q)


@pytest.mark.parametrize("kind", ["random", "clustered"])
@pytest.mark.parametrize("d", sorted(A_DIMS))
def test_a_row_length(fir, kind, d):
    """d = 1, 3, 33, 127: one unit of 128 features (ODD = 2); 129: two; 300: three (ODD = 1, never run from float64 rows before);
    513: five, streamed; 700: six, streamed. Odd d takes the packers' k + 1 < kmax arm (dp2 = (d + 1) / 2)."""
    data = set_a(kind, d)
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        assert knn_state(fir, m) is None
        m.profile_enable(True)
        for kp in (1, 8):
            grade(fir, m, data, kp, "A %s d=%d" % (kind, d))
            name = m.last_dispatch()["kernel"]
            got = re.search(r"k_gemm_proxy_f16x<(\d), (\d), (\d)>", name)
            assert got, name
            assert (int(got.group(2)), int(got.group(3))) == A_DIMS[d], (d, name)
            assert int(got.group(1)) in ((1, 3) if kp == 1 else (1, 4)), (kp, name)
        m.profile_enable(False)
        with pytest.raises(fir.FirError) as e:
            knn_rows(fir, m, data.q[:4], 5)                            # production uses K' = 1 and 8 only
        assert e.value.code == FIR_ERR_ARG


# ---- B: row count ----

@pytest.mark.parametrize("nt", [1, 5, 8, 9, 31, 32, 33, 63, 64, 65, 4096])
def test_b_row_count(fir, nt):
    """d = 130 (dp2 = 65: the re-rank's group of eight loads clamps at the row's end), 130 queries; row counts around the packers'
    32-row blocks and the 64-row tiles, fewer rows than K' (padded slots, certified: every row was re-ranked), and a list that can
    be exactly full."""
    d, qb = 130, 130
    rng = np.random.default_rng(900 + nt)
    tr = rng.random((nt, d))
    ncls = min(nt, 3)
    q = rng.random((qb, d))
    q[:8] = tr[rng.integers(0, nt, 8)]
    data = Data(tr, (np.arange(nt) * ncls) // nt, ncls, tr.mean(0), q)
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        for kp in (1, 8):
            rows, dist, ok = grade(fir, m, data, kp, "B nt=%d" % nt)
            assert np.all((rows >= 0).sum(axis=1) == min(nt, kp))


# ---- C: the K'-best merge ----

@functools.lru_cache(maxsize=None)
def set_c():
    """2999 x 130; row 3 + 7 j exists COPIES[j] times (the other copies scattered over the rows from 64 on), query j is that row:
    1, 7, 8, 9, 64, 65, 200 list entries with the same proxy and the same distance +0.0 -- fewer than the eight slots, exactly
    eight, one more, one batch of 64 list entries, one more, several batches. Ten more rows are one base vector plus j = 1..10 ulps
    in one feature, at row positions that do not ascend with j; query 7 is the base vector (not a row)."""
    d = 130
    rng = np.random.default_rng(77)
    tr = rng.random((NT, d))
    q = rng.random((130, d))
    perm = rng.permutation(np.arange(64, NT))
    copies, at = [], 0
    for j, c in enumerate(COPIES):
        copies.append(np.sort(np.concatenate(([3 + 7 * j], perm[at:at + c - 1]))))
        at += c - 1
    fam = perm[at:at + 10]
    base = rng.random(d)
    f = 17
    base[f] = 0.625                                       # (g - avg is exact for g in [avg / 2, 2 avg], avg about 0.5; ulp = 2^-53 up to 1)
    for j, rr in enumerate(copies):
        tr[rr] = tr[3 + 7 * j]
        q[j] = tr[3 + 7 * j]
    for j in range(1, 11):
        tr[fam[j - 1]] = base
        tr[fam[j - 1], f] = 0.625 + j * 2.0 ** -53
    q[7] = base
    data = Data(tr, (np.arange(NT) * 37) // NT, 37, tr.mean(0), q)
    return data, copies, fam


def test_c_merge_seams_equal_distances_and_a_family_one_ulp_apart(fir):
    data, copies, fam = set_c()
    # the reference alone: the family's distances are (j ulp)^2 / d exactly, in the order of j
    want = np.array([(j * 2.0 ** -53) ** 2 / data.d for j in range(1, 11)])
    assert np.array_equal(data.ref_d[7, fam], want) and 0.25 < data.avg[17] < 1.0
    assert np.array_equal(ref.nearest(data.ref_d[7:8], 8)[0][0], fam[:8])
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        for kp in (1, 8):
            rows, dist, ok = grade(fir, m, data, kp, "C")
            for j, rr in enumerate(copies):
                have = min(len(rr), kp)
                print("C K'", kp, "copies", len(rr), "rows", rows[j].tolist())
                assert np.array_equal(rows[j, :have], rr[:have]), (kp, j, rows[j].tolist(), rr[:8].tolist())
                assert np.all(dist[j, :have].view(np.uint64) == 0), (kp, j, dist[j])         # +0.0
            assert np.array_equal(rows[7], fam[:kp]) and np.array_equal(dist[7], want[:kp]), (kp, rows[7], fam[:8])


# ---- D: long rows ----

@pytest.mark.parametrize("nt,d", [(300, 6144), (300, 6145), (70, 18432)])
def test_d_long_rows(fir, nt, d):
    """dk16 = 384, 392 and 1152 sixteen-feature pieces per row block (the float32 path ends at 288); d = 6145: the first length whose
    centred query exceeds 48 KiB of LDS in k_gemm_rerank_f64 (hipFuncSetAttribute); 18432: the longest the path takes (144 KiB).
    fir_cls_create takes all three."""
    rng = np.random.default_rng(d)
    tr = rng.random((nt, d))
    q = rng.random((130, d))
    q[:40] = tr[rng.integers(0, nt, 40)] + 0.05 * rng.standard_normal((40, d))
    data = Data(tr, (np.arange(nt) * 3) // nt, 3, tr.mean(0), q)
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        for kp in (1, 8):
            grade(fir, m, data, kp, "D %dx%d" % (nt, d))


def test_d_one_feature_too_many_is_refused_when_forced_and_answered_by_the_scan(fir):
    nt, d, qb = 70, 18433, 130
    rng = np.random.default_rng(d)
    tr = rng.random((nt, d))
    q = tr[rng.integers(0, nt, qb)] + 0.05 * rng.standard_normal((qb, d))
    data = Data(tr, (np.arange(nt) * 3) // nt, 3, tr.mean(0), q)
    off = ref.class_offsets(data.tcls, 3)
    want = [ref.vote(data.ref_d[i], off, 3) for i in range(qb)]
    assert not any(t for _, _, t in want)
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        with pytest.raises(fir.FirError) as e:
            m.knn_predict(q, 3)
        assert e.value.code == FIR_ERR_ARG and "too long" in str(e.value), str(e.value)
        m.set_knn_mfma(0)
        got = m.knn_predict(q, 3)
    assert np.array_equal(got, [c for c, _, _ in want])


# ---- E: bad and odd queries ----

def test_e_bad_and_odd_queries(fir):
    """On A's 2999 x 129 random set: a NaN feature, +inf, -inf, 1e300 (its square is not a double), the average itself (a centred
    query of zeros), a training row. The first four must be uncertified -- their rows, if any, still sound --, the rest certified;
    through fir_cls_knn_predict every class is the exact scan's."""
    base = set_a("random", 129)
    q = base.q.copy()
    q[0, 5] = np.nan
    q[1, 6] = np.inf
    q[2, 128] = -np.inf
    q[3, 0] = 1e300
    q[4] = base.avg
    q[5] = base.tr[1234]
    data = Data(base.tr, base.tcls, base.ncls, base.avg, q)
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        for kp in (1, 8):
            rows, dist, ok = grade(fir, m, data, kp, "E", all_ok=False, bound=False)
            assert not ok[:4].any() and ok[4:].all(), (kp, np.nonzero(ok == 0)[0][:8].tolist())
            assert rows[5, 0] == 1234 and dist[5, 0] == 0.0
        got = {k: m.knn_predict(q, k) for k in (1, 3)}
        st = m.knn_stats()
        m.set_knn_mfma(0)
        exact = {k: m.knn_predict(q, k) for k in (1, 3)}
    assert st["matrix_core_queries"] == 2 * QB and st["exact_scan_queries_of_them"] >= 8, st
    for k in (1, 3):
        assert np.array_equal(got[k], exact[k]), k


# ---- F: scale ----

@functools.lru_cache(maxsize=None)
def set_f(kind):
    if kind == "random":
        return set_a("random", 129)
    # the coherent-rounding pair of test_gpu_cls.py's certificate test: every component of row A rounds DOWN to fp16, every component
    # of row B UP, so B's proxy is lower than A's by 0.77 of a window although A is the query itself; avg = 0
    rng = np.random.default_rng(91)
    d = 512
    tr = rng.random((NT, d))
    ia, ib = NT // 3, 2 * NT // 3 + 5
    tr[ia] = 1.0 + 0.499 * 2.0 ** -10
    tr[ib] = 1.0 + 0.501 * 2.0 ** -10
    q = np.vstack([tr[ia]] + [tr[i] * 0.999 for i in (7, 99, 1234)] + [rng.random(d) for _ in range(126)])
    data = Data(tr, (np.arange(NT) >= NT // 2).astype(np.int32), 2, np.zeros(d), q)
    assert ref.nearest(data.ref_d[:1], 2)[0][0].tolist() == [ia, ib]
    return data


@pytest.mark.parametrize("kind", ["random", "pair"])
@pytest.mark.parametrize("e", (0,) + SCALES)
def test_f_powers_of_two(fir, kind, e):
    """Rows, average and queries times 2^e, exact in float64: every distance is the unscaled one times 4^e, bit for bit, and the
    nearest rows are the same. A certified query has the reference's rows at EVERY scale (the float norms, the window and the
    bound overflow, go denormal or vanish on the way out: the sweep looks for a certificate that survives that); |e| <= 40: every
    query is certified; e = -140 and 120, outside the scale guard: none is, and the exact scan answers all of them."""
    base = set_f(kind)
    s = 2.0 ** e
    ref_d = base.ref_d * 4.0 ** e
    assert np.all(ref_d > 0.0 if kind == "random" else ref_d >= 0.0) and np.all(np.isfinite(ref_d)) and np.all(ref_d[ref_d > 0] > 1e-290)
    data = Data(base.tr * s, base.tcls, base.ncls, base.avg * s, base.q * s, ref_d)
    qb = data.q.shape[0]
    inside = abs(e) <= 40
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        for kp in (1, 8):
            rows, dist, ok = grade(fir, m, data, kp, "F %s e=%d" % (kind, e), all_ok=inside, bound=inside)
            if inside:
                r0, d0 = ref.nearest(base.ref_d, kp)
                assert np.array_equal(rows, r0) and np.array_equal(dist, d0 * 4.0 ** e)
            if e in (-140, 120):
                assert not ok.any(), np.nonzero(ok)[0][:8].tolist()
        if e in (-140, 120):
            got = m.knn_predict(data.q, 1)
            st = m.knn_stats()
            assert st["matrix_core_queries"] == qb and st["exact_scan_queries_of_them"] == qb, st
            r0, d0 = ref.nearest(base.ref_d, 2)
            clear = d0[:, 0] != d0[:, 1]
            off = ref.class_offsets(base.tcls, base.ncls)
            assert clear.sum() >= qb - 1
            assert np.array_equal(got[clear], (np.searchsorted(off, r0[:, 0], side="right") - 1)[clear])


# ---- through the public call only ----

@pytest.mark.parametrize("d", [300, 513])
def test_one_row_per_class_the_class_is_the_row(fir, d):
    """train_class = arange(nt), k = 1: fir_cls_knn_predict's answer IS the nearest row, through the vote and the delivery."""
    base = set_a("random", d)
    want, wd = ref.nearest(base.ref_d, 2)
    assert np.all(wd[:, 0] < wd[:, 1])                                 # no equal distances: the vote may not send anything on
    with fir.ClsModel(base.tr, np.arange(NT, dtype=np.int32), NT, base.avg, 0) as m:
        m.set_knn_mfma(1)
        got = m.knn_predict(base.q, 1)
        st = m.knn_stats()
    print("one row per class d", d, st, "wrong", int((got != want[:, 0]).sum()))
    assert np.array_equal(got, want[:, 0])
    assert st == {"matrix_core_queries": QB, "exact_scan_queries_of_them": 0}, st


@functools.lru_cache(maxsize=None)
def set_seams():
    """1500 x 40 in 50 well-separated classes of 30 rows, 16384 + 70 queries; the reference's nearest nine rows of every query"""
    nt, d, ncls, qb = 1500, 40, 50, 16384 + 70
    rng = np.random.default_rng(5)
    centres = rng.random((ncls, d))
    tcls = (np.arange(nt) // 30).astype(np.int32)
    tr = centres[tcls] + 0.01 * rng.standard_normal((nt, d))
    pick = rng.integers(0, ncls, qb)
    q = centres[pick] + 0.01 * rng.standard_normal((qb, d))
    data = Data(tr, tcls, ncls, tr.mean(0), q)
    order = np.argsort(data.ref_d, axis=1, kind="stable")[:, :9]       # (stable: by (distance, row), as nearest() orders)
    near_d = np.take_along_axis(data.ref_d, order, axis=1)
    for a in (order, near_d):
        a.setflags(write=False)
    return data, order, near_d


@pytest.mark.parametrize("qb", [8192 + 130, 16384 + 70])
def test_batch_seams(fir, qb):
    """More than one super-batch of 8192 queries inside fir_gemm_knn_f64_ (q0 offsets into rows, dist and ok) and more than one
    batch of 16384 inside fir_cls_knn_predict. k = 1 with one row per class: the class is the row. k = 3 with the 50 classes: from
    the reference alone every walk ends inside the 8 nearest rows and meets no equal distance (asserted first), and every finite
    query is certified (above), so nothing may take the exact scan: the cap is 0."""
    data, order, near_d = set_seams()
    order, near_d, q = order[:qb], near_d[:qb], data.q[:qb]
    assert np.all(near_d[:, 1:] > near_d[:, :-1])                      # no equal distances among the nine nearest
    cls9 = order // 30
    votes = np.cumsum(cls9[:, :8, None] == np.arange(data.ncls)[None, None, :], axis=1)        # [qb, 8, classes]
    done = (votes >= 3).any(axis=2)
    assert done.any(axis=1).all()                                      # every walk of k = 3 ends inside 8 rows
    at = done.argmax(axis=1)
    want3 = np.take_along_axis(votes, at[:, None, None], axis=1)[:, 0, :].argmax(axis=1)
    for i in (0, 1, qb // 2, qb - 1):                                  # the vectorised walk against knn_rows_ref.vote
        assert ref.vote(data.ref_d[i], np.arange(0, 1501, 30), 3) == (want3[i], at[i] + 1, False)
    with fir.ClsModel(data.tr, np.arange(data.nt, dtype=np.int32), data.nt, data.avg, 0) as m:
        m.set_knn_mfma(1)
        got1 = m.knn_predict(q, 1)
        st1 = m.knn_stats()
    with data.model(fir) as m:
        m.set_knn_mfma(1)
        got3 = m.knn_predict(q, 3)
        st3 = m.knn_stats()
    bad1, bad3 = np.nonzero(got1 != order[:, 0])[0], np.nonzero(got3 != want3)[0]
    print("seams qb", qb, "k=1", st1, "wrong", len(bad1), bad1[:6].tolist(), "k=3", st3, "wrong", len(bad3), bad3[:6].tolist())
    assert len(bad1) == 0 and len(bad3) == 0
    for st in (st1, st3):
        assert st == {"matrix_core_queries": qb, "exact_scan_queries_of_them": 0}, st
