"""The chi-square / KL nomination scans of the candidate-list path (csrc/fir_capi.hip: topk_lists_dev) in plain numpy float64: the
reference's distances, the three error bounds as fir_capi.hip derives them, and the inputs the bounds have to survive.
tests/test_nomination_scan_formulation.py holds a float32 emulation of the three forms to these bounds on the CPU;
tests/test_gpu_nomination_scans.py holds the kernels' own values, thresholds and lists to them."""
import numpy as np

U24 = 2.0 ** -24                 # u, half an ulp of 1.0f
LIST_CAP = 4096                  # kListCap
TILE_ROWS = 64
PLAIN_LO, PLAIN_HI = np.float32(2.0 ** -26), np.float32(2.0 ** 16)

CHI2, KL = 1, 2                  # FIR_METRIC_*
FORM_APPROX, FORM_HARM, FORM_ENT = 5, 6, 7      # kChi2Approx, kChi2Harm, kKLEnt (csrc/fir_common.h)


# ---- the reference (qt_cpp/db_features.cpp:22-42), float64 --------------------------------------------------------------------
def feature_terms(metric, q, rows, start, end):
    """t[k - start, qi, row] = feature k's term of the reference's sum, float64. Chi-square skips l + r = 0, KL skips the zero
    operand of a pair (db_features.cpp:29-36)."""
    q = np.asarray(q, np.float64)
    rows = np.asarray(rows, np.float64)
    out = np.zeros((end - start, q.shape[0], rows.shape[0]), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(start, end):
            l, r = q[:, k][:, None], rows[:, k][None, :]
            s = l + r
            live = s > 0
            s1 = np.where(live, s, 1.0)
            if metric == CHI2:
                df = l - r
                out[k - start] = np.where(live, df * df / s1, 0.0)
            else:
                tl = np.where(live & (l > 0), l * np.log(np.where(l > 0, 2.0 * l, 1.0) / s1), 0.0)
                tr = np.where(live & (r > 0), r * np.log(np.where(r > 0, 2.0 * r, 1.0) / s1), 0.0)
                out[k - start] = tl + tr
    return out


def distances(metric, q, rows, start, end, terms=None):
    """out[qi, row] = the reference's distance over features [start, end) in float64: the sum of the features' terms divided by
    their count (db_features.cpp:40). terms: feature_terms(metric, q, rows, 0, d), when many ranges are asked for."""
    t = feature_terms(metric, q, rows, start, end) if terms is None else terms[start:end]
    return t.sum(axis=0) / float(end - start)


def range_sums(x, start, end):
    """sum over [start, end) of every vector of x (the values are >= 0), float64"""
    return np.asarray(x, np.float64)[:, start:end].sum(axis=1)


def range_entropies(x, start, end):
    """sum over [start, end) of v log2 v + v, zeros skipped: Lq / Lg of the entropy form, float64"""
    v = np.asarray(x, np.float64)[:, start:end]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(v > 0, v * np.log2(np.where(v > 0, v, 1.0)) + v, 0.0).sum(axis=1)


# ---- the bounds, from the derivations above harm_bound_coef / entropy_bound_coef / approx_tau_scale ---------------------------
def harm_coef(nf):
    """|harmonic form - reference| <= B = (3 nf + 19) 2^-24 (sum(l) + max_rows sum(r)) / nf"""
    return (3.0 * nf + 19.0) * U24 / nf


def entropy_coef(nf):
    """|entropy form - reference| <= B = [ln2 (26.1 (64 + nf / 32) + 150) + 2 nf + 8] 2^-24 (sum(l) + max_rows sum(r)) / nf"""
    return (0.6932 * (26.1 * (64.0 + nf / 32.0) + 150.0) + 2.0 * nf + 8.0) * U24 / nf


ENT_FLOOR = 2.0 ** -93          # ... + 2^-93: the query tile holds l + 2^-100, a term of -100 * 2^-100 where l = r = 0 and the reference has none


def approx_rel(nf):
    """kChi2Approx: within (2 nf + 8) 2^-24 RELATIVE of the reference's value"""
    return (2.0 * nf + 8.0) * U24


def approx_tau_scale(nf):
    return 1.0 + 1.5 * (2.0 * nf + 16.0) * U24


def bound(form, q, rows, start, end):
    """B[qi] of the additive forms (6, 7) from the query's sum and the largest row sum over the range (form 7: + 2^-93, all there
    is of it when the query and every row are 0 over the range); for form 5 the relative bound, the same for every query."""
    nf = float(end - start)
    if form == FORM_APPROX:
        return np.full(np.asarray(q).shape[0], approx_rel(nf))
    s = range_sums(q, start, end) + range_sums(rows, start, end).max()
    return harm_coef(nf) * s if form == FORM_HARM else entropy_coef(nf) * s + ENT_FLOOR


def allowed(form, B, ref):
    """the deviation from `ref` [nq, n] the form is allowed: B[qi] itself, or B[qi] * ref for the relative bound of form 5"""
    B = np.asarray(B, np.float64)[:, None]
    return B * np.abs(ref) if form == FORM_APPROX else np.broadcast_to(B, ref.shape)


# ---- packed keys (csrc/fir_common.h: key_pack) --------------------------------------------------------------------------------
def key_values(keys):
    o = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)
    b = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o)
    return b.astype(np.uint32).view(np.float32)


def key_rows(keys):
    return (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
KINDS = ("l1", "both_zero", "pair_zero", "range_ends", "dominant_row", "unnormalised")
SEED = 20240611


def in_plain_range(x):
    x = np.asarray(x, np.float32)
    return bool(np.all((x.view(np.uint32) == 0) | ((x >= PLAIN_LO) & (x <= PLAIN_HI))))


def _l1(x):
    s = x.sum(axis=1, keepdims=True)
    s[s == 0] = 1
    return x / s


def make_case(kind, n, d, qb):
    """(rows[n, d], queries[qb, d]) float32, every value +0 or inside [2^-26, 2^16] (the gallery stays in the plain range), the
    same bits for the same arguments. Even queries are fresh draws, odd ones perturbed gallery rows, so near neighbours exist.
      l1            L1-normalised vectors, a tenth of the values 0 on either side (zeros coincide by chance)
      both_zero     ... and features that are 0 in every row AND every query, and queries that take over a row's zero pattern
      pair_zero     ... and harmonic pairs (4c, 4c+1), (4c+2, 4c+3) with one member or both members 0, in the rows, the queries, both
      range_ends    2^-26, 2^16, 0 and log-uniform values in between, mixed in every vector
      dominant_row  L1-normalised rows but for two rows of 2^16 throughout: max_rows sum(r) = 2^16 d
      unnormalised  values in [0, 100), rows and queries on different scales"""
    assert kind in KINDS
    rng = np.random.default_rng(SEED + 1000 * KINDS.index(kind) + d)
    rows = rng.random((n, d))
    rows[rng.random((n, d)) < 0.1] = 0
    fresh = rng.random((qb, d))
    fresh[rng.random((qb, d)) < 0.1] = 0
    pick = rng.integers(0, n, qb)
    pert = rows[pick] * (1 + 0.05 * (rng.random((qb, d)) - 0.5))
    q = np.where((np.arange(qb) % 2 == 0)[:, None], fresh, pert)
    if kind == "range_ends":
        def mix(shape):
            v = 2.0 ** rng.uniform(-26, 16, shape)
            c = rng.random(shape)
            v[c < 0.15] = 2.0 ** -26
            v[(c >= 0.15) & (c < 0.3)] = 2.0 ** 16
            v[(c >= 0.3) & (c < 0.4)] = 0
            return v
        rows, q = mix((n, d)), mix((qb, d))
        q[1::2] = rows[pick[1::2]]
        q[1::4, ::3] = 2.0 ** -26
    elif kind == "unnormalised":
        rows, q = rows * 100, q * 37
    else:
        rows, q = _l1(rows), _l1(q)
    if kind == "both_zero":
        cols = [c for c in (0, 5, 6, 7, 33, 34, d - 1) if c < d]
        rows[:, cols] = 0
        q[:, cols] = 0
        for i in range(qb):
            q[i, rows[(i * 97) % n] == 0] = 0
    if kind == "pair_zero":
        def z(a, cols):
            a[:, [c for c in cols if c < d]] = 0
        z(rows, (4, 5, 20)); z(q, (10, 11, 23))                   # a pair, one member: one side only
        z(rows, (0, 1, 34, 35, 64, 65)); z(q, (0, 1, 34, 35, 64, 65))          # both members, both sides
        rows[::5, 40:42] = 0
        q[::3, 40:42] = 0
        rows[::7, 46:48] = 0
        q[::2, 44:46] = 0
    if kind == "dominant_row":
        rows[n // 3] = 2.0 ** 16
        rows[n - 1] = 2.0 ** 16
    rows, q = rows.astype(np.float32), q.astype(np.float32)
    rows[rows < PLAIN_LO] = 0
    q[q < PLAIN_LO] = 0
    assert in_plain_range(rows) and in_plain_range(q)
    return rows, q


# feature ranges: ragged edges, inside one chunk, one to three features, and whole-chunk parts of 7, 8, 9, 16 and 17 chunks
# around the load group of 8 chunks (the last four with ragged edges on either side as well)
def ranges(d):
    out = [(0, d), (5, d - 3), (33, 35), (3, 70), (0, 1), (4, 7)]
    out += [(0, 28), (1, 33), (4, 36), (2, 38), (3, 41), (0, 64), (1, 70), (8, 76), (7, 77)]       # 7, 7, 8, 8, 9, 16, 16, 17, 17
    return [(a, b) for a, b in out if b <= d]


def whole_chunks_of(start, end):
    return max(0, (end >> 2) - ((start + 3) >> 2))
