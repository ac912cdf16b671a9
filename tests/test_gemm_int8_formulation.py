"""The int8 nomination's error bound (fir_gemm_i8.h), without a GPU: the quantisation is done here exactly as the kernels do it --
column means, f32 centring, one scale for the gallery and one per query, rint and clamp, exact integer sums, one f32 fma -- and

    |(qnorm_c + p) - d D| <= eabs_q + e_rel (qnorm_c + G^2)

is tested against the reference's own f32 distance D (sequential, un-fused sum, one division) for d = 64 .. 1 024 on the suite's
synthetic rows, signed rows, rows with an outlier coordinate, a constant gallery and zero queries. One fixture is built to be
tight: it reaches the quantisation term eabs_q to within a few per cent, so a bound shrunk by a small factor fails here."""
import numpy as np
import pytest

import synth

F32 = np.float32
U = 2.0 ** -24


def up_f32(v):
    """f64_up_to_f32_: the smallest f32 >= v, then one more part in 10^6"""
    f = np.asarray(v, np.float64).astype(F32)
    f = np.where(f.astype(np.float64) < v, np.nextafter(f, F32(np.inf)), f).astype(F32)
    return (f + f * F32(1e-6)).astype(F32)


def quant(c, s):
    v = np.rint((np.asarray(s, F32) * c).astype(F32))
    return np.clip(np.where(np.isnan(v), 0, v), -127, 127).astype(np.int64)


class I8Form:
    def __init__(self, rows):
        rows = np.ascontiguousarray(rows, F32)
        self.n, self.d = rows.shape
        self.rows64 = rows.astype(np.float64)
        self.mu = (rows.astype(np.float64).sum(axis=0) / self.n).astype(F32)              # k_i8_colsum / k_i8_mean
        self.cg = (rows - self.mu).astype(F32)
        mx = np.abs(self.cg).max()
        self.s_g = F32(127.0) / mx if mx > 0 else F32(1.0)                               # k_i8_scale
        if not (self.s_g > F32(1e-30) and self.s_g < F32(1e30)):
            self.s_g = F32(np.nan)                                                        # ... every query is left to the exact scan
        self.g8 = quant(self.cg, self.s_g)
        self.gnorm = (self.cg * self.cg).sum(axis=1, dtype=F32)                           # k_i8_rows<0>
        self.G2 = F32(self.gnorm.max())
        res = self.g8.astype(np.float64) / np.float64(self.s_g) - self.cg.astype(np.float64)
        self.R = F32(up_f32(np.sqrt((res * res).sum(axis=1))).max())                      # k_i8_rows<1>
        self.e_rel = F32(F32(F32(8.0) * F32(self.d)) * F32(5.9604645e-8))

    def eabs_of(self, qn, G2, e_q):
        """eabs_q as k_gemm_qprep_i8 evaluates it in f32, from |c_q|^2, G^2 and the measured e_q"""
        G = (np.sqrt(F32(G2)) * F32(1.0 + 2e-7)).astype(F32)
        return (F32(2.0) * ((np.sqrt(np.asarray(qn, F32)) * F32(1.0 + 2e-7)).astype(F32) * self.R + e_q * (G + self.R)) * F32(1.0 + 1e-4)).astype(F32)

    def prepare(self, q):
        """k_gemm_qprep_i8 / k_gemm_pack_queries_i8: (c_q, q8, qnorm_c, e_q, qinv) of every query; sets self.unanswered"""
        cq = (np.asarray(q, F32) - self.mu).astype(F32)
        m = np.abs(cq).max(axis=1)
        s_q = np.where(m > 0, F32(127.0) / np.where(m > 0, m, 1).astype(F32), F32(1.0)).astype(F32)
        q8 = quant(cq, s_q[:, None])
        qn = (cq * cq).sum(axis=1, dtype=F32)
        res = q8.astype(np.float64) / s_q.astype(np.float64)[:, None] - cq.astype(np.float64)
        e_q = up_f32(np.sqrt((res * res).sum(axis=1)))
        with np.errstate(over="ignore", under="ignore", divide="ignore"):
            s_qg = (s_q * self.s_g).astype(F32)
            qinv = (F32(1.0) / s_qg).astype(F32)
        # k_gemm_qprep_i8's guard: outside it the query gets a NaN window and the exact scan answers -- nothing is claimed
        self.unanswered = ~((s_q > F32(1e-30)) & (s_q < F32(1e30)) & (s_qg > F32(1e-30)) & (s_qg < F32(1e30)))
        return cq, q8, qn, e_q, qinv

    def proxies(self, q):
        """For the nomination tests (tests/test_gpu_gemm_int8_nominations.py), per (query, row) in float64:
        p_emu   gnorm_c - 2 qinv S with the exact integer sum S and |c_g|^2 in float64 of the f32 centred row;
        B       what the device adds on top: its f32 row norm (d - 1 additions and a rounding per square: d u |c_g|^2 to first order)
                and the one rounding of the fma (u |p| <= u (|c_g|^2 + 2 qinv |S|)) -- u ((d + 2) |c_g|^2 + 4 qinv |S|) with room for
                the second order; nothing else differs: the sums are integers, the scales are the same f32 operations;
        dist2   |q - g|^2 of the rows and queries as they are (what qnorm_c + p stands for);
        and per query |c_q|^2 (float64 of the f32 centred query) and e_q."""
        cq, q8, _, e_q, qinv = self.prepare(q)
        S = q8.astype(np.float64) @ self.g8.astype(np.float64).T                          # exact: |S| < 2^24
        qi = qinv.astype(np.float64)[:, None]
        gn = (self.cg.astype(np.float64) ** 2).sum(axis=1)[None, :]
        p_emu = gn - 2.0 * qi * S
        B = U * ((self.d + 2) * gn + 4.0 * qi * np.abs(S))
        q64, g64 = np.asarray(q, F32).astype(np.float64), self.rows64
        dist2 = (q64 * q64).sum(axis=1)[:, None] + (g64 * g64).sum(axis=1)[None, :] - 2.0 * (q64 @ g64.T)
        return p_emu, B, dist2, (cq.astype(np.float64) ** 2).sum(axis=1), e_q

    def emulate(self, q):
        """(qnorm_c + p, eabs, bound) per (query, row) / per query, as k_gemm_qprep_i8 and the pass form them"""
        cq, q8, qn, e_q, qinv = self.prepare(q)
        eabs = self.eabs_of(qn, self.G2, e_q)
        S = q8 @ self.g8.T                                                                # exact
        assert np.abs(S).max() < 2 ** 24
        p = (self.gnorm.astype(np.float64)[None, :] - 2.0 * qinv.astype(np.float64)[:, None] * S).astype(F32)      # one rounding: the fma
        lhs = qn.astype(np.float64)[:, None] + p.astype(np.float64)
        bound = eabs.astype(np.float64) + np.float64(self.e_rel) * (qn.astype(np.float64) + np.float64(self.G2))
        bound = np.where(self.unanswered, np.inf, bound)
        return lhs, eabs.astype(np.float64), bound


def reference_dD(rows, q):
    """d times the reference's distance: db_features.cpp's sequential, un-fused f32 sum of (q - g)^2 and its one division"""
    d = rows.shape[1]
    out = np.empty((q.shape[0], rows.shape[0]))
    for i in range(q.shape[0]):
        t = (q[i][None, :] - rows).astype(F32)
        s = np.cumsum((t * t).astype(F32), axis=1, dtype=F32)[:, -1]                      # (cumsum adds in order)
        out[i] = (s / F32(d)).astype(F32).astype(np.float64) * d
    return out


def worst_ratio(rows, q):
    f = I8Form(rows)
    lhs, _, bound = f.emulate(q)
    with np.errstate(invalid="ignore"):
        err = np.abs(lhs - reference_dD(np.asarray(rows, F32), np.asarray(q, F32)))
    err = np.where(f.unanswered[:, None], 0.0, err)                                       # (no claim for a query the guard turns away)
    return float((err / np.maximum(bound[:, None], 1e-300)).max()), f


def cases(d):
    n, c = 1500, 12
    rows = synth.make_gallery(31 + d, n, d, 0)
    q, _ = synth.make_queries(31 + d, rows, c, 0)
    signed = synth.normalise(synth.uniform01(n * d, 77 + d).reshape(n, d) - F32(0.5), 0)
    qs = synth.normalise(synth.uniform01(c * d, 78 + d).reshape(c, d) - F32(0.5), 0)
    outl = rows.copy()
    outl[::97, 3] = F32(5.0)                                                              # inflates max|c_g| and with it R
    zero_q = np.zeros((2, d), F32)
    return {"synthetic": (rows, q), "signed": (signed, qs), "outlier": (outl, q), "constant": (np.full((64, d), F32(0.25)), q),
            "zero queries": (rows, zero_q), "queries far away": (rows, q * F32(40.0))}


@pytest.mark.parametrize("d", [64, 200, 512, 1024])
def test_the_bound_holds(d):
    for name, (rows, q) in cases(d).items():
        r, f = worst_ratio(rows, q)
        assert r <= 1.0, (name, d, r)
        if name == "constant":
            assert f.R == 0 and not f.g8.any()


@pytest.mark.parametrize("scale", [1e-6, 1e-11, 1e-13, 1e-16, 1e-17, 1e-18, 3e-19])
@pytest.mark.parametrize("which", ["both", "rows", "queries"])
def test_small_magnitudes_hold_the_bound_or_are_turned_away(scale, which):
    """Rows and / or queries of small magnitude: s_q and s_g inside their own guards multiply to inf from about 1e-17 each (qinv = 0:
    every proxy is gnorm_c, off by two orders of magnitude of the bound) and to a subnormal qinv before that. The guard on fl(s_q s_g)
    turns such queries away; whatever it lets through holds the bound. The synthetic rows' centred coordinates reach about 0.1, so
    s ~ 1.3e3 / scale: both at 1e-13 or below are outside (1e-30, 1e30), both at 1e-11 or above inside."""
    d = 512
    rows = synth.make_gallery(31 + d, 1500, d, 0)
    q, _ = synth.make_queries(31 + d, rows, 12, 0)
    if which in ("both", "rows"):
        rows = (rows * F32(scale)).astype(F32)
    if which in ("both", "queries"):
        q = (q * F32(scale)).astype(F32)
    r, f = worst_ratio(rows, q)
    assert r <= 1.0, (scale, which, r)
    if which == "both":
        assert f.unanswered.all() == (scale <= 1e-13) and f.unanswered.any() == (scale <= 1e-13), (scale, f.unanswered)
    else:
        # one side small: the other's scale is ~1e3, so the product stays inside the guard (4e24 at 3e-19)
        assert not f.unanswered.any(), (scale, which)


def tight_fixture(d):
    """Column means exactly zero (rows come in +- pairs), the grid step a power of two, one row at the top of the scale; the query's
    centred coordinates are +-c (so q8 = +-127, e_q = 0) and row 0 sits 0.49 of a step off the grid, everywhere with the sign of the
    query's coordinate: every coordinate's quantisation error pulls the sum the same way."""
    rng = np.random.default_rng(5 + d)
    step = 2.0 ** -10
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0)
    mk = rng.integers(-100, 101, d).astype(np.float64)
    row = (step * (mk + 0.49 * sign)).astype(F32)
    top = np.zeros(d, F32)
    top[0] = F32(127 * step)
    rows = np.stack([row, -row, top, -top]).astype(F32)
    q = (F32(0.03125) * sign).astype(F32)[None, :]
    return rows, q


@pytest.mark.parametrize("d", [64, 512, 1024])
def test_the_tight_fixture_reaches_the_quantisation_term(d):
    rows, q = tight_fixture(d)
    f = I8Form(rows)
    assert not f.mu.any() and f.s_g == F32(1024.0)
    lhs, eabs, bound = f.emulate(q)
    err = np.abs(lhs - reference_dD(rows, q))
    assert (err <= bound[:, None]).all()
    assert err[0, 0] >= 0.9 * eabs[0], (err[0, 0], eabs[0])          # a bound shrunk by more than a tenth is caught


def near_tie_fixture(d=512, seed=9):
    """The tight row A (row 0) next to a row B (row 2) that lies ON the grid -- its proxy is exact -- and is farther from the query by a
    quarter of eabs_q: A's proxy is too high by nearly eabs_q, so B's is the smaller one. With the bound as derived A lies inside the
    re-rank's window and wins; with the bound shrunk to a quarter A falls out of it and the certificate 'proves' B. 58 far rows on the
    grid fill two row blocks; rows come in +- pairs (column means exactly zero). 64 queries: query 0 is the crafted one, the others are
    gallery rows."""
    rng = np.random.default_rng(seed)
    step, c = 2.0 ** -10, 32.0
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0)
    mk = rng.integers(-60, 61, d).astype(np.float64)
    x = mk - c * sign
    target = 0.25 * 2 * 0.49 * c * d                                                      # a quarter of eabs_q, in step^2
    b, run = np.zeros(d), 0.0
    for k in range(d):                                                                    # B = A moved onto the grid, coordinate by coordinate
        terms = [(x[k] + sign[k] * bk) ** 2 - (x[k] + 0.49 * sign[k]) ** 2 for bk in (0.0, 1.0)]
        pick = int(abs(run + terms[1] - target * (k + 1) / d) < abs(run + terms[0] - target * (k + 1) / d))
        b[k] = pick
        run += terms[pick]
    a_row, b_row = step * (mk + 0.49 * sign), step * (mk + b * sign)
    top = -127 * step * sign                                                              # (fixes the scale; far from the query)
    far = step * rng.integers(-127, 128, (29, d)).astype(np.float64)
    rows = np.concatenate([np.stack([a_row, -a_row, b_row, -b_row, top, -top]), np.stack([far, -far], axis=1).reshape(58, d)]).astype(F32)
    q = np.concatenate([(F32(c * step) * sign)[None, :], rows[6:6 + 63]]).astype(F32)[:64]
    return rows, q


def test_the_near_tie_fixture_separates_a_sound_bound_from_a_shrunken_one():
    """(what tests/test_gpu_gemm_int8.py runs on the device, decided here with the emulation: the re-rank's window 2 E d hung on the
    smallest proxy, and the certificate of the rows left outside)"""
    rows, q = near_tie_fixture()
    f = I8Form(rows)
    assert not f.mu.any() and f.s_g == F32(1024.0)
    lhs, eabs, bound = f.emulate(q[:1])
    dD = reference_dD(rows, q[:1])
    assert int(np.argmin(dD[0])) == 0 and int(np.argmin(lhs[0])) == 2                  # A is the nearest row, B has the smallest proxy
    gap = lhs[0, 0] - lhs[0, 2]
    assert gap <= 2 * bound[0]                                                            # sound: A is re-ranked
    assert gap > 2 * 0.25 * bound[0] and lhs[0, 0] - 0.25 * bound[0] > dD[0, 2]           # a quarter: A is left out and B is "proved"
    assert np.sort(lhs[0])[2] - 0.25 * bound[0] > dD[0, 2]                                # ... against every other row too


def descending_fixture(n=32 * 626 + 5, d=512, qb=256, seed=77):
    """Rows whose distance from every query FALLS with the row index, for the second-chance rounds of the int8 pass
    (tests/test_gpu_gemm_int8_nominations.py): rows = c + r_i u_i with |u_i| = 1 and r_i^2 falling evenly from 0.36 to 0.21, queries
    = c + 0.1 v, the u_i zero in the sixteen coordinates the v live in -- |q - g_i|^2 = r_i^2 + 0.01 for every query, no noise but
    the quantisation's. A workgroup that keeps its own bound (the audit build's FIR_GEMM_ADAPT_DBG=3) then appends every row of its
    range, whatever the range, as long as it is shorter than 512 rows (256 queries: two pairs share a launch, 128 ranges of ~157
    rows) -- every list overflows; and the second-chance round's bound -- the smallest STORED proxy + one window, where every
    workgroup stores some of its rows, the last range's among them -- has fewer than a list's rows below it, so that round certifies. Both premises are checked below with the emulation."""
    rng = np.random.default_rng(seed)
    c = rng.random(d)
    c /= np.linalg.norm(c)
    u = rng.standard_normal((n, d))
    u[:, :16] = 0
    u /= np.linalg.norm(u, axis=1)[:, None]
    r2 = np.linspace(0.36, 0.21, n)
    rows = (c[None, :] + np.sqrt(r2)[:, None] * u).astype(F32)
    v = rng.standard_normal((qb, d))
    v[:, 16:] = 0
    v /= np.linalg.norm(v, axis=1)[:, None]
    q = (c[None, :] + 0.1 * v).astype(F32)
    return rows, q


def test_the_descending_fixture_overflows_every_list_and_its_second_bound_holds_few_rows():
    rows, q = descending_fixture()
    f = I8Form(rows)
    p, B, dist2, qn64, e_q = f.proxies(q)
    assert not f.unanswered.any()
    assert (np.argmin(dist2, axis=1) == f.n - 1).all()
    qn = qn64.astype(F32)
    w = (F32(2.5) * (f.e_rel * (qn + f.G2) + f.eabs_of(qn, f.G2, e_q))).astype(np.float64)
    # a row is appended when its proxy is below (the smallest proxy its workgroup has seen) + w: here below the smallest of the 512 rows
    # on either side + w, for EVERY row
    pad = np.pad(p, ((0, 0), (512, 512)), constant_values=np.inf)
    local_min = np.lib.stride_tricks.sliding_window_view(pad, 1025, axis=1).min(axis=2)
    assert (p < local_min + w[:, None] - B).all()
    # the second-chance round appends below min(first bound, smallest stored proxy + w): with a stored proxy among the last 512 rows'
    # that is at most this
    below = (p < (p[:, -512:].max(axis=1) + w * (1 + 1e-5))[:, None] + B).sum(axis=1)
    assert below.max() <= 3072 and below.min() >= 64, (below.min(), below.max())
