"""A float64 emulation of what the matrix-core nomination passes (fir_gemm.hip, fir_gemm_f16x.h) are MEANT to compute, written
from the code and not from a kernel's output: plain numpy, no GPU. The passes only nominate rows -- k_gemm_rerank* re-computes
the nominees in the reference's arithmetic and a certificate decides whether the answer stands -- and that certificate rests on
two premises about the pass:

  1. every proxy is within E d of its row's true |g|^2 - 2 q.g (comment above rerank_window_, fir_gemm_rerank.h);
  2. whatever was not appended has a proxy >= tau, and every row within one window of the smallest proxy of ALL rows is
     appended (header of fir_gemm_f16x.h, MODE 3).

tests/test_gemm_f16_formulation.py checks here, without a GPU, that the rounding the forms intend satisfies premise 1 on the test
data; tests/test_gpu_gemm_nominations.py compares the device's proxies, lists and bounds with this emulation.

The three forms (fir_gemm::precision)

  FIR_GEMM_F16 (2)   the gallery is multiplied by ONE power of two, 2^gallery_exp, that takes its largest |value| (over whole
                     rows, k_gemm_absmax) into [2^13, 2^14); every query by its own 2^sh (largest |q_k| of the compared features
                     into the same interval, k_gemm_qprep_f16); both are rounded to fp16, round to nearest even; features past
                     the compared range are zero. qinv = 2^(-sh - gallery_exp) turns the sum back into q.g.
  FIR_GEMM_BF16_SPLIT (1)   x = hi + lo + r, hi = bf16(x), lo = bf16(x - hi); the sum is hi.hi + hi.lo + lo.hi.
  FIR_GEMM_F32 (0)   the f32 values themselves.

  p_emu  = |g|^2 - 2 qinv (q~ . g~)     |g|^2 in float64 of the f32 row, the dot product of the ROUNDED operands exact (float64:
                                         a product of two fp16 / bf16 values has at most 22 bits)
  p_true = |g|^2 - 2 q.g                the unrounded f32 values, in float64

What the device adds on top of p_emu: B(q, g). With u = 2^-24 and any summation order,

  * the row norm gn is an f32 sum of d squares: |gn - |g|^2| <= d u |g|^2 to first order (d - 1 additions and one rounding per
    square; k_gemm_row_norms / k_gemm_pack_gallery);
  * the matrix cores add D products into an f32 accumulator, D = the padded feature count of the fragments (x 3 for the three
    bf16 terms). fp16 and bf16 products are exact in f32, f32 products round once. D - 1 additions, each within u of its
    partial sum, every partial sum within sum_k |q~_k g~_k| =: S: |acc - q~.g~| <= (D - 1) u S, + u S for rounded products: D u S;
  * p = fma(-2 qinv, acc, gn) (fp16) or gn - 2 acc (f32, bf16; the doubling is exact) rounds once more: u |p| <= u (|g|^2 + 2 qinv S);
  * qinv is a power of two: scaling by it is exact.

  |p_device - p_emu| <= u (2 qinv D S + 2 qinv S + d |g|^2 + |g|^2) <= u (2 (D + 2) qinv S + (d + 1) |g|^2) =: B

The internal 32-term sum of v_mfma_f32_16x16x32_f16 (and the 16-term one of the bf16 MFMA) is not known to round like an IEEE
chain, so the tests allow kMargin * B with kMargin = 4. That hides nothing: a pass that drops or repeats ONE 32-feature step is
off by about |q.g| / (d / 32) -- two to three orders of magnitude above 4 B at these shapes.

The project's own quantities are formed in float32 exactly as gemm_search, k_gemm_qprep_f16, the pieces of fir_gemm_rerank.h and
k_gemm_adapt_final form them, with erel_scale = 1:

  e_rel = 8 d u + {0, 2^-14, 2^-10 (1 + 2^-4)}          (f32, bf16 split, fp16)
  E d   = e_rel (|q|^2 + max |g|^2)
  w     = 2.5 E d, nudged up by 1e-6 relative and 1e-30  (the window T and tau are hung on)
  tau   = (smallest proxy the pass lowered T with + |q|^2 + w) - |q|^2
"""
import numpy as np

U = 2.0 ** -24
K_LIST_CAP = 4096       # kListCap
K_MARGIN = 4.0          # allowed |p_device - p_emu| / B (see above)
F32 = np.float32


def f32_from_orderable(o):
    """fir::f32_from_orderable on a uint32 array"""
    o = np.asarray(o, np.uint32)
    b = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return b.view(np.float32)


def bf16_round(x):
    """f32 -> the nearest bf16 (ties to even), returned as f32; finite values only"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((b + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _exp_to_2_13(m):
    """sh with m * 2^sh in [2^13, 2^14) (frexp: m = f 2^ex, f in [0.5, 1)); 0 for m == 0"""
    ex = np.frexp(np.asarray(m, np.float32))[1]
    return np.where(np.asarray(m) > 0, 14 - ex, 0).astype(np.int64)


def e_rel_of(precision, d):
    """gemm_search's c.e_rel, in float32 like the host code"""
    term = {0: F32(0.0), 1: F32(6.1035156e-5), 2: F32(9.765625e-4) * F32(1.0625)}[precision]
    return F32(F32(F32(8.0) * F32(d)) * F32(5.9604645e-8)) + term


def f32_share_of(d):
    """the part of e_rel that covers the device's f32 work (both norms, the accumulation, the reference's own roundings)"""
    return F32(F32(F32(8.0) * F32(d)) * F32(5.9604645e-8))


def window_of(e_rel, qn, gmax):
    """nudge_up_(rounding_window_()) of fir_gemm_rerank.h -- k_gemm_qprep_f16 / k_gemm_tau_min / rerank_hand_over_'s second-pass bound: 2.5 E d
    with its nudge (float32)"""
    w = F32(2.5) * F32(e_rel) * (np.asarray(qn, F32) + F32(gmax))
    return (w + np.abs(w) * F32(1e-6) + F32(1e-30)).astype(F32)


def e_d_of(e_rel, qn, gmax):
    """E d = e_rel (|q|^2 + max |g|^2) (float32), the bound of premise 1 in proxy units"""
    return (F32(e_rel) * (np.asarray(qn, F32) + F32(gmax))).astype(F32)


class Form:
    """The rounded gallery of one fir_gemm state: rows [n, d_row] float32, precision 0 / 1 / 2, end = a feature prefix (fp16 only)."""

    def __init__(self, rows, precision=2, end=0):
        rows = np.ascontiguousarray(rows, np.float32)
        self.n, self.d_row = rows.shape
        self.precision = precision
        self.d = end if 0 < end < self.d_row else self.d_row
        g = rows[:, :self.d]
        self.g64 = g.astype(np.float64)
        self.gn = (self.g64 * self.g64).sum(axis=1)                       # |g|^2, float64 of the f32 rows
        self.gmax = F32(self.gn.max()) if self.n else F32(0)              # (the device's own maximum is within d u of it)
        self.e_rel = e_rel_of(precision, self.d)
        if precision == 2:
            self.d_pad = (self.d + 127) // 128 * 128                      # dk16 k-blocks of 16, whole units of kRing = 8
            self.gallery_exp = int(_exp_to_2_13(np.abs(rows).max()))      # over WHOLE rows (k_gemm_absmax), also for a prefix state
            self.terms = 1
            gt = (g * F32(2.0 ** self.gallery_exp)).astype(np.float16).astype(np.float64)
            self.gt = [gt]
        elif precision == 1:
            self.d_pad = (self.d + 127) // 128 * 128                      # dk16 padded to 8 k-blocks
            self.gallery_exp = 0
            self.terms = 3
            hi = bf16_round(g)
            lo = bf16_round(g - hi)
            self.gt = [hi.astype(np.float64), lo.astype(np.float64)]
        else:
            self.d_pad = (self.d + 31) // 32 * 32                         # dq8 groups of 8, padded to 4 groups
            self.gallery_exp = 0
            self.terms = 1
            self.gt = [self.g64]
        self.nonneg = bool((rows[:, :self.d] >= 0).all())

    def emulate(self, q):
        """q [c, d_row] float32 -> (p_emu, p_true, B), each [c, n] float64, and |q|^2 [c] (float64)"""
        qf = np.ascontiguousarray(np.asarray(q, np.float32)[:, :self.d])
        q64 = qf.astype(np.float64)
        qn = (q64 * q64).sum(axis=1)
        if self.precision == 2:
            sh = _exp_to_2_13(np.abs(qf).max(axis=1))
            qt = (qf * np.exp2(sh).astype(np.float32)[:, None]).astype(np.float16).astype(np.float64)
            qinv = np.exp2((-sh - self.gallery_exp).astype(np.float64))[:, None]
            dot = qt @ self.gt[0].T
            absdot = dot if (self.nonneg and (qf >= 0).all()) else np.abs(qt) @ np.abs(self.gt[0]).T
        elif self.precision == 1:
            hi = bf16_round(qf)
            lo = bf16_round(qf - hi)
            hi64, lo64 = hi.astype(np.float64), lo.astype(np.float64)
            qinv = 1.0
            dot = hi64 @ (self.gt[0] + self.gt[1]).T + lo64 @ self.gt[0].T          # hi.hi + hi.lo + lo.hi
            absdot = np.abs(hi64) @ (np.abs(self.gt[0]) + np.abs(self.gt[1])).T + np.abs(lo64) @ np.abs(self.gt[0]).T
        else:
            qinv = 1.0
            dot = q64 @ self.g64.T
            absdot = dot if (self.nonneg and (qf >= 0).all()) else np.abs(q64) @ np.abs(self.g64).T
        true_dot = dot if self.precision == 0 else q64 @ self.g64.T
        p_emu = self.gn[None, :] - 2.0 * qinv * dot
        p_true = self.gn[None, :] - 2.0 * true_dot
        D = self.terms * self.d_pad
        B = U * (2.0 * (D + 2) * qinv * absdot + (self.d + 1) * self.gn[None, :])
        return p_emu, p_true, B, qn

    def slot_of_rows(self):
        """MODE 4: the slot (0..7) a row's proxy lowers -- its position among a lane's eight rows of the block; -1 for the rows of a
        block that is not full (they are appended row by row and lower nothing)"""
        r = np.arange(self.n)
        s = 4 * ((r % 32) // 16) + (r % 4)
        s[r >= (self.n // 32) * 32] = -1
        return s


def certificate(form, p_emu, p_true, qn64, k=1, qn_dev=None, gmax_dev=None, tau=None):
    """The re-rank's certificate (k_gemm_rerank<KMAX>: rerank_window_, rerank_walk_, rerank_certified_<float>) on the emulated proxies, per query of p_emu [c, n]:
    dict of p1 (the K-th smallest proxy), E d, w, tau (the emulated one unless given), margin = (|q|^2 + p_excl) / d - E - (the
    K-th exact distance among the re-ranked rows): the certificate holds where margin > 0, by that much (distance units)."""
    c, n = p_emu.shape
    qn = np.asarray(qn64 if qn_dev is None else qn_dev, F32)
    gmax = form.gmax if gmax_dev is None else F32(gmax_dev)
    ed = e_d_of(form.e_rel, qn, gmax).astype(np.float64)
    w = window_of(form.e_rel, qn, gmax).astype(np.float64)
    kk = min(k, n)
    part = np.partition(p_emu, kk - 1, axis=1)
    pk = part[:, kk - 1] if kk == k else np.full(c, np.inf)
    p_min = part[:, :kk].min(axis=1)
    if tau is None:
        # what the pass lowers T with: the rows of full blocks only; top-K: the K-th smallest of eight slot minima
        full = (n // 32) * 32
        if full == 0:
            tau = np.full(c, np.inf)
        elif k == 1:
            tau = p_emu[:, :full].min(axis=1) + w
        else:
            slots = form.slot_of_rows()
            mins = np.stack([p_emu[:, slots == s].min(axis=1) if (slots == s).any() else np.full(c, np.inf) for s in range(8)], axis=1)
            tau = np.sort(mins, axis=1)[:, k - 1] + w
    tau = np.asarray(tau, np.float64)
    win = pk + 2.0 * ed
    win = win + np.abs(win) * 1e-6
    listed = p_emu < tau[:, None]
    rer = listed & (p_emu <= win[:, None])
    dist = (qn64[:, None] + p_true) / form.d
    dr = np.where(rer, dist, np.inf)
    bd = np.partition(dr, kk - 1, axis=1)[:, kk - 1] if kk == k else np.full(c, 100000.0)
    bd = np.where(np.isfinite(bd), bd, 100000.0)
    p_out = np.where(listed & ~rer, p_emu, np.inf).min(axis=1)
    p_excl = np.minimum(p_out, tau)
    margin = (qn.astype(np.float64) + p_excl) / form.d - ed / form.d - bd
    margin = np.where(rer.sum(axis=1) >= n, np.inf, margin)                # every row was re-ranked
    return {"pk": pk, "p_min": p_min, "ed": ed, "w": w, "tau": tau, "win": win, "margin": margin, "count": listed.sum(axis=1)}
