"""The three nomination forms of the candidate-list path (csrc/fir_capi.hip: topk_lists_dev) emulated in float32 on the CPU, in
the kernels' own order of operations (csrc/fir_kernels.h: TileAcc::chunk / group / masked, k_nominate's epilogue; fir_common.h:
accum), against the float64 reference of nomination_scan_ref.py: |form - reference| <= B for every (query, row) of every input
kind and feature range. This pins the DERIVATION of the three bounds -- tests/test_gpu_nomination_scans.py holds the kernels to
the same bounds.

What the emulation keeps of the kernels:
  kChi2Harm   the query tile holds min(1 / l, 2^60) (IEEE division); whole chunks inside a load group of 8 take two features per
              reciprocal -- A = 1/l_j + min(rcp(r_j), 2^60), B the same for j + 1, acc = fma(A + B, rcp(A B), acc) --, every other
              feature (ragged edges, the whole chunks past the last full group) the one-term form acc + rcp(1/l + rcp(r));
              value = ((sq + sg) - 4 acc) / nf with float32 sums sq (64 lanes + butterfly) and sg (in feature order)
  kKLEnt      the query tile holds l + 2^-100; a load group's 32 terms fma(s, log2 s, part) are added up on their own and join
              the running sum once, the other features go straight into it; value = (0.693147181f ((sq + sg) - acc)) / nf with
              sq, sg added up in double and rounded once
  kChi2Approx acc + (l - r)^2 * rcp(max(l + r, 2^-60)), feature by feature; value = acc / nf
Every v_rcp_f32 / v_log_f32 result is the correctly rounded one moved by -1, 0 or +1 ulp: all down, none, all up, and at random."""
import numpy as np
import pytest

import nomination_scan_ref as ref

F = np.float32
U = 8                                      # chunks per load group (kU)
CLAMP = F(2.0 ** 60)
N_ROWS, QB = 160, 8


class Hw:
    """v_rcp_f32 / v_log_f32 to 1 ulp: mode -1 / 0 / +1 moves every result that way, "rand" each one at random"""

    def __init__(self, mode):
        self.mode = mode
        self.rng = np.random.default_rng(77)

    def _move(self, y):
        if self.mode == 0:
            return y
        p = self.rng.integers(-1, 2, y.shape) if self.mode == "rand" else np.full(y.shape, self.mode)
        moved = np.where(p > 0, np.nextafter(y, F(np.inf)), np.where(p < 0, np.nextafter(y, F(-np.inf)), y))
        return np.where(np.isfinite(y) & (y != 0), moved, y).astype(F)

    def rcp(self, x):
        with np.errstate(divide="ignore", over="ignore"):
            return self._move((1.0 / x.astype(np.float64)).astype(F))

    def log2(self, x):
        with np.errstate(divide="ignore"):
            return self._move(np.log2(x.astype(np.float64)).astype(F))


def fma(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def plan(start, end):
    """the kernels' walk over [start, end): ("one", features) for the masked chunks, ("group", chunks) for a full load group"""
    c_lo, c_hi = (start + 3) >> 2, end >> 2
    if c_lo > c_hi:
        return [("one", list(range(start, end)))]
    steps = []
    if start & 3:
        steps.append(("one", list(range(start, 4 * c_lo))))
    ng = (c_hi - c_lo) // U
    for gi in range(ng):
        steps.append(("group", list(range(c_lo + gi * U, c_lo + (gi + 1) * U))))
    c_end = c_lo + ng * U
    if c_end < c_hi:
        steps.append(("one", list(range(4 * c_end, 4 * c_hi))))
    if end & 3:
        steps.append(("one", list(range(4 * c_hi, end))))
    return steps


def lane_sum_f32(x, start, end):
    """k_query_sums_widen: lane i adds features start + i, start + i + 64, ...; then the xor butterfly"""
    lanes = np.zeros((x.shape[0], 64), F)
    for k in range(start, end):
        lanes[:, (k - start) % 64] += x[:, k]
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ off]
    return lanes[:, 0]


def seq_sum_f32(x, start, end):
    s = np.zeros(x.shape[0], F)
    for k in range(start, end):
        s = s + x[:, k]
    return s


def emulate(form, q, rows, start, end, hw):
    q, rows = np.asarray(q, F), np.asarray(rows, F)
    nf = F(end - start)
    acc = np.zeros((q.shape[0], rows.shape[0]), F)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if form == ref.FORM_HARM:
            qt = np.minimum(F(1) / q, CLAMP)
        elif form == ref.FORM_ENT:
            qt = q + F(2.0 ** -100)
        else:
            qt = q
        L = lambda k: qt[:, k][:, None]
        R = lambda k: rows[:, k][None, :]

        def one(acc, k):
            if form == ref.FORM_HARM:
                return acc + hw.rcp(L(k) + hw.rcp(R(k)))
            if form == ref.FORM_ENT:
                s = L(k) + R(k)
                return fma(s, hw.log2(s), acc)
            df = L(k) - R(k)
            s = np.maximum(L(k) + R(k), F(2.0 ** -60))
            return acc + (df * df) * hw.rcp(s)

        for what, items in plan(start, end):
            if what == "one":
                for k in items:
                    acc = one(acc, k)
            elif form == ref.FORM_HARM:
                for c in items:
                    v = [np.minimum(hw.rcp(R(4 * c + j)), CLAMP) for j in range(4)]
                    for j in (0, 2):
                        A, B = L(4 * c + j) + v[j], L(4 * c + j + 1) + v[j + 1]
                        acc = fma(A + B, hw.rcp(A * B), acc)
            elif form == ref.FORM_ENT:
                part = np.zeros_like(acc)
                for c in items:
                    for j in range(4):
                        part = one(part, 4 * c + j)
                acc = acc + part
            else:
                for c in items:
                    for j in range(4):
                        acc = one(acc, 4 * c + j)
        if form == ref.FORM_HARM:
            sq, sg = lane_sum_f32(q, start, end), seq_sum_f32(rows, start, end)
            return ((sq[:, None] + sg[None, :]) - F(4) * acc) / nf
        if form == ref.FORM_ENT:
            sq, sg = ref.range_entropies(q, start, end).astype(F), ref.range_entropies(rows, start, end).astype(F)
            return (F(0.693147181) * ((sq[:, None] + sg[None, :]) - acc)) / nf
        return acc / nf


def test_the_plan_walks_every_feature_once_in_order():
    for d in (96, 100):
        for a, b in ref.ranges(d):
            feats = []
            for what, items in plan(a, b):
                feats += items if what == "one" else [4 * c + j for c in items for j in range(4)]
            assert feats == list(range(a, b)), (a, b)
    assert [ref.whole_chunks_of(a, b) for a, b in ref.ranges(96)[6:]] == [7, 7, 8, 8, 9, 16, 16, 17, 17]
    assert sum(1 for w, _ in plan(8, 76) if w == "group") == 2 and plan(8, 76)[-1] == ("one", [72, 73, 74, 75])


def test_the_generator_makes_what_it_promises():
    for kind in ref.KINDS:
        rows, q = ref.make_case(kind, N_ROWS, 96, QB)
        r2, q2 = ref.make_case(kind, N_ROWS, 96, QB)
        assert np.array_equal(rows, r2) and np.array_equal(q, q2)
        assert ref.in_plain_range(rows) and ref.in_plain_range(q)
    rows, q = ref.make_case("both_zero", N_ROWS, 96, QB)
    assert np.any((rows[None, :, :] == 0) & (q[:, None, :] == 0))
    rows, q = ref.make_case("pair_zero", N_ROWS, 96, QB)
    assert not rows[:, 34:36].any() and not q[:, 34:36].any() and not rows[:, 4:6].any() and q[:, 4:6].any()
    rows, q = ref.make_case("range_ends", N_ROWS, 96, QB)
    both = (rows == ref.PLAIN_LO).any(axis=1) & (rows == ref.PLAIN_HI).any(axis=1)
    assert both.all()
    rows, q = ref.make_case("dominant_row", N_ROWS, 96, QB)
    assert rows.sum(axis=1).max() == 2.0 ** 16 * 96 and np.median(rows.sum(axis=1)) < 1.001


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("form", [ref.FORM_HARM, ref.FORM_APPROX, ref.FORM_ENT])
def test_form_stays_within_its_bound(form, kind):
    metric = ref.KL if form == ref.FORM_ENT else ref.CHI2
    worst = worst_floor = 0.0
    for d in (96, 100):
        rows, q = ref.make_case(kind, N_ROWS, d, QB)
        for a, b in ref.ranges(d):
            want = ref.distances(metric, q, rows, a, b)
            B = ref.bound(form, q, rows, a, b)
            lim = ref.allowed(form, B, want)
            floor_only = ((B <= ref.ENT_FLOOR) & (form == ref.FORM_ENT))[:, None] & np.ones_like(want, bool)     # the query and every row 0 over the range
            for mode in (0, -1, 1, "rand"):
                got = emulate(form, q, rows, a, b, Hw(mode)).astype(np.float64)
                assert np.all(np.isfinite(got)), (kind, d, a, b, mode)
                dev = np.abs(got - want)
                ratio = np.where(lim > 0, dev / np.where(lim > 0, lim, 1.0), np.where(dev > 0, np.inf, 0.0))
                worst = max(worst, float(ratio[~floor_only].max(initial=0.0)))
                worst_floor = max(worst_floor, float(ratio[floor_only].max(initial=0.0)))
                assert ratio.max() <= 1.0, (kind, d, a, b, mode, float(ratio.max()))
    print(f"nomination_form_ratio form={form} kind={kind} largest |form - float64| / B = {worst:.4f}"
          + (f" (all-zero ranges, B = 2^-93: {worst_floor:.4f})" if worst_floor else ""))
