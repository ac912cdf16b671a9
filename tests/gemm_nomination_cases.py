"""The datasets and kernel forms of the nomination tests: tests/test_gemm_f16_formulation.py shows (no GPU) that every dataset here
satisfies the premises with the emulation alone, tests/test_gpu_gemm_nominations.py runs the forms on them.

Shapes: the smallest at which each path of k_gemm_proxy_f16x exists (gemm_streamed_ / gemm_odd_ in fir_gemm.hip: dk16 = the
compared features in k-blocks of 16, padded to whole units of 8; streamed from dk16 > 32; ODD = 2 for one unit, else units & 1):

  d = 100  one unit (ODD = 2)       d = 256  two units      d = 384  three (ODD = 1)      d = 512  four, the whole resident tile
  d = 520  five units, streamed, odd                       d = 641  dk16 = 48: six units, the smallest streamed even shape

n = 32 * 626 + 5 with 2 048 queries: sixteen (eight) pairs share a launch and every wave walks several row blocks (the reasoning is
in test_gpu_gemm_last_unit.py); n = 32 * 70 + 5: a wave walks one block, one block straddles the end; n = 20: not one full block."""
import functools

import numpy as np

import synth

N_MULTI, QB_MULTI = 32 * 626 + 5, 2048
N_SMALL = 32 * 70 + 5
N_TINY = 20


@functools.lru_cache(maxsize=2)
def random_data(n, d, qb):
    """synth's gallery and queries (half fresh draws, half perturbed rows); the LAST row is a copy of row 11 and query 5 is that
    row (an exact tie between the first row block and the last), query 6 is the row before the last. All values >= 0."""
    seed = 7000 + d + n % 1000
    rows = synth.make_gallery(seed, n, d, 0)
    q, _ = synth.make_queries(seed, rows, qb, 0)
    if n > 12:
        rows[n - 1] = rows[11]
        if qb > 6:
            q[5] = rows[11]
            q[6] = rows[n - 2]
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q


@functools.lru_cache(maxsize=1)
def near_duplicate_data():
    """test_class_ordered_near_duplicates_append_often's gallery: 500 identities x 40 near-duplicate rows, class-ordered -- dozens
    of rows inside one window of the nearest, so the lists are long and the staged appends overflow into the global lists"""
    rng = np.random.default_rng(47)
    ident, per, d, qb = 500, 40, 512, 2048
    centres = rng.random((ident, d), dtype=np.float32)
    rows = np.repeat(centres, per, axis=0) * (1 + 1e-4 * (rng.random((ident * per, d), dtype=np.float32) - 0.5))
    rows = synth.normalise(rows.astype(np.float32), 0)
    who = rng.integers(0, ident, qb)
    q = synth.normalise((centres[who] * (1 + 1e-4 * (rng.random((qb, d), dtype=np.float32) - 0.5))).astype(np.float32), 0)
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q


@functools.lru_cache(maxsize=1)
def second_pass_data():
    """The one deliberately hostile dataset: 20 037 unit rows of 128 features around one centre c. The rows of the even row
    blocks -- the ones the sample flow's strided sample sees -- are far from c, those of the odd blocks lie at every distance
    from it: 10 000 rows nearer than anything sampled, so the first bound lets all of them pass and every list overflows;
    min(first bound, smallest stored proxy + one window) then gives the second-chance round <1, *> a bound a few rows lie below."""
    rng = np.random.default_rng(2024)
    n, d, qb = N_MULTI, 128, 200
    c = rng.random(d).astype(np.float32)
    far = rng.random((n, d)).astype(np.float32)
    t = rng.random((n, 1)).astype(np.float32) * 0.8 + 0.1
    near = c[None, :] * (1 - t) + far * t
    odd = ((np.arange(n) // 32) % 2 == 1)[:, None]
    rows = synth.normalise(np.where(odd, near, far).astype(np.float32), 0)
    q = synth.normalise((c[None, :] * (1 + 0.02 * (rng.random((qb, d)).astype(np.float32) - 0.5))).astype(np.float32), 0)
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q


def data_of(case):
    if case["data"] == "near-duplicates":
        return near_duplicate_data()
    return random_data(case["n"], case["d"], case["qb"])


def _case(name, kernel, n, d, qb, k=1, precision=2, end=0, entry="top", env=None, data="random"):
    return dict(name=name, kernel=kernel, n=n, d=d, qb=qb, k=k, precision=precision, end=end, entry=entry, env=env or {}, data=data)


SAMPLE_FLOW = {"FIR_GEMM_ADAPTIVE": "0"}      # the sample pass <2, *> + append below its bound <1, *> (a knob of the shipped library)

# (d, streamed, odd) of the six unit sequences
SHAPES = [(100, 0, 2), (256, 0, 0), (384, 0, 1), (512, 0, 0), (520, 1, 1), (641, 1, 0)]

CASES = []
for _d, _s, _o in SHAPES:
    CASES.append(_case(f"top1-d{_d}", f"k_gemm_proxy_f16x<3, {_s}, {_o}>", N_MULTI, _d, QB_MULTI))
for _d, _s, _o in SHAPES:
    CASES.append(_case(f"top5-d{_d}", f"k_gemm_proxy_f16x<4, {_s}, {_o}>", N_MULTI, _d, QB_MULTI, k=5))
for _d, _s, _o in SHAPES:
    CASES.append(_case(f"sampled-d{_d}", f"k_gemm_proxy_f16x<1, {_s}, {_o}>", N_MULTI, _d, QB_MULTI, env=SAMPLE_FLOW))
CASES.append(_case("sampled-top5-d512", "k_gemm_proxy_f16x<1, 0, 0>", N_MULTI, 512, QB_MULTI, k=5, env=SAMPLE_FLOW))
CASES.append(_case("near-duplicates", "k_gemm_proxy_f16x<3, 0, 0>", 20000, 512, 2048, data="near-duplicates"))
# few row blocks (a wave walks one block, one straddles) and fewer rows than a block (clamped norm loads)
for _n in (N_SMALL, N_TINY):
    for _d, _s, _o in ((100, 0, 2), (512, 0, 0), (520, 1, 1), (641, 1, 0)):
        CASES.append(_case(f"top1-n{_n}-d{_d}", f"k_gemm_proxy_f16x<3, {_s}, {_o}>", _n, _d, 128))
    CASES.append(_case(f"top5-n{_n}-d512", "k_gemm_proxy_f16x<4, 0, 0>", _n, 512, 128, k=5))
# 16 / 32 queries: one / two live query blocks (whole, even numbers of the form's units only: 512 features resident, 641 streamed)
for _qb, _j in ((16, 1), (32, 2)):
    for _n in (N_MULTI, N_SMALL, N_TINY):
        CASES.append(_case(f"njb{_j}-n{_n}-d512", f"k_gemm_proxy_f16x<3, 0, 0, 0, {_j}>", _n, 512, _qb))
    CASES.append(_case(f"njb{_j}-n{N_SMALL}-d641", f"k_gemm_proxy_f16x<3, 1, 0, 0, {_j}>", N_SMALL, 641, _qb))
# the few-query scan (1, 2, 4 or 8 queries per row read)
for _qb in (1, 2, 3, 8):
    for _n, _d in ((N_SMALL, 512), (N_SMALL, 100), (N_TINY, 520)):
        CASES.append(_case(f"few{_qb}-n{_n}-d{_d}", "k_gemm_scan_f16x", _n, _d, _qb, entry="few"))
# the other two states (sample pass + append pass of k_gemm_proxy / k_gemm_proxy_bf16*; 136 queries = a pair and a single pass)
CASES.append(_case("f32-d200", "k_gemm_proxy<1>", N_MULTI, 200, 136, precision=0))
CASES.append(_case("bf16-d200", "k_gemm_proxy_bf16_wide", N_MULTI, 200, 136, precision=1))
CASES.append(_case("bf16-single-d512", "k_gemm_proxy_bf16<1>", N_SMALL, 512, 64, precision=1))
# a feature prefix state: 64 of 512 features, its own fragments and norms, one unit
CASES.append(_case("prefix64-of-512", "k_gemm_proxy_f16x<3, 0, 2>", N_MULTI, 512, QB_MULTI, end=64))

CASE_IDS = [c["name"] for c in CASES]
