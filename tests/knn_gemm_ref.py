"""numpy restatement of the matrix-core form of the K nearest rows for 8 < K <= 256 (fir_gemm_search_knn_keys_dev, csrc/fir_gemm_knn.h),
written from the code and not from a kernel's output: plain numpy, no GPU.

  sample_plan    knn_sample_plan (csrc/fir_knn_select.h): R = min(n, max(32768, n K / div)) rows in whole 64-row tiles, taken as up to
                 16 runs of run_len = ceil(tiles / 16) consecutive tiles (the last one what is left), run i moved up by
                 floor(i slack / runs) tiles: spread evenly over the gallery
  sample_bound   D_s[q] = the exact K-th smallest reference distance (float32: the reference's sequential sum and one division) over
                 the sample rows with dist < 100000; 100000 with fewer than K of them
  tau_of         k_gemm_tau_class: (D_s d - |q|^2) + 2.5 e_rel (|q|^2 + max |g|^2), nudged up -- +inf for D_s = 100000
  expected       the contract, knn_select_ref.expected_keys

D_s is an order statistic of a subset of the rows, so D_s >= D_K, the gallery's K-th distance, whatever the sample is. A row whose
reference distance is <= D_s has a true |g|^2 - 2 q.g within E d of D_s d - |q|^2 and a proxy within E d of that: it lies below tau
and is appended. tests/test_knn_gemm_formulation.py checks that, the list capacity and the certificate on the float64 emulation of
the fp16 proxies (gemm_f16_form.py) over the shapes tests/test_gpu_knn_gemm.py runs on the device.
"""
import functools

import numpy as np

import gemm_f16_form as gf
import knn_select_ref
import synth

F32 = np.float32
NOT_FOUND = F32(100000.0)
GEMM_KNN_MAX = 256          # FIR_GEMM_KNN_MAX
SAMPLE_RUNS = 16            # kKnnSampleRuns
SAMPLE_FLOOR = 32768        # kKnnSampleFloor
SAMPLE_DIV = 1024           # kKnnSampleDiv
SAMPLE_BYTES = 64 << 20     # kKnnSampleBytes

# (n, d, qb, K): the shapes of the device test; every one must come through without the exact form
SHAPES = [
    (3000, 64, 130, 9),
    (3000, 64, 130, 256),
    (5000, 512, 70, 33),
    (333, 100, 40, 256),
    (4097, 100, 17, 64),        # one row more than a list holds
    (66000, 128, 200, 64),      # crosses 65 536 rows and the sample floor: the bound decides what is appended
]


@functools.lru_cache(maxsize=None)
def case(seed, n, d, qb):
    rows = synth.make_gallery(seed, n, d, 0)
    q, _ = synth.make_queries(seed, rows, qb, 0)
    for a in (rows, q):
        a.setflags(write=False)
    return rows, q


def clustered(spread, ids=150, per=40, d=128, qb=70, seed=17):
    """ids identities x per images, class-major (the reference's getTrainingAndTestImages emits class by class)"""
    rng = np.random.default_rng(seed)
    centres = rng.random((ids, d), dtype=np.float32)
    rows = synth.normalise(np.repeat(centres, per, axis=0) * (1 + spread * (rng.random((ids * per, d), dtype=np.float32) - 0.5)), 0)
    who = rng.integers(0, ids, qb)
    q = synth.normalise(centres[who] * (1 + spread * (rng.random((qb, d), dtype=np.float32) - 0.5)), 0)
    return rows, q


def sample_plan(n, k, div=SAMPLE_DIV, budget=SAMPLE_BYTES):
    """dict(tiles, rows, runs=[(begin tile, tiles)], stride, group) as knn_sample_plan gives them"""
    n, k, div = max(n, 0), max(k, 1), max(div, 1)
    gallery_tiles = (n + 63) // 64
    want = min(n, max(SAMPLE_FLOOR, n * k // div))
    tiles = (want + 63) // 64
    run_len = (tiles + SAMPLE_RUNS - 1) // SAMPLE_RUNS
    nruns = (tiles + run_len - 1) // run_len if run_len else 0
    slack = gallery_tiles - tiles
    runs = [(i * run_len + i * slack // nruns, min(run_len, tiles - i * run_len)) for i in range(nruns)]
    rows = tiles * 64
    if runs and runs[-1][0] + runs[-1][1] == gallery_tiles:
        rows -= gallery_tiles * 64 - n
    per_query = (tiles * 64 if tiles else 64) * 4
    group = min(max(budget // per_query, 1), 8192)
    if group >= 8:
        group = group // 8 * 8
    return {"tiles": tiles, "rows": rows, "runs": runs, "stride": tiles * 64, "group": group}


def sample_rows(n, k, div=SAMPLE_DIV):
    """the gallery rows of the sample, in the order their distances are stored"""
    plan = sample_plan(n, k, div)
    idx = [np.arange(b * 64, min((b + t) * 64, n)) for b, t in plan["runs"]]
    out = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    assert out.shape[0] == plan["rows"]
    return out


def reference_distances(rows, q, d):
    """the reference's float32 distance of one query to rows [m, >= d] over features [0, d): the sequential sum of (q - g)^2, each
    operation rounded once, then one division (db_features.cpp:22-42)"""
    rows = np.asarray(rows, F32)
    acc = np.zeros(rows.shape[0], F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for f in range(d):
            df = F32(q[f]) - rows[:, f]
            acc = acc + df * df
        return acc / F32(d)


def sample_bound(rows, q, k, d=0, div=SAMPLE_DIV):
    """D_s [c] float32. Exact at float32 level without a float32 pass over the whole sample: float64 distances place every row, and
    only the rows within 1e-4 (relative) of the K-th smallest of those -- far more than float32's (d + 3) 2^-24 -- are re-computed in
    the reference's arithmetic."""
    rows = np.asarray(rows, F32)
    q = np.atleast_2d(np.asarray(q, F32))
    d = d if 0 < d < rows.shape[1] else rows.shape[1]
    s = rows[sample_rows(rows.shape[0], k, div)][:, :d]
    out = np.full(q.shape[0], NOT_FOUND, F32)
    if s.shape[0] < k:
        return out
    s64 = s.astype(np.float64)
    sn = (s64 * s64).sum(axis=1)
    for i in range(q.shape[0]):
        q64 = q[i, :d].astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            d64 = (sn - 2.0 * (s64 @ q64) + (q64 * q64).sum()) / d
        if not np.isfinite(d64).all():                               # hostile values: the whole sample in float32
            f = reference_distances(s, q[i], d)
            f = np.sort(f[knn_select_ref.qualifies(f)])
            out[i] = f[k - 1] if f.shape[0] >= k else NOT_FOUND
            continue
        kth = np.partition(d64, k - 1)[k - 1]
        band = np.abs(d64 - kth) <= 1e-4 * abs(kth) + 1e-12
        below = int((~band & (d64 < kth)).sum())
        f = np.sort(reference_distances(s[band], q[i], d))
        v = f[k - 1 - below]
        out[i] = v if v < NOT_FOUND else NOT_FOUND
    return out


def tau_of(e_rel, ds, d, qn, gmax):
    """k_gemm_tau_class in float32: [c]"""
    ds, qn = np.asarray(ds, F32), np.asarray(qn, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = F32(2.5) * F32(e_rel) * (qn + F32(gmax))
        v = (ds * F32(d) - qn) + w
        t = v + np.abs(v) * F32(1e-6) + F32(1e-30)
    return np.where(ds < NOT_FOUND, t, F32(np.inf)).astype(F32)


def formulation(rows, q, k, d=0, div=SAMPLE_DIV, chunk=32):
    """What the form rests on, on the float64 emulation of the fp16 proxies, per query: dict of D_s, tau, count (rows below tau),
    listed_all (every row whose distance is <= D_s, with float32's rounding allowed for, is below tau) and the certificate's margin."""
    form = gf.Form(rows, 2, d)
    q = np.asarray(q, F32)
    ds = sample_bound(rows, q, k, d, div)
    out = {"ds": ds, "tau": [], "count": [], "listed_all": [], "margin": []}
    for c0 in range(0, q.shape[0], chunk):
        p_emu, p_true, _, qn = form.emulate(q[c0:c0 + chunk])
        tau = tau_of(form.e_rel, ds[c0:c0 + chunk], form.d, qn.astype(F32), form.gmax)
        cert = gf.certificate(form, p_emu, p_true, qn, k=k, tau=tau)
        dist = (qn[:, None] + p_true) / form.d
        near = dist <= ds[c0:c0 + chunk].astype(np.float64)[:, None] * (1.0 + 2.0 * (form.d + 3) * gf.U)
        out["tau"].append(tau)
        out["count"].append(cert["count"])
        out["listed_all"].append((~near | (p_emu < tau.astype(np.float64)[:, None])).all(axis=1))
        out["margin"].append(cert["margin"])
    for key in ("tau", "count", "listed_all", "margin"):
        out[key] = np.concatenate(out[key])
    return out


def expected(dist, k, row_offset=0):
    """the K keys of one query from its reference distances to ALL rows: knn_select_ref.expected_keys"""
    return knn_select_ref.expected_keys(np.asarray(dist, F32), k, row_offset)
