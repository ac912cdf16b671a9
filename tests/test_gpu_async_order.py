"""Back-to-back asynchronous calls on one gallery handle. The device-pointer searches queue everything on the caller's stream and
return (include/fir_amd.h, "Streams"); every handle reuses its device scratch from call to call, so a call that read or wrote
another call's scratch -- or a stale list of uncertified queries that names the previous call's queries -- would only show when
calls of different shapes and different queries are queued without a host synchronisation in between. Each schedule below gives
every call its own queries and its own poisoned key buffer with a tail of canary words, then checks every call against

- the exact streaming scan of a second handle over the same rows, one call at a time (index and distance bits);
- float64 sums of squared differences over every row for a sample of its queries (the rows it returns are the nearest up to the
  reference arithmetic's rounding, their distances are the reference's own arithmetic bit for bit);

and that no call wrote past its buffer or left a slot unwritten."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
POISON = 0xA5A5A5A5A5A5A5A5 - (1 << 64)      # int64 view of the word every key buffer starts out as
POISON32 = 0xA5A5A5A5 - (1 << 32)           # int32 view of the one the range-distance buffers start out as (a negative float)
CANARY = 64                                 # poisoned words after the end of every buffer
KEY_NONE = -1                               # int64 view of FIR_KEY_NONE
DEVICE_KINDS = ("top1", "topk", "gemm_top1", "gemm_few")
U = 2.0 ** -24
LOWER = {250_001: 4_321}                    # _gallery_300k's duplicate pair: a copy of either row comes back as the lower one


def _unit(gen, rows, d):
    x = torch.rand((rows, d), generator=gen, device=DEV)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _ulp_up(x):
    return torch.nextafter(x, torch.tensor(2.0, device=DEV))


class Call:
    """One call of a schedule: its queries, its output buffer, the stream it is queued on (None: the handle's own)."""

    def __init__(self, name, kind, q, n, k=1, start=0, end=None, stream=None, hard=None, expect=None):
        self.name, self.kind, self.q, self.k, self.start = name, kind, q.contiguous(), k, start
        self.end = q.shape[1] if end is None else end
        self.qb = q.shape[0]
        self.stream = stream
        self.hard = hard or {}          # position -> "nan" | "inf" | "zero" | ("copy", row) | ("ulp", row)
        self.expect = expect            # what last_dispatch() must report: a substring of the kernel name, "mfma" or "scan"
        self.dispatch = None
        self.host = None
        if kind == "range":
            self.buf = torch.full((self.qb * n + CANARY,), POISON32, dtype=torch.int32, device=DEV)
        elif kind in DEVICE_KINDS:
            self.buf = torch.full((self.qb * k + CANARY,), POISON, dtype=torch.int64, device=DEV)
        else:
            self.buf = None
            self.q_host = self.q.cpu().numpy()

    def enqueue(self, g, m=None):
        s = self.stream.cuda_stream if self.stream is not None else None
        qp, qb = self.q.data_ptr(), self.qb
        if self.kind == "top1":
            g.search_top1_keys_dev(qp, qb, self.buf.data_ptr(), self.start, self.end, stream=s)
        elif self.kind == "topk":
            g.search_topk_keys_dev(qp, qb, self.k, self.buf.data_ptr(), self.start, self.end, stream=s)
        elif self.kind == "range":
            g.range_distances_dev(qp, qb, self.buf.data_ptr(), self.start, self.end, stream=s)
        elif self.kind == "gemm_top1":
            m.search_top1_keys_dev(qp, qb, self.buf.data_ptr(), stream=s)
        elif self.kind == "gemm_few":
            m.search_few_keys_dev(qp, qb, self.buf.data_ptr(), stream=s)
        elif self.kind == "host_top1":
            self.host = g.search_top1(self.q_host, self.start, self.end)
        elif self.kind == "host_topk":
            self.host = g.search_topk(self.q_host, self.k, self.start, self.end)
        else:
            raise ValueError(self.kind)
        self.dispatch = g.last_dispatch()        # host-side record: does not synchronise

    def reference(self, ref, n):
        """The exact streaming scan of the second handle (matrix cores off), synchronously."""
        qp, qb = self.q.data_ptr(), self.qb
        if self.kind == "range":
            out = torch.empty(qb * n, dtype=torch.float32, device=DEV)
            ref.range_distances_dev(qp, qb, out.data_ptr(), self.start, self.end)
        else:
            out = torch.empty(qb * self.k, dtype=torch.int64, device=DEV)
            if self.k == 1:
                ref.search_top1_keys_dev(qp, qb, out.data_ptr(), self.start, self.end)
            else:
                ref.search_topk_keys_dev(qp, qb, self.k, out.data_ptr(), self.start, self.end)
        ref.sync()
        return out


def _make_queries(seed, qb, rows, hard):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    q = _unit(gen, qb, rows.shape[1])
    for pos, what in hard.items():
        if what == "nan":
            q[pos, (pos * 7) % q.shape[1]] = float("nan")
        elif what == "inf":
            q[pos, (pos * 5) % q.shape[1]] = float("inf") if pos % 2 else -float("inf")
        elif what == "zero":
            q[pos] = 0.0
        elif what[0] == "copy":
            q[pos] = rows[what[1]]
        elif what[0] == "ulp":                    # one ulp from a row in one component
            q[pos] = rows[what[1]]
            q[pos, 9] = _ulp_up(q[pos, 9])
    return q.contiguous()


def _s_direct(rows, q, ids, start, end):
    """float64 sum of squared differences (direct differences, no norm expansion) of query q with rows[ids] over [start, end)."""
    x = rows[ids, start:end].double()
    return ((x - q[start:end].double()[None, :]) ** 2).sum(1)


def _k_smallest_s64(rows, qs, start, end, k, chunk=65536):
    """For each query of qs: the k smallest float64 sums of squared differences over all rows, ascending. The norm expansion in
    float64 (good to ~1e-15 for rows and queries of length <= 1) nominates every row within 1e-9 of the k-th smallest; those are
    recomputed from direct differences, which is what decides between a row and its planted one-ulp neighbour."""
    n = rows.shape[0]
    q64 = qs[:, start:end].double()
    q2 = (q64 * q64).sum(1)
    s_exp = torch.empty((qs.shape[0], n), dtype=torch.float64, device=DEV)
    for r0 in range(0, n, chunk):
        x = rows[r0:r0 + chunk, start:end].double()
        s_exp[:, r0:r0 + x.shape[0]] = q2[:, None] + (x * x).sum(1)[None, :] - 2.0 * (q64 @ x.T)
    t = torch.topk(s_exp, k, dim=1, largest=False).values[:, -1]
    out = []
    for i in range(qs.shape[0]):
        cand = torch.nonzero(s_exp[i] <= t[i] + 1e-9).flatten()
        out.append(torch.sort(_s_direct(rows, qs[i], cand, start, end)).values[:k])
    return out


def _sample(c, rng, count=16):
    """the finite hard queries of a call and random others: `count` in all, at least half of them random where the call has them"""
    hard = sorted(i for i, w in c.hard.items() if w not in ("nan", "inf"))[: count // 2]
    rest = [i for i in rng.permutation(c.qb).tolist() if i not in c.hard][: count - len(hard)]
    return hard + rest


def _check_call(c, expected, rows, rows_host, oracle, fir, rng, n):
    """Everything one call must satisfy; returns its expected keys (int64, on the device) for the distinct-answers check."""
    name = c.name
    if c.kind == "range":
        got = c.buf[: c.qb * n]
        assert torch.all(c.buf[c.qb * n:] == POISON32), f"{name}: wrote past the end of its buffer"
        assert not torch.any(got == POISON32), f"{name}: left distances unwritten"
        assert torch.equal(got, expected.view(torch.int32)), f"{name}: distances differ from the exact scan's"
        # float64: every distance (the MEAN over the range, as the reference's feature_distance) within the reference arithmetic's
        # rounding of the exact one, and two per query bit for bit
        m = c.end - c.start
        gam = (m + 3) * U / (1 - (m + 3) * U)
        dist = got.view(torch.float32).view(c.qb, n).double()
        qh = c.q.cpu().numpy()
        for i in range(c.qb):
            s = _s_direct(rows, c.q[i], torch.arange(n, device=DEV), c.start, c.end) / m
            assert torch.all((dist[i] - s).abs() <= gam * s), f"{name}: query {i} off the float64 sums"
            for j in (0, int(rng.integers(n))):
                assert dist[i, j].item() == oracle.feature_distance(qh[i], rows_host(j), c.start, c.end, 0), (name, i, j)
        return expected
    if c.kind in DEVICE_KINDS:
        keys = c.buf[: c.qb * c.k]
        assert torch.all(c.buf[c.qb * c.k:] == POISON), f"{name}: wrote past the end of its key buffer"
        assert not torch.any(keys == POISON), f"{name}: left {int((keys == POISON).sum())} key slots unwritten"
        bad = torch.nonzero(keys != expected).flatten()
        assert bad.numel() == 0, f"{name}: {bad.numel()} keys differ from the exact scan's (first slots {bad[:8].tolist()})"
        idx, dist = fir.keys_unpack(keys.cpu().numpy().view(np.uint64))
    else:
        idx, dist = c.host
        eidx, edist = fir.keys_unpack(expected.cpu().numpy().view(np.uint64))
        assert np.array_equal(idx, eidx.reshape(idx.shape)), f"{name}: rows differ from the exact scan's"
        assert np.array_equal(dist.view(np.uint32), edist.reshape(dist.shape).view(np.uint32)), f"{name}: distances differ"
    idx = idx.reshape(c.qb, c.k)
    dist = dist.reshape(c.qb, c.k)
    keys_np = expected.cpu().numpy().reshape(c.qb, c.k)
    # hard queries
    for pos, what in c.hard.items():
        if what in ("nan", "inf"):
            assert np.all(keys_np[pos] == KEY_NONE), f"{name}: query {pos} ({what}) found a row"
        elif what != "zero" and what[0] == "copy":
            want = LOWER.get(what[1], what[1])
            assert idx[pos, 0] == want and dist[pos, 0].view(np.uint32) == 0, f"{name}: copy of row {what[1]} -> {idx[pos, 0]} at {dist[pos, 0]}"
    # float64 check of a sample (always the hard queries)
    sample = _sample(c, rng)
    m = c.end - c.start
    gam = (m + 3) * U / (1 - (m + 3) * U)
    fac = (1 + gam) / (1 - gam)
    best = _k_smallest_s64(rows, c.q[sample], c.start, c.end, c.k)
    qh = c.q[sample].cpu().numpy()
    for j, i in enumerate(sample):
        r = idx[i]
        assert np.all(r >= 0) and len(set(r.tolist())) == c.k, f"{name}: query {i} rows {r}"
        assert np.all(np.diff(dist[i].astype(np.float64)) >= 0), f"{name}: query {i} distances not ascending {dist[i]}"
        s = _s_direct(rows, c.q[i], torch.from_numpy(r.astype(np.int64)).to(DEV), c.start, c.end)
        assert torch.all(s <= best[j] * fac), f"{name}: query {i} rows {r} sums {s.tolist()} against the smallest {best[j].tolist()}"
        for t in range(c.k):
            want = oracle.feature_distance(qh[j], rows_host(int(r[t])), c.start, c.end, 0)
            assert dist[i, t].view(np.uint32) == np.float32(want).view(np.uint32), f"{name}: query {i} slot {t}: {dist[i, t]} != {want}"
    return expected


def _run_checks(calls, rows, oracle, fir, ref, n, seed):
    """Exact keys, canaries, float64 sample of every call; no two calls with the same answers."""
    cache = {}

    def rows_host(j):
        if j not in cache:
            cache[j] = rows[j].cpu().numpy()
        return cache[j]

    rng = np.random.default_rng(seed)
    expected = []
    for c in calls:
        e = c.reference(ref, n)
        expected.append(_check_call(c, e, rows, rows_host, oracle, fir, rng, n))
    for a in range(len(calls)):
        for b in range(a + 1, len(calls)):
            if expected[a].shape == expected[b].shape:
                assert not torch.equal(expected[a], expected[b]), f"{calls[a].name} and {calls[b].name} have the same answers"


def _path_misses(calls):
    miss = []
    for c in calls:
        if c.expect is None:
            continue
        got = c.dispatch
        ok = got["path"] == c.expect if c.expect in ("mfma", "scan") else c.expect in got["kernel"]
        if not ok:
            miss.append((c.name, c.expect, got["path"], got["kernel"]))
    return miss


def _gallery_300k(seed=41):
    n, d = 300_000, 512
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    rows = _unit(gen, n, d)
    rows[250_001] = rows[4_321]                     # an exact duplicate further down: the lower row wins
    rows[200_000] = rows[7_777]                     # a one-ulp neighbour further down
    rows[200_000, 11] = _ulp_up(rows[200_000, 11])
    return rows.contiguous(), n, d


def _hard(qb, seed, nan=0, inf=0, zero=0, copies=(), ulps=()):
    """hard queries at positions that differ from call to call"""
    rng = np.random.default_rng(seed)
    pos = rng.permutation(qb).tolist()
    h = {}
    for what, count in (("nan", nan), ("inf", inf), ("zero", zero)):
        for _ in range(count):
            h[pos.pop()] = what
    for r in copies:
        h[pos.pop()] = ("copy", r)
    for r in ulps:
        h[pos.pop()] = ("ulp", r)
    return h


def test_one_stream_pipeline(fir, oracle):
    """About fifteen calls of every shape the dispatch distinguishes, queued on one stream with no host synchronisation until the
    end; the 8 192-query call with 40 NaN queries is directly followed by a 16-query call (where a stale list of uncertified queries
    would write past the smaller buffer)."""
    rows, n, d = _gallery_300k()
    st = torch.cuda.Stream()
    spec = [
        # name, kind, qb, k, start, end, hard, expected dispatch
        ("top1_8192_nan40", "top1", 8192, 1, 0, d, dict(nan=40, inf=2, zero=1, copies=(4_321, 200_000), ulps=(7_777,)), "mfma"),
        ("top1_16", "top1", 16, 1, 0, d, dict(inf=1, copies=(250_001,)), "f16x<3, 0, 0, 0, 1>"),
        ("top1_1000", "top1", 1000, 1, 0, d, dict(nan=3, zero=1, ulps=(7_777,)), "mfma"),
        ("top1_256", "top1", 256, 1, 0, d, dict(inf=2, copies=(4_321,)), "mfma"),
        ("top1_24", "top1", 24, 1, 0, d, dict(nan=2, zero=1), "f16x<3, 0, 0, 0, 2>"),
        ("top1_5", "top1", 5, 1, 0, d, dict(nan=1, copies=(4_321,)), None),
        ("top1_33", "top1", 33, 1, 0, d, dict(nan=1, inf=1, copies=(200_000,)), "mfma"),
        ("topk5_4096", "topk", 4096, 5, 0, d, dict(nan=5, zero=1, copies=(4_321,), ulps=(7_777,)), "mfma"),
        ("topk8_256", "topk", 256, 8, 0, d, dict(inf=1, copies=(250_001,)), "mfma"),
        ("topk2_129", "topk", 129, 2, 0, d, dict(nan=2, copies=(7_777,)), "mfma"),
        ("top1_prefix256", "top1", 300, 1, 0, 256, dict(nan=1, zero=1, copies=(4_321,)), "mfma"),
        ("top1_sub3_509", "top1", 64, 1, 3, 509, dict(inf=1, copies=(4_321,)), "scan"),
        ("range_3", "range", 3, 1, 5, 300, {}, None),
        ("gemm_few_1", "gemm_few", 1, 1, 0, d, dict(copies=(250_001,)), "k_gemm_scan_f16"),
        ("gemm_few_8", "gemm_few", 8, 1, 0, d, dict(nan=1, copies=(200_000,), ulps=(7_777,)), "k_gemm_scan_f16"),
    ]
    calls = []
    for i, (name, kind, qb, k, s0, e0, hard, expect) in enumerate(spec):
        h = _hard(qb, 1000 + i, **hard)
        calls.append(Call(name, kind, _make_queries(2000 + i, qb, rows, h), n, k, s0, e0, st, h, expect))
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g, \
            fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as ref:
        ref.set_large_batch_mfma(0)
        with fir.GemmSearch(g, 2) as m:
            for c in calls:
                c.enqueue(g, m)
            st.synchronize()
            stats = g.mfma_stats()
        _run_checks(calls, rows, oracle, fir, ref, n, 7)
    through_mfma = sum(sum(1 for w in c.hard.values() if w in ("nan", "inf")) for c in calls
                       if c.kind in ("top1", "topk") and c.dispatch["path"] == "mfma")
    assert stats["fallback_queries"] >= through_mfma, (stats, through_mfma)
    assert not _path_misses(calls), _path_misses(calls)
    print("top1_5 took", calls[5].dispatch["path"], calls[5].dispatch["kernel"])


def _identity_gallery(n_ids, per, d, seed):
    """class-ordered rows = identity centre x (1 +- 2.5 %), unit length (tests/test_gpu_gemm.py's recipe)"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    centres = torch.rand((n_ids, d), generator=g, device=DEV)
    rows = centres.repeat_interleave(per, dim=0) * (1 + 0.05 * (torch.rand((n_ids * per, d), generator=g, device=DEV) - 0.5))
    return (rows / rows.norm(dim=1, keepdim=True)).contiguous(), centres


def _identity_queries(centres, qb, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    who = torch.randint(0, centres.shape[0], (qb,), generator=g, device=DEV)
    q = centres[who] * (1 + 0.05 * (torch.rand((qb, centres.shape[1]), generator=g, device=DEV) - 0.5))
    return (q / q.norm(dim=1, keepdim=True)).contiguous()


def test_pipeline_with_overflowing_lists(fir, oracle, monkeypatch):
    """The second-chance rounds of many calls back to back: a row sample cut down to almost nothing (FIR_GEMM_SAMPLE_DIV) with the
    sample flow (FIR_GEMM_ADAPTIVE=0) over class-ordered identities -- experiment knobs that change no answer -- makes the
    candidate lists of many queries of every call overflow; those rounds carry the lists of uncertified queries and their bounds
    from the first pass to the second."""
    n_ids, per, d = 25_000, 40, 128
    n = n_ids * per
    rows, centres = _identity_gallery(n_ids, per, d, 77)
    st = torch.cuda.Stream()
    spec = [("top1", 4096, 1), ("top1", 128, 1), ("top1", 1000, 1), ("topk", 384, 5), ("top1", 2048, 1), ("top1", 200, 1),
            ("topk", 129, 5), ("top1", 3000, 1), ("top1", 256, 1), ("top1", 640, 1)]
    calls = []
    for i, (kind, qb, k) in enumerate(spec):
        q = _identity_queries(centres, qb, 300 + i)
        h = {}
        if i % 3 == 0:
            h = _hard(qb, 400 + i, nan=1, copies=(int(i * 97_001 % n),))
            q = _make_queries_onto(q, rows, h)
        calls.append(Call(f"{kind}{k}_{qb}", kind, q, n, k, 0, d, st, h, "mfma"))
    torch.cuda.synchronize()
    monkeypatch.setenv("FIR_GEMM_ADAPTIVE", "0")
    monkeypatch.setenv("FIR_GEMM_SAMPLE_DIV", "1000000")
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g, \
            fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as ref:
        ref.set_large_batch_mfma(0)
        for c in calls:
            c.enqueue(g)
        st.synchronize()
        stats = g.mfma_stats()
        assert "FIR_GEMM_SAMPLE_DIV" in g.last_dispatch()["knobs"]
        _run_checks(calls, rows, oracle, fir, ref, n, 8)
    assert stats["second_pass_queries"] > 0, stats
    assert not _path_misses(calls), _path_misses(calls)


def _make_queries_onto(q, rows, hard):
    q = q.clone()
    for pos, what in hard.items():
        if what == "nan":
            q[pos, (pos * 7) % q.shape[1]] = float("nan")
        elif what[0] == "copy":
            q[pos] = rows[what[1]]
    return q.contiguous()


def test_config5_shape_back_to_back(fir, oracle):
    """1M x 1280, the streamed d = 1280 form: 32- and 256-query calls queued back to back on one stream, as bench.py's rate()
    does. Whole pairs or calls of benign queries have been seen to lose their certificate only in this pattern; whatever the
    second passes cost, every key must be the exact scan's."""
    n, d = 1_000_000, 1280
    gen = torch.Generator(device=DEV)
    gen.manual_seed(55)
    rows = _unit(gen, n, d)
    st = torch.cuda.Stream()
    calls = []
    for i in range(12):
        qb = 32 if i % 2 == 0 else 256
        h = _hard(qb, 600 + i, copies=(int(i * 83_003 % n),)) if i % 4 == 1 else {}
        calls.append(Call(f"cfg5_{i}_{qb}", "top1", _make_queries(700 + i, qb, rows, h), n, 1, 0, d, st, h, "mfma"))
    torch.cuda.synchronize()
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g, \
            fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as ref:
        ref.set_large_batch_mfma(0)
        for c in calls:
            c.enqueue(g)
        st.synchronize()
        stats = g.mfma_stats()
        notes = g.uncertified_notes()
        try:
            _run_checks(calls, rows, oracle, fir, ref, n, 9)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  mfma_stats {stats}\n  uncertified notes {notes}") from None
    assert not _path_misses(calls), (_path_misses(calls), stats, notes)
    print("config-5 shape back to back:", stats, notes)


def test_sync_waits_for_calls_on_caller_streams(fir):
    """fir_gallery_sync blocks until all work queued by the handle is done -- including a device-pointer call queued on the
    caller's stream."""
    rows, n, d = _gallery_300k(43)
    q = _make_queries(51, 8192, rows, {})
    torch.cuda.synchronize()
    k = torch.empty(8192, dtype=torch.int64, device=DEV)
    st = torch.cuda.Stream()
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        g.search_top1_keys_dev(q.data_ptr(), 8192, k.data_ptr(), stream=st.cuda_stream)     # (builds the fp16 copy: synchronises)
        st.synchronize()
        g.search_top1_keys_dev(q.data_ptr(), 8192, k.data_ptr(), stream=st.cuda_stream)
        g.sync()
        idle = st.query()
        st.synchronize()
    assert idle, "fir_gallery_sync returned while a call queued on the caller's stream was still running"


def test_calls_across_streams(fir, oracle):
    """Calls on one handle take effect in call order whatever stream each is given: two user streams, the handle's own stream,
    host-pointer calls and an explicit matrix-core state, each small call right after a large one on another stream."""
    rows, n, d = _gallery_300k(45)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    spec = [
        ("s1_top1_8192", "top1", 8192, 1, s1, dict(nan=30, copies=(4_321,)), "mfma"),
        ("s2_top1_16", "top1", 16, 1, s2, dict(nan=1, copies=(200_000,)), None),
        ("own_topk5_4096", "topk", 4096, 5, None, dict(nan=4, ulps=(7_777,)), "mfma"),
        ("s1_top1_33", "top1", 33, 1, s1, dict(inf=1, copies=(250_001,)), "mfma"),
        ("host_top1_3", "host_top1", 3, 1, None, dict(copies=(4_321,)), None),
        ("s2_top1_2048", "top1", 2048, 1, s2, dict(nan=5, zero=1), "mfma"),
        ("gemm_s2_few_8", "gemm_few", 8, 1, s2, dict(nan=1, copies=(7_777,)), "k_gemm_scan_f16"),
        ("s1_topk2_129", "topk", 129, 2, s1, dict(nan=2, copies=(4_321,)), "mfma"),
        ("s2_gemm_top1_1000", "gemm_top1", 1000, 1, s2, dict(nan=3), "mfma"),
        ("host_topk3_5", "host_topk", 5, 3, None, dict(copies=(200_000,)), None),
        ("s1_top1_24", "top1", 24, 1, s1, dict(nan=2, copies=(250_001,)), None),
        ("own_top1_256", "top1", 256, 1, None, dict(inf=2), "mfma"),
        ("s2_top1_5", "top1", 5, 1, s2, dict(nan=1), None),
    ]
    calls = []
    for i, (name, kind, qb, k, s, hard, expect) in enumerate(spec):
        h = _hard(qb, 3000 + i, **hard)
        calls.append(Call(name, kind, _make_queries(4000 + i, qb, rows, h), n, k, 0, d, s, h, expect))
    torch.cuda.synchronize()
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g, \
            fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as ref:
        ref.set_large_batch_mfma(0)
        with fir.GemmSearch(g, 2) as m:
            for c in calls:
                c.enqueue(g, m)
            g.sync()
            idle = s1.query() and s2.query()
        s1.synchronize()
        s2.synchronize()
        _run_checks(calls, rows, oracle, fir, ref, n, 10)
    assert idle, "fir_gallery_sync returned while calls on the user streams were still running"
    assert not _path_misses(calls), _path_misses(calls)


def test_teardown_waits_for_inflight_calls(fir, oracle):
    """Freeing a matrix-core state (set_large_batch_mfma(0)) or a whole handle right after queueing a call on another stream:
    the call still completes with exact keys and intact canaries."""
    rows, n, d = _gallery_300k(47)
    s1 = torch.cuda.Stream()
    ha, hc = _hard(8192, 82, nan=10, copies=(4_321,)), _hard(4096, 85, nan=3)
    a = Call("s1_top1_8192", "top1", _make_queries(81, 8192, rows, ha), n, 1, 0, d, s1, ha, "mfma")
    b = Call("s1_top1_1000_after_off", "top1", _make_queries(83, 1000, rows, {}), n, 1, 0, d, s1, {}, "scan")
    c = Call("s1_topk5_4096_closed", "topk", _make_queries(84, 4096, rows, hc), n, 5, 0, d, s1, hc, "mfma")
    torch.cuda.synchronize()
    with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as ref:
        ref.set_large_batch_mfma(0)
        with fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0) as g:
            a.enqueue(g)
            g.set_large_batch_mfma(0)                      # frees the state call a is using
            b.enqueue(g)
        g2 = fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=0, device=0)
        c.enqueue(g2)
        g2.close()                                         # right after queueing on it
        s1.synchronize()
        _run_checks([a, b, c], rows, oracle, fir, ref, n, 11)
    assert not _path_misses([a, b, c]), _path_misses([a, b, c])
