"""The nomination passes themselves -- k_gemm_proxy_f16x<MODE, STREAMED, ODD, 0, NJB>, k_gemm_scan_f16x, k_gemm_proxy<1>,
k_gemm_proxy_bf16* -- against the float64 emulation of their form (gemm_f16_form.py), not just the final keys: the re-rank and
its certificate are sound against rounding, not against a pass that computes a wrong proxy or leaves a row out, and the final keys
cannot tell (a proxy that is too small only lengthens a list; a lost certificate is answered by the second pass or the exact scan).

Part one reads, through the library's internal fir_gemm_nominations_, what each form handed the re-rank -- counts, bounds, list
entries -- for one call of one super-batch and asserts per query

  soundness      every listed (p, row): row < n, no row twice, |p - p_emu| <= 4 B, |p - p_true| <= E d, count = entries
  completeness   count <= kListCap: every row with p_emu < tau - 4 B is listed; in particular every row within one window of the
                 smallest proxy of all rows
  the bound      tau >= (smallest proxy of all rows) + window - slack for the forms that find it on the way or in a sample
  no detour      both counters (second pass, exact scan) are 0: test_gemm_f16_formulation.py shows that the emulation's
                 certificate holds with room for every query of these datasets

Part two makes every row of the gallery the winner of some query (the gallery's own rows, in order and shuffled): a proxy that is
too LARGE for one (row, position in its block, block's place in a wave's walk) shows only when that row is a query's true winner.

Every entry of kXTable is reached by a call of the shipped library: <3, *> and <4, *> by default; <2, *> and <1, *> with the
sample flow (FIR_GEMM_ADAPTIVE=0, a knob the shipped library honours; the K-nearest and distinct-class calls take it by default at
some shapes). The sample pass <2, *> writes no list: it is checked through the bound it produces. <1, *> also runs as the
second-chance round, whose lists live elsewhere (the state's `sc` set): fir_gemm_nominations_ reads them with which = 1
(test_second_pass_lists). The distinct-classes flow rewrites its list entries in the re-rank and is not
covered here."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_f16_form as form
import gemm_nomination_cases as cases

pytestmark = pytest.mark.gpu

CHUNK = 256
U = form.U
FIR_ERR_STATE = -5


def _export_fn(fir):
    lib = C.CDLL(fir.lib_path())
    fn = lib.fir_gemm_nominations_
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    return fn


def nominations(fir, m, which=0, n_rows=0, proxies=False):
    """what the most recent call on GemmSearch `m` handed its re-rank: dict of counts, tau, qnorm, lists [slots, max entries]
    (uint64, zero beyond a slot's entries), gmax, qmap and (the few-query scan) every row's proxy"""
    fn = _export_fn(fir)
    live, gmax = C.c_int32(), C.c_float()
    assert fn(m._h, which, 0, 0, 0, None, None, None, None, None, C.byref(gmax), None, C.byref(live)) == 0
    nq = live.value
    counts, tau, qn, qmap = np.zeros(nq, np.int32), np.zeros(nq, np.float32), np.zeros(nq, np.float32), np.zeros(nq, np.int32)
    if nq:
        assert fn(m._h, which, 0, nq, 0, counts.ctypes.data, tau.ctypes.data, qn.ctypes.data, None, None, None, qmap.ctypes.data, None) == 0
    me = int(min(max(int(counts.max()) if nq else 0, 1), form.K_LIST_CAP))
    lists = np.zeros((nq, me), np.uint64)
    px = np.zeros((nq, n_rows), np.float32) if proxies else None
    if nq:
        assert fn(m._h, which, 0, nq, me, None, None, None, lists.ctypes.data, px.ctypes.data if proxies else None, None, None, None) == 0
    lists[np.arange(me)[None, :] >= np.minimum(counts, form.K_LIST_CAP)[:, None]] = 0
    return dict(counts=counts, tau=tau, qnorm=qn, lists=lists, gmax=np.float32(gmax.value), qmap=qmap, proxies=px)


def _dev(a):
    t = torch.from_numpy(np.array(a, order="C", copy=True)).to(torch.device("cuda", 0))      # (a copy: the datasets are read-only)
    torch.cuda.synchronize()                            # (the library's streams do not wait for torch's)
    return t


def _search(m, case, q_t, qb, keys_t):
    if case["entry"] == "few":
        m.search_few_keys_dev(q_t.data_ptr(), qb, keys_t.data_ptr())
    elif case["k"] == 1:
        m.search_top1_keys_dev(q_t.data_ptr(), qb, keys_t.data_ptr())
    else:
        m.search_topk_keys_dev(q_t.data_ptr(), qb, case["k"], keys_t.data_ptr())
    torch.cuda.synchronize()


def _exact(g, case, q_t, qb):
    """the exact scan's keys on the same gallery handle"""
    k, end = case["k"], case["end"]
    keys = torch.empty(qb * k, dtype=torch.int64, device=q_t.device)
    g.set_large_batch_mfma(0)
    if k == 1:
        g.search_top1_keys_dev(q_t.data_ptr(), qb, keys.data_ptr(), 0, end)
    else:
        g.search_topk_keys_dev(q_t.data_ptr(), qb, k, keys.data_ptr(), 0, end)
    torch.cuda.synchronize()
    assert g.last_dispatch()["path"] == "scan"
    return keys


def check_lists(f, q, ex, k=1, qmap=None, adaptive_bound=False, sampled_blocks=None, label=""):
    """Part one's assertions for the slots of `ex` (slot i = query qmap[i] of q); returns the figures of the summary."""
    n = f.n
    qmap = np.arange(len(ex["counts"])) if qmap is None else qmap
    figs = dict(b_ratio=0.0, e_ratio=0.0, counts=ex["counts"].copy())
    for c0 in range(0, len(qmap), CHUNK):
        sl = slice(c0, c0 + CHUNK)
        p_emu, p_true, B, qn64 = f.emulate(q[qmap[sl]])
        cnt, tau, qn = ex["counts"][sl].astype(np.int64), ex["tau"][sl].astype(np.float64), ex["qnorm"][sl]
        c = len(cnt)
        assert np.all(np.isfinite(qn)) and np.allclose(qn, qn64, rtol=f.d * U, atol=0), label            # (|q|^2 as the device summed it)
        have = np.minimum(cnt, form.K_LIST_CAP)
        L = ex["lists"][sl]
        valid = np.arange(L.shape[1])[None, :] < have[:, None]
        row = (L & np.uint64(0xFFFFFFFF)).astype(np.int64)
        p = form.f32_from_orderable((L >> np.uint64(32)).astype(np.uint32)).astype(np.float64)
        qi = np.broadcast_to(np.arange(c)[:, None], row.shape)
        # soundness
        assert np.all(cnt >= 0), label
        assert np.all(row[valid] < n), (label, "a listed row past the end", int(row[valid].max()))
        listed = np.zeros((c, n), np.int32)
        np.add.at(listed, (qi[valid], row[valid]), 1)
        assert listed.max(initial=0) <= 1, (label, "a row listed twice", np.argwhere(listed > 1)[:4].tolist())
        assert np.array_equal(listed.sum(axis=1)[cnt <= form.K_LIST_CAP], cnt[cnt <= form.K_LIST_CAP]), label
        r_safe = np.where(valid, row, 0)
        pe, pt, b = (np.take_along_axis(a, r_safe, axis=1) for a in (p_emu, p_true, B))
        ed = form.e_d_of(f.e_rel, qn, ex["gmax"]).astype(np.float64)
        w = form.window_of(f.e_rel, qn, ex["gmax"]).astype(np.float64)
        rb = np.where(valid, np.abs(p - pe) / b, 0.0)
        re = np.where(valid, np.abs(p - pt) / ed[:, None], 0.0)
        figs["b_ratio"] = max(figs["b_ratio"], float(rb.max(initial=0.0)))
        figs["e_ratio"] = max(figs["e_ratio"], float(re.max(initial=0.0)))
        bad = np.argwhere(rb > form.K_MARGIN)
        assert bad.size == 0, (label, "|p - p_emu| > 4 B", float(rb.max()), [(int(qmap[c0 + i]), int(row[i, j])) for i, j in bad[:8]])
        assert np.all(re <= 1.0), (label, "|p - p_true| > E d", float(re.max()))
        if not adaptive_bound:
            # (a pass that finds its bound on the way appends below the bound of THAT moment, which is at or above the final one)
            assert np.all((p < tau[:, None])[valid]), (label, "a listed proxy at or above tau")
        # completeness
        assert not np.any(np.isnan(tau)), label
        fits = cnt <= form.K_LIST_CAP
        must = (p_emu < (tau[:, None] - form.K_MARGIN * B)) & fits[:, None]
        missing = np.argwhere(must & (listed == 0))
        assert missing.size == 0, (label, "rows below tau - 4 B that are not listed", [(int(qmap[c0 + i]), int(j)) for i, j in missing[:8]])
        # the bound: what the three float32 roundings of T and tau can take away is 4 u (|q|^2 + |tau| + w)
        kk = min(k, n)
        part = np.partition(p_emu, kk - 1, axis=1)
        slack = form.K_MARGIN * B.max(axis=1) + 4.0 * U * (qn64 + np.abs(np.where(np.isfinite(tau), tau, 0.0)) + w)
        assert np.all(tau >= part[:, :kk].min(axis=1) - slack), (label, "a bound below the smallest proxy")
        if adaptive_bound:
            # every T the pass held was >= (the K-th smallest proxy of all rows + |q|^2) + w, so tau is; and every row within the
            # window of it is listed
            assert np.all(tau >= part[:, kk - 1] + w - slack), (label, "tau below the K-th smallest proxy + window")
            inwin = (p_emu <= (part[:, 0] + w - slack)[:, None]) & fits[:, None]
            assert not np.any(inwin & (listed == 0)), (label, "a row inside the window of the smallest proxy is not listed")
        if sampled_blocks is not None and k == 1:
            # the sample flow's top-1 bound IS the smallest proxy of the sampled blocks' rows + one window (k_gemm_tau_min): the
            # sample pass <2, *> computed a wrong minimum if it is anything else
            rows_s = (sampled_blocks[:, None] * 32 + np.arange(32)[None, :]).ravel()
            rows_s = rows_s[rows_s < n]
            smin = p_emu[:, rows_s].min(axis=1)
            assert np.all(np.abs(tau - (smin + w)) <= slack + 2e-6 * np.abs(smin + w)), (label, "the sampled bound", float(np.abs(tau - (smin + w)).max()))
    return figs


def _report(case, kern, figs, st):
    cn = figs["counts"]
    print(f"NOMINATION {case['name']}: {kern} | max |p-p_emu|/B {figs['b_ratio']:.3f} | max |p-p_true|/(E d) {figs['e_ratio']:.4f} | "
          f"counts {int(cn.min())}/{int(np.median(cn))}/{int(cn.max())} | second pass {st['second_pass_queries']}, exact scan {st['fallback_queries']}")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_lists_and_bounds_of_every_form(fir, monkeypatch, case):
    rows, q = cases.data_of(case)
    n, qb, k = rows.shape[0], q.shape[0], case["k"]
    for name, val in case["env"].items():
        monkeypatch.setenv(name, val)
    f = form.Form(rows, case["precision"], case["end"])
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(qb * k, dtype=torch.int64, device=q_t.device)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=rows.shape[1], metric=0, device=0) as g:
        with fir.GemmSearch(g, case["precision"], case["end"]) as m:
            _search(m, case, q_t, qb, keys)
            kern = g.last_dispatch()["kernel"]
            st = m.stats()
            ex = nominations(fir, m, 0, n, proxies=case["entry"] == "few")
        want = _exact(g, case, q_t, qb)
    assert case["kernel"] in kern, kern
    assert len(ex["counts"]) == qb
    assert torch.equal(keys, want)
    sampled = None
    if case["env"] and case["precision"] == 2:
        # gemm_prep_f16_: every rb_stride-th row block, (rt_sample_rows + 31) / 32 of them
        nblk = (n + 31) // 32
        sample_blocks = (min(n, max(8192, n // 32)) + 31) // 32
        sampled = np.arange(sample_blocks) * max(1, nblk // sample_blocks)
        sampled = sampled[sampled < nblk]
    adaptive = case["precision"] == 2 and not case["env"]
    figs = check_lists(f, q, ex, k=k, adaptive_bound=adaptive, sampled_blocks=sampled, label=case["name"])
    if case["entry"] == "few":
        # every row's proxy, not only the listed ones
        p_emu, p_true, B, _ = f.emulate(q)
        r = np.abs(ex["proxies"].astype(np.float64) - p_emu) / B
        figs["b_ratio"] = max(figs["b_ratio"], float(r.max()))
        assert r.max() <= form.K_MARGIN, (case["name"], float(r.max()), np.argwhere(r > form.K_MARGIN)[:8].tolist())
    _report(case, kern, figs, st)
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


def test_no_call_yet_is_a_state_error(fir):
    rows, q = cases.random_data(cases.N_TINY, 100, 128)
    rows_t = _dev(rows)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=rows.shape[0], d=rows.shape[1], metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            live = C.c_int32(-1)
            assert _export_fn(fir)(m._h, 0, 0, 0, 0, None, None, None, None, None, None, None, C.byref(live)) == FIR_ERR_STATE


def test_second_pass_lists(fir, monkeypatch):
    """MODE 1 as the second-chance round: its lists (the `sc` set, which = 1) are held to the same assertions, against the bound
    k_gemm_sc_prep handed it; the detour is explained -- every query that took it had overflowed its first list."""
    rows, q = cases.second_pass_data()
    n, qb = rows.shape[0], q.shape[0]
    monkeypatch.setenv("FIR_GEMM_ADAPTIVE", "0")
    f = form.Form(rows, 2, 0)
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(qb, dtype=torch.int64, device=q_t.device)
    case = dict(entry="top", k=1, end=0)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=rows.shape[1], metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            _search(m, case, q_t, qb, keys)
            st = m.stats()
            first = nominations(fir, m, 0)
            second = nominations(fir, m, 1)
        want = _exact(g, case, q_t, qb)
    assert torch.equal(keys, want)
    over = first["counts"] > form.K_LIST_CAP
    assert over.sum() >= 8, first["counts"]
    # no unexplained detour: exactly the overflowed queries took the second pass, none the exact scan
    assert st["second_pass_queries"] == int(over.sum()) and st["fallback_queries"] == 0, (st, int(over.sum()))
    # the LAST round's slots: the queries behind the first 128 (k_gemm_fb.h: rounds of 128)
    took = int(over.sum())
    assert len(second["counts"]) == (took - 1) % 128 + 1
    assert np.all(over[second["qmap"]])
    figs = check_lists(f, q, second, k=1, qmap=second["qmap"].astype(np.int64), label="second pass")
    assert np.all(second["counts"] <= form.K_LIST_CAP)
    _report(dict(name="second-pass"), "fir::k_gemm_proxy_f16x<1, 0, 2> (second-chance round)", figs, st)


# ---- part two: every row as a winner ----

def _winner_queries(rows, order):
    """the gallery's own rows in `order`, scaled by 1 + 2^-12 so that none is bit-equal to its row"""
    return np.ascontiguousarray((rows[order] * np.float32(1 + 2.0 ** -12)).astype(np.float32))


def _orders(n):
    return {"in-order": np.arange(n), "shuffled": np.random.default_rng(5).permutation(n)}


def _expected_winner(rows, order):
    """row i itself; the planted copy (the last row = row 11): the lower row wins"""
    want = order.copy()
    n = rows.shape[0]
    if n > 12 and np.array_equal(rows[n - 1], rows[11]):
        want[order == n - 1] = 11
    return want


WINNER_CASES = [c for c in cases.CASES if c["n"] == cases.N_MULTI and c["qb"] == cases.QB_MULTI and c["data"] == "random"]
WINNER_CASES += [c for c in cases.CASES if c["name"] in ("f32-d200", "bf16-d200")]


@pytest.mark.parametrize("order", ["in-order", "shuffled"])
@pytest.mark.parametrize("case", WINNER_CASES, ids=[c["name"] for c in WINNER_CASES])
def test_every_row_wins_its_own_query(fir, monkeypatch, case, order):
    rows, _ = cases.data_of(case)
    n, k = rows.shape[0], case["k"]
    for name, val in case["env"].items():
        monkeypatch.setenv(name, val)
    perm = _orders(n)[order]
    q = _winner_queries(rows, perm)
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(n * k, dtype=torch.int64, device=q_t.device)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=rows.shape[1], metric=0, device=0) as g:
        with fir.GemmSearch(g, case["precision"], case["end"]) as m:
            _search(m, case, q_t, n, keys)
            kern = g.last_dispatch()["kernel"]
            st = m.stats()
        want = _exact(g, case, q_t, n)
    assert case["kernel"] in kern, kern
    idx, _ = fir.keys_unpack(keys.cpu().numpy().view(np.uint64))
    first = idx.reshape(n, k)[:, 0]
    wrong = np.flatnonzero(first != _expected_winner(rows, perm))
    assert wrong.size == 0, (case["name"], "queries whose own row did not win", [(int(i), int(perm[i]), int(first[i])) for i in wrong[:8]])
    assert torch.equal(keys, want)
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


@pytest.mark.parametrize("order", ["in-order", "shuffled"])
@pytest.mark.parametrize("qb,njb,d,streamed", [(16, 1, 512, 0), (32, 2, 512, 0), (16, 1, 641, 1), (32, 2, 641, 1)])
def test_every_row_wins_in_the_16_and_32_query_forms(fir, order, qb, njb, d, streamed):
    """many small calls through the device-pointer entry: every row of 2 245 in some query slot of a one- / two-block call"""
    rows, _ = cases.random_data(cases.N_SMALL, d, qb)
    n = rows.shape[0]
    perm = _orders(n)[order]
    q = _winner_queries(rows, perm)
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(n, dtype=torch.int64, device=q_t.device)
    case = dict(entry="top", k=1, end=0)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            kern = None
            for q0 in range(0, n, qb):
                m.search_top1_keys_dev(q_t.data_ptr() + q0 * d * 4, min(qb, n - q0), keys.data_ptr() + q0 * 8)
                kern = kern or g.last_dispatch()["kernel"]          # (the last call is a short one)
            torch.cuda.synchronize()
            st = m.stats()
        want = _exact(g, case, q_t, n)
    assert f"<3, {streamed}, 0, 0, {njb}>" in kern, kern
    idx, _ = fir.keys_unpack(keys.cpu().numpy().view(np.uint64))
    assert np.array_equal(idx, _expected_winner(rows, perm))
    assert torch.equal(keys, want)
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


@pytest.mark.parametrize("d", [100, 512, 520])
def test_sampled_rows_win_in_the_few_query_scan(fir, d):
    """eight queries a call: row 0, rows of the last full block, of the short block, the last but one (n - 1 is the planted copy)
    and a stride through the rest"""
    rows, _ = cases.random_data(cases.N_SMALL, d, 8)
    n = rows.shape[0]
    full = (n // 32) * 32
    picks = np.array([0, full - 32, full - 1, full, n - 2, n - 1, 777, 1234])
    q = _winner_queries(rows, picks)
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(8, dtype=torch.int64, device=q_t.device)
    case = dict(entry="few", k=1, end=0)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            _search(m, case, q_t, 8, keys)
            assert "k_gemm_scan_f16x" in g.last_dispatch()["kernel"]
            st = m.stats()
        want = _exact(g, case, q_t, 8)
    idx, _ = fir.keys_unpack(keys.cpu().numpy().view(np.uint64))
    assert np.array_equal(idx, _expected_winner(rows, picks))
    assert torch.equal(keys, want)
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st
