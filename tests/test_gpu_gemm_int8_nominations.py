"""The int8 nomination pass itself -- k_gemm_proxy_f16x<3 | 1, 0, ODD, 0, 8, I8 = 1> (reported as k_gemm_proxy_i8x<MODE, ODD>) -- against
the float64 restatement of its form (I8Form, tests/test_gemm_int8_formulation.py), not just the final keys: the re-rank hides a pass
that nominates too much, and the exact device scan hides one that nominates too little or whose bound is in the wrong units.

Through the library's internal fir_gemm_nominations_ (the hook of tests/test_gpu_gemm_nominations.py, whose helpers and datasets --
tests/gemm_nomination_cases.py -- are used as they are) each case reads what one call of one super-batch handed its re-rank and asserts per
query

  soundness      every listed (p, row): row < n, no row twice, count = entries, |p - p_emu| <= B (the sums are exact integers: B is the
                 device's f32 row norm and the one rounding of its fma, no margin), and |(qnorm_c + p) - |q - g|^2| <= eabs_q +
                 e_rel (qnorm_c + G^2) with eabs_q formed from the DEVICE's qnorm_c and G^2
  completeness   every row with p_emu < tau - B is listed; in particular every row within one window of the smallest proxy of all rows
  the bound      tau = fl(T - qnorm_c), T = max((smallest proxy of the rows of full row blocks + qnorm_c) + window, 0): what
                 k_gemm_adapt_final computes from the T the pass was left with -- from both sides
  no detour      both counters (second pass, exact scan) are 0

The second-chance rounds' form <1, *> is reached with the audit build only (FIR_GEMM_ADAPT_DBG=3: every workgroup keeps its own bound)
on a gallery made for it (descending_fixture): every first list overflows, the int8 round's lists (which = 1) are held to the same
assertions against the bound the hand-over gave them, and the round answers every query -- no exact device scan."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_f16_form as form
import gemm_nomination_cases as cases
from test_gemm_int8_formulation import I8Form, descending_fixture
from test_gpu_gemm_nominations import CHUNK, _dev, _exact, nominations

pytestmark = pytest.mark.gpu

F32 = np.float32
U = form.U


def _set_int8(fir, m, mode):
    fn = C.CDLL(fir.lib_path()).fir_gemm_set_int8_
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int32]
    fn(m._h, mode)


def window_of(e_rel, qn, gmax, eabs):
    """nudge_up_(rounding_window_(e_rel, qn, gmax, eabs)) of fir_gemm_rerank.h, in float32"""
    w = F32(2.5) * (F32(e_rel) * (np.asarray(qn, F32) + F32(gmax)) + np.asarray(eabs, F32))
    return (w + np.abs(w) * F32(1e-6) + F32(1e-30)).astype(F32)


def check_i8_lists(f, q, ex, qmap=None, adaptive=False, label=""):
    n = f.n
    qmap = np.arange(len(ex["counts"])) if qmap is None else qmap
    gmax = F32(ex["gmax"])
    assert np.isclose(gmax, f.G2, rtol=f.d * U, atol=0), (label, gmax, f.G2)          # (the centred rows' largest norm, as the device summed it)
    figs = dict(b_ratio=0.0, e_ratio=0.0, tau_ratio=0.0, counts=ex["counts"].copy())
    for c0 in range(0, len(qmap), CHUNK):
        sl = slice(c0, c0 + CHUNK)
        p_emu, B, dist2, qn64, e_q = f.proxies(q[qmap[sl]])
        assert not f.unanswered.any(), label
        cnt, tau, qn = ex["counts"][sl].astype(np.int64), ex["tau"][sl].astype(np.float64), ex["qnorm"][sl]
        c = len(cnt)
        assert np.all(np.isfinite(qn)) and np.allclose(qn, qn64, rtol=f.d * U, atol=0), label
        eabs = f.eabs_of(qn, gmax, e_q)
        bound = eabs.astype(np.float64) + np.float64(f.e_rel) * (qn.astype(np.float64) + np.float64(gmax))
        w = window_of(f.e_rel, qn, gmax, eabs).astype(np.float64)
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
        fits = cnt <= form.K_LIST_CAP
        assert np.array_equal(listed.sum(axis=1)[fits], cnt[fits]), label
        r_safe = np.where(valid, row, 0)
        pe, b, d2 = (np.take_along_axis(a, r_safe, axis=1) for a in (p_emu, B, dist2))
        rb = np.where(valid, np.abs(p - pe) / b, 0.0)
        re = np.where(valid, np.abs(qn.astype(np.float64)[:, None] + p - d2) / bound[:, None], 0.0)
        figs["b_ratio"] = max(figs["b_ratio"], float(rb.max(initial=0.0)))
        figs["e_ratio"] = max(figs["e_ratio"], float(re.max(initial=0.0)))
        bad = np.argwhere(rb > 1.0)
        assert bad.size == 0, (label, "|p - p_emu| > B", float(rb.max()), [(int(qmap[c0 + i]), int(row[i, j])) for i, j in bad[:8]])
        assert np.all(re <= 1.0), (label, "|(qnorm_c + p) - |q - g|^2| above its bound", float(re.max()))
        if not adaptive:
            assert np.all((p < tau[:, None])[valid]), (label, "a listed proxy at or above tau")
        # completeness
        assert not np.any(np.isnan(tau)), label
        must = (p_emu < (tau[:, None] - B)) & fits[:, None]
        missing = np.argwhere(must & (listed == 0))
        assert missing.size == 0, (label, "rows below tau - B that are not listed", [(int(qmap[c0 + i]), int(j)) for i, j in missing[:8]])
        if adaptive:
            # T only falls, and only to (a full block's proxy + qnorm_c) + w: the smallest of them is what is left. The three f32 roundings
            # of T and tau take at most 4 u (qnorm_c + |tau| + w); the row's own proxy is within B of the emulation's.
            full = (n // 32) * 32
            qd = qn.astype(np.float64)
            if full:
                k = np.argmin(p_emu[:, :full], axis=1)
                pm = p_emu[np.arange(c), k]
                want = np.maximum((pm + qd) + w, 0.0) - qd
                slack = B.max(axis=1) + 4.0 * U * (qd + np.abs(want) + w)
                figs["tau_ratio"] = max(figs["tau_ratio"], float((np.abs(tau - want) / slack).max()))
                assert np.all(np.abs(tau - want) <= slack), (label, "tau is not (smallest proxy + qnorm_c + window) - qnorm_c", float((np.abs(tau - want) / slack).max()))
            else:
                assert np.all(np.isposinf(tau)), (label, "no full row block: T stays +inf")
                slack = np.zeros(c)
            inwin = (p_emu <= (p_emu.min(axis=1) + w - slack)[:, None] - B) & fits[:, None]
            assert not np.any(inwin & (listed == 0)), (label, "a row inside the window of the smallest proxy is not listed")
    return figs


def _report(name, kern, figs, st):
    cn = figs["counts"]
    print(f"INT8 NOMINATION {name}: {kern} | max |p-p_emu|/B {figs['b_ratio']:.3f} | max |err|/bound {figs['e_ratio']:.4f} | max |tau-want|/slack "
          f"{figs['tau_ratio']:.3f} | counts {int(cn.min())}/{int(np.median(cn))}/{int(cn.max())} | second pass {st['second_pass_queries']}, exact scan {st['fallback_queries']}")


# (name, rows, features, queries, ODD of the int8 form: units of 256 features -- 2 = one, 0 = an even number, 1 = three)
I8_CASES = [
    ("top1-d100", cases.N_MULTI, 100, cases.QB_MULTI, 2),
    ("top1-d512", cases.N_MULTI, 512, cases.QB_MULTI, 0),
    ("top1-d768", cases.N_MULTI, 768, cases.QB_MULTI, 1),
    ("near-duplicates", 20000, 512, 2048, 0),
    (f"top1-n{cases.N_SMALL}-d512", cases.N_SMALL, 512, 128, 0),
    (f"top1-n{cases.N_TINY}-d512", cases.N_TINY, 512, 128, 0),
]


@pytest.mark.parametrize("name,n,d,qb,odd", I8_CASES, ids=[c[0] for c in I8_CASES])
def test_lists_and_bounds_of_the_int8_form(fir, name, n, d, qb, odd):
    rows, q = cases.near_duplicate_data() if name == "near-duplicates" else cases.random_data(n, d, qb)
    assert rows.shape == (n, d) and q.shape == (qb, d)
    f = I8Form(rows)
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(qb, dtype=torch.int64, device=q_t.device)
    case = dict(entry="top", k=1, end=0)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            _set_int8(fir, m, 1)
            m.search_top1_keys_dev(q_t.data_ptr(), qb, keys.data_ptr())
            torch.cuda.synchronize()
            kern = g.last_dispatch()["kernel"]
            st = m.stats()
            ex = nominations(fir, m, 0)
        want = _exact(g, case, q_t, qb)
    assert f"k_gemm_proxy_i8x<3, {odd}>" in kern, kern
    assert len(ex["counts"]) == qb
    assert torch.equal(keys, want)
    figs = check_i8_lists(f, q, ex, adaptive=True, label=name)
    _report(name, kern, figs, st)
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


def test_second_chance_rounds_stay_int8_and_answer(fir_audit, monkeypatch):
    """MODE 1 of the int8 form as the second-chance round. With FIR_GEMM_ADAPT_DBG=3 (audit build) every workgroup of the first pass
    keeps its own bound, and on descending_fixture each then appends its whole range: the lists overflow. The round's lists are held to
    check_i8_lists against tau2 -- the smallest stored proxy of the first list + one window, in the units of the centred int8 proxies -- and
    every query is answered by the round: identical keys, nothing left to the exact device scan."""
    rows, q = descending_fixture()
    n, d = rows.shape
    qb = q.shape[0]
    monkeypatch.setenv("FIR_GEMM_ADAPT_DBG", "3")
    f = I8Form(rows)
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(qb, dtype=torch.int64, device=q_t.device)
    case = dict(entry="top", k=1, end=0)
    with fir_audit.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        with fir_audit.GemmSearch(g, 2) as m:
            _set_int8(fir_audit, m, 1)
            m.search_top1_keys_dev(q_t.data_ptr(), qb, keys.data_ptr())
            torch.cuda.synchronize()
            kern = g.last_dispatch()["kernel"]
            st = m.stats()
            first = nominations(fir_audit, m, 0)
            second = nominations(fir_audit, m, 1)
        want = _exact(g, case, q_t, qb)
    assert "k_gemm_proxy_i8x<3, 0>" in kern, kern
    over = first["counts"] > form.K_LIST_CAP
    print(f"INT8 SECOND CHANCE: first counts {int(first['counts'].min())}/{int(first['counts'].max())}, overflowed {int(over.sum())} of {qb}, "
          f"second counts {int(second['counts'].min())}/{int(second['counts'].max())}, {st}")
    assert over.sum() > 128, first["counts"]                                     # (more than one round)
    # exactly the overflowed queries took the round, and it answered all of them
    assert st["second_pass_queries"] == int(over.sum()) and st["fallback_queries"] == 0, (st, int(over.sum()))
    assert torch.equal(keys, want)
    idx, _ = fir_audit.keys_unpack(keys.cpu().numpy().view(np.uint64))
    assert np.all(idx == n - 1)
    # the LAST round's slots
    took = int(over.sum())
    assert len(second["counts"]) == (took - 1) % 128 + 1
    assert np.all(over[second["qmap"]])
    assert np.all(second["counts"] <= form.K_LIST_CAP) and np.all(second["counts"] >= 1)
    figs = check_i8_lists(f, q, second, qmap=second["qmap"].astype(np.int64), label="int8 second chance")
    # tau2 is what rerank_hand_over_ says: min(the first pass's bound, smallest STORED proxy of the first list + one window), in the
    # centred int8 proxies' units. (Not the smallest proxy of all rows + window: a workgroup stops appending to a list that is full,
    # and with it stops lowering T.) It lies above the smallest proxy of all rows, so the round's list holds every possible winner.
    qm = second["qmap"].astype(np.int64)
    p_emu, B, _, _, e_q = f.proxies(q[qm])
    qn = second["qnorm"]
    w = window_of(f.e_rel, qn, second["gmax"], f.eabs_of(qn, second["gmax"], e_q)).astype(np.float64)
    stored = form.f32_from_orderable((first["lists"][qm] >> np.uint64(32)).astype(np.uint32)).astype(np.float64)
    anchor = stored.min(axis=1)
    want_tau2 = np.minimum(first["tau"][qm].astype(np.float64), anchor + w)
    assert np.all(np.abs(second["tau"] - want_tau2) <= 4.0 * U * (np.abs(anchor) + w)), float(np.abs(second["tau"] - want_tau2).max())
    assert np.all(second["tau"] > p_emu.min(axis=1) + B.max(axis=1)), "tau2 at or below the smallest proxy"
    _report("second-chance", "fir::k_gemm_proxy_i8x<1, 0> (second-chance round)", figs, st)
