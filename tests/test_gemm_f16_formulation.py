"""No GPU: the float64 emulation of the nomination forms (gemm_f16_form.py) alone shows, for every dataset the GPU tests of the
nomination pass use (gemm_nomination_cases.py), that the rounding the forms INTEND satisfies what the certificate rests on:

  1. |p_emu - p_true| <= E d minus the share of E d that is set aside for the device's f32 work (8 d u (|q|^2 + max |g|^2));
  2. the float64-nearest row of every query (the K nearest for K = 5) lies inside the re-rank's window [p1, p1 + 2 E d];
  3. the certificate inequality holds for every query -- none of these datasets is hostile -- and by more than 4 B / d, so a
     query that takes a second pass or the exact scan on the GPU has no excuse (test_gpu_gemm_nominations.py: both counters 0)."""
import numpy as np
import pytest

import gemm_f16_form as form
import gemm_nomination_cases as cases

CHUNK = 256


def _combos():
    seen, out = {}, []
    for c in cases.CASES:
        key = (c["data"], c["n"], c["d"], c["qb"], c["precision"], c["end"])
        if key not in seen:
            seen[key] = dict(c, ks=set())
            out.append(seen[key])
        seen[key]["ks"].add(c["k"])
    return out


COMBOS = _combos()


@pytest.mark.parametrize("combo", COMBOS, ids=[f"{c['data']}-n{c['n']}-d{c['d']}-q{c['qb']}-p{c['precision']}-e{c['end']}" for c in COMBOS])
def test_the_intended_rounding_satisfies_the_premises(combo):
    rows, q = cases.data_of(combo)
    f = form.Form(rows, combo["precision"], combo["end"])
    assert f.n == combo["n"] and f.d_row == combo["d"]
    worst_err, worst_margin = 0.0, np.inf
    for c0 in range(0, q.shape[0], CHUNK):
        p_emu, p_true, B, qn = f.emulate(q[c0:c0 + CHUNK])
        ed = form.e_d_of(f.e_rel, qn, f.gmax).astype(np.float64)
        share = (form.f32_share_of(f.d) * (qn.astype(np.float32) + f.gmax)).astype(np.float64)
        # 1. the form's own rounding leaves the f32 share of E d to the device
        err = np.abs(p_emu - p_true)
        assert np.all(err <= (ed - share)[:, None]), (combo["name"], float((err / (ed - share)[:, None]).max()))
        worst_err = max(worst_err, float((err / ed[:, None]).max()))
        # ... and the device's f32 work on top of it, bounded by B, fits that share: premise 1 for the device's proxies
        assert np.all(B <= share[:, None]), combo["name"]
        for k in sorted(combo["ks"]):
            kk = min(k, f.n)
            cert = form.certificate(f, p_emu, p_true, qn, k=k)
            # 2. the K float64-nearest rows lie inside the window hung on the K-th smallest proxy
            nearest = np.argpartition(p_true, kk - 1, axis=1)[:, :kk]
            pn = np.take_along_axis(p_emu, nearest, axis=1)
            assert np.all(pn >= cert["p_min"][:, None]) and np.all(pn <= (cert["pk"] + 2.0 * cert["ed"])[:, None]), (combo["name"], k)
            # 3. the certificate holds, and by more than the device's f32 work can take away
            bmax = B.max(axis=1)
            assert np.all(cert["margin"] > form.K_MARGIN * bmax / f.d), (combo["name"], k, float(cert["margin"].min()))
            assert np.all(cert["count"] <= form.K_LIST_CAP), (combo["name"], k, int(cert["count"].max()))
            worst_margin = min(worst_margin, float((cert["margin"] * f.d / cert["ed"]).min()))
    print(f"{combo['name']}: max |p_emu - p_true| / (E d) = {worst_err:.4f}, smallest certificate margin = {worst_margin:.3f} E")


def test_the_second_pass_dataset_overflows_the_sampled_bound_and_certifies_under_the_second():
    """the hostile dataset of test_second_pass_lists: more than kListCap rows lie below (smallest SAMPLED proxy + window), a few
    below (smallest proxy of all rows + window), under which the certificate holds"""
    rows, q = cases.second_pass_data()
    f = form.Form(rows, 2, 0)
    p_emu, p_true, B, qn = f.emulate(q)
    ed = form.e_d_of(f.e_rel, qn, f.gmax).astype(np.float64)
    share = (form.f32_share_of(f.d) * (qn.astype(np.float32) + f.gmax)).astype(np.float64)
    assert np.all(np.abs(p_emu - p_true) <= (ed - share)[:, None]) and np.all(B <= share[:, None])
    w = form.window_of(f.e_rel, qn, f.gmax).astype(np.float64)
    even = (np.arange(f.n) // 32) % 2 == 0
    first = p_emu[:, even].min(axis=1) + w
    assert np.all((p_emu < first[:, None] - form.K_MARGIN * B).sum(axis=1) > form.K_LIST_CAP)
    # the second bound hangs on a STORED proxy: at worst the (overflow + 1)-th smallest of the rows below the first bound
    cert = form.certificate(f, p_emu, p_true, qn, k=1, tau=p_emu.min(axis=1) + w)
    assert np.all(cert["margin"] > form.K_MARGIN * B.max(axis=1) / f.d) and np.all(cert["count"] <= 1024), int(cert["count"].max())


def test_orderable_bits_round_trip():
    v = np.array([-3.5, -0.0, 0.0, 1e-30, 2.25, np.inf], np.float32)
    b = v.view(np.uint32)
    o = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)      # fir::f32_orderable
    assert np.array_equal(form.f32_from_orderable(o).view(np.uint32), b)
    assert np.all(np.diff(o[[0, 2, 3, 4, 5]].astype(np.int64)) > 0)


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20)], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7)], np.float32)
    assert np.array_equal(form.bf16_round(x), want)
