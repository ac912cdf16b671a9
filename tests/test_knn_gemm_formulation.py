"""The matrix-core form of the K nearest rows for 8 < K <= 256 (csrc/fir_gemm_knn.h), checked without a GPU on the numpy restatement
of tests/knn_gemm_ref.py: over the shapes tests/test_gpu_knn_gemm.py runs on the device, with the shipped constants, every row at or
below the sample bound D_s is listed, no list overflows and the certificate holds -- so the device test's "no query went to the exact
form" is a condition the formulation alone can satisfy. The sizing of the sample (plain C++ at the top of csrc/fir_knn_select.h) runs
in a stand-alone program under the address and undefined-behaviour sanitizers and is compared with the restatement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gemm_f16_form as gf
import knn_gemm_ref as ref
import knn_select_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def holds(f, where=""):
    assert f["listed_all"].all(), (where, np.flatnonzero(~f["listed_all"])[:8])
    assert f["count"].max() <= gf.K_LIST_CAP, (where, int(f["count"].max()))
    assert (f["margin"] > 0).all(), (where, np.flatnonzero(~(f["margin"] > 0))[:8], float(f["margin"].min()))


@pytest.mark.parametrize("n,d,qb,k", ref.SHAPES)
def test_the_device_shapes_need_no_exact_form(n, d, qb, k):
    rows, q = ref.case(n + d, n, d, qb)
    f = ref.formulation(rows, q, k)
    holds(f, (n, d, qb, k))
    if n >= 65536:
        assert (f["ds"] < ref.NOT_FOUND).all() and f["count"].max() < n // 4       # the bound, not the list capacity, decides what is appended
    if n <= gf.K_LIST_CAP:
        assert f["count"].max() <= n


def test_a_feature_prefix():
    rows, q = ref.case(11, 3000, 512, 70)
    holds(ref.formulation(rows, q, 33, d=64))


@pytest.mark.parametrize("spread", [0.3, 0.005])
def test_clustered_class_major_identities(spread):
    rows, q = ref.clustered(spread)
    f = ref.formulation(rows, q, 64)
    assert f["listed_all"].all()
    if spread == 0.3:
        holds(f, spread)


def test_copies_of_one_row():
    """200 copies: K = 50 cuts the run of equal distances, K = 250 asks for more rows than there are (no bound: everything is listed
    and re-ranked). 6 000 copies: every row is at the bound and every list overflows -- the exact form's case."""
    one = synth.make_gallery(5, 1, 64, 0)
    q, _ = synth.make_queries(5, synth.make_gallery(6, 100, 64, 0), 9, 0)
    rows = np.tile(one, (200, 1)).astype(np.float32)
    for k in (50, 250):
        f = ref.formulation(rows, q, k)
        holds(f, k)
        assert (f["count"] == 200).all()
        assert ((f["ds"] == ref.NOT_FOUND) == (k > 200)).all()
    f = ref.formulation(np.tile(one, (6000, 1)).astype(np.float32), q, 16)
    assert f["listed_all"].all() and (f["count"] == 6000).all()


def test_the_sample_bound_is_an_upper_bound_of_the_kth_distance_and_exact_on_the_sample():
    rows, q = ref.case(66128, 66000, 128, 200)
    q = q[:6]
    for k in (9, 64):
        idx = ref.sample_rows(rows.shape[0], k)
        assert idx.shape[0] == 32768 and np.all(np.diff(idx) > 0) and idx[-1] >= rows.shape[0] * 15 // 16
        ds = ref.sample_bound(rows, q, k)
        for i in range(q.shape[0]):
            full = np.sort(ref.reference_distances(rows, q[i], 128))
            samp = np.sort(ref.reference_distances(rows[idx], q[i], 128))
            assert ds[i].view(np.uint32) == samp[k - 1].view(np.uint32)
            assert ds[i] >= full[k - 1]
    # fewer than K rows, and rows that do not qualify
    small = rows[:40].copy()
    assert (ref.sample_bound(small, q, 41) == ref.NOT_FOUND).all() and (ref.sample_bound(small, q, 40) < ref.NOT_FOUND).all()
    small[7] = 1.0e4
    assert (ref.sample_bound(small, q, 40) == ref.NOT_FOUND).all()


def test_tau_follows_the_kernel():
    e = gf.e_rel_of(2, 128)
    t = ref.tau_of(e, np.array([0.01, 100000.0, np.nan], np.float32), 128, np.array([1.0, 1.0, 1.0], np.float32), np.float32(1.0))
    w = np.float32(2.5) * e * np.float32(2.0)
    v = (np.float32(0.01) * np.float32(128) - np.float32(1.0)) + w
    assert t[0] == v + abs(v) * np.float32(1e-6) + np.float32(1e-30) and t[0] > v
    assert t[1] == np.inf and t[2] == np.inf                       # no bound; (a NaN bound cannot come out of the select)
    assert np.isnan(ref.tau_of(e, np.array([0.01], np.float32), 128, np.array([np.nan], np.float32), np.float32(1.0))[0])


def test_expected_keys_are_the_contract():
    d = np.array([3.0, 1.0, 1.0, np.nan, 100000.0, 0.5], np.float32)
    keys = ref.expected(d, 5, 10)
    idx, dist = knn_select_ref.unpack(keys)
    assert idx.tolist() == [15, 11, 12, 10, -1] and dist.tolist() == [0.5, 1.0, 1.0, 3.0, 100000.0]


def test_bound_and_declared_symbols():
    import __graft_entry__ as ge

    pkg = ge.load_package()
    sigs = {name: args for name, _, args in pkg.capi.SYMBOLS}
    assert "fir_gemm_search_knn_keys_dev" in sigs and len(sigs["fir_gemm_search_knn_keys_dev"]) == 6
    assert hasattr(pkg.lib(), "fir_gemm_search_knn_keys_dev") and callable(pkg.GemmSearch.search_knn_keys_dev)
    header = open(os.path.join(ROOT, "include", "fir_amd.h")).read()
    assert re.search(r"#define\s+FIR_GEMM_KNN_MAX\s+256\b", header)
    assert re.search(r"\bint\s+fir_gemm_search_knn_keys_dev\s*\(", header)
    assert ref.GEMM_KNN_MAX == 256


PLAN_CASES = [(0, 9), (1, 9), (63, 256), (64, 9), (65, 256), (333, 256), (3000, 9), (4097, 64), (32767, 9), (32768, 256), (32769, 9), (66000, 64),
              (100000, 256), (1000000, 9), (1000000, 64), (1000000, 256), (3728270, 9), (3728399, 9)]


def test_the_sample_sizing_under_sanitizers(tmp_path):
    """tests/knn_gemm_plan_main.cpp, a stand-alone program, runs knn_sample_plan over the edge sizes under the address and
    undefined-behaviour sanitizers and prints the plans asked for here: they are the restatement's. Nothing here is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knn_gemm_plan_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # (clang links them statically by itself)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *static, os.path.join(ROOT, "tests", "knn_gemm_plan_main.cpp"), "-o", exe], check=True)
    args = [str(v) for n, k in PLAN_CASES for div in (ref.SAMPLE_DIV, 64) for v in (n, k, div)]
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert out[-1] == "ok", out[-3:]
    lines = out[:-1]
    assert len(lines) == 2 * len(PLAN_CASES)
    for line in lines:
        w = line.split()
        n, k, div, tiles, rows, group, stride = (int(x) for x in w[:7])
        runs = [tuple(int(x) for x in r.split(":")) for r in w[7:]]
        p = ref.sample_plan(n, k, div)
        assert (p["tiles"], p["rows"], p["group"], p["stride"], p["runs"]) == (tiles, rows, group, stride, runs), line
        assert sum(t for _, t in runs) == tiles and len(runs) <= ref.SAMPLE_RUNS
