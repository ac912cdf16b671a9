"""fir_search_knn without a GPU: the numpy emulation of the radix select (knn_select_ref.emulate: the kernels' digit widths, pass
order, early exit, compaction rule and sorting network) held to a plain sort of the keys (knn_select_ref.expected_keys), on the
inputs where a select goes wrong: cuts inside runs of equal distances, all-equal rows, signed zeros and denormals, NaN / inf /
values at and above 100000, fewer rows than k, no rows. And the binding: capi.py resolves the new symbols, the header declares them."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import knn_select_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 8, 9, 64, 255, 256, 1000, 1024)


def check(dist, k, row_offset=0):
    dist = np.asarray(dist, np.float32)
    want = ref.expected_keys(dist, k, row_offset)
    got = ref.emulate(dist, k, row_offset, shuffle_seed=k)
    assert got.dtype == np.uint64 and got.shape == (k,)
    assert np.array_equal(got, want)
    # the contract read off the result itself: ascending, padding last, only qualifying rows, the row offset in the low word
    live = got[got != ref.KEY_NONE]
    assert np.all(live[1:] > live[:-1])
    assert np.all(got[live.shape[0]:] == ref.KEY_NONE)
    idx, d = ref.unpack(got)
    assert np.all(d[: live.shape[0]] < ref.NOT_FOUND)
    assert live.shape[0] == min(k, int(ref.qualifies(dist).sum()))
    rows = idx[: live.shape[0]].astype(np.int64) - row_offset
    assert np.array_equal(d[: live.shape[0]].view(np.uint32), (dist[rows] + np.float32(0.0)).view(np.uint32))
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", (1, 63, 64, 65, 200, 4097, 20000))
def test_random_distances(n, k):
    rng = np.random.default_rng(n * 131 + k)
    check(rng.random(n, dtype=np.float32) * np.float32(3.0), k)
    check((rng.standard_normal(n) * 1e-3).astype(np.float32), k)        # negative distances order below positive ones


@pytest.mark.parametrize("k", KS)
def test_more_than_k_rows_share_the_kth_distance(k):
    rng = np.random.default_rng(k)
    n = 3000
    d = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), n)          # three distinct distances: every cut falls inside a run
    got = check(d, k)
    idx, _ = ref.unpack(got)
    cut = d[idx[k - 1]]
    run = np.flatnonzero(d == cut)
    assert run.shape[0] > k // 3                                        # the K-th place lies inside a long run ...
    taken = idx[d[idx] == cut]
    assert np.array_equal(taken, run[: taken.shape[0]])                 # ... of which exactly the lowest rows are taken


@pytest.mark.parametrize("k", (1, 8, 9, 300, 1024))
@pytest.mark.parametrize("value", (0.0, 1.5, 99999.99, -2.0))
def test_all_equal(value, k):
    got = check(np.full(1500, value, np.float32), k)
    idx, _ = ref.unpack(got)
    assert np.array_equal(idx, np.arange(k))


@pytest.mark.parametrize("k", (1, 5, 64, 500))
def test_signed_zeros_and_denormals(k):
    rng = np.random.default_rng(5)
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38], np.float32)
    d = rng.choice(tiny, 700)
    got = check(d, k)
    idx, dist = ref.unpack(got)
    # -0 and +0 are one distance: among the zeros the order is the row's alone, and what comes back is +0
    z = idx[(dist == 0) & (idx >= 0)]
    assert np.all(np.diff(z) > 0)
    assert not np.any(np.signbit(dist[(dist == 0) & (idx >= 0)]))


@pytest.mark.parametrize("k", (1, 8, 40, 256, 1024))
def test_nan_inf_and_the_not_found_bound(k):
    rng = np.random.default_rng(9)
    d = (rng.random(900, dtype=np.float32) * np.float32(2e5)).astype(np.float32)     # about half at or above 100000
    d[::7] = np.nan
    d[3::11] = np.inf
    d[5::13] = -np.inf                                                               # -inf < 100000: qualifies, sorts first
    d[17] = np.float32(100000.0)                                                     # the bound itself does not qualify
    d[18] = np.nextafter(np.float32(100000.0), np.float32(0.0))                      # one ulp below does
    got = check(d, k)
    idx, _ = ref.unpack(got)
    assert 17 not in idx
    few = np.full(300, np.nan, np.float32)
    few[[4, 250, 77]] = [2.0, 1.0, 2.0]
    got = check(few, k)
    idx, _ = ref.unpack(got)
    assert np.array_equal(idx[:3], [250, 4, 77][: min(k, 3)])
    check(np.full(100, np.nan, np.float32), k)                                       # nothing qualifies: all padding
    check(np.full(100, np.inf, np.float32), k)


@pytest.mark.parametrize("k", (1, 8, 9, 1024))
@pytest.mark.parametrize("n", (0, 1, 5, 8, 9))
def test_fewer_rows_than_k(n, k):
    check(np.arange(n, 0, -1).astype(np.float32), k)


@pytest.mark.parametrize("k", (1, 9, 200))
def test_row_offset_is_the_low_word(k):
    d = np.random.default_rng(3).random(500, dtype=np.float32)
    a = check(d, k, 0)
    b = check(d, k, 1 << 20)
    assert np.array_equal(b, a + np.uint64(1 << 20))


def test_passes_stop_when_the_rank_takes_a_whole_bin():
    """Random distances are decided within the distance word and its first row byte or so; equal distances need the row digits."""
    d = np.random.default_rng(1).random(100000, dtype=np.float32)
    _, passes = ref.radix_threshold(ref.all_keys(d), 100)
    assert passes <= 5
    _, passes = ref.radix_threshold(ref.all_keys(np.ones(100000, np.float32)), 100)
    assert passes > 5


def test_prefix_property():
    d = np.random.default_rng(2).choice(np.array([1.0, 2.0, 3.0, 4.0], np.float32), 2000)
    big = ref.emulate(d, 300)
    for k in (1, 5, 8, 299):
        assert np.array_equal(ref.emulate(d, k), big[:k])


def test_bound_and_declared_symbols():
    """capi.py resolves fir_search_knn / _keys_dev / fir_sharded_search_knn with their argument lists, the wrappers exist, and
    include/fir_amd.h declares the three calls and FIR_KNN_MAX = 1024."""
    import __graft_entry__ as ge

    pkg = ge.load_package()
    sigs = {name: args for name, _, args in pkg.capi.SYMBOLS}
    for name in ("fir_search_knn", "fir_search_knn_keys_dev", "fir_sharded_search_knn"):
        assert name in sigs and len(sigs[name]) == 8
        assert hasattr(pkg.lib(), name)
    assert callable(pkg.Gallery.search_knn) and callable(pkg.Gallery.search_knn_keys_dev) and callable(pkg.ShardedGallery.search_knn)
    header = open(os.path.join(ROOT, "include", "fir_amd.h")).read()
    assert re.search(r"#define\s+FIR_KNN_MAX\s+1024\b", header)
    for name in ("fir_search_knn", "fir_search_knn_keys_dev", "fir_sharded_search_knn"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert ref.KNN_MAX == 1024


def test_host_side_checks_under_sanitizers(tmp_path):
    """The k check and the tile / scratch sizing of fir_search_knn are plain host functions (the top of csrc/fir_knn_select.h):
    tests/knn_plan_main.cpp, a stand-alone program, runs them over the edge sizes under the address and undefined-behaviour
    sanitizers. Nothing here is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knn_plan_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # (clang links them statically by itself)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *static, os.path.join(ROOT, "tests", "knn_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "ok"
