"""host/fir_eigen.cpp (fir::symmetric_eigen, cyclic Jacobi) without a GPU: tests/pca_eigen_main.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers, decomposes random symmetric, diagonal, repeated-eigenvalue and rank-1 matrices
of d in {1, 2, 7, 64}; here the results are held to numpy.linalg.eigh and to the order and sign conventions of fir_eigen.h.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = (1, 2, 7, 64)


def matrices(d):
    rng = np.random.default_rng(900 + d)
    b = rng.standard_normal((d, d))
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    rep = np.repeat(rng.standard_normal((d + 2) // 3) * 4.0, 3)[:d]            # every eigenvalue three times (as far as d allows)
    u = rng.standard_normal(d)
    return {"random": (b + b.T) * 10.0,
            "diagonal": np.diag(rng.permutation(d) - d / 3.0),
            "equal diagonal": np.diag(np.repeat([2.0, -1.0], [(d + 1) // 2, d // 2])),
            "repeated": (q * rep[None, :]) @ q.T,
            "rank 1": np.outer(u, u),
            "zero": np.zeros((d, d))}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("eigen") / "pca_eigen_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++14", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    os.path.join(ROOT, "tests", "pca_eigen_main.cpp"), os.path.join(ROOT, "fast-image-recognition_amd", "host", "fir_eigen.cpp"), "-o", exe],
                   check=True)
    cases = [(d, name, (a + a.T) / 2) for d in DS for name, a in matrices(d).items()]
    text = "".join(f"{d}\n" + "\n".join(repr(float(x)) for x in a.reshape(-1)) + "\n" for d, _, a in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert out[-1] == "ok"
    got, at = {}, 0
    for d, name, a in cases:
        sweeps = int(out[at])
        nums = np.array([float(w) for w in out[at + 1:at + 1 + d + d * d]])
        at += 1 + d + d * d
        got[d, name] = (a, sweeps, nums[:d], nums[d:].reshape(d, d))
    assert at == len(out) - 1
    return got


@pytest.mark.parametrize("d", DS)
def test_against_numpy_eigh(results, d):
    for (dd, name), (a, sweeps, values, vectors) in results.items():
        if dd != d:
            continue
        norm = np.linalg.norm(a, 2)
        want = np.linalg.eigh(a)[0][::-1]
        assert 0 <= sweeps < 20, (d, name, sweeps)
        assert np.all(np.abs(values - want) <= 1e-12 * norm), (d, name)
        for k in range(d):
            assert np.linalg.norm(a @ vectors[k] - values[k] * vectors[k]) <= 1e-12 * d * norm, (d, name, k)
        assert np.linalg.norm(vectors @ vectors.T - np.eye(d)) <= 1e-12 * d, (d, name)


@pytest.mark.parametrize("d", DS)
def test_order_and_sign_conventions(results, d):
    for (dd, name), (a, _, values, vectors) in results.items():
        if dd != d:
            continue
        assert np.all(values[:-1] >= values[1:]), (d, name)                     # descending
        big = np.argmax(np.abs(vectors), axis=1)                                # (argmax: the first on ties)
        assert np.all(vectors[np.arange(d), big] > 0), (d, name)                # the largest-magnitude component is positive
    # equal eigenvalues keep the order of their index: a diagonal matrix needs no rotation, so its vectors are unit vectors and
    # tell which index each value came from
    a, _, values, vectors = results[d, "equal diagonal"]
    src = np.argmax(np.abs(vectors), axis=1)
    assert np.array_equal(vectors, np.eye(d)[src])
    for k in range(d - 1):
        if values[k] == values[k + 1]:
            assert src[k] < src[k + 1], (d, k)
    a, sweeps, values, vectors = results[d, "zero"]
    assert sweeps == 0 and np.all(values == 0) and np.array_equal(vectors, np.eye(d))
