"""host/pca_driver: extractPCA, fir::fit_pca, fir::project_gallery and fir::project (host/fir_pca.h) over a synthetic feature file
(tests/golden holds none).

extractPCA keeps every component, so it is a rotation about the mean followed by ONE rounding of each coordinate to float32: every
pairwise mean squared distance D = |x - y|^2 / d moves by at most (2 |x - y| e + e^2) / d with e = sqrt(d) 2^-23 (|x| + |y|) -- each
of the d coordinates of x' and y' is off by at most half an ulp of a value no larger than the centred row's norm, |x - mean| <=
|x| + |mean|, and the rows here have norm 1; the eigen solver's orthogonality error (1e-12 d, tests/test_pca_eigen.py) is far below
that. The brute-force answers are therefore unchanged wherever the two best float64 distances differ by more than 2^-18 relative."""
import json
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    driver = os.path.join(ROOT, "fast-image-recognition_amd", "host", "pca_driver")
    d, n, ncls = 32, 300, 6
    rng = np.random.default_rng(3100)
    base = np.abs(rng.standard_normal((n, 5)) @ rng.standard_normal((5, d))) + 0.1 * rng.random((n, d))
    names = [f"/data/cls{k * ncls // n}/img{k}.jpg" for k in range(n)]
    classes = [f"class_{k * ncls // n}" for k in range(n)]                    # class-major, as the loader expects
    path = str(tmp_path_factory.mktemp("pca") / "features.txt")
    synth.write_feature_file(path, names, classes, base.astype(F32))
    out = subprocess.run([driver, path, str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout)
    assert r["images"] == n and r["classes"] == ncls
    r["d"], r["n"] = d, n
    r["x"] = np.array(r["rows"], F32).reshape(n, d)
    r["y"] = np.array(r["pca"], F32).reshape(n, d)
    return r


def test_extract_pca_keeps_every_pairwise_distance(res):
    x, y, d = res["x"].astype(F64), res["y"].astype(F64), res["d"]
    assert res["class_no"] == sorted(res["class_no"])                           # same class and image order
    dx = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    dy = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    norms = np.linalg.norm(x, axis=1)
    e = np.sqrt(d) * 2.0 ** -23 * (norms[:, None] + norms[None, :])
    bound = (2 * np.sqrt(dx) * e + e * e) / d
    err = np.abs(dy - dx) / d
    print("worst |dD| / bound", float(np.max(err / bound)))
    assert np.all(err <= bound)
    assert np.abs(y.mean(axis=0)).max() < 1e-6                                  # centred
    var = y.var(axis=0)
    assert np.all(var[:-1] >= var[1:] * (1 - 1e-6))                             # leading components first


def test_brute_force_answers_are_unchanged_away_from_ties(res):
    x, n = res["x"].astype(F64), res["n"]
    gal = np.array([r for r in range(n) if r % 3], np.int64)
    tests = np.array([r for r in range(n) if r % 3 == 0], np.int64)
    assert len(res["bf_orig"]) == len(res["bf_pca"]) == tests.size
    dist = ((x[tests][:, None, :] - x[gal][None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]
    d1, d2 = dist[np.arange(tests.size), order[:, 0]], dist[np.arange(tests.size), order[:, 1]]
    graded = (d2 - d1) > 2.0 ** -18 * d2
    assert np.mean(~graded) <= 0.05
    orig, pca = np.array(res["bf_orig"]), np.array(res["bf_pca"])
    assert np.array_equal(orig[graded], order[graded, 0])
    assert np.array_equal(pca[graded], orig[graded])
    cls = np.array(res["class_no"])
    assert np.array_equal(cls[gal[pca[graded]]], cls[gal[orig[graded]]])        # the brute-force class of every graded query


def test_fit_pca_with_a_take_list_is_scatter_then_symmetric_eigen(res):
    d, n = res["d"], res["n"]
    count = res["direct_count"]
    assert count == n // 2
    assert res["fit_mean"] == res["direct_mean"]
    assert res["fit_basis"] == res["direct_basis"]                              # the same bytes: "%.17g" round-trips a double
    assert res["fit_values"] == [v / count for v in res["direct_values"]]
    basis = np.array(res["fit_basis"]).reshape(d, d)
    assert np.linalg.norm(basis @ basis.T - np.eye(d)) <= 1e-12 * d
    x = res["x"].astype(F64)[1::2]
    cov = np.cov(x.T, bias=True)
    want = np.linalg.eigh(cov)[0][::-1]
    assert np.allclose(res["fit_values"], want, rtol=0, atol=1e-10 * want[0])
    assert res["projected_equal"] == 1                                          # project_gallery's rows = project's, bit for bit
