"""host/split_driver: fir::recognize_split_bf -- one whole train / test split on the device (the gallery is the subset handle of the
split's rows, the queries are the other rows gathered out of the same upload, the keys mapped back) against
fir::recognize_images_bf_subset, the masked search over that upload, for two splits. One upload serves everything. The feature
file is the one of tests/test_gpu_masked_shim.py, written by synth."""
import json
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_device_side_splits_equal_the_masked_searches(tmp_path):
    driver = os.path.join(ROOT, "fast-image-recognition_amd", "host", "split_driver")
    d, n, ncls = 48, 230, 5
    names, classes, feats = [], [], []
    for k in range(n):
        names.append(f"/data/cls{k * ncls // n}/img{k}.jpg")
        classes.append(f"class_{k * ncls // n}")                     # class-major, as the loader expects
        feats.append(synth.uniform01(d, 3000 + k))
    feats[200] = feats[4]                                            # duplicates: row 3 is a test row of split A and its copy 202 a gallery row;
    feats[202] = feats[3]                                            # rows 4 and 200 are both gallery rows there
    path = str(tmp_path / "features.txt")
    synth.write_feature_file(path, names, classes, np.array(feats, np.float32))
    out = subprocess.run([driver, path, str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    assert res["images"] == n
    assert res["uploads"] == 1                                       # the total set went up once: no split uploaded anything
    assert res["a_test_rows"] == [r for r in range(n) if r % 3 == 0]
    assert res["a_test_rows"] != res["b_test_rows"] and 0 < len(res["b_test_rows"]) < n
    for s in ("a", "b"):
        tests, split, masked = res[s + "_test_rows"], res[s + "_split"], res[s + "_masked"]
        assert len(split) == len(masked) == len(tests)
        assert split == masked, s                                    # the contract: the masked call's answers
        outside = set(tests)
        assert all(0 <= r < n and r not in outside for r in split)   # every answer is a gallery row of the split
    a = dict(zip(res["a_test_rows"], res["a_split"]))
    assert a[3] == 202                                               # row 3's copy answers at distance 0
