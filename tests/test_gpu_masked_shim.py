"""host/subset_driver: fir::recognize_images_bf_subset -- two different splits of one cached gallery vector searched through a row
mask, against a cold cache over each compacted vector (what a caller without masks uploads per split), mapped back. One upload
serves both splits. The feature file is written by synth, like those of the other shim tests (tests/golden holds none)."""
import json
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_splits_of_one_upload_equal_the_compacted_galleries(tmp_path):
    driver = os.path.join(ROOT, "fast-image-recognition_amd", "host", "subset_driver")
    d, n, ncls = 48, 230, 5
    names, classes, feats = [], [], []
    for k in range(n):
        names.append(f"/data/cls{k * ncls // n}/img{k}.jpg")
        classes.append(f"class_{k * ncls // n}")                     # class-major, as the loader expects
        feats.append(synth.uniform01(d, 3000 + k))
    feats[200] = feats[4]                                            # duplicates: row 3 is outside split A and its copy inside; rows 4 and 200 are both inside
    feats[202] = feats[3]
    path = str(tmp_path / "features.txt")
    synth.write_feature_file(path, names, classes, np.array(feats, np.float32))
    out = subprocess.run([driver, path, str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    assert res["images"] == n
    assert res["masked_uploads"] == 1                                # the total set went up once for both splits
    assert res["a_rows"] == [r for r in range(n) if r % 3 != 0]
    assert res["a_rows"] != res["b_rows"] and 0 < len(res["b_rows"]) < n
    for s in ("a", "b"):
        rows, masked, cold = res[s + "_rows"], res[s + "_masked"], res[s + "_cold"]
        assert len(masked) == len(cold) == n
        assert all(0 <= c < len(rows) for c in cold)
        assert masked == [rows[c] for c in cold], s                  # the compacted answers, mapped back
        inside = set(rows)
        assert all(m in inside for m in masked)
        assert all(masked[r] == r for r in rows if r not in (200, 202, 3, 4))      # a row of the split finds itself
    assert res["a_masked"][3] == 202 and res["a_masked"][200] == 4 and res["a_masked"][0] != 0     # row 3 is outside split A: its copy answers; row 0 has none
