"""host/update_driver: fir::GalleryCache::appended after push_backs onto a cached gallery vector, then recognize_images_bf. The
answers equal a cold cache's over the same vector; an edited prefix makes the cache fall back to a whole upload."""
import json
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_appends_in_place_and_falls_back(tmp_path):
    driver = os.path.join(ROOT, "fast-image-recognition_amd", "host", "update_driver")
    d, n, n0, ncls = 48, 230, 130, 5
    names, classes, feats = [], [], []
    for k in range(n):
        names.append(f"/data/cls{k * ncls // n}/img{k}.jpg")
        classes.append(f"class_{k * ncls // n}")                     # class-major, as the loader expects
        feats.append(synth.uniform01(d, 2000 + k))
    path = str(tmp_path / "features.txt")
    synth.write_feature_file(path, names, classes, np.array(feats, np.float32))
    out = subprocess.run([driver, path, str(d), str(n0)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    assert res["images"] == n
    own = list(range(n))
    # the pushed-back rows reached the device as an append: every image finds itself, as with a cold cache
    assert res["plain_extended"] == 1
    assert res["plain_before"][:n0] == own[:n0] and all(0 <= i < n0 for i in res["plain_before"])
    assert res["plain_warm"] == res["plain_cold"] == own
    # a row of the prefix was edited before the push_backs: nothing is extended in place, the next lookup uploads everything
    assert res["edited_extended"] == 0
    assert res["edited_warm"] == res["edited_cold"] == own
