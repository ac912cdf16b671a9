"""bench.py's --full / --dump-outputs options and what --dump-outputs writes (no GPU: the keys are packed on the host)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_a_plain_run_is_lean_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def _keys(fir, n):
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 1_000_000, n)
    dist = rng.random(n).astype(np.float32)
    keys = np.array([fir.key_pack(float(dv), int(i)) for i, dv in zip(idx, dist)], np.uint64)
    return torch.from_numpy(keys.view(np.int64)), idx, dist


def test_dump_outputs_writes_index_and_distance(fir, tmp_path):
    keys, idx, dist = _keys(fir, 300)
    bench.dump_outputs(str(tmp_path / "d"), fir, keys)
    assert sorted(os.listdir(tmp_path / "d")) == ["top1_distance.npy", "top1_index.npy"]
    gi = np.load(tmp_path / "d" / "top1_index.npy")
    gd = np.load(tmp_path / "d" / "top1_distance.npy")
    assert gi.dtype == np.float64 and gd.dtype == np.float32
    assert np.array_equal(gi, idx.astype(np.float64)) and np.array_equal(gd.view(np.uint32), dist.view(np.uint32))


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(fir, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 12 * 50)
    keys, idx, dist = _keys(fir, 300)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), fir, keys)
    q = np.load(tmp_path / "a" / "query.npy")
    assert q.shape == (50,) and np.array_equal(q, np.load(tmp_path / "b" / "query.npy"))
    sel = q.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "top1_index.npy"), idx[sel].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "top1_distance.npy"), dist[sel])
