"""Cross-check of the C restatement against the real reference build (oracle/_ref) on fresh seeds -- beyond what
tests/golden/reference_outputs.npz pins. The reference's results for these cases are recorded in
tests/golden/oracle_vs_ref.npz (tests/golden/make_vs_ref_golden.py), so the restatement is checked everywhere; where
oracle/_ref is built, the live reference must still produce exactly the recorded results."""
import functools
import os

import numpy as np
import pytest

import golden_cases as gc
import oracle_lib
import synth

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_ref.npz")

DIST_CASES = [(metric, seed, n, d) for seed, n, d in [(1, 333, 48), (2, 2048, 512), (3, 129, 1536), (4, 64, 200)]
              for metric in (gc.L2, gc.CHI2, gc.KL)]
TWD_SEEDS = [5, 6]
CLS_CASES = [(7, 5.0), (8, 0.3)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ranges(d):
    return ((0, d), (0, min(64, d)), (d // 3, d - 1))


def live_distances(metric, seed, n, d):
    ref = oracle_lib.load_ref(gc.METRIC_NAMES[metric])
    rows = synth.make_gallery(seed, n, d, metric)
    q, _ = synth.make_queries(seed, rows, 4, metric)
    db = ref.db(rows, None, 0)
    out = {"metric": ref.metric}
    for i, qi in enumerate(q):
        for j, (s, e) in enumerate(ranges(d)):
            out[f"dist/{i}/{j}"] = db.all_distances(qi, s, e)
        out[f"bf/{i}"] = db.recognize_image_bf(qi, d)
        out[f"fd/{i}"] = ref.feature_distance(qi, rows[0], 1, d - 1)
    db.close()
    return out


def live_default_max_features():
    ref = oracle_lib.load_ref("l2")
    rows = synth.make_gallery(9, 200, 1536, 0)
    q, _ = synth.make_queries(9, rows, 3, 0)
    db = ref.db(rows, None, 1536)
    out = {"features_count": ref.features_count}
    for i, qi in enumerate(q):
        out[f"bf/{i}"] = db.recognize_image_bf(qi, 0)
        out[f"ann/{i}"] = db.ann_bruteforce(qi)
    db.close()
    return out


def live_twd(seed):
    ref = oracle_lib.load_ref("l2")
    rows, cls, q, ncls = gc.twd_case(seed=seed, n=808, d=280, n_classes=101)
    db = ref.db(rows, cls, 0)
    out = {}
    for i, qi in enumerate(q):
        out[f"conv/{i}"] = [db.twd_conventional(qi, ncls, typ, th, 64) for (typ, th) in gc.TWD_CONVENTIONAL]
        out[f"prop/{i}"] = [db.twd_proposed(qi, ncls, fc, th) for (fc, th) in gc.TWD_PROPOSED]
    db.close()
    return out


def live_cls(seed, frac):
    rc = oracle_lib.load_ref("cls")
    x, lab, ncls = gc.cls_case(seed=seed, n=300, d=64, n_classes=10)
    rc.set_dataset(x, lab, ncls)
    train, tcls, test = rc.split(frac, seed=seed)
    out = dict(zip(("train", "tcls", "test", "mn", "mx", "avg", "sd"), (train, tcls, test) + tuple(rc.stats())))
    out["pred"] = [[rc.predict_row(kind, param, int(r)) for kind, param in ((0, 1), (0, 3), (1, 0), (2, 0))] for r in test[:60]]
    return out


@functools.lru_cache(maxsize=None)
def load_gold():
    return np.load(GOLD_PATH)


def recorded(key, live):
    """The reference's results for case `key` as recorded; when oracle/_ref is built, `live()` must reproduce them bit for bit."""
    gold = load_gold()
    want = {k[len(key) + 1:]: gold[k] for k in gold.files if k.startswith(key + "/")}
    assert want, f"no recorded reference results for {key} (tests/golden/make_vs_ref_golden.py)"
    if oracle_lib.have_ref():
        got = {k: np.asarray(v) for k, v in live().items()}
        assert sorted(got) == sorted(want), key
        for k, v in got.items():
            assert v.dtype == want[k].dtype and v.shape == want[k].shape and v.tobytes() == want[k].tobytes(), f"{key}/{k}"
    return want


def all_recorded():
    """Every case through the live reference (for make_vs_ref_golden.py)."""
    out = {}
    for metric, seed, n, d in DIST_CASES:
        out.update({f"dist/{metric}/{seed}_{n}_{d}/{k}": v for k, v in live_distances(metric, seed, n, d).items()})
    out.update({f"maxf/{k}": v for k, v in live_default_max_features().items()})
    for seed in TWD_SEEDS:
        out.update({f"twd/{seed}/{k}": v for k, v in live_twd(seed).items()})
    for seed, frac in CLS_CASES:
        out.update({f"cls/{seed}_{frac}/{k}": v for k, v in live_cls(seed, frac).items()})
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("metric", [gc.L2, gc.CHI2, gc.KL])
@pytest.mark.parametrize("seed,n,d", [(1, 333, 48), (2, 2048, 512), (3, 129, 1536), (4, 64, 200)])
def test_distances_and_argmin(oracle, metric, seed, n, d):
    want = recorded(f"dist/{metric}/{seed}_{n}_{d}", lambda: live_distances(metric, seed, n, d))
    assert int(want["metric"]) == metric
    rows = synth.make_gallery(seed, n, d, metric)
    q, _ = synth.make_queries(seed, rows, 4, metric)
    for i, qi in enumerate(q):
        for j, (s, e) in enumerate(ranges(d)):
            assert np.array_equal(bits(want[f"dist/{i}/{j}"]), bits(oracle.all_distances(rows, qi, s, e, metric)))
        assert int(want[f"bf/{i}"]) == oracle.recognize_bf(rows, qi, 0, d, metric)[0]
        assert bits(want[f"fd/{i}"]) == bits(oracle.feature_distance(qi, rows[0], 1, d - 1, metric))


def test_default_max_features_is_features_count(oracle):
    """max_features == 0 -> FEATURES_COUNT (db_features.cpp:320-321); ann BruteForce uses the full range."""
    want = recorded("maxf", live_default_max_features)
    assert int(want["features_count"]) == 1536
    rows = synth.make_gallery(9, 200, 1536, 0)
    q, _ = synth.make_queries(9, rows, 3, 0)
    for i, qi in enumerate(q):
        e = oracle.recognize_bf(rows, qi, 0, 1536, 0)[0]
        assert int(want[f"bf/{i}"]) == e
        assert int(want[f"ann/{i}"]) == e


@pytest.mark.parametrize("seed", TWD_SEEDS)
def test_twd_classifiers(oracle, seed):
    want = recorded(f"twd/{seed}", lambda: live_twd(seed))
    rows, cls, q, ncls = gc.twd_case(seed=seed, n=808, d=280, n_classes=101)
    for i, qi in enumerate(q):
        for c, (typ, th) in enumerate(gc.TWD_CONVENTIONAL):
            assert tuple(want[f"conv/{i}"][c]) == oracle.twd_conventional(rows, cls, qi, ncls, typ, th, 64)
        for c, (fc, th) in enumerate(gc.TWD_PROPOSED):
            assert tuple(want[f"prop/{i}"][c]) == oracle.twd_proposed(rows, cls, qi, fc, th)[:2]


@pytest.mark.parametrize("seed,frac", CLS_CASES)
def test_classification_predictors(oracle, seed, frac):
    want = recorded(f"cls/{seed}_{frac}", lambda: live_cls(seed, frac))
    x, lab, ncls = gc.cls_case(seed=seed, n=300, d=64, n_classes=10)
    train, tcls, test = want["train"], want["tcls"], want["test"]
    tr = x[train]
    mn, mx, avg, sd = oracle.train_stats(tr)
    assert np.array_equal(avg, want["avg"]) and np.array_equal(sd, want["sd"]) and np.array_equal(mn, want["mn"]) and np.array_equal(mx, want["mx"])
    for r, pred in zip(test[:60], want["pred"]):
        assert pred[0] == oracle.knn_predict(tr, tcls, avg, ncls, x[r], 1)[0]
        assert pred[1] == oracle.knn_predict(tr, tcls, avg, ncls, x[r], 3)[0]
        assert pred[2] == oracle.pnn_predict(tr, tcls, avg, ncls, x[r])[0]
        assert pred[3] == oracle.pnn_predict_seq(tr, tcls, avg, ncls, x[r])[0]
