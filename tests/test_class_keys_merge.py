"""fir_class_keys_merge: the host-side merge of the per-shard lists of fir_search_top_classes_keys_dev (keys[parts][qb][k] ascending,
classes likewise, FIR_KEY_NONE / -1 padding) into the list of the whole gallery -- per class the smallest key, then the k smallest.
Pure integer work: runs without a GPU. The expected lists are built with numpy from the same inputs."""
import numpy as np
import pytest

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def reference_merge(keys, classes, k):
    parts, qb, _ = keys.shape
    ko = np.full((qb, k), KEY_NONE, np.uint64)
    co = np.full((qb, k), -1, np.int32)
    for q in range(qb):
        kk = keys[:, q, :].reshape(-1)
        cc = classes[:, q, :].reshape(-1)
        live = kk != KEY_NONE
        kk, cc = kk[live], cc[live]
        best = {}
        for key, c in zip(kk.tolist(), cc.tolist()):
            if c not in best or key < best[c]:
                best[c] = key
        ranked = sorted((key, c) for c, key in best.items())[:k]
        for r, (key, c) in enumerate(ranked):
            ko[q, r], co[q, r] = key, c
    return ko, co


def shard_lists(fir, rng, parts, qb, k, n_classes, fill):
    """Per shard and query: `fill` (<= k) distinct classes with distinct keys (distance, global row), ascending, then padding.
    Rows are unique across the whole input, as the rows of disjoint shards are."""
    keys = np.full((parts, qb, k), KEY_NONE, np.uint64)
    classes = np.full((parts, qb, k), -1, np.int32)
    rows = rng.permutation(parts * qb * k).reshape(parts, qb, k)
    for p in range(parts):
        for q in range(qb):
            m = min(int(fill(p, q)), k, n_classes)
            cls = rng.choice(n_classes, size=m, replace=False)
            dist = rng.integers(0, 50, size=m).astype(np.float32) / np.float32(64.0)      # few values: equal distances are common
            kq = np.array([fir.key_pack(d, r) for d, r in zip(dist, rows[p, q, :m])], np.uint64)
            order = np.argsort(kq)
            keys[p, q, :m] = kq[order]
            classes[p, q, :m] = cls[order]
    return keys, classes


@pytest.mark.parametrize("parts", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 4, 32])
def test_random_lists_match_the_numpy_merge(fir, parts, k):
    rng = np.random.default_rng(100 * parts + k)
    # 12 classes over 5 parts of up to 32 slots: the same class turns up in several parts, and with k = 32 fewer than k classes exist
    for n_classes, fill in ((12, lambda p, q: k), (200, lambda p, q: k), (40, lambda p, q: rng.integers(0, k + 1))):
        keys, classes = shard_lists(fir, rng, parts, 7, k, n_classes, fill)
        ko, co = fir.class_keys_merge(keys, classes, k)
        eko, eco = reference_merge(keys, classes, k)
        assert np.array_equal(ko, eko)
        assert np.array_equal(co, eco)
        assert ko.shape == (7, k) and ko.dtype == np.uint64 and co.dtype == np.int32
        live = ko != KEY_NONE
        assert np.array_equal(co >= 0, live)
        for q in range(7):
            assert np.all(np.diff(ko[q][live[q]].astype(object)) > 0)             # ascending, no key twice
            assert len(set(co[q][live[q]].tolist())) == int(live[q].sum())       # no class twice


def test_the_smaller_key_of_a_class_wins_and_fewer_classes_than_k_come_back_padded(fir):
    kp = fir.key_pack
    keys = np.array([[[kp(0.50, 10), kp(0.75, 11), KEY_NONE]],
                     [[kp(0.25, 70), kp(0.50, 71), kp(0.90, 72)]]], np.uint64)
    classes = np.array([[[3, 5, -1]], [[5, 9, 3]]], np.int32)
    ko, co = fir.class_keys_merge(keys, classes, 3)
    # class 5: 0.25 (row 70) beats 0.75 (row 11); class 3: 0.50 (row 10) beats 0.90; class 9 at 0.50 with row 71 comes after row 10
    assert co.tolist() == [[5, 3, 9]]
    assert ko.tolist() == [[kp(0.25, 70), kp(0.50, 10), kp(0.50, 71)]]
    idx, dist = fir.keys_unpack(ko)
    assert idx.tolist() == [[70, 10, 71]] and dist.tolist() == [[0.25, 0.5, 0.5]]
    # two classes in all, k = 4: two slots of padding
    keys4 = np.array([[[kp(0.5, 1), KEY_NONE, KEY_NONE, KEY_NONE]], [[kp(0.5, 0), kp(0.6, 2), KEY_NONE, KEY_NONE]]], np.uint64)
    classes4 = np.array([[[1, -1, -1, -1]], [[2, 1, -1, -1]]], np.int32)
    ko, co = fir.class_keys_merge(keys4, classes4, 4)
    assert co.tolist() == [[2, 1, -1, -1]]                      # equal distances: the lower row index first
    assert ko.tolist() == [[kp(0.5, 0), kp(0.5, 1), int(KEY_NONE), int(KEY_NONE)]]


def test_all_padding_and_empty_batch(fir):
    keys = np.full((3, 2, 4), KEY_NONE, np.uint64)
    classes = np.full((3, 2, 4), -1, np.int32)
    ko, co = fir.class_keys_merge(keys, classes, 4)
    assert np.all(ko == KEY_NONE) and np.all(co == -1)
    ko, co = fir.class_keys_merge(np.zeros((2, 0, 4), np.uint64), np.zeros((2, 0, 4), np.int32), 4)
    assert ko.shape == (0, 4) and co.shape == (0, 4)
    with pytest.raises(ValueError):
        fir.class_keys_merge(keys, classes[:, :, :3], 4)
