"""numpy restatement of fir_search_top1_other_class, of the gallery self-join over it and of the false-accept threshold
(include/fir_amd.h), on knn_select_ref's keys: no tolerance anywhere. Everything works from a distance matrix.

A row qualifies for query q iff `label[row] != exclude[q]` (an int32 compare) and `dist < 100000.0f` is true (NaN: never). The answer
is the smallest packed key (orderable(distance bits) << 32) | uint32(row + row offset) of the qualifying rows -- the first minimum
in row order --, FIR_KEY_NONE when there is none."""
import numpy as np

import knn_select_ref as ks

KEY_NONE = ks.KEY_NONE
F32 = np.float32


def expected_keys(dist, labels, exclude, row_offset=0):
    """[qb] uint64: dist [qb, n] float32, labels [n] int32, exclude a scalar or [qb] int32."""
    dist = np.atleast_2d(np.asarray(dist, F32))
    labels = np.asarray(labels, np.int32)
    exclude = np.broadcast_to(np.asarray(exclude, np.int32).reshape(-1), (dist.shape[0],))
    out = np.full(dist.shape[0], KEY_NONE, np.uint64)
    for q in range(dist.shape[0]):
        keys = ks.all_keys(dist[q], row_offset)[labels != exclude[q]]      # FIR_KEY_NONE where the row does not qualify by distance
        if keys.shape[0]:
            out[q] = keys.min()
    return out


def first_minimum(dist_row, labels, exclude):
    """The same answer the reference's way (db_features.cpp:329-332 over the rows of other classes): a running strict minimum in
    row order. (idx, dist), -1 / 100000 when nothing qualifies."""
    best, best_i = F32(100000.0), -1
    for j, v in enumerate(np.asarray(dist_row, F32)):
        if int(labels[j]) != int(exclude) and v < best:                      # (False for NaN)
            best, best_i = v, j
    return best_i, best


def self_join_keys(dist, labels, row0=0, row_offset=0):
    """Keys of rows [row0, row0 + m) of a gallery against the whole gallery, each with its own class excluded: dist [m, n] holds
    feature_distance(row row0 + i, row j) -- row i is the query."""
    labels = np.asarray(labels, np.int32)
    m = np.atleast_2d(dist).shape[0]
    return expected_keys(dist, labels, labels[row0:row0 + m], row_offset)


def other_class_dists_reference_way(dist, labels):
    """otherClassesDists of ann.cpp:286-298 for a square matrix dist[i, j]: sort row i's (distance, j) pairs ascending -- std::sort on
    pairs, so ties by ascending row --, take the first entry of another class; a row without one contributes nothing. The reference
    has no cut-off at 100000 and no NaN: the caller passes distances below it."""
    labels = np.asarray(labels, np.int32)
    out = []
    for i in range(dist.shape[0]):
        order = np.lexsort((np.arange(dist.shape[1]), np.asarray(dist[i], F32)))
        for j in order:
            if labels[j] != labels[i]:
                out.append(dist[i, j])
                break
    return np.array(out, F32)


def threshold(dists, rate):
    """(threshold, min, max, rows_counted, ind) of getThreshold (ann.cpp:84-93) over the distances of the counted rows: ind =
    (int)((float)size * rate), the float product of size_t and float; None for the threshold when ind is outside [0, size)."""
    dists = np.asarray(dists, F32)
    size = dists.shape[0]
    prod = F32(size) * F32(rate)
    if size == 0 or np.isnan(prod) or prod < 0:
        return None, None, None, size, None
    ind = int(prod)                                                          # truncation, as the C cast
    s = np.sort(dists)
    return (s[ind] if ind < size else None), s[0], s[-1], size, ind


def keys_to_dists(keys):
    """The statistic the threshold reads: the distances of the keys that are not FIR_KEY_NONE."""
    keys = np.asarray(keys, np.uint64)
    return ks.unpack(keys[keys != KEY_NONE])[1]


def pick_of_two(keys2, cls2, exclude):
    """The lemma of the routed form: keys2 / cls2 [qb, 2] = the two nearest distinct classes (ascending keys, FIR_KEY_NONE / -1 for an
    unused slot); the answer is the first entry whose class differs from exclude[q], FIR_KEY_NONE when neither does."""
    keys2 = np.asarray(keys2, np.uint64).reshape(-1, 2)
    cls2 = np.asarray(cls2, np.int32).reshape(-1, 2)
    exclude = np.broadcast_to(np.asarray(exclude, np.int32).reshape(-1), (keys2.shape[0],))
    out = np.full(keys2.shape[0], KEY_NONE, np.uint64)
    for q in range(keys2.shape[0]):
        for r in range(2):
            if keys2[q, r] != KEY_NONE and cls2[q, r] != exclude[q]:
                out[q] = keys2[q, r]
                break
    return out


def two_nearest_classes(dist_row, labels, num_classes, row_offset=0):
    """fir_search_top_classes(k = 2) for one query: per class in [0, num_classes) its smallest key, then the two smallest of those."""
    labels = np.asarray(labels, np.int32)
    keys = ks.all_keys(dist_row, row_offset)
    best = {}
    for j in range(labels.shape[0]):
        c = int(labels[j])
        if 0 <= c < num_classes and keys[j] != KEY_NONE and (c not in best or keys[j] < best[c]):
            best[c] = keys[j]
    top = sorted((k, c) for c, k in best.items())[:2]
    k2 = [k for k, _ in top] + [KEY_NONE] * (2 - len(top))
    c2 = [c for _, c in top] + [-1] * (2 - len(top))
    return np.array(k2, np.uint64), np.array(c2, np.int32)
