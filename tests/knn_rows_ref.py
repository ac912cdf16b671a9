"""KNNClassifier::predict (qt_cpp/classification.cpp:116-170) row by row, in plain numpy float64: the mean distances of every
training row in the reference's own operation order, the K' nearest rows in (distance, row) order, and the vote's walk over that
order. tests/test_knn_rows_formulation.py pins it to the oracle on the CPU; tests/test_gpu_knn_rows.py grades what the matrix-core
kNN path hands its vote against it."""
import numpy as np

CHUNK_BYTES = 1 << 20        # a temporary of mean_distances: queries are taken in chunks whose [chunk, nt] arrays stay in the cache


def mean_distances(tr, avg, q):
    """dist[qi, t] = (sum over features, in feature order, of ((tr[t] - avg) - (q[qi] - avg))^2) / d: classification.cpp:123-143,
    one rounding per operation. Non-finite queries give non-finite distances without a warning."""
    tr = np.ascontiguousarray(tr, np.float64)
    q = np.ascontiguousarray(q, np.float64).reshape(-1, tr.shape[1])
    avg = np.asarray(avg, np.float64)
    nt, d = tr.shape
    gc = np.ascontiguousarray((tr - avg).T)             # [d, nt]: one feature of every row is contiguous
    qc = q - avg
    out = np.empty((q.shape[0], nt), np.float64)
    step = max(1, CHUNK_BYTES // (8 * max(nt, 1)))
    with np.errstate(all="ignore"):
        for c0 in range(0, q.shape[0], step):
            qs = qc[c0:c0 + step]
            acc = np.zeros((qs.shape[0], nt), np.float64)
            diff = np.empty_like(acc)
            for f in range(d):
                np.subtract(gc[f][None, :], qs[:, f][:, None], out=diff)        # (g - avg) - (q - avg)
                np.multiply(diff, diff, out=diff)
                np.add(acc, diff, out=acc)                                       # acc = acc + diff * diff, two roundings
            out[c0:c0 + step] = acc / float(d)
    return out


def nearest(dist, kp):
    """(rows[nq, kp] int32, dist[nq, kp]): per query the first kp rows by (distance, row), padded with -1 / +inf where the training
    set has fewer than kp rows. The distances must not be NaN."""
    dist = np.atleast_2d(dist)
    nq, nt = dist.shape
    rows = np.full((nq, kp), -1, np.int32)
    out = np.full((nq, kp), np.inf, np.float64)
    idx = np.arange(nt)
    for i in range(nq):
        order = np.lexsort((idx, dist[i]))[:kp]
        rows[i, :len(order)] = order
        out[i, :len(order)] = dist[i, order]
    return rows, out


def vote(dist, class_off, k):
    """The walk of classification.cpp:151-160 over one query's rows in (distance, row) order; class_off[c] = first row of class c
    (num_classes + 1 entries, class-major rows). Returns (class, rows walked, tie): the class is the first with the most votes
    when the walk ends (:161-168), tie says that an equal distance occurs among the rows walked or between the deciding row and
    its successor -- the reference's unstable sort may then walk another order."""
    dist = np.asarray(dist, np.float64)
    nt = dist.shape[0]
    class_off = np.asarray(class_off)
    order = np.lexsort((np.arange(nt), dist))
    cls = np.searchsorted(class_off, order, side="right") - 1
    votes = np.zeros(len(class_off) - 1, np.int64)
    walked = 0
    for c in cls:
        votes[c] += 1
        walked += 1
        if votes[c] >= k:
            break
    ds = dist[order[:min(walked + 1, nt)]]
    tie = bool(np.any(ds[1:] == ds[:-1]))
    return int(np.argmax(votes)), walked, tie


def class_offsets(train_class, num_classes):
    """class_off of a non-decreasing class array"""
    return np.searchsorted(np.asarray(train_class), np.arange(num_classes + 1), side="left")
