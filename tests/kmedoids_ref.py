"""numpy restatement of the table formulation of PNNwithClusteringClassifier::train (classification.cpp:320-388) that
fir_cls_kmedoids states in include/fir_amd.h: one n x n table of mean squared distances per class, then assign / update
steps on the medoid vector, optionally stopping at the first step that leaves it unchanged."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def pair_table(rows):
    """T[t][t1] = (sum_f (rows[t1][f] - rows[t][f])^2, added in feature order) / d -- fir_cls_distance_sums / d with
    query = row t. np.add.accumulate adds one feature at a time, in order."""
    r = np.ascontiguousarray(rows, np.float64)
    n, d = r.shape
    t = np.empty((n, n), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            diff = r - r[i]
            sq = diff * diff
            t[i] = np.add.accumulate(sq, axis=1)[:, -1] / np.float64(d)
    return t


def cluster_table(table, num_clusters, steps=100, early=True):
    """-> (live medoids in cluster order, steps computed). table: pair_table of the class."""
    n = table.shape[0]
    k = int(num_clusters)
    if n <= k:
        return np.arange(n, dtype=np.int32), 0
    med = list(range(k))
    run = 0
    for _ in range(steps):
        assign = np.full(n, -1, np.int64)
        best = np.full(n, DBL_MAX)
        for c in range(k):
            if med[c] < 0:
                continue
            with np.errstate(invalid="ignore"):
                take = table[med[c]] < best              # strict: the first cluster keeps a tie; NaN never qualifies
            best[take] = table[med[c]][take]
            assign[take] = c
        new = []
        for c in range(k):
            members = np.nonzero(assign == c)[0]
            m = -1
            if members.size:
                with np.errstate(invalid="ignore", over="ignore"):
                    sums = np.add.accumulate(table[np.ix_(members, members)], axis=1)[:, -1]   # plain double sum in ascending t1
                    ok = sums < DBL_MAX
                if ok.any():
                    m = int(members[np.argmin(np.where(ok, sums, np.inf))])                     # the first strict minimum
            new.append(m)
        run += 1
        same = new == med
        med = new
        if early and same:
            break
    return np.array([m for m in med if m >= 0], np.int32), run


def cluster_class(rows, num_clusters, steps=100, early=True):
    return cluster_table(pair_table(rows), num_clusters, steps, early)


def cluster_train(train_rows, class_off, num_clusters, steps=100, early=True):
    """What ClsModel.kmedoids returns for rows already centred (rows - avg): (rows[num_classes, K] -1 padded, count, steps)."""
    nc = len(class_off) - 1
    rows = np.full((nc, num_clusters), -1, np.int32)
    count = np.zeros(nc, np.int32)
    run = np.zeros(nc, np.int32)
    for i in range(nc):
        r0, r1 = int(class_off[i]), int(class_off[i + 1])
        med, run[i] = cluster_class(train_rows[r0:r1], num_clusters, steps, early)
        count[i] = med.size
        rows[i, : med.size] = r0 + med
    return rows, count, run
