"""The two three-way-decision classifiers as functions of a DISTANCE TABLE, not of rows: what oracle/oracle.c:134-229
(orc_twd_conventional, orc_twd_proposed) does with the float distances once it has them. Plain Python and numpy, no GPU.

Order and precision are the oracle's: every float distance is widened to double before anything else happens to it, the
running sums and the comparisons are double, a running minimum starts at 100000 and is replaced under strict `<` in row
order (a NaN is never smaller), the posteriors come from libm's exp (math.exp -- numpy's vectorised exp need not be libm's),
and the second-stage tail `distance * (256 - reduced)` is a FLOAT product (float * int, oracle.c:176).

tests/test_twd_walk_formulation.py proves walk(oracle's tables) == oracle, integer for integer; that entitles
tests/test_gpu_subrange_scans.py to grade the device's KL verdicts as walk(device's tables), with the tolerance on the tables."""
import math

import numpy as np

import golden_cases as gc
import synth

START = 100000.0
LAST_FEATURE = 256
DIST_WEIGHT = 100
MAX_PROBABS_COUNT = 5


def case(seed, n, ncls, metric, nq):
    """golden_cases.twd_case with nq queries (its generator, so the first twelve are its queries), made positive for chi-square
    and KL the way test_gpu_twd_forms.metric_case does; the last three queries sit next to rows 1, n // 2 and n - 1."""
    rows, cls, _, _ = gc.twd_case(seed=seed, n=n, d=LAST_FEATURE, n_classes=ncls)
    q, _ = synth.make_queries(seed, rows, nq, gc.L2, noise=0.4)
    if metric != gc.L2:
        rows = np.abs(rows) + np.float32(1e-3)
        q = np.abs(q) + np.float32(1e-3)
    q[nq - 3:] = q[nq - 3:] * np.float32(0.05) + rows[[1, n // 2, n - 1]] * np.float32(0.95)
    return rows, cls, q


def _first_min_below(dist, bound):
    """(index, value) of the first smallest entry strictly below `bound`, (-1, bound) when there is none: the row a strict `<`
    running minimum from `bound` ends at. NaN entries never qualify."""
    ok = dist < bound
    if not ok.any():
        return -1, bound
    j = int(np.argmin(np.where(ok, dist, np.inf)))
    return j, float(dist[j])


def proposed(sub, cls, th):
    """sub[ci][row]: float distance of the row over chunk ci, for every chunk of [0, 256). -> (class, unreliable, chunks)"""
    sub = np.asarray(sub, np.float32)
    cls = np.asarray(cls)
    n = sub.shape[1]
    threshold = 1.0 / th
    best = -1
    dist = np.zeros(n, np.float64)
    alive = np.ones(n, bool)
    unreliable = chunks = 0
    for ci in range(sub.shape[0]):
        chunks += 1
        dist[alive] += sub[ci, alive].astype(np.float64)
        j, best_dist = _first_min_below(np.where(alive, dist, np.nan), START)
        if j >= 0:
            best = j                                          # (bestInd outlives the chunk, bestDist does not: oracle.c:194,201)
        limit = best_dist * threshold
        pruned = alive & (dist > limit)                       # (a NaN sum is not above the limit: the row stays)
        alive &= ~pruned
        # one for the best class, one for every surviving ROW of another class; no best row yet: every class is another one
        variants = 1 + int((alive & (cls != cls[best])).sum() if best >= 0 else alive.sum())
        if variants == 1:
            break
        if ci == 0:
            unreliable += 1
    return (int(cls[best]) if best >= 0 else -1), unreliable, chunks


def _records(dist):
    """Rows at which a strict `<` running minimum from 100000 is replaced, in row order."""
    clean = np.where(np.isnan(dist), np.inf, dist)
    before = np.minimum(START, np.concatenate(([np.inf], np.minimum.accumulate(clean)[:-1])))
    return np.flatnonzero(dist < before)


def conventional(d1, d2, cls, num_classes, typ, threshold, reduced):
    """d1[row] / d2[row]: float distances over [0, reduced) / [reduced, 256). -> (class, unreliable, margin); margin is
    |max_probab / sum - threshold| / threshold for typ 0 (how far the posterior test is from its threshold), None otherwise."""
    cls = np.asarray(cls)
    dist = np.asarray(d1, np.float32).astype(np.float64)
    best, best_dist, second = -1, START, START
    for j in _records(dist).tolist():
        if best != -1 and cls[best] != cls[j]:
            second = best_dist
        best_dist, best = float(dist[j]), j
    margin = None
    if typ == 0:
        probabs = [0.0] * max(num_classes, MAX_PROBABS_COUNT)
        for c, x in zip(cls.tolist(), dist.tolist()):
            p = math.exp(-x * DIST_WEIGHT)
            if p > probabs[c]:
                probabs[c] = p
        max_probab = math.exp(-best_dist * DIST_WEIGHT) if best >= 0 else 0.0
        probabs[:num_classes] = sorted(probabs[:num_classes], reverse=True)
        total = 0.0
        for p in probabs[:MAX_PROBABS_COUNT]:
            total += p
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.float64(max_probab) / np.float64(total))
        reliable = ratio > threshold
        margin = abs(ratio - threshold) / threshold
    elif typ == 1:
        reliable = (second - best_dist) > threshold
    else:
        reliable = (best_dist / second) < threshold
    if not reliable:
        tail = np.asarray(d2, np.float32) * np.float32(LAST_FEATURE - reduced)            # float * int -> float
        full = (dist * reduced + tail.astype(np.float64)) / LAST_FEATURE
        best, _ = _first_min_below(full, START)
    return (int(cls[best]) if best >= 0 else -1), int(not reliable), margin
