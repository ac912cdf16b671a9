"""FPNNClassifier::predict_sequentional (qt_cpp/classification.cpp:736-791) re-walked from the oracle's brute-force
outputs on feature prefixes, with the margin every comparison of the walk was decided by -- for the tests of
fir_fpnn_predict / fir_fpnn_predict_seq (test_fpnn_walk_formulation.py proves the walk, test_gpu_fpnn.py uses it).

The model is feature-major (a[(f*C + c)*(2J+1) + k]), so a[:m*C*(2J+1)] with avg[:m], sd[:m], q[:m] is the model of the
first m features and one predict_bf call on it gives every class's float sum after m features. A class that is still
checked at chunk end m has added exactly those terms in that order, so the prefix value is its sum bit for bit; a
dropped class keeps the sum it had when it was dropped (:758).

A query is CLEAR when no comparison its verdict rests on -- a class against the pruning threshold at any chunk walked, or
the best class against the runner-up -- can be turned by an error within the output tolerance of the GPU tests. On clear
queries the device's (class, chunks) have to be the oracle's exactly.

The cases, their data recipe and a per-process cache of the oracle's answers are here too, so that the CPU test and the
GPU tests judge the same queries and the reference is computed once."""
import numpy as np

import golden_cases as gc

CHUNK = 32                                  # PNNClassifier::delta_features_count, classification.cpp:182
# outputs are float sums of d fast-log terms; a last-bit difference in `probab` can move one term by one float ulp
OUT_RTOL, OUT_ATOL = 2e-6, 1e-4

SCALES = (1.0, 0.33, 4.0)                   # 4.0 drives many values into the +-0.5 clamp
# (seed, n, d, classes, training rows per class, output ratios)
OLD_CASES = ((71, 900, 256, 30, 20, (0.9, 0.99, 0.5)), (72, 400, 33, 5, 64, (0.9, 0.99, 0.5)),
             (73, 3000, 64, 300, 5, (0.9, 0.99, 0.5)), (74, 130, 200, 2, 50, (0.9, 0.99, 0.5)))
# nsub = features staged in LDS at a time by k_fpnn_predict = min(32, (60 KiB - 5 C) / (4 C))
NEW_CASES = ((81, 2200, 72, 700, 3, (0.9, 0.99, 0.5)),     # nsub = 20: chunks staged 20 + 12, the last chunk 8; three class strides
             (82, 6200, 70, 3000, 2, (0.99, 0.5)),         # nsub = 3: 3 + 3 + ... + 2   (ratio 0.9: 13 / 70 not clear)
             (85, 14000, 70, 6826, 2, (0.99, 0.5)))        # nsub = 1, the largest LDS request, the documented class limit
MAX_UNCLEAR = 1.0 / 8                       # share of a (case, scale, ratio)'s queries that may be left out as not clear


def tolerance(outputs):
    """What one comparison between two sums may be off by: each side moves by at most the output tolerance."""
    return 2.0 * (OUT_ATOL + OUT_RTOL * float(np.max(np.abs(outputs))))


def _gap(values):
    """top1 - top2 (inf for a single value)"""
    if values.size < 2:
        return np.inf
    s = np.partition(values.astype(np.float64), values.size - 2)
    return float(s[-1] - s[-2])


def bf_margin(outputs):
    return _gap(np.asarray(outputs)) / tolerance(outputs)


def clear_bf(outputs):
    """predict's class does not depend on an output error within the tolerance"""
    return bf_margin(outputs) > 1.0


def prefix_outputs(oracle, a, J, C, avg, sd, scale, q):
    """[(m, float sums of every class after the first m features)] for every chunk end m = 32, 64, ..., d"""
    d, K = q.size, 2 * J + 1
    ends = list(range(CHUNK, d, CHUNK)) + [d]
    return [(m, oracle.fpnn_predict(a[:m * C * K], J, C, avg[:m], sd[:m], scale, q[:m])[1]) for m in ends]


def walk(oracle, a, J, C, avg, sd, scale, q, ratio, prefix=None):
    """-> (best_class, chunks, margin). `prefix`: prefix_outputs() of the same query (it does not depend on the ratio)."""
    if prefix is None:
        prefix = prefix_outputs(oracle, a, J, C, avg, sd, scale, q)
    delta = np.float32(oracle.fastlog(ratio))                  # the constructor's fastlog(output_ratio), :621
    outputs = np.zeros(C, np.float32)
    checked = np.ones(C, bool)
    best, chunks, margin = -1, 0, np.inf
    for m, pref in prefix:
        chunks += 1
        outputs[checked] = pref[checked]
        cand = np.where(checked, outputs, -np.inf)
        best = int(np.argmax(cand))                            # first maximum among the checked classes (:770-776)
        threshold = np.float32(outputs[best] + np.float32(delta * np.float32(m)))    # :778
        tol = tolerance(outputs)
        margin = min(margin, float(np.min(np.abs(outputs.astype(np.float64) - float(threshold)))) / tol)
        last_gap = _gap(outputs[checked]) / tol
        keep = ~(outputs < threshold)                          # :780-785: every class is tested and counted,
        checked &= keep                                        # dropped ones are never revived
        if int(keep.sum()) == 1:
            break
    return best, chunks, min(margin, last_gap)


def case_data(oracle, seed, n, d, ncls, per_class):
    """-> (x, train rows, their classes, query rows, avg, sd): the first per_class rows of each class train, the next 3
    per class (cut to 70: more than one internal batch of 64) are queries, one feature is constant."""
    x, lab, _ = gc.cls_case(seed=seed, n=n, d=d, n_classes=ncls)
    train = np.concatenate([np.nonzero(lab == c)[0][:per_class] for c in range(ncls)])
    test = np.concatenate([np.nonzero(lab == c)[0][per_class:per_class + 3] for c in range(ncls)])[:70]
    _, _, avg, sd = oracle.train_stats(x[train])
    sd[d // 2] = 0.0                                           # a constant feature: normalize() maps it to 0 (:647)
    return x, train, lab[train], test, avg, sd


def unequal_case(oracle):
    """J = 13, classes of 3400, 0 (empty: cur_mult = 1/0 is never used), 300 and 3500 rows; the last 10 rows of each
    class are the queries. -> like case_data()"""
    x, lab, ncls = gc.cls_case(seed=86, n=15000, d=37, n_classes=4)
    rows = [np.nonzero(lab == c)[0] for c in range(ncls)]
    train = np.concatenate([rows[0][:3400], rows[1][:0], rows[2][:300], rows[3][:3500]])
    test = np.concatenate([r[-10:] for r in rows])
    _, _, avg, sd = oracle.train_stats(x[train])
    sd[37 // 2] = 0.0
    return x, train, lab[train], test, avg, sd


class Reference:
    """The oracle's answers for one (training set, scale) and a set of queries; read-only."""

    def __init__(self, oracle, rows, tcls, ncls, avg, sd, scale, queries, ratios):
        self.J, self.a = oracle.fpnn_train(rows, tcls, ncls, avg, sd, scale)
        bf = [oracle.fpnn_predict(self.a, self.J, ncls, avg, sd, scale, q) for q in queries]
        self.bf_class = np.array([e[0] for e in bf], np.int32)
        self.bf_outputs = np.stack([e[1] for e in bf])
        self.bf_clear = np.array([clear_bf(o) for o in self.bf_outputs])
        prefix = [prefix_outputs(oracle, self.a, self.J, ncls, avg, sd, scale, q) for q in queries]
        self.seq, self.walk = {}, {}
        for ratio in ratios:
            es = [oracle.fpnn_predict(self.a, self.J, ncls, avg, sd, scale, q, True, ratio) for q in queries]
            self.seq[ratio] = (np.array([e[0] for e in es], np.int32), np.array([e[2] for e in es], np.int32))
            w = [walk(oracle, self.a, self.J, ncls, avg, sd, scale, q, ratio, p) for q, p in zip(queries, prefix)]
            self.walk[ratio] = (np.array([e[0] for e in w], np.int32), np.array([e[1] for e in w], np.int32), np.array([e[2] for e in w]))
        for arr in [self.a, self.bf_class, self.bf_outputs, self.bf_clear] + [v for t in list(self.seq.values()) + list(self.walk.values()) for v in t]:
            arr.setflags(write=False)

    def seq_clear(self, ratio):
        return self.walk[ratio][2] > 1.0


_cache = {}


def reference(oracle, key, rows, tcls, ncls, avg, sd, scale, queries, ratios):
    """Reference of (key, scale), computed once per process."""
    k = (key, scale, tuple(ratios))
    if k not in _cache:
        _cache[k] = Reference(oracle, rows, tcls, ncls, avg, sd, scale, queries, ratios)
    return _cache[k]
