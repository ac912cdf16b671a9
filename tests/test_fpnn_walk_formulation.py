"""tests/fpnn_walk.py against the oracle's literal predict_sequentional (classification.cpp:736-791), for every case, scale
and ratio test_gpu_fpnn.py uses: the walk over feature prefixes gives the oracle's (class, chunks) for every query, and
the queries it calls not clear -- the only ones the GPU tests do not hold to the oracle exactly -- are at most one in
eight of every (case, scale, ratio). Both are facts of the oracle alone, so the GPU tests cannot hide a wrong kernel
behind "not clear"."""
import numpy as np
import pytest

import fpnn_walk as fw


def _check(ref, ratios, tag, all_clear=False):
    n = ref.bf_class.size
    limit = 0 if all_clear else int(n * fw.MAX_UNCLEAR)
    assert int(np.sum(~ref.bf_clear)) <= limit, (tag, "bf", int(np.sum(~ref.bf_clear)))
    for ratio in ratios:
        wc, wn, _ = ref.walk[ratio]
        ec, en = ref.seq[ratio]
        assert np.array_equal(wc, ec) and np.array_equal(wn, en), (tag, ratio)
        unclear = int(np.sum(~ref.seq_clear(ratio)))
        print(f"fpnn_walk {tag} ratio={ratio}: not clear {unclear}/{n} (bf {int(np.sum(~ref.bf_clear))}/{n})")
        assert unclear <= limit, (tag, ratio, unclear)


@pytest.mark.parametrize("seed,n,d,ncls,per_class,ratios", fw.OLD_CASES + fw.NEW_CASES)
def test_walk_equals_the_oracle_and_most_queries_are_clear(oracle, seed, n, d, ncls, per_class, ratios):
    x, train, tcls, test, avg, sd = fw.case_data(oracle, seed, n, d, ncls, per_class)
    assert test.size == min(70, 3 * ncls)
    nchunks = (d + fw.CHUNK - 1) // fw.CHUNK
    for sc in fw.SCALES:
        ref = fw.reference(oracle, seed, x[train], tcls, ncls, avg, sd, sc, x[test], ratios)
        _check(ref, ratios, (seed, sc))
        if (seed, n, d, ncls, per_class, ratios) in fw.NEW_CASES:      # what the GPU test asserts of the device's chunk counts
            en = ref.seq[0.99][1]
            assert np.any(en == 1) and np.any(en == nchunks), (seed, sc, np.bincount(en))


def test_unequal_classes_all_clear(oracle):
    x, train, tcls, test, avg, sd = fw.unequal_case(oracle)
    assert train.size == 7200 and test.size == 40 and np.array_equal(np.bincount(tcls, minlength=4), [3400, 0, 300, 3500])
    ref = fw.reference(oracle, 86, x[train], tcls, 4, avg, sd, 1.0, x[test], (0.9, 0.99))
    assert ref.J == 13
    _check(ref, (0.9, 0.99), 86, all_clear=True)
