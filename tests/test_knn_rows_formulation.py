"""knn_rows_ref.py against the oracle's KNNClassifier::predict on the CPU: mean_distances gives the oracle's distance vector bit for
bit, vote its class for k = 1, 3, 5 wherever the walk meets no equal distances -- small sets, among them one feature, odd row
lengths, more features than a register tile, and a duplicated row (whose queries carry the tie flag)."""
import numpy as np
import pytest

import knn_rows_ref as ref

# (nt, d, classes, duplicated row)
SETS = [(40, 1, 3, False), (300, 33, 7, False), (257, 129, 5, False), (64, 8, 64, False), (100, 6145, 4, False), (120, 7, 6, True)]


def make(nt, d, ncls, dup, nq=12):
    rng = np.random.default_rng(1000 * nt + d)
    tcls = np.sort(rng.integers(0, ncls, nt)).astype(np.int32)
    tcls[0], tcls[-1] = 0, ncls - 1
    centres = rng.random((ncls, d))
    tr = centres[tcls] + 0.2 * rng.standard_normal((nt, d))
    if dup:
        tr[nt - 3] = tr[2]                      # the same row in the first and in the last class
    q = centres[rng.integers(0, ncls, nq)] + 0.2 * rng.standard_normal((nq, d))
    q[0] = tr[2]
    q[1] = tr.mean(0)
    return tr, tcls, q


@pytest.mark.parametrize("nt,d,ncls,dup", SETS)
def test_distances_and_votes_are_the_oracles(oracle, nt, d, ncls, dup):
    tr, tcls, q = make(nt, d, ncls, dup)
    _, _, avg, _ = oracle.train_stats(tr)
    dist = ref.mean_distances(tr, avg, q)
    off = ref.class_offsets(tcls, ncls)
    graded = 0
    for i in range(len(q)):
        want = {k: oracle.knn_predict(tr, tcls, avg, ncls, q[i], k) for k in (1, 3, 5)}
        assert dist[i].tobytes() == want[1][1].tobytes(), (i, np.nonzero(dist[i] != want[1][1])[0][:4])
        for k in (1, 3, 5):
            cls, walked, tie = ref.vote(dist[i], off, k)
            assert 1 <= walked <= nt
            if not tie:
                assert cls == want[k][0], (i, k, cls, want[k][0])
                graded += 1
    if dup:
        assert all(ref.vote(dist[0], off, k)[2] for k in (1, 3, 5))      # the query that IS the duplicated row: two rows at distance 0
        assert graded >= 2 * len(q), graded                     # (a longer walk of another query may meet both copies too)
    else:
        assert graded == 3 * len(q), graded                     # no equal distances anywhere: every query is graded


def test_nearest_orders_by_distance_then_row_and_pads():
    dist = np.array([[3.0, 1.0, 1.0, 0.5], [2.0, 2.0, 2.0, 2.0]])
    rows, dd = ref.nearest(dist, 3)
    assert rows.tolist() == [[3, 1, 2], [0, 1, 2]] and dd.tolist() == [[0.5, 1.0, 1.0], [2.0, 2.0, 2.0]]
    rows, dd = ref.nearest(dist[:, :2], 8)
    assert rows[0].tolist() == [1, 0] + [-1] * 6 and np.all(np.isinf(dd[:, 2:])) and dd[0, :2].tolist() == [1.0, 3.0]


def test_vote_walks_until_one_class_has_k_rows():
    #       rows 0-2: class 0      3-5: class 1       6: class 2
    dist = np.array([0.9, 0.1, 0.8, 0.2, 0.3, 0.7, 0.05])
    off = np.array([0, 3, 6, 7])
    assert ref.vote(dist, off, 1) == (2, 1, False)              # row 6
    assert ref.vote(dist, off, 2) == (1, 4, False)              # 6, 1, 3, 4: class 1 has two
    assert ref.vote(dist, off, 3) == (1, 5, False)              # 6, 1, 3, 4, 5: class 1 has three
    dist[4] = 0.2
    assert ref.vote(dist, off, 2) == (1, 4, True)               # rows 3 and 4 at the same distance
    assert ref.vote(np.array([1.0, 2.0, 3.0]), np.array([0, 1, 2, 3]), 2) == (0, 3, False)   # nobody reaches K: the first of the most
