"""The run-walk over uncertified queries of the matrix-core forms that answer them through an exact form (K > 8 nearest rows, rows
within a radius, distinct classes): one batch of 40 queries in which positions {0, 5, 6, 20, 21, 22, 39} carry one NaN feature --
runs of 1, 2, 3 and 1 uncertified queries, at both ends of the batch and inside it. Every key, count and class must be, bit for
bit, what the exact form of the gallery handle gives for the same batch, the state's fallback_queries counter must rise by exactly
the seven planted queries per call, and the certified queries next to each run must keep the slots the exact form gives them."""
import numpy as np
import pytest
import torch

import knn_gemm_ref as kg
import knn_select_ref as ks
import synth

pytestmark = pytest.mark.gpu

L2 = 0
DEV = torch.device("cuda", 0)
GUARD = 0x5A5A5A5A5A5A5A5A
GUARD32 = 0x5A5A5A5A
N, D, QB = 200, 64, 40                      # the smallest gallery shape test_gpu_knn_gemm.py runs through the matrix cores
PLANTED = (0, 5, 6, 20, 21, 22, 39)
NEIGHBOURS = (4, 7, 19, 23, 38)
NUM_CLASSES = 11


@pytest.fixture(scope="module")
def batch():
    rows, q = kg.case(N + D, N, D, QB)
    clean = q.copy()
    q = q.copy()
    q[list(PLANTED), 7] = np.nan
    for a in (clean, q):
        a.setflags(write=False)
    return rows, synth.make_labels(N, NUM_CLASSES), clean, q


def run(fn, qb, slots, want_count, want_classes):
    """fn(keys_ptr, count_ptr, classes_ptr) -> (keys [qb, slots], count [qb] or None, classes [qb, slots] or None); guard words behind all"""
    keys = torch.full((qb * slots + 4,), GUARD, dtype=torch.int64, device=DEV)
    count = torch.full((qb + 4,), GUARD32, dtype=torch.int32, device=DEV)
    classes = torch.full((qb * slots + 4,), GUARD32, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    fn(keys.data_ptr(), count.data_ptr(), classes.data_ptr())
    torch.cuda.synchronize()
    assert torch.all(keys[qb * slots:] == GUARD)
    assert torch.all(count[qb:] == GUARD32) and (want_count or torch.all(count == GUARD32))
    assert torch.all(classes[qb * slots:] == GUARD32) and (want_classes or torch.all(classes == GUARD32))
    return (keys[:qb * slots].cpu().numpy().view(np.uint64).reshape(qb, slots), count[:qb].cpu().numpy() if want_count else None,
            classes[:qb * slots].cpu().numpy().reshape(qb, slots) if want_classes else None)


def compare(kind, exact, gemm, before, after):
    rose = after["fallback_queries"] - before["fallback_queries"]
    print(kind, "fallback_queries rose by", rose)
    for name, e, m in zip(("keys", "count", "classes"), exact, gemm):
        if e is None:
            continue
        assert np.array_equal(m, e), (kind, name, np.nonzero((m != e).reshape(QB, -1).any(axis=1))[0])
        assert np.array_equal(m[list(NEIGHBOURS)], e[list(NEIGHBOURS)]), (kind, name)     # nothing written past a run's slots
    assert rose == len(PLANTED), (kind, before, after)


def test_knn_radius_and_classes_answer_runs_of_uncertified_queries_in_place(fir, batch):
    rows, labels, clean, q = batch
    tq = torch.from_numpy(q.copy()).to(DEV)
    with fir.Gallery(rows, labels, L2, 0) as g, fir.GemmSearch(g, fir.GemmSearch.F16) as m:
        g.set_large_batch_mfma(0)                                           # the gallery handle answers with its exact forms only
        # finite radii: a little beyond each (clean) query's fifth nearest row, so some rows lie inside and they fit max_results = 9
        dist = g.range_distances(clean)
        radius = np.nextafter(np.array([np.sort(r[ks.qualifies(r)])[4] for r in dist], np.float32), np.float32(np.inf))
        assert np.all(np.isfinite(radius))
        tr = torch.from_numpy(radius).to(DEV)

        k = 9
        exact = run(lambda kp, cp, lp: g.search_knn_keys_dev(tq.data_ptr(), QB, k, kp), QB, k, False, False)
        before = m.stats()
        gemm = run(lambda kp, cp, lp: m.search_knn_keys_dev(tq.data_ptr(), QB, k, kp), QB, k, False, False)
        compare("knn", exact, gemm, before, m.stats())

        exact = run(lambda kp, cp, lp: g.search_radius_keys_dev(tq.data_ptr(), QB, tr.data_ptr(), k, cp, kp), QB, k, True, False)
        before = m.stats()
        gemm = run(lambda kp, cp, lp: m.search_radius_keys_dev(tq.data_ptr(), QB, tr.data_ptr(), k, cp, kp), QB, k, True, False)
        compare("radius", exact, gemm, before, m.stats())
        good = [i for i in range(QB) if i not in PLANTED]
        assert np.all(gemm[1][good] >= 5) and np.all(gemm[1][list(PLANTED)] == 0)       # the case is what it says it is

        k = 3
        exact = run(lambda kp, cp, lp: g.search_top_classes_keys_dev(tq.data_ptr(), QB, NUM_CLASSES, k, kp, lp), QB, k, False, True)
        before = m.stats()
        gemm = run(lambda kp, cp, lp: m.search_top_classes_keys_dev(tq.data_ptr(), QB, NUM_CLASSES, k, kp, lp), QB, k, False, True)
        compare("classes", exact, gemm, before, m.stats())
