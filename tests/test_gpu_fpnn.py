"""GPU parity of FPNNClassifier (qt_cpp/classification.cpp:618-791): coefficients, log-scores and classes against the
REAL reference's outputs (tests/golden) and against the oracle on fresh data.

Decisions are graded exactly wherever they do not rest on a tie: tests/fpnn_walk.py gives, from the oracle alone, the
queries whose verdict no output error within OUT_RTOL / OUT_ATOL can turn ("clear"); on those the class of predict and the
(class, chunks) of predict_seq have to be the oracle's. test_fpnn_walk_formulation.py proves on the CPU that at most one
query in eight of any (case, scale, ratio) is left out that way."""
import os

import numpy as np
import pytest

import fpnn_walk as fw
import golden_cases as gc

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz"))

# The coefficients are sums of cos/sin of the device's libm (<= 2 ulp) where the reference used glibc's; each term is
# at most (J-j)/(J(J+1)) <= 0.25 in magnitude, so a few 1e-16 absolute per coefficient.
A_ATOL = 5e-15
# outputs are float sums of d fast-log terms; a last-bit difference in `probab` can move one term by one float ulp
OUT_RTOL, OUT_ATOL = fw.OUT_RTOL, fw.OUT_ATOL
FIR_ERR_ARG = -1                            # include/fir_amd.h


def golden_cases():
    x, lab, ncls = gc.cls_case()
    x2, lab2, ncls2 = gc.fpnn_case2()
    return (("fpnn", x, ncls, GOLD["cls/train"], GOLD["cls/train_class"], GOLD["cls/test"], GOLD["cls/avg"], GOLD["cls/std"]),
            ("fpnn2", x2, ncls2, GOLD["fpnn2/train"], GOLD["fpnn2/train_class"], GOLD["fpnn2/test"], GOLD["fpnn2/avg"], GOLD["fpnn2/std"]))


def test_reference_model_and_decisions_reproduced(fir):
    for tag, x, nc, train, tcls, test, avg, sd in golden_cases():
        for sc in gc.FPNN_SCALES:
            m = fir.Fpnn(x[train], tcls, nc, avg, sd, sc)
            assert m.J == int(GOLD[f"{tag}/{sc}/J"])
            a = m.model()
            ga = GOLD[f"{tag}/{sc}/a"]
            assert a.shape == ga.shape and np.max(np.abs(a - ga)) <= A_ATOL, (tag, sc, np.max(np.abs(a - ga)))
            best, _ = m.predict(x[test])
            assert np.array_equal(best, GOLD[f"{tag}/{sc}/bf"]), (tag, sc)
            for ratio in gc.FPNN_RATIOS:
                bs, _ = m.predict_seq(x[test], ratio)
                assert np.array_equal(bs, GOLD[f"{tag}/{sc}/seq_{ratio}"]), (tag, sc, ratio)
            m.close()


def _exact_on_clear(m, ref, queries, ratios, tag):
    """Outputs within the tolerance; predict's class and predict_seq's (class, chunks) the oracle's on every clear query.
    -> (best, outs, {ratio: (classes, chunks)})"""
    best, outs = m.predict(queries)
    assert outs.shape == ref.bf_outputs.shape
    for i in range(len(queries)):
        assert np.allclose(outs[i], ref.bf_outputs[i], rtol=OUT_RTOL, atol=OUT_ATOL), (tag, i)
    same = int(np.sum(outs.view(np.uint32) == ref.bf_outputs.view(np.uint32)))
    print(f"fpnn {tag}: {same}/{outs.size} predict outputs bit-equal to the oracle's, max |diff| {np.max(np.abs(outs - ref.bf_outputs)):.3g}; "
          f"predict not clear {int(np.sum(~ref.bf_clear))}/{len(queries)}")
    clear = ref.bf_clear
    assert np.array_equal(best[clear], ref.bf_class[clear]), (tag, np.nonzero(clear & (best != ref.bf_class))[0])
    seq = {}
    for ratio in ratios:
        bs, chunks = m.predict_seq(queries, ratio)
        ec, en = ref.seq[ratio]
        clear = ref.seq_clear(ratio)
        bad = np.nonzero(clear & ((bs != ec) | (chunks != en)))[0]
        print(f"fpnn {tag} ratio={ratio}: not clear {int(np.sum(~clear))}/{len(queries)}, of those {int(np.sum(~clear & ((bs != ec) | (chunks != en))))} differ")
        assert bad.size == 0, (tag, ratio, bad, bs[bad], ec[bad], chunks[bad], en[bad])
        seq[ratio] = (bs, chunks)
    return best, outs, seq


@pytest.mark.parametrize("seed,n,d,ncls,per_class", [c[:5] for c in fw.OLD_CASES])
def test_matches_oracle_on_fresh_data(fir, oracle, seed, n, d, ncls, per_class):
    x, train, tcls, test, avg, sd = fw.case_data(oracle, seed, n, d, ncls, per_class)
    ratios = (0.9, 0.99, 0.5)
    for sc in fw.SCALES:
        ref = fw.reference(oracle, seed, x[train], tcls, ncls, avg, sd, sc, x[test], ratios)
        m = fir.Fpnn(x[train], tcls, ncls, avg, sd, sc)
        assert m.J == ref.J
        a = m.model()
        print(f"fpnn {(seed, sc)}: largest coefficient difference {np.max(np.abs(a - ref.a)):.3g} (A_ATOL {A_ATOL})")
        assert np.max(np.abs(a - ref.a)) <= A_ATOL
        best, _, seq = _exact_on_clear(m, ref, x[test], ratios, (seed, sc))
        for i in range(test.size):
            e = ref.bf_outputs[i]
            gap = np.sort(e)[-1] - np.sort(e)[-2]
            if gap > 2 * OUT_ATOL:                             # away from a score tie the class is the reference's
                assert best[i] == ref.bf_class[i], (sc, i)
        assert np.mean(best == ref.bf_class) > 0.98
        for ratio in ratios:
            bs, chunks = seq[ratio]
            agree = np.mean((bs == ref.seq[ratio][0]) & (chunks == ref.seq[ratio][1]))
            assert agree > 0.97, (sc, ratio, agree)            # a pruning decision can sit on a threshold tie
        m.close()


@pytest.mark.parametrize("seed,n,d,ncls,per_class,ratios", fw.NEW_CASES)
def test_many_classes_match_oracle(fir, oracle, seed, n, d, ncls, per_class, ratios):
    """More classes than fit the LDS stage of a whole 32-feature chunk: k_fpnn_predict adds a chunk in ragged sub-stages of
    nsub = 20, 3 and 1 features, the class loops make several strides and k_fpnn_terms runs with one feature per workgroup.
    C = 6826 is the documented limit and asks for the largest LDS block."""
    x, train, tcls, test, avg, sd = fw.case_data(oracle, seed, n, d, ncls, per_class)
    nchunks = (d + fw.CHUNK - 1) // fw.CHUNK
    for sc in fw.SCALES:
        ref = fw.reference(oracle, seed, x[train], tcls, ncls, avg, sd, sc, x[test], ratios)
        m = fir.Fpnn(x[train], tcls, ncls, avg, sd, sc)
        assert m.J == ref.J
        a = m.model()
        print(f"fpnn {(seed, sc)}: largest coefficient difference {np.max(np.abs(a - ref.a)):.3g} (A_ATOL {A_ATOL})")
        assert np.max(np.abs(a - ref.a)) <= A_ATOL, (sc, np.max(np.abs(a - ref.a)))
        _, _, seq = _exact_on_clear(m, ref, x[test], ratios, (seed, sc))
        chunks = seq[0.99][1]
        assert np.any(chunks == 1) and np.any(chunks == nchunks), (sc, np.bincount(chunks))    # the early exit and the whole walk both ran
        m.close()


def coefficient_bound(J, d, class_sizes):
    """Worst-case |device - reference| per coefficient, shaped like the model: [d][C][2J+1].

    Coefficient (c, j) is a sum of n_c terms trig(PI (j+1) val) * (1/n_c) * (J-j) / (J (J+1)), each at most w / n_c in
    magnitude with w = (J-j)/(J(J+1)), added in the same order on both sides. Every partial sum is at most w, so each of
    the n_c additions rounds by at most 2^-53 w on either side: n_c * 2^-52 w in all. A term itself differs by the trig
    functions' difference (the device's are within 2 ulp, of a value <= 1) carried through the term's three roundings (two
    products and a quotient): roughly 3 * 2^-52 * w / n_c per term, so 3 * 2^-52 w over the n_c terms.
    Together (n_c + 3) * 2^-52 * w. The constant a0 = 0.5 is stored, not computed: its bound is 0."""
    K = 2 * J + 1
    w = np.zeros(K)
    for j in range(J):
        w[2 * j + 1] = w[2 * j + 2] = (J - j) / (J * (J + 1))
    nc = np.asarray(class_sizes, np.float64)
    return np.broadcast_to((nc[:, None] + 3) * 2.0 ** -52 * w[None, :], (d, nc.size, K)).reshape(-1)


def _model_within_bound(a, ea, J, d, class_sizes, tag):
    diff, bound = np.abs(a - ea), coefficient_bound(J, d, class_sizes)
    k = int(np.argmax(diff))
    print(f"fpnn {tag}: largest coefficient difference {diff[k]:.3g} (its bound {bound[k]:.3g}); largest difference / bound "
          f"{np.max(diff[bound > 0] / bound[bound > 0]):.3g}")
    assert np.all(diff <= bound), (tag, k, diff[k], bound[k])


def test_thirteen_harmonics_unequal_and_empty_classes(fir, oracle):
    """J = 13 (the angle-addition recurrence and the (J-j)/(J(J+1)) weights beyond 4 harmonics), classes of 3400, 0, 300
    and 3500 training rows: cur_mult differs per class and is 1/0, never used, for the empty one. Every query is clear."""
    x, train, tcls, test, avg, sd = fw.unequal_case(oracle)
    ratios = (0.9, 0.99)
    ref = fw.reference(oracle, 86, x[train], tcls, 4, avg, sd, 1.0, x[test], ratios)
    m = fir.Fpnn(x[train], tcls, 4, avg, sd, 1.0)
    assert m.J == ref.J == 13
    _model_within_bound(m.model(), ref.a, 13, 37, np.bincount(tcls, minlength=4), "J=13")
    assert ref.bf_clear.all() and all(ref.seq_clear(r).all() for r in ratios)
    _exact_on_clear(m, ref, x[test], ratios, "J=13")
    m.close()


def test_sixty_four_harmonics(fir, oracle):
    """kMaxJ = 64: 250100 rows of one class and one feature."""
    x = np.random.default_rng(5).standard_normal((250120, 1))
    rows, queries = x[:250100], x[250100:]
    tcls = np.zeros(250100, np.int32)
    _, _, avg, sd = oracle.train_stats(rows)
    ref = fw.reference(oracle, "J64", rows, tcls, 1, avg, sd, 1.0, queries, (0.9,))
    m = fir.Fpnn(rows, tcls, 1, avg, sd, 1.0)
    assert m.J == ref.J == 64
    _model_within_bound(m.model(), ref.a, 64, 1, [250100], "J=64")
    best, _, seq = _exact_on_clear(m, ref, queries, (0.9,), "J=64")
    assert np.all(best == 0) and np.all(seq[0.9][0] == 0) and np.all(seq[0.9][1] == 1)
    m.close()


def test_one_query_calls_and_batch_edges(fir, oracle):
    """One handle: one-query calls (the ticket word in pinned memory instead of a stream synchronisation; four of them,
    so tickets 1 to 4), exactly one internal batch of 64, one more than it, and a one-query call after a multi-query one. No term
    depends on the batch, so every result is bit-identical to the same rows of one 70-query call on a fresh handle."""
    seed, n, d, ncls, per_class, _ = fw.OLD_CASES[0]
    assert seed == 71
    x, train, tcls, test, avg, sd = fw.case_data(oracle, seed, n, d, ncls, per_class)
    q, ratio = x[test], 0.99
    fresh = fir.Fpnn(x[train], tcls, ncls, avg, sd, 1.0)
    best, outs = fresh.predict(q)
    sbest, schunks = fresh.predict_seq(q, ratio)
    fresh.close()
    assert np.unique(schunks).size > 1                        # the rows compared below stop at different chunks
    m = fir.Fpnn(x[train], tcls, ncls, avg, sd, 1.0)

    def same_bf(lo, hi):
        b, o = m.predict(q[lo:hi])
        assert np.array_equal(b, best[lo:hi]) and np.array_equal(o.view(np.uint32), outs[lo:hi].view(np.uint32)), (lo, hi)

    def same_seq(lo, hi):
        b, c = m.predict_seq(q[lo:hi], ratio)
        assert np.array_equal(b, sbest[lo:hi]) and np.array_equal(c, schunks[lo:hi]), (lo, hi, b, c)

    same_bf(0, 1)
    same_seq(0, 1)
    same_bf(0, 64)
    same_bf(5, 6)
    same_seq(0, 65)
    same_seq(69, 70)
    m.close()


def test_argument_limits(fir):
    """More classes than the LDS score table holds, and more rows per class than kMaxJ harmonics serve, are refused; a
    valid handle trains and predicts after each refusal."""
    x, lab, ncls = gc.cls_case(seed=75, n=60, d=16, n_classes=3)
    order = np.argsort(lab, kind="stable")
    avg, sd = x.mean(0), x.std(0)

    def still_works():
        m = fir.Fpnn(x[order], lab[order], ncls, avg, sd)
        best, outs = m.predict(x[:5])
        assert best.shape == (5,) and np.all((best >= 0) & (best < ncls)) and np.all(np.isfinite(outs))
        bs, chunks = m.predict_seq(x[:1])
        assert 0 <= bs[0] < ncls and chunks[0] == 1
        m.close()
        return best, outs

    first = still_works()
    one = np.ones(1)
    with pytest.raises(fir.FirError) as e:
        fir.Fpnn(np.zeros((6827, 1)), np.arange(6827, dtype=np.int32), 6827, one, one)
    assert e.value.code == FIR_ERR_ARG
    again = still_works()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    with pytest.raises(fir.FirError) as e:
        fir.Fpnn(np.zeros((262145, 1)), np.zeros(262145, np.int32), 1, one, one)          # J would be 65
    assert e.value.code == FIR_ERR_ARG
    again = still_works()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    m = fir.Fpnn(np.zeros((6826, 1)), np.arange(6826, dtype=np.int32), 6826, one, one)   # the limit itself is served
    assert m.J == 3
    m.close()


def test_argument_errors(fir):
    x, lab, ncls = gc.cls_case(seed=75, n=60, d=16, n_classes=3)
    order = np.argsort(lab, kind="stable")
    avg, sd = x.mean(0), x.std(0)
    with pytest.raises(fir.FirError):
        fir.Fpnn(x, lab, ncls, avg, sd)                        # classes not grouped
    with pytest.raises(fir.FirError):
        fir.Fpnn(x[order], lab[order], 2, avg, sd)             # label outside [0, C)
    m = fir.Fpnn(x[order], lab[order], ncls, avg, sd)
    best, outs = m.predict(np.empty((0, 16)))
    assert best.size == 0 and outs.shape == (0, ncls)
    m.close()
