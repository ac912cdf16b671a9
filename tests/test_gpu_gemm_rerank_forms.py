"""The exact re-rank behind every matrix-core search form (k_gemm_rerank<1>, k_gemm_rerank<kTopKMax>, k_gemm_rerank_classes, and
the few-query form's k_gemm_rerank<1>; fir_gemm_rerank.h holds what they share), aimed at the seams of that shared code: the LDS
group of 8 candidate rows, the batch of 64 list entries, the two row sources (row-major shadow / tiled gallery) and rows that are
not whole float4s. The float64 re-rank, k_gemm_rerank_f64 (fir_gemm_f64.h), shares the window, the walk and the certificate but has
its own K'-best merge and is not reached from here: test_gpu_knn_rows.py tests it, with the same seams (case C there).

Six queries are rows of the gallery that exist 1, 8, 9, 64, 65 and 200 times: every copy has the same proxy, so exactly that many
list entries lie inside the query's rounding window -- one candidate, one full LDS group, a group plus one, one full batch, a
batch plus one, several batches. 2999 rows: no multiple of 32 or 64. The expected keys are the exact scan's, bit for bit, and no
query may reach the second pass or the exact device scan, which would hide a broken re-rank (the CPU emulation of the pass,
gemm_f16_form.Form(rows, 2).emulate + certificate, certifies all 40 queries of this input for k = 1, 5, 8 with a margin of at
least 4.9e-6 in distance units and lists of at most 200 entries).

FIR_GEMM_ROWMAJOR picks the row source when a matrix-core state is created. Gallery.memory_bytes() reports the gallery's OWN
state, so each mode first sends one routed call through a fresh one -- created by the same constructor under the same knob as the
GemmSearch that follows -- and checks its shadow copy there."""
import numpy as np
import pytest
import torch

import synth
from test_gpu_class_rank_gemm import both, same

pytestmark = pytest.mark.gpu

L2 = 0
N, QB, NC = 2999, 40, 37
COPIES = (1, 8, 9, 64, 65, 200)
DEV = torch.device("cuda", 0)


def copies_of(d):
    """per special query j: the rows that hold its vector, ascending (row 3 + 7 j and COPIES[j] - 1 others)"""
    perm = np.random.default_rng(11 + d).permutation(np.arange(64, N))
    out, at = [], 0
    for j, c in enumerate(COPIES):
        out.append(np.sort(np.concatenate(([3 + 7 * j], perm[at:at + c - 1]))))
        at += c - 1
    return out


def keys_of(call, qb, k):
    keys = torch.full((qb * k + 4,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    call(keys.data_ptr())
    torch.cuda.synchronize()
    assert torch.all(keys[qb * k:] == 0x5A5A5A5A)                                  # nothing past the end
    return keys[:qb * k].cpu().numpy().view(np.uint64).reshape(qb, k)


class Case:
    pass


@pytest.fixture(scope="module", params=[100, 130, 520])
def case(request, fir):
    """rows, queries, one Gallery and the exact scan's keys (computed once per row length; nothing below changes them)"""
    d = request.param
    c = Case()
    c.d = d
    rows = synth.make_gallery(11 + d, N, d, L2).copy()
    q, _ = synth.make_queries(11 + d, rows, QB, L2)
    q = q.copy()
    c.copies = copies_of(d)
    for j, rr in enumerate(c.copies):
        rows[rr] = rows[3 + 7 * j]
        q[j] = rows[3 + 7 * j]
    c.rows, c.q = rows, q
    c.tq = torch.from_numpy(q).to(DEV)
    c.g = fir.Gallery(rows, synth.make_labels(N, NC), L2, 0)
    c.g.set_large_batch_mfma(0)                                                    # the exact scan, whatever the batch size
    c.scan = {1: keys_of(lambda p: c.g.search_top1_keys_dev(c.tq.data_ptr(), QB, p), QB, 1)}
    assert c.g.last_dispatch()["path"] == "scan"
    for k in (5, 8):
        c.scan[k] = keys_of(lambda p: c.g.search_topk_keys_dev(c.tq.data_ptr(), QB, k, p), QB, k)
        assert c.g.last_dispatch()["path"] == "scan"
    for a in (rows, q, *c.scan.values()):
        a.setflags(write=False)
    yield c
    c.g.close()


@pytest.fixture(params=["0", "1"])
def rowmajor(request, monkeypatch, fir, case):
    """FIR_GEMM_ROWMAJOR set, and seen to decide the row source of a state created now"""
    monkeypatch.setenv("FIR_GEMM_ROWMAJOR", request.param)
    g = case.g
    g.set_shadow_copies(fir.SHADOW_NONE)                                           # drops the gallery's own state, if any
    g.set_shadow_copies(fir.SHADOW_ALL)
    g.set_large_batch_mfma(32)
    routed = keys_of(lambda p: g.search_top1_keys_dev(case.tq.data_ptr(), QB, p), QB, 1)
    assert g.last_dispatch()["path"] == "mfma", g.last_dispatch()
    shadow = g.memory_bytes()["rowmajor_shadow"]
    g.set_large_batch_mfma(0)
    assert shadow == (N * ((case.d + 3) // 4) * 16 if request.param == "1" else 0), shadow
    assert np.array_equal(routed, case.scan[1])
    return request.param


def test_rows_top1_topk_and_few(fir, case, rowmajor):
    q_ptr = case.tq.data_ptr()
    with fir.GemmSearch(case.g, 2) as m:
        top1 = keys_of(lambda p: m.search_top1_keys_dev(q_ptr, QB, p), QB, 1)
        st = m.stats()
        print("d", case.d, "rowmajor", rowmajor, "top-1", st)
        assert np.array_equal(top1, case.scan[1]), np.nonzero(top1 != case.scan[1])[0][:8]
        assert st["fallback_queries"] == 0 and st["second_pass_queries"] == 0, st
        idx, dist = fir.keys_unpack(top1)
        for j, rr in enumerate(case.copies):
            assert idx[j, 0] == rr[0] and dist[j, 0] == 0.0, (j, idx[j], dist[j])

        for k in (5, 8):
            topk = keys_of(lambda p: m.search_topk_keys_dev(q_ptr, QB, k, p), QB, k)
            st = m.stats()
            print("d", case.d, "rowmajor", rowmajor, "top-%d" % k, st)
            assert np.array_equal(topk, case.scan[k]), (k, np.nonzero((topk != case.scan[k]).any(axis=1))[0][:8])
            assert st["fallback_queries"] == 0 and st["second_pass_queries"] == 0, (k, st)
            idx, dist = fir.keys_unpack(topk)
            for j, rr in enumerate(case.copies):
                if len(rr) >= k:
                    assert np.array_equal(idx[j], rr[:k]) and np.all(dist[j] == 0.0), (k, j, idx[j], dist[j])

        few = keys_of(lambda p: m.search_few_keys_dev(q_ptr, len(COPIES), p), len(COPIES), 1)
        st = m.stats()
        print("d", case.d, "rowmajor", rowmajor, "few", st)
        assert np.array_equal(few, case.scan[1][:len(COPIES)])
        # (its bound is the smallest proxy of ALL rows plus one window: every excluded row is a whole window above the winner)
        assert st["fallback_queries"] == 0, st


def test_classes(fir, case, rowmajor):
    """K = 3 nearest distinct classes: the copies of one row carry different labels (row % 37), so the rounds over distinct
    classes have whole runs of equal keys' worth of entries to step over."""
    scan, gemm, st = both(fir, case.g, case.q, NC, 3)
    print("d", case.d, "rowmajor", rowmajor, "classes", st)
    same(scan, gemm)
    assert st["fallback_queries"] == 0, st
    idx, dist = fir.keys_unpack(gemm[0])
    for j, rr in enumerate(case.copies):
        # the first three distinct labels among the copies, in row order
        want, seen = [], set()
        for r in rr:
            if r % NC not in seen and len(want) < 3:
                seen.add(r % NC)
                want.append(r)
        assert list(idx[j, :len(want)]) == want and np.all(dist[j, :len(want)] == 0.0), (j, idx[j], want)
