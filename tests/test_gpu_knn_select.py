"""fir_search_knn / fir_search_knn_keys_dev / fir_sharded_search_knn on the device (include/fir_amd.h: the K nearest rows, K up
to 1024). The expected keys never come from the select under test: fir_range_distances on the same handle gives every row's
distance bits (the arithmetic the parity tests pin to the reference), a numpy lexsort on (bits, row) with the qualification rule
`dist < 100000` orders them (knn_select_ref.expected_keys), and uint64 keys are compared for equality -- no tolerance anywhere.
For k <= 8 fir_search_topk_keys_dev is the authority and is compared as well."""
import numpy as np
import pytest
import torch

import knn_select_ref as ref
import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
L2, CHI2, KL = 0, 1, 2
ERR_ARG = -1
KS = (1, 8, 9, 64, 255, 256, 1024)
QBS = (1, 3, 9, 17)
POISON = 0x5A5A5A5A5A5A5A5A


def host_keys(idx, dist):
    """(idx, dist) of a host-pointer call packed back into keys."""
    idx = np.asarray(idx).astype(np.int64)
    keys = (ref.orderable(np.asarray(dist, np.float32)).astype(np.uint64) << np.uint64(32)) | (idx.astype(np.uint64) & np.uint64(0xFFFFFFFF))
    return np.where(idx < 0, ref.KEY_NONE, keys)


def expected(g, q, k, start=0, end=0, row_offset=0, dist=None):
    """[qb, k] keys from the handle's own range distances; dist: those distances when the caller already has them."""
    q = np.atleast_2d(q)
    if dist is None:
        dist = g.range_distances(q, start, end) if g.n else np.zeros((q.shape[0], 0), np.float32)
    return np.stack([ref.expected_keys(dist[i], k, row_offset) for i in range(q.shape[0])])


def knn_keys(g, q, k, start=0, end=0):
    """The host-pointer call, as keys; its padding is checked on the way."""
    idx, dist = g.search_knn(q, k, start, end)
    assert idx.shape == dist.shape == (np.atleast_2d(q).shape[0], k)
    assert np.all(dist[idx < 0] == np.float32(100000.0))
    return host_keys(idx, dist)


def new_out(count):
    """A poisoned key buffer with a tail of canary words, filled before anything else is queued."""
    out = torch.full((count + 8,), POISON, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    return out


def dev_keys(g, qt, k, start=0, end=0, stream=None, call="knn", out=None):
    """The device-pointer call into `out`. On the handle's own stream it is waited for; on a caller's stream that is the caller's."""
    if out is None:
        out = new_out(qt.shape[0] * k)
    fn = g.search_knn_keys_dev if call == "knn" else g.search_topk_keys_dev
    fn(qt.data_ptr(), qt.shape[0], k, out.data_ptr(), start, end, stream=stream)
    if stream is None:
        g.sync()
    return out


def as_u64(t, qb, k):
    a = t.cpu().numpy().view(np.uint64)
    assert np.all(a[qb * k:] == np.uint64(POISON))          # nothing written past the end
    return a[: qb * k].reshape(qb, k)


def ranges_of(d):
    return [(0, 0), (7, 9)] + ([(0, 64)] if d >= 64 else [])


@pytest.mark.parametrize("d", (16, 100))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 200, 4097))
@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_every_shape_against_sorted_range_distances(fir, metric, n, d):
    rows = synth.make_gallery(41 + n, n, d, metric)
    q, _ = synth.make_queries(43 + n, rows, max(QBS), metric)
    with fir.Gallery(rows, None, metric, 0) as g:
        for start, end in ranges_of(d):
            dist = g.range_distances(q, start, end)
            for qb in QBS:
                for k in KS:
                    got = knn_keys(g, q[:qb], k, start, end)
                    want = expected(g, q[:qb], k, dist=dist[:qb])
                    assert np.array_equal(got, want), (metric, n, d, start, end, qb, k)


@pytest.mark.parametrize("metric", (CHI2, KL))
def test_out_of_range_operand_takes_the_full_division_sequence(fir, metric):
    n, d = 200, 100
    rows = synth.make_gallery(5, n, d, metric)
    rows[17, 3] = np.float32(1e-9)                           # below 2^-26: outside the plain range
    q, _ = synth.make_queries(6, rows, 9, metric)
    with fir.Gallery(rows, None, metric, 0) as g:
        assert g.value_range()[0] == 0
        for k in (1, 9, 200, 256):
            assert np.array_equal(knn_keys(g, q, k), expected(g, q, k))
        q[4, 8] = np.float32(3e-10)                          # ... and a query value outside it
        for k in (8, 64):
            assert np.array_equal(knn_keys(g, q, k), expected(g, q, k))


@pytest.mark.parametrize("distinct", (3, 1))
def test_cuts_inside_runs_of_equal_distances(fir, distinct):
    n, d = 300, 100
    base = synth.make_gallery(7, distinct, d, L2)
    pick = (synth.splitmix64(np.arange(n, dtype=np.uint64), 11) % np.uint64(distinct)).astype(np.int64)
    rows = base[pick]
    q, _ = synth.make_queries(8, rows, 9, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        assert all(np.unique(dist[i].view(np.uint32)).shape[0] <= distinct for i in range(q.shape[0]))
        for k in KS:
            got = knn_keys(g, q, k)
            assert np.array_equal(got, expected(g, q, k, dist=dist)), (distinct, k)
            idx, _ = ref.unpack(got[0])
            live = idx[idx >= 0]
            assert live.shape[0] == min(k, n)
            # within one distance the rows ascend, and a run that is cut gives up its LOWEST rows
            dq = dist[0][live]
            for v in np.unique(dq.view(np.uint32)):
                run = np.flatnonzero(dist[0].view(np.uint32) == v)
                taken = live[dq.view(np.uint32) == v]
                assert np.array_equal(taken, run[: taken.shape[0]])


@pytest.mark.parametrize("blocks", (None, 1, 2))
def test_several_workgroups_per_query(fir, monkeypatch, blocks):
    """20 000 rows are three workgroups per query and digit (8192 keys each); FIR_KNN_SELECT_BLOCKS caps them: 1 is the
    one-workgroup form, 2 gives slices of 10 240. Half of the rows are copies of five vectors, so the digits of the row word decide."""
    n, d, qb = 20000, 16, 9
    if blocks is not None:
        monkeypatch.setenv("FIR_KNN_SELECT_BLOCKS", str(blocks))
    rows = synth.make_gallery(51, n, d, L2)
    pick = (synth.splitmix64(np.arange(n, dtype=np.uint64), 52) % np.uint64(10)).astype(np.int64)
    base = synth.make_gallery(54, 5, d, L2)
    rows = np.where((pick < 5)[:, None], base[pick % 5], rows)
    q, _ = synth.make_queries(53, rows, qb, L2)
    q[1] = base[2]
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        for k in KS:
            assert np.array_equal(knn_keys(g, q, k), expected(g, q, k, dist=dist)), (blocks, k)
        idx, _ = g.search_knn(q[1:2], 1024)
        assert np.array_equal(idx[0], np.flatnonzero(pick == 2)[:1024])          # 2000 rows at distance 0: the lowest 1024 of them


def test_hostile_values(fir):
    n, d = 200, 100
    rows = synth.make_gallery(13, n, d, L2)
    scale = np.float32(1.0) + np.float32(4000.0) * synth.uniform01(n, 17)      # mean squared differences up to ~ 16e6 / 100
    rows = (rows * scale[:, None]).astype(np.float32)
    rows[50] = np.nan                                                         # a NaN row never qualifies
    q, _ = synth.make_queries(14, rows[:40], 9, L2)
    q[2, 5] = np.nan                                                          # a NaN query: no row qualifies
    q[3, 7] = np.inf                                                          # an inf query: every distance is inf or NaN
    q[5] = q[5] * np.float32(2000.0)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        qual = ref.qualifies(dist).sum(axis=1)
        assert qual[2] == 0 and qual[3] == 0 and 0 < qual[0] < n and not ref.qualifies(dist[:, 50]).any()
        for k in (1, 8, 9, 64, 256, 1024):
            got = knn_keys(g, q, k)
            assert np.array_equal(got, expected(g, q, k, dist=dist)), k
            live = (got != ref.KEY_NONE).sum(axis=1)
            assert np.array_equal(live, np.minimum(qual, k))                  # fewer than k qualify: the rest is padding
            assert np.all(got[2] == ref.KEY_NONE) and np.all(got[3] == ref.KEY_NONE)


def test_row_offset_shows_in_the_low_word(fir):
    rows = synth.make_gallery(19, 200, 16, L2)
    q, _ = synth.make_queries(20, rows, 3, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        plain = knn_keys(g, q, 64)
        g.set_row_offset(1 << 20)
        moved = knn_keys(g, q, 64)
        assert np.array_equal(moved, expected(g, q, 64, row_offset=1 << 20))
        assert np.array_equal(moved, plain + np.uint64(1 << 20))
        qt = torch.from_numpy(q).to(DEV)
        top = as_u64(dev_keys(g, qt, 5, call="topk"), 3, 5)
        g.sync()
        assert np.array_equal(moved[:, :5], top)


def test_empty_gallery_and_k_beyond_n(fir):
    q = synth.uniform01(3 * 16, 23).reshape(3, 16)
    with fir.Gallery(np.zeros((0, 16), np.float32), None, L2, 0) as g:
        for k in (1, 9, 1024):
            assert np.all(knn_keys(g, q, k) == ref.KEY_NONE)
    rows = synth.make_gallery(24, 5, 16, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        got = knn_keys(g, q, 1024)
        assert np.array_equal(got, expected(g, q, 1024))
        assert np.all(got[:, 5:] == ref.KEY_NONE) and np.all(got[:, :5] != ref.KEY_NONE)


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_agrees_with_topk_and_has_the_prefix_property(fir, metric):
    n, d, qb = 4097, 100, 17
    rows = synth.make_gallery(29, n, d, metric)
    rows[4000] = rows[12]
    q, _ = synth.make_queries(30, rows, qb, metric)
    q[1] = rows[12]
    qt = torch.from_numpy(q).to(DEV)
    with fir.Gallery(rows, None, metric, 0) as g:
        for start, end in ((0, 0), (0, 64), (7, 9)):
            big = as_u64(dev_keys(g, qt, 300, start, end), qb, 300)
            for k in (1, 5, 8):
                top = as_u64(dev_keys(g, qt, k, start, end, call="topk"), qb, k)
                knn = as_u64(dev_keys(g, qt, k, start, end), qb, k)
                assert np.array_equal(knn, top), (metric, start, end, k)        # bit-identical for k <= 8
                assert np.array_equal(big[:, :k], top), (metric, start, end, k)  # and the first k' keys of any larger call
        hidx, hdist = g.search_topk(q, 8)
        assert np.array_equal(knn_keys(g, q, 8), host_keys(hidx, hdist))
        whole = as_u64(dev_keys(g, qt, 300), qb, 300)
        assert list(ref.unpack(whole[1, :2])[0]) == [12, 4000]                   # equal distances: the lower row first


def test_two_calls_give_the_same_bytes(fir):
    n, d, qb, k = 4097, 16, 9, 1024
    pick = (synth.splitmix64(np.arange(n, dtype=np.uint64), 31) % np.uint64(7)).astype(np.int64)
    rows = synth.make_gallery(32, 7, d, L2)[pick]            # long runs of equal distances: the compaction order varies freely
    q, _ = synth.make_queries(33, rows, qb, L2)
    qt = torch.from_numpy(q).to(DEV)
    with fir.Gallery(rows, None, L2, 0) as g:
        a = dev_keys(g, qt, k)
        b = dev_keys(g, qt, k)
        g.sync()
        assert torch.equal(a, b)
        assert np.array_equal(as_u64(a, qb, k), expected(g, q, k))


def test_device_form_on_caller_streams_in_call_order(fir):
    """_keys_dev on one torch stream, a top-1 call on another right behind it, nothing synchronised in between: the handle's call
    order makes the second wait for the first (they share the transposed-query scratch), and both results are right."""
    n, d = 4097, 100
    rows = synth.make_gallery(35, n, d, L2)
    qa, _ = synth.make_queries(36, rows, 17, L2)
    qb_, _ = synth.make_queries(37, rows, 9, L2)
    ta, tb = torch.from_numpy(qa).to(DEV), torch.from_numpy(qb_).to(DEV)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with fir.Gallery(rows, None, L2, 0) as g:
        want_knn = expected(g, qa, 256)
        want_top = expected(g, qb_, 1)
        record = g.last_dispatch()
        scratch0 = g.memory_bytes()["scratch"]
        first = dev_keys(g, ta, 256, stream=s1.cuda_stream)
        assert g.last_dispatch() == record                           # not a top-1 search: the dispatch record is left alone
        assert g.memory_bytes()["scratch"] > scratch0                # the distance tile is counted under scratch
        s1.synchronize()
        assert np.array_equal(as_u64(first, 17, 256), want_knn)
        for _ in range(2):
            knn, top, again = new_out(17 * 256), new_out(9), new_out(17 * 9)
            dev_keys(g, ta, 256, stream=s1.cuda_stream, out=knn)
            g.search_top1_keys_dev(tb.data_ptr(), 9, top.data_ptr(), stream=s2.cuda_stream)
            dev_keys(g, ta, 9, stream=s1.cuda_stream, out=again)
            s1.synchronize()
            s2.synchronize()
            assert np.array_equal(as_u64(knn, 17, 256), want_knn)
            assert np.array_equal(as_u64(top, 9, 1), want_top)
            assert np.array_equal(as_u64(again, 17, 9)[:3], want_knn[:3, :9])
        # the scratch holds ONE query tile's distances whatever qb is
        a = g.memory_bytes()["scratch"]
        big = torch.from_numpy(np.tile(qa, (8, 1))).to(DEV)
        out = dev_keys(g, big, 9)
        assert g.memory_bytes()["scratch"] == a
        assert np.array_equal(as_u64(out, 17 * 8, 9), np.tile(want_knn[:, :9], (8, 1)))


def test_profile_read_times_store_and_select_of_every_tile(fir):
    """fir_profile_enable: two event pairs per tile of queries, the store pass and then the select; the keys are what they are without."""
    n, d, qb, k = 4097, 100, 17, 64
    rows = synth.make_gallery(47, n, d, L2)
    q, _ = synth.make_queries(48, rows, qb, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        want = knn_keys(g, q, k)
        g.set_tuning(8, 0)                                   # tiles of 8, 8 and 1 queries
        g.profile_enable(True)
        g.profile_read()
        got = knn_keys(g, q, k)
        ms, _ = g.profile_read()
        g.profile_enable(False)
        assert ms.shape[0] == 2 * 3 and np.all(ms > 0)
        assert np.array_equal(got, want)
        knn_keys(g, q, k)
        assert g.profile_read()[0].shape[0] == 0             # off again: nothing recorded


def test_argument_errors_and_their_order(fir):
    rows = synth.make_gallery(39, 70, 16, L2)
    q, _ = synth.make_queries(40, rows, 2, L2)
    qt = torch.from_numpy(q).to(DEV)
    L = fir.lib()
    idx = np.full((2, 4), 77, np.int32)
    dist = np.full((2, 4), 77, np.float32)
    pi, pd, pq = idx.ctypes.data, dist.ctypes.data, np.ascontiguousarray(q).ctypes.data

    def err(rc):
        assert rc == ERR_ARG
        return L.fir_last_error().decode()

    with fir.Gallery(rows, None, L2, 0) as g:
        for k, text in ((0, "k=0 outside [1,1024]"), (1025, "k=1025 outside [1,1024]"), (-3, "k=-3 outside [1,1024]")):
            with pytest.raises(fir.FirError) as e:
                g.search_knn(q, k) if k >= 0 else fir.capi._check(L.fir_search_knn(g._h, pq, 2, 0, 0, k, pi, pd))
            assert e.value.code == ERR_ARG and str(e.value).endswith(text)
            keys = torch.full((8,), POISON, dtype=torch.int64, device=DEV)
            assert err(L.fir_search_knn_keys_dev(g._h, qt.data_ptr(), 2, 0, 0, k, keys.data_ptr(), None)) == text
        h = g._h
        # NULL first, then qb < 0, then k, then qb == 0 (nothing to do), then the range
        assert err(L.fir_search_knn(h, pq, 2, 0, 0, 4, None, pd)) == "NULL argument"
        assert err(L.fir_search_knn(h, pq, 2, 0, 0, 4, pi, None)) == "NULL argument"
        assert err(L.fir_search_knn(h, None, 2, 0, 0, 4, pi, pd)) == "NULL argument"
        assert err(L.fir_search_knn(None, pq, 2, 0, 0, 4, pi, pd)) == "NULL argument"
        assert err(L.fir_search_knn_keys_dev(h, qt.data_ptr(), 2, 0, 0, 4, None, None)) == "NULL argument"
        assert err(L.fir_search_knn(h, pq, -1, 5, 3, 0, None, pd)) == "NULL argument"
        assert err(L.fir_search_knn(h, pq, -1, 5, 3, 0, pi, pd)) == "qb < 0"
        assert err(L.fir_search_knn(h, pq, 0, 5, 3, 0, pi, pd)) == "k=0 outside [1,1024]"
        assert err(L.fir_search_knn(h, pq, 2, 5, 3, 2000, pi, pd)) == "k=2000 outside [1,1024]"
        assert L.fir_search_knn(h, pq, 0, 5, 3, 4, pi, pd) == 0                      # qb == 0 comes before the range
        assert L.fir_search_knn(h, None, 0, 0, 0, 4, pi, pd) == 0                    # ... and needs no queries
        assert err(L.fir_search_knn(h, pq, 2, 5, 3, 4, pi, pd)) == "feature range [5,3) not inside [0,16)"
        assert err(L.fir_search_knn(h, pq, 2, 0, 17, 4, pi, pd)) == "feature range [0,17) not inside [0,16)"
        assert np.all(idx == 77) and np.all(dist == 77)                              # no failed or empty call touched the outputs
        scratch = g.memory_bytes()["scratch"]
        assert err(L.fir_search_knn(h, pq, 2, 0, 0, 1025, pi, pd)) == "k=1025 outside [1,1024]"
        assert g.memory_bytes()["scratch"] == scratch                                # checked before anything is allocated
        assert np.array_equal(knn_keys(g, q, 4), expected(g, q, 4))                  # and the handle is fine afterwards


@pytest.mark.parametrize("spd", (1, 5))
def test_sharded_keys_equal_the_unsharded_handle(fir, spd):
    n, d, qb = 1000, 100, 9
    rows = synth.make_gallery(45, n, d, L2)
    rows[990] = rows[3]
    rows[500] = rows[3]
    q, _ = synth.make_queries(46, rows, qb, L2)
    q[0] = rows[3]                                           # equal distances in different shards: ordered by global row
    q[4] = np.float32(1e4)                                   # nothing qualifies anywhere
    with fir.Gallery(rows, None, L2, 0) as g:
        want = {(k, r): expected(g, q, k, *r) for k in (1, 5, 9, 256, 1024) for r in ((0, 0), (7, 9))}
    with fir.ShardedGallery(rows, None, L2, devices=[0], shards_per_device=spd) as s:
        smallest = min(s.shard(i)[2] for i in range(spd))
        for (k, r), w in want.items():
            idx, dist = s.search_knn(q, k, *r)
            assert np.array_equal(host_keys(idx, dist), w), (spd, k, r)
        if spd > 1:
            assert smallest < 256                            # k exceeds a shard's rows: its list arrives padded
        idx, _ = s.search_knn(q, 9)
        assert list(idx[0][:3]) == [3, 500, 990] and np.all(idx[4] == -1)
        ti, td = s.search_topk(q, 8)                         # the K <= 8 call is what it was
        ki, kd = s.search_knn(q, 8)
        assert np.array_equal(ti, ki) and np.array_equal(td.view(np.uint32), kd.view(np.uint32))
        with pytest.raises(fir.FirError) as e:
            s.search_knn(q, 1025)
        assert e.value.code == ERR_ARG and str(e.value).endswith("k=1025 outside [1,1024]")
        with pytest.raises(fir.FirError) as e:
            s.search_topk(q, 9)
        assert str(e.value).endswith("k=9 outside [1,8]")
