"""fir_search_radius / fir_search_radius_keys_dev on the device (include/fir_amd.h: every row within a per-query radius).
The expected counts and keys never come from the code under test: fir_range_distances on the same handle gives every row's
distance bits (the arithmetic the parity tests pin to the reference), radius_ref.expected filters them with the contract's two
float compares and sorts the packed keys, and counts and uint64 keys are compared for equality -- no tolerance anywhere. The radii
are made from those distances too, sorted on the host: below the minimum, the exact bits of the r-th smallest distance (which
leaves that row and its ties out: the compare is strict), its nextafter (which takes them in), r in {1, max_results,
max_results + 1, n}, and +inf -- a different kind for every query of a call."""
import numpy as np
import pytest
import torch

import knn_select_ref as kref
import radius_ref as ref
import synth
from test_gpu_knn_select import host_keys

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
L2, CHI2, KL = 0, 1, 2
ERR_ARG = -1
F32 = np.float32
MS = (0, 1, 8, 9, 256, 1024)
QBS = (1, 3, 9, 17)
POISON = 0x5A5A5A5A5A5A5A5A
POISON32 = 0x5A5A5A5A
INF = F32(np.inf)


def radii_from(dist, m, shift=0):
    """One radius per query of dist [qb, n], the kind rotating with the query: see the module's docstring."""
    qb, n = dist.shape
    out = np.empty(qb, F32)
    ranks = (1, max(m, 1), m + 1, n)
    for i in range(qb):
        s = np.sort(dist[i][kref.qualifies(dist[i])])
        kind = (i + shift) % 10
        if s.shape[0] == 0:
            out[i] = F32(1.0)
        elif kind == 0:
            out[i] = np.nextafter(s[0], -INF)                     # below the minimum
        elif kind == 9:
            out[i] = INF
        else:
            at = s[min(ranks[(kind - 1) // 2], s.shape[0]) - 1]
            out[i] = at if kind % 2 else np.nextafter(at, INF)
    return out


def host_call(g, q, radius, m, start=0, end=0):
    """The host-pointer call as (count, keys); its shapes and padding are checked on the way."""
    qb = np.atleast_2d(q).shape[0]
    count, idx, dist = g.search_radius(q, radius, m, start, end)
    assert count.shape == (qb,) and count.dtype == np.int32
    if m == 0:
        assert idx is None and dist is None
        return count, np.zeros((qb, 0), np.uint64)
    assert idx.shape == dist.shape == (qb, m)
    assert np.all(dist[idx < 0] == F32(100000.0))
    assert np.array_equal((idx >= 0).sum(axis=1), np.minimum(count, m))
    return count, host_keys(idx, dist)


def check_host(g, q, radius, m, dist, start=0, end=0, row_offset=0, label=None):
    count, keys = host_call(g, q, radius, m, start, end)
    want_c, want_k = ref.expected_batch(dist, radius, m, row_offset)
    assert np.array_equal(count, want_c), (label, m, count.tolist(), want_c.tolist())
    assert np.array_equal(keys, want_k), (label, m)
    return count, keys


class DevOut:
    """Poisoned key and count buffers, each with a tail of canary words, filled before anything else is queued."""

    def __init__(self, qb, m):
        self.qb, self.m = qb, m
        self.keys = torch.full((qb * m + 8,), POISON, dtype=torch.int64, device=DEV)
        self.count = torch.full((qb + 8,), POISON32, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def read(self):
        k = self.keys.cpu().numpy().view(np.uint64)
        c = self.count.cpu().numpy()
        assert np.all(k[self.qb * self.m:] == np.uint64(POISON)) and np.all(c[self.qb:] == POISON32)      # nothing written past the end
        return c[: self.qb].copy(), k[: self.qb * self.m].reshape(self.qb, self.m).copy()


def dev_call(g, qt, rt, m, start=0, end=0, stream=None, out=None):
    """The device-pointer call into `out`. On the handle's own stream it is waited for; on a caller's stream that is the caller's."""
    if out is None:
        out = DevOut(qt.shape[0], m)
    g.search_radius_keys_dev(qt.data_ptr(), qt.shape[0], rt.data_ptr(), m, out.count.data_ptr(), out.keys.data_ptr() if m else None,
                             start, end, stream=stream)
    if stream is None:
        g.sync()
    return out


def ranges_of(d):
    return [(0, 0), (7, 9)] + ([(0, 64)] if d >= 64 else [])


@pytest.mark.parametrize("d", (16, 100))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 200, 4097))
@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_every_shape_against_filtered_range_distances(fir, metric, n, d):
    rows = synth.make_gallery(141 + n, n, d, metric)
    q, _ = synth.make_queries(143 + n, rows, max(QBS), metric)
    with fir.Gallery(rows, None, metric, 0) as g:
        for start, end in ranges_of(d):
            dist = g.range_distances(q, start, end)
            for qb in QBS:
                for m in MS:
                    radius = radii_from(dist[:qb], m, shift=qb)
                    check_host(g, q[:qb], radius, m, dist[:qb], start, end, label=(metric, n, d, start, end, qb))


def test_several_workgroups_per_query_in_count_and_select(fir):
    """20 000 rows are three workgroups per query in the count and in every digit of the select; half of the rows are copies of
    five vectors, so counts run into the thousands and the digits of the row word decide."""
    n, d, qb = 20000, 16, 17
    rows = synth.make_gallery(151, n, d, L2)
    pick = (synth.splitmix64(np.arange(n, dtype=np.uint64), 152) % np.uint64(10)).astype(np.int64)
    base = synth.make_gallery(154, 5, d, L2)
    rows = np.where((pick < 5)[:, None], base[pick % 5], rows)
    q, _ = synth.make_queries(153, rows, qb, L2)
    q[1] = base[2]
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        for m in MS:
            radius = radii_from(dist, m)
            radius[1] = np.nextafter(F32(0.0), INF)                # the 2000 copies of the query and nothing else
            count, keys = check_host(g, q, radius, m, dist, label="20000")
            assert count[1] == (pick == 2).sum()
            if m:
                assert np.array_equal(kref.unpack(keys[1])[0][: min(m, count[1])], np.flatnonzero(pick == 2)[:m])
        count, _ = check_host(g, q, INF, 0, dist)
        assert np.all(count == n)


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_infinite_radius_is_search_knn_bit_for_bit(fir, metric):
    n, d, qb = 4097, 100, 17
    rows = synth.make_gallery(129, n, d, metric)
    rows[4000] = rows[12]
    q, _ = synth.make_queries(130, rows, qb, metric)
    q[1] = rows[12]
    qt = torch.from_numpy(q).to(DEV)
    with fir.Gallery(rows, None, metric, 0) as g:
        qual = kref.qualifies(g.range_distances(q)).sum(axis=1)
        for value in (INF, F32(100000.0), F32(3e38)):
            rt = torch.full((qb,), float(value), dtype=torch.float32, device=DEV)
            for m in (1, 8, 9, 300, 1024):
                knn = torch.full((qb * m,), POISON, dtype=torch.int64, device=DEV)
                g.search_knn_keys_dev(qt.data_ptr(), qb, m, knn.data_ptr())
                g.sync()
                count, keys = dev_call(g, qt, rt, m).read()
                assert np.array_equal(keys, knn.cpu().numpy().view(np.uint64).reshape(qb, m)), (metric, value, m)
                assert np.array_equal(count, qual)


@pytest.mark.parametrize("distinct", (3, 1))
def test_cuts_inside_runs_of_equal_distances(fir, distinct):
    n, d = 300, 100
    base = synth.make_gallery(107, distinct, d, L2)
    pick = (synth.splitmix64(np.arange(n, dtype=np.uint64), 111) % np.uint64(distinct)).astype(np.int64)
    rows = base[pick]
    q, _ = synth.make_queries(108, rows, 9, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        values = [np.unique(dist[i]) for i in range(9)]
        assert all(v.shape[0] <= distinct for v in values)
        for m in MS:
            for which in range(distinct):
                at = np.array([v[min(which, v.shape[0] - 1)] for v in values], F32)
                # the run's own distance leaves the whole run out; one ulp more takes all of it in, and max_results cuts inside it
                for radius in (at, np.nextafter(at, INF)):
                    count, keys = check_host(g, q, radius, m, dist, label=(distinct, which))
                    assert np.array_equal(count, [(dist[i] < radius[i]).sum() for i in range(9)])
                    if m:
                        idx, _ = kref.unpack(keys[0])
                        live = idx[idx >= 0]
                        for v in np.unique(dist[0][live].view(np.uint32)):
                            run = np.flatnonzero(dist[0].view(np.uint32) == v)
                            taken = live[dist[0][live].view(np.uint32) == v]
                            assert np.array_equal(taken, run[: taken.shape[0]])      # a run that is cut gives up its LOWEST rows


def test_zero_radius_against_copies_of_the_query_counts_nothing(fir):
    n, d = 200, 16
    rows = synth.make_gallery(113, n, d, L2)
    rows[::7] = rows[3]
    q = np.stack([rows[3], rows[5], rows[3]])
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        assert (dist[0] == 0).sum() == len(range(0, n, 7)) + 1
        for radius in (F32(0.0), F32(-0.0)):
            count, keys = check_host(g, q, radius, 9, dist)
            assert np.all(count == 0) and np.all(keys == ref.KEY_NONE)
        count, _ = check_host(g, q, np.nextafter(F32(0.0), INF), 9, dist)
        assert count.tolist() == [30, 1, 30]


def test_hostile_radii_rows_and_queries(fir):
    n, d = 200, 100
    rows = synth.make_gallery(213, n, d, L2)
    scale = F32(1.0) + F32(4000.0) * synth.uniform01(n, 217)      # mean squared differences up to ~ 16e6 / 100
    rows = (rows * scale[:, None]).astype(F32)
    rows[50] = np.nan                                             # a NaN row never qualifies
    rows[51, 3] = np.inf                                          # an inf row: its distance is inf
    q, _ = synth.make_queries(214, rows[:40], 17, L2)
    q[2, 5] = np.nan                                              # a NaN query: no row qualifies
    q[3, 7] = np.inf                                              # an inf query: every distance is inf or NaN
    q[5] = q[5] * F32(2000.0)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        qual = kref.qualifies(dist).sum(axis=1)
        assert qual[2] == 0 and qual[3] == 0 and 0 < qual[0] < n and not kref.qualifies(dist[:, 50]).any()
        finite = np.sort(np.where(kref.qualifies(dist), dist, INF), axis=1)
        for m in MS:
            radius = radii_from(dist, m)
            radius[6], radius[7], radius[8] = np.nan, -INF, F32(-1.0)
            radius[9], radius[10] = INF, F32(100000.0)            # both: every row fir_search_knn considers
            radius[11] = finite[11, 5]                            # the sixth smallest distance itself: five rows
            radius[2], radius[3] = INF, INF
            assert finite[11, 4] < finite[11, 5] < F32(100000.0)
            count, keys = check_host(g, q, radius, m, dist, label="hostile")
            assert np.all(count[[2, 3, 6, 7, 8]] == 0) and count[9] == qual[9] and count[10] == qual[10] and count[11] == 5
            assert np.all(keys[[2, 3, 6, 7, 8]] == ref.KEY_NONE)


def test_row_offset_shows_in_the_low_word(fir):
    rows = synth.make_gallery(119, 200, 16, L2)
    q, _ = synth.make_queries(120, rows, 3, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        radius = radii_from(dist, 64, shift=5)
        plain_c, plain = check_host(g, q, radius, 64, dist)
        g.set_row_offset(1 << 20)
        moved_c, moved = check_host(g, q, radius, 64, dist, row_offset=1 << 20)
        live = plain != ref.KEY_NONE
        assert live.any() and np.array_equal(moved_c, plain_c) and np.array_equal(live, moved != ref.KEY_NONE)
        assert np.array_equal(moved[live], plain[live] + np.uint64(1 << 20))


def test_empty_gallery(fir):
    q = synth.uniform01(3 * 16, 123).reshape(3, 16)
    qt = torch.from_numpy(q).to(DEV)
    rt = torch.full((3,), float("inf"), dtype=torch.float32, device=DEV)
    with fir.Gallery(np.zeros((0, 16), np.float32), None, L2, 0) as g:
        for m in MS:
            count, keys = host_call(g, q, INF, m)
            assert np.all(count == 0) and np.all(keys == ref.KEY_NONE)
            count, keys = dev_call(g, qt, rt, m).read()
            assert np.all(count == 0) and np.all(keys == ref.KEY_NONE)


def test_device_form_fills_exactly_its_slots_and_two_calls_give_the_same_bytes(fir):
    n, d, qb = 4097, 16, 9
    pick = (synth.splitmix64(np.arange(n, dtype=np.uint64), 131) % np.uint64(7)).astype(np.int64)
    rows = synth.make_gallery(132, 7, d, L2)[pick]            # long runs of equal distances: the compaction order varies freely
    q, _ = synth.make_queries(133, rows, qb, L2)
    qt = torch.from_numpy(q).to(DEV)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        for m in MS:
            radius = radii_from(dist, m, shift=3)
            rt = torch.from_numpy(radius).to(DEV)
            a = dev_call(g, qt, rt, m)
            b = dev_call(g, qt, rt, m)
            assert torch.equal(a.keys, b.keys) and torch.equal(a.count, b.count)
            count, keys = a.read()                            # (the canaries behind keys and counts are checked here)
            want_c, want_k = ref.expected_batch(dist, radius, m)
            assert np.array_equal(count, want_c) and np.array_equal(keys, want_k), m


def test_device_form_on_caller_streams_in_call_order(fir):
    """_keys_dev on one torch stream, a top-1 call on another right behind it, nothing synchronised in between: the handle's call
    order makes the second wait for the first (they share the transposed-query scratch), and both results are right."""
    n, d = 4097, 100
    rows = synth.make_gallery(135, n, d, L2)
    qa, _ = synth.make_queries(136, rows, 17, L2)
    qb_, _ = synth.make_queries(137, rows, 9, L2)
    ta, tb = torch.from_numpy(qa).to(DEV), torch.from_numpy(qb_).to(DEV)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(qa)
        radius = radii_from(dist, 256)
        rt = torch.from_numpy(radius).to(DEV)
        want_c, want_k = ref.expected_batch(dist, radius, 256)
        want_c9, want_k9 = ref.expected_batch(dist, radius, 9)
        want_top = np.stack([kref.expected_keys(r, 1) for r in g.range_distances(qb_)])
        record = g.last_dispatch()
        first = dev_call(g, ta, rt, 256, stream=s1.cuda_stream)
        assert g.last_dispatch() == record                           # not a top-1 search: the dispatch record is left alone
        s1.synchronize()
        count, keys = first.read()
        assert np.array_equal(count, want_c) and np.array_equal(keys, want_k)
        for _ in range(2):
            big, top, again = DevOut(17, 256), torch.full((9 + 8,), POISON, dtype=torch.int64, device=DEV), DevOut(17, 9)
            torch.cuda.synchronize()
            dev_call(g, ta, rt, 256, stream=s1.cuda_stream, out=big)
            g.search_top1_keys_dev(tb.data_ptr(), 9, top.data_ptr(), stream=s2.cuda_stream)
            dev_call(g, ta, rt, 9, stream=s1.cuda_stream, out=again)
            s1.synchronize()
            s2.synchronize()
            count, keys = big.read()
            assert np.array_equal(count, want_c) and np.array_equal(keys, want_k)
            assert np.array_equal(top.cpu().numpy().view(np.uint64)[:9].reshape(9, 1), want_top)
            count, keys = again.read()
            assert np.array_equal(count, want_c9) and np.array_equal(keys, want_k9)
        # the scratch holds ONE query tile's distances whatever qb is
        a = g.memory_bytes()["scratch"]
        out = dev_call(g, torch.from_numpy(np.tile(qa, (8, 1))).to(DEV), torch.from_numpy(np.tile(radius, 8)).to(DEV), 9)
        assert g.memory_bytes()["scratch"] == a
        count, keys = out.read()
        assert np.array_equal(count, np.tile(want_c9, 8)) and np.array_equal(keys, np.tile(want_k9, (8, 1)))


def test_profile_read_times_store_and_count_select_of_every_tile(fir):
    """fir_profile_enable: two event pairs per tile of queries, the store pass and then count + select + sort (max_results = 0:
    the count alone); the results are what they are without."""
    n, d, qb = 4097, 100, 17
    rows = synth.make_gallery(147, n, d, L2)
    q, _ = synth.make_queries(148, rows, qb, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        for m in (64, 0):
            radius = radii_from(dist, m)
            want = check_host(g, q, radius, m, dist)
            g.set_tuning(8, 0)                                   # tiles of 8, 8 and 1 queries
            g.profile_enable(True)
            g.profile_read()
            got = host_call(g, q, radius, m)
            ms, _ = g.profile_read()
            g.profile_enable(False)
            assert ms.shape[0] == 2 * 3 and np.all(ms > 0)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            host_call(g, q, radius, m)
            assert g.profile_read()[0].shape[0] == 0             # off again: nothing recorded
            g.set_tuning(0, 0)


def test_argument_errors_and_their_order(fir):
    rows = synth.make_gallery(139, 70, 16, L2)
    q, _ = synth.make_queries(140, rows, 2, L2)
    qt = torch.from_numpy(q).to(DEV)
    rt = torch.ones(2, dtype=torch.float32, device=DEV)
    L = fir.lib()
    idx = np.full((2, 4), 77, np.int32)
    dist = np.full((2, 4), 77, np.float32)
    cnt = np.full(2, 77, np.int32)
    rad = np.ones(2, np.float32)
    pi, pd, pc, pr, pq = idx.ctypes.data, dist.ctypes.data, cnt.ctypes.data, rad.ctypes.data, np.ascontiguousarray(q).ctypes.data

    def err(rc):
        assert rc == ERR_ARG
        return L.fir_last_error().decode()

    with fir.Gallery(rows, None, L2, 0) as g:
        h = g._h
        keys = torch.full((8,), POISON, dtype=torch.int64, device=DEV)
        dcnt = torch.full((2,), POISON32, dtype=torch.int32, device=DEV)
        for m, text in ((1025, "max_results=1025 outside [0,1024]"), (-3, "max_results=-3 outside [0,1024]")):
            assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, m, pc, pi, pd)) == text
            assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, m, pc, None, None)) == text
            assert err(L.fir_search_radius_keys_dev(h, qt.data_ptr(), 2, 0, 0, rt.data_ptr(), m, dcnt.data_ptr(), keys.data_ptr(), None)) == text
        with pytest.raises(fir.FirError) as e:
            g.search_radius(q, 1.0, 1025)
        assert e.value.code == ERR_ARG and str(e.value).endswith("max_results=1025 outside [0,1024]")
        # NULL first, then qb < 0, then max_results, then qb == 0 (nothing to do), then the range
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 4, pc, None, pd)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 4, pc, pi, None)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 4, None, pi, pd)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, None, 4, pc, pi, pd)) == "NULL argument"
        assert err(L.fir_search_radius(h, None, 2, 0, 0, pr, 4, pc, pi, pd)) == "NULL argument"
        assert err(L.fir_search_radius(None, pq, 2, 0, 0, pr, 4, pc, pi, pd)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 0, pc, pi, None)) == "NULL argument"      # count-only: keys, idx and dist must be NULL
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 0, pc, None, pd)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 0, None, None, None)) == "NULL argument"
        assert err(L.fir_search_radius_keys_dev(h, qt.data_ptr(), 2, 0, 0, rt.data_ptr(), 4, dcnt.data_ptr(), None, None)) == "NULL argument"
        assert err(L.fir_search_radius_keys_dev(h, qt.data_ptr(), 2, 0, 0, rt.data_ptr(), 0, dcnt.data_ptr(), keys.data_ptr(), None)) == "NULL argument"
        assert err(L.fir_search_radius_keys_dev(h, qt.data_ptr(), 2, 0, 0, rt.data_ptr(), 4, None, keys.data_ptr(), None)) == "NULL argument"
        assert err(L.fir_search_radius_keys_dev(h, qt.data_ptr(), 2, 0, 0, None, 4, dcnt.data_ptr(), keys.data_ptr(), None)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, -1, 5, 3, pr, 2000, None, pi, pd)) == "NULL argument"
        assert err(L.fir_search_radius(h, pq, -1, 5, 3, pr, 2000, pc, pi, pd)) == "qb < 0"
        assert err(L.fir_search_radius(h, pq, 0, 5, 3, pr, 2000, pc, pi, pd)) == "max_results=2000 outside [0,1024]"
        assert err(L.fir_search_radius(h, pq, 2, 5, 3, pr, -1, pc, pi, pd)) == "max_results=-1 outside [0,1024]"
        assert L.fir_search_radius(h, pq, 0, 5, 3, pr, 4, pc, pi, pd) == 0                    # qb == 0 comes before the range
        assert L.fir_search_radius(h, None, 0, 0, 0, None, 4, pc, pi, pd) == 0                # ... and needs neither queries nor radii
        assert err(L.fir_search_radius(h, pq, 2, 5, 3, pr, 4, pc, pi, pd)) == "feature range [5,3) not inside [0,16)"
        assert err(L.fir_search_radius(h, pq, 2, 0, 17, pr, 0, pc, None, None)) == "feature range [0,17) not inside [0,16)"
        assert np.all(idx == 77) and np.all(dist == 77) and np.all(cnt == 77)                 # no failed or empty call touched the outputs
        assert np.all(keys.cpu().numpy() == POISON) and np.all(dcnt.cpu().numpy() == POISON32)
        scratch = g.memory_bytes()["scratch"]
        assert err(L.fir_search_radius(h, pq, 2, 0, 0, pr, 1025, pc, pi, pd)) == "max_results=1025 outside [0,1024]"
        assert g.memory_bytes()["scratch"] == scratch                                         # checked before anything is allocated
        d_all = g.range_distances(q)
        check_host(g, q, radii_from(d_all, 4, shift=3), 4, d_all)                             # and the handle is fine afterwards


@pytest.mark.parametrize("spd", (1, 3))
def test_sharded_counts_and_keys_equal_the_unsharded_handle(fir, spd):
    n, d, qb = 1000, 100, 9
    rows = synth.make_gallery(145, n, d, L2)
    rows[990] = rows[3]
    rows[500] = rows[3]
    q, _ = synth.make_queries(146, rows, qb, L2)
    q[0] = rows[3]                                           # equal distances in different shards: ordered by global row
    q[4] = F32(1e4)                                          # nothing qualifies anywhere
    want = {}
    with fir.Gallery(rows, None, L2, 0) as g:
        for r in ((0, 0), (7, 9)):
            dist = g.range_distances(q, *r)
            for m in MS:
                radius = radii_from(dist, m, shift=m)
                radius[0] = np.nextafter(F32(0.0), INF) if m != 8 else INF
                want[(m, r)] = (radius,) + ref.expected_batch(dist, radius, m) + host_call(g, q, radius, m, *r)
    with fir.ShardedGallery(rows, None, L2, devices=[0], shards_per_device=spd) as s:
        for (m, r), (radius, want_c, want_k, one_c, one_k) in want.items():
            count, idx, dist = s.search_radius(q, radius, m, *r)
            assert np.array_equal(count, want_c) and np.array_equal(count, one_c), (spd, m, r, count.tolist(), want_c.tolist())
            if m == 0:
                assert idx is None and dist is None
                continue
            keys = host_keys(idx, dist)
            assert np.array_equal(keys, want_k) and np.array_equal(keys, one_k), (spd, m, r)
        count, idx, _ = s.search_radius(q, np.nextafter(F32(0.0), INF), 9)
        assert count[0] == 3 and list(idx[0][:4]) == [3, 500, 990, -1] and count[4] == 0 and np.all(idx[4] == -1)
        count, _, _ = s.search_radius(q[:8], INF, 0)         # an even number of queries: no padding word behind the counts
        assert np.array_equal(count, [n] * 3 + [n] + [0] + [n] * 3)
        ki, kd = s.search_knn(q, 256)                        # the kNN call is what it was, and an infinite radius gives its keys
        count, ri, rd = s.search_radius(q, INF, 256)
        assert np.array_equal(ki, ri) and np.array_equal(kd.view(np.uint32), rd.view(np.uint32))
        with pytest.raises(fir.FirError) as e:
            s.search_radius(q, 1.0, 1025)
        assert e.value.code == ERR_ARG and str(e.value).endswith("max_results=1025 outside [0,1024]")
