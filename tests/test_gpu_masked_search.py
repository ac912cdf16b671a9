"""The masked searches on the device (include/fir_amd.h, "searches over a subset of the rows"): top-1, kNN, radius, classes and the
class-mask builders. No expected value comes from the code under test and nothing has a tolerance -- keys, counts and classes are
compared for equality against TWO oracles:
  (a) fir_range_distances on the same handle (the arithmetic the parity tests pin to the reference) plus masked_ref, the numpy
      restatement tests/test_masked_formulation.py pins to the oracle;
  (b) a fresh handle over rows[mask] (labels too) with the UNMASKED call of the same name, every returned row mapped back through
      np.flatnonzero(mask): the contract's own words, distance bits equal.
fir_gallery_set_tuning takes its wave count in whole workgroups of 4: "one and three" are 4 and 12 here."""
import numpy as np
import pytest
import torch

import knn_select_ref as ks
import masked_ref as ref
import synth
from test_gpu_knn_select import host_keys

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
L2, CHI2, KL = 0, 1, 2
ERR_ARG, ERR_STATE = -1, -5
F32, I32 = np.float32, np.int32
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
QBS = (1, 3, 8, 9, 17)
POISON = 0x5A5A5A5A5A5A5A5A
NONE = ref.KEY_NONE


def runs_of_30(n):
    return (np.arange(n) // 30).astype(I32)


def permuted(n, classes, seed):
    return (synth.splitmix64(np.arange(n, dtype=np.uint64), seed) % np.uint64(classes)).astype(I32)


def random_half(n, seed):
    return (synth.splitmix64(np.arange(n, dtype=np.uint64), seed) & np.uint64(1)).astype(bool)


def ranges_of(d):
    return [r for r in ((0, 0), (3, 61), (4, 5)) if r[1] <= d]


def masks_of(n, seed):
    """name -> bool[n]: the shapes of the issue. Zero words lie between non-zero ones wherever n has three tiles or more."""
    m = {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 1, "half": random_half(n, seed)}
    for name, r in (("first", 0), ("last", n - 1), ("one bit", n // 2)):
        m[name] = np.zeros(n, bool)
        m[name][r] = True
    gaps = random_half(n, seed + 1)
    gaps[64:128] = False                                   # a zero word between two others (n > 128) ...
    if n > 64:
        gaps[(n - 1) // 64 * 64:] = False                  # ... and a zero word for the last, part-full tile
        gaps[0] = True
    m["zero words"] = gaps
    return m


def with_garbage(take):
    """The packed words of `take` with every bit at or past n set: they must change nothing."""
    words = ref.pack_bits(take)
    n = take.shape[0]
    if n % 64:
        words[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))
    return words


def kth_radii(dist, take, k):
    """One radius per query around the masked k-th distance: at it, just below, just above, +inf, in turn."""
    kd = ks.unpack(ref.knn_keys(dist, take, k))[1][:, -1]                     # 100000 where fewer than k rows qualify
    r = kd.copy()
    r[1::4] = np.nextafter(kd[1::4], F32(-np.inf))
    r[2::4] = np.nextafter(kd[2::4], F32(np.inf))
    r[3::4] = F32(np.inf)
    return r.astype(F32)


class Fresh:
    """Oracle (b): the compacted gallery as a handle of its own, its answers mapped back."""

    def __init__(self, fir, rows, labels, metric, take):
        self.sel = np.flatnonzero(take)
        self.g = None
        if self.sel.shape[0]:
            self.g = fir.Gallery(np.ascontiguousarray(rows[self.sel]), None if labels is None else labels[self.sel], metric, 0)

    def close(self):
        if self.g is not None:
            self.g.close()

    def back(self, idx, dist, off):
        return ref.map_back(host_keys(idx, dist), self.sel, off)

    def top1(self, q, start, end, off=0):
        if self.g is None:
            return np.full(q.shape[0], NONE, np.uint64)
        return self.back(*self.g.search_top1(q, start, end), off)

    def knn(self, q, k, start, end, off=0):
        if self.g is None:
            return np.full((q.shape[0], k), NONE, np.uint64)
        return self.back(*self.g.search_knn(q, k, start, end), off)

    def radius(self, q, radius, m, start, end, off=0):
        if self.g is None:
            return np.zeros(q.shape[0], I32), np.full((q.shape[0], m), NONE, np.uint64)
        cnt, idx, dist = self.g.search_radius(q, radius, m, start, end)
        return cnt, (self.back(idx, dist, off) if m else np.zeros((q.shape[0], 0), np.uint64))

    def classes(self, q, nc, k, start, end, off=0):
        if self.g is None:
            return np.full((q.shape[0], k), NONE, np.uint64), np.full((q.shape[0], k), -1, I32)
        cls, idx, dist = self.g.search_top_classes(q, nc, k, start, end)
        return self.back(idx, dist, off), cls


def check_rows_calls(g, fresh, q, take, mask_arg, dist, start, end, off, tag, ks_=(1, 9), ms=(0, 8)):
    """Masked top-1, kNN and radius of one (handle, mask, range, batch) against both oracles."""
    got = host_keys(*g.search_top1_masked(q, mask_arg, start, end))
    assert np.array_equal(got, ref.top1_keys(dist, take, off)), ("top1 (a)",) + tag
    assert np.array_equal(got, fresh.top1(q, start, end, off)), ("top1 (b)",) + tag
    for k in ks_:
        idx, dd = g.search_knn_masked(q, mask_arg, k, start, end)
        assert idx.shape == dd.shape == (q.shape[0], k)
        got = host_keys(idx, dd)
        assert np.array_equal(got, ref.knn_keys(dist, take, k, off)), ("knn (a)", k) + tag
        assert np.array_equal(got, fresh.knn(q, k, start, end, off)), ("knn (b)", k) + tag
    radii = kth_radii(dist, take, 5)
    for m in ms:
        cnt, idx, dd = g.search_radius_masked(q, mask_arg, radii, m, start, end)
        wc, wk = ref.radius_keys(dist, take, radii, m, off)
        bc, bk = fresh.radius(q, radii, m, start, end, off)
        assert np.array_equal(cnt, wc) and np.array_equal(cnt, bc), ("radius counts", m) + tag
        if m:
            got = host_keys(idx, dd)
            assert np.array_equal(got, wk) and np.array_equal(got, bk), ("radius keys", m) + tag
        else:
            assert idx is None and dd is None


@pytest.mark.parametrize("d", (5, 64, 100))
@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_rows_ranges_metrics_batch_sizes_and_masks(fir, metric, d):
    """The mask word at the tile edge (n around 64 and 128), chunks at the range edges, part-full query tiles, skipped and read tiles."""
    for n in (1, 63, 64, 65, 129, 1000):
        rows = synth.make_gallery(401 + n, n, d, metric)
        q, _ = synth.make_queries(405 + n, rows, max(QBS), metric)
        names = ("half", "zero words", "last") if n != 129 else tuple(masks_of(n, 0))
        with fir.Gallery(rows, None, metric, 0) as g:
            dists = {r: g.range_distances(q, *r) for r in ranges_of(d)}
            for name in names:
                take = masks_of(n, 407 + n)[name]
                fresh = Fresh(fir, rows, None, metric, take)
                for (start, end), dist in dists.items():
                    for qb in QBS:
                        # all five batch sizes through top-1 and kNN; the radius calls with the two that differ in their tiles
                        check_rows_calls(g, fresh, q[:qb], take, take, dist[:qb], start, end, 0, (metric, n, d, name, start, end, qb),
                                         ks_=(9,), ms=(8,) if qb in (3, 17) else ())
                fresh.close()


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_every_mask_shape_garbage_bits_and_the_unmasked_bytes(fir, metric):
    n, d, qb = 1000, 64, 9
    rows = synth.make_gallery(411, n, d, metric)
    q, _ = synth.make_queries(412, rows, qb, metric)
    with fir.Gallery(rows, None, metric, 0) as g:
        dist = g.range_distances(q, 3, 61)
        for name, take in masks_of(n, 413).items():
            fresh = Fresh(fir, rows, None, metric, take)
            for arg in (take, fir.pack_row_mask(take), with_garbage(take)):      # bools, packed words, packed words with bits past n
                check_rows_calls(g, fresh, q, take, arg, dist, 3, 61, 0, (metric, name, arg.dtype))
            fresh.close()
            if name == "zeros":
                idx, dd = g.search_knn_masked(q, take, 8, 3, 61)
                assert np.all(idx == -1) and np.all(dd == F32(100000.0))
                cnt, _, _ = g.search_radius_masked(q, take, np.inf, 8, 3, 61)
                assert np.all(cnt == 0)
                idx, dd = g.search_top1_masked(q, take, 3, 61)
                assert np.all(idx == -1) and np.all(dd == F32(100000.0))
        # all ones: the unmasked calls' bytes
        ones = np.ones(n, bool)
        for a, b in zip(g.search_top1_masked(q, ones, 3, 61), g.search_top1(q, 3, 61)):
            assert a.tobytes() == b.tobytes()
        for k in (1, 8, 64):
            for a, b in zip(g.search_knn_masked(q, ones, k, 3, 61), g.search_knn(q, k, 3, 61)):
                assert a.tobytes() == b.tobytes()
        for a, b in zip(g.search_knn_masked(q, ones, 5, 3, 61), g.search_topk(q, 5, 3, 61)):      # k <= 8: also the masked top-K
            assert a.tobytes() == b.tobytes()
        radii = kth_radii(dist, ones, 20)
        for a, b in zip(g.search_radius_masked(q, ones, radii, 8, 3, 61), g.search_radius(q, radii, 8, 3, 61)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("metric", (CHI2, KL))
def test_a_negative_gallery_value_takes_the_full_division_sequence(fir, metric):
    """Chi-square / KL operands outside the plain range: the other kernel of the pair answers, masked the same way."""
    n, d, qb = 129, 64, 9
    rows = synth.make_gallery(421, n, d, metric)
    rows[77, 13] = F32(-0.001)
    labels = permuted(n, 5, 422)
    q, _ = synth.make_queries(423, rows, qb, metric)
    take = masks_of(n, 424)["zero words"]
    take[77] = True
    with fir.Gallery(rows, labels, metric, 0) as g:
        assert g.value_range()[0] is False
        fresh = Fresh(fir, rows, labels, metric, take)
        for start, end in ranges_of(d):
            dist = g.range_distances(q, start, end)
            check_rows_calls(g, fresh, q, take, take, dist, start, end, 0, (metric, start, end))
            kc, cc = ref.class_keys(dist, take, labels, 5, 3)
            cls, idx, dd = g.search_top_classes_masked(q, take, 5, 3, start, end)
            assert np.array_equal(host_keys(idx, dd), kc) and np.array_equal(cls, cc), (metric, start, end)
        fresh.close()


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_every_instantiation_through_the_tuning(fir, metric):
    """queries_per_pass 1, 2, 4, 8 pick the tile of the top-1 and store passes; one workgroup and three: a wave then walks many tiles,
    zero words between non-zero ones inside its stride. The dispatch record names the masked kernel that ran."""
    d, qb = 100, 17
    for n in (1000, 20000):
        rows = synth.make_gallery(431 + n, n, d, metric)
        q, _ = synth.make_queries(433, rows, qb, metric)
        take = random_half(n, 434)
        for t in range(1, (n + 63) // 64, 3):                                  # every third word zero, the last tile among them or not
            take[64 * t:64 * t + 64] = False
        with fir.Gallery(rows, None, metric, 0) as g:
            dist = g.range_distances(q, 3, 61)
            want1, want9 = ref.top1_keys(dist, take), ref.knn_keys(dist, take, 9)
            radii = kth_radii(dist, take, 5)
            wc, wk = ref.radius_keys(dist, take, radii, 8)
            seen = set()
            for qpp in (1, 2, 4, 8, 16):
                for waves in (0, 4, 12):
                    g.set_tuning(qpp, waves)
                    assert np.array_equal(host_keys(*g.search_top1_masked(q, take, 3, 61)), want1), (metric, n, qpp, waves)
                    ld = g.last_dispatch()
                    assert ld["path"] == "scan" and ld["kernel"].startswith("fir::k_scan<") and ld["kernel"].endswith(", 0, 8, 4, 0, 1>"), ld
                    g.search_top1_masked(q[:min(qpp, 8)], take, 3, 61)             # one whole tile of the size asked for: its kernel is the record
                    seen.add(g.last_dispatch()["kernel"])
                    assert np.array_equal(host_keys(*g.search_knn_masked(q, take, 9, 3, 61)), want9), (metric, n, qpp, waves)
                    cnt, idx, dd = g.search_radius_masked(q, take, radii, 8, 3, 61)
                    assert np.array_equal(cnt, wc) and np.array_equal(host_keys(idx, dd), wk), (metric, n, qpp, waves)
            assert {k.split("<")[1].split(",")[0] for k in seen} == {"1", "2", "4", "8"}, seen      # tiles of 1, 2, 4 and 8 queries all ran


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_ties_nan_rows_cutoff_row_offset_and_the_nearest_row_outside(fir, metric):
    n, d = 300, 64
    rows = synth.make_gallery(441, n, d, metric)
    q, _ = synth.make_queries(442, rows, 8, metric)
    rows[55] = rows[40]                                                        # query 0 = row 40, copied to rows 55, 100 and 250
    rows[100] = rows[40]
    rows[250] = rows[40]
    q[0] = rows[40]
    rows[101, 5] = np.nan                                                      # a NaN row inside the mask: never an answer
    q[1] = rows[101]
    q[1, 5] = rows[102, 5]
    big = rows.copy()
    big[200:] *= F32(1.0e7)                                                    # rows at distance >= 100000 (L2), or simply far
    take = random_half(n, 443)
    take[[55, 100, 101, 250]] = True
    take[40] = False                                                           # the nearest row of query 0 is outside the mask
    take[200:232] = True
    for gal in (rows, big):
        with fir.Gallery(gal, None, metric, 0) as g:
            fresh = Fresh(fir, gal, None, metric, take)
            for off in (0, 1 << 20):
                g.set_row_offset(off)
                dist = g.range_distances(q)
                check_rows_calls(g, fresh, q, take, take, dist, 0, 0, off, (metric, off, gal is big), ks_=(1, 9, 64), ms=(0, 8, 300))
                idx = g.search_top1_masked(q, take)[0]
                assert not np.any(idx == 40 + off)
                # (chi-square and KL pass over a feature whose sum is not > 0, a NaN included: only the L2 distance of row 101 is NaN)
                assert np.all(np.isnan(dist[:, 101])) == (metric == L2) and not np.any(idx[np.isnan(dist[:, 101])] == 101 + off)
                if gal is rows:
                    assert idx[0] == 55 + off                                  # the LOWEST masked-in copy
                    assert g.search_knn_masked(q[:1], take, 3)[0][0].tolist() == [55 + off, 100 + off, 250 + off]
            fresh.close()
            if gal is big and metric == L2:
                g.set_row_offset(0)
                assert np.all(g.range_distances(q[2:3])[0, 200:] >= F32(100000.0))
                far_only = np.zeros(n, bool)
                far_only[200:] = True                                          # every masked-in row at or beyond the cut-off: no answer
                assert np.all(g.search_top1_masked(q[2:3], far_only)[0] == -1)
                assert g.search_radius_masked(q[2:3], far_only, np.inf, 0)[0][0] == 0


def test_knn_sizes_and_radii_around_the_masked_kth_distance(fir):
    n, d, qb = 1000, 64, 9
    rows = synth.make_gallery(451, n, d, L2)
    q, _ = synth.make_queries(452, rows, qb, L2)
    with fir.Gallery(rows, None, L2, 0) as g:
        dist = g.range_distances(q)
        for take in (random_half(n, 453), masks_of(n, 454)["zero words"], np.arange(n) % 50 == 7):    # populations ~500, ~400 and 20
            fresh = Fresh(fir, rows, None, L2, take)
            for k in (1, 8, 9, 64, 1024):                                      # 1024 is more than any of the masks holds
                got = host_keys(*g.search_knn_masked(q, take, k))
                assert np.array_equal(got, ref.knn_keys(dist, take, k)) and np.array_equal(got, fresh.knn(q, k, 0, 0)), (k, int(take.sum()))
                assert np.all((got != NONE).sum(axis=1) == min(k, int(take.sum())))
            for kk in (3, 20):
                radii = kth_radii(dist, take, kk)
                for m in (0, 8, 300):
                    cnt, idx, dd = g.search_radius_masked(q, take, radii, m)
                    wc, wk = ref.radius_keys(dist, take, radii, m)
                    bc, bk = fresh.radius(q, radii, m, 0, 0)
                    assert np.array_equal(cnt, wc) and np.array_equal(cnt, bc), (kk, m)
                    if m:
                        assert np.array_equal(host_keys(idx, dd), wk) and np.array_equal(wk, bk), (kk, m)
            fresh.close()


@pytest.mark.parametrize("metric", (L2, CHI2, KL))
def test_classes(fir, metric):
    d, qb = 64, 17
    for n, labelling in ((129, "runs"), (1000, "runs"), (1000, "permuted"), (9000, "permuted")):     # 9000 rows: the sample bound runs first
        rows = synth.make_gallery(461 + n, n, d, metric)
        labels = runs_of_30(n) if labelling == "runs" else permuted(n, 40, 462)
        labels = labels.copy()
        labels[5::97] = -3                                                     # labels outside [0, num_classes) take no part
        labels[6::97] = 1 << 20
        nc = int(labels[(labels >= 0) & (labels < (1 << 20))].max()) + 1
        q, _ = synth.make_queries(463, rows, qb, metric)
        masks = {"half": random_half(n, 464), "zero words": masks_of(n, 465)["zero words"], "zeros": np.zeros(n, bool), "ones": np.ones(n, bool),
                 "class 2 masked out": labels != 2}
        with fir.Gallery(rows, labels, metric, 0) as g:
            dist = g.range_distances(q, 3, 61)
            for name, take in masks.items():
                fresh = Fresh(fir, rows, labels, metric, take)
                for k in (1, 5, 32):
                    for num_classes in (nc, max(nc - 2, 1)):
                        cls, idx, dd = g.search_top_classes_masked(q, take, num_classes, k, 3, 61)
                        kc, cc = ref.class_keys(dist, take, labels, num_classes, k)
                        bk, bc = fresh.classes(q, num_classes, k, 3, 61)
                        tag = (metric, n, labelling, name, k, num_classes)
                        assert np.array_equal(host_keys(idx, dd), kc) and np.array_equal(cls, cc), ("(a)",) + tag
                        assert np.array_equal(kc, bk) and np.array_equal(cc, bc), ("(b)",) + tag
                        if name == "class 2 masked out":
                            assert not np.any(cls == 2)
                ld = g.last_dispatch()
                assert ld["path"] == "scan" and ", 5, 8, " in ld["kernel"] and ld["kernel"].endswith(", 0, 1>"), ld
                fresh.close()
            ones = np.ones(n, bool)
            for a, b in zip(g.search_top_classes_masked(q, ones, nc, 5, 3, 61), g.search_top_classes(q, nc, 5, 3, 61)):
                assert a.tobytes() == b.tobytes()


class DevBuf:
    """A poisoned device buffer of 64-bit (or 32-bit) words with a tail of canaries, filled before anything else is queued."""

    def __init__(self, words, dtype=torch.int64):
        self.words = words
        self.poison = POISON if dtype == torch.int64 else 0x5A5A5A5A
        self.t = torch.full((words + 8,), self.poison, dtype=dtype, device=DEV)
        torch.cuda.synchronize()

    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        a = self.t.cpu().numpy()
        assert np.all(a[self.words:] == self.poison)                            # nothing written past the end
        a = a[: self.words].copy()
        return a.view(np.uint64) if a.dtype == np.int64 else a


def dev_mask(fir, take):
    return torch.from_numpy(fir.pack_row_mask(take).view(np.int64)).to(DEV)


def test_device_calls_streams_canaries_and_a_mask_built_on_the_stream(fir):
    n, d, qb, k, m, nc = 1000, 100, 17, 9, 8, 40
    rows = synth.make_gallery(471, n, d, L2)
    labels = permuted(n, nc, 472)
    q, _ = synth.make_queries(473, rows, qb, L2)
    take = masks_of(n, 474)["zero words"]
    qt, mt = torch.from_numpy(q).to(DEV), dev_mask(fir, take)
    with fir.Gallery(rows, labels, L2, 0) as g:
        dist, dist_r = g.range_distances(q), g.range_distances(q, 3, 61)
        radii = kth_radii(dist, take, 5)
        rt = torch.from_numpy(radii).to(DEV)

        def all_calls(take_, mask_ptr, start, end, stream, dd):
            o1, ok, oc, ork, ock, occ = DevBuf(qb), DevBuf(qb * k), DevBuf(qb, torch.int32), DevBuf(qb * m), DevBuf(qb * 5), DevBuf(qb * 5, torch.int32)
            g.search_top1_masked_keys_dev(qt.data_ptr(), qb, mask_ptr, o1.ptr(), start, end, stream=stream)
            g.search_knn_masked_keys_dev(qt.data_ptr(), qb, mask_ptr, k, ok.ptr(), start, end, stream=stream)
            g.search_radius_masked_keys_dev(qt.data_ptr(), qb, mask_ptr, rt.data_ptr(), m, oc.ptr(), ork.ptr(), start, end, stream=stream)
            g.search_top_classes_masked_keys_dev(qt.data_ptr(), qb, mask_ptr, nc, 5, ock.ptr(), occ.ptr(), start, end, stream=stream)

            def verify():
                assert np.array_equal(o1.read(), ref.top1_keys(dd, take_))
                assert np.array_equal(ok.read().reshape(qb, k), ref.knn_keys(dd, take_, k))
                wc, wk = ref.radius_keys(dd, take_, radii, m)
                assert np.array_equal(oc.read(), wc) and np.array_equal(ork.read().reshape(qb, m), wk)
                kc, cc = ref.class_keys(dd, take_, labels, nc, 5)
                assert np.array_equal(ock.read().reshape(qb, 5), kc) and np.array_equal(occ.read().reshape(qb, 5), cc)
            return verify

        v = all_calls(take, mt.data_ptr(), 0, 0, None, dist)                     # the handle's own stream
        g.sync()
        v()
        st = torch.cuda.Stream()                                               # a caller's stream
        v = all_calls(take, mt.data_ptr(), 3, 61, st.cuda_stream, dist_r)
        st.synchronize()
        v()
        # back to back on two streams: both use the handle's scratch, the second waits for the first
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        v1 = all_calls(take, mt.data_ptr(), 0, 0, s1.cuda_stream, dist)
        v2 = all_calls(take, mt.data_ptr(), 3, 61, s2.cuda_stream, dist_r)
        g.sync()
        s1.synchronize()
        s2.synchronize()
        v1()
        v2()
        # a mask produced on the same stream just before, nothing in between
        wanted = np.array(sorted([3, 3, 7, 11, 39, 1000]), I32)
        ct = torch.from_numpy(wanted).to(DEV)
        built = DevBuf(fir.mask_words(n))
        torch.cuda.synchronize()
        g.mask_of_classes_dev(ct.data_ptr(), wanted.shape[0], built.ptr(), invert=False, stream=st.cuda_stream)
        v = all_calls(np.isin(labels, wanted), built.ptr(), 0, 0, st.cuda_stream, dist)
        st.synchronize()
        v()
        assert np.array_equal(built.read(), ref.pack_bits(np.isin(labels, wanted)))
        # qb == 0: nothing to do, nothing written
        o0 = DevBuf(4)
        g.search_top1_masked_keys_dev(qt.data_ptr(), 0, mt.data_ptr(), o0.ptr())
        g.search_knn_masked_keys_dev(qt.data_ptr(), 0, mt.data_ptr(), 3, o0.ptr())
        g.sync()
        assert np.all(o0.read() == np.uint64(POISON))


@pytest.mark.parametrize("metric", (L2, CHI2))
def test_the_gates_do_not_fire(fir, metric):
    """70 000 x 64 rows and 128 queries: an unmasked call of this shape goes to the matrix cores (L2) or the nomination lists
    (chi-square). A masked one takes the exact scan, under the default settings and under a caller's threshold of 8 queries."""
    n, d, qb = 70000, 64, 128
    rows = synth.make_gallery(481, n, d, metric)
    labels = permuted(n, 700, 482)
    q, _ = synth.make_queries(483, rows, qb, metric)
    with fir.Gallery(rows, labels, metric, 0) as g:
        dist = g.range_distances(q)
        winners = ks.unpack(ref.top1_keys(dist, np.ones(n, bool)))[0]
        take = random_half(n, 484) | (np.arange(n) < 4096)
        take[64 * 100:64 * 300] = False                                        # two hundred skipped tiles
        take[winners] = False                                                  # every query's unmasked winner is masked out
        want1, want9 = ref.top1_keys(dist, take), ref.knn_keys(dist, take, 9)
        kc, cc = ref.class_keys(dist, take, labels, 700, 5)
        assert not np.any(np.isin(ks.unpack(want1)[0], winners))
        for threshold in (None, 8):
            if threshold is not None:
                g.set_large_batch_mfma(threshold)
            before = g.mfma_stats()
            got = host_keys(*g.search_top1_masked(q, take))
            ld = g.last_dispatch()
            assert ld["path"] == "scan" and ld["kernel"].startswith("fir::k_scan<") and ld["kernel"].endswith(", 0, 1>") and ", 0, 8, " in ld["kernel"], ld
            assert np.array_equal(got, want1), (metric, threshold)
            assert np.array_equal(host_keys(*g.search_knn_masked(q, take, 9)), want9), (metric, threshold)
            cls, idx, dd = g.search_top_classes_masked(q, take, 700, 5)
            ld = g.last_dispatch()
            assert ld["path"] == "scan" and ", 5, 8, " in ld["kernel"] and ld["kernel"].endswith(", 0, 1>"), ld
            assert np.array_equal(host_keys(idx, dd), kc) and np.array_equal(cls, cc), (metric, threshold)
            assert g.mfma_stats() == before, (metric, threshold)


def test_inverted_class_mask_is_the_other_class_search(fir):
    n, d, qb = 1000, 64, 17
    rows = synth.make_gallery(491, n, d, L2)
    labels = permuted(n, 9, 492)
    q, _ = synth.make_queries(493, rows, qb, L2)
    with fir.Gallery(rows, labels, L2, 0) as g:
        g.set_large_batch_mfma(0)
        for c in (0, 4, 8, 77):
            mask = g.mask_of_classes([c], invert=True)
            a = g.search_top1_masked(q, mask, 3, 61)
            b = g.search_top1_other_class(q, c, 3, 61)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), c


def test_mask_of_classes(fir):
    for n in (1, 63, 64, 65, 130, 1000):
        labels = permuted(n, 12, 501 + n) - 4
        labels[::7] = I32_MIN
        labels[3::11] = I32_MAX
        lists = ([], [0], [-4, 7, 7, -1], [I32_MIN], [I32_MAX, I32_MIN, 2, 2, 2], [100, -100], list(range(-4, 8)))
        rows = synth.make_gallery(502, n, 8, L2)
        with fir.Gallery(rows, labels, L2, 0) as g:
            for classes in lists:
                for invert in (False, True):
                    want = np.isin(labels, np.array(classes, I32)) != invert
                    got = g.mask_of_classes(classes, invert)
                    assert got.dtype == np.uint64 and got.shape == (fir.mask_words(n),)
                    assert np.array_equal(got, ref.pack_bits(want)), (n, classes, invert)      # pack_bits leaves the tail bits zero
                    srt = np.sort(np.array(classes, I32))
                    ct = torch.from_numpy(srt).to(DEV) if srt.shape[0] else None
                    out = DevBuf(fir.mask_words(n))
                    g.mask_of_classes_dev(ct.data_ptr() if ct is not None else None, srt.shape[0], out.ptr(), invert)
                    g.sync()
                    assert np.array_equal(out.read(), ref.pack_bits(want)), (n, classes, invert)
    with fir.Gallery(synth.make_gallery(503, 10, 8, L2), None, L2, 0) as g:
        with pytest.raises(fir.FirError) as e:
            g.mask_of_classes([1])
        assert e.value.code == ERR_STATE and "without class labels" in str(e.value)
        out = DevBuf(1)
        ct = torch.zeros(1, dtype=torch.int32, device=DEV)
        with pytest.raises(fir.FirError) as e:
            g.mask_of_classes_dev(ct.data_ptr(), 1, out.ptr())
        assert e.value.code == ERR_STATE
        g.sync()
        assert np.all(out.read() == np.uint64(POISON))


def test_masks_after_in_place_updates(fir):
    n, d, qb, nc = 200, 64, 9, 12
    rows = synth.make_gallery(511, n + 70, d, L2)
    labels = permuted(n + 70, nc, 512)
    q, _ = synth.make_queries(513, rows, qb, L2)
    with fir.Gallery(rows[:n], labels[:n], L2, 0) as g:
        g.reserve(1000)
        g.append(rows[n:], labels[n:])
        g.remove_rows([3, 150, 268])
        g.set_rows([10, 200], rows[[5, 6]] * F32(0.5), np.array([1, 2], I32))
        cur, cur_labels = g.read_rows(with_classes=True)
        assert g.n == cur.shape[0] == n + 67 and g.capacity() >= 1000
        for take in (random_half(g.n, 514), masks_of(g.n, 515)["zero words"], np.ones(g.n, bool)):
            fresh = Fresh(fir, cur, cur_labels, L2, take)
            dist = g.range_distances(q)
            check_rows_calls(g, fresh, q, take, with_garbage(take), dist, 0, 0, 0, ("after updates", int(take.sum())), ms=(0, 8, 300))
            cls, idx, dd = g.search_top_classes_masked(q, take, nc, 5)
            bk, bc = fresh.classes(q, nc, 5, 0, 0)
            assert np.array_equal(host_keys(idx, dd), bk) and np.array_equal(cls, bc)
            fresh.close()
        assert np.array_equal(g.mask_of_classes([1, 2]), ref.pack_bits(np.isin(cur_labels, [1, 2])))


def test_argument_errors_queue_nothing_and_leave_the_next_call_intact(fir):
    n, d = 100, 16
    rows = synth.make_gallery(521, n, d, L2)
    q = rows[:3].copy()
    labels = runs_of_30(n)
    L = fir.lib()
    p = lambda a: a.ctypes.data_as(fir.capi._vp)
    idx, dist, cnt, cls = np.full(3 * 8, 77, I32), np.full(3 * 8, 7.0, F32), np.full(3, 77, I32), np.full(3 * 8, 77, I32)
    rad = np.ones(3, F32)
    mask = fir.pack_row_mask(np.arange(n) % 2 == 0)

    def err(rc, code, text):
        assert rc == code and text in L.fir_last_error().decode(), (rc, L.fir_last_error())

    with fir.Gallery(rows, labels, L2, 0) as g:
        h = g._h
        good = g.search_top1(q)
        # NULL mask with n > 0, among the NULL checks (before qb < 0 and k)
        err(L.fir_search_top1_masked(h, p(q), 3, 0, 0, None, p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_masked(h, p(q), -1, 0, 0, None, p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_knn_masked(h, p(q), 3, 0, 0, None, 0, p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_radius_masked(h, p(q), 3, 0, 0, None, p(rad), 8, p(cnt), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top_classes_masked(h, p(q), 3, 0, 0, None, 4, 2, p(cls), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_masked_keys_dev(h, p(q), 3, 0, 0, None, p(idx), None), ERR_ARG, "NULL argument")
        err(L.fir_search_knn_masked_keys_dev(h, p(q), 3, 0, 0, None, 2, p(idx), None), ERR_ARG, "NULL argument")
        err(L.fir_search_radius_masked_keys_dev(h, p(q), 3, 0, 0, None, p(rad), 8, p(cnt), p(idx), None), ERR_ARG, "NULL argument")
        err(L.fir_search_top_classes_masked_keys_dev(h, p(q), 3, 0, 0, None, 4, 2, p(idx), p(cls), None), ERR_ARG, "NULL argument")
        # the siblings' order and messages
        err(L.fir_search_top1_masked(None, p(q), 3, 0, 0, p(mask), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_masked(h, None, 3, 0, 0, p(mask), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top1_masked(h, p(q), -1, 0, 0, p(mask), p(idx), p(dist)), ERR_ARG, "qb < 0")
        err(L.fir_search_top1_masked(h, p(q), 3, 5, 5, p(mask), p(idx), p(dist)), ERR_ARG, "feature range [5,5) not inside [0,16)")
        err(L.fir_search_knn_masked(h, p(q), 3, 0, 0, p(mask), 0, p(idx), p(dist)), ERR_ARG, "k=0 outside [1,1024]")
        err(L.fir_search_knn_masked(h, p(q), 3, 0, 0, p(mask), 1025, p(idx), p(dist)), ERR_ARG, "k=1025 outside [1,1024]")
        err(L.fir_search_knn_masked(h, p(q), 0, 0, 0, p(mask), 0, p(idx), p(dist)), ERR_ARG, "k=0 outside")                 # k before qb == 0
        err(L.fir_search_knn_masked(h, p(q), 3, 0, 0, p(mask), 3, None, p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_knn_masked(h, p(q), 3, 0, 17, p(mask), 3, p(idx), p(dist)), ERR_ARG, "feature range [0,17)")
        err(L.fir_search_radius_masked(h, p(q), 3, 0, 0, p(mask), p(rad), 1025, p(cnt), p(idx), p(dist)), ERR_ARG, "max_results=1025 outside [0,1024]")
        err(L.fir_search_radius_masked(h, p(q), 3, 0, 0, p(mask), p(rad), -1, p(cnt), None, None), ERR_ARG, "max_results=-1 outside [0,1024]")
        err(L.fir_search_radius_masked(h, p(q), 3, 0, 0, p(mask), p(rad), 0, p(cnt), p(idx), p(dist)), ERR_ARG, "NULL argument")   # count-only: no idx / dist
        err(L.fir_search_radius_masked(h, p(q), 3, 0, 0, p(mask), p(rad), 8, None, p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_radius_masked(h, p(q), 3, 0, 0, p(mask), None, 8, p(cnt), p(idx), p(dist)), ERR_ARG, "NULL argument")
        err(L.fir_search_top_classes_masked(h, p(q), 3, 0, 0, p(mask), 4, 0, p(cls), p(idx), p(dist)), ERR_ARG, "k=0 outside [1,32]")
        err(L.fir_search_top_classes_masked(h, p(q), 3, 0, 0, p(mask), 0, 2, p(cls), p(idx), p(dist)), ERR_ARG, "num_classes=0 outside")
        err(L.fir_search_top_classes_masked(h, p(q), 0, 0, 17, p(mask), 4, 2, p(cls), p(idx), p(dist)), ERR_ARG, "feature range [0,17)")   # the range before qb == 0
        err(L.fir_search_top_classes_masked_keys_dev(h, p(q), 3, 0, 0, p(mask), 4, 2, None, None, None), ERR_ARG, "both NULL")
        err(L.fir_gallery_mask_of_classes(h, None, 2, 0, p(mask)), ERR_ARG, "NULL argument")
        err(L.fir_gallery_mask_of_classes(h, p(cls), 2, 0, None), ERR_ARG, "NULL argument")
        err(L.fir_gallery_mask_of_classes(h, p(cls), -1, 0, p(mask)), ERR_ARG, "m < 0")
        assert L.fir_search_top1_masked(h, None, 0, 0, 0, p(mask), p(idx), p(dist)) == 0                                       # nothing to do
        # nothing was written by any of them, and the next unmasked call answers as before
        assert np.all(idx == 77) and np.all(dist == F32(7.0)) and np.all(cnt == 77) and np.all(cls == 77)
        again = g.search_top1(q)
        assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
        assert np.array_equal(g.search_top1_masked(q, np.ones(n, bool))[0], good[0])
        with pytest.raises(ValueError):
            g.search_top1_masked(q, np.ones(n + 1, bool))
    with fir.Gallery(rows, None, L2, 0) as g:                                   # no labels: the class call is FIR_ERR_STATE, the others work
        err(L.fir_search_top_classes_masked(g._h, p(q), 3, 0, 0, p(mask), 4, 2, p(cls), p(idx), p(dist)), ERR_STATE, "without class labels")
        assert np.all(g.search_top1_masked(q, np.arange(n) >= 3)[0] >= 3)
    # an empty gallery: the mask is not read, NULL is accepted, the unmasked empty-gallery results apply
    with fir.Gallery(np.zeros((0, d), F32), np.zeros(0, I32), L2, 0) as g:
        h = g._h
        assert L.fir_search_top1_masked(h, p(q), 3, 0, 0, None, p(idx), p(dist)) == 0
        assert np.all(idx[:3] == -1) and np.all(dist[:3] == F32(100000.0))
        assert L.fir_search_knn_masked(h, p(q), 3, 0, 0, None, 4, p(idx), p(dist)) == 0
        assert np.all(idx[:12] == -1)
        assert L.fir_search_radius_masked(h, p(q), 3, 0, 0, None, p(rad), 2, p(cnt), p(idx), p(dist)) == 0
        assert np.all(cnt == 0)
        assert L.fir_search_top_classes_masked(h, p(q), 3, 0, 0, None, 4, 2, p(cls), p(idx), p(dist)) == 0
        assert np.all(cls[:6] == -1)
        assert L.fir_gallery_mask_of_classes(h, p(cls), 2, 0, None) == 0
        assert g.mask_of_classes([1, 2]).shape == (0,)
