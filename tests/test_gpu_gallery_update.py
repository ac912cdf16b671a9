"""In-place gallery updates (fir_gallery_append / _append_dev / _set_rows / _remove_rows / _reserve / _read_rows). No expected value
comes from the code under test: the yardstick is a handle fresh from fir_gallery_create over the numpy array that
gallery_update_ref.RefGallery produces from the same operations, compared bit for bit (np.array_equal on bytes / uint64 keys)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gallery_update_ref as ref
import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
L2, CHI2, KL = 0, 1, 2
ERR_ARG, ERR_STATE = -1, -5
POISON64 = 0xA5A5A5A5A5A5A5A5 - (1 << 64)
F32, I32 = np.float32, np.int32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    if isinstance(want, (tuple, list)):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if want is None:
        return got is None
    return np.array_equal(bits(np.asarray(got)), bits(np.asarray(want)))


def labels_for(n, seed, classes=7):
    return (synth.splitmix64(np.arange(n, dtype=np.uint64), seed) % np.uint64(classes)).astype(I32)


def read_all(g, labelled):
    return g.read_rows(0, None, with_classes=labelled)


def assert_holds(g, r, what=""):
    """The handle holds exactly the reference's rows (and labels)."""
    assert g.n == r.n, (what, g.n, r.n)
    if r.n == 0:
        return
    got = read_all(g, r.labels is not None)
    if r.labels is not None:
        assert same(got[0], r.rows) and np.array_equal(got[1], r.labels), what
    else:
        assert same(got, r.rows), what


def padding_words(fir, g):
    fn = fir.lib().fir_gallery_padding_words_
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    w = C.c_int64(-1)
    assert fn(g._h, C.byref(w)) == 0
    return w.value


def append_dev(g, rows, labels):
    """Through device memory on a caller's stream; the sources are overwritten behind the call in stream order and freed only after
    the stream has passed them."""
    st = torch.cuda.Stream()
    src = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(DEV) if labels is not None else None
    st.wait_stream(torch.cuda.current_stream())
    g.append_dev(src.data_ptr(), rows.shape[0], lab.data_ptr() if lab is not None else None, stream=st.cuda_stream)
    with torch.cuda.stream(st):
        src.fill_(float("nan"))
        if lab is not None:
            lab.fill_(-77)
    st.synchronize()
    del src, lab


# ---- 1. tile seams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", (0, 1, 63, 64, 65, 130))
@pytest.mark.parametrize("d", (5, 64, 100))
def test_appends_across_tile_seams(fir, d, n0):
    pool = synth.make_gallery(400 + d, n0 + 2 * 200, d, L2)
    lab = labels_for(pool.shape[0], 401)
    for m in (1, 63, 64, 65, 200):
        for k, mode in enumerate(("host", "dev", "two")):
            labelled = (m + k) % 2 == 0
            r = ref.RefGallery(pool[:n0], lab[:n0] if labelled else None)
            with fir.Gallery(pool[:n0], lab[:n0] if labelled else None, L2, 0) as g:
                steps = [(n0, m)] if mode != "two" else [(n0, m // 2 + 1), (n0 + m // 2 + 1, m)]
                for i, (a, cnt) in enumerate(steps):
                    rows, ll = pool[a:a + cnt], lab[a:a + cnt] if labelled else None
                    if mode == "dev" or (mode == "two" and i == 1):
                        append_dev(g, rows, ll)
                    else:
                        g.append(rows, ll)
                    r.append(rows, ll)
                    assert_holds(g, r, (d, n0, m, mode, i))
                assert padding_words(fir, g) == 0
                # a window that starts inside a tile
                row0 = min(r.n - 1, max(1, n0 - 3))
                cnt = min(r.n - row0, 70)
                got = g.read_rows(row0, cnt, with_classes=labelled)
                assert same(got[0] if labelled else got, r.rows[row0:row0 + cnt]), (d, n0, m, mode)
                if labelled:
                    assert np.array_equal(got[1], r.labels[row0:row0 + cnt])
                # and it answers as the array does: every appended row finds itself
                idx, dist = g.search_top1(r.rows[n0:])
                assert same((idx, dist), fresh_top1(fir, r, r.rows[n0:])), (d, n0, m, mode)


def fresh_top1(fir, r, q):
    with fir.Gallery(r.rows, r.labels, L2, 0) as f:
        return f.search_top1(q)


# ---- 2. the layout invariant -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", (0, 1, 63))
@pytest.mark.parametrize("d", (5, 64))
def test_padding_stays_zero(fir, d, res):
    n0 = 128 + res
    pool = synth.make_gallery(500 + d, n0 + 1500, d, L2) + F32(0.25)        # no zero anywhere: a stray row shows
    lab = labels_for(pool.shape[0], 501)
    r = ref.RefGallery(pool[:n0], lab[:n0])
    with fir.Gallery(pool[:n0], lab[:n0], L2, 0) as g:
        assert padding_words(fir, g) == 0
        at = n0

        def app(m):
            nonlocal at
            g.append(pool[at:at + m], lab[at:at + m])
            r.append(pool[at:at + m], lab[at:at + m])
            at += m

        g.reserve(n0 + 64)                                       # a growth by reserve
        assert padding_words(fir, g) == 0 and g.n % 64 == res
        app(64)                                                  # an append into reserved room
        assert padding_words(fir, g) == 0 and g.n % 64 == res
        cap = g.capacity()
        app(((cap - g.n) // 64 + 10) * 64)                       # an append that grows the buffer
        assert g.capacity() > cap and padding_words(fir, g) == 0 and g.n % 64 == res
        sel = np.array([0, 63, 64, g.n - 1, g.n - 65], I32)
        g.set_rows(sel, pool[at:at + 5])
        r.set_rows(sel, pool[at:at + 5])
        assert padding_words(fir, g) == 0
        rng = np.random.default_rng(d + res)
        for m in (64, 128 + 64):                                 # removals: holes, tail rows, whole tiles vacated
            drop = np.concatenate([rng.choice(g.n - m, m // 2, replace=False), g.n - 1 - rng.choice(m, m - m // 2, replace=False)]).astype(I32)
            moved = g.remove_rows(drop)
            assert np.array_equal(moved, r.remove_rows(drop))
            assert padding_words(fir, g) == 0 and g.n % 64 == res
        app(70)                                                  # rows written where removed ones were cleared
        assert padding_words(fir, g) == 0
        assert_holds(g, r)


# ---- 3. equivalence of answers ---------------------------------------------------------------------------------------------------
def mutate(fir, g, r, pool, lab, n0, sizes):
    """append -> set_rows (with and without labels) -> remove_rows -> append (device). Returns the planted queries."""
    a1, nset, nrem, a2 = sizes
    at = n0
    planted = []
    rows, ll = pool[at:at + a1].copy(), lab[at:at + a1]
    rows[0] = r.rows[min(3, n0 - 1)]                              # a duplicate across the seam: the lower row wins
    g.append(rows, ll)
    r.append(rows, ll)
    at += a1
    planted += [rows[0], rows[1]]
    keep = {min(3, n0 - 1), n0, n0 + 1, 1}                        # rows the planted queries look for: not overwritten (but row 1), not removed
    sel = np.array(sorted({1} | ({n0 - 1, n0 + 2, r.n - 1, r.n // 2 + 7} - keep))[:nset], I32)
    assert sel[0] == 1
    planted += [r.rows[sel[0]].copy(), pool[at].copy()]           # an overwritten row's old and new value
    half = len(sel) // 2
    g.set_rows(sel[:half], pool[at:at + half], lab[at:at + half])
    r.set_rows(sel[:half], pool[at:at + half], lab[at:at + half])
    g.set_rows(sel[half:], pool[at + half:at + len(sel)])
    r.set_rows(sel[half:], pool[at + half:at + len(sel)])
    at += len(sel)
    rng = np.random.default_rng(n0)
    head = np.setdiff1d(np.arange(r.n - nrem), sorted(keep))
    drop = np.concatenate([rng.choice(head, nrem - nrem // 3, replace=False), r.n - 1 - rng.choice(nrem, nrem // 3, replace=False)]).astype(I32)
    planted.append(r.rows[drop[0]].copy())                        # a removed row
    moved = g.remove_rows(drop)
    assert np.array_equal(moved, r.remove_rows(drop)) and (moved >= 0).any()
    planted.append(r.rows[drop[np.argmax(moved >= 0)]].copy())    # a moved row, at its new place
    append_dev(g, pool[at:at + a2], lab[at:at + a2])
    r.append(pool[at:at + a2], lab[at:at + a2])
    planted.append(pool[at + a2 - 1].copy())
    return np.stack(planted)


def answers(g, q, ranges, ncls, ex, rows_sel, radius):
    out = {}
    for (s, e) in ranges:
        t = f"[{s},{e})"
        out["top1" + t] = g.search_top1(q, s, e)
        out["topk" + t] = g.search_topk(q, 5, s, e)
        out["knn" + t] = g.search_knn(q, 70, s, e)
        out["radius" + t] = g.search_radius(q, radius[(s, e)], 16, s, e)
        out["classes" + t] = g.search_top_classes(q, ncls, 3, s, e)
        out["other" + t] = g.search_top1_other_class(q, ex, s, e)
        out["self" + t] = g.other_class(s, e)
        out["far" + t] = tuple(np.asarray(v) for v in g.far_threshold(0.05, s, e))
        out["range" + t] = g.range_distances(q, s, e)
        out["rowsd" + t] = g.rows_distances(q, rows_sel, s, e)
    out["classes_of"] = g.classes_of(out["top1[0,0)"][0])
    return out


@pytest.mark.parametrize("metric,d,n0,sizes", [(L2, 64, 130, (70, 5, 40, 65)), (CHI2, 64, 130, (70, 5, 40, 65)), (KL, 64, 130, (70, 5, 40, 65)),
                                               (L2, 100, 63, (66, 4, 20, 1)), (CHI2, 5, 20, (10, 3, 5, 8)), (L2, 5, 20, (10, 3, 5, 8))])
def test_every_search_answers_as_a_fresh_handle(fir, metric, d, n0, sizes):
    pool = synth.make_gallery(600 + d + metric, n0 + 300, d, metric)
    lab = labels_for(pool.shape[0], 601)
    r = ref.RefGallery(pool[:n0], lab[:n0])
    ranges = [(0, 0), (3, 61), (4, 5)] if d >= 61 else [(0, 0), (4, 5)]
    with fir.Gallery(pool[:n0], lab[:n0], metric, 0) as g:
        g.search_top1(pool[:3])                                   # (a call before the mutations: whatever it cached is stale now)
        planted = mutate(fir, g, r, pool, lab, n0, sizes)
        q = np.concatenate([planted, synth.make_queries(602, r.rows, 17, metric)[0]])
        ex = labels_for(q.shape[0], 603)
        rows_sel = np.stack([(np.arange(6) * 7 + i) % r.n for i in range(q.shape[0])]).astype(I32)
        with fir.Gallery(r.rows, r.labels, metric, 0) as f:
            assert_holds(g, r)
            radius = {rg: np.ascontiguousarray(f.search_topk(q, 5, *rg)[1][:, 4]) for rg in ranges}
            want = answers(f, q, ranges, 7, ex, rows_sel, radius)
            got = answers(g, q, ranges, 7, ex, rows_sel, radius)
            for name in want:
                assert same(got[name], want[name]), (name, metric, d)
            # the winners sit where the mutation happened: a copy of a row finds a row at distance 0, the duplicate its lower twin
            idx, dist = got["top1[0,0)"]
            if metric != KL:
                assert np.all(dist[[0, 1, 3, 5, 6]] == 0), dist[:7]
            assert idx[0] == min(3, n0 - 1) and idx[1] == n0 + 1 and idx[3] == 1 and idx[6] == r.n - 1, idx[:7]
            assert r.rows[idx[5]].tobytes() == planted[5].tobytes()
            assert g.value_range()[0] == f.value_range()[0]


def test_twd_and_dem_after_updates(fir):
    d, n0 = 256, 150
    pool = synth.make_gallery(700, n0 + 300, d, L2)
    lab = labels_for(pool.shape[0], 701, 9)
    r = ref.RefGallery(pool[:n0], lab[:n0])
    with fir.Gallery(pool[:n0], lab[:n0], L2, 0) as g:
        planted = mutate(fir, g, r, pool, lab, n0, (60, 5, 30, 20))
        assert r.n == 200
        q = np.concatenate([planted, synth.make_queries(702, r.rows, 9, L2)[0]])
        with fir.Gallery(r.rows, r.labels, L2, 0) as f:
            for typ, th in ((0, 0.24), (1, 0.003), (2, 0.7)):
                assert same(g.twd_conventional(q, 9, typ, th, 64), f.twd_conventional(q, 9, typ, th, 64)), typ
            assert same(g.twd_proposed(q, 32, 0.7), f.twd_proposed(q, 32, 0.7))
            dg, df = fir.Dem(g, 7, 5), fir.Dem(f, 7, 5)             # made AFTER the mutations
            assert same(dg.get(), df.get())
            thr = float(np.median(df.get(False)[1]))
            for m in (0, 5, 40):
                assert same(dg.recognize(q, thr, m), df.recognize(q, thr, m)), m
            dg.close()
            df.close()


# ---- 4. the routed forms do not see stale copies ---------------------------------------------------------------------------------
def routed_batches(g, q, ncls):
    out = {}
    for name, call in (("top1", lambda: g.search_top1(q)), ("topk", lambda: g.search_topk(q, 5)), ("knn", lambda: g.search_knn(q, 9)),
                       ("classes", lambda: g.search_top_classes(q, ncls, 3))):
        out[name] = call()
        out[name + "/path"] = g.last_dispatch()["path"]
    return out


def test_routed_batches_after_updates(fir):
    n, d, qb = 4099, 64, 130
    pool = synth.make_gallery(800, n + 200, d, L2)
    lab = labels_for(pool.shape[0], 801, 37)
    r = ref.RefGallery(pool[:n], lab[:n])
    q, _ = synth.make_queries(802, pool[:n], qb, L2)
    with fir.Gallery(pool[:n], lab[:n], L2, 0) as g:
        g.set_large_batch_mfma(1)
        before = routed_batches(g, q, 37)                           # the states exist now
        assert all(before[k + "/path"] == "mfma" for k in ("top1", "topk", "knn", "classes")), before
        winner = int(before["top1"][0][4])
        g.append(pool[n:n + 70], lab[n:n + 70])
        r.append(pool[n:n + 70], lab[n:n + 70])
        q[10] = pool[n + 5]                                         # an appended row is the nearest of query 10
        sel = np.array([17, 2048, 4098], I32)
        new = np.stack([q[20], q[21], q[22]])                       # three rows become the nearest rows of three queries
        g.set_rows(sel, new, np.array([1, 2, 3], I32))
        r.set_rows(sel, new, np.array([1, 2, 3], I32))
        moved = g.remove_rows(np.array([winner], I32))              # a row that was a winner goes
        assert np.array_equal(moved, r.remove_rows(np.array([winner], I32)))
        got = routed_batches(g, q, 37)
        assert all(got[k + "/path"] == "mfma" for k in ("top1", "topk", "knn", "classes")), got
        g.set_large_batch_mfma(0)
        scan = routed_batches(g, q, 37)
        assert all(scan[k + "/path"] == "scan" for k in ("top1", "topk", "knn", "classes")), scan
        with fir.Gallery(r.rows, r.labels, L2, 0) as f:              # the fresh handle, routed as the mutated one was, and its scan
            f.set_large_batch_mfma(1)
            fresh = routed_batches(f, q, 37)
            assert all(fresh[k + "/path"] == "mfma" for k in ("top1", "topk", "knn", "classes")), fresh
            f.set_large_batch_mfma(0)
            want = routed_batches(f, q, 37)
        for k in ("top1", "topk", "knn", "classes"):
            assert same(got[k], fresh[k]) and same(got[k], want[k]) and same(scan[k], want[k]), k
        idx, dist = got["top1"]
        assert r.rows[idx[10]].tobytes() == pool[n + 5].tobytes() and dist[10] == 0        # the winners sit where the gallery changed
        assert np.all(dist[20:23] == 0) and set(idx[20:23].tolist()) <= {17, 2048, 4098, winner}
        assert not same(before["top1"], got["top1"])


def test_routed_int8_batches_after_updates(fir):
    n, d, qb = 20, 512, 128                                         # the smallest shape test_gpu_gemm_int8.py routes
    pool = synth.make_gallery(810, n + 100, d, L2)
    r = ref.RefGallery(pool[:n])
    q, _ = synth.make_queries(811, pool[:n + 70], qb, L2)
    with fir.Gallery(pool[:n], None, L2, 0) as g:
        g.set_large_batch_mfma(qb)
        g.set_int8_nomination(1)
        first = g.search_top1(q)
        assert "k_gemm_proxy_i8x<" in g.last_dispatch()["kernel"]
        g.append(pool[n:n + 70])
        r.append(pool[n:n + 70])
        sel = np.array([0, 19, 50], I32)
        g.set_rows(sel, q[:3])
        r.set_rows(sel, q[:3])
        gone = np.array([int(first[0][9])], I32)
        assert np.array_equal(g.remove_rows(gone), r.remove_rows(gone))
        got = g.search_top1(q)
        disp = g.last_dispatch()
        assert disp["path"] == "mfma" and "k_gemm_proxy_i8x<" in disp["kernel"], disp
        g.set_large_batch_mfma(0)
        scan = g.search_top1(q)
        with fir.Gallery(r.rows, None, L2, 0) as f:
            f.set_large_batch_mfma(qb)
            f.set_int8_nomination(1)
            fresh = f.search_top1(q)
            assert "k_gemm_proxy_i8x<" in f.last_dispatch()["kernel"]
            f.set_large_batch_mfma(0)
            want = f.search_top1(q)
        assert same(got, fresh) and same(got, want) and same(scan, want)
        assert np.all(got[1][:3] == 0)


# ---- 5. states the caller made go stale safely -----------------------------------------------------------------------------------
def test_caller_made_states_refuse_after_an_update(fir):
    n, d, qb = 4099, 64, 130
    pool = synth.make_gallery(820, n + 200, d, L2)
    lab = labels_for(pool.shape[0], 821, 37)
    q_host, _ = synth.make_queries(822, pool[:n], qb, L2)
    q = torch.from_numpy(q_host).to(DEV)
    radius = torch.full((qb,), 0.001, dtype=torch.float32, device=DEV)
    L = fir.lib()

    def stale(call):
        with pytest.raises(fir.FirError) as e:
            call()
        assert e.value.code == ERR_STATE and "gallery changed" in str(e.value), e.value

    for how in ("grow", "set"):
        with fir.Gallery(pool[:n], lab[:n], L2, 0) as g:
            m = fir.GemmSearch(g)
            dem = fir.Dem(g, 7, 5)
            keys = torch.full((qb * 9,), POISON64, dtype=torch.int64, device=DEV)
            cls = torch.full((qb * 9,), -1234, dtype=torch.int32, device=DEV)
            m.search_top1_keys_dev(q.data_ptr(), qb, keys.data_ptr())      # both work before the update
            g.sync()
            assert not torch.any(keys[:qb] == POISON64)
            dem.recognize(q_host[:4], 0.001, 5)
            keys.fill_(POISON64)
            torch.cuda.synchronize()
            if how == "grow":
                cap = g.capacity()
                g.append(pool[n:n + 200], lab[n:n + 200])           # beyond the capacity: the buffers the states point into are freed
                assert g.capacity() > cap
                now = ref.RefGallery(pool[:n + 200], lab[:n + 200])
            else:
                g.set_rows(np.array([5], I32), pool[n:n + 1])
                now = ref.RefGallery(pool[:n], lab[:n])
                now.set_rows([5], pool[n:n + 1])
            kp, qp = keys.data_ptr(), q.data_ptr()
            stale(lambda: m.search_top1_keys_dev(qp, qb, kp))
            stale(lambda: m.search_few_keys_dev(qp, 4, kp))
            stale(lambda: m.search_topk_keys_dev(qp, qb, 5, kp))
            stale(lambda: m.search_top_classes_keys_dev(qp, qb, 37, 3, kp, cls.data_ptr()))
            stale(lambda: m.search_knn_keys_dev(qp, qb, 9, kp))
            stale(lambda: m.search_knn_keys_dev(qp, qb, 1, kp))
            stale(lambda: m.search_radius_keys_dev(qp, qb, radius.data_ptr(), 4, cls.data_ptr(), kp))
            out = [np.full(qb, -1234, I32) for _ in range(5)]
            assert L.fir_dem_recognize(dem._h, q_host.ctypes.data, qb, 0.001, 5, *(o.ctypes.data for o in out)) == ERR_STATE
            assert b"gallery changed" in L.fir_last_error()
            assert all(np.all(o == -1234) for o in out)
            stale(lambda: dem.recognize_dev(qp, qb, 0.001, 5, cls.data_ptr(), None, None, None, None))
            lik = np.full((qb, dem.n), -5.0, F32)
            pd = np.full((qb, dem.n_used), -5.0, F32)
            assert L.fir_dem_likelihoods(dem._h, q_host.ctypes.data, qb, pd.ctypes.data, lik.ctypes.data) == ERR_STATE
            assert np.all(lik == -5.0) and np.all(pd == -5.0)
            torch.cuda.synchronize()
            assert torch.all(keys == POISON64) and torch.all(cls == -1234)
            assert m.stats()["passes"] >= 1                         # reads the state's own memory: still fine
            m.close()
            dem.close()
            with fir.Gallery(now.rows, now.labels, L2, 0) as f:      # the gallery itself answers, and new states work
                f.set_large_batch_mfma(0)
                want = f.search_top1(q_host)
                assert same(g.search_top1(q_host), want)
                m2 = fir.GemmSearch(g)
                m2.search_top1_keys_dev(qp, qb, kp)
                g.sync()
                assert same(fir.keys_unpack(keys[:qb].cpu().numpy().view(np.uint64)), want)
                m2.close()
                d2, d3 = fir.Dem(g, 7, 5), fir.Dem(f, 7, 5)
                assert same(d2.recognize(q_host[:8], 0.001, 5), d3.recognize(q_host[:8], 0.001, 5))
                d2.close()
                d3.close()


# ---- 6. capacity and failure -----------------------------------------------------------------------------------------------------
def tiled_bytes(rows, d, label_rows):
    return (rows + 63) // 64 * 64 * ((d + 3) // 4) * 16 + 4 * label_rows


def test_capacity_follows_the_rule(fir):
    n0, d = 100, 20
    pool = synth.make_gallery(900, 2000, d, L2)
    lab = labels_for(2000, 901)
    with fir.Gallery(pool[:n0], lab[:n0], L2, 0) as g:
        # a handle that was never updated reports what it always did
        assert g.memory_bytes() == {"tiled": tiled_bytes(n0, d, n0), "fp16_fragments": 0, "rowmajor_shadow": 0, "scratch": 0}
        g.reserve(50)                                               # below n: nothing happens
        assert g.memory_bytes()["tiled"] == tiled_bytes(n0, d, n0) and g.n == n0
        g.reserve(300)
        cap = g.capacity()
        assert cap == 320 and g.memory_bytes()["tiled"] == tiled_bytes(320, d, 320)
        g.reserve(200)                                              # never shrinks
        assert g.capacity() == cap
        at = n0
        for m in (1, 63, cap - n0 - 64):                            # appends up to the capacity allocate nothing
            g.append(pool[at:at + m], lab[at:at + m])
            at += m
            assert g.capacity() == cap and g.memory_bytes()["tiled"] == tiled_bytes(320, d, 320)
        assert g.n == cap
        g.append(pool[at:at + 1], lab[at:at + 1])                   # one more row: n + m plus a quarter, in whole tiles
        need = cap + 1
        want_cap = (need + need // 4 + 63) // 64 * 64
        assert g.capacity() == want_cap and g.memory_bytes()["tiled"] == tiled_bytes(want_cap, d, want_cap)
        assert same(g.read_rows(), pool[:cap + 1]) and np.array_equal(g.read_rows(0, None, True)[1], lab[:cap + 1])
    with fir.Gallery(pool[:n0], None, L2, 0) as g:
        assert g.memory_bytes()["tiled"] == tiled_bytes(n0, d, 0) and g.capacity() == 128
        g.append(pool[n0:128])                                      # an unlabelled handle has its last tile's rows to give
        assert g.memory_bytes()["tiled"] == tiled_bytes(n0, d, 0) and g.n == 128


def test_label_rules(fir):
    d = 12
    pool = synth.make_gallery(910, 300, d, L2)
    lab = labels_for(300, 911)
    for first_labelled in (True, False):                            # an empty handle takes its labelled-ness from its first append
        with fir.Gallery(pool[:0], lab[:0], L2, 0) as g:
            assert g.n == 0 and g.capacity() == 0
            g.append(pool[:70], lab[:70] if first_labelled else None)
            with pytest.raises(fir.FirError) as e:
                g.append(pool[70:80], None if first_labelled else lab[70:80])
            assert e.value.code == ERR_ARG and g.n == 70
            assert ("appended rows need class_no" if first_labelled else "class_no must be NULL") in str(e.value), e.value
            g.append(pool[70:80], lab[70:80] if first_labelled else None)
            assert same(g.read_rows(), pool[:80])
            if first_labelled:
                assert np.array_equal(g.read_rows(0, None, True)[1], lab[:80])
                assert np.array_equal(g.classes_of(np.array([0, 79, 80, -1], I32)), [lab[0], lab[79], -1, -1])
            else:
                with pytest.raises(fir.FirError) as e:
                    g.read_rows(0, 5, True)
                assert e.value.code == ERR_STATE and "without class labels" in str(e.value)
                with pytest.raises(fir.FirError) as e:
                    g.set_rows(np.array([1], I32), pool[:1], lab[:1])
                assert e.value.code == ERR_ARG and "class_no must be NULL" in str(e.value)
                with pytest.raises(fir.FirError) as e:                  # the label rule answers before the index checks
                    g.set_rows(np.array([3, 3], I32), pool[:2], lab[:2])
                assert e.value.code == ERR_ARG and "class_no must be NULL" in str(e.value)
            # every row removed: the handle is an empty one again, either kind of append is taken
            g.remove_rows(np.arange(80, dtype=I32))
            assert g.n == 0
            g.append(pool[100:105], None if first_labelled else lab[100:105])
            assert same(g.read_rows(), pool[100:105])
            if not first_labelled:
                assert np.array_equal(g.read_rows(0, None, True)[1], lab[100:105])
    any_label = np.array([-(2 ** 31), 2 ** 31 - 1, -1], I32)        # any int32 is a label
    with fir.Gallery(pool[:10], lab[:10], L2, 0) as g:
        g.append(pool[10:13], any_label)
        assert np.array_equal(g.read_rows(10, 3, True)[1], any_label)


def test_bad_arguments_change_nothing(fir):
    n, d = 130, 12
    pool = synth.make_gallery(920, 300, d, L2)
    lab = labels_for(300, 921)
    L = fir.lib()
    one = np.zeros(4, I32)
    with fir.Gallery(pool[:n], lab[:n], L2, 0) as g:
        g.reserve(200)
        g.read_rows(0, None, True)                                  # (its staging buffer exists from here on)
        cap, mem = g.capacity(), g.memory_bytes()
        h, pp, pl, po = g._h, pool.ctypes.data, lab.ctypes.data, one.ctypes.data
        dup = np.array([7, 7], I32)
        moved = np.full(2, -99, I32)
        # (call, the fragment of fir_last_error() that names the reason); where a call is wrong twice, the check that comes first in
        # the order of the header -- NULL, m < 0, labels, index range / duplicates, the 32-bit limit -- is the one that answers
        bad = [(lambda: g.append(pool[n:n + 3], None), "appended rows need class_no"),
               (lambda: g.set_rows(np.array([n], I32), pool[:1]), f"row index {n} outside [0,{n})"),
               (lambda: g.set_rows(np.array([-1], I32), pool[:1]), f"row index -1 outside [0,{n})"),
               (lambda: g.set_rows(np.array([4, 9, 4], I32), pool[:3]), "row index 4 is listed twice"),
               (lambda: g.remove_rows(np.array([n], I32)), f"row index {n} outside [0,{n})"),
               (lambda: g.remove_rows(np.array([-1], I32)), f"row index -1 outside [0,{n})"),
               (lambda: g.remove_rows(dup), "row index 7 is listed twice"),
               (lambda: fir_check(fir, L.fir_gallery_remove_rows(h, dup.ctypes.data, 2, moved.ctypes.data)), "listed twice"),
               (lambda: g.read_rows(n - 2, 3), f"rows [{n - 2},+3) outside [0,{n})"),
               (lambda: g.read_rows(-1, 2), f"rows [-1,+2) outside [0,{n})"),
               (lambda: fir_check(fir, L.fir_gallery_read_rows(h, 0, -1, pp, None)), "m < 0"),
               (lambda: fir_check(fir, L.fir_gallery_read_rows(h, 0, 2, None, None)), "NULL argument"),
               (lambda: fir_check(fir, L.fir_gallery_append(h, pp, -1, pl)), "m < 0"),
               (lambda: fir_check(fir, L.fir_gallery_append(h, pp, -1, None)), "m < 0"),                   # m < 0 before the label rule
               (lambda: fir_check(fir, L.fir_gallery_append(h, None, 2, pl)), "NULL argument"),
               (lambda: fir_check(fir, L.fir_gallery_append(h, None, 2, None)), "NULL argument"),          # NULL before the label rule
               (lambda: fir_check(fir, L.fir_gallery_append(h, pp, 1 << 31, None)), "appended rows need class_no"),   # labels before the limit
               (lambda: fir_check(fir, L.fir_gallery_append(h, pp, 1 << 31, pl)), "does not fit 32-bit"),
               (lambda: fir_check(fir, L.fir_gallery_append_dev(h, None, 2, None, None)), "NULL argument"),
               (lambda: fir_check(fir, L.fir_gallery_append_dev(h, pp, -3, pl, None)), "m < 0"),
               (lambda: fir_check(fir, L.fir_gallery_append_dev(h, pp, 2, None, None)), "appended rows need class_no"),
               (lambda: fir_check(fir, L.fir_gallery_set_rows(h, po, -1, pp, None)), "m < 0"),
               (lambda: fir_check(fir, L.fir_gallery_set_rows(h, None, 1, pp, None)), "NULL argument"),
               (lambda: fir_check(fir, L.fir_gallery_set_rows(h, po, 1, None, None)), "NULL argument"),
               (lambda: fir_check(fir, L.fir_gallery_set_rows(h, None, -1, None, None)), "m < 0"),
               (lambda: fir_check(fir, L.fir_gallery_remove_rows(h, po, -2, None)), "m < 0"),
               (lambda: fir_check(fir, L.fir_gallery_remove_rows(h, None, 2, None)), "NULL argument"),
               (lambda: fir_check(fir, L.fir_gallery_reserve(None, 5)), "gallery is NULL"),
               (lambda: fir_check(fir, L.fir_gallery_capacity(h, None)), "NULL argument")]
        for i, (call, text) in enumerate(bad):
            with pytest.raises(fir.FirError) as e:
                call()
            assert e.value.code == ERR_ARG and text in str(e.value), (i, text, str(e.value))
            assert g.n == n and g.capacity() == cap and g.memory_bytes() == mem, i
            rows, cls = g.read_rows(0, None, True)
            assert rows.tobytes() == pool[:n].tobytes() and cls.tobytes() == lab[:n].tobytes(), i
        assert np.all(moved == -99)                                 # a refused removal writes no plan
        # m == 0: nothing to do
        g.append(pool[:0], lab[:0])
        g.set_rows(np.empty(0, I32), pool[:0])
        assert g.remove_rows(np.empty(0, I32)).size == 0 and g.n == n
        # the 32-bit limit counts the row offset
        g.set_row_offset((1 << 31) - 64 - n - 5)
        with pytest.raises(fir.FirError) as e:
            g.append(pool[n:n + 10], lab[n:n + 10])
        assert e.value.code == ERR_ARG and "does not fit 32-bit" in str(e.value) and g.n == n
        with pytest.raises(fir.FirError) as e:
            g.append(pool[n:n + 10], None)                          # the label rule answers before the limit
        assert e.value.code == ERR_ARG and "appended rows need class_no" in str(e.value) and g.n == n
        with pytest.raises(fir.FirError) as e:
            g.reserve(n + 10)
        assert e.value.code == ERR_ARG and "does not fit 32-bit" in str(e.value)
        g.append(pool[n:n + 4], lab[n:n + 4])
        assert g.n == n + 4
        idx, _ = g.search_top1(pool[n + 3:n + 4])
        assert idx[0] == (1 << 31) - 64 - n - 5 + n + 3
        g.set_row_offset(0)                                         # row_idx are local whatever the offset was
        assert same(g.read_rows(n, 4), pool[n:n + 4])


def fir_check(fir, rc):
    if rc != 0:
        raise fir.FirError(rc, fir.lib().fir_last_error().decode())


def test_a_borrowed_shard_refuses_updates(fir):
    n, d = 300, 16
    rows = synth.make_gallery(930, n, d, L2)
    lab = labels_for(n, 931)
    with fir.ShardedGallery(rows, lab, fir.METRIC_L2, devices=[0], shards_per_device=2) as s:
        g, lo, cnt = s.shard(0)
        assert g is not None and cnt > 0
        for call in (lambda: g.append(rows[:2], lab[:2]), lambda: g.set_rows(np.array([0], I32), rows[:1]),
                     lambda: g.remove_rows(np.array([0], I32)), lambda: g.reserve(1000), lambda: g.append(rows[:0], lab[:0])):
            with pytest.raises(fir.FirError) as e:
                call()
            assert e.value.code == ERR_STATE
        assert same(g.read_rows(0, cnt), rows[lo:lo + cnt])          # reading is no mutation
        idx, dist = s.search_top1(rows[:9])
        assert np.array_equal(idx, np.arange(9)) and np.all(dist == 0)


# ---- 7. call order ---------------------------------------------------------------------------------------------------------------
def test_an_append_takes_effect_in_call_order_across_streams(fir):
    n, d, qb = 20000, 64, 64
    pool = synth.make_gallery(940, n + 1, d, L2)
    q_host, _ = synth.make_queries(941, pool[:n], qb, L2)
    q_host[7] = pool[n]                                             # the row that is appended between the two searches
    q = torch.from_numpy(q_host).to(DEV)
    new_row = torch.from_numpy(pool[n:n + 1].copy()).to(DEV)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    k1 = torch.full((qb,), POISON64, dtype=torch.int64, device=DEV)
    k2 = torch.full((qb,), POISON64, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    with fir.Gallery(pool[:n], None, L2, 0) as g:
        g.set_large_batch_mfma(0)                                   # (the routed forms synchronise: the scan never does)
        g.reserve(n + 64)
        g.search_top1_keys_dev(q.data_ptr(), qb, k1.data_ptr(), stream=a.cuda_stream)
        g.append_dev(new_row.data_ptr(), 1, None, stream=b.cuda_stream)
        g.search_top1_keys_dev(q.data_ptr(), qb, k2.data_ptr(), stream=a.cuda_stream)
        assert g.n == n + 1
        a.synchronize()
        b.synchronize()
        with fir.Gallery(pool[:n], None, L2, 0) as f:
            old = f.search_top1(q_host)
        with fir.Gallery(pool[:n + 1], None, L2, 0) as f:
            new = f.search_top1(q_host)
        assert same(fir.keys_unpack(k1.cpu().numpy().view(np.uint64)), old)
        assert same(fir.keys_unpack(k2.cpu().numpy().view(np.uint64)), new)
        assert old[0][7] != n and new[0][7] == n and new[1][7] == 0
