"""DirectedEnumeration::recognize (qt_cpp/ann.cpp:416-507, PIVOT build) restated twice in numpy, for the tests of
fir_dem_recognize:

- formulation(): the order-free form the device computes (include/fir_amd.h, fir_dem_recognize): one selection threshold,
  two minima, a count, and the tie flag;
- sequential_walk(): the literal walk over a sorted candidate list, equal likelihoods in ascending (the oracle's rule) or
  descending position order.

Both take the per-query inputs as arrays: pd[used] pivot distances, piv[used] pivot rows, order[n] (likelihood_indices after
the pivot loop), lik[n] likelihoods by row, dist_of_row[n] the distance of the query to every row."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def orderable(x):
    """float32 -> uint32 whose unsigned order is the float order (fir_common.h: f32_orderable)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)


def order_after_pivots(n, piv):
    """likelihood_indices after the two plain writes per pivot (ann.cpp:431-432)."""
    li = np.arange(n, dtype=np.int32)
    for s, p in enumerate(piv):
        li[p] = li[s]
        li[s] = p
    return li


def likelihoods(n, piv, table, pd):
    """`likelihoods` after all pivots (ann.cpp:437-446): float32 adds in the reference's order, rows visited by position."""
    li = np.arange(n, dtype=np.int32)
    lik = np.zeros(n, np.float32)
    for i, p in enumerate(piv):
        li[p] = li[i]
        li[i] = p
        for nu in li[i + 1:]:
            m = table[i, nu]
            if m >= 0:
                t = np.float32(pd[i] - m)
                lik[nu] = np.float32(lik[nu] + np.float32(t * t))
    return lik


def _pivot_loop(pd, piv, thr):
    best, row = FLT_MAX, -1
    for k in range(len(piv)):
        if pd[k] < best:
            best, row = np.float32(pd[k]), int(piv[k])
            if best < thr:
                return best, row, k
    return best, row, -1


def count_to_check(image_count, n):
    return image_count if 0 < image_count < n else n


def formulation(pd, piv, order, lik, dist_of_row, image_count, thr):
    """-> (row, dist, found, calc, tie)"""
    n, used = len(order), len(piv)
    thr = np.float32(thr)
    best, row, k = _pivot_loop(pd, piv, thr)
    if k >= 0:
        return row, best, 1, k + 1, 0
    mc = count_to_check(image_count, n) - used
    if mc <= 0:
        return row, best, 0, used, 0
    p = np.arange(used, n, dtype=np.uint64)
    lb = orderable(lik[order[used:]])
    key = (lb << np.uint64(32)) | p
    T = np.sort(key)[mc - 1]
    sel = key <= T
    assert sel.sum() == mc
    tie = int(np.isin(lb[~sel], lb[sel]).any()) | int(np.isnan(np.asarray(pd, np.float32)).any())
    skey, slb = key[sel], lb[sel]
    sdist = np.asarray(dist_of_row, np.float32)[order[used:][sel]] + np.float32(0)
    below = sdist < thr
    if below.any():
        j = np.flatnonzero(below)[np.argmin(skey[below])]
        tie |= int((slb == slb[j]).sum() > 1)
        return int(order[int(skey[j] & np.uint64(0xFFFFFFFF))]), sdist[j], 1, used + int((skey <= skey[j]).sum()), tie
    ok = ~np.isnan(sdist)
    if ok.any():
        cand = np.flatnonzero(ok)
        j = cand[np.lexsort((skey[cand], orderable(sdist[cand])))[0]]
        if sdist[j] < best:
            tie |= int(((slb == slb[j]) & (sdist.view(np.uint32) == sdist[j].view(np.uint32))).sum() > 1)
            return int(order[int(skey[j] & np.uint64(0xFFFFFFFF))]), sdist[j], 0, used + mc, tie
    return row, best, 0, used + mc, tie


def sequential_walk(pd, piv, order, lik, dist_of_row, image_count, thr, descending=False):
    """The walk itself -> (row, dist, found, calc); equal likelihoods by ascending or descending position."""
    n, used = len(order), len(piv)
    thr = np.float32(thr)
    best, row, k = _pivot_loop(pd, piv, thr)
    if k >= 0:
        return row, best, 1, k + 1
    M = count_to_check(image_count, n)
    calc = used
    if M > used:
        p = np.arange(used, n)
        cl = lik[order[used:]]
        walk = p[np.lexsort((-p if descending else p, cl))][: M - used]
        for pp in walk:
            d = np.float32(dist_of_row[order[pp]])
            calc += 1
            if d < best:
                best, row = d, int(order[pp])
                if best < thr:
                    return row, best, 1, calc
    return row, best, 0, calc
