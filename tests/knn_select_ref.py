"""numpy restatement of fir_search_knn's contract and of the select that computes it (csrc/fir_knn_select.h).

Contract (include/fir_amd.h): per query the k smallest packed keys (orderable(distance bits) << 32) | uint32(row + row offset),
ascending; a row qualifies only if `dist < 100000.0f` is true; unused slots hold FIR_KEY_NONE.

Select as the kernels do it: rows that do not qualify count as FIR_KEY_NONE, so n keys enter; eight passes of 8-bit digits from the
most significant, each a 256-bin histogram of the keys that match the prefix found so far; the rank min(k, n) walks into the bin
it falls in; when the rank is the bin's whole count the remaining digits are all ones and the passes stop. Keys <= T that are
not FIR_KEY_NONE are compacted (in any order) and sorted by a bitonic network over the next power of two >= max(k, 2)."""
import numpy as np

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
NOT_FOUND = np.float32(100000.0)
KNN_MAX = 1024
DIGIT_BITS = 8
PASSES = 8


def orderable(dist):
    """float32 -> uint32 whose unsigned order is the float order (fir_common.h: f32_orderable), after -0 -> +0 (key_pack)."""
    d = np.asarray(dist, np.float32) + np.float32(0.0)
    b = d.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def qualifies(dist):
    with np.errstate(invalid="ignore"):
        return np.asarray(dist, np.float32) < NOT_FOUND          # False for NaN


def all_keys(dist, row_offset=0):
    """The n keys of one query's distance row as the select sees them: FIR_KEY_NONE where the row does not qualify."""
    dist = np.asarray(dist, np.float32)
    rows = (np.arange(dist.shape[0], dtype=np.int64) + row_offset).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    keys = (orderable(dist).astype(np.uint64) << np.uint64(32)) | rows
    return np.where(qualifies(dist), keys, KEY_NONE)


def expected_keys(dist, k, row_offset=0):
    """The contract, by sorting: lexsort on (distance bits, row) of the qualifying rows, padded."""
    dist = np.asarray(dist, np.float32)
    ok = np.flatnonzero(qualifies(dist))
    order = ok[np.lexsort((ok, orderable(dist[ok])))]
    keys = all_keys(dist, row_offset)[order][:k]
    return np.concatenate([keys, np.full(k - keys.shape[0], KEY_NONE, np.uint64)])


def radix_threshold(keys, k):
    """T of the kernels for the n >= 1 keys of one query (FIR_KEY_NONE entries included) and the number of passes that ran."""
    keys = np.asarray(keys, np.uint64)
    rank = min(k, keys.shape[0])
    prefix = np.uint64(0)
    for p in range(PASSES):
        shift = np.uint64(64 - DIGIT_BITS * (p + 1))
        match = np.ones(keys.shape, bool) if p == 0 else ((keys ^ prefix) >> np.uint64(64 - DIGIT_BITS * p)) == 0
        hist = np.bincount(((keys[match] >> shift) & np.uint64(255)).astype(np.int64), minlength=256)
        incl = np.cumsum(hist)
        b = int(np.searchsorted(incl, rank))                     # first bin with incl >= rank
        excl = int(incl[b] - hist[b])
        assert hist[b] > 0 and excl < rank <= incl[b]
        prefix = prefix | (np.uint64(b) << shift)
        if rank - excl == hist[b]:                               # the whole bin: the rest of T is all ones
            return prefix | ((np.uint64(1) << shift) - np.uint64(1)), p + 1
        rank -= excl
    return prefix, PASSES


def bitonic_sort(vals):
    """The network k_knn_sort runs, on a power-of-two array."""
    s = np.array(vals, np.uint64)
    n = s.shape[0]
    assert n >= 2 and n & (n - 1) == 0
    i = np.arange(n)
    k2 = 2
    while k2 <= n:
        j = k2 >> 1
        while j > 0:
            o = i ^ j
            lo = o > i
            up = (i & k2) == 0
            a, b = s[i[lo]], s[o[lo]]
            swap = (a > b) == up[lo]
            s[i[lo]] = np.where(swap, b, a)
            s[o[lo]] = np.where(swap, a, b)
            j >>= 1
        k2 <<= 1
    return s


def emulate(dist, k, row_offset=0, shuffle_seed=None):
    """k keys as the kernels produce them. shuffle_seed: the order the compaction's atomics happened to give."""
    assert 1 <= k <= KNN_MAX
    keys = all_keys(dist, row_offset)
    if keys.shape[0] == 0:
        return np.full(k, KEY_NONE, np.uint64)
    T, _ = radix_threshold(keys, k)
    taken = keys[(keys <= T) & (keys != KEY_NONE)]
    assert taken.shape[0] <= k
    if shuffle_seed is not None:
        taken = np.random.default_rng(shuffle_seed).permutation(taken)
    p = 2
    while p < k:
        p *= 2
    s = np.full(p, KEY_NONE, np.uint64)
    s[: taken.shape[0]] = taken
    return bitonic_sort(s)[:k]


def unpack(keys):
    """(idx, dist) as fir_keys_unpack gives them."""
    keys = np.asarray(keys, np.uint64)
    o = (keys >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    none = keys == KEY_NONE
    idx = np.where(none, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    dist = np.where(none, NOT_FOUND, bits.view(np.float32)).astype(np.float32)
    return idx, dist
