"""numpy restatement of the masked searches (include/fir_amd.h, "searches over a subset of the rows"), on knn_select_ref's keys,
radius_ref's rule and the class ranking of other_class_ref: no tolerance anywhere. Everything works from a distance matrix over
ALL rows and a bool mask over them.

A row qualifies iff its mask entry is set and it qualifies in the unmasked call: the masked-out rows simply leave the key list, so
every answer is the unmasked restatement over the rows that remain, with the keys still carrying the rows' own indices."""
import numpy as np

import knn_select_ref as ks
import radius_ref

KEY_NONE = ks.KEY_NONE
F32 = np.float32


def mask_words(n):
    return (int(n) + 63) // 64


def pack_bits(take):
    """bool[n] -> uint64[FIR_MASK_WORDS(n)] by an explicit loop over the bits: row r is bit r & 63 of word r >> 6."""
    take = np.asarray(take, bool).reshape(-1)
    words = [0] * mask_words(take.shape[0])
    for r in range(take.shape[0]):
        if take[r]:
            words[r >> 6] |= 1 << (r & 63)
    return np.array(words, np.uint64)


def unpack_bits(words, n):
    """The bool[n] a packed mask stands for; whatever lies past n is ignored."""
    words = np.asarray(words, np.uint64)
    return np.array([bool((int(words[r >> 6]) >> (r & 63)) & 1) for r in range(n)], bool)


def masked_keys(dist_row, take, row_offset=0):
    """One query's keys as a masked call sees them: FIR_KEY_NONE where the row is masked out or does not qualify by distance."""
    keys = ks.all_keys(dist_row, row_offset)
    return np.where(np.asarray(take, bool), keys, KEY_NONE)


def top1_keys(dist, take, row_offset=0):
    """[qb] uint64: the smallest key among the masked-in qualifying rows (the first minimum in row order), FIR_KEY_NONE without one."""
    dist = np.atleast_2d(np.asarray(dist, F32))
    out = np.full(dist.shape[0], KEY_NONE, np.uint64)
    for q in range(dist.shape[0]):
        keys = masked_keys(dist[q], take, row_offset)
        if keys.shape[0]:
            out[q] = keys.min()
    return out


def knn_keys(dist, take, k, row_offset=0):
    """[qb, k] uint64: the k smallest masked-in keys ascending, FIR_KEY_NONE behind them."""
    dist = np.atleast_2d(np.asarray(dist, F32))
    out = np.full((dist.shape[0], k), KEY_NONE, np.uint64)
    for q in range(dist.shape[0]):
        keys = np.sort(masked_keys(dist[q], take, row_offset))[:k]
        out[q, :keys.shape[0]] = keys
    return out


def radius_keys(dist, take, radius, max_results, row_offset=0):
    """(count[qb] int32, keys[qb, max_results]): radius_ref's rule over the masked-in rows; counts are never capped."""
    dist = np.atleast_2d(np.asarray(dist, F32))
    take = np.asarray(take, bool)
    radius = np.broadcast_to(np.asarray(radius, F32).reshape(-1), (dist.shape[0],))
    count = np.zeros(dist.shape[0], np.int32)
    out = np.full((dist.shape[0], max_results), KEY_NONE, np.uint64)
    for q in range(dist.shape[0]):
        keys = ks.all_keys(dist[q], row_offset)[radius_ref.inside(dist[q], radius[q]) & take]
        count[q] = keys.shape[0]
        keys = np.sort(keys)[:max_results]
        out[q, :keys.shape[0]] = keys
    return count, out


def class_keys(dist, take, labels, num_classes, k, row_offset=0):
    """(keys[qb, k], classes[qb, k]): per class in [0, num_classes) the smallest masked-in key, then the k smallest of those;
    FIR_KEY_NONE / -1 behind. A class with no masked-in qualifying row does not appear."""
    dist = np.atleast_2d(np.asarray(dist, F32))
    labels = np.asarray(labels, np.int32)
    ko = np.full((dist.shape[0], k), KEY_NONE, np.uint64)
    co = np.full((dist.shape[0], k), -1, np.int32)
    counted = (labels >= 0) & (labels < num_classes)
    for q in range(dist.shape[0]):
        keys = masked_keys(dist[q], take, row_offset)
        best = np.full(num_classes, KEY_NONE, np.uint64)
        np.minimum.at(best, labels[counted], keys[counted])
        order = np.argsort(best, kind="stable")[:k]              # keys are unique: only FIR_KEY_NONE entries tie, and they are dropped
        order = order[best[order] != KEY_NONE]
        ko[q, :order.shape[0]] = best[order]
        co[q, :order.shape[0]] = order
    return ko, co


def map_back(keys, sel, row_offset=0):
    """Keys of a search over the compacted rows (no row offset) -> keys over the full gallery: row i of the compacted gallery is row
    sel[i] (sel = np.flatnonzero(mask), ascending: ties keep their order); the distance bits stay."""
    keys = np.asarray(keys, np.uint64)
    sel = np.asarray(sel, np.int64)
    none = keys == KEY_NONE
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    idx = np.where(none, 0, idx)
    rows = (sel[idx] + row_offset).astype(np.uint64) & np.uint64(0xFFFFFFFF) if sel.shape[0] else np.zeros(keys.shape, np.uint64)
    return np.where(none, KEY_NONE, (keys & np.uint64(0xFFFFFFFF00000000)) | rows)
