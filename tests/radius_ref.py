"""numpy restatement of fir_search_radius's contract (include/fir_amd.h), on knn_select_ref's keys: no tolerance anywhere.

A row qualifies iff `dist < radius` and `dist < 100000.0f` are both true as float32 compares: NaN distances never do, a NaN, zero
or negative radius qualifies nothing, a radius >= 100000 qualifies what fir_search_knn considers. count is the number of
qualifying rows; keys are the min(count, max_results) smallest packed keys of them, ascending, FIR_KEY_NONE behind."""
import numpy as np

import knn_select_ref as ref

KEY_NONE = ref.KEY_NONE


def inside(dist_row, radius):
    """The qualification rule, element by element (False wherever a compare involves a NaN)."""
    dist_row = np.asarray(dist_row, np.float32)
    with np.errstate(invalid="ignore"):
        return (dist_row < np.float32(radius)) & ref.qualifies(dist_row)


def expected(dist_row, radius, max_results, row_offset=0):
    """(count, keys[max_results]) for one query's distance row."""
    dist_row = np.asarray(dist_row, np.float32)
    keys = ref.all_keys(dist_row, row_offset)[inside(dist_row, radius)]
    count = int(keys.shape[0])
    keys = np.sort(keys)[:max_results]              # unique keys: (orderable distance, row) ascending
    return count, np.concatenate([keys, np.full(max_results - keys.shape[0], KEY_NONE, np.uint64)])


def expected_batch(dist, radius, max_results, row_offset=0):
    """(count[qb], keys[qb, max_results]); radius a scalar or one per query."""
    dist = np.atleast_2d(np.asarray(dist, np.float32))
    radius = np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (dist.shape[0],))
    both = [expected(dist[i], radius[i], max_results, row_offset) for i in range(dist.shape[0])]
    return (np.array([c for c, _ in both], np.int32),
            np.stack([k for _, k in both]) if both else np.zeros((0, max_results), np.uint64))
