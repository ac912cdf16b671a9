"""What a sequence of in-place gallery updates describes, in numpy: the array (and labels) a fresh fir_gallery_create handle is
made over to judge a handle that went through fir_gallery_append / _set_rows / _remove_rows. Nothing here calls the library.

The removal rule (include/fir_amd.h): n' = n - m; the holes are the removed rows below n', ascending; the survivors are the rows of
[n', n) that are not removed, ascending; the j-th hole receives the j-th survivor; every other row keeps its index."""
import numpy as np


def remove_plan(n, row_idx):
    """moved_from[m]: the former row now sitting at row_idx[i], -1 where row_idx[i] >= n - m. Raises ValueError on an index outside
    [0, n) or a duplicate."""
    row_idx = [int(r) for r in row_idx]
    m = len(row_idx)
    if any(r < 0 or r >= n for r in row_idx) or len(set(row_idx)) != m:
        raise ValueError("row indices must be distinct and inside [0, n)")
    n_new = n - m
    removed = set(row_idx)
    holes = sorted(r for r in removed if r < n_new)
    survivors = [r for r in range(n_new, n) if r not in removed]
    assert len(holes) == len(survivors)
    source = dict(zip(holes, survivors))
    return np.array([source.get(r, -1) for r in row_idx], np.int32)


def remove_order(n, row_idx):
    """old_row[n - m]: the former index of the row that sits at each index after the removal."""
    row_idx = [int(r) for r in row_idx]
    moved = remove_plan(n, row_idx)
    order = np.arange(n - len(row_idx), dtype=np.int64)
    for r, src in zip(row_idx, moved.tolist()):
        if src >= 0:
            order[r] = src
    return order


class RefGallery:
    """rows[n, d] float32 and labels[n] int32 (None: no labels) under the three operations."""

    def __init__(self, rows, labels=None):
        self.rows = np.array(rows, dtype=np.float32, copy=True)
        self.labels = None if labels is None else np.array(labels, dtype=np.int32, copy=True)

    @property
    def n(self):
        return self.rows.shape[0]

    def append(self, rows, labels=None):
        rows = np.asarray(rows, np.float32).reshape(-1, self.rows.shape[1])
        if self.n == 0:                       # an empty gallery takes its labelled-ness from its first append
            self.labels = None if labels is None else np.empty(0, np.int32)
        assert (labels is None) == (self.labels is None)
        self.rows = np.concatenate([self.rows, rows])
        if labels is not None:
            self.labels = np.concatenate([self.labels, np.asarray(labels, np.int32).reshape(-1)])

    def set_rows(self, row_idx, rows, labels=None):
        row_idx = np.asarray(row_idx, np.int64)
        self.rows[row_idx] = np.asarray(rows, np.float32).reshape(-1, self.rows.shape[1])
        if labels is not None:
            self.labels[row_idx] = np.asarray(labels, np.int32).reshape(-1)

    def remove_rows(self, row_idx):
        order = remove_order(self.n, row_idx)
        moved = remove_plan(self.n, row_idx)
        self.rows = self.rows[order].copy()
        if self.labels is not None:
            self.labels = self.labels[order].copy()
            if self.n == 0:
                self.labels = None            # as a gallery created with no rows: it keeps no labels
        return moved
