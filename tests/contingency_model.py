"""The six outputs of ppk_contingency_sums_dev (include/ppk.h "Contingency sums") restated in numpy:
per level the squared class sizes and the number of labels, per pair of levels np.unique over the int64 keys
(x, y) -> x * (n + 1) + y, whose counts are the non-empty cells of the contingency table.  Everything is an integer, so
the device results are compared with this by array_equal."""
import numpy as np


def level_sums(levels):
    """(sq int64 [n_levels], labels int32 [n_levels]) of int [n_levels, n] cluster numbers."""
    levels = np.atleast_2d(np.asarray(levels, dtype=np.int64))
    sq = np.empty(len(levels), dtype=np.int64)
    labels = np.empty(len(levels), dtype=np.int32)
    for t, row in enumerate(levels):
        _, counts = np.unique(row, return_counts=True)
        sq[t] = np.sum(counts.astype(np.int64) ** 2)
        labels[t] = len(counts)
    return sq, labels


def contingency_sums(levels_a, levels_b=None):
    """(sq_a, sq_b, labels_a, labels_b, sq_cells, n_cells), the order of the C call's outputs; levels_b None: B = A."""
    a = np.atleast_2d(np.asarray(levels_a, dtype=np.int64))
    b = a if levels_b is None else np.atleast_2d(np.asarray(levels_b, dtype=np.int64))
    assert a.shape[1] == b.shape[1]
    n = a.shape[1]
    sq_a, labels_a = level_sums(a)
    sq_b, labels_b = level_sums(b)
    sq_cells = np.empty((len(a), len(b)), dtype=np.int64)
    n_cells = np.empty((len(a), len(b)), dtype=np.int64)
    for x, row_a in enumerate(a):
        for y, row_b in enumerate(b):
            _, counts = np.unique(row_a * np.int64(n + 1) + row_b, return_counts=True)
            sq_cells[x, y] = np.sum(counts.astype(np.int64) ** 2)
            n_cells[x, y] = len(counts)
    return sq_a, sq_b, labels_a, labels_b, sq_cells, n_cells


def device_call(levels_a, levels_b=None, device_id=0):
    """What poppunk_amd.scores._device_sums returns, from the restatement: for tests without a device."""
    return contingency_sums(levels_a, levels_b)
