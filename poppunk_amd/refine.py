"""Network scores of `--fit-model refine`'s global search on the MI355X.

    growNetwork(sample_names, i_vec, j_vec, idx_vec, s_range, score_idx=0, thread_idx=0,
                betweenness_sample=100, write_clusters=None, sample_size=None, use_gpu=False) -> list

mirrors PopPUNK/refine.py:375-474: the graph over `sample_names` grows batch by batch (offset index by offset index)
and every step is scored with `networkSummary` (PopPUNK/network.py:1204-1307) without betweenness.  The counts of
every step come from one device call (ppk_network_sweep); `summary_from_stats` and `grow_scores` turn them into
networkSummary's metrics and growNetwork's list on the host.

The score follows networkSummary's graph-tool branch (network.py:1256-1264), not its cugraph branch (:1236-1249):
density = E / (0.5 n (n - 1)) (cugraph: E / (0.5 n^2 - 1)), and transitivity = 3T / W, NaN when W = 0 (cugraph: 0).
graph-tool's `global_clustering` itself cannot be run here: that it returns NaN for a graph without connected
triples is UNVERIFIED.

Not mirrored (NotImplementedError, raised before the device is touched): betweenness scores (score_idx > 0),
random vertex subsampling (sample_size), and writing each step's clusters (write_clusters: printClusters).
`use_gpu` selects cugraph upstream; it is accepted and ignored (this is the device path either way).
"""
import ctypes as C

import numpy as np

from . import _lib

betweenness_sample_default = 100       # PopPUNK/__init__.py


def summary_from_stats(stats, n):
    """networkSummary(G, calc_betweenness=False) from one row {edges, components, triangles, triples} of a graph of
    n vertices -> (metrics [components, density, transitivity, 0, 0], scores [base, base, base])."""
    edges, components, triangles, triples = (int(x) for x in stats)
    density = edges / (0.5 * n * (n - 1))
    transitivity = 3 * triangles / triples if triples > 0 else float("nan")
    metrics = [components, density, transitivity, 0, 0]
    base_score = transitivity * (1 - density)
    return metrics, [base_score, base_score * (1 - metrics[3]), base_score * (1 - metrics[4])]


def grow_scores(stats, n, score_idx=0):
    """growNetwork's list from the per-offset counts (int [n_off, 4]): for each offset index that adds edges, in
    increasing order, -score of the graph after it, repeated (idx - previous idx) times (refine.py:455-468; the
    previous idx starts at -1).  Offsets without new edges therefore take the score of the next one that has them,
    and the list ends at the last offset with edges.  No edges at all: ValueError, as max() of the reference's
    empty idx_values."""
    stats = np.asarray(stats, dtype=np.int64).reshape(-1, 4)
    grown = np.flatnonzero(np.diff(np.concatenate(([0], stats[:, 0]))) > 0)
    if grown.size == 0:
        raise ValueError("max() arg is an empty sequence")
    scores = []
    prev_idx = -1
    for idx in grown:
        latest_score = -summary_from_stats(stats[idx], n)[1][score_idx]
        scores.extend([latest_score] * int(idx - prev_idx))
        prev_idx = idx
    return scores


def network_sweep(i_vec, j_vec, idx_vec, n, n_off=None, labels_at=None, device=0):
    """ppk_network_sweep on host arrays -> (stats int64 [n_off, 4], labels int32 [n] or None)."""
    i = np.ascontiguousarray(i_vec, dtype=np.int64).ravel()
    j = np.ascontiguousarray(j_vec, dtype=np.int64).ravel()
    o = np.ascontiguousarray(idx_vec, dtype=np.int64).ravel()
    if not (i.size == j.size == o.size):
        raise ValueError("i_vec, j_vec and idx_vec differ in length")
    if n_off is None:
        n_off = int(o.max()) + 1 if o.size else 1
    la = -1 if labels_at is None else int(labels_at)
    stats = np.zeros((max(int(n_off), 1), 4), dtype=np.int64)
    labels = np.zeros(max(int(n), 1), dtype=np.int32) if la >= 0 else None
    llp = C.POINTER(C.c_longlong)
    rc = _lib.lib().ppk_network_sweep(i.ctypes.data_as(llp), j.ctypes.data_as(llp), o.ctypes.data_as(llp), i.size,
                                      int(n), int(n_off), int(device), la, stats.ctypes.data_as(llp),
                                      labels.ctypes.data_as(C.POINTER(C.c_int32)) if labels is not None else None)
    _lib.check(rc, "ppk_network_sweep")
    return stats, (labels[:int(n)] if labels is not None else None)


def growNetwork(sample_names, i_vec, j_vec, idx_vec, s_range, score_idx=0, thread_idx=0,
                betweenness_sample=betweenness_sample_default, write_clusters=None, sample_size=None,
                use_gpu=False):
    """PopPUNK/refine.py:375-474 (see the module docstring for what is not mirrored).  idx_vec: each edge's offset
    index, as thresholdIterate1D/2D return it; the graph of step idx holds every edge of index <= idx."""
    if score_idx > 0:
        raise NotImplementedError("growNetwork: betweenness scores (score_idx > 0) are not computed on the device")
    if sample_size is not None:
        raise NotImplementedError("growNetwork: random vertex subsampling (sample_size) is not mirrored")
    if write_clusters:
        raise NotImplementedError("growNetwork: writing clusters per step (write_clusters) is not mirrored")
    idx = np.asarray(idx_vec, dtype=np.int64).ravel()
    if idx.size == 0:
        raise ValueError("max() arg is an empty sequence")
    n = len(sample_names)
    stats, _ = network_sweep(i_vec, j_vec, idx, n, int(idx.max()) + 1)
    return grow_scores(stats, n, score_idx)
