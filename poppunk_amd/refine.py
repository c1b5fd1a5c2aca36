"""Network scores of `--fit-model refine`'s global search on the MI355X.

    growNetwork(sample_names, i_vec, j_vec, idx_vec, s_range, score_idx=0, thread_idx=0,
                betweenness_sample=100, write_clusters=None, sample_size=None, use_gpu=False) -> list

mirrors PopPUNK/refine.py:375-474: the graph over `sample_names` grows batch by batch (offset index by offset index)
and every step is scored with `networkSummary` (PopPUNK/network.py:1204-1307) without betweenness.  The counts of
every step come from one device call (ppk_network_sweep); `summary_from_stats` and `grow_scores` turn them into
networkSummary's metrics and growNetwork's list on the host.  Given the per-step betweenness means of
ppk_network_summary as `bt`, they also fill metrics 3 and 4 and the scores of score_idx 1 and 2.

The score follows networkSummary's graph-tool branch (network.py:1256-1264), not its cugraph branch (:1236-1249):
density = E / (0.5 n (n - 1)) (cugraph: E / (0.5 n^2 - 1)), and transitivity = 3T / W, NaN when W = 0 (cugraph: 0).
graph-tool's `global_clustering` itself cannot be run here: that it returns NaN for a graph without connected
triples is UNVERIFIED.

Not mirrored by growNetwork (NotImplementedError, raised before the device is touched): betweenness scores
(score_idx > 0; the device path for those is engine.refine_sweep_scores_dev(..., score_idx=...)),
random vertex subsampling (sample_size), and writing each step's clusters (write_clusters: printClusters).
`use_gpu` selects cugraph upstream; it is accepted and ignored (this is the device path either way).
"""
import ctypes as C

import numpy as np

from . import _lib

betweenness_sample_default = 100       # PopPUNK/__init__.py


def summary_from_stats(stats, n, bt=None):
    """networkSummary(G, calc_betweenness=False) from one row {edges, components, triangles, triples} of a graph of
    n vertices -> (metrics [components, density, transitivity, 0, 0], scores [base, base, base]).  With bt = the
    row's {mean, size-weighted mean} betweenness (ppk_network_summary): networkSummary(G, calc_betweenness=True),
    metrics 3 and 4 = bt and scores [base, base (1 - bt[0]), base (1 - bt[1])]."""
    edges, components, triangles, triples = (int(x) for x in stats)
    density = edges / (0.5 * n * (n - 1))
    transitivity = 3 * triangles / triples if triples > 0 else float("nan")
    mean_bt, weighted_mean_bt = (0, 0) if bt is None else (float(bt[0]), float(bt[1]))
    metrics = [components, density, transitivity, mean_bt, weighted_mean_bt]
    base_score = transitivity * (1 - density)
    return metrics, [base_score, base_score * (1 - metrics[3]), base_score * (1 - metrics[4])]


def grow_scores(stats, n, score_idx=0, bt=None):
    """growNetwork's list from the per-offset counts (int [n_off, 4]): for each offset index that adds edges, in
    increasing order, -score of the graph after it, repeated (idx - previous idx) times (refine.py:455-468; the
    previous idx starts at -1).  Offsets without new edges therefore take the score of the next one that has them,
    and the list ends at the last offset with edges.  No edges at all: ValueError, as max() of the reference's
    empty idx_values.  score_idx 1 and 2 need bt (float [n_off, 2], ppk_network_summary's betweenness means);
    score_idx 0 ignores it, as growNetwork computes no betweenness then (refine.py:452-457)."""
    if score_idx not in (0, 1, 2):
        raise ValueError("score_idx must be 0, 1 or 2")
    if score_idx > 0 and bt is None:
        raise ValueError("score_idx %d needs the betweenness means (bt)" % score_idx)
    stats = np.asarray(stats, dtype=np.int64).reshape(-1, 4)
    if score_idx > 0:
        bt = np.asarray(bt, dtype=np.float64).reshape(-1, 2)
        if bt.shape[0] != stats.shape[0]:
            raise ValueError("bt and stats differ in their number of offsets")
    grown = np.flatnonzero(np.diff(np.concatenate(([0], stats[:, 0]))) > 0)
    if grown.size == 0:
        raise ValueError("max() arg is an empty sequence")
    scores = []
    prev_idx = -1
    for idx in grown:
        latest_score = -summary_from_stats(stats[idx], n, bt[idx] if score_idx > 0 else None)[1][score_idx]
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


def network_summary(i_vec, j_vec, idx_vec, n, n_off=None, values_at=None, device=0):
    """ppk_network_summary on host arrays -> (stats int64 [n_off, 4], bt float64 [n_off, 2], scored int64 [n_off],
    values float64 [n] or None); idx_vec None puts every edge at offset 0."""
    i = np.ascontiguousarray(i_vec, dtype=np.int64).ravel()
    j = np.ascontiguousarray(j_vec, dtype=np.int64).ravel()
    o = None if idx_vec is None else np.ascontiguousarray(idx_vec, dtype=np.int64).ravel()
    if i.size != j.size or (o is not None and o.size != i.size):
        raise ValueError("i_vec, j_vec and idx_vec differ in length")
    if n_off is None:
        n_off = int(o.max()) + 1 if o is not None and o.size else 1
    va = -1 if values_at is None else int(values_at)
    no = max(int(n_off), 1)
    stats = np.zeros((no, 4), dtype=np.int64)
    bt = np.zeros((no, 2), dtype=np.float64)
    scored = np.zeros(no, dtype=np.int64)
    values = np.zeros(max(int(n), 1), dtype=np.float64) if va >= 0 else None
    llp, dp = C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    rc = _lib.lib().ppk_network_summary(i.ctypes.data_as(llp), j.ctypes.data_as(llp),
                                        o.ctypes.data_as(llp) if o is not None else None, i.size, int(n), int(n_off),
                                        int(device), va, stats.ctypes.data_as(llp), bt.ctypes.data_as(dp),
                                        scored.ctypes.data_as(llp), values.ctypes.data_as(dp) if values is not None else None)
    _lib.check(rc, "ppk_network_summary")
    return stats, bt, scored, (values[:int(n)] if values is not None else None)


def growNetwork(sample_names, i_vec, j_vec, idx_vec, s_range, score_idx=0, thread_idx=0,
                betweenness_sample=betweenness_sample_default, write_clusters=None, sample_size=None,
                use_gpu=False):
    """PopPUNK/refine.py:375-474 (see the module docstring for what is not mirrored).  idx_vec: each edge's offset
    index, as thresholdIterate1D/2D return it; the graph of step idx holds every edge of index <= idx.  score_idx > 0
    raises NotImplementedError here; the device path for betweenness scores is
    engine.refine_sweep_scores_dev(..., score_idx=...) (or grow_scores with network_summary's bt)."""
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
