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

Fitting the boundary mirrors PopPUNK/refine.py:51-247 and :476-664:

    refineFit(distMat, sample_names, mean0, mean1, scale, max_move, min_move, slope=2, score_idx=0,
              unconstrained=False, no_local=False, num_processes=1, betweenness_sample=100, sample_size=None,
              use_gpu=False) -> (optimal_x, optimal_y, optimised_s)
    newNetwork(s, ...), newNetwork2D(y_idx, ...), check_search_range(...), readManualStart(startFile)

`distMat` is a float32 [n(n-1)/2, 2] numpy array (uploaded once per call) or a resident CUDA tensor; the sweeps, every
evaluation of the local search and the 2-D grid run on that one tensor and no edge list leaves the device.  The local
search is scipy's bounded minimiser, as upstream; its objective takes the four integer counts of one boundary from
ppk_refine_score_dev, or, between the two lines of the search's bounds, from the bracket handle ppk_refine_local_*
(option refine_local, 1 by default; both give the same counts, hence the same fit).  score_idx 1 and 2 evaluate through
edge_threshold_dev + network_summary_graph_dev; with sampled_betweenness=True (and seed=s) the sweep and the local search
score from at most betweenness_sample Brandes sources per component instead (ppk_network_summary_sampled, DESIGN.md
3.8).  `num_processes` and `use_gpu` are accepted and ignored; `sample_size`
raises NotImplementedError before the device is touched.  `last_fit` describes the latest refineFit call: the global
scores, the bounds, every evaluation of the local search (s, counts, score), which path scored it, and the betweenness
mode ("exact" / "sampled") with its sample size and seed.

Clusters at several boundaries mirrors PopPUNK/refine.py:249-312:

    multi_refine(distMat, sample_names, mean0, mean1, scale, s_max, n_boundary_points, output_prefix, ...)
        -> (numbers int32 [n_files, n], file indices)

one thresholdIterate1D sweep, one ppk_cluster_sweep_dev for the cluster numbers of every graph, and the files
growNetwork(write_clusters=...) would write (boundary_files states its index rule).  It makes its own device calls.

Not mirrored by growNetwork (NotImplementedError, raised before the device is touched): betweenness scores
(score_idx > 0; the device path for those is engine.refine_sweep_scores_dev(..., score_idx=...)),
random vertex subsampling (sample_size), and writing each step's clusters (write_clusters: multi_refine writes them).
`use_gpu` selects cugraph upstream; it is accepted and ignored (this is the device path either way).
"""
import ctypes as C
import sys
from itertools import chain

import numpy as np

from . import _lib
from .utils import decisionBoundary, transformLine

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


def network_summary_sampled(i_vec, j_vec, idx_vec, n, n_off=None, values_at=None, device=0, sources=100, seed=0,
                            whole_graph=False):
    """ppk_network_summary_sampled on host arrays: network_summary with at most `sources` Brandes sources per
    component, the sample fixed by `seed`.  whole_graph: `values` are vertex_betweenness(G, norm=True)
    of the whole graph (components of 3 vertices included, divisor (n - 1)(n - 2)); bt and scored do not change."""
    sources = int(sources)
    if sources < 1:
        raise ValueError("network_summary_sampled: sources must be >= 1")
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
    rc = _lib.lib().ppk_network_summary_sampled(
        i.ctypes.data_as(llp), j.ctypes.data_as(llp), o.ctypes.data_as(llp) if o is not None else None, i.size, int(n),
        int(n_off), int(device), va, stats.ctypes.data_as(llp), bt.ctypes.data_as(dp), scored.ctypes.data_as(llp),
        values.ctypes.data_as(dp) if values is not None else None, sources, int(seed) & 0xFFFFFFFFFFFFFFFF,
        _lib.BT_WHOLE_GRAPH if whole_graph else 0)
    _lib.check(rc, "ppk_network_summary_sampled")
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


# ---- fitting the boundary (PopPUNK/refine.py:51-247, :476-664) -----------------------------------
last_fit = {}          # the latest refineFit call: see the module docstring


def check_search_range(scale, mean0, mean1, lower_s, upper_s):
    """The axis intercepts at both ends of a search range along mean0 -> mean1, with the reference's report on stderr
    (PopPUNK/refine.py:314-352) -> ((min_x, max_x), (min_y, max_y))."""
    gradient = (mean1[1] - mean0[1]) / (mean1[0] - mean0[0])
    bottom_end = transformLine(lower_s, mean0, mean1)
    top_end = transformLine(upper_s, mean0, mean1)
    min_x, min_y = decisionBoundary(bottom_end, gradient)
    max_x, max_y = decisionBoundary(top_end, gradient)
    sys.stderr.write("Search range (" + ",".join(["{:.3f}".format(x) for x in bottom_end * scale]) + ") to (" +
                     ",".join(["{:.3f}".format(x) for x in top_end * scale]) + ")\n")
    sys.stderr.write("Searching core intercept from " + "{:.3f}".format(min_x * scale[0]) + " to " +
                     "{:.3f}".format(max_x * scale[0]) + "\n")
    sys.stderr.write("Searching accessory intercept from " + "{:.3f}".format(min_y * scale[1]) + " to " +
                     "{:.3f}".format(max_y * scale[1]) + "\n")
    return ((min_x, max_x), (min_y, max_y))


def boundary_of_s(s, mean0, mean1, gradient, slope=2):
    """(x_max, y_max) of the boundary at distance s along mean0 -> mean1, as newNetwork sets it up
    (refine.py:523-532), in double; the device calls narrow it to float32 as pybind11 does for edgeThreshold."""
    new_intercept = transformLine(s, mean0, mean1)
    if slope == 2:
        x_max, y_max = decisionBoundary(new_intercept, gradient)
    elif slope == 0:
        x_max = new_intercept[0]
        y_max = 0
    elif slope == 1:
        x_max = 0
        y_max = new_intercept[1]
    else:
        raise RuntimeError("slope must be 0, 1 or 2")
    return x_max, y_max


class DeviceScorer:
    """What refineFit asks of the device, on one resident matrix: the two sweeps' score lists, the counts of one
    boundary, and the bracket handle.  (The CPU tests drive refineFit with a stand-in of the same four methods.)"""

    def __init__(self, distMat, device_id=0):
        import torch
        from . import engine
        self.engine = engine
        if isinstance(distMat, torch.Tensor):
            self.dist_t = distMat
        else:
            X = np.ascontiguousarray(distMat, dtype=np.float32)
            if X.ndim != 2 or X.shape[1] != 2:
                raise ValueError("distMat must be a float32 [n, 2] array")
            self.dist_t = torch.from_numpy(X).to("cuda:%d" % device_id)
        self.n_rows = int(self.dist_t.shape[0])
        self.bt_sources, self.bt_seed = None, 0

    def set_betweenness_sample(self, sources, seed=0):
        """score_idx 1 / 2 from at most `sources` Brandes sources per component (None: every source, the default)"""
        if sources is not None and int(sources) < 1:
            raise ValueError("betweenness_sample must be >= 1")
        self.bt_sources, self.bt_seed = (None if sources is None else int(sources)), int(seed)

    def sweep_1d(self, s_range, slope, mean0, mean1, score_idx):
        """-> (rows the sweep lists, growNetwork's list)"""
        stats, scores = self.engine.refine_sweep_scores_dev(self.dist_t, s_range, slope, mean0[0], mean0[1], mean1[0],
                                                            mean1[1], score_idx, self.bt_sources, self.bt_seed)
        return int(stats[-1, 0].item()), scores

    def sweep_2d(self, x_range, y_max, score_idx):
        stats, scores = self.engine.refine_sweep_scores_2d_dev(self.dist_t, x_range, y_max, score_idx,
                                                               self.bt_sources, self.bt_seed)
        return int(stats[-1, 0].item()), scores

    def score(self, slope, x_max, y_max, score_idx):
        """-> (counts int64 [4], betweenness means or None) of one boundary"""
        if score_idx == 0:
            return self.engine.refine_score_dev(self.dist_t, slope, x_max, y_max), None
        edges = self.engine.edge_threshold_dev(self.dist_t, slope, x_max, y_max)
        n = self.engine._samples_of(self.n_rows)
        if self.bt_sources is None:
            stats, bt, _, _ = self.engine.network_summary_graph_dev(edges, n)
        else:
            stats, bt, _, _ = self.engine.network_summary_sampled_graph_dev(edges, n, sources=self.bt_sources,
                                                                            seed=self.bt_seed)
        return stats.cpu().numpy(), bt.cpu().numpy()

    def bracket(self, slope, lo, hi):
        """-> an object with eval(x_max, y_max) -> counts and split, or None (the lines are not nested)"""
        return self.engine.RefineLocal.create(self.dist_t, slope, lo[0], lo[1], hi[0], hi[1])


class _SketchBracket:
    """SketchScorer.bracket's handle: the counts of any line between two nested lines, from the candidates of the
    upper one.  split = (rows within the lower line, further rows within the upper one, the rest), exact counts (the
    matrix route's handle sorts with a margin; nothing reads the numbers but last_fit)."""

    def __init__(self, scorer, slope, lo, hi):
        self.scorer, self.slope = scorer, slope
        self.edges, self.rows = scorer._candidates(slope, [hi[0]], [hi[1]])
        eng = scorer.engine
        within_hi = int((eng.assign_threshold_dev(self.rows, slope, hi[0], hi[1]) <= 0).sum().item())
        within_lo = int((eng.assign_threshold_dev(self.rows, slope, lo[0], lo[1]) <= 0).sum().item())
        self.split = (within_lo, within_hi - within_lo, scorer.n_rows - within_hi)

    def eval(self, x_max, y_max):
        return self.scorer._counts(self.edges, self.rows, self.slope, x_max, y_max)[0]

    def close(self):
        self.edges = self.rows = None


class SketchScorer:
    """DeviceScorer's interface on a resident engine.SketchDB self job: refineFit without the [n_pairs, 2] matrix
    (DESIGN.md 3.26).  One fused pass (engine.dist_edges_rows) under an OUTER line yields the candidate pairs with their
    rows; the exact verdict of every boundary then comes from the sweeps' and assign_threshold_dev's own statements on
    the candidates' scaled rows (rows / scale in float32, the rule fit_dev applies to the matrix).

    The outer line is a superset filter by construction: the largest x_max and the largest y_max of the request, each
    pushed out by 2^-10 relatively (a row the float test of a boundary accepts lies within ~2^-20 of its exact line).
    The last candidate list is kept with its un-inflated outer intercepts: a request whose boundaries all lie inside it
    (same slope, every x_max and y_max no larger) is served from it.  A request with an intercept that is not positive
    and finite where its slope reads it (a slope-2 line on an axis takes line_dist's sqrt branch) is not cached: one
    boundary takes a fused pass under that very line, a sweep a pass that lists every pair."""

    MARGIN = 1.0 + 2.0 ** -10

    def __init__(self, db, kmers, random_tbl, scale, random_correct=True):
        import torch
        from . import engine
        self.engine, self.torch = engine, torch
        self.db, self.kmers, self.random_tbl, self.random_correct = db, kmers, random_tbl, random_correct
        self.scale = np.asarray(scale, dtype=np.float32).reshape(2)
        self.n = int(db.n)
        self.n_rows = self.n * (self.n - 1) // 2
        self.bt_sources, self.bt_seed = None, 0
        self._cache = None            # (slope, x_outer, y_outer, edges, scaled rows)
        self.passes = 0               # fused passes run so far

    def set_betweenness_sample(self, sources, seed=0):
        if sources is not None and int(sources) < 1:
            raise ValueError("betweenness_sample must be >= 1")
        self.bt_sources, self.bt_seed = (None if sources is None else int(sources)), int(seed)

    # ---- candidates -----------------------------------------------------------------------------------------------
    def _pass(self, slope, x_max, y_max):
        edges, rows, _ = self.engine.dist_edges_rows(self.db, None, self.kmers, self.random_tbl,
                                                     random_correct=self.random_correct, slope=slope, x_max=x_max,
                                                     y_max=y_max, scale=(float(self.scale[0]), float(self.scale[1])),
                                                     inclusive=True)
        self.passes += 1
        return edges, rows / self.torch.as_tensor(self.scale, device=rows.device)

    def _candidates(self, slope, x_maxes, y_maxes):
        """(edges int64 [m, 2], scaled rows float32 [m, 2]): every pair some boundary of the request may hold."""
        xs = np.asarray(x_maxes, dtype=np.float32).ravel()
        ys = np.asarray(y_maxes, dtype=np.float32).ravel()
        reads_x, reads_y = slope != 1, slope != 0
        ok = (not reads_x or bool(np.all(np.isfinite(xs) & (xs > 0)))) and \
             (not reads_y or bool(np.all(np.isfinite(ys) & (ys > 0))))
        if not ok:
            if xs.size == 1:
                return self._pass(slope, float(xs[0]), float(ys[0]))
            return self._pass(0, float("inf"), 0.0)          # x - inf <= 0: every pair
        xo = np.float32(xs.max()) if reads_x else np.float32(0)
        yo = np.float32(ys.max()) if reads_y else np.float32(0)
        c = self._cache
        if c is not None and c[0] == slope and xo <= c[1] and yo <= c[2]:
            return c[3], c[4]
        edges, rows = self._pass(slope, float(xo) * self.MARGIN, float(yo) * self.MARGIN)
        self._cache = (slope, xo, yo, edges, rows)
        return edges, rows

    def prime(self, slope, x_max, y_max):
        """Make the candidate list of an outer line now, so that every later request inside it is served from it (a
        search that works outwards, like the 2-D grid's rows of growing y, would otherwise make a list per step)."""
        self._candidates(slope, [x_max], [y_max])

    def _counts(self, edges, rows, slope, x_max, y_max, score_idx=0):
        """(counts int64 [4], betweenness means or None) of one boundary over a candidate list"""
        eng = self.engine
        sel = edges[eng.assign_threshold_dev(rows, slope, x_max, y_max) <= 0]
        if score_idx == 0:
            level = self.torch.zeros(sel.shape[0], dtype=self.torch.int64, device=sel.device)
            stats, _ = eng.network_sweep_dev(sel[:, 0], sel[:, 1], level, self.n, 1)
            return stats.cpu().numpy().reshape(-1, 4)[0], None
        if self.bt_sources is None:
            stats, bt, _, _ = eng.network_summary_graph_dev(sel, self.n)
        else:
            stats, bt, _, _ = eng.network_summary_sampled_graph_dev(sel, self.n, sources=self.bt_sources,
                                                                    seed=self.bt_seed)
        return stats.cpu().numpy(), bt.cpu().numpy()

    def _sweep(self, slope, x_max, y_max, score_idx):
        edges, rows = self._candidates(slope, x_max, y_max)
        n_off = int(x_max.size)
        level = self.engine.sweep_levels_dev(rows, x_max, y_max, slope)
        keep = level < n_off
        listed = edges[keep]
        sweep = (listed[:, 0], listed[:, 1], level[keep].to(self.torch.int64))
        stats, scores = self.engine._sweep_scores_of(self.n, sweep, n_off, score_idx, self.bt_sources, self.bt_seed)
        return int(stats[-1, 0].item()), scores

    # ---- DeviceScorer's four methods ------------------------------------------------------------------------------
    def sweep_1d(self, s_range, slope, mean0, mean1, score_idx):
        """-> (rows the sweep lists, growNetwork's list)"""
        x_max, y_max = self.engine.sweep_boundaries_1d(s_range, slope, mean0[0], mean0[1], mean1[0], mean1[1])
        return self._sweep(slope, x_max, y_max, self.engine._check_score_idx(score_idx))

    def sweep_2d(self, x_range, y_max, score_idx):
        x_max = np.ascontiguousarray(x_range, dtype=np.float32).ravel()
        if x_max.size > 1 and np.any(np.diff(x_max) < 0):
            raise RuntimeError("x_max range to thresholdIterate2D must be sorted")
        return self._sweep(2, x_max, np.full(x_max.size, y_max, dtype=np.float32),
                           self.engine._check_score_idx(score_idx))

    def score(self, slope, x_max, y_max, score_idx):
        """-> (counts int64 [4], betweenness means or None) of one boundary"""
        x_max, y_max = float(np.float32(x_max)), float(np.float32(y_max))
        edges, rows = self._candidates(slope, [x_max], [y_max])
        return self._counts(edges, rows, slope, x_max, y_max, score_idx)

    def bracket(self, slope, lo, hi):
        """-> an object with eval(x_max, y_max) -> counts and split, or None (the lines are not nested: the rule of
        ppk_refine_local_create_dev)"""
        lo = [np.float32(v) for v in lo]
        hi = [np.float32(v) for v in hi]
        tiny = np.float32(2.0 ** -40)
        if slope == 0:
            nested = lo[0] <= hi[0]
        elif slope == 1:
            nested = lo[1] <= hi[1]
        else:
            nested = (lo[0] <= hi[0] and lo[1] <= hi[1] and lo[0] >= tiny and lo[1] >= tiny
                      and bool(np.isfinite(hi[0])) and bool(np.isfinite(hi[1])))
        if not nested:
            return None
        return _SketchBracket(self, slope, [float(v) for v in lo], [float(v) for v in hi])


def _scorer_of(distMat, bt_sources=None, seed=0):
    scorer = distMat if hasattr(distMat, "sweep_1d") else DeviceScorer(distMat)
    if hasattr(scorer, "set_betweenness_sample"):
        scorer.set_betweenness_sample(bt_sources, seed)
    elif bt_sources is not None:
        raise TypeError("sampled_betweenness needs a scorer with set_betweenness_sample (DeviceScorer)")
    return scorer


def _check_fit_args(score_idx, sample_size, who):
    if sample_size is not None:
        raise NotImplementedError(who + ": random vertex subsampling (sample_size) is not mirrored")
    if score_idx not in (0, 1, 2):
        raise ValueError("score_idx must be 0, 1 or 2")


def newNetwork(s, sample_names, distMat, mean0, mean1, gradient, slope=2, score_idx=0, cpus=1,
               betweenness_sample=betweenness_sample_default, sample_size=None, use_gpu=False):
    """PopPUNK/refine.py:476-548: -score of the network of the boundary at s, in one device call
    (ppk_refine_score_dev; score_idx 1 / 2: edge_threshold_dev + network_summary_graph_dev)."""
    _check_fit_args(score_idx, sample_size, "newNetwork")
    scorer = _scorer_of(distMat)
    x_max, y_max = boundary_of_s(s, mean0, mean1, gradient, slope)
    stats, bt = scorer.score(slope, x_max, y_max, score_idx)
    return -summary_from_stats(stats, len(sample_names), bt)[1][score_idx]


def newNetwork2D(y_idx, sample_names, distMat, x_range, y_range, score_idx=0,
                 betweenness_sample=betweenness_sample_default, sample_size=None, use_gpu=False):
    """PopPUNK/refine.py:550-610: growNetwork's list over x_range at y_range[y_idx]; [0] * len(x_range) when the
    sweep lists every row."""
    _check_fit_args(score_idx, sample_size, "newNetwork2D")
    scorer = _scorer_of(distMat)
    y_max = y_range[y_idx]
    listed, scores = scorer.sweep_2d(x_range, y_max, score_idx)
    if listed == scorer.n_rows:
        scores = [0] * len(x_range)
    return scores


def _local_objective(scorer, n, mean0, mean1, gradient, slope, score_idx, bounds, evals, info):
    """newNetwork as the local search calls it, scoring through the bracket handle where one can be made: the two
    lines of the bounds, computed as newNetwork computes them and narrowed to float32, must be nested."""
    handle = None
    info["local_path"] = "summary" if score_idx > 0 else "score"
    if score_idx == 0 and _lib.get_option("refine_local") != 0 and hasattr(scorer, "bracket"):
        lo = [np.float32(v) for v in boundary_of_s(bounds[0], mean0, mean1, gradient, slope)]
        hi = [np.float32(v) for v in boundary_of_s(bounds[1], mean0, mean1, gradient, slope)]
        handle = scorer.bracket(slope, lo, hi)
        if handle is not None:
            info["local_path"] = "bracket"
            info["split"] = getattr(handle, "split", None)

    def inside(v, k):
        return lo[k] <= np.float32(v) <= hi[k]

    def objective(s):
        x_max, y_max = boundary_of_s(s, mean0, mean1, gradient, slope)
        if handle is not None and (slope == 1 or inside(x_max, 0)) and (slope == 0 or inside(y_max, 1)):
            stats, bt = handle.eval(x_max, y_max), None
        else:
            stats, bt = scorer.score(slope, x_max, y_max, score_idx)
        score = -summary_from_stats(stats, n, bt)[1][score_idx]
        evals.append((float(s), [int(v) for v in stats], float(score)))
        return score

    return objective, handle


def refineFit(distMat, sample_names, mean0, mean1, scale, max_move, min_move, slope=2, score_idx=0,
              unconstrained=False, no_local=False, num_processes=1, betweenness_sample=betweenness_sample_default,
              sample_size=None, use_gpu=False, sampled_betweenness=False, seed=0):
    """PopPUNK/refine.py:51-247: the global sweep (40 offsets along mean0 -> mean1, or the 20 x 20 grid of the
    unconstrained search), then scipy's bounded minimiser between the global minimum's neighbours
    -> (optimal_x, optimal_y, optimised_s).  sampled_betweenness=True (score_idx 1 | 2): the sweep and the local
    search score from at most betweenness_sample Brandes sources per component, the sample fixed by `seed` (DESIGN.md
    3.8); False, the default, ignores betweenness_sample as before."""
    global last_fit
    _check_fit_args(score_idx, sample_size, "refineFit")
    import scipy.optimize
    sampled = bool(sampled_betweenness) and score_idx > 0
    if sampled and int(betweenness_sample) < 1:
        raise ValueError("refineFit: betweenness_sample must be >= 1")
    info = {"global_s": None, "bounds": None, "evals": [], "local_path": None, "split": None,
            "betweenness": "sampled" if sampled else "exact", "betweenness_sample": int(betweenness_sample) if sampled
            else None, "seed": int(seed) if sampled else None}
    last_fit = info
    n = len(sample_names)
    sys.stderr.write("Trying to optimise score globally\n")

    gradient = (mean1[1] - mean0[1]) / (mean1[0] - mean0[0])

    if unconstrained:
        if slope != 2:
            raise RuntimeError("Unconstrained optimization and indiv-refine incompatible")

        global_grid_resolution = 20
        x_max_start, y_max_start = decisionBoundary(mean0, gradient, adj=-1 * min_move)
        x_max_end, y_max_end = decisionBoundary(mean1, gradient, adj=max_move)

        if x_max_start < 0 or y_max_start < 0:
            raise RuntimeError("Boundary range below zero")

        x_max = np.linspace(x_max_start, x_max_end, global_grid_resolution, dtype=np.float32)
        y_max = np.linspace(y_max_start, y_max_end, global_grid_resolution, dtype=np.float32)
        sys.stderr.write("Searching core intercept from " + "{:.3f}".format(x_max_start * scale[0]) + " to " +
                         "{:.3f}".format(x_max_end * scale[0]) + "\n")
        sys.stderr.write("Searching accessory intercept from " + "{:.3f}".format(y_max_start * scale[1]) + " to " +
                         "{:.3f}".format(y_max_end * scale[1]) + "\n")

        scorer = _scorer_of(distMat, int(betweenness_sample) if sampled else None, seed)
        global_s = [newNetwork2D(y_idx, sample_names, scorer, x_max, y_max, score_idx, betweenness_sample,
                                 sample_size, use_gpu) for y_idx in range(global_grid_resolution)]
        global_s = np.array(list(chain.from_iterable(global_s)))
        global_s[np.isnan(global_s)] = 1
        info["global_s"] = global_s
        min_idx = np.argmin(global_s)
        optimal_x = x_max[min_idx % global_grid_resolution]
        optimal_y = y_max[min_idx // global_grid_resolution]
        optimised_s = global_s[min_idx]

        if not (optimal_x > x_max_start and optimal_x < x_max_end and
                optimal_y > y_max_start and optimal_y < y_max_end):
            no_local = True
        elif not no_local:
            # the reference's parameterisation of the 1-D search along the found slope, kept as it stands
            gradient = optimal_x / optimal_y
            delta = x_max[1] - x_max[0]
            bounds = [-delta, delta]
            mean1 = (optimal_x + delta, delta * gradient)
    else:
        search_length = max_move + ((mean1[0] - mean0[0])**2 + (mean1[1] - mean0[1])**2)**0.5
        global_grid_resolution = 40
        s_range = np.linspace(-min_move, search_length, num=global_grid_resolution)
        (min_x, max_x), (min_y, max_y) = check_search_range(scale, mean0, mean1, s_range[0], s_range[-1])
        if min_x < 0 or min_y < 0:
            raise RuntimeError("Boundary range below zero")

        scorer = _scorer_of(distMat, int(betweenness_sample) if sampled else None, seed)
        listed, scores = scorer.sweep_1d(s_range, slope, mean0, mean1, score_idx)
        if listed == scorer.n_rows:
            raise RuntimeError("Boundary range includes all points")
        global_s = np.array(scores)
        global_s[np.isnan(global_s)] = 1
        info["global_s"] = global_s
        min_idx = np.argmin(np.array(global_s))
        if min_idx > 0 and min_idx < len(s_range) - 1:
            bounds = [s_range[min_idx - 1], s_range[min_idx + 1]]
        else:
            no_local = True
        if no_local:
            optimised_s = s_range[min_idx]

    if not no_local:
        sys.stderr.write("Trying to optimise score locally\n")
        info["bounds"] = [float(bounds[0]), float(bounds[1])]
        objective, handle = _local_objective(scorer, n, mean0, mean1, gradient, slope, score_idx, bounds,
                                             info["evals"], info)
        try:
            local_s = scipy.optimize.minimize_scalar(objective, bounds=bounds, method='Bounded',
                                                     options={'disp': True})
        finally:
            if handle is not None and hasattr(handle, "close"):
                handle.close()
        optimised_s = local_s.x

    if not unconstrained or not no_local:
        optimised_coor = transformLine(optimised_s, mean0, mean1)
        if slope == 2:
            optimal_x, optimal_y = decisionBoundary(optimised_coor, gradient)
            if optimal_x < 0 or optimal_y < 0:
                raise RuntimeError("Optimisation failed: produced a boundary outside of allowed range\n")
        else:
            optimal_x = optimised_coor[0]
            optimal_y = optimised_coor[1]
            if (slope == 0 and optimal_x < 0) or (slope == 1 and optimal_y < 0):
                raise RuntimeError("Optimisation failed: produced a boundary outside of allowed range\n")

    return optimal_x, optimal_y, optimised_s


def boundary_files(edge_counts, n_clusters, n):
    """Which `_boundary<k>_clusters.csv` files growNetwork(write_clusters=...) writes, and from which graph
    (PopPUNK/refine.py:435-472), from the per-offset edge counts and cluster counts of one sweep -> a list of
    (file index k, offset index of the graph).  The loop runs over the offset indices that add edges; the graph after
    index idx is written as boundary prev_idx + 1 .. idx (prev_idx starts at -1), so an index without edges of its own
    gets the NEXT graph that has some, not the one before it; only a graph with fewer clusters than samples is
    written; nothing is written after the last index with edges."""
    out = []
    prev_idx = -1
    for idx in np.flatnonzero(np.asarray(edge_counts).ravel() > 0).tolist():
        if int(n_clusters[idx]) < int(n):
            out.extend((k, idx) for k in range(prev_idx + 1, idx + 1))
        prev_idx = idx
    return out


def multi_refine(distMat, sample_names, mean0, mean1, scale, s_max, n_boundary_points, output_prefix,
                 num_processes=1, betweenness_sample=betweenness_sample_default, sample_size=None, use_gpu=False):
    """PopPUNK/refine.py:249-312: the boundary moved in n_boundary_points steps from where the line mean0 -> mean1
    meets an axis to the optimum s_max, and the clusters at each step written to
    `<output_prefix>/<basename>_boundary<k>_clusters.csv` (printClusters without unword names).

    distMat: the scaled float32 [n(n-1)/2, 2] matrix, a numpy array (uploaded once) or a resident CUDA tensor.  One
    threshold_iterate_1d_dev, one cluster_sweep_dev; only the rows that are written leave the device.  The reference
    returns None; this returns (numbers int32 [n_files, n]: row r is the number array of the r-th file; the file
    indices k).  `num_processes`, `betweenness_sample` and `use_gpu` are accepted and ignored; `sample_size` raises
    NotImplementedError before the device is touched."""
    if sample_size is not None:
        raise NotImplementedError("multi_refine: random vertex subsampling (sample_size) is not mirrored")
    import os
    import torch
    from . import engine, network

    # the range (refine.py:283-295): from where the line through mean0 and mean1, followed backwards from mean0, first
    # meets an axis -- x = 0 when mean0 lies on or above the line of the same slope through the origin, else y = 0 --
    # to the optimum; per unit of x the line is sqrt(1 + m^2) long, per unit of y sqrt(1 + 1 / m^2)
    m = (mean1[1] - mean0[1]) / (mean1[0] - mean0[0])
    meets_y_axis = mean0[1] >= m * mean0[0]
    s_start = -mean0[0] * np.sqrt(1 + m * m) if meets_y_axis else -mean0[1] * np.sqrt(1 + 1 / (m * m))
    s_range = np.linspace(s_start, s_max, num=n_boundary_points)
    x_ends, y_ends = check_search_range(scale, mean0, mean1, s_range[0], s_range[-1])
    if x_ends[0] < 0 or y_ends[0] < 0:
        sys.stderr.write("Boundary range below zero")

    dist_t = distMat if isinstance(distMat, torch.Tensor) else DeviceScorer(distMat).dist_t
    n = len(sample_names)
    n_off = len(s_range)
    i_t, j_t, idx_t = engine.threshold_iterate_1d_dev(dist_t, s_range, 2, mean0[0], mean0[1], mean1[0], mean1[1])
    clusters, counts = engine.cluster_sweep_dev(i_t.contiguous(), j_t.contiguous(), idx_t.contiguous(), n, n_off)
    edge_counts = torch.bincount(idx_t, minlength=n_off).cpu().numpy()
    files = boundary_files(edge_counts, counts.cpu().numpy(), n)
    rows = sorted(set(idx for _, idx in files))
    fetched = dict(zip(rows, clusters[torch.as_tensor(rows, dtype=torch.int64, device=clusters.device)].cpu().numpy())) \
        if rows else {}
    if files:
        os.makedirs(output_prefix, exist_ok=True)
    for k, idx in files:
        o_prefix = f"{output_prefix}/{os.path.basename(output_prefix)}_boundary{k}"
        network.print_cluster_numbers(fetched[idx], sample_names, outPrefix=o_prefix, write_unwords=False)
    kept = np.stack([fetched[idx] for _, idx in files]) if files else np.zeros((0, n), dtype=np.int32)
    return kept, [k for k, _ in files]


def readManualStart(startFile):
    """PopPUNK/refine.py:612-664: `start x,y`, `end x,y` and an optional `scaled False` line -> (mean0, mean1, scaled);
    a badly formed file is reported on stderr and ends the process, as upstream."""
    mean0 = None
    mean1 = None
    scaled = True

    with open(startFile, 'r') as start:
        for line in start:
            (param, value) = line.rstrip().split()
            if param == 'start':
                mean0 = np.array([float(v) for v in value.split(',')])
            elif param == 'end':
                mean1 = np.array([float(v) for v in value.split(',')])
            elif param == 'scaled':
                if value == "False" or value == "false":
                    scaled = False
            else:
                raise RuntimeError("Incorrectly formatted manual start file")
    try:
        if not isinstance(mean0, np.ndarray) or not isinstance(mean1, np.ndarray):
            raise RuntimeError('Must set both start and end')
        if mean0.shape != (2,) or mean1.shape != (2,):
            raise RuntimeError('Wrong size for values')
        for val in np.nditer(np.hstack([mean0, mean1])):
            if val > 1 or val < 0:
                raise RuntimeError('Value out of range (between 0 and 1)')
    except RuntimeError as e:
        sys.stderr.write("Could not read manual start file " + startFile + "\n")
        sys.stderr.write(str(e) + "\n")
        sys.exit(1)

    return mean0, mean1, scaled
