"""The boundary-assignment half of PopPUNK's refine/threshold models on the MI355X.

Mirrors what `RefineFit.assign` / `RefineFit.apply_threshold` (PopPUNK/models.py:956-994,
:1065-1091) do around kernel 2, and the hand-off `construct_network_from_assignments` makes to
`generateTuples` (PopPUNK/network.py:1170-1184), and the fit itself (`RefineFit.fit`, models.py:807-954;
DESIGN.md 3.14).

  * `fit(X, sample_names, model, max_move, min_move, ...)` / `fit_dev(dist_t, ...)` : the boundary refined from the
                           means of a fitted BGMMModel / DBSCANModel or a manual start file (refine.refineFit on the
                           device), then the core-only and accessory-only boundaries for `indiv_refine`
  * `save(prefix)` / `from_npz(source)` : `<prefix>_fit.npz` with `RefineFit.save`'s keys

  * `assign(X)`          : `poppunk_refine.assignThreshold(X/self.scale, slope, x_max, y_max)` with
                           the slope -> (x_max, y_max) mapping of the reference
                           (2: optimal_x/optimal_y, 0: core_boundary/0, 1: 0/accessory_boundary)
  * `assign_dev(dist_t)` : the same on a resident CUDA matrix (float32 division on the device is
                           the IEEE division numpy does)
  * `edges(X)`           : assign -> generateTuples(y, within_label = -1)
  * `edges_from_sketches(db, ...)` : distances, X/scale, boundary and edge compaction fused in
                           one pass (`engine.dist_edges`): the distance matrix never exists

`BGMMModel` is the same for PopPUNK's default model, a fitted Bayesian Gaussian mixture: the assignment half of
`BGMMFit` (PopPUNK/models.py:359-375 load, :411-465 assign; PopPUNK/bgmm.py:100-176 log_likelihood) and the
edge list `construct_network_from_assignments` builds from it.

`DBSCANModel` is PopPUNK's `--fit-model dbscan` (DBSCANFit, PopPUNK/models.py:468-783), fit and assignment: core
distances, the mutual-reachability spanning tree and the per-row assignment on the device, the hierarchy between
them on the host (poppunk_amd/dbscan.py).
"""
import ctypes as C
import os

import numpy as np

from . import engine, poppunk_refine

WITHIN_LABEL = -1          # RefineFit.within_label, PopPUNK/models.py:801


class RefineBoundary:
    """A fitted refine/threshold boundary (the state `RefineFit.assign` reads)."""

    def __init__(self, scale=(1.0, 1.0), slope=2, optimal_x=None, optimal_y=None,
                 core_boundary=None, accessory_boundary=None, threads=1):
        self.scale = np.asarray(scale, dtype=np.float32)
        self.slope = int(slope)
        self.optimal_x, self.optimal_y = optimal_x, optimal_y
        self.core_boundary, self.accessory_boundary = core_boundary, accessory_boundary
        self.threads = threads
        self.within_label = WITHIN_LABEL
        self.fitted = optimal_x is not None or core_boundary is not None or accessory_boundary is not None
        self.threshold = False
        self.indiv_fitted = False
        self.unconstrained = False
        self.mean0 = self.mean1 = self.min_move = self.max_move = None

    @classmethod
    def from_threshold(cls, threshold, dtype=np.float32):
        """RefineFit.apply_threshold (models.py:956-994): vertical line at core = threshold,
        scale (1, 1)."""
        b = cls(scale=np.array([1, 1], dtype=dtype), slope=0, optimal_x=threshold, optimal_y=np.nan,
                core_boundary=threshold, accessory_boundary=np.nan)
        b.threshold = True
        return b

    def _line(self, slope):
        if slope == 2:
            return self.optimal_x, self.optimal_y
        if slope == 0:
            return self.core_boundary, 0
        if slope == 1:
            return 0, self.accessory_boundary
        raise RuntimeError("slope must be 0, 1 or 2")

    def assign(self, X, slope=None):
        """models.py:1065-1091."""
        if not self.fitted:
            raise RuntimeError("Trying to assign using an unfitted model")
        if slope is None:
            slope = self.slope
        x_max, y_max = self._line(slope)
        return poppunk_refine.assignThreshold(X / self.scale, slope, x_max, y_max, self.threads)

    def assign_dev(self, dist_t, slope=None):
        if not self.fitted:
            raise RuntimeError("Trying to assign using an unfitted model")
        import torch
        if slope is None:
            slope = self.slope
        x_max, y_max = self._line(slope)
        scaled = dist_t / torch.as_tensor(self.scale, device=dist_t.device)
        return engine.assign_threshold_dev(scaled, slope, x_max, y_max)

    # ---- fitting (RefineFit.fit, models.py:807-954) ----------------------------------------------
    def _start_points(self, model, startFile):
        """mean0, mean1 in the scaled space: a manual start file, a DBSCAN fit's cluster means or a BGMM fit's
        component means (models.py:866-882).  Copies: the unconstrained search moves them in place."""
        import sys
        from . import refine
        if startFile:
            mean0, mean1, scaled = refine.readManualStart(startFile)
            if not scaled:
                mean0 /= self.scale
                mean1 /= self.scale
            return mean0, mean1
        if isinstance(model, DBSCANModel):
            sys.stderr.write("Initial model-based network construction based on DBSCAN fit\n")
            means = model.cluster_means
        elif isinstance(model, BGMMModel):
            sys.stderr.write("Initial model-based network construction based on Gaussian fit\n")
            means = model.means
        else:
            raise RuntimeError("Unrecognised model type")
        return (np.array(means[model.within_label, :], dtype=np.float64),
                np.array(means[model.between_label, :], dtype=np.float64))

    def fit_dev(self, dist_t, sample_names, model, max_move, min_move, startFile=None, indiv_refine=None,
                unconstrained=False, score_idx=0, no_local=False, betweenness_sample=100, sample_size=None,
                use_gpu=False, multi_boundary=0, outPrefix=None, sampled_betweenness=False, seed=0):
        """RefineFit.fit on a resident float32 [n(n-1)/2, 2] CUDA matrix: the 2-D refinement from the start points of
        `model` (a BGMMModel, a DBSCANModel, or `startFile`), then, for indiv_refine 'core' / 'accessory' / 'both',
        the slope-0 and slope-1 refinements, with the reference's fall-back when one of them fails.  Returns the
        assignment (assign_dev).  multi_boundary > 1: after the 2-D fit, refine.multi_refine writes the clusters at that
        many boundaries between the axis and the optimum under `outPrefix` (models.py:905-918); what it returns is kept
        in self.multi_boundary_clusters.  The fit itself is the same with or without it.  sampled_betweenness / seed:
        refine.refineFit's (score_idx 1 | 2 from at most betweenness_sample sources per component)."""
        import sys
        import torch
        from . import refine
        if sample_size is not None:
            raise NotImplementedError("RefineBoundary.fit: random vertex subsampling (sample_size) is not mirrored")
        self.scale = np.asarray(np.copy(model.scale), dtype=np.float32).reshape(2)
        self.max_move, self.min_move = max_move, min_move
        self.unconstrained = unconstrained
        self.mean0, self.mean1 = self._start_points(model, startFile)

        scaled = dist_t / torch.as_tensor(self.scale, device=dist_t.device)      # (the rule of assign_dev)
        scorer = refine.DeviceScorer(scaled)
        common = dict(score_idx=score_idx, no_local=no_local, num_processes=self.threads,
                      betweenness_sample=betweenness_sample, sample_size=sample_size, use_gpu=use_gpu,
                      sampled_betweenness=sampled_betweenness, seed=seed)
        self.optimal_x, self.optimal_y, self.optimal_s = refine.refineFit(
            scorer, sample_names, self.mean0, self.mean1, self.scale, max_move, min_move, slope=2,
            unconstrained=unconstrained, **common)
        self.slope = 2
        self.fitted = True
        self.threshold = False
        self.indiv_fitted = False

        if multi_boundary > 1:
            if outPrefix is None:
                raise ValueError("multi_boundary needs outPrefix")
            sys.stderr.write("Creating multiple boundary fits\n")
            self.multi_boundary_clusters = refine.multi_refine(
                scaled, sample_names, self.mean0, self.mean1, self.scale, self.optimal_s, multi_boundary, outPrefix,
                num_processes=self.threads, betweenness_sample=betweenness_sample, sample_size=sample_size,
                use_gpu=use_gpu)

        self.core_boundary = self.optimal_x
        self.accessory_boundary = self.optimal_y
        if indiv_refine is not None:
            try:
                for dist_type, slope in zip(['core', 'accessory'], [0, 1]):
                    if indiv_refine == 'both' or indiv_refine == dist_type:
                        sys.stderr.write("Refining " + dist_type + " distances separately\n")
                        core_boundary, accessory_boundary, _ = refine.refineFit(
                            scorer, sample_names, self.mean0, self.mean1, self.scale, max_move, min_move, slope=slope,
                            **common)
                        if dist_type == "core":
                            self.core_boundary = core_boundary
                        if dist_type == "accessory":
                            self.accessory_boundary = accessory_boundary
                self.indiv_fitted = True
            except RuntimeError as e:
                print(e)
                sys.stderr.write("Could not separately refine core and accessory boundaries. "
                                 "Using joint 2D refinement only.\n")
        return self.assign_dev(dist_t)

    def fit(self, X, sample_names, model, max_move, min_move, startFile=None, indiv_refine=None, unconstrained=False,
            score_idx=0, no_local=False, betweenness_sample=100, sample_size=None, use_gpu=False, device_id=0,
            multi_boundary=0, outPrefix=None, sampled_betweenness=False, seed=0):
        """fit_dev on a host float32 [n(n-1)/2, 2] array, uploaded once: the same model to the bit.  Returns the
        assignment as a numpy array."""
        import torch
        if sample_size is not None:
            raise NotImplementedError("RefineBoundary.fit: random vertex subsampling (sample_size) is not mirrored")
        X = np.ascontiguousarray(X, dtype=np.float32)
        y = self.fit_dev(torch.from_numpy(X).to("cuda:%d" % device_id), sample_names, model, max_move, min_move,
                         startFile=startFile, indiv_refine=indiv_refine, unconstrained=unconstrained,
                         score_idx=score_idx, no_local=no_local, betweenness_sample=betweenness_sample,
                         sample_size=sample_size, use_gpu=use_gpu, multi_boundary=multi_boundary, outPrefix=outPrefix,
                         sampled_betweenness=sampled_betweenness, seed=seed)
        return y.cpu().numpy()

    def plot(self, X, y=None, outPrefix=None, raster_above=1000000):
        """RefineFit.plot (models.py:1038-1062): plot.plot_refined_results into <outPrefix>/<basename>_refined_fit.png.
        X: a numpy array or a resident CUDA tensor; y: its assignments (None: assigned here, as the reference does).
        The reference draws a sample of 12 500 000 rows of a larger matrix; here every row is drawn (above
        raster_above rows as an occupancy raster made on the device).  outPrefix is required (ValueError without it):
        the model keeps no output directory of its own."""
        from . import plot as _plot
        if outPrefix is None:
            raise ValueError("plot needs outPrefix: the directory the picture is written into")
        prefix = outPrefix
        if y is None:
            y = self.assign_dev(X) if hasattr(X, "is_cuda") else self.assign(X)
        _plot.plot_refined_results(X, y, self.optimal_x, self.optimal_y, self.core_boundary, self.accessory_boundary,
                                   self.mean0, self.mean1, self.min_move, self.max_move, self.scale, self.threshold,
                                   self.indiv_fitted, self.unconstrained, "Refined fit boundary",
                                   prefix + "/" + os.path.basename(prefix) + "_refined_fit", raster_above=raster_above)

    def save(self, prefix):
        """`<prefix>/<basename>_fit.npz` with RefineFit.save's keys (models.py:996-1005: intercept,
        core_acc_intercepts, scale, indiv_fitted), which `from_npz` and PopPUNK's RefineFit.load read.  No `_fit.pkl`
        is written.  Returns the path."""
        import os
        if not self.fitted:
            raise RuntimeError("Trying to save unfitted model")
        prefix = str(prefix)
        os.makedirs(prefix, exist_ok=True)
        path = os.path.join(prefix, os.path.basename(os.path.normpath(prefix)) + "_fit.npz")
        np.savez(path, intercept=np.array([self.optimal_x, self.optimal_y]),
                 core_acc_intercepts=np.array([self.core_boundary, self.accessory_boundary]), scale=self.scale,
                 indiv_fitted=self.indiv_fitted)
        return path

    @classmethod
    def from_npz(cls, source):
        """RefineFit.load (models.py:1010-1036) from a path to `<prefix>_fit.npz` or a mapping of its arrays, a file
        PopPUNK wrote included: a file without `indiv_fitted` predates it (False), and NaN in both `intercept[1]` and
        `core_acc_intercepts[1]` marks a threshold model."""
        if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
            with np.load(source, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        else:
            d = dict(source)
        missing = [k for k in ("intercept", "core_acc_intercepts", "scale") if k not in d]
        if missing:
            raise ValueError("not a refine fit: missing %s" % ", ".join(missing))
        b = cls(scale=d["scale"], slope=2, optimal_x=np.asarray(d["intercept"]).item(0),
                optimal_y=np.asarray(d["intercept"]).item(1),
                core_boundary=np.asarray(d["core_acc_intercepts"]).item(0),
                accessory_boundary=np.asarray(d["core_acc_intercepts"]).item(1))
        b.indiv_fitted = bool(np.asarray(d["indiv_fitted"]).item()) if "indiv_fitted" in d else False
        if np.isnan(b.optimal_y) and np.isnan(b.accessory_boundary):
            b.threshold = True
        return b

    def edges(self, X, self_comparison=True, num_ref=0, int_offset=0, slope=None):
        """assign -> generateTuples(assignments, within_label, self, num_ref, int_offset):
        the connections construct_network_from_assignments passes on (network.py:1180-1184)."""
        y = self.assign(X, slope)
        return poppunk_refine.generateTuples(y, self.within_label, self=self_comparison,
                                             num_ref=num_ref, int_offset=int_offset)

    def edges_from_sketches(self, db, qry_db, kmers, random_tbl, slope=None, return_rows=False, **kw):
        """CUDA int64 [n_edges, 2]: (i, j) of every pair strictly within the boundary, in the
        order generateTuples would emit them; and n_failed.  return_rows: (edges, rows, n_failed), rows float32
        [n_edges, 2] the unscaled (core, accessory) of every edge from the same pass (engine.dist_edges_rows)."""
        if not self.fitted:
            raise RuntimeError("Trying to assign using an unfitted model")
        if slope is None:
            slope = self.slope
        x_max, y_max = self._line(slope)
        call = engine.dist_edges_rows if return_rows else engine.dist_edges
        return call(db, qry_db, kmers, random_tbl, slope=slope, x_max=float(x_max),
                    y_max=float(y_max), scale=tuple(float(v) for v in self.scale),
                    inclusive=False, **kw)

    def fit_from_sketches(self, db, kmers, random_tbl, sample_names, model, max_move, min_move, startFile=None,
                          indiv_refine=None, unconstrained=False, score_idx=0, no_local=False, betweenness_sample=100,
                          sample_size=None, use_gpu=False, outPrefix=None, sampled_betweenness=False, seed=0,
                          random_correct=True):
        """fit_dev without the [n_pairs, 2] matrix: refine.refineFit driven by a refine.SketchScorer
        on the resident sketches of `db` (a self job), the same searches, evaluations and attributes as fit_dev on
        engine.dist(db, ...).  No assignment vector exists without the matrix: returns
        self.edges_from_sketches(db, None, kmers, random_tbl) -- (edges, n_failed), the edges fit_dev's assignment gives
        through generateTuples.  Clusters at several boundaries (multi_boundary) need the matrix route."""
        import sys
        from . import refine
        if sample_size is not None:
            raise NotImplementedError("RefineBoundary.fit: random vertex subsampling (sample_size) is not mirrored")
        self.scale = np.asarray(np.copy(model.scale), dtype=np.float32).reshape(2)
        self.max_move, self.min_move = max_move, min_move
        self.unconstrained = unconstrained
        self.mean0, self.mean1 = self._start_points(model, startFile)

        scorer = refine.SketchScorer(db, kmers, random_tbl, self.scale, random_correct=random_correct)
        if unconstrained:
            # the far corner of the 20 x 20 grid, as refineFit sets it up: one list for every row of the grid
            from .utils import decisionBoundary
            gradient = (self.mean1[1] - self.mean0[1]) / (self.mean1[0] - self.mean0[0])
            scorer.prime(2, *decisionBoundary(self.mean1, gradient, adj=max_move))
        common = dict(score_idx=score_idx, no_local=no_local, num_processes=self.threads,
                      betweenness_sample=betweenness_sample, sample_size=sample_size, use_gpu=use_gpu,
                      sampled_betweenness=sampled_betweenness, seed=seed)
        self.optimal_x, self.optimal_y, self.optimal_s = refine.refineFit(
            scorer, sample_names, self.mean0, self.mean1, self.scale, max_move, min_move, slope=2,
            unconstrained=unconstrained, **common)
        self.slope = 2
        self.fitted = True
        self.threshold = False
        self.indiv_fitted = False
        self.core_boundary = self.optimal_x
        self.accessory_boundary = self.optimal_y
        if indiv_refine is not None:
            try:
                for dist_type, slope in zip(['core', 'accessory'], [0, 1]):
                    if indiv_refine == 'both' or indiv_refine == dist_type:
                        sys.stderr.write("Refining " + dist_type + " distances separately\n")
                        core_boundary, accessory_boundary, _ = refine.refineFit(
                            scorer, sample_names, self.mean0, self.mean1, self.scale, max_move, min_move, slope=slope,
                            **common)
                        if dist_type == "core":
                            self.core_boundary = core_boundary
                        if dist_type == "accessory":
                            self.accessory_boundary = accessory_boundary
                self.indiv_fitted = True
            except RuntimeError as e:
                print(e)
                sys.stderr.write("Could not separately refine core and accessory boundaries. "
                                 "Using joint 2D refinement only.\n")
        self.fit_passes = scorer.passes
        return self.edges_from_sketches(db, None, kmers, random_tbl, random_correct=random_correct)


# ---- BGMM assignment (PopPUNK's default --fit-model bgmm) -----------------------------------------------
SAMPLE_ROWS_PERMUTE_MAX = 1 << 27


def sample_rows(n_rows, max_samples, seed):
    """The rows a fit trains on when there are more than `max_samples`; None when every row is used.  Up to 2^27 rows
    this is `DBSCANModel.subsample_index`, the draw the matrix routes make (a permutation's head).  Above that a
    permutation is the matrix problem again -- 5e9 rows are 40 GB of host memory -- and the rows are
    `default_rng(seed).choice(n_rows, max_samples, replace=False)`, whose memory is O(max_samples)."""
    n_rows, max_samples = int(n_rows), int(max_samples)
    if n_rows <= SAMPLE_ROWS_PERMUTE_MAX:
        return DBSCANModel.subsample_index(n_rows, max_samples, seed)
    if n_rows <= max_samples:
        return None
    return np.random.default_rng(seed).choice(n_rows, max_samples, replace=False).astype(np.int64, copy=False)


def _training_rows(db, kmers, random_tbl, max_samples, seed, rows, random_correct):
    """float32 [m, 2] CUDA tensor: the distances of the training rows of `db`'s self job, from its sketches."""
    import torch
    n_rows = db.n * (db.n - 1) // 2
    if rows is None:
        rows = sample_rows(n_rows, max_samples, seed)
    if rows is None:
        rows = np.arange(n_rows, dtype=np.int64)
    pairs_t = torch.as_tensor(engine.rows_to_pairs(rows, db.n), device="cuda:%d" % db.device)
    dist_t, _ = engine.dist_pairs(db, None, kmers, random_tbl, pairs_t, random_correct=random_correct)
    return dist_t


class BGMMModel:
    """PopPUNK's default model, a Bayesian Gaussian mixture: `BGMMFit.fit` / `.assign` / `.save` / `.load`
    (PopPUNK/models.py:296-465).  The constructor takes fitted arrays (the state `BGMMFit.assign` reads).

      * `fit(X, max_components, ...)` / `fit_dev(dist_t, max_components, ...)` : class methods returning a fitted
                                      model: subsample, scale, the variational fit on the device (include/ppk.h
                                      "BGMM fit"), assignment, within / between labels.  `max_samples=None` fits on
                                      every row.  `fit_info` and `labels` describe the fit.
      * `save(prefix)`              : `<prefix>/<basename>_fit.npz` with `BGMMFit.save`'s keys (models.py:341-352)
      * `from_npz(path_or_mapping)` : the arrays `BGMMFit.load` reads from `<prefix>_fit.npz` (models.py:359-375);
                                      the `_fit.pkl` is never opened (unpickling needs sklearn and runs code)
      * `assign(X, values=False)`   : `BGMMFit.assign` (models.py:411-465) through ppk_bgmm_assign: int64 labels, or
                                      the float32 [n, K] responsibilities with values=True
      * `assign_dev(dist_t, values=False)` : the same on a resident CUDA matrix (int32 labels / float32 resp)
      * `edges(X, ...)`             : assign -> generateTuples(y, within_label, ...) (network.py:1170-1184)
      * `edges_from_sketches(db, qry_db, kmers, random_tbl)` : distances, assignment and edge compaction fused
                                      in one pass (engine.dist_bgmm_edges): the distance matrix never exists
      * `edges_host(refs, qrys, kmers, random_tbl)` : the same on one or several devices into a host array
    """

    def __init__(self, weights, means, covariances, scale, within_label, between_label=None):
        from . import _lib
        self.weights = np.asarray(weights, dtype=np.float64).reshape(-1)
        K = self.weights.shape[0]
        self.means = np.asarray(means, dtype=np.float64).reshape(K, 2)
        self.covariances = np.asarray(covariances, dtype=np.float64).reshape(K, 2, 2)
        self.scale = np.asarray(scale)
        if self.scale.dtype not in (np.float32, np.float64):
            self.scale = self.scale.astype(np.float64)
        self.within_label = int(within_label)
        self.between_label = None if between_label is None else int(between_label)
        self.n_components = K
        # PopPUNK's scale is np.amax of the float32 matrix: X / scale is then a float32 quotient; a float64 scale
        # gives a float64 one (numpy's promotion, models.py:246-254)
        self._model = _lib.Bgmm()
        arrays = [np.ascontiguousarray(a, dtype=np.float64)
                  for a in (self.weights, self.means, self.covariances, self.scale.reshape(2))]
        ptrs = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrays]
        rc = _lib.lib().ppk_bgmm_prepare(K, *ptrs, 1 if self.scale.dtype == np.float64 else 0, self.within_label,
                                         self._model)
        if rc == _lib.ERR_ARG:      # the reference's ValueError (bgmm.py:170-172) and bad shapes
            raise ValueError(_lib.last_error())
        _lib.check(rc, "ppk_bgmm_prepare")
        self.fitted = True
        self.fit_info = None        # set by fit / fit_dev
        self.fit_result = None
        self.labels = None
        self.assign_points = True

    # -- fitting -------------------------------------------------------------------------------------------------
    @staticmethod
    def _fit_inputs(n_rows, max_components, max_samples, seed, n_init, init_labels):
        params = engine.bgmm_fit_params(max_components, n_init=1 if init_labels is not None else n_init)
        idx = None if max_samples is None else DBSCANModel.subsample_index(n_rows, max_samples, seed)
        return params, idx

    @classmethod
    def _fitted(cls, res, scale, seed, init, assign_points, labels_of):
        """The model of a `bgmm.FitResult`: BGMMFit.fit after fit2dMultiGaussian (models.py:326-338).
        labels_of(model) -> (the labels, the number of rows per label)."""
        from . import bgmm
        model = cls(res.weights, res.means, res.covariances, scale, 0)
        y, counts = labels_of(model)
        model = cls(res.weights, res.means, res.covariances, scale, bgmm.within_from_counts(res.means, counts),
                    bgmm.between_from_counts(counts))
        model.labels = y
        model.fit_result, model.assign_points, model.seed = res, bool(assign_points), int(seed)
        model.fit_info = {"n_iter": res.n_iter, "converged": res.converged, "lower_bound": res.lower_bound,
                          "lower_bounds": res.lower_bounds, "n_train": res.n_train, "init": init,
                          "best_init": res.best_init, "init_lower_bounds": res.init_lower_bounds,
                          "kmeans_iter": res.kmeans_iter}
        return model

    @classmethod
    def fit(cls, X, max_components, max_samples=100000, seed=42, assign_points=True, device_id=0, init_labels=None,
            n_init=5):
        """`BGMMFit.fit` (models.py:305-338) from a host matrix; returns the fitted model, whose `labels` are the
        int64 assignments of X (`assign_points`) or of the subsample.  More rows than `max_samples`: a seeded
        subsample (`DBSCANModel.subsample_index`); `max_samples=None`: every row.  scale = np.amax of the training
        rows.  `init_labels` (one per training row) replaces the own initialisation (one run); otherwise `n_init`
        runs from k-means++ centres drawn with seeds seed, seed + 1, ... (poppunk_amd/bgmm.py)."""
        from . import bgmm
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != 2:
            raise ValueError("X must be [n, 2] (core, accessory)")
        params, idx = cls._fit_inputs(X.shape[0], max_components, max_samples, seed, n_init, init_labels)
        sub = X if idx is None else X[idx]
        if sub.shape[0] < 1:
            raise ValueError("no rows to fit")
        scale = np.amax(sub, axis=0)
        centres = None
        if init_labels is None:
            centres = bgmm.initial_centres(lambda pos: sub if pos is None else sub[pos], sub.shape[0], scale,
                                           params.K, seed, params.n_init)
        res = engine.bgmm_fit(X, scale, params, index=idx, init_labels=init_labels, init_centres=centres,
                              device_id=device_id)

        def labels_of(model):
            y = model.assign(X if assign_points else sub, device_id=device_id)
            return y, np.bincount(y, minlength=params.K)
        return cls._fitted(res, scale, seed, "labels" if init_labels is not None else "kmeans++", assign_points,
                           labels_of)

    @classmethod
    def fit_dev(cls, dist_t, max_components, max_samples=100000, seed=42, assign_points=True, init_labels=None,
                n_init=5):
        """The same from a resident CUDA matrix: the training rows are read where they are (through the subsample's
        index list, or all of them); besides the sums of each pass, only the scale and the k-means++ draw's rows (at
        most 4 096 per run) come to the host.  `labels` is an int32 CUDA tensor."""
        from . import bgmm
        import torch
        engine._check_dist_tensor(dist_t)
        params, idx = cls._fit_inputs(dist_t.shape[0], max_components, max_samples, seed, n_init, init_labels)
        dev = dist_t.device
        idx_t = None if idx is None else torch.as_tensor(idx, device=dev)
        n_train = dist_t.shape[0] if idx is None else idx.shape[0]
        if n_train < 1:
            raise ValueError("no rows to fit")
        scale = (dist_t if idx_t is None else dist_t[idx_t]).amax(dim=0).cpu().numpy()

        def fetch(pos):
            if pos is None:
                return (dist_t if idx_t is None else dist_t[idx_t]).cpu().numpy()
            at = torch.as_tensor(pos if idx is None else idx[pos], device=dev)
            return dist_t[at].cpu().numpy()
        centres, lab_t = None, None
        if init_labels is None:
            centres = bgmm.initial_centres(fetch, n_train, scale, params.K, seed, params.n_init)
        else:
            lab_t = torch.as_tensor(np.ascontiguousarray(init_labels, dtype=np.int32), device=dev)
        res = engine.bgmm_fit_dev(dist_t, scale, params, index_t=idx_t, init_labels_t=lab_t, init_centres=centres)
        rows_t = dist_t if (assign_points or idx_t is None) else dist_t[idx_t].contiguous()

        def labels_of(model):
            y = model.assign_dev(rows_t)
            return y, torch.bincount(y, minlength=params.K).cpu().numpy()
        return cls._fitted(res, scale, seed, "labels" if init_labels is not None else "kmeans++", assign_points,
                           labels_of)

    @classmethod
    def fit_from_sketches(cls, db, kmers, random_tbl, max_components, max_samples=100000, seed=42, init_labels=None,
                          n_init=5, rows=None, random_correct=True):
        """The fit without a distance matrix: the training rows -- `rows`, or `sample_rows` of the
        self job's n (n - 1) / 2 -- are computed from the resident database `db` as a pair list (engine.dist_pairs),
        and fitted by `fit_dev` on that [m, 2] tensor as it stands (max_samples=None, assign_points=False): `labels`
        are the subsample's, `within_label` comes from their counts.  The model equals fit_dev's on the same rows of
        the dense matrix bit for bit."""
        dist_t = _training_rows(db, kmers, random_tbl, max_samples, seed, rows, random_correct)
        return cls.fit_dev(dist_t, max_components, max_samples=None, seed=seed, assign_points=False,
                           init_labels=init_labels, n_init=n_init)

    def plot(self, X, y, outPrefix=None, raster_above=1000000):
        """The two pictures of BGMMFit.plot (models.py:404-408): plot.plot_results into <outPrefix>/<basename>_DPGMM_fit
        .png and plot.plot_contours into ..._DPGMM_fit_contours.pdf.  X, y: numpy arrays or resident CUDA tensors (y as
        `assign` / `assign_dev` return it).  The "Fit summary" entropy line of the reference is not written.  outPrefix is
        required (ValueError without it): the model keeps no output directory of its own."""
        from . import plot as _plot
        if outPrefix is None:
            raise ValueError("plot needs outPrefix: the directory the picture is written into")
        prefix = outPrefix
        used = int((_plot._label_counts(y, 0, self.n_components) > 0).sum())
        title = "DPGMM – estimated number of spatial clusters: " + str(used)
        outfile = prefix + "/" + os.path.basename(prefix) + "_DPGMM_fit"
        _plot.plot_results(X, y, self.means, self.covariances, self.scale, title, outfile, raster_above=raster_above)
        _plot.plot_contours(self, y, title + " assignment boundary", outfile + "_contours")

    def save(self, prefix):
        """`<prefix>/<basename>_fit.npz` with exactly `BGMMFit.save`'s keys (models.py:341-352: weights, means,
        covariances, within, between, scale), which `from_npz` and PopPUNK's `BGMMFit.load` read, plus -- for a model
        fitted here -- the variational state, `n_iter`, `lower_bound` and `seed` under `ppk_*` keys.  No `_fit.pkl`
        is written: the reference's holds a pickled sklearn object.  Returns the path."""
        import os
        self._check()
        prefix = str(prefix)
        os.makedirs(prefix, exist_ok=True)
        path = os.path.join(prefix, os.path.basename(os.path.normpath(prefix)) + "_fit.npz")
        extra = {}
        if self.fit_result is not None:
            r = self.fit_result
            extra = {"ppk_weight_concentration": r.weight_concentration, "ppk_mean_precision": r.mean_precision,
                     "ppk_degrees_of_freedom": r.degrees_of_freedom, "ppk_n_iter": r.n_iter,
                     "ppk_converged": r.converged, "ppk_lower_bound": r.lower_bound,
                     "ppk_lower_bounds": r.lower_bounds, "ppk_n_train": r.n_train, "ppk_seed": self.seed}
        np.savez(path, weights=self.weights, means=self.means, covariances=self.covariances, within=self.within_label,
                 between=self.between_label if self.between_label is not None else -1, scale=self.scale, **extra)
        return path

    @classmethod
    def from_npz(cls, source):
        """`source`: a path to `<prefix>_fit.npz` or a mapping of its arrays."""
        if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
            with np.load(source, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        else:
            d = dict(source)
        keys = set(d)
        if {"intercept", "core_acc_intercepts"} & keys:
            raise ValueError("this is a refine/threshold fit (RefineFit, models.py:1001-1026): use RefineBoundary")
        if {"n_clusters", "maxs", "mins"} & keys:
            raise ValueError("this is a DBSCAN fit (DBSCANFit, models.py:618-657): its assignment "
                             "(hdbscan.approximate_predict) needs the fitted condensed tree and has no per-row closed "
                             "form, so it is not supported here")
        missing = [k for k in ("weights", "means", "covariances", "scale", "within", "between") if k not in keys]
        if missing:
            raise ValueError("not a BGMM fit: missing %s" % ", ".join(missing))
        return cls(d["weights"], d["means"], d["covariances"], d["scale"], np.asarray(d["within"]).item(),
                   np.asarray(d["between"]).item())

    @property
    def model(self):
        """The prepared `_lib.Bgmm` the entry points take."""
        return self._model

    def _check(self):
        if not self.fitted:
            raise RuntimeError("Trying to assign using an unfitted model")

    def assign(self, X, values=False, device_id=0):
        """models.py:411-465: int64 labels [n] (np.zeros(n, dtype=int)), or float32 responsibilities [n, K] with
        values=True (the array has X's dtype in the reference; distances are float32)."""
        from . import _lib
        self._check()
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != 2:
            raise ValueError("X must be [n, 2] (core, accessory)")
        n = X.shape[0]
        lab = None if values else np.empty(n, dtype=np.int32)
        resp = np.empty((n, self.n_components), dtype=np.float32) if values else None
        rc = _lib.lib().ppk_bgmm_assign(X.ctypes.data_as(C.POINTER(C.c_float)), n, self._model, int(device_id),
                                        lab.ctypes.data_as(C.POINTER(C.c_int32)) if lab is not None else None,
                                        resp.ctypes.data_as(C.POINTER(C.c_float)) if resp is not None else None)
        _lib.check(rc, "ppk_bgmm_assign")
        return resp if values else lab.astype(np.int64)

    def assign_dev(self, dist_t, values=False):
        self._check()
        lab, resp = engine.bgmm_assign_dev(dist_t, self._model, labels=not values, values=values)
        return resp if values else lab

    def edges(self, X, self_comparison=True, num_ref=0, int_offset=0):
        """assign -> generateTuples(assignments, within_label, self, num_ref, int_offset) (network.py:1180-1184)."""
        y = self.assign(X)
        return poppunk_refine.generateTuples(y, self.within_label, self=self_comparison, num_ref=num_ref,
                                             int_offset=int_offset)

    def edges_from_sketches(self, db, qry_db, kmers, random_tbl, return_rows=False, **kw):
        """CUDA int64 [n_edges, 2]: the pairs assigned within_label, in generateTuples order; and n_failed.
        return_rows: (edges, rows, n_failed), rows float32 [n_edges, 2] the (core, accessory) of every edge from the
        same pass (engine.dist_bgmm_edges_rows)."""
        self._check()
        call = engine.dist_bgmm_edges_rows if return_rows else engine.dist_bgmm_edges
        return call(db, qry_db, kmers, random_tbl, model=self._model, **kw)

    def edges_host(self, refs, qrys, kmers, random_tbl, **kw):
        """The same as a host int64 [m, 2] array over every device holding a copy of the database; and n_failed."""
        self._check()
        return engine.bgmm_edges_host(refs, qrys, kmers, random_tbl, model=self._model, **kw)


# ---- DBSCAN (PopPUNK's --fit-model dbscan) ----------------------------------------------------------------------
class DBSCANModel:
    """PopPUNK's HDBSCAN model: `DBSCANFit.fit` / `.assign` / `.save` / `.load` (PopPUNK/models.py:468-783).

      * `fit(X, max_num_clusters, min_cluster_prop, ...)` : subsample, scale, and the reference's loop over
                                      (min_samples, min_cluster_size) until the within- and between-strain clusters are
                                      distinct; RuntimeError where the reference exits.  Returns the labels of X.
      * `fit_dev(dist_t, ...)`      : the same from a resident CUDA matrix (the subsample is gathered on the device)
      * `assign(X)` / `assign_dev(dist_t)` : int64 labels [n] / int32 CUDA labels [n]
      * `edges(X, ...)` / `edges_dev(dist_t, ...)` : assign -> generateTuples(y, within_label, ...)
      * `save(prefix)` / `from_npz(path_or_mapping)` : `<prefix>_fit.npz` with the reference's keys plus this model's
                                      own state under `ppk_*` keys (allow_pickle=False both ways)
    The subsample is a seeded `numpy.random.Generator` permutation (the reference's `random.randint` seed cannot be
    reproduced).  What "a DBSCAN fit" means here is written down in include/ppk.h, section DBSCAN."""

    FORMAT_VERSION = 1
    _STATE = ("points", "core2", "pt_cluster", "pt_lambda", "cl_parent", "cl_birth", "cl_label", "labels")

    def __init__(self):
        self.fitted = False
        self._handles = {}
        self.assign_points = True

    # -- state ---------------------------------------------------------------------------------------------------
    def _set_state(self, points, core2, tree, min_samples, min_cluster_size):
        self.points = np.ascontiguousarray(points, dtype=np.float32)
        self.core2 = np.ascontiguousarray(core2, dtype=np.float64)
        self.pt_cluster = np.ascontiguousarray(tree.pt_cluster, dtype=np.int32)
        self.pt_lambda = np.ascontiguousarray(tree.pt_lambda, dtype=np.float64)
        self.cl_parent = np.ascontiguousarray(tree.cl_parent, dtype=np.int32)
        self.cl_birth = np.ascontiguousarray(tree.cl_birth, dtype=np.float64)
        self.cl_label = np.ascontiguousarray(tree.cl_label, dtype=np.int32)
        self.labels = np.ascontiguousarray(tree.labels, dtype=np.int32)
        self.min_samples, self.min_cluster_size = int(min_samples), int(min_cluster_size)
        self._drop_handles()

    def _drop_handles(self):
        from . import _lib
        for h in self._handles.values():
            _lib.lib().ppk_dbscan_destroy(h)
        self._handles = {}

    def __del__(self):
        try:
            self._drop_handles()
        except Exception:
            pass

    def _create(self, scale, within_label, device_id):
        from . import _lib
        scale = np.asarray(scale)
        s64 = np.ascontiguousarray(scale.reshape(2), dtype=np.float64)
        h = C.c_void_p()
        f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        rc = _lib.lib().ppk_dbscan_create(
            self.points.ctypes.data_as(C.POINTER(C.c_float)), self.core2.ctypes.data_as(f64p), self.points.shape[0],
            self.min_samples, self.pt_cluster.ctypes.data_as(i32p), self.pt_lambda.ctypes.data_as(f64p),
            self.cl_parent.ctypes.data_as(i32p), self.cl_birth.ctypes.data_as(f64p), self.cl_label.ctypes.data_as(i32p),
            self.cl_parent.shape[0], s64.ctypes.data_as(f64p), 1 if scale.dtype == np.float64 else 0,
            int(within_label), int(device_id), C.byref(h))
        if rc == _lib.ERR_ARG:
            raise ValueError(_lib.last_error())
        _lib.check(rc, "ppk_dbscan_create")
        return h

    def handle(self, device_id=0):
        """The model on `device_id` as the `ppk_dbscan_*` entry points take it (made on first use)."""
        self._check()
        device_id = int(device_id)
        if device_id not in self._handles:
            self._handles[device_id] = self._create(self.scale, self.within_label, device_id)
        return self._handles[device_id]

    def _check(self):
        if not self.fitted:
            raise RuntimeError("Trying to assign using an unfitted model")

    # -- fitting -------------------------------------------------------------------------------------------------
    @staticmethod
    def subsample_index(n_rows, max_samples, seed):
        """Rows of the subsample, in the order they are fitted in; None when every row is used."""
        if max_samples is None or n_rows <= max_samples:
            return None
        return np.random.default_rng(seed).permutation(n_rows)[:max_samples]

    def _fit_loop(self, sub, tree_of, max_num_clusters, min_cluster_prop, device_id):
        """models.py:515-600 on the scaled subsample `sub`; tree_of(min_samples) -> (core2, a, b, mr2)."""
        from . import _lib, dbscan
        n = sub.shape[0]
        min_samples = dbscan.min_samples_for(n, min_cluster_prop)
        min_cluster_size = dbscan.min_cluster_size_for(n)
        indistinct = True
        self.fitted = False
        while dbscan.loop_continues(indistinct, min_samples, min_cluster_size):
            core2, a, b, mr2 = tree_of(min_samples)
            tree = dbscan.fit_tree(a, b, mr2, n, min_cluster_size)
            n_clusters = tree.n_clusters
            if dbscan.acceptable(n_clusters, max_num_clusters):
                self._set_state(sub, core2, tree, min_samples, min_cluster_size)
                self.n_clusters = n_clusters
                sub64 = sub.astype(np.float64)
                self.cluster_means = np.stack([sub64[tree.labels == k].mean(axis=0) for k in range(n_clusters)])
                self.cluster_mins = np.stack([sub64[tree.labels == k].min(axis=0) for k in range(n_clusters)])
                self.cluster_maxs = np.stack([sub64[tree.labels == k].max(axis=0) for k in range(n_clusters)])
                # the reference assigns the (already scaled) subsample back through the model, scale (1, 1)
                h = self._create(np.ones(2, dtype=np.float32), 0, device_id)
                try:
                    y = np.empty(n, dtype=np.int32)
                    _lib.check(_lib.lib().ppk_dbscan_assign(sub.ctypes.data_as(C.POINTER(C.c_float)), n, h,
                                                            y.ctypes.data_as(C.POINTER(C.c_int32))), "ppk_dbscan_assign")
                finally:
                    _lib.lib().ppk_dbscan_destroy(h)
                self.subsample_labels = y.astype(np.int64)
                self.within_label = dbscan.findWithinLabel(self.cluster_means, y)
                try:
                    self.between_label = dbscan.findBetweenLabel(y, self.within_label)
                except ValueError:
                    self.between_label = None
                indistinct = (self.between_label is None or
                              dbscan.evaluate_dbscan_clusters(self.cluster_mins, self.cluster_maxs, self.within_label,
                                                              self.between_label))
            min_samples, min_cluster_size = dbscan.next_parameters(min_samples, min_cluster_size)
        if indistinct:
            raise RuntimeError("Failed to find distinct clusters in this dataset")
        self.fitted = True

    def fit(self, X, max_num_clusters, min_cluster_prop, max_samples=100000, seed=42, assign_points=True, device_id=0):
        from . import _lib
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != 2:
            raise ValueError("X must be [n, 2] (core, accessory)")
        idx = self.subsample_index(X.shape[0], max_samples, seed)
        sub = np.array(X if idx is None else X[idx], dtype=np.float32, order="C")
        self.scale = np.amax(sub, axis=0)
        if not np.all(np.isfinite(sub)) or not np.all(self.scale > 0):
            raise ValueError("distances must be finite, with a positive maximum in both columns")
        sub /= self.scale
        self.assign_points = bool(assign_points)
        n = sub.shape[0]

        def tree_of(min_samples):
            core2 = np.empty(n, dtype=np.float64)
            a, b = np.empty(n - 1, dtype=np.int32), np.empty(n - 1, dtype=np.int32)
            mr2 = np.empty(n - 1, dtype=np.float64)
            f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
            rc = _lib.lib().ppk_dbscan_fit(sub.ctypes.data_as(C.POINTER(C.c_float)), n, int(min_samples),
                                           int(device_id), core2.ctypes.data_as(f64p), a.ctypes.data_as(i32p),
                                           b.ctypes.data_as(i32p), mr2.ctypes.data_as(f64p))
            if rc == _lib.ERR_ARG:
                raise ValueError(_lib.last_error())
            _lib.check(rc, "ppk_dbscan_fit")
            return core2, a, b, mr2

        self._fit_loop(sub, tree_of, max_num_clusters, min_cluster_prop, device_id)
        return self.assign(X, device_id=device_id) if self.assign_points else self.subsample_labels

    def fit_dev(self, dist_t, max_num_clusters, min_cluster_prop, max_samples=100000, seed=42, assign_points=True):
        import torch
        engine._check_dist_tensor(dist_t)
        idx = self.subsample_index(dist_t.shape[0], max_samples, seed)
        sub_t = dist_t.clone() if idx is None else dist_t[torch.as_tensor(idx, device=dist_t.device)]
        scale_t = sub_t.amax(dim=0)
        self.scale = scale_t.cpu().numpy()
        if not bool(torch.isfinite(sub_t).all()) or not np.all(self.scale > 0):
            raise ValueError("distances must be finite, with a positive maximum in both columns")
        sub_t = (sub_t / scale_t).contiguous()          # IEEE float32 division, as numpy's
        self.assign_points = bool(assign_points)

        def tree_of(min_samples):
            core2_t = engine.dbscan_core_dev(sub_t, min_samples)
            a_t, b_t, w_t = engine.dbscan_mst_dev(sub_t, core2_t)
            return core2_t.cpu().numpy(), a_t.cpu().numpy(), b_t.cpu().numpy(), w_t.cpu().numpy()

        self._fit_loop(sub_t.cpu().numpy(), tree_of, max_num_clusters, min_cluster_prop, dist_t.device.index)
        if self.assign_points:
            return self.assign_dev(dist_t)
        return torch.as_tensor(self.subsample_labels.astype(np.int32), device=dist_t.device)

    def fit_from_sketches(self, db, kmers, random_tbl, max_num_clusters, min_cluster_prop, max_samples=100000, seed=42,
                          rows=None, random_correct=True):
        """`fit_dev` without a distance matrix, as BGMMModel.fit_from_sketches: the training rows come from the
        resident database as a pair list; returns the subsample's labels (int32 CUDA tensor)."""
        dist_t = _training_rows(db, kmers, random_tbl, max_samples, seed, rows, random_correct)
        return self.fit_dev(dist_t, max_num_clusters, min_cluster_prop, max_samples=None, seed=seed,
                            assign_points=False)

    # -- assignment ----------------------------------------------------------------------------------------------
    def assign(self, X, device_id=0):
        """models.py:707-783: int64 labels [n] (np.zeros(n, dtype=int))."""
        from . import _lib
        self._check()
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != 2:
            raise ValueError("X must be [n, 2] (core, accessory)")
        lab = np.empty(X.shape[0], dtype=np.int32)
        _lib.check(_lib.lib().ppk_dbscan_assign(X.ctypes.data_as(C.POINTER(C.c_float)), X.shape[0],
                                                self.handle(device_id), lab.ctypes.data_as(C.POINTER(C.c_int32))),
                   "ppk_dbscan_assign")
        return lab.astype(np.int64)

    def assign_dev(self, dist_t):
        self._check()
        return engine.dbscan_assign_dev(dist_t, self.handle(dist_t.device.index))

    def edges(self, X, self_comparison=True, num_ref=0, int_offset=0, device_id=0):
        """assign -> generateTuples(assignments, within_label, self, num_ref, int_offset) (network.py:1180-1184)."""
        y = self.assign(X, device_id=device_id)
        return poppunk_refine.generateTuples(y, self.within_label, self=self_comparison, num_ref=num_ref,
                                             int_offset=int_offset)

    def edges_dev(self, dist_t, n_ref=0, int_offset=0, cap=None):
        """CUDA int64 [m, 2]: the rows assigned within_label, in generateTuples order (n_ref 0: self)."""
        self._check()
        return engine.dbscan_edges_dev(dist_t, self.handle(dist_t.device.index), n_ref=n_ref, int_offset=int_offset,
                                       cap=cap)

    def plot(self, X, y=None, outPrefix=None, raster_above=1000000):
        """DBSCANFit.plot's picture (models.py:695-704): plot.plot_dbscan_results into <outPrefix>/<basename>_dbscan.png.
        X: the un-scaled distances, a numpy array or a resident CUDA tensor; y: their assignments (None: assigned
        here).  The reference draws its fit's subsample; any matrix may be passed here.  outPrefix is required
        (ValueError without it): the model keeps no output directory of its own."""
        from . import plot as _plot
        if outPrefix is None:
            raise ValueError("plot needs outPrefix: the directory the picture is written into")
        prefix = outPrefix
        if y is None:
            y = self.assign_dev(X) if hasattr(X, "is_cuda") else self.assign(X)
        _plot.plot_dbscan_results(X, y, self.n_clusters, prefix + "/" + os.path.basename(prefix) + "_dbscan",
                                  raster_above=raster_above)

    # -- persistence ---------------------------------------------------------------------------------------------
    def save(self, prefix):
        """`<prefix>_fit.npz`: DBSCANFit.save's keys (models.py:618-627) and the `ppk_*` arrays.  Returns the path."""
        if not self.fitted:
            raise RuntimeError("Trying to save unfitted model")
        path = str(prefix) + "_fit.npz"
        np.savez(path, n_clusters=self.n_clusters, within=self.within_label, between=self.between_label,
                 means=self.cluster_means, maxs=self.cluster_maxs, mins=self.cluster_mins, scale=self.scale,
                 assign_points=self.assign_points, use_gpu=True,
                 ppk_format=self.FORMAT_VERSION, ppk_min_samples=self.min_samples,
                 ppk_min_cluster_size=self.min_cluster_size,
                 **{"ppk_" + k: getattr(self, k) for k in self._STATE})
        return path

    @classmethod
    def from_npz(cls, source):
        """`source`: a path to `<prefix>_fit.npz` or a mapping of its arrays."""
        if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
            with np.load(source, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        else:
            d = dict(source)
        keys = set(d)
        if {"intercept", "core_acc_intercepts"} & keys:
            raise ValueError("this is a refine/threshold fit (RefineFit, models.py:1001-1026): use RefineBoundary")
        if {"weights", "covariances"} & keys:
            raise ValueError("this is a BGMM fit (BGMMFit, models.py:359-375): use BGMMModel")
        missing = [k for k in ("n_clusters", "within", "between", "means", "maxs", "mins", "scale") if k not in keys]
        if missing:
            raise ValueError("not a DBSCAN fit: missing %s" % ", ".join(missing))
        need = ["ppk_format", "ppk_min_samples", "ppk_min_cluster_size"] + ["ppk_" + k for k in cls._STATE]
        if any(k not in keys for k in need):
            raise ValueError("this DBSCAN fit was written by PopPUNK: its state is a pickled hdbscan.HDBSCAN object "
                             "(<prefix>_fit.pkl), which cannot be read without that package and is never unpickled "
                             "here; fit the database again with DBSCANModel.fit, which saves its own arrays")
        if int(np.asarray(d["ppk_format"]).item()) != cls.FORMAT_VERSION:
            raise ValueError("unknown DBSCANModel format version %s" % np.asarray(d["ppk_format"]).item())
        m = cls()

        class _T:
            pass
        t = _T()
        for k in ("pt_cluster", "pt_lambda", "cl_parent", "cl_birth", "cl_label", "labels"):
            setattr(t, k, d["ppk_" + k])
        m._set_state(d["ppk_points"], d["ppk_core2"], t, np.asarray(d["ppk_min_samples"]).item(),
                     np.asarray(d["ppk_min_cluster_size"]).item())
        if m.points.ndim != 2 or m.points.shape[1] != 2 or any(
                getattr(m, k).shape[0] != m.points.shape[0] for k in ("core2", "pt_cluster", "pt_lambda")):
            raise ValueError("inconsistent ppk_* arrays in the DBSCAN fit")
        m.n_clusters = int(np.asarray(d["n_clusters"]).item())
        m.within_label = int(np.asarray(d["within"]).item())
        m.between_label = int(np.asarray(d["between"]).item())
        m.cluster_means, m.cluster_maxs, m.cluster_mins = d["means"], d["maxs"], d["mins"]
        m.scale = np.asarray(d["scale"])
        if m.scale.dtype not in (np.float32, np.float64):
            m.scale = m.scale.astype(np.float64)
        m.assign_points = bool(np.asarray(d["assign_points"]).item()) if "assign_points" in keys else True
        m.fitted = True
        return m


# ---- the lineage models' neighbour matrices (PopPUNK/models.py:1095-1385) -----------------------------
EPSILON = 1e-10            # PopPUNK/models.py:75: sparse matrices hold no explicit zeros


def rankFile(rank):
    """PopPUNK/models.py:78-79: the file suffix of one rank's fit."""
    return '_rank_' + str(rank) + '_fit.npz'


class LineageRanks:
    """The state `LineageFit` builds and reads -- `nn_dists` (the neighbours at the search depth) and
    `lower_rank_dists[rank]`, scipy COO matrices -- with the same steps behind the same method names:

      * `fit(X)`                   : models.py:1188-1237 on a long-form distance matrix:
                                     longToSquare -> get_kNN_distances -> lowerRank per rank
      * `fit_from_database(...)`   : the same matrices straight from the sketches
                                     (`pp_sketchlib.queryDatabaseKNN`): no distance matrix in any form
      * `extend(qqDists, qrDists)` : models.py:1334-1385, queries added to a fitted model
      * `assign(rank)` / `edge_weights(rank)` : models.py:1300-1332
    As in the reference a rank equal to the search depth without link filtering is stored as it is
    (`reduce_rank`, models.py:1095-1107) and distances below 1e-10 are raised to it (`__save_sparse__`)."""

    def __init__(self, ranks, max_search_depth, reciprocal_only=False, count_unique_distances=False,
                 lineage_resolution=EPSILON, dist_col=0, threads=1):
        self.ranks = sorted(int(r) for r in ranks)
        if self.ranks[0] < 1:
            raise RuntimeError("Rank must be at least 1")
        self.max_search_depth = max(int(max_search_depth), self.ranks[-1] + 5)      # models.py:1126
        self.reciprocal_only = bool(reciprocal_only)
        self.count_unique_distances = bool(count_unique_distances)
        self.resolution = lineage_resolution
        self.dist_col = int(dist_col)
        self.threads = threads
        self.nn_dists = None
        self.lower_rank_dists = {}
        self.fitted = False

    @staticmethod
    def _coo(data, row, col, n_samples):
        from scipy.sparse import coo_matrix
        data = np.array(data, dtype=np.float32)
        data[data < EPSILON] = EPSILON
        return coo_matrix((data, (np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64))),
                          shape=(n_samples, n_samples), dtype=np.float32)

    def _ranks_from(self, higher, n_samples):
        i, j, d = higher
        for rank in self.ranks:
            if rank == self.max_search_depth and not self.reciprocal_only and not self.count_unique_distances:
                self.lower_rank_dists[rank] = self._coo(d, i, j, n_samples)
            else:
                li, lj, ld = poppunk_refine.lowerRank_arrays((i, j, d), n_samples, rank, self.reciprocal_only,
                                                             self.count_unique_distances, self.resolution,
                                                             self.threads)
                self.lower_rank_dists[rank] = self._coo(ld, li, lj, n_samples)

    def _search_depth(self, n_samples):
        if self.ranks[-1] >= n_samples:
            raise RuntimeError("Maximum rank must be less than the number of samples: " + str(n_samples))
        return min(self.max_search_depth, n_samples - 1)

    def fit(self, X):
        from . import pp_sketchlib
        X = np.asarray(X)
        n = int(round(0.5 * (1 + np.sqrt(1 + 8 * X.shape[0]))))
        depth = self._search_depth(n)
        square = pp_sketchlib.longToSquare(np.ascontiguousarray(X[:, self.dist_col]), self.threads)
        i, j, d = poppunk_refine.get_kNN_distances(square, depth, self.dist_col, self.threads)
        return self._fitted((np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64),
                             np.asarray(d, dtype=np.float32)), depth, n)

    def fit_from_database(self, db_name, names, klist, random_correct=True, device_id=0):
        from . import pp_sketchlib
        n = len(names)
        depth = self._search_depth(n)
        if depth > 32:
            raise RuntimeError("neighbours straight from the sketches: search depth <= 32 (fit(X) has no limit)")
        return self._fitted(pp_sketchlib.queryDatabaseKNN(db_name, names, klist, depth, self.dist_col,
                                                          random_correct, device_id=device_id), depth, n)

    def _fitted(self, higher, depth, n):
        self.nn_dists = self._coo(higher[2], higher[0], higher[1], n)
        self._ranks_from(higher, n)
        self.fitted = True
        return self.assign(self.ranks[0])

    def extend(self, qqDists, qrDists):
        from . import pp_sketchlib
        if not self.fitted:
            raise RuntimeError("Trying to extend an unfitted model")
        qq = pp_sketchlib.longToSquare(np.ascontiguousarray(np.asarray(qqDists)[:, self.dist_col]), self.threads)
        qq[qq < EPSILON] = EPSILON
        n_ref, n_query = self.nn_dists.shape[0], qq.shape[1]
        qr = np.asarray(qrDists)[:, self.dist_col].reshape(n_query, n_ref).T
        qr = np.where(qr < EPSILON, np.float32(EPSILON), qr).astype(np.float32)
        higher = poppunk_refine.extend_arrays((self.nn_dists.row, self.nn_dists.col, self.nn_dists.data), qq, qr,
                                              self.max_search_depth, self.threads)
        self.nn_dists = self._coo(higher[2], higher[0], higher[1], n_ref + n_query)
        self._ranks_from(higher, n_ref + n_query)
        return self.assign(self.ranks[0])

    def extend_from_databases(self, ref_db_name, query_db_name, rList, qList, klist, random_correct=True,
                              device_id=0):
        """`extend` for queries that are still sketches (`pp_sketchlib.extendFromDatabases`): the same matrices,
        without the query x reference and query x query distance matrices."""
        from . import pp_sketchlib
        if not self.fitted:
            raise RuntimeError("Trying to extend an unfitted model")
        if self.max_search_depth > 32:
            raise RuntimeError("neighbours straight from the sketches: search depth <= 32 (extend(qq, qr) has no limit)")
        higher = pp_sketchlib.extendFromDatabases((self.nn_dists.row, self.nn_dists.col, self.nn_dists.data),
                                                  ref_db_name, query_db_name, rList, qList, klist,
                                                  self.max_search_depth, self.dist_col, random_correct,
                                                  device_id=device_id)
        n = len(rList) + len(qList)
        self.nn_dists = self._coo(higher[2], higher[0], higher[1], n)
        self._ranks_from((higher[0], higher[1], self.nn_dists.data), n)
        return self.assign(self.ranks[0])

    def save(self, prefix):
        """LineageFit.save (models.py:1240-1262) with `prefix` for its outPrefix: `<prefix>/<basename>_sparse_dists.npz`,
        one `<basename>_rank_<r>_fit.npz` per rank (rankFile, models.py:78-79) and `<basename>_fit.pkl` holding
        [[ranks, max_search_depth, reciprocal_only, count_unique_distances, dist_col, resolution], 'lineage']."""
        import pickle

        import scipy.sparse
        if not self.fitted:
            raise RuntimeError("Trying to save unfitted model")
        stem = os.path.join(prefix, os.path.basename(prefix))
        scipy.sparse.save_npz(stem + "_sparse_dists.npz", self.nn_dists)
        for rank in self.ranks:
            scipy.sparse.save_npz(stem + rankFile(rank), self.lower_rank_dists[rank])
        with open(stem + "_fit.pkl", "wb") as pickle_file:
            pickle.dump([[self.ranks, self.max_search_depth, self.reciprocal_only, self.count_unique_distances,
                          self.dist_col, self.resolution], "lineage"], pickle_file)

    @classmethod
    def load(cls, prefix):
        """The model `save(prefix)` wrote (loadClusterFit's lineage branch, models.py:127-140, and LineageFit.load,
        :1264-1276; the rank matrices too, as assign.py reads them back)."""
        import pickle

        import scipy.sparse
        stem = os.path.join(prefix, os.path.basename(prefix))
        with open(stem + "_fit.pkl", "rb") as pickle_file:
            fit_obj, fit_type = pickle.load(pickle_file)
        if fit_type != "lineage":
            raise RuntimeError("not a lineage model: " + str(fit_type))
        ranks, depth, reciprocal_only, count_unique_distances, dist_col, resolution = fit_obj
        m = cls(ranks, depth, reciprocal_only, count_unique_distances, resolution, dist_col)
        m.max_search_depth = depth
        m.nn_dists = scipy.sparse.load_npz(stem + "_sparse_dists.npz")
        m.lower_rank_dists = {rank: scipy.sparse.load_npz(stem + rankFile(rank)) for rank in m.ranks}
        m.fitted = True
        return m

    def assign(self, rank):
        if not self.fitted:
            raise RuntimeError("Trying to assign using an unfitted model")
        m = self.lower_rank_dists[rank]
        return list(zip(m.row.tolist(), m.col.tolist()))

    def edge_weights(self, rank):
        if not self.fitted:
            raise RuntimeError("Trying to get weights from an unfitted model")
        return self.lower_rank_dists[rank].data
