"""What engine.py raises for a faulty argument, and what `_lib.call` does with a status: pinned without a GPU and
without the built library.

Every wrapper of engine.py checks its arguments before it touches libppk_hip.so, so a call with exactly one faulty
argument raises before a device is needed.  A plain CPU tensor fails the first `is_cuda`; `cu(t)` makes a CPU tensor
that answers `is_cuda` with True (its device stays "cpu", so "same device" checks pass), which reaches the checks
behind the first one.  The table below is (callable, arguments) -> (exception type, exact message).

Raises of engine.py that no CPU-only call reaches, and why:
  * SketchDB.__init__ (five ValueErrors), dist ("out has the wrong size"), _host_edges ("one query database per
    reference database"), bgmm_fit_params (ERR_ARG -> ValueError, unknown parameter TypeError): not without the built
    library (rows_in_band and ppk_bgmm_fit_params_default are library calls, and the constructor used to load it first);
  * dist_pairs ("the pair list is not on the databases' device") and what follows it, knn_ref_query / knn_band /
    knn_from_sketches / knn_candidates after _check_pair: a CUDA allocation or a tensor with a device index comes first
    (_prep_tables' messages are reached through extend_from_sketches instead);
  * the ERR_ARG -> ValueError mapping of bgmm_stats_dev, bgmm_kmeans_dev, bgmm_fit_dev, bgmm_fit and dbscan_core_dev,
    every RuntimeError of `_lib.check`, and PeerStoreQuery.open's RuntimeErrors: the library call has to run (the
    mapping itself is pinned on `_lib.call` below);
  * strain_knn_dev ("the matrix must hold n(n-1)/2 rows") and nj_dev ("a long-form matrix must have n(n-1)/2 rows"):
    _samples_of raises its own ValueError for every such row count first;
  * PeerStoreQuery._check_against_gather's RuntimeError: it follows a run on the device.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from poppunk_amd import _lib, engine


class _CudaLike(torch.Tensor):
    is_cuda = True


def cu(t):
    return t.as_subclass(_CudaLike)


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def i64(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


D = cu(f32(3, 2))                    # a good condensed matrix: 3 rows, 3 samples
D4 = cu(f32(4, 2))                   # a good [n, 2] matrix whose row count is no n(n-1)/2
CPU_D = f32(4, 2)
E = cu(i64(3, 2))                    # a good [m, 2] edge list
CPU_E = i64(3, 2)
I, J = cu(i64(3)), cu(i64(3))        # a good (i, j) pair
LAB = cu(i32(4))
LEV = cu(i32(2, 3))
SEG = [0, 2, 4]
MEM = cu(i64(4))
NNJ, NND = cu(i64(4)), cu(f32(4))    # strain_knn_dev's lists for SEG at depth 1
DB = types.SimpleNamespace(nk=2, sketchsize64=2, bbits=14, device=0, n=5)
DB_OTHER = types.SimpleNamespace(nk=3, sketchsize64=2, bbits=14, device=0, n=5)
PARAMS = types.SimpleNamespace(n_init=2, K=3)
RASTER = (0.0, 1.0, 4, 0.0, 1.0, 4)

DIST_MSG = "distMat must be a C-contiguous float32 [n,2] CUDA tensor"
PTS_MSG = "points must be a C-contiguous float32 [n,2] CUDA tensor"
EDGES_MSG = "edges must be a contiguous int64 [m, 2] CUDA tensor"
EDGES_OR_PAIR_MSG = "edges must be a contiguous int64 [m, 2] CUDA tensor, or an (i, j) pair of int64 tensors"
STREAM_MSG = "edge arrays must be int64 CUDA tensors of one length"
STREAM_STRIDE_MSG = "edge arrays must be contiguous, or the two columns of a contiguous [m, 2] tensor"
INDEX_MSG = "index must be a contiguous int64 [m] CUDA tensor on the matrix's device"
NO_PAIR_MSG = "'tuple' object has no attribute 'is_cuda'"
SAMPLES_MSG = "row count is not n(n-1)/2 for any n (self/condensed matrix expected)"
SEG_MSG = "seg_off must be a one-dimensional array of n_strains + 1 offsets"
CODES_MSG = "codes_t must be a contiguous one-dimensional uint8 CUDA tensor"
SEQ_OFF_MSG = "seq_off must be a one-dimensional array of n + 1 offsets"
SLOTS_MSG = "n_slots must be 1 .. 32 and nx, ny 1 .. 4096"
WEIGHTS_TYPE_MSG = "weights_type must be one of ['accessory', 'core', 'euclidean']"
EMBED_VALUE_MSG = "%s: lists of n*k entries with n >= 2 and 1 <= k <= n - 1 expected (n = %d, %d entries)"
LEVELS_MSG = "levels must be a contiguous int32 [n_levels, 3] CUDA tensor on the matrix's device"
STRAIN_LISTS_MSG = ("members, and the stored lists, must be contiguous CUDA tensors on one device: int64 [m], "
                    "int64 and float32 [nnz]")
CODES = cu(torch.zeros(10, dtype=torch.uint8))

e = engine
CASES = [
    # ---- host-only arguments -------------------------------------------------------------------------------------
    (lambda: e.band_split_weighted(100, 0, [1.0, -1.0]), ValueError, "weights must be non-negative, finite and not all zero"),
    (lambda: e.band_split_weighted(100, 0, [0, 0]), ValueError, "weights must be non-negative, finite and not all zero"),
    (lambda: e.band_split_weighted(100, 0, [[1.0]]), ValueError, "weights must be non-negative, finite and not all zero"),
    (lambda: e.check_assign_sizes("who", 4, 4, 0), RuntimeError, "who: max_links must be 1 .. 64"),
    (lambda: e.check_assign_sizes("who", 4, 4, 65), RuntimeError, "who: max_links must be 1 .. 64"),
    (lambda: e.check_assign_sizes("who", 4, 2 ** 31), RuntimeError, "who: n_ref + n_qry must be < 2^31"),
    (lambda: e.check_assign_sizes("who", -1, 4), RuntimeError, "who: n_ref + n_qry must be < 2^31"),
    (lambda: e.strain_nnz([[0, 2]], 1), ValueError, SEG_MSG),
    (lambda: e.strain_nnz([0], 1), ValueError, SEG_MSG),
    (lambda: e.rows_to_pairs([3], 3), ValueError, "row index outside [0, 3)"),
    (lambda: e.rows_to_pairs([-1], 3, 2), ValueError, "row index outside [0, 6)"),
    (lambda: e._samples_of(4), ValueError, SAMPLES_MSG),
    (lambda: e.dist_bgmm_edges(DB), ValueError, "a prepared BGMM model is needed"),
    (lambda: e.bgmm_edges_host(DB), ValueError, "a prepared BGMM model is needed"),
    # ---- the host-array twins ------------------------------------------------------------------------------------
    (lambda: e.bgmm_fit(np.zeros((4, 3)), (1, 1), PARAMS), ValueError, "X must be [n, 2] (core, accessory)"),
    (lambda: e.bgmm_fit(np.zeros((4, 2)), (1, 1), PARAMS, init_labels=np.zeros(3)), ValueError,
     "init_labels must have one entry per training row"),
    (lambda: e.bgmm_fit(np.zeros((4, 2)), (1, 1), PARAMS, index=[0, 1], init_labels=np.zeros(4)), ValueError,
     "init_labels must have one entry per training row"),
    (lambda: e.bgmm_fit(np.zeros((4, 2)), (1, 1), PARAMS, init_centres=np.zeros((2, 2, 2))), ValueError,
     "init_centres must be [n_init, K, 2]"),
    (lambda: e.pick_references(np.zeros((3, 2)), -1), RuntimeError, "ppk_pick_refs: n_vertices must be < 2^31"),
    (lambda: e.pick_references(np.zeros((3, 2)), 2 ** 31), RuntimeError, "ppk_pick_refs: n_vertices must be < 2^31"),
    (lambda: e.pick_references(np.zeros((3, 2)), 4, existing=[1, 0]), ValueError, "existing must hold n flags"),
    (lambda: e.pick_references(np.zeros((3, 2)), 4, merged=[1, 0]), ValueError, "merged must hold n flags"),
    (lambda: e.density_kde(np.zeros((4, 3)), [0.0], [0.0], 0.1), ValueError, "dist must be [n, 2]"),
    (lambda: e.density_kde(np.zeros((4, 2)), [[0.0]], [0.0], 0.1), ValueError, "gx and gy must be one-dimensional"),
    (lambda: e.density_kde(np.zeros((4, 2)), [0.0], [[0.0]], 0.1), ValueError, "gx and gy must be one-dimensional"),
    (lambda: e.density_counts(np.zeros((4, 3)), RASTER), ValueError, "dist must be [n, 2]"),
    (lambda: e.density_counts(np.zeros((4, 2)), RASTER, labels=[0, 1]), ValueError, "one label per row"),
    (lambda: e.density_counts(np.zeros((4, 2)), RASTER, n_slots=33), ValueError, SLOTS_MSG),
    (lambda: e.density_counts(np.zeros((4, 2)), (0.0, 1.0, 4097, 0.0, 1.0, 4)), ValueError, SLOTS_MSG),
    (lambda: e.nj(np.zeros((3, 2))), ValueError, "the matrix must be square"),
    (lambda: e.embed([0, 1], [1], [0.1, 0.1], 2, 0), ValueError, EMBED_VALUE_MSG % ("embed", 2, 2)),
    (lambda: e.embed([0, 1, 0], [1, 0, 1], [0.1] * 3, 2, 0), ValueError, EMBED_VALUE_MSG % ("embed", 2, 3)),
    (lambda: e.refine_score(np.zeros((3, 3)), 2, 0.1, 0.1), ValueError, "distances must be a float32 [n, 2] array"),
    (lambda: e.extend_from_sketches(([0], [1], [0.1]), [DB, DB], [DB], [13, 17], None, 1), ValueError,
     "one query database per reference database"),
    (lambda: e.extend_from_sketches(([0], [1], [0.1]), [DB], [DB_OTHER], [13, 17], None, 1), ValueError,
     "ref and query databases are incompatible"),
    (lambda: e.extend_from_sketches(([0], [1], [0.1]), [DB], [DB], [13, 17, 21], None, 1), ValueError,
     "klist length 3 does not match the sketches' 2 k-mer lengths"),
    (lambda: e.extend_from_sketches(([0], [1], [0.1]), [DB], [DB], [13, 17], np.zeros((2, 3, 4)), 1), ValueError,
     "random table must be [nk, n_clu, n_clu]"),
    (lambda: e.extend_from_sketches(([0], [1], [0.1]), [DB], [DB], [13, 17], np.zeros((3, 3, 3)), 1), ValueError,
     "random table must be [nk, n_clu, n_clu]"),
    (lambda: e.knn_ref_query(DB, DB_OTHER, [13, 17], None, 1), ValueError, "ref and query databases are incompatible"),
    (lambda: e.dist_pairs(DB, DB_OTHER, [13, 17], None, E), ValueError, "ref and query databases are incompatible"),
    (lambda: e.dist_pairs(DB, None, [13, 17], None), ValueError, "dist_pairs needs a pair list"),
    (lambda: e.dist_pairs(DB, None, [13, 17], None, CPU_E), TypeError, EDGES_OR_PAIR_MSG),
    (lambda: e.dist_pairs(DB, None, [13, 17], None, (i64(3), i64(3))), TypeError, STREAM_MSG),
    (lambda: e.edge_weights_from_sketches(DB, None, [13, 17], None, E, weights_type="x"), ValueError, WEIGHTS_TYPE_MSG),
    (lambda: e.refine_sweep_scores_dev(D, [0.0], 2, 0, 0, 1, 1, score_idx=3), ValueError, "score_idx must be 0, 1 or 2"),
    (lambda: e.refine_sweep_scores_2d_dev(D, [0.1], 0.1, score_idx=-1), ValueError, "score_idx must be 0, 1 or 2"),
    (lambda: e.threshold_iterate_2d_dev(D, [0.2, 0.1], 0.1), RuntimeError,
     "x_max range to thresholdIterate2D must be sorted"),
    (lambda: e.prune_long_dev(f32(6, 2), 4, [2, 1]), RuntimeError,
     "kept indices must be strictly ascending and inside the matrix"),
    (lambda: e.prune_long_dev(f32(6, 2), 4, [1, 4]), RuntimeError,
     "kept indices must be strictly ascending and inside the matrix"),
    (lambda: e.prune_query_rows_dev(f32(6, 2), 3, [2]), RuntimeError, "kept query index outside the matrix"),
    (lambda: e.prune_query_rows_dev(f32(6, 2), 3, [-1]), RuntimeError, "kept query index outside the matrix"),
    # ---- the [n, 2] matrix, every wrapper that takes one -----------------------------------------------------------
    (lambda: e.bgmm_assign_dev(CPU_D, None), TypeError, DIST_MSG),
    (lambda: e.bgmm_assign_dev(cu(f32(4, 3)), None), TypeError, DIST_MSG),
    (lambda: e.bgmm_assign_dev(cu(f32(4)), None), TypeError, DIST_MSG),
    (lambda: e.bgmm_assign_dev(cu(torch.zeros((4, 2), dtype=torch.float64)), None), TypeError, DIST_MSG),
    (lambda: e.bgmm_assign_dev(cu(f32(2, 4).T), None), TypeError, DIST_MSG),
    (lambda: e.bgmm_assign_dev(D, None, labels=False, values=False), ValueError,
     "ask for labels, responsibilities or both"),
    (lambda: e.bgmm_edges_dev(CPU_D, _lib.Bgmm()), TypeError, DIST_MSG),
    (lambda: e.bgmm_stats_dev(CPU_D, None, (1, 1)), TypeError, DIST_MSG),
    (lambda: e.bgmm_kmeans_dev(CPU_D, np.zeros((2, 2)), (1, 1), i32(4)), TypeError, DIST_MSG),
    (lambda: e.bgmm_fit_dev(CPU_D, (1, 1), PARAMS), TypeError, DIST_MSG),
    (lambda: e.dbscan_assign_dev(CPU_D, None), TypeError, DIST_MSG),
    (lambda: e.dbscan_edges_dev(CPU_D, None), TypeError, DIST_MSG),
    (lambda: e.assign_threshold_dev(CPU_D, 2, 0.1, 0.1), TypeError, DIST_MSG),
    (lambda: e.edge_threshold_dev(CPU_D, 2, 0.1, 0.1), TypeError, DIST_MSG),
    (lambda: e.qc_edges_dev(CPU_D, 0.5, 0.5), TypeError, DIST_MSG),
    (lambda: e.nearest_reference_dev(CPU_D, 2, 2), TypeError, DIST_MSG),
    (lambda: e.cluster_pair_sums_dev(CPU_D, LEV), TypeError, DIST_MSG),
    (lambda: e.silhouette_dev(CPU_D, LEV), TypeError, DIST_MSG),
    (lambda: e.strain_knn_dev(CPU_D, MEM, SEG, 1), TypeError, DIST_MSG),
    (lambda: e.density_kde_dev(CPU_D, [0.0], [0.0], 0.1), TypeError, DIST_MSG),
    (lambda: e.density_counts_dev(CPU_D, RASTER), TypeError, DIST_MSG),
    (lambda: e.edge_weights_dev(CPU_D, E), TypeError, DIST_MSG),
    (lambda: e.refine_score_dev(CPU_D, 2, 0.1, 0.1), TypeError, DIST_MSG),
    (lambda: e.RefineLocal.create(CPU_D, 2, 0.1, 0.1, 0.2, 0.2), TypeError, DIST_MSG),
    # ---- BGMM fit passes -----------------------------------------------------------------------------------------
    (lambda: e.bgmm_stats_dev(D, None, (1, 1), index_t=i64(2)), TypeError, INDEX_MSG),
    (lambda: e.bgmm_stats_dev(D, None, (1, 1), index_t=cu(i32(2))), TypeError, INDEX_MSG),
    (lambda: e.bgmm_stats_dev(D, None, (1, 1), index_t=cu(i64(2, 1))), TypeError, INDEX_MSG),
    (lambda: e.bgmm_stats_dev(D, None, (1, 1), index_t=cu(i64(4)[::2])), TypeError, INDEX_MSG),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros((2, 2)), (1, 1), cu(i32(3)), index_t=i64(2)), TypeError, INDEX_MSG),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros((2, 2)), (1, 1), i32(3)), TypeError,
     "labels must be a contiguous int32 CUDA tensor with one entry per training row"),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros((2, 2)), (1, 1), cu(i32(4))), TypeError,
     "labels must be a contiguous int32 CUDA tensor with one entry per training row"),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros((2, 2)), (1, 1), cu(i32(3)), index_t=cu(i64(2))), TypeError,
     "labels must be a contiguous int32 CUDA tensor with one entry per training row"),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros((2, 2)), (1, 1), cu(i64(3))), TypeError,
     "labels must be a contiguous int32 CUDA tensor with one entry per training row"),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros((2, 3)), (1, 1), cu(i32(3))), ValueError, "centres must be [K, 2]"),
    (lambda: e.bgmm_kmeans_dev(D, np.zeros(2), (1, 1), cu(i32(3))), ValueError, "centres must be [K, 2]"),
    (lambda: e.bgmm_fit_dev(D, (1, 1), PARAMS, index_t=cu(i32(2))), TypeError, INDEX_MSG),
    (lambda: e.bgmm_fit_dev(D, (1, 1), PARAMS, init_labels_t=i32(3)), TypeError,
     "init_labels must be a contiguous int32 CUDA tensor with one entry per training row"),
    (lambda: e.bgmm_fit_dev(D, (1, 1), PARAMS, init_labels_t=cu(i32(4))), TypeError,
     "init_labels must be a contiguous int32 CUDA tensor with one entry per training row"),
    (lambda: e.bgmm_fit_dev(D, (1, 1), PARAMS, init_centres=np.zeros((2, 3, 3))), ValueError,
     "init_centres must be [n_init, K, 2]"),
    # ---- generateTuples, DBSCAN ----------------------------------------------------------------------------------
    (lambda: e.generate_tuples_dev(i32(4), 0), TypeError, "assignments must be a contiguous int32 CUDA tensor"),
    (lambda: e.generate_tuples_dev(cu(i64(4)), 0), TypeError, "assignments must be a contiguous int32 CUDA tensor"),
    (lambda: e.generate_tuples_dev(cu(i32(8)[::2]), 0), TypeError, "assignments must be a contiguous int32 CUDA tensor"),
    (lambda: e.dbscan_core_dev(CPU_D, 3), TypeError, PTS_MSG),
    (lambda: e.dbscan_core_dev(cu(f32(4, 3)), 3), TypeError, PTS_MSG),
    (lambda: e.dbscan_mst_dev(CPU_D, cu(torch.zeros(4, dtype=torch.float64))), TypeError, PTS_MSG),
    (lambda: e.dbscan_mst_dev(D4, torch.zeros(4, dtype=torch.float64)), TypeError,
     "core2 must be a contiguous float64 [n] CUDA tensor"),
    (lambda: e.dbscan_mst_dev(D4, cu(f32(4))), TypeError, "core2 must be a contiguous float64 [n] CUDA tensor"),
    (lambda: e.dbscan_mst_dev(D4, cu(torch.zeros(3, dtype=torch.float64))), TypeError,
     "core2 must be a contiguous float64 [n] CUDA tensor"),
    (lambda: e.dbscan_mst_dev(D4, cu(torch.zeros((4, 1), dtype=torch.float64))), TypeError,
     "core2 must be a contiguous float64 [n] CUDA tensor"),
    # ---- the edge stream -----------------------------------------------------------------------------------------
    (lambda: e.network_sweep_dev(i64(3), i64(3), None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.network_sweep_dev(I, cu(i64(4)), None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.network_sweep_dev(I, cu(i32(3)), None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.network_sweep_dev(I, J, cu(i64(2)), 4, 2), TypeError, STREAM_MSG),
    (lambda: e.network_sweep_dev(I, J, i64(3), 4, 2), TypeError, STREAM_MSG),
    (lambda: e.network_sweep_dev(E, J, None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.network_sweep_dev(E[:, 0], J, None, 4, 1), TypeError, STREAM_STRIDE_MSG),
    (lambda: e.network_sweep_dev(cu(i64(3, 3))[:, 0], cu(i64(3, 3))[:, 1], None, 4, 1), TypeError, STREAM_STRIDE_MSG),
    (lambda: e.network_sweep_dev(I, J, cu(i64(3, 2))[:, 0], 4, 2), TypeError, "the offset array must be contiguous"),
    (lambda: e.cluster_sweep_dev(i64(3), i64(3), None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.cluster_sweep_dev(E[:, 0], J, None, 4, 1), TypeError, STREAM_STRIDE_MSG),
    (lambda: e.network_summary_dev(i64(3), i64(3), None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.network_summary_dev(I, J, cu(i64(3, 2))[:, 0], 4, 2), TypeError, "the offset array must be contiguous"),
    (lambda: e.network_summary_sampled_dev(I, J, None, 4, 1, sources=0), ValueError,
     "network_summary_sampled_dev: sources must be >= 1"),
    (lambda: e.network_summary_sampled_dev(i64(3), i64(3), None, 4, 1), TypeError, STREAM_MSG),
    (lambda: e.network_summary_sampled_dev(E[:, 0], J, None, 4, 1), TypeError, STREAM_STRIDE_MSG),
    # ---- the [m, 2] form alone: a CPU tensor, a wrong dtype or rank, a transposed view, and a pair ---------------
    (lambda: e.network_stats_dev(CPU_E, 4), TypeError, EDGES_MSG),
    (lambda: e.network_stats_dev(cu(i32(3, 2)), 4), TypeError, EDGES_MSG),
    (lambda: e.network_stats_dev(cu(i64(3, 3)), 4), TypeError, EDGES_MSG),
    (lambda: e.network_stats_dev(cu(i64(6)), 4), TypeError, EDGES_MSG),
    (lambda: e.network_stats_dev(cu(i64(2, 3).T), 4), TypeError, EDGES_MSG),
    (lambda: e.network_stats_dev((I, J), 4), AttributeError, NO_PAIR_MSG),
    (lambda: e.cluster_numbers_dev(CPU_E, 4), TypeError, EDGES_MSG),
    (lambda: e.cluster_numbers_dev((I, J), 4), AttributeError, NO_PAIR_MSG),
    (lambda: e.network_summary_graph_dev(CPU_E, 4), TypeError, EDGES_MSG),
    (lambda: e.network_summary_graph_dev(cu(i32(3, 2)), 4), TypeError, EDGES_MSG),
    (lambda: e.network_summary_graph_dev((I, J), 4), AttributeError, NO_PAIR_MSG),
    (lambda: e.network_summary_sampled_graph_dev(CPU_E, 4), TypeError, EDGES_MSG),
    (lambda: e.network_summary_sampled_graph_dev((I, J), 4), AttributeError, NO_PAIR_MSG),
    (lambda: e.network_summary_sampled_graph_dev(E, 4, sources=0), ValueError,
     "network_summary_sampled_dev: sources must be >= 1"),
    # ---- [m, 2] or a pair ------------------------------------------------------------------------------------------
    (lambda: e.query_links_dev(CPU_E, LAB, 2), TypeError, EDGES_MSG),
    (lambda: e.query_links_dev(cu(i64(3, 3)), LAB, 2), TypeError, EDGES_MSG),
    (lambda: e.query_links_dev((i64(3), i64(3)), LAB, 2), TypeError, STREAM_MSG),
    (lambda: e.query_links_dev((E[:, 0], J), LAB, 2), TypeError, STREAM_STRIDE_MSG),
    (lambda: e.query_links_dev(E, i32(4), 2), TypeError,
     "ref_label must be a contiguous int32 CUDA tensor on the edges' device"),
    (lambda: e.query_links_dev((I, J), cu(i64(4)), 2), TypeError,
     "ref_label must be a contiguous int32 CUDA tensor on the edges' device"),
    (lambda: e.query_links_dev(E, cu(i32(4, 1)), 2), TypeError,
     "ref_label must be a contiguous int32 CUDA tensor on the edges' device"),
    (lambda: e.query_links_dev(E, LAB, 2, max_links=0), RuntimeError, "ppk_query_links: max_links must be 1 .. 64"),
    (lambda: e.query_links_dev(E, LAB, 2 ** 31 - 4), RuntimeError, "ppk_query_links: n_ref + n_qry must be < 2^31"),
    (lambda: e.cluster_extend_dev(CPU_E, LAB, 2), TypeError, EDGES_MSG),
    (lambda: e.cluster_extend_dev((i64(3), i64(3)), LAB, 2), TypeError, STREAM_MSG),
    (lambda: e.cluster_extend_dev(E, cu(i32(8)[::2]), 2), TypeError,
     "ref_label must be a contiguous int32 CUDA tensor on the edges' device"),
    (lambda: e.cluster_extend_dev(E, LAB, 2 ** 31), RuntimeError, "ppk_cluster_extend: n_ref + n_qry must be < 2^31"),
    (lambda: e.pick_references_dev(CPU_E, 4), TypeError, EDGES_MSG),
    (lambda: e.pick_references_dev(cu(i32(3, 2)), 4), TypeError, EDGES_MSG),
    (lambda: e.pick_references_dev((i64(3), i64(3)), 4), TypeError, STREAM_MSG),
    (lambda: e.pick_references_dev(E, -1), RuntimeError, "ppk_pick_refs: n_vertices must be < 2^31"),
    (lambda: e.pick_references_dev((I, J), 2 ** 31), RuntimeError, "ppk_pick_refs: n_vertices must be < 2^31"),
    (lambda: e.pick_references_dev(E, 4, existing=torch.zeros(4, dtype=torch.uint8)), TypeError,
     "existing must be a uint8 or bool CUDA tensor of n flags on the edges' device"),
    (lambda: e.pick_references_dev(E, 4, existing=cu(torch.zeros(3, dtype=torch.bool))), TypeError,
     "existing must be a uint8 or bool CUDA tensor of n flags on the edges' device"),
    (lambda: e.pick_references_dev(E, 4, merged=cu(i32(4))), TypeError,
     "merged must be a uint8 or bool CUDA tensor of n flags on the edges' device"),
    (lambda: e.pick_references_dev(E, 4, existing=cu(torch.zeros(4, dtype=torch.bool)),
                                   merged=cu(torch.zeros((4, 1), dtype=torch.uint8))), TypeError,
     "merged must be a uint8 or bool CUDA tensor of n flags on the edges' device"),
    (lambda: e.mst_dev(CPU_E, cu(f32(3)), 4), TypeError, EDGES_OR_PAIR_MSG),
    (lambda: e.mst_dev(cu(i64(3, 3)), cu(f32(3)), 4), TypeError, EDGES_OR_PAIR_MSG),
    (lambda: e.mst_dev((i64(3), i64(3)), cu(f32(3)), 4), TypeError, STREAM_MSG),
    (lambda: e.mst_dev((E[:, 0], J), cu(f32(3)), 4), TypeError, STREAM_STRIDE_MSG),
    (lambda: e.mst_dev(E, f32(3), 4), TypeError, "weights must be a contiguous float32 CUDA tensor, one per edge"),
    (lambda: e.mst_dev((I, J), cu(f32(4)), 4), TypeError, "weights must be a contiguous float32 CUDA tensor, one per edge"),
    (lambda: e.mst_dev(E, cu(torch.zeros(3, dtype=torch.float64)), 4), TypeError,
     "weights must be a contiguous float32 CUDA tensor, one per edge"),
    (lambda: e.mst_dev(E, cu(f32(6)[::2]), 4), TypeError, "weights must be a contiguous float32 CUDA tensor, one per edge"),
    (lambda: e.edge_weights_dev(D, E, weights_type="x"), ValueError, WEIGHTS_TYPE_MSG),
    (lambda: e.edge_weights_dev(D, CPU_E), TypeError, EDGES_OR_PAIR_MSG),
    (lambda: e.edge_weights_dev(D, (i64(3), i64(3))), TypeError, STREAM_MSG),
    # ---- assignment, clusters, scores ----------------------------------------------------------------------------
    (lambda: e.nearest_reference_dev(D4, 3, 2), ValueError, "the matrix must have n_qry * n_ref rows"),
    (lambda: e.cluster_pair_sums_dev(D4, LEV), ValueError, SAMPLES_MSG),
    (lambda: e.cluster_pair_sums_dev(D, i32(2, 3)), TypeError, LEVELS_MSG),
    (lambda: e.cluster_pair_sums_dev(D, cu(i32(2, 4))), TypeError, LEVELS_MSG),
    (lambda: e.cluster_pair_sums_dev(D, cu(i64(2, 3))), TypeError, LEVELS_MSG),
    (lambda: e.cluster_pair_sums_dev(D, cu(i32(3))), TypeError, LEVELS_MSG),
    (lambda: e.silhouette_dev(D4, LEV), ValueError, SAMPLES_MSG),
    (lambda: e.silhouette_dev(D, i32(2, 3)), TypeError, LEVELS_MSG),
    (lambda: e.silhouette_dev(D, cu(i32(3, 2).T)), TypeError, LEVELS_MSG),
    (lambda: e.contingency_sums_dev(i32(2, 3)), TypeError, "levels_a must be a contiguous int32 [n_levels, n] CUDA tensor"),
    (lambda: e.contingency_sums_dev(cu(i64(2, 3))), TypeError, "levels_a must be a contiguous int32 [n_levels, n] CUDA tensor"),
    (lambda: e.contingency_sums_dev(cu(i32(3))), TypeError, "levels_a must be a contiguous int32 [n_levels, n] CUDA tensor"),
    (lambda: e.contingency_sums_dev(LEV, i32(2, 3)), TypeError, "levels_b must be a contiguous int32 [n_levels, n] CUDA tensor"),
    (lambda: e.contingency_sums_dev(LEV, cu(i32(2, 4))), TypeError,
     "levels_b must have levels_a's 3 samples and live on its device"),
    # ---- sketches ------------------------------------------------------------------------------------------------
    (lambda: e.sketch_dev(torch.zeros(10, dtype=torch.uint8), [0, 10], [13], 2), TypeError, CODES_MSG),
    (lambda: e.sketch_dev(cu(i32(10)), [0, 10], [13], 2), TypeError, CODES_MSG),
    (lambda: e.sketch_dev(cu(torch.zeros((10, 1), dtype=torch.uint8)), [0, 10], [13], 2), TypeError, CODES_MSG),
    (lambda: e.sketch_dev(CODES, [[0, 10]], [13], 2), ValueError, SEQ_OFF_MSG),
    (lambda: e.sketch_dev(CODES, [], [13], 2), ValueError, SEQ_OFF_MSG),
    (lambda: e.sketch_dev(CODES, [0, 11], [13], 2), ValueError, "seq_off ends beyond codes_t"),
    (lambda: e.sketch_reads_dev(torch.zeros(10, dtype=torch.uint8), [0, 10], [13], 2, 2), TypeError, CODES_MSG),
    (lambda: e.sketch_reads_dev(cu(torch.zeros(20, dtype=torch.uint8)[::2]), [0, 10], [13], 2, 2), TypeError, CODES_MSG),
    (lambda: e.sketch_reads_dev(CODES, [[0, 10]], [13], 2, 2), ValueError, SEQ_OFF_MSG),
    (lambda: e.sketch_reads_dev(CODES, [0, 11], [13], 2, 2), ValueError, "seq_off ends beyond codes_t"),
    # ---- lineages ------------------------------------------------------------------------------------------------
    (lambda: e.strain_knn_dev(D4, MEM, SEG, 1), ValueError, SAMPLES_MSG),
    (lambda: e.strain_knn_dev(D, i64(4), SEG, 1), TypeError,
     "members must be a contiguous int64 [m] CUDA tensor on the matrix's device"),
    (lambda: e.strain_knn_dev(D, cu(i32(4)), SEG, 1), TypeError,
     "members must be a contiguous int64 [m] CUDA tensor on the matrix's device"),
    (lambda: e.strain_knn_dev(D, MEM, [0], 1), ValueError, SEG_MSG),
    (lambda: e.strain_knn_dev(D, MEM, [0, 2, 5], 1), ValueError, "seg_off must end at the number of members"),
    (lambda: e.strain_extend_dev(i64(4), SEG, None, [0, 0, 0], NNJ, NND, None, None, 4, 0, 1), TypeError,
     STRAIN_LISTS_MSG),
    (lambda: e.strain_extend_dev(MEM, SEG, None, [0, 0, 0], cu(i32(4)), NND, None, None, 4, 0, 1), TypeError,
     STRAIN_LISTS_MSG),
    (lambda: e.strain_extend_dev(MEM, SEG, None, [0, 0, 0], NNJ, cu(f32(4, 1)), None, None, 4, 0, 1), TypeError,
     STRAIN_LISTS_MSG),
    (lambda: e.strain_extend_dev(MEM, [0], None, [0, 0, 0], NNJ, NND, None, None, 4, 0, 1), ValueError, SEG_MSG),
    (lambda: e.strain_extend_dev(MEM, SEG, None, [0, 0], NNJ, NND, None, None, 4, 0, 1), ValueError,
     "seg_off and qry_off must have one entry per strain and one more"),
    (lambda: e.strain_extend_dev(MEM, [0, 2, 5], None, [0, 0, 0], NNJ, NND, None, None, 4, 0, 1), ValueError,
     "seg_off must end at the number of members"),
    (lambda: e.strain_extend_dev(MEM, SEG, cu(i64(3)), [0, 1, 2], NNJ, NND, cu(f32(8, 2)), None, 4, 2, 1), TypeError,
     "queries must be a contiguous int64 [mq] CUDA tensor on the members' device, qry_off ending at mq"),
    (lambda: e.strain_extend_dev(MEM, SEG, cu(i64(2)), [0, 1, 2], NNJ, NND, cu(f32(7, 2)), None, 4, 2, 1), TypeError,
     "qr must be a contiguous float32 [n_qry * n_ref, 2] CUDA tensor on the members' device"),
    (lambda: e.strain_extend_dev(MEM, SEG, cu(i64(2)), [0, 1, 2], NNJ, NND, cu(f32(8, 2)), cu(f32(2, 2)), 4, 2, 1),
     TypeError, "qq must be a contiguous float32 [n_qry(n_qry-1)/2, 2] CUDA tensor on the members' device"),
    (lambda: e.strain_extend_dev(MEM, SEG, None, [0, 0, 0], cu(i64(5)), cu(f32(5)), None, None, 4, 0, 1), ValueError,
     "the stored lists must hold the entries of strain_knn_dev at this depth"),
    (lambda: e.strain_extend_dev(MEM, SEG, None, [0, 0, 0], NNJ, cu(f32(5)), None, None, 4, 0, 1), ValueError,
     "the stored lists must hold the entries of strain_knn_dev at this depth"),
    (lambda: e.strain_ranks_dev(i64(4), NND, SEG, 1, [1]), TypeError,
     "the lists must be contiguous CUDA tensors of one length, int64 columns and float32 distances"),
    (lambda: e.strain_ranks_dev(NNJ, cu(f32(5)), SEG, 1, [1]), TypeError,
     "the lists must be contiguous CUDA tensors of one length, int64 columns and float32 distances"),
    (lambda: e.strain_ranks_dev(NNJ, f32(4), SEG, 1, [1]), TypeError,
     "the lists must be contiguous CUDA tensors of one length, int64 columns and float32 distances"),
    (lambda: e.strain_ranks_dev(NNJ, NND, [0], 1, [1]), ValueError, SEG_MSG),
    (lambda: e.strain_ranks_dev(NNJ, NND, SEG, 1, []), ValueError, "ranks must be a non-empty one-dimensional array"),
    (lambda: e.strain_ranks_dev(NNJ, NND, SEG, 1, [[1]]), ValueError, "ranks must be a non-empty one-dimensional array"),
    (lambda: e.strain_ranks_dev(cu(i64(5)), cu(f32(5)), SEG, 1, [1]), ValueError,
     "the lists must hold the 4 entries of strain_knn_dev at this depth"),
    # ---- density -------------------------------------------------------------------------------------------------
    (lambda: e.density_kde_dev(D, [[0.0]], [0.0], 0.1), ValueError, "gx and gy must be one-dimensional"),
    (lambda: e.density_kde_dev(D, [0.0], [[0.0]], 0.1), ValueError, "gx and gy must be one-dimensional"),
    (lambda: e.density_kde_dev(D, [0.0], [0.0], 0.1, idx_t=i64(2)), TypeError,
     "idx must be a contiguous int64 CUDA vector on the matrix's device"),
    (lambda: e.density_kde_dev(D, [0.0], [0.0], 0.1, idx_t=cu(i32(2))), TypeError,
     "idx must be a contiguous int64 CUDA vector on the matrix's device"),
    (lambda: e.density_kde_dev(D, [0.0], [0.0], 0.1, idx_t=cu(i64(4)[::2])), TypeError,
     "idx must be a contiguous int64 CUDA vector on the matrix's device"),
    (lambda: e.density_counts_dev(D, RASTER, labels_t=i32(3)), TypeError,
     "labels must be a contiguous int32 [n] CUDA tensor on the matrix's device"),
    (lambda: e.density_counts_dev(D, RASTER, labels_t=cu(i32(4))), TypeError,
     "labels must be a contiguous int32 [n] CUDA tensor on the matrix's device"),
    (lambda: e.density_counts_dev(D, RASTER, labels_t=cu(i64(3))), TypeError,
     "labels must be a contiguous int32 [n] CUDA tensor on the matrix's device"),
    (lambda: e.density_counts_dev(D, RASTER, n_slots=33), ValueError, SLOTS_MSG),
    (lambda: e.density_counts_dev(D, RASTER, n_slots=0), ValueError, SLOTS_MSG),
    (lambda: e.density_counts_dev(D, (0.0, 1.0, 4, 0.0, 1.0, 0)), ValueError, SLOTS_MSG),
    # ---- trees and embeddings ------------------------------------------------------------------------------------
    (lambda: e.nj_dev(f32(3, 3)), TypeError,
     "the matrix must be a contiguous float32 CUDA tensor: [n, n] square or [n_pairs(, k)] long"),
    (lambda: e.nj_dev(cu(torch.zeros((3, 3), dtype=torch.float64))), TypeError,
     "the matrix must be a contiguous float32 CUDA tensor: [n, n] square or [n_pairs(, k)] long"),
    (lambda: e.nj_dev(cu(f32(3, 3, 1))), TypeError,
     "the matrix must be a contiguous float32 CUDA tensor: [n, n] square or [n_pairs(, k)] long"),
    (lambda: e.nj_dev(cu(f32(3, 4).T)), TypeError,
     "the matrix must be a contiguous float32 CUDA tensor: [n, n] square or [n_pairs(, k)] long"),
    (lambda: e.nj_dev(D4), ValueError, SAMPLES_MSG),
    (lambda: e.nj_dev(D, col=2), ValueError, "col must index a column of the long form"),
    (lambda: e.nj_dev(cu(f32(3)), col=1), ValueError, "col must index a column of the long form"),
    (lambda: e.nj_dev(D, n=4), ValueError, "n = 4 does not match the matrix (3 samples)"),
    (lambda: e.nj_dev(cu(f32(4, 4)), n=3), ValueError, "n = 3 does not match the matrix (4 samples)"),
    (lambda: e.embed_weights_dev(i64(4), cu(i64(4)), cu(f32(4)), 4), TypeError,
     "embed_weights_dev: i and j must be contiguous int64 CUDA vectors"),
    (lambda: e.embed_weights_dev(cu(i64(4)), cu(i32(4)), cu(f32(4)), 4), TypeError,
     "embed_weights_dev: i and j must be contiguous int64 CUDA vectors"),
    (lambda: e.embed_weights_dev(cu(i64(4)), cu(i64(5)), cu(f32(4)), 4), ValueError,
     EMBED_VALUE_MSG % ("embed_weights_dev", 4, 4)),
    (lambda: e.embed_weights_dev(cu(i64(5)), cu(i64(5)), cu(f32(5)), 4), ValueError,
     EMBED_VALUE_MSG % ("embed_weights_dev", 4, 5)),
    (lambda: e.embed_weights_dev(cu(i64(4)), cu(i64(4)), f32(4), 4), TypeError,
     "embed_weights_dev: dist must be a contiguous float32 CUDA vector as long as i"),
    (lambda: e.embed_weights_dev(cu(i64(4)), cu(i64(4)), cu(f32(5)), 4), TypeError,
     "embed_weights_dev: dist must be a contiguous float32 CUDA vector as long as i"),
    (lambda: e.embed_dev(cu(i64(4)), i64(4), cu(torch.zeros(4, dtype=torch.float64)), 4, 0), TypeError,
     "embed_dev: i and j must be contiguous int64 CUDA vectors"),
    (lambda: e.embed_dev(cu(i64(4)), cu(i64(4)), cu(torch.zeros(4, dtype=torch.float64)), 1, 0), ValueError,
     EMBED_VALUE_MSG % ("embed_dev", 1, 4)),
    (lambda: e.embed_dev(cu(i64(4)), cu(i64(4)), cu(f32(4)), 4, 0), TypeError,
     "embed_dev: P must be a contiguous float64 CUDA vector as long as i"),
    (lambda: e.embed_dev(cu(i64(4)), cu(i64(4)), torch.zeros(4, dtype=torch.float64), 4, 0), TypeError,
     "embed_dev: P must be a contiguous float64 CUDA vector as long as i"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_one_faulty_argument_raises_what_it_always_did(case):
    call, kind, message = CASES[case]
    with pytest.raises(kind) as got:
        call()
    assert type(got.value) is kind and str(got.value) == message


def test_closed_handles_raise_before_the_device():
    bracket = object.__new__(engine.RefineLocal)
    bracket._h, bracket.device = None, torch.device("cpu")
    with pytest.raises(RuntimeError) as got:
        bracket.eval(0.1, 0.1)
    assert str(got.value) == "the bracket handle is closed"
    job = object.__new__(engine.PeerStoreQuery)
    job.window = None
    with pytest.raises(RuntimeError) as got:
        job.run()
    assert str(got.value) == "PeerStoreQuery.run before open()"


# ---- _lib.call against a stub of the library -------------------------------------------------------------------------
class _Stub:
    """A function object as ctypes makes them: `argtypes`, called with the converted arguments."""

    def __init__(self, argtypes, rc=0):
        self.argtypes, self.rc, self.seen = argtypes, rc, None

    def __call__(self, *args):
        self.seen = args
        return self.rc


@pytest.fixture
def stub(monkeypatch):
    fns = types.SimpleNamespace(ppk_last_error=lambda: b"the library's words")
    monkeypatch.setattr(_lib, "lib", lambda: fns)

    def make(rc=0):
        fns.ppk_stub = _Stub([C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_longlong), C.c_void_p, C.c_double,
                              C.POINTER(C.c_size_t)], rc)
        return fns.ppk_stub
    return make


def test_call_converts_host_arrays_by_the_declared_types_and_nothing_else(stub):
    fn = stub()
    x = np.arange(4, dtype=np.float32)
    n_out = C.c_size_t(0)
    ref = C.byref(n_out)
    ptr = C.c_void_p(1234)
    assert _lib.call("ppk_stub", x, 4, None, ptr, 0.5, ref) == _lib.OK
    got = fn.seen
    assert isinstance(got[0], C.POINTER(C.c_float)) and C.addressof(got[0].contents) == x.ctypes.data
    assert got[1] == 4 and type(got[1]) is int
    assert got[2] is None
    assert got[3] is ptr and got[4] == 0.5 and got[5] is ref
    idx = np.arange(3, dtype=np.int64)
    _lib.call("ppk_stub", x, 4, idx, None, 1.0, None)
    assert isinstance(fn.seen[2], C.POINTER(C.c_longlong)) and C.addressof(fn.seen[2].contents) == idx.ctypes.data
    assert fn.seen[3] is None and fn.seen[5] is None


def test_call_returns_accepted_codes_maps_err_arg_where_asked_and_checks_the_rest(stub):
    x = np.zeros(1, dtype=np.float32)
    args = (x, 1, None, None, 0.0, None)
    stub(_lib.ERR_CAPACITY)
    assert _lib.call("ppk_stub", *args, accept=(_lib.ERR_CAPACITY,)) == _lib.ERR_CAPACITY
    with pytest.raises(RuntimeError) as got:
        _lib.call("ppk_stub", *args)
    assert str(got.value) == "ppk_stub failed (3): the library's words"
    stub(_lib.ERR_ARG)
    with pytest.raises(ValueError) as got:
        _lib.call("ppk_stub", *args, arg_error=ValueError)
    assert type(got.value) is ValueError and str(got.value) == "the library's words"
    with pytest.raises(RuntimeError) as got:
        _lib.call("ppk_stub", *args)
    assert type(got.value) is RuntimeError and str(got.value) == "ppk_stub failed (1): the library's words"
    with pytest.raises(RuntimeError) as got:
        _lib.call("ppk_stub", *args, accept=(_lib.ERR_CAPACITY,))
    assert str(got.value) == "ppk_stub failed (1): the library's words"
    stub(_lib.ERR_HIP)
    with pytest.raises(RuntimeError) as got:
        _lib.call("ppk_stub", *args, arg_error=ValueError)
    assert str(got.value) == "ppk_stub failed (2): the library's words"
