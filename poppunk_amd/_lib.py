"""ctypes binding of libppk_hip.so (the C ABI declared in include/ppk.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded the
import of this module's `lib()` raises, and every product entry point fails.
"""
import ctypes as C
import os

from numpy import ndarray as _ndarray

_HERE = os.path.dirname(os.path.abspath(__file__))
# PPK_LIBRARY: another build of the same library (the measurement tools load csrc/libppk_hip_exp.so, tools/_exp.py)
SO_PATH = os.environ.get("PPK_LIBRARY") or os.path.join(_HERE, "csrc", "libppk_hip.so")

OK, ERR_ARG, ERR_HIP, ERR_CAPACITY, ERR_STATE, ERR_INTERRUPTED = 0, 1, 2, 3, 4, 5
REFINE_NOT_NESTED = 6      # ppk_refine_local_create_dev: the two lines do not form a bracket
FLAG_RANDOM_CORRECT, FLAG_JACCARD, FLAG_COUNTS = 1, 2, 4
SKETCH_STRAND_PRESERVED = 1      # flag of ppk_sketch / ppk_sketch_dev / ppk_sketch_reads / ppk_sketch_reads_dev
SKETCH_EXACT = 2                 # flag of ppk_sketch_reads / ppk_sketch_reads_dev: the exact route
BT_WHOLE_GRAPH = 1               # flag of ppk_network_summary_sampled / _dev: values normalised by the whole graph

# every symbol include/ppk.h declares: name -> (restype, argtypes)
_u64p, _f32p, _i32p, _u16p = (C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                              C.POINTER(C.c_uint16))
_llp, _ullp, _szp, _intp = (C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong),
                            C.POINTER(C.c_size_t), C.POINTER(C.c_int))
_vp, _sz = C.c_void_p, C.c_size_t

BGMM_MAX_K = 16


class Bgmm(C.Structure):
    """struct ppk_bgmm (include/ppk.h): a fitted BGMM model as the kernels read it (ppk_bgmm_prepare fills it)."""
    _fields_ = [("K", C.c_int), ("within_label", C.c_int), ("scale_is_f64", C.c_int), ("n_jitter", C.c_int),
                ("scale_f32", C.c_float * 2), ("scale_f64", C.c_double * 2),
                ("mean", (C.c_double * 2) * BGMM_MAX_K), ("chol", (C.c_double * 3) * BGMM_MAX_K),
                ("inv_diag", (C.c_double * 2) * BGMM_MAX_K), ("log_const", C.c_double * BGMM_MAX_K),
                ("lin", (C.c_double * 5) * BGMM_MAX_K),
                ("jitter", C.c_int * BGMM_MAX_K)]


BGMM_FIT_STATS, BGMM_FIT_MAX_ITER, BGMM_FIT_MAX_INIT, BGMM_KMEANS_MAX_ITER = 7, 1024, 32, 50


class BgmmFitParams(C.Structure):
    """struct ppk_bgmm_fit_params (include/ppk.h, "BGMM fit"); ppk_bgmm_fit_params_default fills it."""
    _fields_ = [("K", C.c_int), ("max_iter", C.c_int), ("n_init", C.c_int), ("reserved", C.c_int),
                ("weight_concentration_prior", C.c_double), ("mean_precision_prior", C.c_double),
                ("mean_prior", C.c_double * 2), ("degrees_of_freedom_prior", C.c_double), ("reg_covar", C.c_double),
                ("tol", C.c_double)]


class BgmmState(C.Structure):
    """struct ppk_bgmm_state: the variational state after an M-step (ppk_bgmm_mstep fills it)."""
    _fields_ = [("K", C.c_int), ("reserved", C.c_int),
                ("weight_conc_a", C.c_double * BGMM_MAX_K), ("weight_conc_b", C.c_double * BGMM_MAX_K),
                ("mean_precision", C.c_double * BGMM_MAX_K), ("means", (C.c_double * 2) * BGMM_MAX_K),
                ("dof", C.c_double * BGMM_MAX_K), ("covariances", (C.c_double * 4) * BGMM_MAX_K),
                ("chol", (C.c_double * 3) * BGMM_MAX_K), ("weights", C.c_double * BGMM_MAX_K),
                ("lin", (C.c_double * 5) * BGMM_MAX_K), ("log_const", C.c_double * BGMM_MAX_K)]


class BgmmFitResult(C.Structure):
    """struct ppk_bgmm_fit_result."""
    _fields_ = [("state", BgmmState), ("n_iter", C.c_int), ("converged", C.c_int), ("best_init", C.c_int),
                ("n_init_run", C.c_int), ("n_train", C.c_ulonglong), ("lower_bound", C.c_double),
                ("cov_prior", C.c_double * 4), ("train_mean", C.c_double * 2),
                ("init_lower_bound", C.c_double * BGMM_FIT_MAX_INIT), ("init_n_iter", C.c_int * BGMM_FIT_MAX_INIT),
                ("kmeans_iter", C.c_int * BGMM_FIT_MAX_INIT), ("lower_bounds", C.c_double * BGMM_FIT_MAX_ITER)]


_bgmmp, _f64p = C.POINTER(Bgmm), C.POINTER(C.c_double)
_fitpp, _statep, _fitrp = C.POINTER(BgmmFitParams), C.POINTER(BgmmState), C.POINTER(BgmmFitResult)

SIGNATURES = {
    "ppk_bgmm_prepare": (C.c_int, [C.c_int, _f64p, _f64p, _f64p, _f64p, C.c_int, C.c_int, _bgmmp]),
    "ppk_bgmm_assign_dev": (C.c_int, [_vp, _sz, _bgmmp, _vp, _vp, _vp]),
    "ppk_bgmm_edges_dev": (C.c_int, [_vp, _sz, _sz, _bgmmp, C.c_longlong, _vp, _sz, _vp, _vp]),
    "ppk_dist_bgmm_edges_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _sz, _sz, _bgmmp, _vp, _sz, _vp, _vp,
                                          _vp]),
    "ppk_query_bgmm_edges_dbs": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), C.c_int, _i32p, _f32p, _sz, C.c_int,
                                           _bgmmp, _llp, _sz, _szp, _ullp]),
    "ppk_bgmm_assign": (C.c_int, [_f32p, _sz, _bgmmp, C.c_int, _i32p, _f32p]),
    "ppk_bgmm_fit_params_default": (C.c_int, [C.c_int, _fitpp]),
    "ppk_bgmm_fit_struct_sizes": (C.c_int, [_szp]),
    "ppk_bgmm_digamma": (C.c_double, [C.c_double]),
    "ppk_bgmm_mstep": (C.c_int, [_fitpp, _f64p, _f64p, _f64p, _statep, _f64p]),
    "ppk_bgmm_stats_dev": (C.c_int, [_vp, _sz, _vp, _sz, _f32p, _statep, _vp, _vp]),
    "ppk_bgmm_kmeans_dev": (C.c_int, [_vp, _sz, _vp, _sz, _f32p, C.c_int, _f64p, _vp, _vp, _vp, _vp]),
    "ppk_bgmm_fit_dev": (C.c_int, [_vp, _sz, _vp, _sz, _f32p, _vp, _f64p, _fitpp, _fitrp, _vp]),
    "ppk_bgmm_fit": (C.c_int, [_f32p, _sz, _llp, _sz, _f32p, _i32p, _f64p, _fitpp, C.c_int, _fitrp]),
    "ppk_network_sweep_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, C.c_longlong, _vp, _vp, _vp]),
    "ppk_network_sweep": (C.c_int, [_llp, _llp, _llp, _sz, _sz, _sz, C.c_int, C.c_longlong, _llp, _i32p]),
    "ppk_network_summary_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, C.c_longlong, _vp, _vp, _vp, _vp, _vp]),
    "ppk_network_summary": (C.c_int, [_llp, _llp, _llp, _sz, _sz, _sz, C.c_int, C.c_longlong, _llp, _f64p, _llp, _f64p]),
    "ppk_network_summary_sampled_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, C.c_longlong, _vp, _vp, _vp, _vp,
                                                  _sz, C.c_ulonglong, C.c_int, _vp]),
    "ppk_network_summary_sampled": (C.c_int, [_llp, _llp, _llp, _sz, _sz, _sz, C.c_int, C.c_longlong, _llp, _f64p, _llp,
                                              _f64p, _sz, C.c_ulonglong, C.c_int]),
    "ppk_cluster_sweep_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp, _vp, _vp]),
    "ppk_cluster_sweep": (C.c_int, [_llp, _llp, _llp, _sz, _sz, _sz, C.c_int, _i32p, _i32p]),
    "ppk_cluster_pair_sums_dev": (C.c_int, [_vp, _sz, C.c_int, _vp, _sz, C.c_int, _vp, _vp, _vp]),
    "ppk_cluster_pair_sums": (C.c_int, [_f32p, _sz, C.c_int, _i32p, _sz, C.c_int, C.c_int, _llp, _llp]),
    "ppk_silhouette_dev": (C.c_int, [_vp, _sz, C.c_int, _vp, _sz, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ppk_silhouette": (C.c_int, [_f32p, _sz, C.c_int, _i32p, _sz, C.c_int, C.c_int, _f64p, _f64p, _f64p, _i32p,
                                 _i32p]),
    "ppk_contingency_sums_dev": (C.c_int, [_vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ppk_contingency_sums": (C.c_int, [_i32p, _sz, _i32p, _sz, _sz, C.c_int, _llp, _llp, _i32p, _i32p, _llp, _llp]),
    "ppk_strain_knn_dev": (C.c_int, [_vp, _sz, C.c_int, _vp, _llp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "ppk_strain_ranks_dev": (C.c_int, [_vp, _vp, _llp, _sz, _sz, _i32p, _sz, C.c_int, C.c_int, C.c_float, _vp, _vp, _vp,
                                       _vp, _vp, _sz, _szp, _vp]),
    "ppk_strain_knn": (C.c_int, [_f32p, _sz, C.c_int, _llp, _llp, _sz, _sz, C.c_int, _llp, _llp, _f32p]),
    "ppk_strain_ranks": (C.c_int, [_llp, _f32p, _llp, _sz, _sz, _i32p, _sz, C.c_int, C.c_int, C.c_float, C.c_int, _i32p,
                                   _llp, _llp, _llp, _f32p, _sz, _szp]),
    "ppk_strain_extend_dev": (C.c_int, [_vp, _llp, _vp, _llp, _sz, _vp, _vp, _vp, _vp, _sz, _sz, C.c_int, C.c_float,
                                        _sz, _vp, _vp, _vp, _vp]),
    "ppk_strain_extend": (C.c_int, [_llp, _llp, _llp, _llp, _sz, _llp, _f32p, _f32p, _f32p, _sz, _sz, C.c_int,
                                    C.c_float, _sz, C.c_int, _llp, _llp, _f32p]),
    "ppk_sketch_dev": (C.c_int, [_vp, _vp, _sz, _i32p, _sz, _sz, _sz, C.c_int, _vp, _vp, _vp, _vp]),
    "ppk_sketch": (C.c_int, [C.POINTER(C.c_uint8), _llp, _sz, _i32p, _sz, _sz, _sz, C.c_int, C.c_int, _u64p, _llp, _i32p]),
    "ppk_sketch_reads_dev": (C.c_int, [_vp, _vp, _sz, _i32p, _sz, _sz, _sz, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "ppk_sketch_reads": (C.c_int, [C.POINTER(C.c_uint8), _llp, _sz, _i32p, _sz, _sz, _sz, C.c_int, C.c_int, C.c_int, _u64p,
                                   _llp, _llp, _i32p]),
    "ppk_density_kde_dev": (C.c_int, [_vp, _sz, _vp, _sz, _f32p, _f64p, _sz, _f64p, _sz, C.c_double, C.c_int, _vp, _f32p,
                                      _vp]),
    "ppk_density_kde": (C.c_int, [_f32p, _sz, _llp, _sz, _f32p, _f64p, _sz, _f64p, _sz, C.c_double, C.c_int, C.c_int,
                                  _llp, _f32p]),
    "ppk_density_counts_dev": (C.c_int, [_vp, _sz, _vp, C.c_int, C.c_int, C.c_double, C.c_double, _sz, C.c_double,
                                         C.c_double, _sz, _vp, _vp, _vp]),
    "ppk_density_counts": (C.c_int, [_f32p, _sz, _i32p, C.c_int, C.c_int, C.c_double, C.c_double, _sz, C.c_double,
                                     C.c_double, _sz, C.c_int, C.POINTER(C.c_uint32), _llp]),
    "ppk_query_links_dev": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, C.c_int, _vp, _vp, _vp, _vp]),
    "ppk_query_links": (C.c_int, [_llp, _llp, _sz, _i32p, _sz, _sz, C.c_int, C.c_int, _i32p, _i32p, _i32p]),
    "ppk_cluster_extend_dev": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _vp]),
    "ppk_cluster_extend": (C.c_int, [_llp, _llp, _sz, _i32p, _sz, _sz, C.c_int, _i32p, _i32p]),
    "ppk_pick_refs_dev": (C.c_int, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "ppk_pick_refs": (C.c_int, [_llp, _llp, _sz, _sz, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int, C.c_int,
                                C.POINTER(C.c_uint8), _llp, _llp]),
    "ppk_mst_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "ppk_mst": (C.c_int, [_llp, _llp, _f32p, _sz, _sz, C.c_int, _llp, _ullp, _i32p]),
    "ppk_edge_weights_dev": (C.c_int, [_vp, _sz, _vp, _vp, _sz, _sz, _sz, C.c_longlong, C.c_int, _vp, _vp]),
    "ppk_row_norms_dev": (C.c_int, [_vp, _sz, _vp, _vp]),
    "ppk_nj_dev": (C.c_int, [_vp, C.c_int, _sz, _sz, _sz, _vp, _vp, _vp]),
    "ppk_nj": (C.c_int, [_f32p, _sz, C.c_int, _llp, _f64p]),
    "ppk_embed_weights_dev": (C.c_int, [_vp, _vp, _vp, _sz, _sz, C.c_double, _vp, _vp, _vp]),
    "ppk_embed_dev": (C.c_int, [_vp, _vp, _vp, _sz, _sz, C.c_ulonglong, C.c_longlong, C.c_int, C.c_double,
                                C.c_longlong, _vp, _vp]),
    "ppk_embed": (C.c_int, [_llp, _llp, _f32p, _sz, _sz, C.c_double, C.c_ulonglong, C.c_longlong, C.c_int,
                            C.c_double, C.c_longlong, C.c_int, _f64p, _f64p]),
    "ppk_dbscan_core_dev": (C.c_int, [_vp, _sz, C.c_int, _vp, _vp]),
    "ppk_dbscan_mst_dev": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "ppk_dbscan_fit": (C.c_int, [_f32p, _sz, C.c_int, C.c_int, _f64p, _i32p, _i32p, _f64p]),
    "ppk_dbscan_create": (C.c_int, [_f32p, _f64p, _sz, C.c_int, _i32p, _f64p, _i32p, _f64p, _i32p, _sz, _f64p,
                                    C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "ppk_dbscan_destroy": (None, [_vp]),
    "ppk_dbscan_assign_dev": (C.c_int, [_vp, _sz, _vp, _vp, _vp]),
    "ppk_dbscan_edges_dev": (C.c_int, [_vp, _sz, _sz, _vp, C.c_longlong, _vp, _sz, _vp, _vp]),
    "ppk_dbscan_assign": (C.c_int, [_f32p, _sz, _vp, _i32p]),
    "ppk_dbscan_stats": (C.c_int, [_vp, _ullp]),
    "ppk_refine_score_dev": (C.c_int, [_vp, _sz, C.c_int, C.c_float, C.c_float, _vp, _vp]),
    "ppk_refine_score": (C.c_int, [_f32p, _sz, C.c_int, C.c_float, C.c_float, C.c_int, _llp]),
    "ppk_refine_local_create_dev": (C.c_int, [_vp, _sz, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _vp,
                                              C.POINTER(_vp)]),
    "ppk_refine_local_destroy": (None, [_vp]),
    "ppk_refine_local_stats": (C.c_int, [_vp, _ullp]),
    "ppk_refine_local_eval_dev": (C.c_int, [_vp, C.c_float, C.c_float, _vp, _vp]),
    "ppk_last_error": (C.c_char_p, []),
    "ppk_version": (C.c_char_p, []),
    "ppk_release_scratch": (C.c_int, []),
    "ppk_device_count": (C.c_int, [_intp]),
    "ppk_db_create": (C.c_int, [C.c_int, _vp, _sz, _sz, _sz, _sz, _vp, C.c_int, _vp,
                                C.POINTER(_vp)]),
    "ppk_db_destroy": (None, [_vp]),
    "ppk_db_size": (_sz, [_vp]),
    "ppk_db_rank_planes": (C.c_int, [_vp]),
    "ppk_db_rank_read": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_rank_block_planes": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_fold_planes": (C.c_int, [_vp]),
    "ppk_db_fold_block_planes": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_fold_read": (C.c_int, [_vp, C.c_int, _vp, _sz]),
    "ppk_db_fold2_planes": (C.c_int, [_vp]),
    "ppk_db_fold2_block_planes": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_fold2_stream_planes": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_fold2_position_order": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_fold2_read": (C.c_int, [_vp, C.c_int, _vp, _sz]),
    "ppk_db_fold2_events": (_sz, [_vp, C.POINTER(C.c_size_t)]),
    "ppk_db_fold2_events_read": (C.c_int, [_vp, _vp, _sz, _vp, _sz]),
    "ppk_db_rank_counts": (_sz, [_vp, _vp, _sz]),
    "ppk_db_foldh_holders": (C.c_uint, [_vp]),
    "ppk_db_foldh_chunk_planes": (C.c_int, [_vp]),
    "ppk_db_foldh_stream_planes": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_foldh_position_order": (C.c_int, [_vp, _vp, _sz]),
    "ppk_db_foldh_read": (C.c_int, [_vp, C.c_int, _vp, _sz]),
    "ppk_db_foldh_entries": (_sz, [_vp, C.POINTER(C.c_size_t)]),
    "ppk_db_foldh_entries_read": (C.c_int, [_vp, _vp, _sz, _vp, _sz]),
    "ppk_rows_in_band": (_sz, [_sz, _sz, _sz, _sz]),
    "ppk_band_split": (C.c_int, [_sz, _sz, C.c_int, _szp]),
    "ppk_dist_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _sz, _sz, _vp, _vp, _vp]),
    "ppk_dist_pairs_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _vp, _vp, _sz, _sz, C.c_longlong, _vp, _vp,
                                     _vp]),
    "ppk_dist_pairs": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _llp, _llp, _sz, C.c_longlong, _vp, _ullp]),
    "ppk_dist_edges_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _sz, _sz, C.c_int,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _vp,
                                     _sz, _vp, _vp, _vp]),
    "ppk_dist_edges_rows_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _sz, _sz, C.c_int,
                                          C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _vp, _vp,
                                          _sz, _vp, _vp, _vp]),
    "ppk_dist_bgmm_edges_rows_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _sz, _sz, _bgmmp, _vp, _vp, _sz,
                                               _vp, _vp, _vp]),
    "ppk_sweep_boundaries_1d": (C.c_int, [C.POINTER(C.c_double), _sz, C.c_int, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ppk_sweep_levels_dev": (C.c_int, [_vp, _sz, C.POINTER(C.c_float), C.POINTER(C.c_float), _sz, C.c_int, _vp, _vp]),
    "ppk_assign_threshold_dev": (C.c_int, [_vp, _sz, C.c_int, C.c_float, C.c_float, _vp, _vp]),
    "ppk_edge_threshold_dev": (C.c_int, [_vp, _sz, _sz, C.c_int, C.c_float, C.c_float, C.c_int,
                                         _vp, _sz, _vp, _vp]),
    "ppk_generate_tuples_dev": (C.c_int, [_vp, _sz, C.c_int, C.c_int, _sz, C.c_longlong, _vp,
                                          _sz, _vp, _vp]),
    "ppk_query": (C.c_int, [_u64p, _sz, _u64p, _sz, _i32p, _sz, _sz, _sz, _f32p, _u16p, _u16p,
                            _sz, C.c_int, _intp, C.c_int, _vp, _ullp]),
    "ppk_assign_threshold": (C.c_int, [_f32p, _sz, C.c_int, C.c_float, C.c_float, C.c_int,
                                       _f32p]),
    "ppk_edge_threshold": (C.c_int, [_f32p, _sz, _sz, C.c_int, C.c_float, C.c_float, C.c_int,
                                     C.c_int, _llp, _sz, _szp]),
    "ppk_generate_tuples": (C.c_int, [_i32p, _sz, C.c_int, C.c_int, _sz, C.c_longlong, C.c_int,
                                      _llp, _sz, _szp]),
    "ppk_threshold_iterate_1d_dev": (C.c_int, [_vp, _sz, C.POINTER(C.c_double), _sz, C.c_int,
                                               C.c_float, C.c_float, C.c_float, C.c_float, _vp,
                                               _vp, _vp, _sz, _vp, _vp]),
    "ppk_threshold_iterate_2d_dev": (C.c_int, [_vp, _sz, _f32p, _sz, C.c_float, _vp, _vp, _vp,
                                               _sz, _vp, _vp]),
    "ppk_threshold_iterate_1d": (C.c_int, [_f32p, _sz, C.POINTER(C.c_double), _sz, C.c_int,
                                           C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                           _llp, _llp, _llp, _sz, _szp]),
    "ppk_threshold_iterate_2d": (C.c_int, [_f32p, _sz, _f32p, _sz, C.c_float, C.c_int, _llp,
                                           _llp, _llp, _sz, _szp]),
    "ppk_long_to_square_dev": (C.c_int, [_vp, _sz, _sz, _sz, _vp, _vp]),
    "ppk_long_to_square_multi_dev": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    "ppk_square_to_long_dev": (C.c_int, [_vp, _sz, _vp, _vp]),
    "ppk_knn_dev": (C.c_int, [_vp, _sz, C.c_int, _vp, _vp, _vp, _vp]),
    "ppk_knn_rect_dev": (C.c_int, [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _vp, _vp, _vp]),
    "ppk_knn_sketches_dev": (C.c_int, [_vp, _i32p, _f32p, _sz, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp,
                                       _ullp, _vp]),
    "ppk_knn_candidates_dev": (C.c_int, [_vp, _i32p, _f32p, _sz, C.c_int, C.c_int, C.c_int, _sz, _sz, _vp, _vp,
                                         _sz, _ullp, _vp]),
    "ppk_knn_select_dev": (C.c_int, [_vp, _vp, _sz, _sz, C.c_int, _vp, _vp, _vp, _vp]),
    "ppk_prune_long_dev": (C.c_int, [_vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "ppk_prune_query_rows_dev": (C.c_int, [_vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    "ppk_prune_long": (C.c_int, [_f32p, _sz, _sz, _llp, _sz, C.c_int, _f32p]),
    "ppk_long_to_square": (C.c_int, [_f32p, _sz, C.c_int, _f32p]),
    "ppk_long_to_square_multi": (C.c_int, [_f32p, _f32p, _f32p, _sz, _sz, C.c_int, _f32p]),
    "ppk_long_to_square2": (C.c_int, [_f32p, _f32p, _f32p, _sz, _sz, C.c_int, _f32p, _f32p]),
    "ppk_square_to_long": (C.c_int, [_f32p, _sz, C.c_int, _f32p]),
    "ppk_knn": (C.c_int, [_f32p, _sz, C.c_int, C.c_int, _llp, _llp, _f32p]),
    "ppk_qc_edges_dev": (C.c_int, [_vp, _sz, _sz, C.c_int, C.c_float, C.c_float, _vp, _sz, _vp, _vp]),
    "ppk_window_alloc": (C.c_int, [C.c_int, _sz, C.POINTER(C.c_void_p)]),
    "ppk_window_free": (C.c_int, [C.c_int, _vp]),
    "ppk_window_export": (C.c_int, [C.c_int, _vp, C.c_char_p]),
    "ppk_window_open": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    "ppk_window_close": (C.c_int, [C.c_int, _vp]),
    "ppk_prof_enable": (C.c_int, [C.c_int]),
    "ppk_prof_read": (C.c_int, [C.POINTER(C.c_double), _llp, C.c_int]),
    "ppk_choose_route": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ppk_choose_coding": (C.c_int, [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_size_t), _vp, _vp, _vp, C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_int)]),
    "ppk_choose_holder": (C.c_int, [_vp, _sz, _sz, _sz, _sz, C.c_int, _sz, _sz, C.c_longlong, C.c_longlong,
                                    C.POINTER(C.c_uint), _vp, _vp, C.POINTER(C.c_size_t)]),
    "ppk_sweep_plan": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ppk_prof_stages_enable": (C.c_int, [C.c_int]),
    "ppk_prof_stages_read": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int]),
    "ppk_last_kernel_name": (C.c_char_p, []),
    "ppk_set_option": (C.c_int, [C.c_char_p, C.c_longlong]),
    "ppk_get_option": (C.c_int, [C.c_char_p, _llp]),
    "ppk_set_interrupt_check": (C.c_int, [_vp]),
    "ppk_query_db": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, _vp, _ullp]),
    "ppk_query_dbs": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), C.c_int, _i32p, _f32p, _sz, C.c_int, _vp, _ullp]),
    "ppk_query_last_stats": (C.c_int, [C.POINTER(C.c_double), C.c_int]),
    "ppk_parked_fetch": (C.c_int, [_llp, _llp, _llp, _sz, _szp]),
    "ppk_generate_all_tuples_dev": (C.c_int, [_sz, _sz, C.c_int, C.c_longlong, _vp, _sz, _szp, _vp]),
    "ppk_generate_all_tuples": (C.c_int, [_sz, _sz, C.c_int, C.c_longlong, C.c_int, _llp, _sz, _szp]),
    "ppk_lower_rank": (C.c_int, [_llp, _llp, _f32p, _sz, _sz, _sz, C.c_int, C.c_int, C.c_float, C.c_int, _llp, _llp,
                                 _f32p, _sz, _szp]),
    "ppk_extend": (C.c_int, [_llp, _llp, _f32p, _sz, _f32p, _f32p, _sz, _sz, _sz, C.c_int, _llp, _llp, _f32p, _sz,
                             _szp]),
    "ppk_query_knn_dbs": (C.c_int, [C.POINTER(_vp), C.c_int, _i32p, _f32p, _sz, C.c_int, C.c_int, C.c_int, _llp, _llp,
                                    _f32p]),
    "ppk_query_knn": (C.c_int, [_u64p, _sz, _i32p, _sz, _sz, _sz, _f32p, _u16p, _sz, C.c_int, C.c_int, C.c_int, _intp,
                                C.c_int, _llp, _llp, _f32p]),
    "ppk_knn_sketches_band_dev": (C.c_int, [_vp, _i32p, _f32p, _sz, C.c_int, C.c_int, C.c_int, _sz, _sz, _vp, _vp, _vp, _ullp,
                                            _vp]),
    "ppk_knn_sketches_rq_dev": (C.c_int, [_vp, _vp, _i32p, _f32p, _sz, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _ullp, _vp]),
    "ppk_extend_sketches": (C.c_int, [_llp, _llp, _f32p, _sz, _vp, _vp, _i32p, _f32p, _sz, C.c_int, C.c_int, C.c_int, _llp,
                                      _llp, _f32p, _sz, _szp]),
    "ppk_extend_sketches_dbs": (C.c_int, [_llp, _llp, _f32p, _sz, C.POINTER(_vp), C.POINTER(_vp), C.c_int, _i32p, _f32p, _sz,
                                          C.c_int, C.c_int, C.c_int, _llp, _llp, _f32p, _sz, _szp]),
    "ppk_qc_edges": (C.c_int, [_f32p, _sz, _sz, C.c_int, C.c_float, C.c_float, C.c_int, _llp, _sz, _szp, _szp]),
    "ppk_query_edges_dbs": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), C.c_int, _i32p, _f32p, _sz, C.c_int,
                                      C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _llp, _sz,
                                      _szp, _ullp]),
    "ppk_query_edges": (C.c_int, [_u64p, _sz, _u64p, _sz, _i32p, _sz, _sz, _sz, _f32p, _u16p, _u16p, _sz,
                                  C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _intp,
                                  C.c_int, _llp, _sz, _szp, _ullp]),
    "ppk_h5_set_library": (C.c_int, [C.c_char_p]),
    "ppk_h5_open": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_vp)]),
    "ppk_h5_close": (None, [_vp]),
    "ppk_h5_backend": (C.c_int, [_vp]),
    "ppk_h5_declined": (C.c_char_p, [_vp]),
    "ppk_h5_has_random": (C.c_int, [_vp]),
    "ppk_h5_count": (_sz, [_vp]),
    "ppk_h5_names": (C.c_int, [_vp, _vp, _sz, _szp]),
    "ppk_h5_params": (C.c_int, [_vp, C.c_char_p, _szp, _szp, _llp, _sz, _szp]),
    "ppk_h5_codon_phased": (C.c_int, [_vp]),
    "ppk_h5_all_params": (C.c_int, [_vp, _sz, _llp, _llp, _llp, _sz, _szp]),
    "ppk_h5_read": (C.c_int, [_vp, C.c_char_p, _sz, _i32p, _sz, _sz, _vp, _vp, _vp, _vp, C.c_int]),
}

_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own
    libamdhip64 (SONAME libamdhip64.so.7, the name libppk_hip.so NEEDs).  If
    libppk_hip.so were loaded first it would pull /opt/rocm's copy, and a later
    `import torch` would load the wheel's copy next to it: two runtimes fighting over
    the device ("No HIP GPUs are available").  So the wheel's copy is loaded first,
    by path, and both libppk_hip.so and torch then resolve to that one instance.
    Without torch installed, /opt/rocm's runtime is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libppk_hip.so; raises RuntimeError (never falls back) when it is unavailable."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "poppunk_amd: HIP extension %s not built (run __graft_entry__.build() / "
                "make -C poppunk_amd/csrc); there is no CPU fallback" % SO_PATH)
        _preload_hip_runtime()
        try:
            handle = C.CDLL(SO_PATH)
        except OSError as e:
            raise RuntimeError("poppunk_amd: cannot load %s: %s" % (SO_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def source_hash():
    """The hash of the sources libppk_hip.so was built from (`ppk_version()` ends in "src:<hash>")."""
    v = lib().ppk_version().decode()
    return v.rsplit("src:", 1)[1] if "src:" in v else None


def sources_hash_now():
    """The same hash computed from the sources as they are on disk now (csrc/Makefile HASHED): differs from
    `source_hash()` when the library has not been rebuilt since an edit.  None when a source is missing."""
    import hashlib
    import re
    here = os.path.join(_HERE, "csrc")
    try:
        with open(os.path.join(here, "Makefile")) as f:
            mk = f.read()
        srcs, hdrs = (re.search(r"^%s\s*:=\s*(.*)$" % v, mk, re.M).group(1).split() for v in ("SRCS", "HDRS"))
    except (OSError, AttributeError):
        return None
    names = srcs + ["ppk_h5.cpp"] + hdrs       # the order HASHED concatenates them in
    h = hashlib.sha256()
    try:
        for n in names:
            with open(os.path.join(here, n), "rb") as f:
                h.update(f.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


def set_option(name, value):
    """ppk_set_option: measurement knobs and the [EXT] switches (include/ppk.h)."""
    check(lib().ppk_set_option(name.encode(), int(value)), "ppk_set_option(%s)" % name)


def get_option(name):
    v = C.c_longlong(0)
    check(lib().ppk_get_option(name.encode(), C.byref(v)), "ppk_get_option(%s)" % name)
    return int(v.value)


class interruptible:
    """`with interruptible(): rc = lib.ppk_query(...)` -- Ctrl-C during a long host call.

    ctypes releases the GIL for the call and Python runs signal handlers only between bytecodes of
    the main thread, so a SIGINT would otherwise wait for the call to return.  The library polls a
    check between sub-bands (include/ppk.h: ppk_set_interrupt_check); the check is a ctypes callback
    -- executing it gives Python's pending handlers their chance to run -- that reports a flag which
    a temporary SIGINT handler sets.  On exit the previous handler is restored and, if the flag is
    set, KeyboardInterrupt is raised (the reference's loops raise through PyErr_CheckSignals,
    src/extend.cpp:263,:284-286).  Outside the main thread it does nothing."""
    _CB = C.CFUNCTYPE(C.c_int)

    def __enter__(self):
        import signal
        import threading
        self.flag = False
        self.installed = False
        if threading.current_thread() is not threading.main_thread():
            return self
        try:
            self.prev = signal.signal(signal.SIGINT, self._on_sigint)
        except ValueError:
            return self
        self.cb = self._CB(lambda: 1 if self.flag else 0)
        lib().ppk_set_interrupt_check(C.cast(self.cb, C.c_void_p))
        self.installed = True
        return self

    def _on_sigint(self, signum, frame):
        self.flag = True

    def __exit__(self, *exc):
        if self.installed:
            import signal
            lib().ppk_set_interrupt_check(None)
            signal.signal(signal.SIGINT, self.prev)
            if self.flag:
                raise KeyboardInterrupt
        return False


def last_error():
    return lib().ppk_last_error().decode("utf-8", "replace")


def check(rc, what="ppk call"):
    """C status -> RuntimeError, as pybind11 turns std::runtime_error into RuntimeError
    (src/python_bindings.cpp:54-56)."""
    if rc != OK:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, last_error()))


def call(name, *args, arg_error=None, accept=(), what=None):
    """Call the status-returning function `name` and deal with its status.  A numpy array (a plain ndarray, as
    np.ascontiguousarray and np.empty make them: the caller made it contiguous and of the right dtype) goes in as the
    pointer type SIGNATURES declares for its position; everything else --
    None, ints, floats, ctypes objects, byref -- is passed as it is.  A status in `accept` is returned (the
    ERR_CAPACITY retries); with `arg_error`, ERR_ARG raises arg_error(last_error()); every other failure is `check`'s
    RuntimeError, under `what` where the error has always been reported under another name than the symbol's."""
    fn = getattr(lib(), name)
    if _ndarray in map(type, args):         # (most device calls carry no host array: one C-level scan finds that out)
        types = fn.argtypes
        args = [a.ctypes.data_as(types[i]) if type(a) is _ndarray else a for i, a in enumerate(args)]
    rc = fn(*args)
    if rc in accept:
        return rc
    if arg_error is not None and rc == ERR_ARG:
        raise arg_error(last_error())
    check(rc, what or name)
    return rc
