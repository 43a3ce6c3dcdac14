"""ctypes binding of include/dialog_ransac.h (libdialog_amd.so, built in-tree for gfx950).

No fallback: if the library is missing or no gfx950 device is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdialog_amd.so")  # (A/B tooling rebinds it: tools/with_lib.py)

DLG_OK = 0
DLG_ERR_INVALID = 1
DLG_ERR_INTERNAL = 6
DLG_ERR_COMM = 4
DLG_ERR_CAPACITY = 5
DLG_SACMODEL_PLANE = 0
DLG_SACMODEL_NORMAL_PLANE = 11
DLG_SACMODEL_PERPENDICULAR_PLANE = 9
DLG_SACMODEL_PARALLEL_PLANE = 15
DLG_REFIT_PCL = 0
DLG_REFIT_FAST = 1
ABI_VERSION = 5  # include/dialog_ransac.h DLG_ABI_VERSION: the structs below match that header

SYMBOLS = [
    "dlg_abi_version", "dlg_status_string", "dlg_sac_params_default", "dlg_ctx_create",
    "dlg_get_unique_id", "dlg_ctx_create_dist", "dlg_ctx_create_loopback_group", "dlg_ctx_destroy",
    "dlg_last_error", "dlg_ctx_info", "dlg_cloud_upload", "dlg_cloud_destroy", "dlg_cloud_reset",
    "dlg_cloud_active", "dlg_sac_segment", "dlg_sac_segment_host", "dlg_extract_planes",
    "dlg_set_profiling", "dlg_synchronize", "dlg_allreduce_max_f64", "dlg_barrier",
    "dlg_score_benchmark", "dlg_estimate_normals", "dlg_regulate_normals",
    "dlg_cloud_set_normals", "dlg_orient_normals_nn", "dlg_preprocess", "dlg_refit_planes",
    "dlg_post_process_planes", "dlg_cluster_filter", "dlg_sac_control_create",
    "dlg_sac_control_destroy", "dlg_sac_control_next", "dlg_sac_control_consume",
    "dlg_sac_control_result", "dlg_cloud_build_spatial", "dlg_ctx_set_option",
    "dlg_ctx_get_option", "dlg_prune_stats", "dlg_estimate_normals_ex", "dlg_cloud_drop_spatial",
    "dlg_abi_struct_size", "dlg_float_sums", "dlg_cloud_estimate_normals", "dlg_plane_border",
    "dlg_cloud_regulate_normals", "dlg_shard_range", "dlg_cloud_signature",
    "dlg_ctx_set_axis", "dlg_ctx_get_axis", "dlg_score_samples", "dlg_axis_verdicts",
    "dlg_voxel_grid", "dlg_voxel_grid_cloud",
    "dlg_statistical_outlier_removal", "dlg_statistical_outlier_removal_cloud",
    "dlg_moving_least_squares", "dlg_moving_least_squares_cloud",
    "dlg_icp_params_default", "dlg_icp_align", "dlg_icp_correspondences", "dlg_cull_stats",
    "dlg_fpfh_estimate", "dlg_cloud_fpfh",
    "dlg_sac_ia_params_default", "dlg_fpfh_knn", "dlg_sac_ia_score", "dlg_sac_ia_align",
    "dlg_debug_live_bytes", "dlg_debug_pip_masks",
    "dlg_gs_params_default", "dlg_gs_space", "dlg_gs_vote", "dlg_gs_segment",
    "dlg_cloud_gs_segment", "dlg_knn_stats",
]

# context options (include/dialog_ransac.h): equivalent execution paths, identical results
DLG_OPT_PRUNE = 1
DLG_OPT_LEAN_ROUNDS = 2
DLG_OPT_SPEC_PICK = 3
DLG_OPT_PRUNE_NP = 4
DLG_OPT_SCORE_KERNEL = 5
DLG_OPT_PRUNE_STATS = 6
DLG_OPT_SELECT_TILE = 7
DLG_OPT_PCL_REFIT_DEVICE = 8
DLG_OPT_PRUNE_TILE_SCORER = 9
DLG_OPT_NORMALS_FUSED = 10
DLG_OPT_REGULATE_WAVE = 11
DLG_OPT_FS_POISON = 12
DLG_OPT_HYP_SHARD = 13
DLG_OPT_FS_ONE_WALK = 14
DLG_OPT_FS_SEGMENTS = 15
DLG_OPT_FAULT_INJECT = 16
DLG_OPT_SYNC_CHECK = 17
DLG_OPT_COMM_TIMEOUT_MS = 18
DLG_OPT_SEL1_TICKET = 19
DLG_OPT_BOUNDS_STREAM = 20
DLG_OPT_SPATIAL_CURVE = 21
DLG_OPT_FS_JOIN = 22
DLG_OPT_UNREFINED_LIST = 23
DLG_OPT_VOXEL_LONG_RUN = 24
DLG_OPT_SOR_LITERAL = 25
DLG_OPT_ICP_REVERSED = 26
DLG_OPT_ICP_MAX_BLOCKS = 27
DLG_OPT_CULL = 28
DLG_OPT_CULL_FUSE = 29
DLG_ICP_NOT_CONVERGED = 0
DLG_ICP_ITERATIONS = 1
DLG_ICP_TRANSFORM = 2
DLG_ICP_ABS_MSE = 3
DLG_ICP_REL_MSE = 4
DLG_ICP_NO_CORRESPONDENCES = 5
DLG_TILE_EXACT = 0
DLG_TILE_BF16 = 1
DLG_TILE_MFMA = 2
DLG_SCORE_EXACT = 0
DLG_SCORE_BF16 = 1
DLG_SCORE_PRUNED = 2
DLG_SCORE_BOUND = 3
DLG_SCORE_CULLED = 4


class Points(C.Structure):
    _fields_ = [("xyz", C.POINTER(C.c_float)), ("n", C.c_int64), ("stride_bytes", C.c_int64)]


class Planes(C.Structure):
    _fields_ = [("n_planes", C.c_int32), ("coeffs", C.POINTER(C.c_float)),
                ("points", C.POINTER(C.c_float)), ("points_stride_bytes", C.c_int64),
                ("point_offsets", C.POINTER(C.c_int64)), ("borders", C.POINTER(C.c_float)),
                ("borders_stride_bytes", C.c_int64), ("border_offsets", C.POINTER(C.c_int64))]


class PostProcessParams(C.Structure):
    _fields_ = [("t_dist_point_plane", C.c_float), ("radius_local", C.c_float),
                ("t_cluster_num", C.c_int32), ("plane_start_index", C.c_int32),
                ("rand_seed", C.c_uint32)]


class VoxelParams(C.Structure):
    _fields_ = [("leaf", C.c_float * 3), ("min_points_per_voxel", C.c_int32)]


class VoxelStats(C.Structure):
    _fields_ = [("n_finite", C.c_int64), ("n_voxels", C.c_int64), ("div", C.c_int32 * 3),
                ("min_b", C.c_int32 * 3), ("device_ms", C.c_double)]


class SorParams(C.Structure):
    _fields_ = [("mean_k", C.c_int32), ("negative", C.c_int32), ("stddev_mul", C.c_double)]


class SorStats(C.Structure):
    _fields_ = [("n_finite", C.c_int64), ("n_valid", C.c_int64), ("sum", C.c_double),
                ("sq_sum", C.c_double), ("mean", C.c_double), ("stddev", C.c_double),
                ("threshold", C.c_double), ("literal_queries", C.c_int64),
                ("exact_sums", C.c_int32), ("device_ms", C.c_double)]


class MlsParams(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("polynomial_fit", C.c_int32),
                ("polynomial_order", C.c_int32), ("compute_normals", C.c_int32),
                ("sqr_gauss_param", C.c_double)]


class MlsStats(C.Structure):
    _fields_ = [("n_finite", C.c_int64), ("n_out", C.c_int64), ("n_too_few", C.c_int64),
                ("n_plane_only", C.c_int64), ("n_fit_nonfinite", C.c_int64),
                ("max_neighbours", C.c_int64), ("n_lds_overflow", C.c_int64),
                ("device_ms", C.c_double)]


class IcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("compute_fitness", C.c_int32),
                ("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("fitness_max_range", C.c_double)]


class IcpStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("state", C.c_int32),
                ("levels", C.c_int32), ("n_corr", C.c_int64), ("n_src_finite", C.c_int64),
                ("n_tgt_finite", C.c_int64), ("host_syncs", C.c_int64), ("mse", C.c_double),
                ("fitness", C.c_double), ("build_ms", C.c_double), ("device_ms", C.c_double)]


class IcpIteration(C.Structure):
    _fields_ = [("n_corr", C.c_int64), ("mse", C.c_double), ("e", C.c_int32), ("e2", C.c_int32),
                ("T", C.c_float * 16)]


class FpfhParams(C.Structure):
    _fields_ = [("search_radius", C.c_float)]


class FpfhStats(C.Structure):
    _fields_ = [("n_finite", C.c_int64), ("n_nan_rows", C.c_int64), ("n_zero_rows", C.c_int64),
                ("max_neighbours", C.c_int64), ("n_lds_overflow", C.c_int64),
                ("n_pairs", C.c_int64), ("n_pairs_failed", C.c_int64),
                ("n_sum_literal", C.c_int64), ("device_ms", C.c_double), ("build_ms", C.c_double),
                ("spfh_ms", C.c_double), ("weight_ms", C.c_double)]


class SacIaParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("nr_samples", C.c_int32),
                ("k_correspondences", C.c_int32), ("rng", C.c_int32), ("seed", C.c_uint32),
                ("compute_fitness", C.c_int32), ("batch", C.c_int32), ("max_blocks", C.c_int32),
                ("min_sample_distance", C.c_float), ("max_correspondence_distance", C.c_double),
                ("fitness_max_range", C.c_double)]


class SacIaHypothesis(C.Structure):
    _fields_ = [("sample", C.c_int32 * 8), ("match", C.c_int32 * 8), ("rank", C.c_int32 * 8),
                ("valid", C.c_int32), ("relaxations", C.c_int32), ("draws", C.c_int64),
                ("T", C.c_float * 16), ("err_hi", C.c_uint64), ("err_lo", C.c_uint64),
                ("n_far", C.c_int64), ("n_used", C.c_int64)]


class SacIaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("best_iteration", C.c_int32),
                ("n_valid", C.c_int32), ("n_invalid", C.c_int32), ("batches", C.c_int32),
                ("levels", C.c_int32), ("reserved", C.c_int32), ("draws", C.c_int64),
                ("relaxations", C.c_int64), ("n_queries", C.c_int64), ("host_syncs", C.c_int64),
                ("error", C.c_double), ("fitness", C.c_double), ("build_ms", C.c_double),
                ("knn_ms", C.c_double), ("score_ms", C.c_double), ("device_ms", C.c_double)]


class GsParams(C.Structure):
    _fields_ = [("num_res", C.c_float), ("std_dev_gaussian", C.c_float),
                ("search_radius_create_gradient", C.c_float), ("t_vote_num", C.c_int32),
                ("radius_base", C.c_float), ("delta_radius", C.c_float),
                ("s_threshold", C.c_float), ("dev_threshold", C.c_float),
                ("search_radius_for_plane_seg", C.c_float), ("t_num_of_single_plane", C.c_int32)]


class GsStats(C.Structure):
    _fields_ = [("n_cells", C.c_int64), ("n_occupied", C.c_int64), ("n_voters", C.c_int64),
                ("n_fallback_votes", C.c_int64), ("n_filter_pairs", C.c_int64),
                ("n_sinks", C.c_int64), ("n_planes", C.c_int64), ("n_plane_points", C.c_int64),
                ("space_ms", C.c_double), ("vote_ms", C.c_double), ("filter_ms", C.c_double),
                ("segment_ms", C.c_double), ("host_ms", C.c_double), ("device_ms", C.c_double)]


class GsResult(C.Structure):
    _fields_ = [("plane_offsets", C.POINTER(C.c_int64)), ("planes_cap", C.c_int64),
                ("plane_ids", C.POINTER(C.c_int32)), ("ids_cap", C.c_int64),
                ("sink_cells", C.POINTER(C.c_int32)), ("sink_votes", C.POINTER(C.c_int64)),
                ("sinks_cap", C.c_int64), ("cell_of_point", C.POINTER(C.c_int32)),
                ("raw_vote", C.POINTER(C.c_int32)), ("filtered_vote", C.POINTER(C.c_int32)),
                ("sink_init", C.POINTER(C.c_int32)), ("sink", C.POINTER(C.c_int32)),
                ("cells_cap", C.c_int64), ("n_planes", C.c_int64), ("n_ids", C.c_int64),
                ("n_sinks", C.c_int64), ("n_cells", C.c_int64)]


class KnnRecord(C.Structure):
    _fields_ = [("valid", C.c_int32), ("k", C.c_int32), ("n", C.c_int64),
                ("levels_planned", C.c_int32), ("reserved", C.c_int32),
                ("queries", C.c_int64 * 12), ("built", C.c_int32 * 12)]


class SacParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("max_iterations", C.c_int), ("probability", C.c_double),
                ("optimize", C.c_int), ("seed", C.c_uint32), ("model", C.c_int),
                ("normal_distance_weight", C.c_double), ("refit_mode", C.c_int),
                ("hypotheses_per_launch", C.c_int), ("gather_inliers", C.c_int)]


class SacStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("skipped", C.c_int), ("has_model", C.c_int),
                ("launches", C.c_int), ("draws", C.c_int64), ("best_sample", C.c_int32 * 3),
                ("coeff_unrefined", C.c_float * 4), ("n_unrefined", C.c_int64),
                ("n_active", C.c_int64), ("tests", C.c_int64), ("tests_scored", C.c_int64),
                ("score_ms", C.c_double)]


class ExtractStats(C.Structure):
    _fields_ = [("rounds", C.c_int), ("tests", C.c_int64), ("tests_scored", C.c_int64),
                ("score_launches", C.c_int), ("score_ms", C.c_double), ("select_ms", C.c_double),
                ("wall_ms", C.c_double), ("lean_rounds", C.c_int), ("spec_misses", C.c_int),
                ("pcl_host_checks", C.c_int), ("refit_walk_ms", C.c_double),
                ("refit_repair_ms", C.c_double), ("refit_repairs", C.c_int),
                ("refit_rebase_ms", C.c_double)]


_lib = None


def load():
    """Load libdialog_amd.so (building it first if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if LIB_PATH != os.path.join(HERE, "libdialog_amd.so"):
            raise RuntimeError(f"{LIB_PATH}: no such library")
        from . import build as _b
        _b.build()
    L = C.CDLL(LIB_PATH)
    if L.dlg_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: ABI version {L.dlg_abi_version()}, binding expects {ABI_VERSION}")
    vp = C.c_void_p
    pp = C.POINTER(C.c_void_p)
    i32p = C.POINTER(C.c_int32)
    i64p = C.POINTER(C.c_int64)
    fp = C.POINTER(C.c_float)
    L.dlg_abi_version.restype = C.c_int
    L.dlg_abi_struct_size.restype = C.c_int64
    L.dlg_abi_struct_size.argtypes = [C.c_int]
    L.dlg_status_string.restype = C.c_char_p
    L.dlg_status_string.argtypes = [C.c_int]
    L.dlg_sac_params_default.argtypes = [C.POINTER(SacParams)]
    L.dlg_sac_params_default.restype = None
    L.dlg_ctx_create.argtypes = [pp, C.c_int]
    L.dlg_get_unique_id.argtypes = [vp]
    L.dlg_ctx_create_dist.argtypes = [pp, C.c_int, C.c_int, C.c_int, vp]
    L.dlg_ctx_create_loopback_group.argtypes = [pp, C.c_int, C.c_int]
    L.dlg_ctx_destroy.argtypes = [vp]
    L.dlg_last_error.argtypes = [vp]
    L.dlg_last_error.restype = C.c_char_p
    L.dlg_ctx_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dlg_cloud_upload.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64, C.c_int32, pp]
    L.dlg_cloud_destroy.argtypes = [vp]
    L.dlg_cloud_reset.argtypes = [vp]
    L.dlg_cloud_build_spatial.argtypes = [vp, vp]
    L.dlg_cloud_drop_spatial.argtypes = [vp]
    L.dlg_cloud_active.argtypes = [vp, i64p]
    L.dlg_cloud_signature.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.dlg_sac_segment.argtypes = [vp, vp, C.POINTER(SacParams), fp, i32p, C.c_int64, i64p,
                                  C.POINTER(SacStats)]
    L.dlg_sac_segment_host.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                       C.POINTER(SacParams), fp, i32p, C.c_int64, i64p,
                                       C.POINTER(SacStats)]
    L.dlg_extract_planes.argtypes = [vp, vp, C.POINTER(SacParams), C.c_int, C.c_int64, fp, i64p,
                                     i32p, C.c_int64, C.POINTER(C.c_int), C.POINTER(ExtractStats)]
    L.dlg_set_profiling.argtypes = [vp, C.c_int]
    L.dlg_synchronize.argtypes = [vp]
    L.dlg_allreduce_max_f64.argtypes = [vp, C.POINTER(C.c_double)]
    L.dlg_barrier.argtypes = [vp]
    L.dlg_score_benchmark.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double,
                                      C.POINTER(C.c_double), i32p]
    L.dlg_debug_live_bytes.restype = C.c_int64
    L.dlg_debug_live_bytes.argtypes = [C.c_int]
    L.dlg_debug_pip_masks.argtypes = [vp, C.POINTER(Points), C.POINTER(Planes), C.c_float,
                                      C.c_uint32, i64p, i32p, C.POINTER(C.c_uint32), C.c_int64,
                                      i64p]
    L.dlg_float_sums.argtypes = [vp, fp, C.c_int64, fp, C.c_int, fp, fp, C.POINTER(C.c_int),
                                 C.POINTER(C.c_double), i64p]
    L.dlg_ctx_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.dlg_ctx_get_option.argtypes = [vp, C.c_int, i64p]
    L.dlg_prune_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.dlg_cull_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.dlg_knn_stats.argtypes = [vp, C.POINTER(KnnRecord)]
    L.dlg_preprocess.argtypes = [vp, C.POINTER(Points), C.c_int, C.c_float, fp, C.c_int64, i32p,
                                 C.c_int64, i64p, fp]
    L.dlg_orient_normals_nn.argtypes = [vp, C.POINTER(Points), fp, C.c_int64, C.POINTER(Points),
                                        fp, C.c_int64]
    L.dlg_cloud_set_normals.argtypes = [vp, vp, fp, C.c_int64, C.c_int64]
    L.dlg_cloud_estimate_normals.argtypes = [vp, vp, C.c_float, C.c_int, fp, C.c_int, fp,
                                             C.c_int64]
    L.dlg_plane_border.argtypes = [C.POINTER(Points), fp, C.c_float, fp, C.c_int64, C.c_int64,
                                   i64p]
    L.dlg_estimate_normals.argtypes = [vp, C.POINTER(Points), C.c_float, C.c_int, fp, fp, C.c_int64]
    L.dlg_estimate_normals_ex.argtypes = [vp, C.POINTER(Points), C.c_float, C.c_int, fp, fp,
                                          C.c_int64, C.c_int]
    L.dlg_regulate_normals.argtypes = [vp, C.POINTER(Points), fp, C.c_int64, C.c_int64, C.c_int,
                                       C.c_float, C.POINTER(C.c_uint8), i64p]
    L.dlg_cloud_regulate_normals.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_float,
                                             C.POINTER(C.c_uint8), i64p, fp, C.c_int64]
    L.dlg_refit_planes.argtypes = [C.POINTER(Planes), fp]
    L.dlg_shard_range.argtypes = [C.c_int64, C.c_int, C.c_int, i64p, i64p, C.POINTER(C.c_int)]
    L.dlg_sac_control_create.argtypes = [pp, C.POINTER(SacParams), C.c_int64, C.c_int]
    L.dlg_sac_control_destroy.argtypes = [vp]
    L.dlg_sac_control_next.argtypes = [vp, i32p, C.c_int64, C.POINTER(C.c_int)]
    L.dlg_sac_control_consume.argtypes = [vp, i32p, i32p, C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int)]
    L.dlg_sac_control_result.argtypes = [vp, C.POINTER(SacStats), i64p]
    L.dlg_post_process_planes.argtypes = [vp, C.POINTER(Points), C.POINTER(Planes),
                                          C.POINTER(PostProcessParams), fp, i64p, i32p, C.c_int64,
                                          i32p, C.c_int64, i64p]
    L.dlg_ctx_set_axis.argtypes = [vp, fp, C.c_double]
    L.dlg_ctx_get_axis.argtypes = [vp, fp, C.POINTER(C.c_double)]
    L.dlg_score_samples.argtypes = [vp, vp, C.POINTER(SacParams), i32p, C.c_int, i32p, i32p, i32p,
                                    fp]
    L.dlg_axis_verdicts.argtypes = [C.c_int, C.c_double, fp, C.c_int64, i32p, i32p, fp]
    L.dlg_cluster_filter.argtypes = [vp, C.POINTER(Points), C.c_float, C.c_int32, i32p,
                                     C.c_int64, i64p]
    L.dlg_voxel_grid.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64, C.POINTER(VoxelParams),
                                 fp, C.c_int64, C.c_int64, i64p, i32p, i32p,
                                 C.POINTER(VoxelStats)]
    L.dlg_voxel_grid_cloud.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                       C.POINTER(VoxelParams), C.c_int32, pp, i64p, i32p,
                                       C.POINTER(VoxelStats)]
    L.dlg_statistical_outlier_removal.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                                  C.POINTER(SorParams), i32p, C.c_int64, i64p,
                                                  i32p, C.c_int64, i64p, fp, C.POINTER(SorStats)]
    L.dlg_statistical_outlier_removal_cloud.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                                        C.POINTER(SorParams), C.c_int32, pp, i64p,
                                                        i32p, C.POINTER(SorStats)]
    L.dlg_moving_least_squares.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                           C.POINTER(MlsParams), fp, C.c_int64, fp, C.c_int64, i64p,
                                           i32p, i32p, C.POINTER(MlsStats)]
    L.dlg_moving_least_squares_cloud.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                                 C.POINTER(MlsParams), C.c_int32, pp, i64p, i32p,
                                                 C.POINTER(MlsStats)]
    L.dlg_icp_params_default.argtypes = [C.POINTER(IcpParams)]
    L.dlg_icp_params_default.restype = None
    L.dlg_icp_align.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64, C.POINTER(Points),
                                C.POINTER(IcpParams), fp, fp, fp, C.c_int64,
                                C.POINTER(IcpIteration), C.c_int64, C.POINTER(IcpStats)]
    L.dlg_icp_correspondences.argtypes = [vp, C.POINTER(Points), i32p, C.c_int64,
                                          C.POINTER(Points), fp, C.c_double, i32p, fp, i64p]
    L.dlg_fpfh_estimate.argtypes = [vp, C.POINTER(Points), fp, C.c_int64, i32p, C.c_int64,
                                    C.POINTER(FpfhParams), fp, C.c_int64, i32p, i32p,
                                    C.POINTER(FpfhStats)]
    L.dlg_cloud_fpfh.argtypes = [vp, vp, C.POINTER(FpfhParams), fp, C.c_int64, i32p,
                                 C.POINTER(FpfhStats)]
    L.dlg_sac_ia_params_default.argtypes = [C.POINTER(SacIaParams)]
    L.dlg_sac_ia_params_default.restype = None
    L.dlg_fpfh_knn.argtypes = [vp, fp, C.c_int64, C.c_int64, fp, C.c_int64, C.c_int64, C.c_int32,
                               i32p, fp]
    L.dlg_sac_ia_score.argtypes = [vp, C.POINTER(Points), C.POINTER(Points), fp, C.c_int64,
                                   C.c_double, C.c_int32, C.c_int32, C.POINTER(SacIaHypothesis)]
    L.dlg_sac_ia_align.argtypes = [vp, C.POINTER(Points), fp, C.c_int64, C.POINTER(Points), fp,
                                   C.c_int64, C.POINTER(SacIaParams), fp, fp, fp, C.c_int64,
                                   C.POINTER(SacIaHypothesis), C.c_int64, C.POINTER(SacIaStats)]
    L.dlg_gs_params_default.argtypes = [C.POINTER(GsParams)]
    L.dlg_gs_params_default.restype = None
    L.dlg_gs_space.argtypes = [C.POINTER(GsParams), fp, C.c_int64, i64p]
    L.dlg_gs_vote.argtypes = [vp, fp, C.c_int64, C.c_int64, C.POINTER(GsParams), i32p, i32p,
                              C.c_int64, C.POINTER(GsStats)]
    L.dlg_gs_segment.argtypes = [vp, C.POINTER(Points), fp, C.c_int64, C.POINTER(GsParams),
                                 C.POINTER(GsResult), C.POINTER(GsStats)]
    L.dlg_cloud_gs_segment.argtypes = [vp, vp, C.POINTER(GsParams), C.POINTER(GsResult),
                                       C.POINTER(GsStats)]
    for s in SYMBOLS:
        if s not in ("dlg_abi_version", "dlg_status_string", "dlg_sac_params_default",
                     "dlg_last_error", "dlg_abi_struct_size", "dlg_icp_params_default",
                     "dlg_sac_ia_params_default", "dlg_debug_live_bytes",
                     "dlg_gs_params_default"):
            getattr(L, s).restype = C.c_int
    _lib = L
    return L


class DialogError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"dialog_amd error {status}: {msg}")
        self.status = status


def check(status, ctx=None):
    if status != DLG_OK:
        L = load()
        detail = L.dlg_last_error(ctx).decode(errors="replace")
        raise DialogError(status, f"{L.dlg_status_string(status).decode()}: {detail}")
