"""ctypes binding of include/dvo_amd.h plus a thin Python mirror of the reference interface.

``DenseTracker`` / ``RgbdImagePyramid`` / ``Config`` / ``Result`` carry the same names, argument meaning and error
behaviour as dvo::DenseTracker, dvo::core::RgbdImagePyramid and their nested types
(dvo_core/include/dvo/dense_tracking.h:39-213, dvo_core/include/dvo/core/rgbd_image.h:242-262), so that the parity
tests read like calls into the reference.  All compute goes through the C ABI of libdvo_amd.so (HIP, gfx950): there is
no CPU path here, and loading fails loudly if the library is missing.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

from . import _build

MAX_LEVELS = 8
TERMINATION = {0: "IterationsExceeded", 1: "IncrementTooSmall", 2: "LogLikelihoodDecreased", 3: "TooFewConstraints",
               -1: "Unset"}

EXPORTS = [
    "dvo_amd_abi_version", "dvo_amd_build_id", "dvo_amd_status_string", "dvo_amd_last_error", "dvo_amd_device_count",
    "dvo_amd_default_config", "dvo_amd_context_create", "dvo_amd_context_destroy", "dvo_amd_configure",
    "dvo_amd_get_config", "dvo_amd_pyramid_create", "dvo_amd_pyramid_create_from_device", "dvo_amd_pyramid_retain",
    "dvo_amd_pyramid_release", "dvo_amd_pyramid_levels", "dvo_amd_pyramid_timestamp", "dvo_amd_pyramid_level_info",
    "dvo_amd_pyramid_download_plane", "dvo_amd_pyramid_select", "dvo_amd_match", "dvo_amd_match_batch",
    "dvo_amd_residuals", "dvo_amd_error_image", "dvo_amd_kernel_timing", "dvo_amd_se3_exp", "dvo_amd_se3_log",
    "dvo_amd_solve6", "dvo_amd_bench_residual_pass", "dvo_amd_match_many",
    "dvo_amd_debug_finalize_stamps", "dvo_amd_comm_unique_id", "dvo_amd_comm_create", "dvo_amd_comm_destroy",
    "dvo_amd_match_sharded", "dvo_amd_match_banded", "dvo_amd_context_device", "dvo_amd_debug_combine_bands", "dvo_amd_debug_wire_layout", "dvo_amd_debug_take_wire", "dvo_amd_pyramid_create_raw",
    "dvo_amd_default_validator_stages", "dvo_amd_proposals_for_candidates", "dvo_amd_validate_proposals",
    "dvo_amd_track_frame", "dvo_amd_png_info", "dvo_amd_png_read_bgr8", "dvo_amd_png_read_gray16",
    "dvo_amd_format_trajectory_line", "dvo_amd_debug_tick_log", "dvo_amd_debug_iteration", "dvo_amd_match_selection", "dvo_amd_bench_residual_pass_pairs",
    "dvo_amd_exchange_create", "dvo_amd_exchange_attach", "dvo_amd_exchange_destroy",
    "dvo_amd_match_submit", "dvo_amd_match_wait", "dvo_amd_match_poll", "dvo_amd_debug_next_seq",
    "dvo_amd_set_reciprocal_mode", "dvo_amd_get_reciprocal_mode", "dvo_amd_debug_rcp", "dvo_amd_debug_block_trace",
    "dvo_amd_debug_ll_overflow", "dvo_amd_debug_marker", "dvo_amd_debug_rcp_form", "dvo_amd_debug_weights", "dvo_amd_debug_hw_queue",
    "dvo_amd_debug_level_geometry", "dvo_amd_point_cloud", "dvo_amd_map_cloud", "dvo_amd_voxel_downsample", "dvo_amd_write_pcd",
    "dvo_amd_debug_map_timing", "dvo_amd_default_graph_options", "dvo_amd_optimize_graph", "dvo_amd_graph_marginals", "dvo_amd_debug_graph_timing",
    "dvo_amd_debug_graph_system", "dvo_amd_debug_graph_system_sparse", "dvo_amd_debug_graph_symbolic",
    "dvo_amd_debug_graph_sparse_timing", "dvo_amd_optimize_graphs_batch", "dvo_amd_debug_graph_batch_records",
    "dvo_amd_debug_tick_layout",
    "dvo_amd_map_create", "dvo_amd_map_destroy", "dvo_amd_map_insert", "dvo_amd_map_set_poses", "dvo_amd_map_remove",
    "dvo_amd_map_stats", "dvo_amd_map_extract", "dvo_amd_map_render", "dvo_amd_map_render_pyramid", "dvo_amd_debug_keyframe_map_timing", "dvo_amd_debug_map_merge",
    "dvo_amd_default_covisibility_options", "dvo_amd_covisibility", "dvo_amd_find_constraint_candidates",
    "dvo_amd_debug_covisibility_ms",
    "dvo_amd_remap_create", "dvo_amd_remap_create_undistort", "dvo_amd_remap_retain", "dvo_amd_remap_release", "dvo_amd_remap_info",
    "dvo_amd_remap_download", "dvo_amd_pyramid_create_raw_remapped", "dvo_amd_debug_ingest_timing",
    "dvo_amd_default_registration", "dvo_amd_pyramid_create_raw_registered",
    "dvo_amd_pyramid_create_raw_batch", "dvo_amd_debug_batch_build_stats",
    "dvo_amd_mask_create", "dvo_amd_mask_create_levels", "dvo_amd_mask_retain", "dvo_amd_mask_release", "dvo_amd_mask_info",
    "dvo_amd_mask_download", "dvo_amd_pyramid_select_masked", "dvo_amd_match_masked", "dvo_amd_match_many_masked",
    "dvo_amd_default_budget_options", "dvo_amd_mask_create_budget",
    "dvo_amd_default_mask_warp_options", "dvo_amd_mask_combine", "dvo_amd_mask_morph", "dvo_amd_mask_warp", "dvo_amd_mask_warp_many",
    "dvo_amd_debug_mask_ops_timing",
    "dvo_amd_default_residual_mask_options", "dvo_amd_mask_from_residuals", "dvo_amd_mask_from_residuals_many",
    "dvo_amd_default_fuse_options", "dvo_amd_pyramid_fuse_depth", "dvo_amd_pyramid_fuse_depth_many", "dvo_amd_debug_fuse_timing",
    "dvo_amd_default_place_options", "dvo_amd_default_place_query_options", "dvo_amd_place_index_create", "dvo_amd_place_index_destroy",
    "dvo_amd_place_index_add", "dvo_amd_place_index_info", "dvo_amd_place_index_download", "dvo_amd_place_scores", "dvo_amd_place_query",
    "dvo_amd_place_query_frames", "dvo_amd_debug_place_timing",
    "dvo_amd_debug_residuals_masked", "dvo_amd_debug_iteration_masked", "dvo_amd_debug_weights_masked",
    "dvo_amd_default_normal_options", "dvo_amd_pyramid_normals", "dvo_amd_mask_from_normals", "dvo_amd_point_cloud_normals",
    "dvo_amd_write_pcd_normals", "dvo_amd_debug_normals_timing",
    "dvo_amd_default_depth_filter_options", "dvo_amd_pyramid_filter_depth", "dvo_amd_pyramid_filter_depth_many",
    "dvo_amd_debug_depth_filter_timing",
    "dvo_amd_default_component_options", "dvo_amd_mask_filter_components", "dvo_amd_mask_filter_components_many",
    "dvo_amd_mask_components", "dvo_amd_debug_components_timing",
    "dvo_amd_default_pose_score_options", "dvo_amd_score_poses", "dvo_amd_score_poses_many", "dvo_amd_rank_poses", "dvo_amd_pose_grid",
    "dvo_amd_default_exposure_options", "dvo_amd_estimate_exposure", "dvo_amd_estimate_exposure_many",
    "dvo_amd_pyramid_adjust_intensity", "dvo_amd_pyramid_adjust_intensity_many", "dvo_amd_debug_exposure_timing",
    "dvo_amd_default_warp_options", "dvo_amd_warp_inverse", "dvo_amd_warp_inverse_many", "dvo_amd_pyramid_warp_inverse",
    "dvo_amd_pyramid_warp_inverse_many", "dvo_amd_warp_forward", "dvo_amd_warp_forward_many", "dvo_amd_pyramid_warp_forward",
    "dvo_amd_pyramid_warp_forward_many", "dvo_amd_debug_warp_timing",
    "dvo_amd_default_volume_options", "dvo_amd_default_volume_raycast_options", "dvo_amd_volume_create", "dvo_amd_volume_destroy",
    "dvo_amd_volume_clear", "dvo_amd_volume_options_get", "dvo_amd_volume_integrate", "dvo_amd_volume_insert",
    "dvo_amd_volume_set_poses", "dvo_amd_volume_remove", "dvo_amd_volume_stats", "dvo_amd_volume_download", "dvo_amd_volume_raycast",
    "dvo_amd_volume_raycast_pyramid", "dvo_amd_volume_extract", "dvo_amd_debug_volume_timing",
    "dvo_amd_volume_mesh", "dvo_amd_volume_upload", "dvo_amd_write_ply",
]


class CConfig(C.Structure):
    _fields_ = [("first_level", C.c_int), ("last_level", C.c_int), ("max_iterations_per_level", C.c_int),
                ("precision", C.c_double), ("mu", C.c_double), ("use_initial_estimate", C.c_int),
                ("intensity_derivative_threshold", C.c_float), ("depth_derivative_threshold", C.c_float),
                ("segment_geometry", C.c_int), ("reserved", C.c_int)]


GEOMETRY_THROUGHPUT, GEOMETRY_LATENCY = 0, 1


class CIterationStats(C.Structure):
    _fields_ = [("id", C.c_int), ("valid_constraints", C.c_int), ("tdist_loglik", C.c_double),
                ("tdist_mean", C.c_double * 2), ("tdist_precision", C.c_double * 4), ("prior_loglik", C.c_double),
                ("increment", C.c_double * 6), ("information", C.c_double * 36), ("has_increment", C.c_int),
                ("reserved", C.c_int), ("estimate", C.c_double * 16), ("initial", C.c_double * 16)]


class CLevelStats(C.Structure):
    _fields_ = [("id", C.c_int), ("max_valid_pixels", C.c_int), ("valid_pixels", C.c_int), ("termination", C.c_int),
                ("n_iterations", C.c_int), ("first_iteration", C.c_int)]


class CResult(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("information", C.c_double * 36), ("loglik", C.c_double),
                ("is_nan", C.c_int), ("n_levels", C.c_int), ("levels", CLevelStats * MAX_LEVELS),
                ("n_iterations", C.c_int), ("iterations_capacity", C.c_int),
                ("iterations", C.POINTER(CIterationStats)), ("n_ticks", C.c_int), ("n_residual_passes", C.c_int),
                ("alg_bytes", C.c_double), ("alg_bytes_discarded", C.c_double)]


class CFrameCriteria(C.Structure):
    _fields_ = [("odometry_is_nan", C.c_int), ("keyframe_is_nan", C.c_int), ("odometry_translation_norm", C.c_double),
                ("keyframe_translation_norm", C.c_double), ("keyframe_constraint_ratio", C.c_double),
                ("odometry_neg_loglik", C.c_double), ("keyframe_neg_loglik", C.c_double),
                ("odometry_condition_number", C.c_double), ("keyframe_condition_number", C.c_double)]


class CIterationProbe(C.Structure):
    _fields_ = [("valid_constraints", C.c_int), ("reserved", C.c_int), ("scale_sums", C.c_double * 3),
                ("scale", C.c_float * 4), ("precision", C.c_float * 4), ("moments", C.c_double * 87),
                ("information", C.c_double * 36), ("rhs", C.c_double * 6), ("loglik_sum", C.c_double),
                ("loglik", C.c_float), ("reserved_f", C.c_float)]


class CQ7Probe(C.Structure):
    _fields_ = [("n_tail", C.c_int), ("valid_constraints", C.c_int), ("valid_counted", C.c_int), ("recomputed_equal", C.c_int),
                ("pixel", C.c_int * 3), ("weight_table", C.c_float * 3), ("weight_exact", C.c_float * 3),
                ("scale_sums_delta", C.c_double * 3), ("moments_delta", C.c_double * 87)]


class CCloudStats(C.Structure):
    _fields_ = [("points_in", C.c_longlong), ("finite", C.c_longlong), ("out_of_range", C.c_longlong), ("voxels", C.c_longlong)]


class CView(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("ox", C.c_float),
                ("oy", C.c_float), ("near_z", C.c_float)]


class CRenderStats(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("voxels", "behind_near", "outside", "drawn", "covered_pixels")]


class CRegistration(C.Structure):
    _fields_ = [("depth_width", C.c_int), ("depth_height", C.c_int), ("k_depth", C.c_float * 4), ("T", C.c_double * 16),
                ("min_z", C.c_float), ("fill", C.c_int)]


class CRawBatch(C.Structure):
    _fields_ = [("count", C.c_int), ("images", C.POINTER(C.c_void_p)), ("depths", C.POINTER(C.c_void_p)),
                ("timestamps", C.POINTER(C.c_double)), ("channels", C.c_int), ("image_stride_bytes", C.c_int),
                ("depth_stride", C.c_int), ("depth_scale", C.c_float), ("on_device", C.c_int), ("width", C.c_int),
                ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("ox", C.c_float), ("oy", C.c_float),
                ("levels", C.c_int), ("build_selection", C.c_int), ("intensity_threshold", C.c_float),
                ("depth_threshold", C.c_float)]


class CRegistrationStats(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("measurements", "behind", "outside", "drawn", "covered_pixels")]


class CKeyframe(C.Structure):
    _fields_ = [("id", C.c_int), ("image", C.c_void_p), ("pose", C.c_double * 16), ("evaluation_kind", C.c_int),
                ("evaluation_average", C.c_double), ("evaluation_n", C.c_double)]


class CCovisibilityOptions(C.Structure):
    _fields_ = [("level", C.c_int), ("near_z", C.c_float), ("depth_sigmas", C.c_float)]


class BudgetOptions(C.Structure):
    """dvo_amd_budget_options, field for field"""
    _fields_ = [("rule", C.c_int), ("budget", C.c_longlong * MAX_LEVELS), ("cell", C.c_int * MAX_LEVELS),
                ("intensity_threshold", C.c_float), ("depth_threshold", C.c_float), ("depth_weight", C.c_float),
                ("within", C.c_void_p)]


class MaskWarpOptions(C.Structure):
    """dvo_amd_mask_warp_options, field for field"""
    _fields_ = [("near_z", C.c_float), ("depth_sigmas", C.c_float), ("unseen_keep", C.c_int), ("inconsistent_keep", C.c_int)]


class WarpOptions(C.Structure):
    """dvo_amd_warp_options, field for field"""
    _fields_ = [("near_z", C.c_float), ("occlusion_margin", C.c_float), ("depth", C.c_int), ("splat", C.c_int),
                ("fill_intensity", C.c_float)]


class VolumeOptions(C.Structure):
    """dvo_amd_volume_options, field for field"""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("voxel", C.c_float), ("origin", C.c_float * 3), ("trunc", C.c_float),
                ("near_z", C.c_float), ("far_z", C.c_float), ("weight", C.c_int)]


class VolumeRaycastOptions(C.Structure):
    """dvo_amd_volume_raycast_options, field for field"""
    _fields_ = [("step_fraction", C.c_float), ("min_weight", C.c_int), ("fill_intensity", C.c_float)]


class CVolumeRaycastStats(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("pixels", "hit", "backface", "missed", "uncoloured")]


class CVolumeExtractCounts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("points", "uncoloured")]


class CVolumeMeshCounts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("vertices", "triangles", "open_edges", "uncoloured", "flat")]


class ResidualMaskOptions(C.Structure):
    """dvo_amd_residual_mask_options, field for field"""
    _fields_ = [("precision", (C.c_float * 4) * MAX_LEVELS), ("max_distance", C.c_float * MAX_LEVELS), ("invalid_keep", C.c_int),
                ("unevaluated_keep", C.c_int)]


class PoseScoreOptions(C.Structure):
    """dvo_amd_pose_score_options, field for field"""
    _fields_ = [("level", C.c_int), ("precision", C.c_float * 4), ("max_distance", C.c_float), ("invalid_distance", C.c_float)]


class PoseGridOptions(C.Structure):
    """dvo_amd_pose_grid_options, field for field"""
    _fields_ = [("count", C.c_int * 6), ("step", C.c_double * 6)]


# one dvo_amd_pose_score, field for field
POSE_SCORE_FIELDS = ("evaluated", "invalid", "inlier", "outlier", "cost", "total")
POSE_SCORE_DTYPE = np.dtype([(name, np.int64) for name in POSE_SCORE_FIELDS[:4]] + [(name, np.uint64) for name in POSE_SCORE_FIELDS[4:]])
POSE_SCORE_TILE = 32  # hypotheses a block of k_score_poses takes per visit (kPoseScoreTile, dvo_types.h)
POSE_GRID_AXES = ("vx", "vy", "vz", "wx", "wy", "wz")


EXPOSURE_MAX_REFITS = 8
# the counts of a dvo_amd_exposure_estimate in the record's order, and its six sums
EXPOSURE_COUNTS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through", "masked", "saturated",
                   "candidates", "used", "trimmed")
EXPOSURE_SUMS = ("n", "sx", "sy", "sxx", "sxy", "syy")


class ExposureOptions(C.Structure):
    """dvo_amd_exposure_options, field for field"""
    _fields_ = [("level", C.c_int), ("near_z", C.c_float), ("depth_sigmas", C.c_float), ("min_intensity", C.c_float),
                ("max_intensity", C.c_float), ("scale", C.c_float), ("trim", C.c_float), ("refits", C.c_int),
                ("min_pairs", C.c_longlong), ("min_gain", C.c_double), ("max_gain", C.c_double)]


class ExposureEstimate(C.Structure):
    """dvo_amd_exposure_estimate, field for field"""
    _fields_ = ([("gain", C.c_double), ("bias", C.c_double), ("r2", C.c_double), ("passes", C.c_int), ("degenerate", C.c_int)] +
                [(name, C.c_longlong) for name in EXPOSURE_COUNTS + EXPOSURE_SUMS] +
                [("gain_pass", C.c_double * (EXPOSURE_MAX_REFITS + 1)), ("bias_pass", C.c_double * (EXPOSURE_MAX_REFITS + 1)),
                 ("used_pass", C.c_longlong * (EXPOSURE_MAX_REFITS + 1))])

    def as_dict(self) -> dict:
        """every field as a Python value (the per-pass arrays as lists of all nine entries)"""
        return {name: (list(getattr(self, name)) if name.endswith("_pass") else getattr(self, name)) for name, _ in self._fields_}


class FuseOptions(C.Structure):
    """dvo_amd_fuse_options, field for field"""
    _fields_ = [("near_z", C.c_float), ("depth_sigmas", C.c_float), ("min_cos", C.c_float), ("sample", C.c_int),
                ("min_observations", C.c_int), ("drop_unconfirmed", C.c_int)]


class DepthFilterOptions(C.Structure):
    """dvo_amd_depth_filter_options, field for field"""
    _fields_ = [("radius", C.c_int), ("range_sigmas", C.c_float), ("min_support", C.c_int), ("fill_radius", C.c_int),
                ("min_fill_support", C.c_int)]


DEPTH_FILTER_MAX_RADIUS = 8
# one record of dvo_amd_pyramid_filter_depth's counts, field for field
DEPTH_FILTER_COUNTS = ("with_depth", "kept", "dropped", "holes", "filled")
DEPTH_FILTER_DTYPE = np.dtype([(name, np.int64) for name in DEPTH_FILTER_COUNTS])


class ComponentOptions(C.Structure):
    """dvo_amd_component_options, field for field"""
    _fields_ = [("connectivity", C.c_int), ("max_step", C.c_float), ("depth_sigmas", C.c_float), ("min_area", C.c_int * MAX_LEVELS),
                ("max_area", C.c_int * MAX_LEVELS), ("keep_largest", C.c_int)]


COMPONENTS_MAX_LARGEST = 8
COMPONENTS_FIRST_CAPACITY = 4096  # records the binding makes room for in its first dvo_amd_mask_components call
# one record of dvo_amd_mask_filter_components' counts and one dvo_amd_component, field for field
COMPONENT_COUNTS = ("foreground", "components", "kept_components", "kept_pixels", "largest_area", "edges_cut")
COMPONENT_COUNTS_DTYPE = np.dtype([(name, np.int64) for name in COMPONENT_COUNTS])
COMPONENT_DTYPE = np.dtype([(name, np.int32) for name in ("root", "area", "x0", "y0", "x1", "y1", "seeded")])


class NormalOptions(C.Structure):
    """dvo_amd_normal_options, field for field"""
    _fields_ = [("radius", C.c_int * MAX_LEVELS), ("depth_step_ratio", C.c_float), ("facing", C.c_int), ("toward_camera", C.c_int)]


NORMAL_MAX_RADIUS = 8
NORMAL_FACING_AXIS, NORMAL_FACING_RAY = 0, 1
# dvo_amd_pyramid_normals' counts and one level of dvo_amd_mask_from_normals' counts, field for field
NORMAL_COUNTS = ("defined", "undefined")
NORMAL_MASK_COUNTS = ("defined", "undefined", "kept")
NORMAL_MASK_DTYPE = np.dtype([(name, np.int64) for name in NORMAL_MASK_COUNTS])


class PlaceOptions(C.Structure):
    """dvo_amd_place_options, field for field"""
    _fields_ = [("level", C.c_int), ("gain", C.c_float)]


class PlaceQueryOptions(C.Structure):
    """dvo_amd_place_query_options, field for field"""
    _fields_ = [("k", C.c_int), ("min_score", C.c_double), ("exclude_recent", C.c_int)]


PLACE_MAX_K = 64
PLACE_MAX_DIM = 65536
PLACE_INITIAL_CAPACITY = 64

FUSE_BILINEAR, FUSE_NEAREST = 0, 1
FUSE_MAX_FRAMES = 255
# one record of dvo_amd_pyramid_fuse_depth's frame counts and of its keyframe counts, field for field
FUSE_FRAME_COUNTS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through", "fused")
FUSE_FRAME_DTYPE = np.dtype([(name, np.int64) for name in FUSE_FRAME_COUNTS])
FUSE_KEYFRAME_COUNTS = ("with_depth", "confirmed", "unconfirmed_kept", "unconfirmed_dropped")
FUSE_KEYFRAME_DTYPE = np.dtype([(name, np.int64) for name in FUSE_KEYFRAME_COUNTS])

# one record of dvo_amd_mask_from_residuals' counts, field for field
RESIDUAL_MASK_COUNTS = ("evaluated", "invalid", "inlier", "outlier", "kept")
RESIDUAL_MASK_DTYPE = np.dtype([(name, np.int64) for name in RESIDUAL_MASK_COUNTS])
RESIDUAL_MASK_MAX_DISTANCE = 9.2103  # -2 ln 0.01: the 99 % point of chi-square with two degrees of freedom

# one record of dvo_amd_mask_warp's counts, field for field
MASK_WARP_COUNTS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through", "dropped_by_source")
MASK_WARP_DTYPE = np.dtype([(name, np.int64) for name in MASK_WARP_COUNTS])

# frame warps: the depth an inverse warp returns, the pixels a forward warp covers, and one record of each direction's counts
WARP_DEPTH_TRANSFORMED, WARP_DEPTH_FIXED = 0, 1
WARP_SPLAT_NEAREST, WARP_SPLAT_FLOOR, WARP_SPLAT_FOOTPRINT = 0, 1, 2
WARP_MAX_FOOTPRINT = 16
WARP_INVERSE_COUNTS = ("valid", "behind", "outside", "border", "hidden", "warped", "partial", "no_depth")
WARP_INVERSE_DTYPE = np.dtype([(name, np.int64) for name in WARP_INVERSE_COUNTS])
WARP_FORWARD_COUNTS = ("valid", "behind", "outside", "too_large", "drawn", "covered_pixels", "no_depth")
WARP_FORWARD_DTYPE = np.dtype([(name, np.int64) for name in WARP_FORWARD_COUNTS])

# the signed-distance volume: its weights, one public voxel record and one record of an integration's counts, field for field
VOLUME_WEIGHT_CONSTANT, VOLUME_WEIGHT_SENSOR = 0, 1
VOLUME_MAX_STEPS = 8192
VOLUME_VOXEL_DTYPE = np.dtype([(name, np.int32) for name in ("w_sum", "sd_sum", "iw_sum", "i_sum")])
VOLUME_COUNTS = ("updated", "near", "free")
VOLUME_COUNTS_DTYPE = np.dtype([(name, np.int64) for name in VOLUME_COUNTS])

# dvo_amd_covisibility_counts, field for field
COVISIBILITY_DTYPE = np.dtype([(name, np.uint32) for name in ("valid", "behind", "outside", "no_depth", "consistent", "occluded",
                                                             "seen_through", "reserved")])


class DvoAmdError(RuntimeError):
    def __init__(self, status: int, where: str):
        L = lib()
        msg = L.dvo_amd_status_string(status).decode()
        detail = L.dvo_amd_last_error().decode()
        super().__init__(f"{where}: {msg}" + (f" [{detail}]" if detail else ""))
        self.status = status


_lib = None


def lib():
    """Load libdvo_amd.so (building it in-tree with hipcc if the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch wheels bundle their own ROCm runtime (libamdhip64 / libhsa-runtime64).  Two HIP runtimes in one process do not
    # share devices ("No HIP GPUs are available" in whichever initialises second), so when torch is installed let it load
    # its copy first: this library's DT_NEEDED libamdhip64.so.N then binds to that same copy.
    if os.environ.get("DVO_AMD_PRELOAD_TORCH", "1") != "0":
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent or broken: the system runtime under /opt/rocm is used
            pass
    path = _build.LIB_PATH
    if _build.needs_build():
        # missing, or not built from exactly the sources next to it (dvo_amd_build_id() != the hash of csrc/* + flags)
        try:
            path = _build.build()
        except RuntimeError as exc:
            raise RuntimeError(f"{path} is missing or stale (build id {_build.library_id()!r}, sources {_build.source_id()!r}) "
                               f"and cannot be rebuilt here: {exc}") from exc
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m dvo_slam_amd._build` (no CPU fallback exists)")
    L = C.CDLL(path)
    L.dvo_amd_build_id.restype = C.c_char_p
    if not os.environ.get("DVO_AMD_LIB") and L.dvo_amd_build_id().decode() != _build.source_id():
        raise RuntimeError(f"{path} carries build id {L.dvo_amd_build_id().decode()!r} but the sources next to it hash to "
                           f"{_build.source_id()!r}: refusing to run an edited tree against a stale binary")
    fp = C.POINTER(C.c_float)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    L.dvo_amd_abi_version.restype = C.c_int
    L.dvo_amd_status_string.restype = C.c_char_p
    L.dvo_amd_status_string.argtypes = [C.c_int]
    L.dvo_amd_last_error.restype = C.c_char_p
    L.dvo_amd_device_count.restype = C.c_int
    L.dvo_amd_default_config.argtypes = [C.POINTER(CConfig)]
    L.dvo_amd_context_create.argtypes = [C.c_int, C.POINTER(CConfig), C.POINTER(vp)]
    L.dvo_amd_context_destroy.argtypes = [vp]
    L.dvo_amd_context_destroy.restype = None
    L.dvo_amd_configure.argtypes = [vp, C.POINTER(CConfig)]
    L.dvo_amd_get_config.argtypes = [vp, C.POINTER(CConfig)]
    L.dvo_amd_set_reciprocal_mode.argtypes = [vp, C.c_int]
    L.dvo_amd_get_reciprocal_mode.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dvo_amd_debug_rcp.argtypes = [vp, C.c_int, fp, fp]
    L.dvo_amd_debug_marker.argtypes = [vp, C.c_uint]
    L.dvo_amd_debug_rcp_form.argtypes = [vp, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.dvo_amd_debug_ll_overflow.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp,
                                            C.POINTER(C.c_int)]
    L.dvo_amd_pyramid_create.argtypes = [C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_int, C.c_double, C.POINTER(vp)]
    L.dvo_amd_pyramid_create_from_device.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                                     C.c_float, C.c_float, C.c_int, C.c_double, C.POINTER(vp)]
    L.dvo_amd_pyramid_create_raw.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_float, C.c_int, C.c_int,
                                             C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_double,
                                             C.POINTER(vp)]
    L.dvo_amd_track_frame.argtypes = [vp, vp, vp, vp, dp, C.POINTER(CResult), C.POINTER(CResult), C.POINTER(CFrameCriteria)]
    L.dvo_amd_pyramid_retain.argtypes = [vp]
    L.dvo_amd_pyramid_retain.restype = None
    L.dvo_amd_pyramid_release.argtypes = [vp]
    L.dvo_amd_pyramid_release.restype = None
    L.dvo_amd_pyramid_levels.argtypes = [vp]
    L.dvo_amd_pyramid_timestamp.argtypes = [vp]
    L.dvo_amd_pyramid_timestamp.restype = C.c_double
    L.dvo_amd_pyramid_level_info.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), fp]
    L.dvo_amd_pyramid_download_plane.argtypes = [vp, C.c_int, C.c_int, fp]
    L.dvo_amd_pyramid_select.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_ubyte)]
    L.dvo_amd_match.argtypes = [vp, vp, vp, dp, C.POINTER(CResult)]
    L.dvo_amd_match_selection.argtypes = [vp, vp, C.c_float, C.c_float, vp, dp, C.POINTER(CResult)]
    L.dvo_amd_match_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(CResult)]
    L.dvo_amd_match_many.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(CResult), C.c_int]
    L.dvo_amd_match_submit.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(CResult), C.c_int,
                                       C.POINTER(C.c_ulonglong)]
    L.dvo_amd_match_wait.argtypes = [vp, C.c_ulonglong]
    L.dvo_amd_match_poll.argtypes = [vp, C.c_ulonglong, C.POINTER(C.c_int)]
    L.dvo_amd_residuals.argtypes = [vp, vp, vp, C.c_int, fp, fp, C.POINTER(C.c_int)]
    L.dvo_amd_error_image.argtypes = [vp, vp, vp, dp, C.c_int, fp]
    L.dvo_amd_debug_iteration.argtypes = [vp, vp, vp, C.c_int, fp, fp, fp, C.POINTER(CIterationProbe)]
    L.dvo_amd_debug_hw_queue.argtypes = [vp, C.POINTER(C.c_int)]
    L.dvo_amd_debug_level_geometry.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dvo_amd_debug_weights.argtypes = [vp, vp, vp, C.c_int, fp, fp, fp, C.POINTER(CQ7Probe)]
    L.dvo_amd_debug_residuals_masked.argtypes = [vp, vp, vp, C.c_int, fp, vp, fp, C.POINTER(C.c_int)]
    L.dvo_amd_debug_iteration_masked.argtypes = [vp, vp, vp, C.c_int, fp, fp, fp, vp, C.POINTER(CIterationProbe)]
    L.dvo_amd_debug_weights_masked.argtypes = [vp, vp, vp, C.c_int, fp, fp, vp, fp, C.POINTER(CQ7Probe)]
    L.dvo_amd_kernel_timing.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_longlong), C.c_int]
    L.dvo_amd_bench_residual_pass.argtypes = [vp, vp, vp, C.c_int, fp, C.c_int, C.c_int, C.c_int, dp, dp,
                                              C.POINTER(C.c_int)]
    L.dvo_amd_bench_residual_pass_pairs.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, fp, C.c_int, C.c_int, dp, dp,
                                                    C.POINTER(C.c_int)]
    L.dvo_amd_debug_finalize_stamps.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.dvo_amd_comm_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
    L.dvo_amd_comm_create.argtypes = [vp, C.POINTER(C.c_ubyte), C.c_int, C.c_int]
    L.dvo_amd_comm_destroy.argtypes = [vp]
    L.dvo_amd_comm_destroy.restype = None
    L.dvo_amd_exchange_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]
    L.dvo_amd_exchange_attach.argtypes = [vp, C.POINTER(C.c_ubyte)]
    L.dvo_amd_exchange_destroy.argtypes = [vp]
    L.dvo_amd_exchange_destroy.restype = None
    L.dvo_amd_match_sharded.argtypes = [vp, vp, vp, dp, C.POINTER(CResult)]
    L.dvo_amd_match_banded.argtypes = [vp, vp, vp, dp, C.POINTER(CResult), C.c_int]
    L.dvo_amd_debug_combine_bands.argtypes = [C.c_int, dp, dp]
    L.dvo_amd_debug_block_trace.restype = C.c_longlong
    L.dvo_amd_debug_block_trace.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_longlong]
    L.dvo_amd_debug_wire_layout.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dvo_amd_debug_take_wire.argtypes = [C.POINTER(C.c_uint), C.c_uint, C.c_int, C.POINTER(C.c_uint)]
    L.dvo_amd_debug_next_seq.argtypes = [C.c_uint]
    ip = C.POINTER(C.c_int)
    L.dvo_amd_debug_tick_layout.argtypes = [C.c_int, ip, ip, ip, ip, ip, C.c_int, C.c_int, ip, ip, ip, ip, ip, ip, ip, C.c_longlong, ip, ip]
    L.dvo_amd_debug_next_seq.restype = C.c_uint
    L.dvo_amd_point_cloud.argtypes = [vp, vp, C.c_int, dp, vp, C.c_int, vp]
    L.dvo_amd_map_cloud.argtypes = [vp, C.c_int, C.POINTER(vp), dp, C.POINTER(vp), C.POINTER(C.c_int), C.c_float, vp,
                                    C.c_longlong, C.POINTER(CCloudStats)]
    L.dvo_amd_voxel_downsample.argtypes = [vp, C.c_longlong, vp, C.c_float, vp, C.c_longlong, C.POINTER(CCloudStats)]
    L.dvo_amd_write_pcd.argtypes = [C.c_char_p, vp, C.c_longlong, C.c_int, C.c_int]
    L.dvo_amd_debug_map_timing.argtypes = [vp, dp, dp, C.POINTER(C.c_longlong)]
    L.dvo_amd_map_create.argtypes = [vp, C.c_float, C.POINTER(vp)]
    L.dvo_amd_map_destroy.argtypes = [vp]
    L.dvo_amd_map_destroy.restype = None
    L.dvo_amd_map_insert.argtypes = [vp, C.c_int, vp, dp, vp, C.c_int]
    L.dvo_amd_map_set_poses.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp]
    L.dvo_amd_map_remove.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.dvo_amd_map_stats.argtypes = [vp, C.POINTER(CCloudStats), C.POINTER(C.c_int)]
    L.dvo_amd_map_extract.argtypes = [vp, C.POINTER(C.c_float), vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.dvo_amd_map_render.argtypes = [vp, dp, C.POINTER(CView), vp, vp, vp, vp, C.POINTER(CRenderStats)]
    L.dvo_amd_map_render_pyramid.argtypes = [vp, dp, C.POINTER(CView), C.c_int, C.c_double, C.POINTER(vp), C.POINTER(CRenderStats)]
    L.dvo_amd_debug_keyframe_map_timing.argtypes = [vp, dp, dp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                                    C.POINTER(C.c_int)]
    L.dvo_amd_debug_map_merge.argtypes = [vp, C.c_longlong, vp, vp, C.c_longlong, vp, vp, vp, vp, C.POINTER(C.c_longlong)]
    L.dvo_amd_default_covisibility_options.argtypes = [C.POINTER(CCovisibilityOptions)]
    L.dvo_amd_default_covisibility_options.restype = None
    L.dvo_amd_covisibility.argtypes = [vp, C.c_int, C.POINTER(CKeyframe), C.POINTER(CCovisibilityOptions), C.c_int,
                                       C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    L.dvo_amd_find_constraint_candidates.argtypes = [vp, C.c_int, C.POINTER(CKeyframe), C.c_int, C.c_float, C.c_double,
                                                     C.POINTER(CCovisibilityOptions), C.POINTER(C.c_int), dp, C.c_int,
                                                     C.POINTER(C.c_int)]
    L.dvo_amd_debug_covisibility_ms.argtypes = [vp, dp]
    L.dvo_amd_remap_create.argtypes = [C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.dvo_amd_remap_create_undistort.argtypes = [C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, fp, C.POINTER(vp)]
    L.dvo_amd_remap_retain.argtypes = [vp]
    L.dvo_amd_remap_retain.restype = None
    L.dvo_amd_remap_release.argtypes = [vp]
    L.dvo_amd_remap_release.restype = None
    L.dvo_amd_remap_info.argtypes = [vp, ip, ip, ip, ip, ip]
    L.dvo_amd_remap_download.argtypes = [vp, fp, fp]
    L.dvo_amd_pyramid_create_raw_remapped.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_float, C.c_int, vp,
                                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_double,
                                                      C.POINTER(vp)]
    L.dvo_amd_debug_ingest_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_default_registration.argtypes = [C.POINTER(CRegistration)]
    L.dvo_amd_default_registration.restype = None
    L.dvo_amd_pyramid_create_raw_registered.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_float, C.c_int,
                                                        C.POINTER(CRegistration), vp, C.c_int, C.c_int, C.c_float, C.c_float,
                                                        C.c_float, C.c_float, C.c_int, C.c_double, C.POINTER(vp),
                                                        C.POINTER(CRegistrationStats)]
    L.dvo_amd_pyramid_create_raw_batch.argtypes = [C.c_int, C.POINTER(CRawBatch), C.POINTER(vp)]
    L.dvo_amd_debug_batch_build_stats.argtypes = [C.c_int, ip, ip, ip]
    L.dvo_amd_mask_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.dvo_amd_mask_create_levels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), ip, C.c_int, C.POINTER(vp)]
    L.dvo_amd_mask_retain.argtypes = [vp]
    L.dvo_amd_mask_retain.restype = None
    L.dvo_amd_mask_release.argtypes = [vp]
    L.dvo_amd_mask_release.restype = None
    L.dvo_amd_mask_info.argtypes = [vp, ip, ip, ip, C.POINTER(C.c_longlong)]
    L.dvo_amd_mask_download.argtypes = [vp, C.c_int, C.POINTER(C.c_ubyte)]
    L.dvo_amd_pyramid_select_masked.argtypes = [vp, C.c_int, C.c_float, C.c_float, vp, C.POINTER(C.c_int), C.POINTER(C.c_ubyte)]
    L.dvo_amd_match_masked.argtypes = [vp, vp, vp, C.c_float, C.c_float, vp, dp, C.POINTER(CResult)]
    L.dvo_amd_match_many_masked.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(CResult), C.c_int]
    L.dvo_amd_default_budget_options.argtypes = [C.POINTER(BudgetOptions)]
    L.dvo_amd_default_budget_options.restype = None
    L.dvo_amd_mask_create_budget.argtypes = [vp, C.POINTER(BudgetOptions), C.POINTER(vp)]
    L.dvo_amd_default_mask_warp_options.argtypes = [C.POINTER(MaskWarpOptions)]
    L.dvo_amd_default_mask_warp_options.restype = None
    L.dvo_amd_mask_combine.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.dvo_amd_mask_morph.argtypes = [vp, C.c_int, ip, C.POINTER(vp)]
    L.dvo_amd_mask_warp.argtypes = [vp, vp, vp, dp, C.POINTER(MaskWarpOptions), C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.dvo_amd_mask_warp_many.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(MaskWarpOptions),
                                         C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.dvo_amd_debug_mask_ops_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_default_residual_mask_options.argtypes = [C.POINTER(ResidualMaskOptions)]
    L.dvo_amd_default_residual_mask_options.restype = None
    L.dvo_amd_mask_from_residuals.argtypes = [vp, vp, vp, dp, C.POINTER(ResidualMaskOptions), C.POINTER(vp), C.POINTER(C.c_longlong),
                                              C.POINTER(C.POINTER(C.c_float))]
    L.dvo_amd_mask_from_residuals_many.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(ResidualMaskOptions),
                                                   C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.dvo_amd_default_pose_score_options.argtypes = [C.POINTER(PoseScoreOptions)]
    L.dvo_amd_default_pose_score_options.restype = None
    L.dvo_amd_score_poses.argtypes = [vp, vp, vp, C.c_int, dp, C.POINTER(PoseScoreOptions), vp]
    L.dvo_amd_score_poses_many.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), ip, dp, C.POINTER(PoseScoreOptions), vp]
    L.dvo_amd_rank_poses.argtypes = [vp, C.c_int, C.c_int, ip, ip]
    L.dvo_amd_pose_grid.argtypes = [C.POINTER(PoseGridOptions), dp, dp, C.c_int, ip]
    L.dvo_amd_default_exposure_options.argtypes = [C.POINTER(ExposureOptions)]
    L.dvo_amd_default_exposure_options.restype = None
    L.dvo_amd_estimate_exposure.argtypes = [vp, vp, vp, dp, vp, C.POINTER(ExposureOptions), C.POINTER(ExposureEstimate)]
    L.dvo_amd_estimate_exposure_many.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), dp, C.POINTER(vp),
                                                 C.POINTER(ExposureOptions), C.POINTER(ExposureEstimate)]
    L.dvo_amd_pyramid_adjust_intensity.argtypes = [vp, C.c_double, C.c_double, C.POINTER(vp)]
    L.dvo_amd_pyramid_adjust_intensity_many.argtypes = [C.c_int, C.POINTER(vp), dp, dp, C.POINTER(vp)]
    L.dvo_amd_debug_exposure_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_default_warp_options.argtypes = [C.POINTER(WarpOptions)]
    L.dvo_amd_default_warp_options.restype = None
    ll, wo, cv = C.POINTER(C.c_longlong), C.POINTER(WarpOptions), C.POINTER(CView)
    L.dvo_amd_warp_inverse.argtypes = [vp, vp, dp, C.c_int, wo, fp, fp, ll]
    L.dvo_amd_warp_inverse_many.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), dp, C.c_int, wo, C.POINTER(vp), C.POINTER(vp), ll]
    L.dvo_amd_pyramid_warp_inverse.argtypes = [vp, vp, dp, wo, C.POINTER(vp), ll]
    L.dvo_amd_pyramid_warp_inverse_many.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), dp, wo, C.POINTER(vp), ll]
    L.dvo_amd_warp_forward.argtypes = [vp, dp, cv, C.c_int, wo, fp, fp, ip, ll]
    L.dvo_amd_warp_forward_many.argtypes = [C.c_int, C.POINTER(vp), dp, cv, C.c_int, wo, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), ll]
    L.dvo_amd_pyramid_warp_forward.argtypes = [vp, dp, cv, wo, C.POINTER(vp), ll]
    L.dvo_amd_pyramid_warp_forward_many.argtypes = [C.c_int, C.POINTER(vp), dp, cv, wo, C.POINTER(vp), ll]
    L.dvo_amd_debug_warp_timing.argtypes = [C.c_int, C.c_int, ip, ip, dp]
    vo, ro = C.POINTER(VolumeOptions), C.POINTER(VolumeRaycastOptions)
    L.dvo_amd_default_volume_options.argtypes = [vo]
    L.dvo_amd_default_volume_options.restype = None
    L.dvo_amd_default_volume_raycast_options.argtypes = [ro]
    L.dvo_amd_default_volume_raycast_options.restype = None
    L.dvo_amd_volume_create.argtypes = [C.c_int, vo, C.POINTER(vp)]
    L.dvo_amd_volume_destroy.argtypes = [vp]
    L.dvo_amd_volume_destroy.restype = None
    L.dvo_amd_volume_clear.argtypes = [vp]
    L.dvo_amd_volume_options_get.argtypes = [vp, vo]
    L.dvo_amd_volume_integrate.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int, dp, C.c_int, ll]
    L.dvo_amd_volume_insert.argtypes = [vp, C.c_int, ip, C.POINTER(vp), C.c_int, dp, ll]
    L.dvo_amd_volume_set_poses.argtypes = [vp, C.c_int, ip, dp]
    L.dvo_amd_volume_remove.argtypes = [vp, C.c_int, ip]
    L.dvo_amd_volume_stats.argtypes = [vp, ip, ll]
    L.dvo_amd_volume_download.argtypes = [vp, ip, vp, C.c_longlong, ll]
    L.dvo_amd_volume_raycast.argtypes = [vp, dp, cv, ro, fp, fp, ip, C.POINTER(CVolumeRaycastStats)]
    L.dvo_amd_volume_raycast_pyramid.argtypes = [vp, dp, cv, ro, C.c_int, C.c_double, C.POINTER(vp), C.POINTER(CVolumeRaycastStats)]
    L.dvo_amd_volume_extract.argtypes = [vp, C.c_int, vp, C.c_longlong, ll, C.POINTER(CVolumeExtractCounts)]
    L.dvo_amd_debug_volume_timing.argtypes = [C.c_int, C.c_int, ip, ip, dp]
    L.dvo_amd_volume_mesh.argtypes = [vp, C.c_int, vp, fp, C.c_longlong, ip, C.c_longlong, C.POINTER(CVolumeMeshCounts)]
    L.dvo_amd_volume_upload.argtypes = [vp, ip, vp, C.c_longlong]
    L.dvo_amd_write_ply.argtypes = [C.c_char_p, vp, fp, C.c_longlong, ip, C.c_longlong]
    L.dvo_amd_default_fuse_options.argtypes = [C.POINTER(FuseOptions)]
    L.dvo_amd_default_fuse_options.restype = None
    L.dvo_amd_pyramid_fuse_depth.argtypes = [vp, C.c_int, C.POINTER(vp), dp, C.POINTER(FuseOptions), C.POINTER(vp),
                                             C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)]
    L.dvo_amd_pyramid_fuse_depth_many.argtypes = [C.c_int, C.POINTER(vp), ip, C.POINTER(vp), dp, C.POINTER(FuseOptions), C.POINTER(vp),
                                                  C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(vp)]
    L.dvo_amd_debug_fuse_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_default_depth_filter_options.argtypes = [C.POINTER(DepthFilterOptions)]
    L.dvo_amd_default_depth_filter_options.restype = None
    L.dvo_amd_pyramid_filter_depth.argtypes = [vp, C.POINTER(DepthFilterOptions), C.POINTER(vp), C.POINTER(C.c_longlong),
                                               C.POINTER(C.c_ushort)]
    L.dvo_amd_pyramid_filter_depth_many.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(DepthFilterOptions), C.POINTER(vp),
                                                    C.POINTER(C.c_longlong), C.POINTER(vp)]
    L.dvo_amd_debug_depth_filter_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_default_component_options.argtypes = [C.POINTER(ComponentOptions)]
    L.dvo_amd_default_component_options.restype = None
    L.dvo_amd_mask_filter_components.argtypes = [vp, vp, vp, C.POINTER(ComponentOptions), C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.dvo_amd_mask_filter_components_many.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ComponentOptions),
                                                      C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.dvo_amd_mask_components.argtypes = [vp, vp, vp, C.POINTER(ComponentOptions), C.c_int, ip, vp, C.c_int, ip]
    L.dvo_amd_debug_components_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_default_normal_options.argtypes = [C.POINTER(NormalOptions)]
    L.dvo_amd_default_normal_options.restype = None
    L.dvo_amd_pyramid_normals.argtypes = [vp, C.c_int, C.POINTER(NormalOptions), fp, fp, C.POINTER(C.c_longlong)]
    L.dvo_amd_mask_from_normals.argtypes = [vp, C.POINTER(NormalOptions), fp, C.c_int, C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.dvo_amd_point_cloud_normals.argtypes = [vp, vp, C.c_int, dp, vp, C.c_int, C.POINTER(NormalOptions), vp, fp]
    L.dvo_amd_write_pcd_normals.argtypes = [C.c_char_p, vp, fp, C.c_longlong, C.c_int, C.c_int]
    L.dvo_amd_debug_normals_timing.argtypes = [C.c_int, C.c_int, ip, ip, dp]
    L.dvo_amd_default_place_options.argtypes = [C.POINTER(PlaceOptions)]
    L.dvo_amd_default_place_options.restype = None
    L.dvo_amd_default_place_query_options.argtypes = [C.POINTER(PlaceQueryOptions)]
    L.dvo_amd_default_place_query_options.restype = None
    L.dvo_amd_place_index_create.argtypes = [C.c_int, C.POINTER(PlaceOptions), C.POINTER(vp)]
    L.dvo_amd_place_index_destroy.argtypes = [vp]
    L.dvo_amd_place_index_destroy.restype = None
    L.dvo_amd_place_index_add.argtypes = [vp, C.c_int, C.POINTER(vp), ip]
    L.dvo_amd_place_index_info.argtypes = [vp, ip, ip, ip, ip]
    L.dvo_amd_place_index_download.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_byte), ip]
    L.dvo_amd_place_scores.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int, ip]
    L.dvo_amd_place_query.argtypes = [vp, C.c_int, ip, C.POINTER(PlaceQueryOptions), ip, dp, ip]
    L.dvo_amd_place_query_frames.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(PlaceQueryOptions), ip, dp, ip]
    L.dvo_amd_debug_place_timing.argtypes = [C.c_int, C.c_int, dp]
    L.dvo_amd_se3_exp.argtypes = [dp, dp]
    L.dvo_amd_se3_exp.restype = None
    L.dvo_amd_se3_log.argtypes = [dp, dp]
    L.dvo_amd_se3_log.restype = None
    L.dvo_amd_solve6.argtypes = [dp, dp, dp]
    L.dvo_amd_solve6.restype = None
    _lib = L
    return L


def build_id() -> str:
    """the hash of the sources and flags the loaded library was built from (dvo_amd_build_id)"""
    return lib().dvo_amd_build_id().decode()


def _check(status: int, where: str):
    if status != 0:
        raise DvoAmdError(status, where)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _pose_cm(pose):
    """a 4x4 pose (row-major numpy, as everywhere in this binding) as the column-major doubles of the C ABI"""
    return np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(4, 4).T)


def _split_points(points):
    """dvo_amd_point records (n x 4 words) -> (xyz float32 [n, 3], rgb uint32 [n])"""
    return points[:, :3].copy(), points[:, 3].view(np.uint32).copy()


def _pack_points(xyz, rgb):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, dtype=np.uint32).reshape(-1)
    if len(rgb) != len(xyz):
        raise ValueError("xyz and rgb must hold the same number of points")
    pts = np.empty((len(xyz), 4), np.float32)
    pts[:, :3] = xyz
    pts[:, 3] = rgb.view(np.float32)
    return pts


_cloud_trackers = {}


def _cloud_tracker(device: int):
    """the context RgbdImagePyramid.point_cloud runs in when no tracker is passed: one DenseTracker per device, created on first
    use and kept (with its point-cloud buffers) for the life of the process"""
    if device not in _cloud_trackers:
        _cloud_trackers[device] = DenseTracker(device=device)
    return _cloud_trackers[device]


class Config:
    """DenseTracker::Config (live fields), defaults from dense_tracking_config.cpp:27-41."""

    def __init__(self, **kw):
        c = CConfig()
        lib().dvo_amd_default_config(C.byref(c))
        self.FirstLevel = c.first_level
        self.LastLevel = c.last_level
        self.MaxIterationsPerLevel = c.max_iterations_per_level
        self.Precision = c.precision
        self.Mu = c.mu
        self.UseInitialEstimate = bool(c.use_initial_estimate)
        self.IntensityDerivativeThreshold = c.intensity_derivative_threshold
        self.DepthDerivativeThreshold = c.depth_derivative_threshold
        # not a field of the reference: how a level is cut into wave segments (dvo_amd.h: dvo_amd_config::segment_geometry);
        # GEOMETRY_THROUGHPUT (default) or GEOMETRY_LATENCY (the shortest single match())
        self.SegmentGeometry = c.segment_geometry
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def getNumLevels(self) -> int:
        return self.FirstLevel + 1

    def IsSane(self) -> bool:
        return self.FirstLevel >= self.LastLevel

    def _c(self) -> CConfig:
        return CConfig(self.FirstLevel, self.LastLevel, self.MaxIterationsPerLevel, self.Precision, self.Mu,
                       int(self.UseInitialEstimate), self.IntensityDerivativeThreshold, self.DepthDerivativeThreshold,
                       int(self.SegmentGeometry), 0)


class Remap:
    """A dvo_amd_remap: the device-resident table pair through which `RgbdImagePyramid.from_raw(..., remap=)` resamples a raw
    frame (what image_proc's cv::initUndistortRectifyMap + cv::remap do on the CPU in front of the reference).  Immutable,
    shareable between trackers and threads; the rules are pinned in include/dvo_amd.h."""

    def __init__(self):
        raise TypeError("use Remap.from_maps or Remap.undistort")

    @classmethod
    def from_maps(cls, map_x, map_y, src_size, device: int = 0):
        """map_x, map_y: float32 [h, w] source positions of every output pixel (cv::remap's CV_32FC1 pair); src_size = (width,
        height) of the source image they refer to."""
        map_x = np.ascontiguousarray(map_x, dtype=np.float32)
        map_y = np.ascontiguousarray(map_y, dtype=np.float32)
        if map_x.shape != map_y.shape or map_x.ndim != 2:
            raise ValueError("map_x and map_y must be 2-D arrays of the same shape")
        h, w = map_x.shape
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _check(lib().dvo_amd_remap_create(device, w, h, _fp(map_x), _fp(map_y), w, int(src_size[0]), int(src_size[1]),
                                          C.byref(self._h)), "dvo_amd_remap_create")
        self.device = device
        return self

    @classmethod
    def undistort(cls, size, K_out, src_size, K_src, dist, device: int = 0):
        """The map of the five-coefficient lens model, computed on the device: size = (width, height) and K_out = (fx, fy, ox, oy)
        of the rectified camera, src_size and K_src of the real one, dist = (k1, k2, p1, p2, k3) in OpenCV's order."""
        k_out = np.ascontiguousarray(K_out, dtype=np.float32).reshape(4)
        k_src = np.ascontiguousarray(K_src, dtype=np.float32).reshape(4)
        d = np.ascontiguousarray(dist, dtype=np.float32).reshape(5)
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _check(lib().dvo_amd_remap_create_undistort(device, int(size[0]), int(size[1]), _fp(k_out), int(src_size[0]),
                                                    int(src_size[1]), _fp(k_src), _fp(d), C.byref(self._h)),
               "dvo_amd_remap_create_undistort")
        self.device = device
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dvo_amd_remap_release(h)
            self._h = None

    def info(self) -> dict:
        """{"width", "height", "src_width", "src_height", "n_inside"}: n_inside = output pixels whose source position lies
        inside the source (the others become 0 / NaN)"""
        v = [C.c_int() for _ in range(5)]
        _check(lib().dvo_amd_remap_info(self._h, *[C.byref(x) for x in v]), "dvo_amd_remap_info")
        return dict(zip(("width", "height", "src_width", "src_height", "n_inside"), (x.value for x in v)))

    def download(self):
        """(map_x, map_y), float32 [h, w] each"""
        i = self.info()
        mx, my = np.empty((i["height"], i["width"]), np.float32), np.empty((i["height"], i["width"]), np.float32)
        _check(lib().dvo_amd_remap_download(self._h, _fp(mx), _fp(my)), "dvo_amd_remap_download")
        return mx, my


def _mask_bytes(a):
    """a mask plane as contiguous uint8 (bytes as they are: the library normalises; anything else by != 0)"""
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype == np.uint8 else a != 0, dtype=np.uint8)


MASK_ALL, MASK_ANY = 0, 1
MAX_MASKED_SELECTIONS = 8
BUDGET_TOPK, BUDGET_GRID = 0, 1
MASK_AND, MASK_OR, MASK_ANDNOT, MASK_NOT = 0, 1, 2, 3
MASK_DILATE, MASK_ERODE = 0, 1
MASK_MAX_RADIUS = 64


def level_budgets(k0: int, levels: int, minimum: int = 0) -> list:
    """A level-0 point budget as per-level budgets for SelectionMask.from_budget: level l has a quarter of the pixels of level
    l - 1, so it gets max(minimum, k0 >> 2l)."""
    return [max(int(minimum), int(k0) >> (2 * l)) for l in range(levels)]


def level_radii(r0: int, levels: int) -> list:
    """A radius in pixels of level 0 as per-level radii for SelectionMask.dilate / erode: level l has half the resolution of
    level l - 1, so it gets r0 / 2^l rounded up, (r0 + (1 << l) - 1) >> l."""
    return [(int(r0) + (1 << l) - 1) >> l for l in range(levels)]


def mask_warp_options(**options) -> MaskWarpOptions:
    """dvo_amd_default_mask_warp_options (near_z 0.1, depth_sigmas 20, unseen_keep 1, inconsistent_keep 1) with the given fields
    replaced"""
    opt = MaskWarpOptions()
    lib().dvo_amd_default_mask_warp_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("near_z", "depth_sigmas", "unseen_keep", "inconsistent_keep"):
            raise TypeError(f"unknown mask warp option {k!r}")
        setattr(opt, k, int(v) if k.endswith("_keep") else float(v))
    return opt


def residual_mask_options(result=None, levels: int = MAX_LEVELS, max_distance=RESIDUAL_MASK_MAX_DISTANCE, **keeps) -> ResidualMaskOptions:
    """dvo_amd_default_residual_mask_options (max_distance 9.2103 on every level, both keeps 0) with precision[l] filled from a
    `Result` for l < levels: the TDistributionPrecision of the last iteration of level l.  A level the match did not run (level 0
    under the default configuration) takes the precision of the nearest level that ran, ties to the finer one.  ValueError if the
    result holds no iteration statistics.  result=None leaves the precisions unset (the library refuses them).  max_distance: one
    value for every level, or one per level; keeps: invalid_keep, unevaluated_keep."""
    opt = ResidualMaskOptions()
    lib().dvo_amd_default_residual_mask_options(C.byref(opt))
    if not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"levels must be 1..{MAX_LEVELS}")
    dist = [float(v) for v in max_distance] if hasattr(max_distance, "__len__") else [float(max_distance)] * MAX_LEVELS
    if len(dist) > MAX_LEVELS:
        raise ValueError(f"max_distance: more than {MAX_LEVELS} levels")
    for l, v in enumerate(dist):
        opt.max_distance[l] = v
    for k, v in keeps.items():
        if k not in ("invalid_keep", "unevaluated_keep"):
            raise TypeError(f"unknown residual mask option {k!r}")
        setattr(opt, k, int(v))
    if result is not None:
        ran = {int(L["Id"]): L["Iterations"][-1]["TDistributionPrecision"] for L in result.Levels if L["Iterations"]}
        if not ran:
            raise ValueError("the result holds no iteration statistics (match with stats=True)")
        for l in range(int(levels)):
            nearest = min(ran, key=lambda have: (abs(have - l), have))
            P = np.asarray(ran[nearest], np.float64)
            opt.precision[l][:] = [P[0, 0], P[1, 0], P[0, 1], P[1, 1]]  # column-major
    return opt


def pose_score_options(level: int, precision=None, result=None, max_distance=None, invalid_distance=None) -> PoseScoreOptions:
    """dvo_amd_default_pose_score_options (max_distance 9.2103, invalid_distance = max_distance) for `level`.  precision: a 2x2
    matrix, or four floats column-major.  With result= and no precision the level takes its precision from a `Result` as
    residual_mask_options does: the TDistributionPrecision of the last iteration of the nearest level that ran.  Neither leaves
    it unset (the library refuses that)."""
    opt = PoseScoreOptions()
    lib().dvo_amd_default_pose_score_options(C.byref(opt))
    opt.level = int(level)
    if precision is not None:
        P = np.asarray(precision, np.float64)
        opt.precision[:] = [P[0, 0], P[1, 0], P[0, 1], P[1, 1]] if P.shape == (2, 2) else [float(v) for v in P.ravel()]
    elif result is not None:
        if not 0 <= int(level) < MAX_LEVELS:
            raise ValueError(f"level must be 0..{MAX_LEVELS - 1}")
        opt.precision[:] = list(residual_mask_options(result, int(level) + 1).precision[int(level)])
    if max_distance is not None:
        opt.max_distance = float(max_distance)
    if invalid_distance is not None:
        opt.invalid_distance = float(invalid_distance)
    return opt


def pose_grid(T_centre=None, **axes) -> np.ndarray:
    """The hypotheses Exp(xi) * T_centre of a grid over xi = (vx, vy, vz, wx, wy, wz) (dvo_amd_pose_grid), as an array [n, 4, 4]
    of row-major 4x4 matrices.  axes: vx=(count, step), ...: count odd, the values (-(count - 1) / 2 ... (count - 1) / 2) * step; an
    axis not given has the one value 0.  wz runs fastest, vx slowest; the middle entry is T_centre itself, bit for bit."""
    opt = PoseGridOptions()
    for a, name in enumerate(POSE_GRID_AXES):
        opt.count[a], opt.step[a] = 1, 0.0
    for name, (count, step) in axes.items():
        if name not in POSE_GRID_AXES:
            raise TypeError(f"unknown grid axis {name!r}")
        a = POSE_GRID_AXES.index(name)
        opt.count[a], opt.step[a] = int(count), float(step)
    Tc = _pose_cm(np.eye(4) if T_centre is None else T_centre)
    dp = C.POINTER(C.c_double)
    n = C.c_int()
    _check(lib().dvo_amd_pose_grid(C.byref(opt), Tc.ctypes.data_as(dp), None, 0, C.byref(n)), "dvo_amd_pose_grid")
    out = np.empty((n.value, 4, 4), np.float64)
    _check(lib().dvo_amd_pose_grid(C.byref(opt), Tc.ctypes.data_as(dp), out.ctypes.data_as(dp), n.value, C.byref(n)), "dvo_amd_pose_grid")
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def rank_poses(scores, k: int) -> np.ndarray:
    """The indices of the min(k, len(scores)) records of smallest total, smallest first, ties to the lower index
    (dvo_amd_rank_poses; host-only)."""
    scores = np.ascontiguousarray(scores, POSE_SCORE_DTYPE)
    order = np.zeros(max(1, min(int(k), len(scores))), np.int32)
    n = C.c_int()
    _check(lib().dvo_amd_rank_poses(scores.ctypes.data_as(C.c_void_p), len(scores), int(k), order.ctypes.data_as(C.POINTER(C.c_int)),
                                    C.byref(n)), "dvo_amd_rank_poses")
    return order[:n.value].copy()


def rigid_inverse(T) -> np.ndarray:
    """inv(T) of a rigid 4x4 transformation as (R^T, -R^T t), every sum in a fixed order: the same sixteen doubles as
    dvo::core::SelectionMask::rigidInverse and examples/residual_mask_example.c form"""
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return out


def level_areas(a0: int, levels: int) -> list:
    """An area in pixels of level 0 as per-level areas for SelectionMask.filter_components: level l has a quarter of the pixels of
    level l - 1, so it gets max(1, ceil(a0 / 4^l))."""
    return [max(1, -(-int(a0) // 4 ** l)) for l in range(levels)]


def component_options(**options) -> ComponentOptions:
    """dvo_amd_default_component_options (connectivity 8, max_step 0, depth_sigmas 10, every min_area 0, every max_area -1,
    keep_largest 0) with the given fields replaced.  min_area / max_area: one value for every level, or one per level."""
    opt = ComponentOptions()
    lib().dvo_amd_default_component_options(C.byref(opt))
    for k, v in options.items():
        if k in ("min_area", "max_area"):
            per_level = [int(a) for a in v] if hasattr(v, "__len__") else [int(v)] * MAX_LEVELS
            if len(per_level) > MAX_LEVELS:
                raise ValueError(f"{k}: more than {MAX_LEVELS} levels")
            for l, a in enumerate(per_level):
                getattr(opt, k)[l] = a
        elif k in ("connectivity", "keep_largest"):
            setattr(opt, k, int(v))
        elif k in ("max_step", "depth_sigmas"):
            setattr(opt, k, float(v))
        else:
            raise TypeError(f"unknown component option {k!r}")
    return opt


def _component_options(options, fields) -> ComponentOptions:
    if options is not None and fields:
        raise TypeError("give options= or option fields, not both")
    return options if options is not None else component_options(**fields)


def components_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event bracket around every component call (filter_components, filter_components_many,
    components) of `device` on or off and returns the device time of the most recent bracketed call in ms
    (dvo_amd_debug_components_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_components_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_components_timing")
    return ms.value


def mask_ops_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event bracket around every mask operation (combine, dilate / erode, warp) of `device` on or
    off and returns the device time of the most recent bracketed call in ms (dvo_amd_debug_mask_ops_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_mask_ops_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_mask_ops_timing")
    return ms.value


def fuse_options(**options) -> FuseOptions:
    """dvo_amd_default_fuse_options (near_z 0.1, depth_sigmas 5, min_cos 0.5, sample FUSE_BILINEAR, min_observations 0,
    drop_unconfirmed 0) with the given fields replaced"""
    opt = FuseOptions()
    lib().dvo_amd_default_fuse_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("near_z", "depth_sigmas", "min_cos", "sample", "min_observations", "drop_unconfirmed"):
            raise TypeError(f"unknown fuse option {k!r}")
        setattr(opt, k, float(v) if k in ("near_z", "depth_sigmas", "min_cos") else int(v))
    return opt


def depth_filter_options(**options) -> DepthFilterOptions:
    """dvo_amd_default_depth_filter_options (radius 2, range_sigmas 3, min_support 1, fill_radius 0, min_fill_support 3) with the
    given fields replaced"""
    opt = DepthFilterOptions()
    lib().dvo_amd_default_depth_filter_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("radius", "range_sigmas", "min_support", "fill_radius", "min_fill_support"):
            raise TypeError(f"unknown depth filter option {k!r}")
        setattr(opt, k, float(v) if k == "range_sigmas" else int(v))
    return opt


def filter_depth_many(pyramids, options=None, counts: bool = False, support: bool = False):
    """Many pyramids' level-0 depth filtered in one call and one kernel launch (dvo_amd_pyramid_filter_depth_many; the rule is
    pinned in include/dvo_amd.h under "Depth filtering"); the pyramids may differ in size.  options: None, a DepthFilterOptions
    or a dict of its fields (radius, range_sigmas, min_support, fill_radius, min_fill_support).  Returns the list of new pyramids;
    with counts=True also the counts (a DEPTH_FILTER_DTYPE array, one record per pyramid); with support=True also the list of
    support planes (uint16 [h, w]: the members of every pixel's window) -- as a tuple, in this order."""
    pyramids = list(pyramids)
    n = len(pyramids)
    opt = options if isinstance(options, DepthFilterOptions) else depth_filter_options(**(options or {}))
    vp = C.c_void_p
    cnt = np.zeros(max(1, n), DEPTH_FILTER_DTYPE)
    planes = []
    if support:
        for p in pyramids:
            w, h, _ = p.level_info(0)
            planes.append(np.zeros((h, w), np.uint16))
    out = (vp * max(1, n))()
    sup = (vp * max(1, n))(*[p.ctypes.data for p in planes]) if support else None
    _check(lib().dvo_amd_pyramid_filter_depth_many(n, (vp * max(1, n))(*[p._h for p in pyramids]), C.byref(opt), out,
                                                   cnt.ctypes.data_as(C.POINTER(C.c_longlong)) if counts else None, sup),
           "dvo_amd_pyramid_filter_depth_many")
    made = []
    for j in range(n):
        p = RgbdImagePyramid.__new__(RgbdImagePyramid)
        p._h, p.device, p.registration_stats = vp(out[j]), pyramids[j].device, None
        made.append(p)
    result = (made,)
    if counts:
        result += (cnt[:n].copy(),)
    if support:
        result += (planes,)
    return result if len(result) > 1 else made


def exposure_options(**options) -> ExposureOptions:
    """dvo_amd_default_exposure_options (level 0, near_z 0.1, depth_sigmas 20, intensities 4..251, scale 16, trim 12, refits 4,
    min_pairs 64, gains 0.25..4) with the given fields replaced"""
    opt = ExposureOptions()
    lib().dvo_amd_default_exposure_options(C.byref(opt))
    for k, v in options.items():
        if k in ("level", "refits", "min_pairs"):
            setattr(opt, k, int(v))
        elif k in ("near_z", "depth_sigmas", "min_intensity", "max_intensity", "scale", "trim", "min_gain", "max_gain"):
            setattr(opt, k, float(v))
        else:
            raise TypeError(f"unknown exposure option {k!r}")
    return opt


def _exposure_options(options) -> ExposureOptions:
    return options if isinstance(options, ExposureOptions) else exposure_options(**(options or {}))


def estimate_exposure_many(tracker, references, currents, Ts=None, masks=None, options=None) -> list:
    """n pairs in one call of refits_max + 1 kernel launches (dvo_amd_estimate_exposure_many): pair k fits I_ref ~ gain * I_cur +
    bias between references[k] and currents[k] at the level its options name.  Ts: None (the identity for every pair) or one 4x4
    per pair, reference -> current, the estimate; masks: None, or one SelectionMask or None per pair, on the reference's pixels;
    options: None, one ExposureOptions / dict for all pairs, or a list of one per pair.  Returns [ExposureEstimate]."""
    references, currents = list(references), list(currents)
    n = len(references)
    per_pair = list(options) if isinstance(options, (list, tuple)) else [options] * n
    if len(currents) != n or len(per_pair) != n or (Ts is not None and len(Ts) != n) or (masks is not None and len(masks) != n):
        raise ValueError("one current, one option set and (where given) one transformation and one mask per reference")
    vp = C.c_void_p
    opts = (ExposureOptions * max(1, n))(*[_exposure_options(o) for o in per_pair])
    T = None if Ts is None else np.ascontiguousarray(np.asarray(Ts, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
    out = (ExposureEstimate * max(1, n))()
    _check(lib().dvo_amd_estimate_exposure_many(tracker._h, n, (vp * max(1, n))(*[p._h for p in references]),
                                                (vp * max(1, n))(*[p._h for p in currents]),
                                                None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)),
                                                None if masks is None else (vp * max(1, n))(*[None if m is None else m._h for m in masks]),
                                                opts, out), "dvo_amd_estimate_exposure_many")
    return [ExposureEstimate.from_buffer_copy(out[k]) for k in range(n)]


def adjust_intensity_many(pyramids, gains, biases) -> list:
    """Many pyramids' level-0 intensity mapped to (gains[k] * I) + biases[k] in one call and one kernel launch
    (dvo_amd_pyramid_adjust_intensity_many); the pyramids may differ in size.  Returns the list of new pyramids."""
    pyramids = list(pyramids)
    n = len(pyramids)
    g, b = np.ascontiguousarray(gains, np.float64).ravel(), np.ascontiguousarray(biases, np.float64).ravel()
    if len(g) != n or len(b) != n:
        raise ValueError("one gain and one bias per pyramid")
    g, b = np.concatenate([g, [1.0]]), np.concatenate([b, [0.0]])  # (never an empty buffer)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    out = (vp * max(1, n))()
    _check(lib().dvo_amd_pyramid_adjust_intensity_many(n, (vp * max(1, n))(*[p._h for p in pyramids]), g.ctypes.data_as(dp),
                                                       b.ctypes.data_as(dp), out), "dvo_amd_pyramid_adjust_intensity_many")
    made = []
    for j in range(n):
        p = RgbdImagePyramid.__new__(RgbdImagePyramid)
        p._h, p.device, p.registration_stats = vp(out[j]), pyramids[j].device, None
        made.append(p)
    return made


def exposure_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event brackets around the launches of every estimate_exposure / adjust_intensity call of
    `device` on or off and returns the device time of the most recent bracketed call in ms, its launches added up
    (dvo_amd_debug_exposure_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_exposure_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_exposure_timing")
    return ms.value


def depth_filter_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event bracket around the filter launch of every filter_depth / filter_depth_many of `device`
    on or off and returns the device time of the most recent bracketed launch in ms (dvo_amd_debug_depth_filter_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_depth_filter_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_depth_filter_timing")
    return ms.value


def normal_options(radius=None, depth_step_ratio: float | None = None, facing: int | None = None,
                   toward_camera: int | None = None) -> NormalOptions:
    """dvo_amd_default_normal_options (everything 0: RgbdImage::calculateNormals) with the given fields replaced.  radius: one
    window radius per level, or one value for every level (0..NORMAL_MAX_RADIUS); depth_step_ratio: a window member is summed
    only within this fraction of the centre's depth (0: no test); facing: NORMAL_FACING_AXIS or NORMAL_FACING_RAY"""
    opt = NormalOptions()
    lib().dvo_amd_default_normal_options(C.byref(opt))
    if radius is not None:
        opt.radius[:] = _per_level(radius, 0, "radius")
    if depth_step_ratio is not None:
        opt.depth_step_ratio = float(depth_step_ratio)
    if facing is not None:
        opt.facing = int(facing)
    if toward_camera is not None:
        opt.toward_camera = int(toward_camera)
    return opt


def _normal_options(options) -> NormalOptions:
    return options if isinstance(options, NormalOptions) else normal_options(**(options or {}))


def normals_timing(enable: bool = True, device: int = 0) -> dict:
    """(instrumentation) what the most recent normals call of `device` enqueued -- kernel launches, host synchronisations -- and,
    once switched on, the device time of its launch in ms (dvo_amd_debug_normals_timing)"""
    launches, syncs, ms = C.c_int(), C.c_int(), C.c_double()
    _check(lib().dvo_amd_debug_normals_timing(device, int(enable), C.byref(launches), C.byref(syncs), C.byref(ms)),
           "dvo_amd_debug_normals_timing")
    return {"launches": launches.value, "synchronisations": syncs.value, "ms": ms.value}


def fuse_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event bracket around the fusion launch of every fuse_depth / fuse_depth_many of `device` on
    or off and returns the device time of the most recent bracketed launch in ms (dvo_amd_debug_fuse_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_fuse_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_fuse_timing")
    return ms.value


def warp_options(**options) -> WarpOptions:
    """dvo_amd_default_warp_options (near_z 0.1, occlusion_margin 0.05, depth WARP_DEPTH_TRANSFORMED, splat WARP_SPLAT_NEAREST,
    fill_intensity 0) with the given fields replaced"""
    opt = WarpOptions()
    lib().dvo_amd_default_warp_options(C.byref(opt))
    for k, v in options.items():
        if k not in dict(WarpOptions._fields_):
            raise TypeError(f"unknown warp option {k!r}")
        setattr(opt, k, v)
    return opt


def _warp_options(options) -> WarpOptions:
    return options if isinstance(options, WarpOptions) else warp_options(**(options or {}))


def warp_timing(enable: bool = True, device: int = 0) -> dict:
    """(instrumentation) switches the event bracket around the launches of every warp_inverse / warp_forward of `device` on or
    off; returns what the most recent such call enqueued of its own (`launches`, `synchronisations`) and the device time of the
    most recent bracketed call in ms (`ms`) (dvo_amd_debug_warp_timing)"""
    n, s, ms = C.c_int(), C.c_int(), C.c_double()
    _check(lib().dvo_amd_debug_warp_timing(device, int(enable), C.byref(n), C.byref(s), C.byref(ms)), "dvo_amd_debug_warp_timing")
    return dict(launches=n.value, synchronisations=s.value, ms=ms.value)


def _warp_poses(Ts, n):
    if len(Ts) != n:
        raise ValueError("one transformation per item")
    return np.ascontiguousarray(np.stack([_pose_cm(t) for t in Ts]) if n else np.zeros((1, 4, 4)), dtype=np.float64)


def _wrap_pyramids(handles, like):
    made = []
    for h, src in zip(handles, like):
        p = RgbdImagePyramid.__new__(RgbdImagePyramid)
        p._h, p.device, p.registration_stats = C.c_void_p(h), src.device, None
        made.append(p)
    return made


def warp_inverse_many(fixed, moving, Ts, level=None, options=None):
    """n inverse warps in one call and one kernel launch (dvo_amd_warp_inverse_many / dvo_amd_pyramid_warp_inverse_many; the rule
    is pinned in include/dvo_amd.h under "Frame warps"): the grey values of moving[k] on the pixels of fixed[k].  Ts[k]: 4x4,
    maps points of moving[k]'s camera into fixed[k]'s: for tracker.match(fixed[k], moving[k]) the result's Transformation as
    returned.  options: None, a WarpOptions or a dict of its fields.  With a level: (intensity planes, depth planes, counts) --
    two lists of float32 [h, w] of the fixed level's size and a WARP_INVERSE_DTYPE array.  With level=None: (pyramids, counts),
    each pyramid with fixed[k]'s size, intrinsics, level count and timestamp."""
    n = len(fixed)
    if len(moving) != n:
        raise ValueError("one moving pyramid per fixed pyramid")
    opt, T = _warp_options(options), _warp_poses(Ts, n)
    vp, ll = C.c_void_p, C.POINTER(C.c_longlong)
    cnt = np.zeros(max(1, n), WARP_INVERSE_DTYPE)
    fh, mh = (vp * max(1, n))(*[p._h for p in fixed]), (vp * max(1, n))(*[p._h for p in moving])
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    if level is None:
        out = (vp * max(1, n))()
        _check(lib().dvo_amd_pyramid_warp_inverse_many(n, fh, mh, Tp, C.byref(opt), out, cnt.ctypes.data_as(ll)),
               "dvo_amd_pyramid_warp_inverse_many")
        return _wrap_pyramids(out[:n], fixed), cnt[:n].copy()
    sizes = [p.level_info(level)[:2] if 0 <= level < p.levels() else (0, 0) for p in fixed]  # (the library refuses a bad level)
    I = [np.empty((h, w), np.float32) for w, h in sizes]
    Z = [np.empty((h, w), np.float32) for w, h in sizes]
    _check(lib().dvo_amd_warp_inverse_many(n, fh, mh, Tp, level, C.byref(opt), (vp * max(1, n))(*[a.ctypes.data for a in I]),
                                           (vp * max(1, n))(*[a.ctypes.data for a in Z]), cnt.ctypes.data_as(ll)),
           "dvo_amd_warp_inverse_many")
    return I, Z, cnt[:n].copy()


def _warp_view(view, near_z) -> CView:
    """a view as (K, width, height) or (K, width, height, near_z), or a CView"""
    if isinstance(view, CView):
        return view
    K, width, height = view[:3]
    fx, fy, ox, oy = [float(k) for k in K]
    return CView(int(width), int(height), fx, fy, ox, oy, float(view[3]) if len(view) > 3 else float(near_z))


def warp_forward_many(moving, Ts, views=None, level=None, options=None):
    """n forward warps in one call and three kernel launches (dvo_amd_warp_forward_many / dvo_amd_pyramid_warp_forward_many):
    every pixel of moving[k] drawn into a view with a nearest-depth test.  Ts[k] as for warp_inverse_many.  views: None (the
    moving level's own camera), or one (K, width, height[, near_z]) or CView per item; near_z defaults to the options'.  With a
    level: (depth planes, intensity planes, index planes, counts) -- float32, float32 and int32 [h, w] of the view's size and a
    WARP_FORWARD_DTYPE array.  With level=None: (pyramids, counts), each pyramid with the view's size and intrinsics and
    moving[k]'s level count and timestamp."""
    n = len(moving)
    opt, T = _warp_options(options), _warp_poses(Ts, n)
    if views is not None and len(views) != n:
        raise ValueError("one view per item")
    vp, ll = C.c_void_p, C.POINTER(C.c_longlong)
    cnt = np.zeros(max(1, n), WARP_FORWARD_DTYPE)
    mh = (vp * max(1, n))(*[p._h for p in moving])
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    cviews = None if views is None else (CView * max(1, n))(*[_warp_view(v, opt.near_z) for v in views])
    if level is None:
        out = (vp * max(1, n))()
        _check(lib().dvo_amd_pyramid_warp_forward_many(n, mh, Tp, cviews, C.byref(opt), out, cnt.ctypes.data_as(ll)),
               "dvo_amd_pyramid_warp_forward_many")
        return _wrap_pyramids(out[:n], moving), cnt[:n].copy()
    if cviews is None:
        sizes = [p.level_info(level)[:2] if 0 <= level < p.levels() else (0, 0) for p in moving]  # (the library refuses a bad level)
    else:
        sizes = [(max(0, cviews[k].width), max(0, cviews[k].height)) for k in range(n)]
    Z = [np.empty((h, w), np.float32) for w, h in sizes]
    I = [np.empty((h, w), np.float32) for w, h in sizes]
    X = [np.empty((h, w), np.int32) for w, h in sizes]
    ptrs = [(vp * max(1, n))(*[a.ctypes.data for a in planes]) for planes in (Z, I, X)]
    _check(lib().dvo_amd_warp_forward_many(n, mh, Tp, cviews, level, C.byref(opt), ptrs[0], ptrs[1], ptrs[2], cnt.ctypes.data_as(ll)),
           "dvo_amd_warp_forward_many")
    return Z, I, X, cnt[:n].copy()


def _per_level(value, default, what):
    """one entry per level from a scalar (every level) or a sequence (level l = value[l]); the rest keeps the default"""
    out = [default] * MAX_LEVELS
    if value is None:
        return out
    vals = [int(v) for v in value] if hasattr(value, "__len__") else [int(value)] * MAX_LEVELS
    if len(vals) > MAX_LEVELS:
        raise ValueError(f"{what}: more than {MAX_LEVELS} levels")
    out[:len(vals)] = vals
    return out


class SelectionMask:
    """A dvo_amd_mask: which reference pixels may take part in an alignment, as a device-resident pyramid of byte planes (1 = keep,
    0 = drop) -- the device form of a user-defined PointSelectionPredicate.  `RgbdImagePyramid.select(..., mask=)`,
    `DenseTracker.match(..., mask=)` and `DenseTracker.match_batch(..., masks=)` take one.  Immutable, shareable between trackers
    and threads; a selection built behind it outlives it.  The rules are pinned in include/dvo_amd.h."""

    def __init__(self):
        raise TypeError("use SelectionMask.from_level0, SelectionMask.from_levels or SelectionMask.from_budget")

    @classmethod
    def from_level0(cls, mask0, levels: int, rule: int = MASK_ALL, device: int = 0):
        """mask0: [h, w] bytes or bools of level 0 (non-zero = keep); levels 1..levels-1 are derived on the device, a pixel kept iff
        all (MASK_ALL) or any (MASK_ANY) of the four pixels under it are kept."""
        m = _mask_bytes(mask0)
        if m.ndim != 2:
            raise ValueError("mask0 must be a 2-D array")
        h, w = m.shape
        return cls._level0(m.ctypes.data, w, h, w, levels, rule, 0, device)

    @classmethod
    def from_level0_device(cls, d_mask0: int, width: int, height: int, levels: int, rule: int = MASK_ALL, device: int = 0,
                           stride: int | None = None):
        """As from_level0, for a byte plane already resident in HBM (a raw device pointer, e.g. torch.Tensor.data_ptr() of a
        segmentation network's uint8 output)."""
        return cls._level0(d_mask0, width, height, width if stride is None else stride, levels, rule, 1, device)

    @classmethod
    def _level0(cls, ptr, w, h, stride, levels, rule, on_device, device):
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _check(lib().dvo_amd_mask_create(device, w, h, levels, C.c_void_p(ptr), stride, on_device, int(rule), C.byref(self._h)),
               "dvo_amd_mask_create")
        self.device = device
        return self

    @classmethod
    def from_levels(cls, planes, device: int = 0):
        """planes: one [h >> l, w >> l] array of bytes or bools per level, every level given (what a per-level predicate needs)"""
        ps = [_mask_bytes(p) for p in planes]
        if not ps or any(p.ndim != 2 for p in ps):
            raise ValueError("one 2-D array per level")
        h, w = ps[0].shape
        n = len(ps)
        ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in ps])
        strides = (C.c_int * n)(*[p.shape[1] for p in ps])
        for l, p in enumerate(ps):
            if p.shape != (h >> l, w >> l):
                raise ValueError(f"level {l} must be {(h >> l, w >> l)}, not {p.shape}")
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _check(lib().dvo_amd_mask_create_levels(device, w, h, n, ptrs, strides, 0, C.byref(self._h)), "dvo_amd_mask_create_levels")
        self.device = device
        return self

    @classmethod
    def from_budget(cls, pyramid, rule: int = BUDGET_TOPK, budget=None, cell=None, thresholds=(0.0, 0.0), depth_weight: float = 0.0,
                    within: "SelectionMask | None" = None):
        """A point budget over the levels of `pyramid` (an RgbdImagePyramid), ranked on the device (dvo_amd_mask_create_budget).
        BUDGET_TOPK: level l keeps its budget[l] strongest candidates (None or negative: every candidate; `level_budgets` makes
        the list from a level-0 budget).  BUDGET_GRID: level l keeps the strongest candidate of every cell[l] x cell[l] cell.
        budget / cell: one value per level, or one value for every level.  A candidate passes the threshold predicate of
        `thresholds` = (intensity, depth) and, if given, the mask `within`; strength is Ix^2 + Iy^2 + depth_weight * (Zx^2 + Zy^2),
        ties go to the lowest pixel index.  The rules are pinned in include/dvo_amd.h."""
        opt = BudgetOptions()
        lib().dvo_amd_default_budget_options(C.byref(opt))
        opt.rule = int(rule)
        opt.budget[:] = _per_level(budget, -1, "budget")
        opt.cell[:] = _per_level(cell, 1, "cell")
        opt.intensity_threshold, opt.depth_threshold = float(thresholds[0]), float(thresholds[1])
        opt.depth_weight = float(depth_weight)
        opt.within = None if within is None else within._h
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _check(lib().dvo_amd_mask_create_budget(pyramid._h, C.byref(opt), C.byref(self._h)), "dvo_amd_mask_create_budget")
        self.device = pyramid.device
        return self

    # ---- masks from masks, on the device (the rules are pinned in include/dvo_amd.h under "Mask operations")

    @classmethod
    def _own(cls, handle, device):
        self = cls.__new__(cls)
        self._h, self.device = handle, device
        return self

    def _combine(self, other, op):
        if other is not None and not isinstance(other, SelectionMask):
            return NotImplemented
        out = C.c_void_p()
        _check(lib().dvo_amd_mask_combine(self._h, None if other is None else other._h, op, C.byref(out)), "dvo_amd_mask_combine")
        return SelectionMask._own(out, self.device)

    def __and__(self, other):
        """kept where both keep, level by level (dvo_amd_mask_combine)"""
        return self._combine(other, MASK_AND)

    def __or__(self, other):
        """kept where either keeps"""
        return self._combine(other, MASK_OR)

    def __invert__(self):
        """kept where this mask drops"""
        return self._combine(None, MASK_NOT)

    def andnot(self, other):
        """kept where this mask keeps and `other` drops"""
        return self._combine(other, MASK_ANDNOT)

    def _morph(self, op, radius):
        levels = self.info()["levels"]
        radii = [int(r) for r in radius] if hasattr(radius, "__len__") else level_radii(radius, levels)
        if len(radii) < levels:
            raise ValueError(f"{len(radii)} radii for a mask of {levels} levels")
        out = C.c_void_p()
        _check(lib().dvo_amd_mask_morph(self._h, op, (C.c_int * len(radii))(*radii), C.byref(out)), "dvo_amd_mask_morph")
        return SelectionMask._own(out, self.device)

    def dilate(self, radius):
        """Grown by a square window: a pixel is kept iff any pixel of the (2 r + 1)^2 window around it, clipped to the plane, is
        kept.  radius: an int in pixels of level 0 (level l gets level_radii(radius, levels)[l]) or one radius per level.  Every
        level is grown on its own (dvo_amd_mask_morph)."""
        return self._morph(MASK_DILATE, radius)

    def erode(self, radius):
        """Shrunk by a square window: a pixel is kept iff every pixel of the clipped window around it is kept; radius as for
        dilate"""
        return self._morph(MASK_ERODE, radius)

    def warp(self, source, target, T, counts: bool = False, **options):
        """This mask, on the pixels of the pyramid `source`, carried onto the pixels of the pyramid `target` (dvo_amd_mask_warp).
        T: 4x4, maps points of the target camera frame into the source camera frame -- for tracker.match(source, target) that is
        result.Transformation as returned.  options: near_z, depth_sigmas, unseen_keep, inconsistent_keep.  Returns the mask, or
        with counts=True (mask, counts): one MASK_WARP_DTYPE record per level."""
        masks, cnt = SelectionMask.warp_many([self], [source], [target], [T], counts=True, **options)
        return (masks[0], cnt[0]) if counts else masks[0]

    @staticmethod
    def warp_many(masks, sources, targets, Ts, counts: bool = False, **options):
        """n warps in one call and one kernel launch (dvo_amd_mask_warp_many): masks[k] on sources[k] onto targets[k] by Ts[k].
        Returns the list of masks, or with counts=True (masks, [counts of pair k: one MASK_WARP_DTYPE record per level])."""
        n = len(masks)
        if not (len(sources) == len(targets) == len(Ts) == n):
            raise ValueError("one source, one target and one transformation per mask")
        opt = mask_warp_options(**options)
        vp = C.c_void_p
        T = np.ascontiguousarray(np.stack([_pose_cm(t) for t in Ts]) if n else np.zeros((0, 4, 4)), dtype=np.float64)
        levels = [t.levels() for t in targets]
        cnt = np.zeros(max(1, sum(levels)), MASK_WARP_DTYPE)
        out = (vp * max(1, n))()
        _check(lib().dvo_amd_mask_warp_many(n, (vp * max(1, n))(*[m._h for m in masks]), (vp * max(1, n))(*[p._h for p in sources]),
                                            (vp * max(1, n))(*[p._h for p in targets]), T.ctypes.data_as(C.POINTER(C.c_double)),
                                            C.byref(opt), out, cnt.ctypes.data_as(C.POINTER(C.c_longlong))), "dvo_amd_mask_warp_many")
        made = [SelectionMask._own(vp(out[k]), targets[k].device) for k in range(n)]
        if not counts:
            return made
        at = np.concatenate([[0], np.cumsum(levels)]).astype(int)
        return made, [cnt[at[k]:at[k + 1]].copy() for k in range(n)]

    # ---- a mask from an alignment's residuals (the rule is pinned in include/dvo_amd.h under "Residual masks")

    @staticmethod
    def _residual_T(T, result):
        if T is None:
            if result is None:
                raise ValueError("give T (reference -> current, the estimate) or result=")
            T = rigid_inverse(result.Transformation)
        return _pose_cm(T)

    @classmethod
    def from_residuals(cls, tracker, reference, current, T=None, result=None, options=None, counts: bool = False,
                       distance: bool = False):
        """The inliers of the alignment of `current` against `reference` at T, on the reference's pixels
        (dvo_amd_mask_from_residuals): a pixel is kept iff its residual pair is valid and its Mahalanobis distance under the
        level's precision is at most the level's max_distance.  T: 4x4, reference -> current, the ESTIMATE -- what
        computeIntensityErrorImage takes.  tracker.match returns the inverse of the estimate, so with result= and no T the
        binding passes inv(result.Transformation), formed by rigid_inverse.  options: a ResidualMaskOptions; None:
        residual_mask_options(result, reference.levels()).  Returns the mask; with counts=True also one RESIDUAL_MASK_DTYPE record per level; with
        distance=True also the per-level float32 planes of the distance (NaN where the pixel is unevaluated or invalid)."""
        levels = reference.levels()
        opt = options if options is not None else residual_mask_options(result, levels)
        Tc = cls._residual_T(T, result)
        cnt = np.zeros(levels, RESIDUAL_MASK_DTYPE)
        planes = []
        for l in range(levels):
            w, h, _ = reference.level_info(l)
            planes.append(np.empty((h, w), np.float32))
        ptrs = (C.POINTER(C.c_float) * levels)(*[_fp(p) for p in planes])
        out = C.c_void_p()
        _check(lib().dvo_amd_mask_from_residuals(tracker._h, reference._h, current._h, Tc.ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.byref(opt), C.byref(out), cnt.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                 ptrs if distance else None), "dvo_amd_mask_from_residuals")
        got = (cls._own(out, reference.device),) + ((cnt,) if counts else ()) + ((planes,) if distance else ())
        return got[0] if len(got) == 1 else got

    @staticmethod
    def from_residuals_many(tracker, references, currents, Ts=None, results=None, options=None, counts: bool = False):
        """n inlier masks in one call and one kernel launch (dvo_amd_mask_from_residuals_many): pair k is (references[k],
        currents[k]) at Ts[k] (reference -> current; None: inv(results[k].Transformation)) under options[k] (None:
        residual_mask_options(results[k], levels)).  Returns the list of masks, or with counts=True (masks, [counts of pair k:
        one RESIDUAL_MASK_DTYPE record per level])."""
        n = len(references)
        Ts = [None] * n if Ts is None else list(Ts)
        results = [None] * n if results is None else list(results)
        options = [None] * n if options is None else list(options)
        if not (len(currents) == len(Ts) == len(results) == len(options) == n):
            raise ValueError("one current, one transformation or result and one option set per reference")
        vp = C.c_void_p
        levels = [r.levels() for r in references]
        opts = (ResidualMaskOptions * max(1, n))()
        for k in range(n):
            opts[k] = options[k] if options[k] is not None else residual_mask_options(results[k], levels[k])
        T = np.ascontiguousarray(np.stack([SelectionMask._residual_T(Ts[k], results[k]) for k in range(n)]) if n
                                 else np.zeros((0, 4, 4)), dtype=np.float64)
        cnt = np.zeros(max(1, sum(levels)), RESIDUAL_MASK_DTYPE)
        out = (vp * max(1, n))()
        _check(lib().dvo_amd_mask_from_residuals_many(tracker._h, n, (vp * max(1, n))(*[p._h for p in references]),
                                                      (vp * max(1, n))(*[p._h for p in currents]),
                                                      T.ctypes.data_as(C.POINTER(C.c_double)), opts, out,
                                                      cnt.ctypes.data_as(C.POINTER(C.c_longlong))),
               "dvo_amd_mask_from_residuals_many")
        made = [SelectionMask._own(vp(out[k]), references[k].device) for k in range(n)]
        if not counts:
            return made
        at = np.concatenate([[0], np.cumsum(levels)]).astype(int)
        return made, [cnt[at[k]:at[k + 1]].copy() for k in range(n)]

    @classmethod
    def from_normals(cls, pyramid, min_facing, options=None, undefined_keep: bool = False, counts: bool = False):
        """The pixels of `pyramid` whose surface faces the camera well enough (dvo_amd_mask_from_normals): kept iff the pixel's
        normal is defined and its facing value is at least min_facing (one value per level, or one for every level); a pixel
        without a normal is kept iff undefined_keep.  options: None, a NormalOptions or a dict of normal_options' arguments.
        Every level in one kernel launch.  With counts=True also one NORMAL_MASK_DTYPE record per level."""
        opt = _normal_options(options)
        n = pyramid.levels()
        mf = np.zeros(MAX_LEVELS, np.float32)
        mf[:] = np.float32(min_facing) if np.ndim(min_facing) == 0 else (list(min_facing) + [0.0] * MAX_LEVELS)[:MAX_LEVELS]
        cnt = np.zeros(MAX_LEVELS, NORMAL_MASK_DTYPE)
        out = C.c_void_p()
        _check(lib().dvo_amd_mask_from_normals(pyramid._h, C.byref(opt), _fp(mf), int(bool(undefined_keep)), C.byref(out),
                                               cnt.ctypes.data_as(C.POINTER(C.c_longlong)) if counts else None),
               "dvo_amd_mask_from_normals")
        mask = cls._own(out, pyramid.device)
        return (mask, cnt[:n].copy()) if counts else mask

    # ---- connected components (the rules are pinned in include/dvo_amd.h under "Mask components")

    def filter_components(self, depth=None, seeds=None, counts: bool = False, options=None, **fields):
        """The components of this mask -- cut further by the depth of the pyramid `depth` when given -- that pass the area band,
        touch `seeds` when given and are among the keep_largest largest when asked (dvo_amd_mask_filter_components).  fields:
        component_options' (connectivity, max_step, depth_sigmas, min_area, max_area, keep_largest).  Returns the mask, or with
        counts=True (mask, counts): one COMPONENT_COUNTS_DTYPE record per level."""
        masks, cnt = SelectionMask.filter_components_many([self], [depth], [seeds], counts=True, options=options, **fields)
        return (masks[0], cnt[0]) if counts else masks[0]

    @staticmethod
    def filter_components_many(masks, depths=None, seeds=None, counts: bool = False, options=None, **fields):
        """n component filters in one call of five kernel launches (dvo_amd_mask_filter_components_many): item k is masks[k] (a
        SelectionMask or None), depths[k] (an RgbdImagePyramid or None) and seeds[k] (a SelectionMask or None); depths and seeds
        may be None altogether.  Returns the list of masks, or with counts=True (masks, [counts of item k: one
        COMPONENT_COUNTS_DTYPE record per level])."""
        n = len(masks)
        depths = [None] * n if depths is None else list(depths)
        seeds = [None] * n if seeds is None else list(seeds)
        if not (len(depths) == len(seeds) == n):
            raise ValueError("one depth pyramid (or None) and one seed mask (or None) per mask")
        opt = _component_options(options, fields)
        vp = C.c_void_p
        handles = lambda items: (vp * max(1, n))(*[None if i is None else i._h for i in items])  # noqa: E731
        levels, devices = [], []
        for m, d in zip(masks, depths):
            levels.append(m.info()["levels"] if m is not None else d.levels() if d is not None else 0)
            devices.append(m.device if m is not None else d.device if d is not None else 0)
        cnt = np.zeros(max(1, sum(levels)), COMPONENT_COUNTS_DTYPE)
        out = (vp * max(1, n))()
        _check(lib().dvo_amd_mask_filter_components_many(n, handles(masks), handles(depths), handles(seeds), C.byref(opt), out,
                                                         cnt.ctypes.data_as(C.POINTER(C.c_longlong))),
               "dvo_amd_mask_filter_components_many")
        made = [SelectionMask._own(vp(out[k]), devices[k]) for k in range(n)]
        if not counts:
            return made
        at = np.concatenate([[0], np.cumsum(levels)]).astype(int)
        return made, [cnt[at[k]:at[k + 1]].copy() for k in range(n)]

    def components(self, level: int, depth=None, seeds=None, options=None, **fields):
        """One level's components (dvo_amd_mask_components): (labels, records) -- labels int32 [h >> level, w >> level], root + 1
        on a component's pixels and 0 on the background; records a COMPONENT_DTYPE array in ascending root order.  Of the options
        only the edge rule (connectivity, max_step, depth_sigmas) is read."""
        return _components(self, depth, seeds, level, _component_options(options, fields))

    def reconstruct(self, seeds):
        """The components of this mask that `seeds` still touches: with seeds = self.erode(r), an erosion's speckle removal
        without its loss of shape.  Shorthand for filter_components(seeds=seeds)."""
        return self.filter_components(seeds=seeds)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dvo_amd_mask_release(h)
            self._h = None

    def info(self) -> dict:
        """{"width", "height", "levels", "kept"}: kept[l] = the kept pixels of level l"""
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        kept = (C.c_longlong * MAX_LEVELS)()
        _check(lib().dvo_amd_mask_info(self._h, C.byref(w), C.byref(h), C.byref(n), kept), "dvo_amd_mask_info")
        return {"width": w.value, "height": h.value, "levels": n.value, "kept": [int(kept[l]) for l in range(n.value)]}

    def download(self, level: int) -> np.ndarray:
        """the plane of a level, uint8 [h >> level, w >> level] of 0 / 1"""
        i = self.info()
        out = np.empty((i["height"] >> level, i["width"] >> level), np.uint8)
        _check(lib().dvo_amd_mask_download(self._h, level, out.ctypes.data_as(C.POINTER(C.c_ubyte))), "dvo_amd_mask_download")
        return out


def _components(mask, depth, seeds, level, opt):
    """dvo_amd_mask_components for a mask (or None) and a depth pyramid (or None): one call with room for COMPONENTS_FIRST_CAPACITY
    records, a second one only when the level has more components than that"""
    if mask is not None:
        i = mask.info()
        w, h = (i["width"] >> level, i["height"] >> level) if 0 <= level < i["levels"] else (0, 0)  # (the library refuses it)
    elif depth is not None:
        w, h, _ = depth.level_info(level) if 0 <= level < depth.levels() else (0, 0, None)
    else:
        w = h = 0
    args = (None if mask is None else mask._h, None if depth is None else depth._h, None if seeds is None else seeds._h, C.byref(opt),
            int(level))
    labels = np.zeros((max(h, 0), max(w, 0)), np.int32)
    n = C.c_int()
    records = np.zeros(COMPONENTS_FIRST_CAPACITY, COMPONENT_DTYPE)
    _check(lib().dvo_amd_mask_components(*args, labels.ctypes.data_as(C.POINTER(C.c_int)), records.ctypes.data_as(C.c_void_p),
                                         len(records), C.byref(n)), "dvo_amd_mask_components")
    if n.value > len(records):  # more components than the first call had room for: once more, for the records alone
        records = np.zeros(n.value, COMPONENT_DTYPE)
        _check(lib().dvo_amd_mask_components(*args, None, records.ctypes.data_as(C.c_void_p), n.value, C.byref(n)),
               "dvo_amd_mask_components")
    records = records[:n.value].copy()
    return labels, records


@dataclasses.dataclass
class Registration:
    """A dvo_amd_registration: how `RgbdImagePyramid.from_raw(..., registration=)` takes raw depth of the depth camera into the
    colour camera (what depth_image_proc/register does on the CPU in front of the reference; the rule is pinned in
    include/dvo_amd.h).  depth_size = (width, height) of the raw depth frame (None: the shape of the depth array given to
    from_raw), K_depth = (fx, fy, ox, oy) of the depth camera, T = 4x4 depth camera -> colour camera, min_z >= 0: a measurement is
    kept only if its colour-frame z > min_z, fill: False one pixel per measurement, True the measurement's footprint."""
    depth_size: "tuple | None" = None
    K_depth: tuple = (0.0, 0.0, 0.0, 0.0)
    T: "np.ndarray | None" = None
    min_z: float = 0.0
    fill: bool = False

    def _c(self, depth_size=None) -> CRegistration:
        c = CRegistration()
        lib().dvo_amd_default_registration(C.byref(c))
        size = depth_size if depth_size is not None else self.depth_size
        if size is None:
            raise ValueError("the registration has no depth_size")
        c.depth_width, c.depth_height = int(size[0]), int(size[1])
        c.k_depth[:] = [float(k) for k in self.K_depth]
        if self.T is not None:
            c.T[:] = [float(v) for v in _pose_cm(self.T).ravel()]
        c.min_z, c.fill = float(self.min_z), int(self.fill)
        return c


def ingest_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event bracket around every pyramid build of `device` on or off and returns the device time
    of the most recent bracketed build in ms (dvo_amd_debug_ingest_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_ingest_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_ingest_timing")
    return ms.value


def batch_build_stats(device: int = 0) -> dict:
    """(instrumentation) what the most recent RgbdImagePyramid.from_raw_batch on `device` enqueued:
    {"kernel_launches", "copies", "synchronisations"} (dvo_amd_debug_batch_build_stats)"""
    v = [C.c_int() for _ in range(3)]
    _check(lib().dvo_amd_debug_batch_build_stats(device, *[C.byref(x) for x in v]), "dvo_amd_debug_batch_build_stats")
    return dict(zip(("kernel_launches", "copies", "synchronisations"), (x.value for x in v)))


class RgbdImagePyramid:
    """RgbdCameraPyramid(w, h, K).create(intensity, depth) with `levels` levels built on the GPU."""

    def __init__(self, intensity, depth, K, levels: int, device: int = 0, timestamp: float = 0.0):
        intensity = np.ascontiguousarray(intensity, dtype=np.float32)
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if intensity.shape != depth.shape or intensity.ndim != 2:
            raise ValueError("intensity and depth must be 2-D arrays of the same shape")
        h, w = intensity.shape
        fx, fy, ox, oy = [float(k) for k in K]
        self._h = C.c_void_p()
        _check(lib().dvo_amd_pyramid_create(device, _fp(intensity), _fp(depth), w, h, w, fx, fy, ox, oy, levels,
                                            timestamp, C.byref(self._h)), "dvo_amd_pyramid_create")
        self.device = device

    @classmethod
    def from_device(cls, d_intensity: int, d_depth: int, width: int, height: int, K, levels: int, device: int = 0,
                    timestamp: float = 0.0, stride: int | None = None):
        """Planes already resident in HBM (raw device pointers, e.g. torch.Tensor.data_ptr())."""
        self = cls.__new__(cls)
        fx, fy, ox, oy = [float(k) for k in K]
        self._h = C.c_void_p()
        _check(lib().dvo_amd_pyramid_create_from_device(device, C.c_void_p(d_intensity), C.c_void_p(d_depth), width,
                                                        height, stride or width, fx, fy, ox, oy, levels, timestamp,
                                                        C.byref(self._h)), "dvo_amd_pyramid_create_from_device")
        self.device = device
        return self

    @classmethod
    def from_raw(cls, image, depth, K, levels: int, depth_scale: float = 1.0 / 5000.0, device: int = 0,
                 timestamp: float = 0.0, remap: "Remap | None" = None, registration: "Registration | None" = None):
        """Frame ingest on the device: uint8 image (HxW gray or HxWx3 BGR) + uint16 depth (0 = invalid), as a camera or a
        TUM PNG pair delivers them (benchmark_slam.cpp:46-93).  Gray conversion and depth scaling run on the GPU.
        With `remap` the frame has the remap's source size and is resampled through it (dvo_amd_pyramid_create_raw_remapped):
        the pyramid has the remap's output size and K is the rectified camera's.
        With `registration` the depth array is the depth camera's own frame, of any size, and is registered into the colour camera
        K (dvo_amd_pyramid_create_raw_registered): only the image goes through `remap`, and the pyramid carries
        `registration_stats`."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.ndim != 2 or image.ndim not in (2, 3) or (registration is None and image.shape[:2] != depth.shape):
            raise ValueError("image must be HxW or HxWx3 uint8 and depth HxW uint16 of the same size")
        channels = 1 if image.ndim == 2 else image.shape[2]
        h, w = image.shape[:2]
        dh, dw = depth.shape
        return cls._raw(image.ctypes.data, channels, w * channels, depth.ctypes.data, dw, depth_scale, 0, w, h, K, levels,
                        device, timestamp, remap, registration, (dw, dh) if registration is not None else None)

    @classmethod
    def from_raw_device(cls, d_image: int, channels: int, d_depth: int, width: int, height: int, K, levels: int,
                        depth_scale: float = 1.0 / 5000.0, device: int = 0, timestamp: float = 0.0,
                        image_stride_bytes: int | None = None, depth_stride: int | None = None,
                        remap: "Remap | None" = None, registration: "Registration | None" = None, depth_size=None):
        """As from_raw, for raw frames already resident in HBM (device pointers).  With `remap`, width and height are the raw
        frame's (the remap's source size).  With `registration`, width and height are the image's and depth_size = (width,
        height) of the depth frame (None: the registration's own depth_size)."""
        if registration is not None and depth_size is None:
            depth_size = registration.depth_size
        depth_width = depth_size[0] if registration is not None and depth_size is not None else width
        return cls._raw(d_image, channels, image_stride_bytes or width * channels, d_depth, depth_stride or depth_width,
                        depth_scale, 1, width, height, K, levels, device, timestamp, remap, registration, depth_size)

    @classmethod
    def _raw(cls, image_ptr, channels, image_stride, depth_ptr, depth_stride, depth_scale, on_device, w, h, K, levels,
             device, timestamp, remap=None, registration=None, depth_size=None):
        self = cls.__new__(cls)
        fx, fy, ox, oy = [float(k) for k in K]
        self._h = C.c_void_p()
        self.registration_stats = None
        if registration is not None:
            if remap is not None:
                i = remap.info()
                if (w, h) != (i["src_width"], i["src_height"]):
                    raise ValueError(f"the raw image is {w}x{h} but the remap's source is {i['src_width']}x{i['src_height']}")
                w, h = i["width"], i["height"]
            reg, st = registration._c(depth_size), CRegistrationStats()
            _check(lib().dvo_amd_pyramid_create_raw_registered(device, C.c_void_p(image_ptr), channels, image_stride,
                                                               C.c_void_p(depth_ptr), depth_stride, depth_scale, on_device,
                                                               C.byref(reg), None if remap is None else remap._h, w, h, fx, fy,
                                                               ox, oy, levels, timestamp, C.byref(self._h), C.byref(st)),
                   "dvo_amd_pyramid_create_raw_registered")
            self.registration_stats = {n: getattr(st, n) for n, _ in CRegistrationStats._fields_}
            self.device = device
            return self
        if remap is not None:
            i = remap.info()
            if (w, h) != (i["src_width"], i["src_height"]):
                raise ValueError(f"the raw frame is {w}x{h} but the remap's source is {i['src_width']}x{i['src_height']}")
            _check(lib().dvo_amd_pyramid_create_raw_remapped(device, C.c_void_p(image_ptr), channels, image_stride,
                                                             C.c_void_p(depth_ptr), depth_stride, depth_scale, on_device,
                                                             remap._h, fx, fy, ox, oy, levels, timestamp, C.byref(self._h)),
                   "dvo_amd_pyramid_create_raw_remapped")
            self.device = device
            return self
        _check(lib().dvo_amd_pyramid_create_raw(device, C.c_void_p(image_ptr), channels, image_stride,
                                                C.c_void_p(depth_ptr), depth_stride, depth_scale, on_device, w, h, fx, fy,
                                                ox, oy, levels, timestamp, C.byref(self._h)),
               "dvo_amd_pyramid_create_raw")
        self.device = device
        return self

    @classmethod
    def from_raw_batch(cls, images, depths, K, levels: int, depth_scale: float = 1.0 / 5000.0, device: int = 0, timestamps=None,
                       selection=None, size=None, channels: int | None = None, image_stride_bytes: int | None = None,
                       depth_stride: int | None = None):
        """from_raw for many frames of one camera in one call (dvo_amd_pyramid_create_raw_batch): a list of pyramids, each
        bit-identical to from_raw's of the same frame, built in a number of kernel launches that does not depend on how many
        frames there are.  images / depths: sequences of numpy arrays (uint8 HxW or HxWx3, uint16 HxW, all of one shape), or of
        device pointers (ints) together with size = (width, height) and channels -- and, when the rows are not packed,
        image_stride_bytes / depth_stride --, as from_raw_device takes them.  timestamps: one per frame, or None for 0.0.
        selection: None, or (intensity_threshold, depth_threshold) to leave every pyramid with that point selection already
        built, so that the first match() with those thresholds launches nothing for it."""
        n = len(images)
        if n < 1 or len(depths) != n or (timestamps is not None and len(timestamps) != n):
            raise ValueError("images, depths and timestamps must name the same number of frames, at least one")
        on_device = not isinstance(images[0], np.ndarray) and isinstance(images[0], int)
        if on_device:
            if size is None or channels is None:
                raise ValueError("device pointers need size=(width, height) and channels")
            w, h = int(size[0]), int(size[1])
            keep, img_ptrs, z_ptrs = None, [int(p) for p in images], [int(p) for p in depths]
        else:
            ims = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
            zs = [np.ascontiguousarray(a, dtype=np.uint16) for a in depths]
            if any(a.shape != ims[0].shape for a in ims) or any(z.shape != zs[0].shape for z in zs) or zs[0].ndim != 2 or \
                    ims[0].ndim not in (2, 3) or ims[0].shape[:2] != zs[0].shape:
                raise ValueError("every image must be HxW or HxWx3 uint8 and every depth HxW uint16, all of one size")
            channels = 1 if ims[0].ndim == 2 else ims[0].shape[2]
            h, w = zs[0].shape
            image_stride_bytes = depth_stride = None
            keep, img_ptrs, z_ptrs = (ims, zs), [a.ctypes.data for a in ims], [z.ctypes.data for z in zs]
        b = CRawBatch()
        b.count = n
        b.images, b.depths = (C.c_void_p * n)(*img_ptrs), (C.c_void_p * n)(*z_ptrs)
        b.timestamps = None if timestamps is None else (C.c_double * n)(*[float(t) for t in timestamps])
        b.channels, b.image_stride_bytes, b.depth_stride = channels, image_stride_bytes or w * channels, depth_stride or w
        b.depth_scale, b.on_device, b.width, b.height = depth_scale, int(on_device), w, h
        b.fx, b.fy, b.ox, b.oy = [float(k) for k in K]
        b.levels, b.build_selection = levels, int(selection is not None)
        if selection is not None:
            b.intensity_threshold, b.depth_threshold = float(selection[0]), float(selection[1])
        out = (C.c_void_p * n)()
        _check(lib().dvo_amd_pyramid_create_raw_batch(device, C.byref(b), out), "dvo_amd_pyramid_create_raw_batch")
        del keep
        pyramids = []
        for f in range(n):
            self = cls.__new__(cls)
            self._h, self.device, self.registration_stats = C.c_void_p(out[f]), device, None
            pyramids.append(self)
        return pyramids

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dvo_amd_pyramid_release(h)
            self._h = None

    def levels(self) -> int:
        return lib().dvo_amd_pyramid_levels(self._h)

    def timestamp(self) -> float:
        return lib().dvo_amd_pyramid_timestamp(self._h)

    def level_info(self, level: int):
        w, h = C.c_int(), C.c_int()
        k = np.zeros(4, np.float32)
        _check(lib().dvo_amd_pyramid_level_info(self._h, level, C.byref(w), C.byref(h), _fp(k)), "level_info")
        return w.value, h.value, k

    def plane(self, level: int, plane: int) -> np.ndarray:
        """0 I, 1 Z, 2 Ix, 3 Iy, 4 Zx, 5 Zy of a level, downloaded."""
        w, h, _ = self.level_info(level)
        out = np.empty((h, w), np.float32)
        _check(lib().dvo_amd_pyramid_download_plane(self._h, level, plane, _fp(out)), "download_plane")
        return out

    def select(self, level: int, ti: float = 0.0, td: float = 0.0, mask: "SelectionMask | None" = None):
        """PointSelection::select: (count, mask[h, w]).  With `mask` (a SelectionMask) a pixel is selected iff the mask keeps it
        and the threshold predicate does (dvo_amd_pyramid_select_masked)."""
        w, h, _ = self.level_info(level)
        out = np.empty((h, w), np.uint8)
        cnt = C.c_int()
        if mask is not None:
            _check(lib().dvo_amd_pyramid_select_masked(self._h, level, ti, td, mask._h, C.byref(cnt),
                                                       out.ctypes.data_as(C.POINTER(C.c_ubyte))), "pyramid_select_masked")
            return cnt.value, out
        _check(lib().dvo_amd_pyramid_select(self._h, level, ti, td, C.byref(cnt),
                                            out.ctypes.data_as(C.POINTER(C.c_ubyte))), "pyramid_select")
        return cnt.value, out

    # ---- depth fusion (the rule is pinned in include/dvo_amd.h under "Depth fusion")

    def fuse_depth(self, frames, transformations, options=None, counts: bool = False, observations: bool = False):
        """This keyframe with the level-0 depth of `frames` averaged into its own (dvo_amd_pyramid_fuse_depth): a new pyramid of
        this one's size, intrinsics, level count and timestamp; this one is only read.  transformations[k]: 4x4, for
        tracker.match(self, frames[k]) the result's Transformation as returned.  options: None, a FuseOptions or a dict of its
        fields (near_z, depth_sigmas, min_cos, sample, min_observations, drop_unconfirmed).  Returns the pyramid; with counts=True
        also the frame counts (one FUSE_FRAME_DTYPE record per frame) and the keyframe counts (one FUSE_KEYFRAME_DTYPE record);
        with observations=True also the observations per pixel (uint8 [h, w]) -- as a tuple, in this order."""
        got = RgbdImagePyramid.fuse_depth_many([self], [frames], [transformations], options, counts=counts, observations=observations)
        return tuple(part[0] for part in got) if counts or observations else got[0]

    @staticmethod
    def fuse_depth_many(keyframes, frames_per_keyframe, transformations_per_keyframe, options=None, counts: bool = False,
                        observations: bool = False):
        """fuse_depth for many keyframes in one call and one kernel launch (dvo_amd_pyramid_fuse_depth_many): keyframes[j] with
        frames_per_keyframe[j] at transformations_per_keyframe[j].  Returns the list of pyramids; with counts=True also the list of
        frame counts (per keyframe one FUSE_FRAME_DTYPE record per frame) and the keyframe counts (a FUSE_KEYFRAME_DTYPE array);
        with observations=True also the list of observation planes (uint8 [h, w]) -- as a tuple, in this order."""
        nk = len(keyframes)
        if not (len(frames_per_keyframe) == len(transformations_per_keyframe) == nk):
            raise ValueError("one list of frames and one list of transformations per keyframe")
        if any(len(f) != len(t) for f, t in zip(frames_per_keyframe, transformations_per_keyframe)):
            raise ValueError("one transformation per frame")
        opt = options if isinstance(options, FuseOptions) else fuse_options(**(options or {}))
        vp = C.c_void_p
        offsets = np.concatenate([[0], np.cumsum([len(f) for f in frames_per_keyframe])]).astype(np.int32)
        total = int(offsets[-1])
        flat = [p for f in frames_per_keyframe for p in f]
        T = np.ascontiguousarray(np.stack([_pose_cm(t) for ts in transformations_per_keyframe for t in ts]) if total
                                 else np.zeros((1, 4, 4)), dtype=np.float64)
        frame_cnt = np.zeros(max(1, total), FUSE_FRAME_DTYPE)
        key_cnt = np.zeros(max(1, nk), FUSE_KEYFRAME_DTYPE)
        planes = []
        for kf in keyframes:
            w, h, _ = kf.level_info(0)
            planes.append(np.zeros((h, w), np.uint8))
        out = (vp * max(1, nk))()
        obs = (vp * max(1, nk))(*[p.ctypes.data for p in planes]) if observations else None
        ll = C.POINTER(C.c_longlong)
        _check(lib().dvo_amd_pyramid_fuse_depth_many(nk, (vp * max(1, nk))(*[p._h for p in keyframes]),
                                                     offsets.ctypes.data_as(C.POINTER(C.c_int)),
                                                     (vp * max(1, total))(*[p._h for p in flat]), T.ctypes.data_as(C.POINTER(C.c_double)),
                                                     C.byref(opt), out, frame_cnt.ctypes.data_as(ll) if counts else None,
                                                     key_cnt.ctypes.data_as(ll) if counts else None, obs),
               "dvo_amd_pyramid_fuse_depth_many")
        made = []
        for j in range(nk):
            p = RgbdImagePyramid.__new__(RgbdImagePyramid)
            p._h, p.device, p.registration_stats = vp(out[j]), keyframes[j].device, None
            made.append(p)
        result = (made,)
        if counts:
            result += ([frame_cnt[offsets[j]:offsets[j + 1]].copy() for j in range(nk)], key_cnt[:nk].copy())
        if observations:
            result += (planes,)
        return result if len(result) > 1 else made

    # ---- frame warps (the rules are pinned in include/dvo_amd.h under "Frame warps")

    def warp_inverse(self, fixed: "RgbdImagePyramid", T, level=None, options=None):
        """THIS frame, the moving one, resampled onto the pixels of `fixed` (dvo_amd_warp_inverse / dvo_amd_pyramid_warp_inverse).
        T: 4x4, maps points of this frame's camera into the fixed camera: for tracker.match(fixed, self) the result's
        Transformation as returned.  With a level: (intensity float32 [h, w], depth float32 [h, w], counts) on the fixed level's
        pixels, NaN where empty; with level=None: (pyramid, counts), a pyramid like `fixed` in which only warped pixels have a
        depth.  counts: one WARP_INVERSE_DTYPE record."""
        got = warp_inverse_many([fixed], [self], [T], level, options)
        return tuple(part[0] for part in got)

    def warp_forward(self, T, view=None, level=None, options=None):
        """This frame's pixels drawn into a view with a nearest-depth test (dvo_amd_warp_forward / dvo_amd_pyramid_warp_forward).
        T: 4x4, maps points of this frame's camera into the view's.  view: None (this frame's own camera at `level`), or
        (K, width, height[, near_z]).  With a level: (depth float32, intensity float32, index int32 [h, w], counts), empty pixels
        NaN, NaN and -1; with level=None: (pyramid, counts).  counts: one WARP_FORWARD_DTYPE record."""
        got = warp_forward_many([self], [T], None if view is None else [view], level, options)
        return tuple(part[0] for part in got)

    def filter_depth(self, options=None, counts: bool = False, support: bool = False):
        """This pyramid with its level-0 depth filtered (dvo_amd_pyramid_filter_depth; the rule is pinned in include/dvo_amd.h
        under "Depth filtering"): a new pyramid of this one's size, intrinsics, level count and timestamp; this one is only read.
        options: None, a DepthFilterOptions or a dict of its fields.  Returns the pyramid; with counts=True also the counts (one
        DEPTH_FILTER_DTYPE record); with support=True also the support plane (uint16 [h, w]) -- as a tuple, in this order."""
        got = filter_depth_many([self], options, counts=counts, support=support)
        return tuple(part[0] for part in got) if counts or support else got[0]

    def estimate_exposure(self, reference: "RgbdImagePyramid", T=None, mask: "SelectionMask | None" = None, options=None,
                          tracker: "DenseTracker | None" = None) -> ExposureEstimate:
        """The gain and bias with which THIS frame, the current one, looks like `reference`: I_ref ~ gain * I_cur + bias over the
        pixels both see (dvo_amd_estimate_exposure; the rule is pinned in include/dvo_amd.h under "Exposure compensation").  T:
        4x4, reference -> current, the estimate (None: the identity); mask: on the reference's pixels; options: None, an
        ExposureOptions or a dict of its fields.  The entry runs in a tracker's context, which gives its device and nothing else:
        `tracker` when one is given, otherwise the shared one point_cloud uses."""
        return estimate_exposure_many(tracker or _cloud_tracker(self.device), [reference], [self], None if T is None else [T],
                                      None if mask is None else [mask], [options])[0]

    def adjust_intensity(self, gain: float, bias: float) -> "RgbdImagePyramid":
        """This pyramid with level 0's intensity mapped to (gain * I) + bias, not clamped (dvo_amd_pyramid_adjust_intensity): a new
        pyramid with this one's depth, intrinsics, level count and timestamp; this one is only read."""
        return adjust_intensity_many([self], [gain], [bias])[0]

    def depth_components(self, seeds=None, counts: bool = False, level=None, options=None, **fields):
        """The depth-connected surfaces of this pyramid, the mask = None form of the component entries: every pixel with a finite
        depth is foreground and the depth rule cuts the edges.  level=None: SelectionMask.filter_components' result (the mask of
        the kept surfaces, with counts=True also the counts); level=l: SelectionMask.components' (labels, records) of that level."""
        opt = _component_options(options, fields)
        if level is not None:
            return _components(None, self, seeds, level, opt)
        masks, cnt = SelectionMask.filter_components_many([None], [self], [seeds], counts=True, options=opt)
        return (masks[0], cnt[0]) if counts else masks[0]

    def normals(self, level: int = 0, options=None, **fields):
        """The surface normals of a level (dvo_amd_pyramid_normals; the rule is pinned in include/dvo_amd.h under "Surface
        normals"): (normals float32 [h, w, 4], facing float32 [h, w], {"defined": n, "undefined": n}).  options: None, a
        NormalOptions or a dict of normal_options' arguments; keyword arguments are normal_options' too."""
        opt = _normal_options(dict(options or {}, **fields) if not isinstance(options, NormalOptions) else options)
        w, h, _ = self.level_info(level)
        normals, facing = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
        cnt = (C.c_longlong * 2)()
        _check(lib().dvo_amd_pyramid_normals(self._h, level, C.byref(opt), _fp(normals), _fp(facing), cnt), "dvo_amd_pyramid_normals")
        return normals, facing, dict(zip(NORMAL_COUNTS, cnt))

    def point_cloud(self, pose=None, bgr=None, level: int = 0, tracker: "DenseTracker | None" = None, normals=None):
        """RgbdCamera::buildPointCloud of a level transformed by `pose` (4x4, None = identity) and coloured from `bgr` (uint8
        HxWx3 of the level, None = grey from the intensity plane): (xyz float32 [h, w, 3], rgb uint32 [h, w]) in scan order,
        NaN points included (dvo_amd_point_cloud).  The entry runs in a tracker's context: `tracker` when one is given,
        otherwise a shared DenseTracker of the pyramid's device that this module creates on the first such call and keeps for
        the life of the process (with the buffers of the largest cloud it built; nothing is allocated per call once warm).
        Pass `tracker=` to choose the context -- and with it where the buffers live and when they are freed.
        With `normals` (True, a NormalOptions or a dict of normal_options' arguments) the result is (xyz, rgb, normals float32
        [h, w, 4]): every point's surface normal in the pose's frame as well (dvo_amd_point_cloud_normals)."""
        w, h, _ = self.level_info(level)
        out = np.empty((h * w, 4), np.float32)
        T = None if pose is None else _pose_cm(pose)
        bgr_ptr, stride = None, 0
        if bgr is not None:
            bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
            if bgr.shape != (h, w, 3):
                raise ValueError(f"bgr must be ({h}, {w}, 3) uint8 for level {level}")
            bgr_ptr, stride = bgr.ctypes.data, w * 3
        trk = tracker or _cloud_tracker(self.device)
        if normals is not None and normals is not False:
            opt = _normal_options(None if normals is True else normals)
            nrm = np.empty((h, w, 4), np.float32)
            _check(lib().dvo_amd_point_cloud_normals(trk._h, self._h, level,
                                                     None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)),
                                                     bgr_ptr, stride, C.byref(opt), out.ctypes.data, _fp(nrm)),
                   "dvo_amd_point_cloud_normals")
            xyz, rgb = _split_points(out)
            return xyz.reshape(h, w, 3), rgb.reshape(h, w), nrm
        _check(lib().dvo_amd_point_cloud(trk._h, self._h, level,
                                         None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)),
                                         bgr_ptr, stride, out.ctypes.data), "dvo_amd_point_cloud")
        xyz, rgb = _split_points(out)
        return xyz.reshape(h, w, 3), rgb.reshape(h, w)


class Result:
    """DenseTracker::Result: Transformation (4x4), Information (6x6), LogLikelihood, Statistics.Levels."""

    def __init__(self, c: CResult, its):
        self.Transformation = np.array(c.transformation[:]).reshape(4, 4).T.copy()
        self.Information = np.array(c.information[:]).reshape(6, 6).T.copy()
        self.LogLikelihood = c.loglik
        self._is_nan = bool(c.is_nan)
        self.n_ticks = c.n_ticks
        self.n_residual_passes = c.n_residual_passes
        self.alg_bytes = c.alg_bytes
        self.alg_bytes_discarded = c.alg_bytes_discarded
        self.Levels = []
        for l in range(c.n_levels):
            L = c.levels[l]
            iters = []
            for k in range(L.n_iterations if its is not None else 0):
                it = its[L.first_iteration + k]
                iters.append({
                    "Id": it.id, "ValidConstraints": it.valid_constraints,
                    "TDistributionLogLikelihood": it.tdist_loglik,
                    "TDistributionPrecision": np.array(it.tdist_precision[:]).reshape(2, 2).T.copy(),
                    "PriorLogLikelihood": it.prior_loglik, "has_increment": bool(it.has_increment),
                    "EstimateIncrement": np.array(it.increment[:]),
                    "EstimateInformation": np.array(it.information[:]).reshape(6, 6).T.copy(),
                    "estimate": np.array(it.estimate[:]).reshape(4, 4).T.copy(),  # instrumentation, not a reference field
                    "initial": np.array(it.initial[:]).reshape(4, 4).T.copy(),    # likewise
                })
            self.Levels.append({"Id": L.id, "MaxValidPixels": L.max_valid_pixels, "ValidPixels": L.valid_pixels,
                                "TerminationCriterion": L.termination, "Iterations": iters})

    def isNaN(self) -> bool:
        return self._is_nan


class Submission:
    """n pairs queued with DenseTracker.submit: the ticket, and the result structs the library fills (kept alive here)"""

    def __init__(self, ticket, res, its, n):
        self.ticket, self._res, self._its, self.n = ticket, res, its, n

    def results(self, raw: bool = False):
        if raw:
            self._res._keepalive = self._its
            return self._res
        return [Result(self._res[i], self._its[i]) for i in range(self.n)]


class DenseTracker:
    """dvo::DenseTracker: configure(), match(reference, current, T_init) -> Result.  One HIP stream; not thread-safe."""

    def __init__(self, config: Config | None = None, device: int = 0):
        self._cfg = config or Config()
        if not self._cfg.IsSane():
            raise DvoAmdError(5, "DenseTracker.configure")
        self._h = C.c_void_p()
        c = self._cfg._c()
        _check(lib().dvo_amd_context_create(device, C.byref(c), C.byref(self._h)), "dvo_amd_context_create")
        self.device = device
        # the library writes the results of a submission until it is complete: the tracker keeps every open Submission (its
        # result structs and iteration arrays) alive, whether or not the caller holds on to it
        self._open = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dvo_amd_context_destroy(h)
            self._h = None

    def configuration(self) -> Config:
        return self._cfg

    def set_reciprocal_mode(self, mode: str):
        """"exact" (default): 1 / z of the projection is the exactly truncated quotient; "host_sse": the warp stage and the
        t-distribution weights use THIS HOST's _mm_rcp_ps bit for bit, from a table probed on the host (dvo_amd_set_reciprocal_mode)"""
        _check(lib().dvo_amd_set_reciprocal_mode(self._h, {"exact": 0, "host_sse": 1}[mode]), "dvo_amd_set_reciprocal_mode")

    def reciprocal_mode(self):
        """(mode name, mantissa bits the host's rcpps table is indexed by -- 0 in the exact mode)"""
        m, k = C.c_int(), C.c_int()
        _check(lib().dvo_amd_get_reciprocal_mode(self._h, C.byref(m), C.byref(k)), "dvo_amd_get_reciprocal_mode")
        return ("host_sse" if m.value else "exact"), k.value

    def reciprocal_form(self):
        """(diagnostic) ("off" | "table" | "nibbles", why the nibble form is not in use)"""
        form, note = C.c_int(), C.create_string_buffer(256)
        _check(lib().dvo_amd_debug_rcp_form(self._h, C.byref(form), note, 256), "dvo_amd_debug_rcp_form")
        return ("off", "table", "nibbles")[form.value], note.value.decode()

    def table_rcp(self, x) -> np.ndarray:
        """the table reciprocal of every element as the kernels compute it (test entry; needs the host_sse mode)"""
        a = np.ascontiguousarray(x, dtype=np.float32).ravel()
        out = np.empty_like(a)
        _check(lib().dvo_amd_debug_rcp(self._h, a.size, _fp(a), _fp(out)), "dvo_amd_debug_rcp")
        return out.reshape(np.shape(x))

    def _voxels(self, call, where, capacity):
        """runs call(out, capacity, stats) and grows the output once on DVO_AMD_ERR_CAPACITY"""
        stats = CCloudStats()
        out = np.empty((max(1, capacity), 4), np.float32)
        rc = call(out.ctypes.data, capacity, C.byref(stats))
        if rc == 7:  # DVO_AMD_ERR_CAPACITY: stats.voxels is the size needed
            capacity = int(stats.voxels)
            out = np.empty((max(1, capacity), 4), np.float32)
            rc = call(out.ctypes.data, capacity, C.byref(stats))
        _check(rc, where)
        xyz, rgb = _split_points(out[:stats.voxels])
        return xyz, rgb, {"points_in": stats.points_in, "finite": stats.finite, "out_of_range": stats.out_of_range,
                          "voxels": stats.voxels}

    def map_cloud(self, pyramids, poses, bgrs=None, leaf: float = 0.01, capacity: int | None = None):
        """The voxel aggregate of level 0 of every pyramid at its pose (4x4 each), coloured from bgrs (None, or one uint8 HxWx3
        or None per pyramid): (xyz float32 [V, 3], rgb uint32 [V], stats dict) in voxel-key order (dvo_amd_map_cloud)."""
        n = len(pyramids)
        if len(poses) != n or (bgrs is not None and len(bgrs) != n):
            raise ValueError("one pose (and one bgr entry) per pyramid")
        hs = (C.c_void_p * max(1, n))(*[p._h for p in pyramids])
        T = np.ascontiguousarray(np.stack([_pose_cm(P) for P in poses])) if n else np.zeros((1, 4, 4))
        keep, bp, st = [], None, None
        if bgrs is not None:
            bp = (C.c_void_p * max(1, n))()
            st = (C.c_int * max(1, n))()
            for k, (p, b) in enumerate(zip(pyramids, bgrs)):
                if b is None:
                    continue
                w, h, _ = p.level_info(0)
                b = np.ascontiguousarray(b, dtype=np.uint8)
                if b.shape != (h, w, 3):
                    raise ValueError(f"bgrs[{k}] must be ({h}, {w}, 3) uint8")
                keep.append(b)
                bp[k], st[k] = b.ctypes.data, w * 3
        if capacity is None:
            capacity = max(1, sum(p.level_info(0)[0] * p.level_info(0)[1] for p in pyramids) // 8)

        def call(out, cap, stats):
            return lib().dvo_amd_map_cloud(self._h, n, hs, T.ctypes.data_as(C.POINTER(C.c_double)), bp, st, leaf, out, cap,
                                           stats)
        return self._voxels(call, "dvo_amd_map_cloud", capacity)

    def voxel_downsample(self, xyz, rgb, leaf: float, capacity: int | None = None):
        """The voxel aggregate of given points (xyz [n, 3], rgb uint32 [n]): as map_cloud (dvo_amd_voxel_downsample)."""
        pts = _pack_points(xyz, rgb)
        n = len(pts)
        if capacity is None:
            capacity = max(1, n // 8)

        def call(out, cap, stats):
            return lib().dvo_amd_voxel_downsample(self._h, n, pts.ctypes.data, leaf, out, cap, stats)
        return self._voxels(call, "dvo_amd_voxel_downsample", capacity)

    def map_timing(self):
        """(diagnostic) the last map_cloud / voxel_downsample: (device ms of its kernels, ms of the output copy, points)"""
        d, c, n = C.c_double(), C.c_double(), C.c_longlong()
        _check(lib().dvo_amd_debug_map_timing(self._h, C.byref(d), C.byref(c), C.byref(n)), "dvo_amd_debug_map_timing")
        return d.value, c.value, n.value

    def debug_map_merge(self, keys_a, acc_a, keys_b, acc_b):
        """(test entry) the keyframe map's merge of a store (keys uint64 [na] ascending and distinct, sums uint64 [na, 8]) and
        a delta (the same, nb entries) on the device: (keys uint64 [n], sums uint64 [n, 8]) of the compacted store
        (dvo_amd_debug_map_merge)."""
        ka, kb = [np.ascontiguousarray(k, dtype=np.uint64).reshape(-1) for k in (keys_a, keys_b)]
        va, vb = [np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 8) for v in (acc_a, acc_b)]
        if len(va) != len(ka) or len(vb) != len(kb):
            raise ValueError("eight uint64 of sums per key")
        total = len(ka) + len(kb)
        ko, vo, n = np.zeros(max(1, total), np.uint64), np.zeros((max(1, total), 8), np.uint64), C.c_longlong(-1)
        _check(lib().dvo_amd_debug_map_merge(self._h, len(ka), ka.ctypes.data, va.ctypes.data, len(kb), kb.ctypes.data,
                                             vb.ctypes.data, ko.ctypes.data, vo.ctypes.data, C.byref(n)), "dvo_amd_debug_map_merge")
        return ko[:n.value].copy(), vo[:n.value].copy()

    def configure(self, config: Config):
        c = config._c()
        _check(lib().dvo_amd_configure(self._h, C.byref(c)), "dvo_amd_configure")
        self._cfg = config

    def _alloc_results(self, n):
        cap = (self._cfg.FirstLevel - self._cfg.LastLevel + 1) * (self._cfg.MaxIterationsPerLevel + 1)
        res = (CResult * n)()
        its = []
        for i in range(n):
            buf = (CIterationStats * cap)()
            its.append(buf)
            res[i].iterations = C.cast(buf, C.POINTER(CIterationStats))
            res[i].iterations_capacity = cap
        return res, its

    def match(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, T_init=None, mask: "SelectionMask | None" = None,
              thresholds=None) -> Result:
        """mask: only the reference pixels it keeps take part; thresholds = (intensity, depth): the selection thresholds of this
        call instead of the configuration's (dvo_amd_match_masked; with thresholds alone, dvo_amd_match_selection)"""
        res, its = self._alloc_results(1)
        T0 = None
        if T_init is not None:
            T0a = np.ascontiguousarray(np.asarray(T_init, dtype=np.float64).T)
            T0 = T0a.ctypes.data_as(C.POINTER(C.c_double))
        if mask is None and thresholds is None:
            _check(lib().dvo_amd_match(self._h, reference._h, current._h, T0, C.byref(res[0])), "dvo_amd_match")
            return Result(res[0], its[0])
        ti, td = thresholds if thresholds is not None else (self._cfg.IntensityDerivativeThreshold, self._cfg.DepthDerivativeThreshold)
        _check(lib().dvo_amd_match_masked(self._h, reference._h, None if mask is None else mask._h, ti, td, current._h, T0,
                                          C.byref(res[0])), "dvo_amd_match_masked")
        return Result(res[0], its[0])

    def match_compensated(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, T_init=None, options=None, rounds: int = 1,
                          **match_kw):
        """match() behind an exposure compensation of the current frame (plain Python over estimate_exposure, adjust_intensity and
        match; match itself is untouched).  Round 1 estimates gain and bias at T_init (reference -> current, the estimate; None:
        the identity), adjusts `current` and matches the adjusted pyramid from T_init.  Every further round estimates again at the
        result (the inverse of its Transformation), adjusts the ORIGINAL frame and matches from the result; like every T_init that
        start counts only with UseInitialEstimate (and a tracker configured so wants a T_init, as match does).  options: the exposure options (None, an ExposureOptions or a dict); a mask= among
        match_kw masks the estimate as well.  A degenerate estimate adjusts by (1, 0), which changes no bit.
        Returns (result, [one ExposureEstimate per round], the adjusted pyramid of the last round)."""
        if rounds < 1:
            raise ValueError("rounds must be at least 1")
        T, estimates, result, adjusted = T_init, [], None, None
        for _ in range(int(rounds)):
            estimate = current.estimate_exposure(reference, T=T, mask=match_kw.get("mask"), options=options, tracker=self)
            adjusted = current.adjust_intensity(estimate.gain, estimate.bias)
            result = self.match(reference, adjusted, T_init=T, **match_kw)
            estimates.append(estimate)
            if result.isNaN():
                break
            T = rigid_inverse(result.Transformation)
        return result, estimates, adjusted

    def alloc_results(self, n):
        """(result structs, per-iteration statistics arrays) for n pairs, reusable across match_batch(results=...) calls"""
        return self._alloc_results(n)

    def match_batch(self, references, currents, T_inits=None, stats: bool = True, in_flight: int = 0, raw: bool = False,
                    results=None, masks=None):
        """n independent match() calls on this tracker's GPU.  in_flight = 0: all advanced in lock step; otherwise at most
        in_flight pairs are resident and a finished pair hands its slot to the next one.  raw=True returns the array of C
        result structs as the library filled them (no per-pair Python objects: for throughput loops).  results: a pair from
        alloc_results(n) to fill (per-iteration statistics included) instead of allocating new ones.  masks: one SelectionMask
        or None per pair (dvo_amd_match_many_masked)."""
        n = len(references)
        assert len(currents) == n
        if results is not None:
            res, its = results
        elif stats:
            res, its = self._alloc_results(n)
        else:
            res, its = (CResult * n)(), [None] * n
        refs = (C.c_void_p * n)(*[r._h for r in references])
        curs = (C.c_void_p * n)(*[c._h for c in currents])
        T0 = None
        if T_inits is not None:
            T0a = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float64).T for T in T_inits]))
            T0 = T0a.ctypes.data_as(C.POINTER(C.c_double))
        if masks is not None:
            assert len(masks) == n
            ms = (C.c_void_p * n)(*[None if m is None else m._h for m in masks])
            _check(lib().dvo_amd_match_many_masked(self._h, n, refs, ms, curs, T0, res, in_flight), "dvo_amd_match_many_masked")
        else:
            _check(lib().dvo_amd_match_many(self._h, n, refs, curs, T0, res, in_flight), "dvo_amd_match_many")
        if raw:
            res._keepalive = its  # the iteration arrays the structs point into
            return res
        if not stats:
            return [Result(res[i], None) for i in range(n)]
        return [Result(res[i], its[i]) for i in range(n)]

    def submit(self, references, currents, T_inits=None, stats: bool = True, in_flight: int = 72, results=None):
        """dvo_amd_match_submit: queue n pairs behind whatever this tracker is still working on and return at once; the
        tracker keeps `in_flight` pairs resident across submissions (it never drains while it is fed).  Returns a
        Submission; wait(submission) / poll(submission) complete it."""
        n = len(references)
        assert len(currents) == n
        if results is not None:
            res, its = results
        elif stats:
            res, its = self._alloc_results(n)
        else:
            res, its = (CResult * n)(), [None] * n
        refs = (C.c_void_p * n)(*[r._h for r in references])
        curs = (C.c_void_p * n)(*[c._h for c in currents])
        T0, T0a = None, None
        if T_inits is not None:
            T0a = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float64).T for T in T_inits]))
            T0 = T0a.ctypes.data_as(C.POINTER(C.c_double))
        ticket = C.c_ulonglong()
        _check(lib().dvo_amd_match_submit(self._h, n, refs, curs, T0, res, in_flight, C.byref(ticket)), "dvo_amd_match_submit")
        sub = Submission(ticket.value, res, its, n)
        self._open[sub.ticket] = sub
        return sub

    def wait(self, submission=None, raw: bool = False):
        """dvo_amd_match_wait: drive the queue until the submission (None: everything submitted) is complete; returns its
        results (raw=True: the C result structs as the library filled them)."""
        try:
            _check(lib().dvo_amd_match_wait(self._h, 0 if submission is None else submission.ticket), "dvo_amd_match_wait")
        finally:  # complete, or dropped by a failed tick: either way the library is done with the result storage
            if submission is None:
                self._open.clear()
            else:
                self._open.pop(submission.ticket, None)
        return None if submission is None else submission.results(raw)

    def poll(self, submission=None) -> bool:
        """dvo_amd_match_poll: advance whatever has landed, never waiting for the GPU; True when the submission is complete"""
        done = C.c_int()
        try:
            _check(lib().dvo_amd_match_poll(self._h, 0 if submission is None else submission.ticket, C.byref(done)),
                   "dvo_amd_match_poll")
        except DvoAmdError:
            self._open.clear()  # a failed tick drops everything queued
            raise
        if done.value:
            if submission is None:
                self._open.clear()
            else:
                self._open.pop(submission.ticket, None)
        return bool(done.value)

    def track_frame(self, keyframe: RgbdImagePyramid, last_frame: RgbdImagePyramid, frame: RgbdImagePyramid,
                    last_keyframe_pose=None):
        """The two alignments of LocalTracker::update (local_tracker.cpp:170-186) as one two-pair batch:
        (r_keyframe, r_odometry, criteria) with criteria = the inputs of KeyframeTracker's accept callbacks."""
        res, its = self._alloc_results(2)
        crit = CFrameCriteria()
        P = None
        if last_keyframe_pose is not None:
            P = np.ascontiguousarray(np.asarray(last_keyframe_pose, dtype=np.float64).T)
        _check(lib().dvo_amd_track_frame(self._h, keyframe._h, last_frame._h, frame._h,
                                         P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None,
                                         C.byref(res[0]), C.byref(res[1]), C.byref(crit)), "dvo_amd_track_frame")
        criteria = {name: getattr(crit, name) for name, _ in CFrameCriteria._fields_}
        criteria["odometry_is_nan"], criteria["keyframe_is_nan"] = bool(crit.odometry_is_nan), bool(crit.keyframe_is_nan)
        return Result(res[0], its[0]), Result(res[1], its[1]), criteria

    def match_banded(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, n_bands: int, T_init=None) -> Result:
        """The tile-shard pipeline with all n_bands bands on this one GPU (verification of the multi-GPU path)."""
        res, its = self._alloc_results(1)
        T0 = None
        if T_init is not None:
            T0a = np.ascontiguousarray(np.asarray(T_init, dtype=np.float64).T)
            T0 = T0a.ctypes.data_as(C.POINTER(C.c_double))
        _check(lib().dvo_amd_match_banded(self._h, reference._h, current._h, T0, C.byref(res[0]), n_bands), "dvo_amd_match_banded")
        return Result(res[0], its[0])

    def comm_create(self, unique_id: bytes, nranks: int, rank: int):
        """Attach an RCCL communicator (one rank per GPU) for match_sharded."""
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        _check(lib().dvo_amd_comm_create(self._h, buf, nranks, rank), "dvo_amd_comm_create")

    def exchange_create(self, nranks: int, rank: int) -> bytes:
        """Allocate this rank's exchange buffer of the one-hop peer exchange; returns its 64-byte IPC handle."""
        buf = (C.c_ubyte * 64)()
        _check(lib().dvo_amd_exchange_create(self._h, nranks, rank, buf), "dvo_amd_exchange_create")
        return bytes(buf)

    def exchange_attach(self, handles):
        """handles: the 64-byte handles of all ranks in rank order (as all-gathered by the caller)."""
        blob = b"".join(handles)
        buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
        _check(lib().dvo_amd_exchange_attach(self._h, buf), "dvo_amd_exchange_attach")

    def match_sharded(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, T_init=None) -> Result:
        """One pair tile-sharded over the communicator's ranks; every rank calls this with the same arguments."""
        res, its = self._alloc_results(1)
        T0 = None
        if T_init is not None:
            T0a = np.ascontiguousarray(np.asarray(T_init, dtype=np.float64).T)
            T0 = T0a.ctypes.data_as(C.POINTER(C.c_double))
        _check(lib().dvo_amd_match_sharded(self._h, reference._h, current._h, T0, C.byref(res[0])), "dvo_amd_match_sharded")
        return Result(res[0], its[0])

    def score_poses(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, Ts, options: PoseScoreOptions) -> np.ndarray:
        """One POSE_SCORE_DTYPE record per hypothesis Ts[j] (4x4, reference -> current, the estimate) of the pair at
        options.level (dvo_amd_score_poses; the rule is pinned in include/dvo_amd.h under "Pose scoring")."""
        return self.score_poses_many([reference], [current], [Ts], [options])[0]

    def score_poses_many(self, references, currents, Ts, options) -> list:
        """n pairs in one call of two kernel launches (dvo_amd_score_poses_many): pair k is (references[k], currents[k]) under
        the hypotheses Ts[k] ([m_k, 4, 4]) and options[k].  Returns [the POSE_SCORE_DTYPE records of pair k]."""
        n = len(references)
        if not (len(currents) == len(Ts) == len(options) == n):
            raise ValueError("one current, one set of transformations and one option set per reference")
        vp = C.c_void_p
        stacks = [np.asarray(t, np.float64).reshape(-1, 4, 4) for t in Ts]
        m = np.array([len(t) for t in stacks] + [0], np.int32)[:max(1, n)]
        T = np.ascontiguousarray(np.concatenate(stacks).transpose(0, 2, 1) if n else np.zeros((0, 4, 4)))
        opts = (PoseScoreOptions * max(1, n))(*options)
        scores = np.zeros(max(1, len(T)), POSE_SCORE_DTYPE)
        _check(lib().dvo_amd_score_poses_many(self._h, n, (vp * max(1, n))(*[p._h for p in references]),
                                              (vp * max(1, n))(*[p._h for p in currents]), m.ctypes.data_as(C.POINTER(C.c_int)),
                                              T.ctypes.data_as(C.POINTER(C.c_double)), opts, scores.ctypes.data_as(vp)),
               "dvo_amd_score_poses_many")
        at = np.concatenate([[0], np.cumsum(m[:n])]).astype(int)
        return [scores[at[k]:at[k + 1]].copy() for k in range(n)]

    def residuals(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, level: int, T, mask: "SelectionMask | None" = None):
        """computeResidualsAndValidFlagsSse: (residuals[h, w, 2] with NaN = invalid, n_valid).  mask (test entry,
        dvo_amd_debug.h): the pass walks the points the mask leaves of the selection."""
        w, h, _ = reference.level_info(level)
        out = np.empty((h, w, 2), np.float32)
        Tf = np.ascontiguousarray(np.asarray(T, dtype=np.float64).astype(np.float32).T)
        n = C.c_int()
        if mask is None:
            _check(lib().dvo_amd_residuals(self._h, reference._h, current._h, level, _fp(Tf), _fp(out), C.byref(n)),
                   "dvo_amd_residuals")
        else:
            _check(lib().dvo_amd_debug_residuals_masked(self._h, reference._h, current._h, level, _fp(Tf), mask._h, _fp(out),
                                                        C.byref(n)), "dvo_amd_debug_residuals_masked")
        return out, n.value

    def iteration_probe(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, level: int, T, precision_in=None,
                        precision_eval=None, mask: "SelectionMask | None" = None):
        """One Gauss-Newton iteration body at the fixed pose T (dense_tracking.cpp:271-347 minus accept test and solve)
        through the kernels and host arithmetic match() uses: unit weights when precision_in is None, else t-distribution
        weights from the 2x2 precision_in.  precision_eval: evaluate A / b / ll with this 2x2 precision instead of the computed
        one.  mask: over the points the mask leaves of the selection.  Returns dict(n, scale, precision, ll, A, b, moments,
        scale_sums)."""
        Tf = np.ascontiguousarray(np.asarray(T, dtype=np.float64).astype(np.float32).T)
        pin = None if precision_in is None else np.ascontiguousarray(np.asarray(precision_in, np.float32).T).ravel()
        pev = None if precision_eval is None else np.ascontiguousarray(np.asarray(precision_eval, np.float32).T).ravel()
        pr = CIterationProbe()
        _check(lib().dvo_amd_debug_iteration_masked(self._h, reference._h, current._h, level, _fp(Tf),
                                                    None if pin is None else _fp(pin), None if pev is None else _fp(pev),
                                                    None if mask is None else mask._h, C.byref(pr)), "dvo_amd_debug_iteration")
        return {"n": pr.valid_constraints, "scale": np.array(pr.scale[:], np.float32).reshape(2, 2).T.copy(),
                "precision": np.array(pr.precision[:], np.float32).reshape(2, 2).T.copy(), "ll": float(pr.loglik),
                "A": np.array(pr.information[:]).reshape(6, 6).T.copy(), "b": np.array(pr.rhs[:]),
                "moments": np.array(pr.moments[:]), "scale_sums": np.array(pr.scale_sums[:]), "ll_sum": pr.loglik_sum}

    def hw_queue(self) -> int:
        """(diagnostic, dvo_amd_debug.h) pipe << 3 | queue of the hardware queue this tracker's main stream runs on, asked of the GPU"""
        q = C.c_int(-2)
        _check(lib().dvo_amd_debug_hw_queue(self._h, C.byref(q)), "dvo_amd_debug_hw_queue")
        return q.value

    def level_geometry(self, reference: RgbdImagePyramid, level: int):
        """(test entry, dvo_amd_debug.h) (64-point steps per wave segment, blocks of four segments, points the pass walks) of the
        residual pass on one level of `reference` under this tracker's configuration"""
        steps, blocks, points = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().dvo_amd_debug_level_geometry(self._h, reference._h, level, C.byref(steps), C.byref(blocks), C.byref(points)),
               "dvo_amd_debug_level_geometry")
        return steps.value, blocks.value, points.value

    def weights_probe(self, reference: RgbdImagePyramid, current: RgbdImagePyramid, level: int, T, precision_in,
                      mask: "SelectionMask | None" = None):
        """(test entry, dvo_amd_debug.h; host-rcpps mode only) the t-distribution weights of one residual pass at T under the 2x2
        precision_in as the product kernel formed them -- [h, w], NaN where the pixel is no constraint -- and what k_q7_tail did
        about the last V mod 4 of them (Q7): dict(n_tail, n, n_counted, recomputed_equal, pixel, w_table, w_exact, scale_sums_delta,
        moments_delta)"""
        w, h, _ = reference.level_info(level)
        out = np.empty((h, w), np.float32)
        Tf = np.ascontiguousarray(np.asarray(T, dtype=np.float64).astype(np.float32).T)
        pin = np.ascontiguousarray(np.asarray(precision_in, np.float32).T).ravel()
        q = CQ7Probe()
        _check(lib().dvo_amd_debug_weights_masked(self._h, reference._h, current._h, level, _fp(Tf), _fp(pin),
                                                  None if mask is None else mask._h, _fp(out), C.byref(q)), "dvo_amd_debug_weights")
        return out, {"n_tail": q.n_tail, "n": q.valid_constraints, "n_counted": q.valid_counted,
                     "recomputed_equal": bool(q.recomputed_equal), "pixel": list(q.pixel[:]),
                     "w_table": np.array(q.weight_table[:], np.float32), "w_exact": np.array(q.weight_exact[:], np.float32),
                     "scale_sums_delta": np.array(q.scale_sums_delta[:]), "moments_delta": np.array(q.moments_delta[:])}

    def ll_overflow_probe(self, residuals, n_blocks: int, steps: int, seg_first: int, n_segs: int, rank_offset: int, rank_end: int,
                          cut_rank: int, precision) -> bool:
        """(test entry, dvo_amd_debug.h) k_ll_overflow over a caller-supplied residual buffer [n_blocks * 4 * 64 * steps, 2] for
        the band of wave segments [seg_first, seg_first + n_segs); rank_end >= 0: a closed band"""
        r = np.ascontiguousarray(residuals, dtype=np.float32)
        assert r.shape == (n_blocks * 4 * 64 * steps, 2)
        P = np.ascontiguousarray(np.asarray(precision, np.float32).T).ravel()
        out = C.c_int(0)
        _check(lib().dvo_amd_debug_ll_overflow(self._h, _fp(r), n_blocks, steps, seg_first, n_segs, rank_offset, rank_end, cut_rank,
                                               _fp(P), C.byref(out)), "dvo_amd_debug_ll_overflow")
        return bool(out.value)

    def computeIntensityErrorImage(self, reference, current, T, level: int = 0) -> np.ndarray:
        w, h, _ = reference.level_info(level)
        out = np.empty((h, w), np.float32)
        Td = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T)
        _check(lib().dvo_amd_error_image(self._h, reference._h, current._h, Td.ctypes.data_as(C.POINTER(C.c_double)),
                                         level, _fp(out)), "dvo_amd_error_image")
        return out

    def bench_residual_pass(self, reference, current, level: int, T, n_items: int, rounds: int = 0, reps: int = 20):
        """Time the fused residual-pass kernel alone.  Returns (avg ms per repetition, algorithmic bytes, launches)."""
        Tf = np.ascontiguousarray(np.asarray(T, dtype=np.float64).astype(np.float32).T)
        ms, ab, nl = C.c_double(), C.c_double(), C.c_int()
        _check(lib().dvo_amd_bench_residual_pass(self._h, reference._h, current._h, level, _fp(Tf), n_items, rounds, reps,
                                                 C.byref(ms), C.byref(ab), C.byref(nl)), "dvo_amd_bench_residual_pass")
        return ms.value, ab.value, nl.value

    def bench_residual_pass_pairs(self, references, currents, level: int, T, rounds: int = 0, reps: int = 20):
        """The same over different (reference, current) pairs: nothing for the caches to deduplicate."""
        n = len(references)
        Tf = np.ascontiguousarray(np.asarray(T, dtype=np.float64).astype(np.float32).T)
        refs = (C.c_void_p * n)(*[r._h for r in references])
        curs = (C.c_void_p * n)(*[c._h for c in currents])
        ms, ab, nl = C.c_double(), C.c_double(), C.c_int()
        _check(lib().dvo_amd_bench_residual_pass_pairs(self._h, n, refs, curs, level, _fp(Tf), rounds, reps, C.byref(ms),
                                                       C.byref(ab), C.byref(nl)), "dvo_amd_bench_residual_pass_pairs")
        return ms.value, ab.value, nl.value

    def tick_log(self) -> np.ndarray:
        """Per-launch log of the timed k_tick launches: rows {ms, items, residual blocks, likelihood blocks, grid.x, px,
        64-pixel wave steps of the residual items, 64-pixel wave steps of the likelihood items}."""
        n = C.c_int()
        L = lib()
        L.dvo_amd_debug_tick_log.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
        _check(L.dvo_amd_debug_tick_log(self._h, None, 0, C.byref(n)), "tick_log")
        out = np.zeros((max(n.value, 1), 8))
        _check(L.dvo_amd_debug_tick_log(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)), "tick_log")
        return out[: n.value]

    def marker(self, tag: int = 0):
        """(profiling aid) a no-op dispatch named k_marker on this tracker's main stream (dvo_amd_debug.h)"""
        _check(lib().dvo_amd_debug_marker(self._h, int(tag)), "dvo_amd_debug_marker")

    def kernel_timing(self, enable: bool, reset: bool = False):
        ms = C.c_double()
        n = C.c_longlong()
        _check(lib().dvo_amd_kernel_timing(self._h, int(enable), C.byref(ms), C.byref(n), int(reset)), "kernel_timing")
        return ms.value, n.value


class KeyframeMap:
    """The keyframe map kept on the device (dvo_amd_map_*): keyframes are inserted, moved and removed one event at a time and
    extract() always equals DenseTracker.map_cloud over the keyframes now in the map, bit for bit.  Bound to `tracker`'s
    context (its stream and buffers); the tracker is kept alive by the map."""

    def __init__(self, tracker: "DenseTracker", leaf: float = 0.01):
        self._trk = tracker
        self._h = C.c_void_p()
        _check(lib().dvo_amd_map_create(tracker._h, leaf, C.byref(self._h)), "dvo_amd_map_create")
        self.leaf = leaf

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and getattr(self._trk, "_h", None):
            lib().dvo_amd_map_destroy(h)
            self._h = None

    def insert(self, id: int, pyramid: "RgbdImagePyramid", pose=None, bgr=None):
        """level 0 of `pyramid` at `pose` (4x4, None = identity), coloured from `bgr` (uint8 HxWx3, None = grey).  The map retains
        the pyramid and copies the image: both may be dropped right after the call."""
        ptr, stride = None, 0
        if bgr is not None:
            w, h, _ = pyramid.level_info(0)
            bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
            if bgr.shape != (h, w, 3):
                raise ValueError(f"bgr must be ({h}, {w}, 3) uint8")
            ptr, stride = bgr.ctypes.data, w * 3
        T = None if pose is None else _pose_cm(pose)
        _check(lib().dvo_amd_map_insert(self._h, id, pyramid._h, None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)),
                                        ptr, stride), "dvo_amd_map_insert")

    def set_poses(self, ids, poses):
        """new poses (4x4 each) of the keyframes `ids`, in one update"""
        ids = [int(i) for i in ids]
        if len(poses) != len(ids):
            raise ValueError("one pose per id")
        n = len(ids)
        arr = (C.c_int * max(1, n))(*ids)
        T = np.ascontiguousarray(np.stack([_pose_cm(P) for P in poses])) if n else np.zeros((1, 4, 4))
        _check(lib().dvo_amd_map_set_poses(self._h, n, arr, T.ctypes.data_as(C.POINTER(C.c_double))), "dvo_amd_map_set_poses")

    def remove(self, ids):
        ids = [int(i) for i in ids]
        arr = (C.c_int * max(1, len(ids)))(*ids)
        _check(lib().dvo_amd_map_remove(self._h, len(ids), arr), "dvo_amd_map_remove")

    def stats(self) -> dict:
        """the stats dict DenseTracker.map_cloud returns for the keyframes now in the map, and "keyframes" """
        st, n = CCloudStats(), C.c_int()
        _check(lib().dvo_amd_map_stats(self._h, C.byref(st), C.byref(n)), "dvo_amd_map_stats")
        return {"points_in": st.points_in, "finite": st.finite, "out_of_range": st.out_of_range, "voxels": st.voxels,
                "keyframes": n.value}

    def extract(self, box=None):
        """(xyz float32 [V, 3], rgb uint32 [V]) in voxel-key order; box = (xmin, ymin, zmin, xmax, ymax, zmax) keeps the voxels
        whose centroid lies in [min, max) on every axis"""
        bx = None
        if box is not None:
            bx = np.ascontiguousarray(box, dtype=np.float32).reshape(6)
        bp = None if bx is None else _fp(bx)
        n = C.c_longlong()
        cap = self.stats()["voxels"] if box is None else 0
        out = np.empty((max(1, cap), 4), np.float32)
        rc = lib().dvo_amd_map_extract(self._h, bp, out.ctypes.data, cap, C.byref(n))
        if rc == 7:  # DVO_AMD_ERR_CAPACITY: n is the size needed
            cap = int(n.value)
            out = np.empty((max(1, cap), 4), np.float32)
            rc = lib().dvo_amd_map_extract(self._h, bp, out.ctypes.data, cap, C.byref(n))
        _check(rc, "dvo_amd_map_extract")
        return _split_points(out[:n.value])

    def _view(self, K, width, height, near):
        fx, fy, ox, oy = [np.float32(k) for k in K]
        if near is None:
            near = max(np.float32(0.1), np.float32(self.leaf) * max(fx, fy) / np.float32(32))
        return CView(int(width), int(height), fx, fy, ox, oy, np.float32(near))

    def render(self, pose, K, width: int, height: int, near=None, planes=("depth", "rgb", "intensity", "index")):
        """The map seen from `pose` (4x4 camera -> world, None = identity) through K = (fx, fy, ox, oy): every voxel splatted
        over a square of its own size with a nearest-depth test (dvo_amd_map_render; the rule is pinned in dvo_amd.h).  A dict of
        the requested planes, [height, width] each -- depth float32 (NaN where empty), rgb uint32, intensity float32, index
        int32 (the voxel's position in extract(), -1 where empty) -- plus "stats".  near=None: max(0.1, leaf * max(fx, fy) / 32),
        the closest the rule admits."""
        kinds = {"depth": np.float32, "rgb": np.uint32, "intensity": np.float32, "index": np.int32}
        unknown = [p for p in planes if p not in kinds]
        if unknown:
            raise ValueError(f"unknown planes {unknown}")
        view = self._view(K, width, height, near)
        ok = view.width >= 1 and view.height >= 1 and view.width * view.height <= 1 << 26  # (the entry rejects the rest)
        out = {p: np.empty((view.height, view.width) if ok else (1, 1), kinds[p]) for p in kinds if p in planes}
        T = None if pose is None else _pose_cm(pose)
        st = CRenderStats()
        ptr = [out[p].ctypes.data if p in out else None for p in ("depth", "rgb", "intensity", "index")]
        _check(lib().dvo_amd_map_render(self._h, None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(view),
                                        ptr[0], ptr[1], ptr[2], ptr[3], C.byref(st)), "dvo_amd_map_render")
        out["stats"] = {n: getattr(st, n) for n, _ in CRenderStats._fields_}
        return out

    def render_pyramid(self, pose, K, width: int, height: int, levels: int, near=None, timestamp: float = 0.0):
        """The same view as an RgbdImagePyramid built on the device from the rendered planes: level 0's intensity and depth are
        render()'s (dvo_amd_map_render_pyramid).  `stats` of the render are left in the pyramid's `render_stats`."""
        view = self._view(K, width, height, near)
        T = None if pose is None else _pose_cm(pose)
        st = CRenderStats()
        pyr = RgbdImagePyramid.__new__(RgbdImagePyramid)
        pyr._h = C.c_void_p()
        _check(lib().dvo_amd_map_render_pyramid(self._h, None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)),
                                                C.byref(view), levels, timestamp, C.byref(pyr._h), C.byref(st)),
               "dvo_amd_map_render_pyramid")
        pyr.device = self._trk.device
        pyr.render_stats = {n: getattr(st, n) for n, _ in CRenderStats._fields_}
        return pyr

    def timing(self):
        """(diagnostic) the last call: (device ms of its kernels, ms of the output copy, delta points, delta voxels, merge tile)"""
        d, c, p, v, t = C.c_double(), C.c_double(), C.c_longlong(), C.c_longlong(), C.c_int()
        _check(lib().dvo_amd_debug_keyframe_map_timing(self._h, C.byref(d), C.byref(c), C.byref(p), C.byref(v), C.byref(t)),
               "dvo_amd_debug_keyframe_map_timing")
        return d.value, c.value, p.value, v.value, t.value


def volume_options(**options) -> VolumeOptions:
    """dvo_amd_default_volume_options (64^3 voxels of 0.05 m, origin (-1.6, -1.6, 0.4), trunc 0.15, near_z 0.4, far_z 5,
    VOLUME_WEIGHT_SENSOR) with the given fields replaced; origin: three floats"""
    opt = VolumeOptions()
    lib().dvo_amd_default_volume_options(C.byref(opt))
    for k, v in options.items():
        if k not in dict(VolumeOptions._fields_):
            raise TypeError(f"unknown volume option {k!r}")
        setattr(opt, k, (C.c_float * 3)(*[float(x) for x in v]) if k == "origin" else v)
    return opt


def volume_raycast_options(**options) -> VolumeRaycastOptions:
    """dvo_amd_default_volume_raycast_options (step_fraction 0.5, min_weight 1, fill_intensity 0) with the given fields replaced"""
    opt = VolumeRaycastOptions()
    lib().dvo_amd_default_volume_raycast_options(C.byref(opt))
    for k, v in options.items():
        if k not in dict(VolumeRaycastOptions._fields_):
            raise TypeError(f"unknown volume raycast option {k!r}")
        setattr(opt, k, v)
    return opt


def volume_timing(enable: bool = True, device: int = 0) -> dict:
    """(instrumentation) switches the event bracket around the launches of every SurfaceVolume call of `device` on or off; returns
    what the most recent such call enqueued of its own (`launches`, `synchronisations`) and the device time of the most recent
    bracketed call in ms (`ms`) (dvo_amd_debug_volume_timing)"""
    n, s, ms = C.c_int(), C.c_int(), C.c_double()
    _check(lib().dvo_amd_debug_volume_timing(device, int(enable), C.byref(n), C.byref(s), C.byref(ms)), "dvo_amd_debug_volume_timing")
    return dict(launches=n.value, synchronisations=s.value, ms=ms.value)


class SurfaceVolume:
    """A truncated signed-distance volume kept on one device (dvo_amd_volume_*; the rules are pinned in include/dvo_amd.h):
    keyframes are fused into a dense grid of integer sums -- inserted, moved and removed exactly, like KeyframeMap's -- which
    raycast() turns into a hole-free model view and extract() into surface points.  options: None, a VolumeOptions or a dict of
    its fields.  Context-free: no tracker is needed; calls on one volume are serialised by the caller."""

    def __init__(self, options=None, device: int = 0):
        self._h = C.c_void_p()
        self.options = options if isinstance(options, VolumeOptions) else volume_options(**(options or {}))
        self.device = device
        _check(lib().dvo_amd_volume_create(device, C.byref(self.options), C.byref(self._h)), "dvo_amd_volume_create")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dvo_amd_volume_destroy(h)
            self._h = None

    @property
    def shape(self):
        """(nz, ny, nx): the shape download() returns"""
        return self.options.nz, self.options.ny, self.options.nx

    @staticmethod
    def _frames(pyramids, poses):
        n = len(pyramids)
        if poses is not None and len(poses) != n:
            raise ValueError("one pose per pyramid")
        T = None
        if poses is not None:
            T = np.ascontiguousarray(np.stack([_pose_cm(np.eye(4) if P is None else P) for P in poses]) if n else np.zeros((1, 4, 4)))
        return n, (C.c_void_p * max(1, n))(*[p._h for p in pyramids]), T, None if T is None else T.ctypes.data_as(C.POINTER(C.c_double))

    def clear(self):
        """all records to zero; the keyframes of the tracked form are dropped"""
        _check(lib().dvo_amd_volume_clear(self._h), "dvo_amd_volume_clear")

    def integrate(self, pyramids, poses=None, level: int = 0, sign: int = 1):
        """the anonymous form: level `level` of every pyramid at its pose (4x4 camera -> world, None = identity) added (sign +1)
        or subtracted (-1) in one launch; returns a VOLUME_COUNTS_DTYPE array, one record per frame"""
        n, ph, T, Tp = self._frames(pyramids, poses)
        cnt = np.zeros(max(1, n), VOLUME_COUNTS_DTYPE)
        _check(lib().dvo_amd_volume_integrate(self._h, n, ph, level, Tp, sign, cnt.ctypes.data_as(C.POINTER(C.c_longlong))),
               "dvo_amd_volume_integrate")
        return cnt[:n].copy()

    def insert(self, ids, pyramids, poses=None, level: int = 0):
        """the tracked form: keyframes `ids` in one launch; the volume retains the pyramids.  Returns the counts as integrate()"""
        ids = [int(i) for i in ids]
        if len(ids) != len(pyramids):
            raise ValueError("one id per pyramid")
        n, ph, T, Tp = self._frames(pyramids, poses)
        cnt = np.zeros(max(1, n), VOLUME_COUNTS_DTYPE)
        _check(lib().dvo_amd_volume_insert(self._h, n, (C.c_int * max(1, n))(*ids), ph, level, Tp, cnt.ctypes.data_as(C.POINTER(C.c_longlong))),
               "dvo_amd_volume_insert")
        return cnt[:n].copy()

    def set_poses(self, ids, poses):
        """new poses (4x4 each) of the keyframes `ids`: subtracted at the old pose and added at the new one in one launch"""
        ids = [int(i) for i in ids]
        if len(poses) != len(ids):
            raise ValueError("one pose per id")
        n = len(ids)
        T = np.ascontiguousarray(np.stack([_pose_cm(P) for P in poses])) if n else np.zeros((1, 4, 4))
        _check(lib().dvo_amd_volume_set_poses(self._h, n, (C.c_int * max(1, n))(*ids), T.ctypes.data_as(C.POINTER(C.c_double))),
               "dvo_amd_volume_set_poses")

    def remove(self, ids):
        ids = [int(i) for i in ids]
        _check(lib().dvo_amd_volume_remove(self._h, len(ids), (C.c_int * max(1, len(ids)))(*ids)), "dvo_amd_volume_remove")

    def stats(self) -> dict:
        """{"keyframes", "updated_total"}: the keyframes of the tracked form and the sum of their `updated` counts"""
        n, total = C.c_int(), C.c_longlong()
        _check(lib().dvo_amd_volume_stats(self._h, C.byref(n), C.byref(total)), "dvo_amd_volume_stats")
        return {"keyframes": n.value, "updated_total": total.value}

    def download(self, box=None) -> np.ndarray:
        """the records as a VOLUME_VOXEL_DTYPE array [nz, ny, nx], or those of the inclusive index box (x0, y0, z0, x1, y1, z1)"""
        bx = None if box is None else (C.c_int * 6)(*[int(b) for b in box])
        shape = self.shape if box is None else tuple(max(0, int(box[3 + a]) - int(box[a]) + 1) for a in (2, 1, 0))
        out = np.zeros(shape, VOLUME_VOXEL_DTYPE)
        n = C.c_longlong()
        _check(lib().dvo_amd_volume_download(self._h, bx, out.ctypes.data, out.size, C.byref(n)), "dvo_amd_volume_download")
        return out

    def raycast(self, pose, K, width: int, height: int, near=None, options=None, planes=("depth", "intensity", "weight")):
        """The volume seen from `pose` (4x4 camera -> world, None = identity) through K = (fx, fy, ox, oy) (dvo_amd_volume_raycast):
        a dict of the requested planes, [height, width] each -- depth and intensity float32 (NaN where empty), weight int32 --
        plus "stats".  near=None: the volume's near_z.  options: None, a VolumeRaycastOptions or a dict of its fields."""
        kinds = {"depth": np.float32, "intensity": np.float32, "weight": np.int32}
        unknown = [p for p in planes if p not in kinds]
        if unknown:
            raise ValueError(f"unknown planes {unknown}")
        view = _warp_view((K, width, height), self.options.near_z if near is None else near)
        opt = options if isinstance(options, VolumeRaycastOptions) else volume_raycast_options(**(options or {}))
        ok = view.width >= 1 and view.height >= 1 and view.width * view.height <= 1 << 26  # (the entry rejects the rest)
        out = {p: np.empty((view.height, view.width) if ok else (1, 1), kinds[p]) for p in kinds if p in planes}
        T = None if pose is None else _pose_cm(pose)
        st = CVolumeRaycastStats()
        ptr = [out[p].ctypes.data_as(C.POINTER(C.c_float if p != "weight" else C.c_int)) if p in out else None
               for p in ("depth", "intensity", "weight")]
        _check(lib().dvo_amd_volume_raycast(self._h, None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(view),
                                            C.byref(opt), ptr[0], ptr[1], ptr[2], C.byref(st)), "dvo_amd_volume_raycast")
        out["stats"] = {n: getattr(st, n) for n, _ in CVolumeRaycastStats._fields_}
        return out

    def raycast_pyramid(self, pose, K, width: int, height: int, levels: int, near=None, options=None, timestamp: float = 0.0):
        """The same view as an RgbdImagePyramid built on the device from the raycast planes (dvo_amd_volume_raycast_pyramid): every
        pixel that is not hit and coloured is empty (depth NaN, intensity fill_intensity).  The stats are left in `raycast_stats`."""
        view = _warp_view((K, width, height), self.options.near_z if near is None else near)
        opt = options if isinstance(options, VolumeRaycastOptions) else volume_raycast_options(**(options or {}))
        T = None if pose is None else _pose_cm(pose)
        st = CVolumeRaycastStats()
        pyr = RgbdImagePyramid.__new__(RgbdImagePyramid)
        pyr._h = C.c_void_p()
        _check(lib().dvo_amd_volume_raycast_pyramid(self._h, None if T is None else T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(view),
                                                    C.byref(opt), levels, timestamp, C.byref(pyr._h), C.byref(st)),
               "dvo_amd_volume_raycast_pyramid")
        pyr.device, pyr.registration_stats = self.device, None
        pyr.raycast_stats = {n: getattr(st, n) for n, _ in CVolumeRaycastStats._fields_}
        return pyr

    def extract(self, min_weight: int = 1, capacity: int | None = None):
        """the surface crossings as (xyz float32 [n, 3], rgb uint32 [n], counts dict) in ascending 3*L + a (dvo_amd_volume_extract).
        capacity=None: asked of the library first; a given capacity that is too small raises DvoAmdError (status 7)"""
        n, cnt = C.c_longlong(), CVolumeExtractCounts()
        cap = 0 if capacity is None else int(capacity)
        out = np.empty((max(1, cap), 4), np.float32)
        rc = lib().dvo_amd_volume_extract(self._h, min_weight, out.ctypes.data, cap, C.byref(n), C.byref(cnt))
        if rc == 7 and capacity is None:  # DVO_AMD_ERR_CAPACITY: n is the size needed
            cap = int(n.value)
            out = np.empty((max(1, cap), 4), np.float32)
            rc = lib().dvo_amd_volume_extract(self._h, min_weight, out.ctypes.data, cap, C.byref(n), C.byref(cnt))
        self.last_extract_size = int(n.value)
        _check(rc, "dvo_amd_volume_extract")
        xyz, rgb = _split_points(out[:n.value])
        return xyz, rgb, {"points": cnt.points, "uncoloured": cnt.uncoloured}

    def mesh(self, min_weight: int = 1, normals: bool = True, capacity=None):
        """the surface as an indexed triangle mesh by surface nets (dvo_amd_volume_mesh): (xyz float32 [V, 3], rgb uint32 [V],
        normals float32 [V, 3] or None, triangles int32 [T, 3], counts dict); one vertex per active cell in ascending cell
        index, two triangles per crossing edge whose four cells are known.  capacity=None: asked of the library first; a given
        (vertices, triangles) that is too small raises DvoAmdError (status 7) with the sizes needed in `last_mesh_size`"""
        cnt = CVolumeMeshCounts()
        cap = (0, 0) if capacity is None else (int(capacity[0]), int(capacity[1]))

        def call():
            pts = np.empty((max(1, cap[0]), 4), np.float32)
            nrm = np.empty((max(1, cap[0]), 3), np.float32) if normals else None
            tri = np.empty((max(1, cap[1]), 3), np.int32)
            rc = lib().dvo_amd_volume_mesh(self._h, min_weight, pts.ctypes.data, None if nrm is None else _fp(nrm), cap[0],
                                           tri.ctypes.data_as(C.POINTER(C.c_int)), cap[1], C.byref(cnt))
            return rc, pts, nrm, tri

        rc, pts, nrm, tri = call()
        if rc == 7 and capacity is None:  # DVO_AMD_ERR_CAPACITY: the counts hold the sizes needed
            cap = (int(cnt.vertices), int(cnt.triangles))
            rc, pts, nrm, tri = call()
        self.last_mesh_size = (int(cnt.vertices), int(cnt.triangles))
        _check(rc, "dvo_amd_volume_mesh")
        xyz, rgb = _split_points(pts[:cnt.vertices])
        return (xyz, rgb, None if nrm is None else nrm[:cnt.vertices].copy(), tri[:cnt.triangles].copy(),
                {n: getattr(cnt, n) for n, _ in CVolumeMeshCounts._fields_})

    def upload(self, records, box=None):
        """the inverse of download(): overwrites the records of the volume, or of the inclusive index box (x0, y0, z0, x1, y1, z1),
        with a VOLUME_VOXEL_DTYPE array (or an integer array [..., 4]) in the order of L (dvo_amd_volume_upload).  Refused while
        the tracked form holds keyframes."""
        rec = np.asarray(records)
        if rec.dtype != VOLUME_VOXEL_DTYPE:
            if rec.ndim < 1 or rec.shape[-1] != 4 or rec.dtype.kind not in "iu" or rec.dtype.itemsize != 4:
                raise ValueError("records: a VOLUME_VOXEL_DTYPE array, or 32-bit integers [..., 4]")
            rec = np.ascontiguousarray(rec).view(VOLUME_VOXEL_DTYPE).reshape(rec.shape[:-1])
        rec = np.ascontiguousarray(rec)
        bx = None if box is None else (C.c_int * 6)(*[int(b) for b in box])
        _check(lib().dvo_amd_volume_upload(self._h, bx, rec.ctypes.data, rec.size), "dvo_amd_volume_upload")


def pack_keyframes(keyframes):
    """dvo_amd_keyframe records of objects with .pose and, where they have them, .id, .image and .evaluation (a
    constraints.Keyframe, or anything of that shape; an absent image becomes NULL)"""
    ckf = (CKeyframe * max(len(keyframes), 1))()
    for i, kf in enumerate(keyframes):
        image = getattr(kf, "image", None)
        ckf[i].id, ckf[i].image = int(getattr(kf, "id", i)), (image._h if image is not None else None)
        ckf[i].pose = (C.c_double * 16)(*_pose_cm(kf.pose).reshape(-1))
        ev = getattr(kf, "evaluation", None)
        if ev is not None:
            ckf[i].evaluation_kind, ckf[i].evaluation_average, ckf[i].evaluation_n = ev.kind, ev.average, ev.n
    return ckf


def covisibility_options(**options) -> CCovisibilityOptions:
    """dvo_amd_default_covisibility_options (level 3, near_z 0.1, depth_sigmas 20) with level / near_z / depth_sigmas replaced"""
    opt = CCovisibilityOptions()
    lib().dvo_amd_default_covisibility_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("level", "near_z", "depth_sigmas"):
            raise TypeError(f"unknown covisibility option {k!r}")
        setattr(opt, k, v)
    return opt


def covisibility(tracker, keyframes, pairs, **options) -> np.ndarray:
    """dvo_amd_covisibility: the eight counts (COVISIBILITY_DTYPE) of every ordered pair (a, b) of indices into `keyframes`,
    in one call.  overlap = covisibility_overlap(counts)."""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    out = np.zeros(len(pairs), COVISIBILITY_DTYPE)
    ip = C.POINTER(C.c_int)
    opt = covisibility_options(**options)
    _check(lib().dvo_amd_covisibility(tracker._h if tracker is not None else None, len(keyframes), pack_keyframes(keyframes),
                                      C.byref(opt), len(pairs), pa.ctypes.data_as(ip), pb.ctypes.data_as(ip),
                                      out.ctypes.data_as(C.c_void_p)), "dvo_amd_covisibility")
    return out


def covisibility_overlap(counts) -> np.ndarray:
    """consistent / valid in double, 0 where valid == 0 (the library's rule)"""
    c, v = counts["consistent"].astype(np.float64), counts["valid"].astype(np.float64)
    return np.where(v > 0, c / np.where(v > 0, v, 1.0), 0.0)


def covisibility_ms(tracker) -> float:
    """device milliseconds of k_covis in the tracker's last covisibility call"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_covisibility_ms(tracker._h, C.byref(ms)), "dvo_amd_debug_covisibility_ms")
    return ms.value


def find_constraint_candidates(tracker, keyframes, keyframe: int, max_distance: float, min_overlap: float = 0.0,
                               capacity: int | None = None, **options):
    """dvo_amd_find_constraint_candidates: (indices of the candidates in ascending order, their overlaps -- NaN when
    min_overlap <= 0).  tracker may be None when min_overlap <= 0: the radius search needs no device.  A capacity that is too
    small raises DvoAmdError (DVO_AMD_ERR_CAPACITY) whose `needed` is the size asked for."""
    capacity = len(keyframes) if capacity is None else capacity
    cand = np.zeros(max(capacity, 1), np.int32)
    over = np.zeros(max(capacity, 1), np.float64)
    n = C.c_int()
    opt = covisibility_options(**options)
    status = lib().dvo_amd_find_constraint_candidates(
        tracker._h if tracker is not None else None, len(keyframes), pack_keyframes(keyframes), keyframe, max_distance,
        min_overlap, C.byref(opt), cand.ctypes.data_as(C.POINTER(C.c_int)), over.ctypes.data_as(C.POINTER(C.c_double)),
        capacity, C.byref(n))
    if status != 0:
        err = DvoAmdError(status, "dvo_amd_find_constraint_candidates")
        err.needed = n.value
        raise err
    return [int(k) for k in cand[:n.value]], over[:n.value].copy()


def place_options(**options) -> PlaceOptions:
    """dvo_amd_default_place_options (level 3, gain 1) with the given fields replaced"""
    opt = PlaceOptions()
    lib().dvo_amd_default_place_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("level", "gain"):
            raise TypeError(f"unknown place option {k!r}")
        setattr(opt, k, int(v) if k == "level" else float(v))
    return opt


def place_query_options(**options) -> PlaceQueryOptions:
    """dvo_amd_default_place_query_options (k 5, min_score 0, exclude_recent 0) with the given fields replaced"""
    opt = PlaceQueryOptions()
    lib().dvo_amd_default_place_query_options(C.byref(opt))
    for k, v in options.items():
        if k not in ("k", "min_score", "exclude_recent"):
            raise TypeError(f"unknown place query option {k!r}")
        setattr(opt, k, float(v) if k == "min_score" else int(v))
    return opt


def place_timing(enable: bool = True, device: int = 0) -> float:
    """(instrumentation) switches the event bracket around the kernel launches of every PlaceIndex.scores / query / query_frames of
    `device` on or off and returns the device time of the most recent bracketed call in ms (dvo_amd_debug_place_timing)"""
    ms = C.c_double()
    _check(lib().dvo_amd_debug_place_timing(device, int(enable), C.byref(ms)), "dvo_amd_debug_place_timing")
    return ms.value


class PlaceIndex:
    """dvo_amd_place_index: loop-closure candidates by appearance.  One int8 descriptor per keyframe on the device (the rule is
    pinned in include/dvo_amd.h under "Place index"); ids are consecutive from 0 in insertion order; nothing is ever removed."""

    def __init__(self, level: int | None = None, gain: float | None = None, device: int = 0):
        options = {k: v for k, v in (("level", level), ("gain", gain)) if v is not None}
        opt = place_options(**options)
        self._h = C.c_void_p()
        _check(lib().dvo_amd_place_index_create(device, C.byref(opt), C.byref(self._h)), "dvo_amd_place_index_create")
        self.device, self.level, self.gain = device, opt.level, opt.gain

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().dvo_amd_place_index_destroy(h)
            self._h = None

    def add(self, pyramids) -> range:
        """the descriptors of `pyramids` appended in ONE kernel launch (dvo_amd_place_index_add); returns their ids"""
        pyramids = list(pyramids)
        n = len(pyramids)
        first = C.c_int()
        _check(lib().dvo_amd_place_index_add(self._h, n, (C.c_void_p * max(1, n))(*[p._h for p in pyramids]), C.byref(first)),
               "dvo_amd_place_index_add")
        return range(first.value, first.value + n)

    def info(self) -> dict:
        """{"size", "width", "height", "dim"}: width, height and dim are 0 before the first add"""
        v = [C.c_int() for _ in range(4)]
        _check(lib().dvo_amd_place_index_info(self._h, *[C.byref(x) for x in v]), "dvo_amd_place_index_info")
        return dict(zip(("size", "width", "height", "dim"), (x.value for x in v)))

    def __len__(self) -> int:
        return self.info()["size"]

    def _range(self, first, n):
        return int(first), len(self) - int(first) if n is None else int(n)

    def descriptors(self, first: int = 0, n: int | None = None):
        """(int8 [n, dim], int32 norms [n]) of rows first .. first + n (n None: to the end)"""
        first, n = self._range(first, n)
        dim = self.info()["dim"]
        rows, norms = np.zeros((max(n, 0), dim), np.int8), np.zeros(max(n, 0), np.int32)
        _check(lib().dvo_amd_place_index_download(self._h, first, n, rows.ctypes.data_as(C.POINTER(C.c_byte)),
                                                  norms.ctypes.data_as(C.POINTER(C.c_int))), "dvo_amd_place_index_download")
        return rows, norms

    def scores(self, query_ids, first: int = 0, n: int | None = None) -> np.ndarray:
        """the exact int32 dot products [len(query_ids), n] of the rows `query_ids` with rows first .. first + n"""
        first, n = self._range(first, n)
        ids = np.ascontiguousarray(query_ids, dtype=np.int32).reshape(-1)
        dots = np.zeros((len(ids), max(n, 0)), np.int32)
        _check(lib().dvo_amd_place_scores(self._h, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int)), first, n,
                                          dots.ctypes.data_as(C.POINTER(C.c_int))), "dvo_amd_place_scores")
        return dots

    @staticmethod
    def _query_options(options, k, min_score, exclude_recent):
        if isinstance(options, PlaceQueryOptions):
            return options
        given = {name: v for name, v in (("k", k), ("min_score", min_score), ("exclude_recent", exclude_recent)) if v is not None}
        return place_query_options(**given)

    @staticmethod
    def _found(nq, k):
        return np.full((nq, k), -1, np.int32), np.full((nq, k), np.nan, np.float64), np.zeros(max(nq, 1), np.int32)

    def query(self, ids, k: int | None = None, min_score: float | None = None, exclude_recent: int | None = None, options=None):
        """per row id of `ids` the k most similar other rows (dvo_amd_place_query): (candidates int32 [n, k], scores float64 [n, k],
        counts int32 [n]); behind counts[i] a row holds -1 / NaN.  A key within exclude_recent ids of the query is not eligible."""
        opt = self._query_options(options, k, min_score, exclude_recent)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        cand, score, counts = self._found(len(ids), max(opt.k, 1))
        ip = C.POINTER(C.c_int)
        _check(lib().dvo_amd_place_query(self._h, len(ids), ids.ctypes.data_as(ip), C.byref(opt), cand.ctypes.data_as(ip),
                                         score.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(ip)), "dvo_amd_place_query")
        return cand, score, counts[:len(ids)]

    def query_frames(self, pyramids, k: int | None = None, min_score: float | None = None, options=None):
        """query for pyramids that are not in the index (dvo_amd_place_query_frames): no key is excluded"""
        opt = self._query_options(options, k, min_score, None)
        pyramids = list(pyramids)
        n = len(pyramids)
        cand, score, counts = self._found(n, max(opt.k, 1))
        ip = C.POINTER(C.c_int)
        _check(lib().dvo_amd_place_query_frames(self._h, n, (C.c_void_p * max(1, n))(*[p._h for p in pyramids]), C.byref(opt),
                                                cand.ctypes.data_as(ip), score.ctypes.data_as(C.POINTER(C.c_double)),
                                                counts.ctypes.data_as(ip)), "dvo_amd_place_query_frames")
        return cand, score, counts[:n]


def se3_exp(xi) -> np.ndarray:
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    T = np.zeros(16)
    lib().dvo_amd_se3_exp(xi.ctypes.data_as(C.POINTER(C.c_double)), T.ctypes.data_as(C.POINTER(C.c_double)))
    return T.reshape(4, 4).T.copy()


def se3_log(T) -> np.ndarray:
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T)
    xi = np.zeros(6)
    lib().dvo_amd_se3_log(Tc.ctypes.data_as(C.POINTER(C.c_double)), xi.ctypes.data_as(C.POINTER(C.c_double)))
    return xi


def solve6(A, b) -> np.ndarray:
    Ac = np.ascontiguousarray(np.asarray(A, dtype=np.float64).T)
    bc = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(6)
    dp = C.POINTER(C.c_double)
    lib().dvo_amd_solve6(Ac.ctypes.data_as(dp), bc.ctypes.data_as(dp), x.ctypes.data_as(dp))
    return x


def comm_unique_id() -> bytes:
    buf = (C.c_ubyte * 128)()
    _check(lib().dvo_amd_comm_unique_id(buf), "dvo_amd_comm_unique_id")
    return bytes(buf)


def wire_layout():
    """(pieces, payload words) of a record on its way to the host: pieces of two {payload word, tick number} halves"""
    a, b = C.c_int(), C.c_int()
    _check(lib().dvo_amd_debug_wire_layout(C.byref(a), C.byref(b)), "wire_layout")
    return a.value, b.value


def take_wire(wire: np.ndarray, tick: int, from_piece: int, record: np.ndarray) -> int:
    """Host side of the record hand-off (host only): `wire` is a 16-byte aligned uint32 array [pieces, 4], `record` the uint32
    payload words collected so far; returns the first piece that does not carry `tick` yet."""
    up = C.POINTER(C.c_uint)
    assert wire.dtype == np.uint32 and record.dtype == np.uint32 and wire.flags.c_contiguous and record.flags.c_contiguous
    rc = lib().dvo_amd_debug_take_wire(wire.ctypes.data_as(up), tick, from_piece, record.ctypes.data_as(up))
    if rc < 0:
        _check(-rc, "take_wire")
    return rc


def tick_layout(res_blocks, ll_blocks, res_steps, ref_key, cur_key, share: int, max_blocks: int = 0) -> dict:
    """Where the blocks of one k_tick launch of these synthetic work items go (host only: dvo_amd_debug_tick_layout).  Returns
    order (launch position -> item), per launch position group_first / xcd_rot / tail_rot / set_size, compact, n_blocks and, for
    a compact grid, block_item / block_index per block of the grid (-1: a block that exits at once)."""
    ip = C.POINTER(C.c_int)
    ins = [np.ascontiguousarray(a, np.int32) for a in (res_blocks, ll_blocks, res_steps, ref_key, cur_key)]
    n = len(ins[0])
    assert all(len(a) == n for a in ins)
    order, rot, tail, size = (np.zeros(n, np.int32) for _ in range(4))
    first = np.zeros(n + 1, np.int32)
    compact, n_blocks = C.c_int(), C.c_int()
    cap = 8 * 65536
    b_item, b_index = np.full(cap, -2, np.int32), np.full(cap, -2, np.int32)
    p = lambda a: a.ctypes.data_as(ip)
    _check(lib().dvo_amd_debug_tick_layout(n, *[p(a) for a in ins], share, max_blocks, p(order), p(first), p(rot), p(tail), p(size),
                                           C.byref(compact), C.byref(n_blocks), cap, p(b_item), p(b_index)), "tick_layout")
    nb = n_blocks.value if compact.value else 0
    return dict(order=order, group_first=first, xcd_rot=rot, tail_rot=tail, set_size=size, compact=compact.value,
                n_blocks=n_blocks.value, block_item=b_item[:nb], block_index=b_index[:nb])


def combine_bands(bands) -> np.ndarray:
    """bands: [n, 10] = {valid, first_w, last_r0, last_r1, S[3], S_odd[3]} -> {valid, S[3], S_odd[3]} (host only)."""
    b = np.ascontiguousarray(bands, dtype=np.float64)
    out = np.zeros(7)
    dp = C.POINTER(C.c_double)
    _check(lib().dvo_amd_debug_combine_bands(b.shape[0], b.ctypes.data_as(dp), out.ctypes.data_as(dp)), "combine_bands")
    return out
