"""slam-sam_amd -- MI355X-native NDT scan-matching engine (Python host binding).

Thin ctypes layer over the C-ABI in include/ndt_hip.h (built in-tree as
slam-sam_amd/libndt_hip.so from slam-sam_amd/csrc).  The class below mirrors the
`pclomp::NormalDistributionsTransform` surface the reference's drivers use
(ref: run/pipeline.cpp:464-481,557-568; extern/svn_ndt/test/test_svn_ndt.cpp:144-179)
so tests read like the reference's own.  There is NO CPU fallback: importing
works anywhere, but if the HIP library is missing or no gfx950 device is present
every compute call raises.

The directory name has a hyphen; load it with `__graft_entry__.load_package()`
(registers the module as `slam_sam_amd`).
"""
import ctypes as C
import os
import sys

import numpy as np

from . import ranks  # noqa: F401  (one process per GPU without torch: launcher, slot board, HIP shim)
from . import synth  # noqa: F401  (seeded synthetic cloud generators)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NDT_HIP_LIB: tuning aid (A/B of two builds in one GPU session); the default is the in-tree build
LIB_PATH = os.environ.get("NDT_HIP_LIB") or os.path.join(_HERE, "libndt_hip.so")

EVAL_WORDS = 32
# pclomp::NeighborSearchMethod order
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3
HESSIAN_FULL, HESSIAN_GAUSS_NEWTON = 0, 1
COV_SVN, COV_PCL_RECALLED = 0, 1
WAIT_SPIN, WAIT_BLOCK = 0, 1
SOURCE_ORDER_AUTO, SOURCE_ORDER_KEEP, SOURCE_ORDER_SORT = 0, 1, 2
PRELAUNCH_AUTO, PRELAUNCH_OFF, PRELAUNCH_ONE_STREAM = 0, 1, 2
RECORDS_F64, RECORDS_PACKED48 = 0, 1
HANDOFF_ASYNC, HANDOFF_SYNC = 0, 1
PRESET_DEFAULT, PRESET_PCLOMP_RECALLED, PRESET_SVN = 0, 1, 2

STATUS = {0: "NDT_OK", -1: "NDT_ERR_INVALID_ARG", -2: "NDT_ERR_NO_DEVICE", -3: "NDT_ERR_HIP",
          -4: "NDT_ERR_NO_TARGET", -5: "NDT_ERR_NO_SOURCE", -6: "NDT_ERR_GRID_OVERFLOW",
          -7: "NDT_ERR_ALLOC", -8: "NDT_ERR_COMM", -9: "NDT_ERR_UNSUPPORTED"}


class NdtError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__("%s (%d): %s" % (STATUS.get(code, "?"), code, msg))


class Params(C.Structure):
    _fields_ = [
        ("resolution", C.c_float), ("step_size", C.c_double), ("trans_epsilon", C.c_double),
        ("max_iterations", C.c_int), ("outlier_ratio", C.c_double), ("search_method", C.c_int),
        ("min_points_per_voxel", C.c_int), ("eig_inflation_ratio", C.c_double),
        ("hessian_mode", C.c_int), ("cov_mode", C.c_int), ("add_ridge", C.c_int),
        ("use_line_search", C.c_int), ("regularization_scale_factor", C.c_float),
        ("num_threads", C.c_int), ("device_id", C.c_int), ("wait_mode", C.c_int), ("source_order", C.c_int),
        ("prelaunch", C.c_int),
    ]


class Result(C.Structure):
    _fields_ = [
        ("final_transformation", C.c_float * 16), ("final_pose", C.c_double * 6),
        ("converged", C.c_int), ("iterations", C.c_int), ("n_evaluations", C.c_int),
        ("hessian", C.c_double * 36), ("score", C.c_double), ("transform_probability", C.c_double),
        ("nearest_voxel_transformation_likelihood", C.c_double), ("n_pairs", C.c_int64),
        ("n_points_with_neighbors", C.c_int64), ("ms_total", C.c_double), ("ms_device", C.c_double),
        ("n_evaluations_reused", C.c_int),
    ]


class Score(C.Structure):
    _fields_ = [
        ("score", C.c_double), ("transform_probability", C.c_double),
        ("nearest_voxel_transformation_likelihood", C.c_double), ("n_pairs", C.c_int64),
        ("n_points_with_neighbors", C.c_int64),
    ]


class Fitness(C.Structure):
    _fields_ = [("fitness_score", C.c_double), ("sum_sq_dist", C.c_double), ("n_inliers", C.c_int64),
                ("n_points", C.c_int64)]


DBL_MAX = sys.float_info.max


class Leaf(C.Structure):
    _fields_ = [
        ("index", C.c_int64), ("point_count", C.c_int32), ("center", C.c_float * 3),
        ("mean", C.c_double * 3), ("cov", C.c_double * 9), ("icov", C.c_double * 9),
        ("evecs", C.c_double * 9), ("evals", C.c_double * 3),
    ]


class GridInfo(C.Structure):
    _fields_ = [
        ("min_b", C.c_int * 3), ("max_b", C.c_int * 3), ("div_b", C.c_int * 3),
        ("leaf_size", C.c_float), ("inverse_leaf_size", C.c_float), ("n_leaves", C.c_int64),
        ("n_cells", C.c_int64), ("n_target_points", C.c_int64), ("ms_build", C.c_double),
    ]


class MapInfo(C.Structure):
    _fields_ = [("leaf", C.c_float), ("with_intensity", C.c_int), ("n_voxels", C.c_int64), ("n_points", C.c_int64),
                ("n_points_dropped", C.c_int64), ("capacity", C.c_int64), ("min_ijk", C.c_int * 3),
                ("max_ijk", C.c_int * 3), ("n_adds", C.c_int64), ("n_grows", C.c_int64)]


class MapLevelStep(C.Structure):
    _fields_ = [("level", C.c_int), ("max_iterations", C.c_int), ("step_size", C.c_double)]


class MapCarveParams(C.Structure):
    """ndt_map_carve_params (ndt_map_carve_default_params: 2, 1, 4096, 0, 0)"""
    _fields_ = [("min_misses", C.c_int), ("keep_last", C.c_int), ("max_steps", C.c_int), ("protect_min_count", C.c_int),
                ("dry_run", C.c_int), ("reserved", C.c_int * 3)]


class ScanContextParams(C.Structure):
    """ndt_scan_context_params (ndt_scan_context_default_params: 20, 60, 80.0, +1.0, 2.0, 1)"""
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("max_radius", C.c_float), ("z_sign", C.c_float),
                ("lift", C.c_float), ("min_points_per_bin", C.c_int32)]


class GicpParams(C.Structure):
    """ndt_gicp_params (ndt_gicp_default_params: 20, +inf, 1e-3, 5.0, 1e-4, 64, 20)"""
    _fields_ = [("k_neighbours", C.c_int), ("max_neighbour_distance", C.c_double), ("covariance_epsilon", C.c_double),
                ("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("max_iterations", C.c_int), ("max_inner_iterations", C.c_int)]


class GicpInfo(C.Structure):
    _fields_ = [("outer_iterations", C.c_int), ("inner_iterations", C.c_int), ("n_evaluations", C.c_int),
                ("n_pairs", C.c_int64), ("n_source_without_covariance", C.c_int64),
                ("n_target_without_covariance", C.c_int64)]


GICP_SOURCE, GICP_TARGET = 0, 1


class VgicpInfo(C.Structure):
    _fields_ = [("n_voxels", C.c_int64), ("n_leaves", C.c_int64), ("n_target_points_in_voxels", C.c_int64),
                ("n_target_without_covariance", C.c_int64), ("n_source_without_covariance", C.c_int64),
                ("n_pairs", C.c_int64), ("n_source_with_pairs", C.c_int64)]


class MapCarveResult(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("n_rays_skipped", C.c_int64), ("n_steps", C.c_int64), ("n_voxels_crossed", C.c_int64),
                ("n_voxels_hit", C.c_int64), ("n_removed", C.c_int64), ("n_points_removed", C.c_int64)]


class MapComponentsParams(C.Structure):
    """ndt_map_components_params (ndt_map_components_default_params: 26, 1)"""
    _fields_ = [("connectivity", C.c_int), ("min_count", C.c_int), ("reserved", C.c_int * 2)]


class MapComponent(C.Structure):
    """ndt_map_component: one record of ndt_map_export_components (48 bytes)"""
    _fields_ = [("root_ijk", C.c_int32 * 3), ("n_voxels", C.c_int32), ("n_points", C.c_int64), ("min_ijk", C.c_int32 * 3),
                ("max_ijk", C.c_int32 * 3)]


class MapComponentsInfo(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("n_voxels_labelled", C.c_int64), ("n_voxels_unlabelled", C.c_int64),
                ("largest", C.c_int64), ("largest_n_voxels", C.c_int64), ("largest_n_points", C.c_int64)]


class MapComponentFilter(C.Structure):
    """ndt_map_component_filter (ndt_map_component_filter_default_params: 1, 0, 0, 0, 0 -- removes nothing)"""
    _fields_ = [("min_voxels", C.c_int32), ("min_points", C.c_int64), ("keep_largest", C.c_int32),
                ("remove_unlabelled", C.c_int32), ("dry_run", C.c_int32), ("reserved", C.c_int32 * 3)]


class MapRemoveComponentsResult(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("n_components_removed", C.c_int64), ("n_removed", C.c_int64),
                ("n_points_removed", C.c_int64)]


DESKEW_MAX_KNOTS = 64


class ScanFilter(C.Structure):
    """ndt_scan_filter: the acquisition filter of the deskew calls, on the raw coordinates.  A zeroed filter keeps every
    finite point."""
    _fields_ = [("use_box", C.c_int), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("use_z_or_intensity", C.c_int), ("z_min", C.c_float), ("z_max", C.c_float),
                ("intensity_keep_min", C.c_float)]

    @classmethod
    def from_vehicle_box(cls, center, dimensions, z_band=None, intensity_keep_min=None):
        """vehicleFilterBox as the drivers configure it (centre and dimensions: the box is centre -/+ dimensions / 2,
        None for no box), zAxisFilter as z_band = (z_min, z_max) and the reflectivity threshold; with a z band and no
        threshold the second alternative of the predicate never holds."""
        f = cls()
        if center is not None:
            c, d = np.asarray(center, np.float32), np.asarray(dimensions, np.float32)
            if c.shape != (3,) or d.shape != (3,):
                raise ValueError("center and dimensions must have 3 components")
            f.use_box = 1
            f.box_min[:] = [float(v) for v in c - d / np.float32(2)]
            f.box_max[:] = [float(v) for v in c + d / np.float32(2)]
        if z_band is not None or intensity_keep_min is not None:
            f.use_z_or_intensity = 1
            # (an empty band when only the threshold is given: z_min > z_max holds for no z)
            f.z_min, f.z_max = (float(z_band[0]), float(z_band[1])) if z_band is not None else (1.0, 0.0)
            f.intensity_keep_min = float("inf") if intensity_keep_min is None else float(intensity_keep_min)
        return f


class RangeGate(C.Structure):
    """ndt_range_gate: the range filter (metres, inclusive) and the channel stride of the unprojection calls.  A zeroed
    gate passes every pixel that has a return."""
    _fields_ = [("use_range", C.c_int), ("range_min", C.c_float), ("range_max", C.c_float), ("row_step", C.c_int)]

    def __init__(self, range_min=None, range_max=None, row_step=0):
        super().__init__()
        if range_min is not None or range_max is not None:
            self.use_range = 1
            self.range_min = 0.0 if range_min is None else float(range_min)
            self.range_max = np.inf if range_max is None else float(range_max)
        self.row_step = int(row_step)


LIDAR_PROFILE_RNG19, LIDAR_PROFILE_LEGACY = 0, 1


class PacketFrameInfo(C.Structure):
    """ndt_packet_frame_info: what the host pre-pass over a frame's packets found"""
    _fields_ = [("frame_id", C.c_int32), ("next_frame_pending", C.c_int32), ("t_ref", C.c_double), ("ts_first", C.c_double),
                ("ts_last", C.c_double)] + [(k, C.c_int64) for k in (
                    "n_columns", "n_packets", "n_packets_accepted", "n_packets_bad_size", "n_packets_bad_type", "n_columns_bad_id",
                    "n_columns_bad_frame", "n_columns_bad_status", "n_columns_overridden")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Timing(C.Structure):
    _fields_ = [
        ("ms_last_eval_kernel", C.c_double), ("ms_last_reduce_kernel", C.c_double),
        ("ms_last_build", C.c_double), ("n_eval_launches", C.c_int64),
        ("ms_eval_kernel_total", C.c_double), ("ms_reduce_kernel_total", C.c_double),
        ("n_timed_evals", C.c_int64),
    ]


class HandoffLaneTiming(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("bytes_in", C.c_int64), ("bytes_dma", C.c_int64),
                ("ms_repack", C.c_double), ("ms_dma", C.c_double), ("dma_gb_per_s", C.c_double),
                ("threads", C.c_int)]


class HandoffTiming(C.Structure):
    _fields_ = [("target", HandoffLaneTiming), ("source", HandoffLaneTiming), ("ms_build_wait", C.c_double),
                ("mode", C.c_int), ("cpu_budget", C.c_int), ("repack_workers", C.c_int)]


class SvnParams(C.Structure):
    _fields_ = [("particle_count", C.c_int), ("max_iterations", C.c_int),
                ("kernel_bandwidth", C.c_double), ("step_size", C.c_double),
                ("stop_threshold", C.c_double)]


class SvnResult(C.Structure):
    _fields_ = [("final_pose", C.c_double * 16), ("final_covariance", C.c_double * 36),
                ("converged", C.c_int), ("iterations", C.c_int), ("last_mean_update", C.c_double),
                ("ms_total", C.c_double), ("ms_stage1", C.c_double), ("ms_stage2", C.c_double),
                ("ms_stage3", C.c_double)]


class Tuning(C.Structure):
    """ndt_tuning (include/ndt_hip.h): the engine's A/B switches.  The library reads none of them from the environment."""
    _fields_ = [(k, C.c_int) for k in (
        "deriv_block", "deriv_summer", "deriv_dedicated", "deriv_single_level_max", "deriv_xcd", "bucket_build",
        "bucket_tile", "fused_sort", "bounds_blocks", "bounds_unroll", "finalize_threads", "build_events",
        "build_wait_sync", "mbox_tagged", "mbox_preload", "prelaunch_streams", "prelaunch_probe", "speculate_first",
        "timing_bracket", "handoff_chunk_pass", "deriv_summer_split", "deriv_one_block_per_cu")] + [("reserved", C.c_int * 10)]


# the variables the tuning programs under tools/ (and bench.py's rehearsals) have always used, mapped onto ndt_tuning by
# apply_env_tuning() -- in Python, on request: the C library itself does not look at them
TUNING_ENV = {
    "NDT_DERIV_BLOCK": "deriv_block", "NDT_DERIV_SUMMER": "deriv_summer", "NDT_DERIV_DEDICATED": "deriv_dedicated",
    "NDT_DERIV_SINGLE_LEVEL_MAX": "deriv_single_level_max", "NDT_DERIV_XCD": "deriv_xcd",
    "NDT_BUCKET_BUILD": "bucket_build", "NDT_BUCKET_TILE": "bucket_tile", "NDT_FUSED_SORT": "fused_sort",
    "NDT_BOUNDS_BLOCKS": "bounds_blocks", "NDT_BOUNDS_UNROLL": "bounds_unroll",
    "NDT_FINALIZE_THREADS": "finalize_threads", "NDT_BUILD_EVENTS": "build_events",
    "NDT_MBOX_TAGGED": "mbox_tagged", "NDT_MBOX_PRELOAD": "mbox_preload",
    "NDT_PRELAUNCH_STREAMS": "prelaunch_streams", "NDT_PRELAUNCH_PROBE": "prelaunch_probe",
    "NDT_SPECULATE_FIRST": "speculate_first", "NDT_TIMING_BRACKET": "timing_bracket",
    "NDT_HANDOFF_CHUNK_PASS": "handoff_chunk_pass", "NDT_DERIV_SUMMER_SPLIT": "deriv_summer_split",
    "NDT_DERIV_ONE_BLOCK_PER_CU": "deriv_one_block_per_cu",
}


def get_tuning():
    t = Tuning()
    rc = lib().ndt_get_tuning(C.byref(t))
    if rc:
        raise NdtError(rc, "ndt_get_tuning")
    return {k: getattr(t, k) for k, _ in Tuning._fields_ if k != "reserved"}


def set_tuning(**fields):
    """ndt_set_tuning with the named fields changed; applies to the handles created and the builds / evaluations begun afterwards."""
    t = Tuning()
    rc = lib().ndt_get_tuning(C.byref(t))
    if rc:
        raise NdtError(rc, "ndt_get_tuning")
    for k, v in fields.items():
        if k == "reserved" or not hasattr(t, k):
            raise KeyError(k)
        setattr(t, k, int(v))
    rc = lib().ndt_set_tuning(C.byref(t))
    if rc:
        raise NdtError(rc, "ndt_set_tuning(%s)" % fields)
    return get_tuning()


def apply_env_tuning(environ=None):
    """For tuning programs and test harnesses: NDT_* variables of the historical names -> ndt_set_tuning."""
    env = os.environ if environ is None else environ
    fields = {f: int(env[k]) for k, f in TUNING_ENV.items() if env.get(k, "") != ""}
    if env.get("NDT_BUILD_WAIT", "") != "":
        fields["build_wait_sync"] = 1 if env["NDT_BUILD_WAIT"] == "sync" else 0
    return set_tuning(**fields) if fields else get_tuning()


EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int,
                      C.POINTER(C.c_double))
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)
EVAL_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_float),
                            C.POINTER(C.c_int), C.POINTER(C.c_double))
ALIGN_BATCH_MAX = 256

# every symbol include/ndt_hip.h declares
ABI_SYMBOLS = [
    "ndt_abi_version", "ndt_default_params", "ndt_create", "ndt_destroy", "ndt_set_params",
    "ndt_get_params", "ndt_last_error", "ndt_backend_info", "ndt_set_target", "ndt_set_target_soa",
    "ndt_set_target_device", "ndt_set_target_device_deferred", "ndt_set_source", "ndt_set_source_soa", "ndt_set_source_device", "ndt_set_source_device_view",
    "ndt_set_regularization_pose", "ndt_clear_regularization_pose", "ndt_align",
    "ndt_eval_derivatives", "ndt_unpack_eval", "ndt_transform_source", "ndt_get_grid_info",
    "ndt_export_leaves", "ndt_newton_align", "ndt_shard_range", "ndt_comm_unique_id",
    "ndt_comm_init_rccl", "ndt_comm_init_shm", "ndt_comm_init_hook", "ndt_comm_destroy",
    "ndt_set_global_source_size", "ndt_enable_kernel_timing", "ndt_get_timing",
    "ndt_svn_default_params", "ndt_svn_sample_particles", "ndt_svn_align",
    "ndt_multigrid_add_target", "ndt_multigrid_remove_target", "ndt_multigrid_count", "ndt_multigrid_create_kdtree",
    "ndt_keyframe_put", "ndt_keyframe_erase", "ndt_keyframe_count", "ndt_set_target_from_keyframes",
    "ndt_result_covariance", "ndt_set_source_from_keyframe",
    "ndt_params_preset", "ndt_score_transform", "ndt_comm_info", "ndt_score_transforms",
    "ndt_xy_covariance_laplace", "ndt_propose_poses_to_search", "ndt_xy_covariance_multi_ndt",
    "ndt_xy_covariance_multi_ndt_score", "ndt_source_changed", "ndt_comm_rank_count", "ndt_comm_p2p_handle", "ndt_comm_init_p2p",
    "ndt_set_record_format", "ndt_get_record_format",
    "ndt_set_handoff_mode", "ndt_get_handoff_mode", "ndt_wait", "ndt_get_handoff_timing",
    "ndt_voxel_downsample_device", "ndt_voxel_downsample", "ndt_get_iteration_history",
    "ndt_get_tuning", "ndt_set_tuning", "ndt_set_keepwarm", "ndt_get_keepwarm",
    "ndt_comm_p2p_selftest", "ndt_comm_p2p_stats", "ndt_angle_tables", "ndt_gauss_constants", "ndt_svn_rbf_kernel",
    "ndt_fitness_score", "ndt_fitness_scores", "ndt_newton_align_batch", "ndt_align_batch",
    "ndt_score_points", "ndt_score_points_device", "ndt_source_size", "ndt_filter_source_device", "ndt_filter_source",
    "ndt_map_reset", "ndt_map_clear", "ndt_map_add", "ndt_map_add_device", "ndt_map_add_keyframe", "ndt_map_get_info",
    "ndt_map_export_device", "ndt_map_export", "ndt_set_target_from_map",
    "ndt_map_enable_moments", "ndt_map_has_moments", "ndt_map_export_moments", "ndt_set_target_from_map_moments",
    "ndt_trajectory_pose", "ndt_deskew_device", "ndt_deskew", "ndt_keyframe_put_deskewed",
    "ndt_scan_model_set", "ndt_scan_model_clear", "ndt_scan_model_get_info", "ndt_scan_model_from_beams",
    "ndt_unproject_device", "ndt_unproject", "ndt_keyframe_put_from_ranges",
    "ndt_packet_columns", "ndt_packet_format_set", "ndt_packet_format_get", "ndt_packet_size", "ndt_packet_frame_begin",
    "ndt_packet_frame_push", "ndt_packet_frame_get_info", "ndt_decode_packet_frame_device",
    "ndt_unproject_packet_frame_device", "ndt_unproject_packet_frame", "ndt_keyframe_put_from_packets",
    "ndt_map_crop", "ndt_map_export_state", "ndt_map_export_state_device", "ndt_map_import_state", "ndt_map_import_state_device",
    "ndt_map_carve_default_params", "ndt_map_carve_device", "ndt_map_carve", "ndt_map_carve_keyframe",
    "ndt_map_components_default_params", "ndt_map_component_filter_default_params", "ndt_map_components",
    "ndt_map_export_components", "ndt_map_export_labels", "ndt_map_export_labels_device", "ndt_map_label_points",
    "ndt_map_label_points_device", "ndt_map_remove_components",
    "ndt_map_transform", "ndt_map_import_state_posed", "ndt_map_import_state_posed_device",
    "ndt_map_level_info", "ndt_map_export_state_level", "ndt_map_export_state_level_device", "ndt_set_target_from_map_level",
    "ndt_map_coarsen", "ndt_map_levels_drop", "ndt_align_map_levels",
    "ndt_set_source_distributions", "ndt_set_source_distributions_device", "ndt_source_distributions_info",
    "ndt_export_source_distributions", "ndt_eval_derivatives_d2d", "ndt_align_d2d",
    "ndt_set_source_times", "ndt_set_source_times_device", "ndt_source_times_info", "ndt_eval_derivatives_ct", "ndt_align_ct",
    "ndt_transform_source_ct", "ndt_transform_source_ct_device",
    "ndt_gicp_default_params", "ndt_gicp_set_params", "ndt_gicp_get_params", "ndt_gicp_export_neighbours",
    "ndt_gicp_export_covariances", "ndt_gicp_pair", "ndt_gicp_export_pairs", "ndt_eval_derivatives_gicp", "ndt_align_gicp",
    "ndt_vgicp_export_voxels", "ndt_vgicp_get_info", "ndt_eval_derivatives_vgicp", "ndt_align_vgicp",
    "ndt_scan_context_default_params", "ndt_scan_context_set_params", "ndt_scan_context_get_params",
    "ndt_scan_context_sector_table", "ndt_scan_context", "ndt_scan_context_device", "ndt_scan_context_keyframe",
    "ndt_scan_context_bank_put", "ndt_scan_context_bank_get", "ndt_scan_context_bank_erase", "ndt_scan_context_bank_clear",
    "ndt_scan_context_bank_count", "ndt_scan_context_match", "ndt_scan_context_match_keyframe",
]

_lib = None


def lib():
    """The C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("slam-sam_amd: %s is missing -- run __graft_entry__.build() "
                              "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        fp, dp, vp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p
        L.ndt_abi_version.restype = C.c_int
        L.ndt_comm_p2p_selftest.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
        L.ndt_comm_p2p_stats.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
        L.ndt_set_keepwarm.argtypes = [vp, C.c_int]
        L.ndt_get_keepwarm.argtypes = [vp, C.POINTER(C.c_longlong)]
        L.ndt_get_tuning.argtypes = [C.POINTER(Tuning)]
        L.ndt_set_tuning.argtypes = [C.POINTER(Tuning)]
        L.ndt_default_params.argtypes = [C.POINTER(Params)]
        L.ndt_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
        L.ndt_destroy.argtypes = [vp]
        L.ndt_set_params.argtypes = [vp, C.POINTER(Params)]
        L.ndt_get_params.argtypes = [vp, C.POINTER(Params)]
        L.ndt_last_error.restype = C.c_char_p
        L.ndt_last_error.argtypes = [vp]
        L.ndt_backend_info.argtypes = [C.c_char_p, C.c_size_t]
        L.ndt_set_target.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
        L.ndt_set_target_soa.argtypes = [vp, vp, vp, vp, C.c_size_t]
        L.ndt_set_target_device.argtypes = [vp, vp, vp, vp, C.c_size_t]
        L.ndt_set_target_device_deferred.argtypes = [vp, vp, vp, vp, C.c_size_t]
        L.ndt_set_source.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
        L.ndt_set_source_soa.argtypes = [vp, vp, vp, vp, C.c_size_t]
        L.ndt_set_source_device.argtypes = [vp, vp, vp, vp, C.c_size_t]
        L.ndt_set_source_device_view.argtypes = [vp, vp, vp, vp, C.c_size_t]
        L.ndt_source_changed.argtypes = [vp]
        L.ndt_set_record_format.argtypes = [vp, C.c_int]
        L.ndt_get_record_format.argtypes = [vp]
        L.ndt_set_regularization_pose.argtypes = [vp, fp]
        L.ndt_clear_regularization_pose.argtypes = [vp]
        L.ndt_align.argtypes = [vp, fp, C.POINTER(Result)]
        L.ndt_eval_derivatives.argtypes = [vp, dp, fp, C.c_int, C.c_int, dp]
        L.ndt_unpack_eval.restype = None
        L.ndt_unpack_eval.argtypes = [dp, dp, dp, dp]
        L.ndt_transform_source.argtypes = [vp, fp, fp, C.c_size_t]
        L.ndt_fitness_score.argtypes = [vp, fp, C.c_double, C.POINTER(Fitness), fp, C.c_size_t]
        L.ndt_fitness_scores.argtypes = [vp, fp, C.c_int, C.c_double, C.POINTER(Fitness)]
        L.ndt_align_batch.argtypes = [vp, fp, C.c_int, C.POINTER(Result)]
        L.ndt_score_points.argtypes = [vp, fp, vp, vp, vp, vp, C.c_size_t]
        L.ndt_score_points_device.argtypes = [vp, fp, vp, vp, vp, vp, C.c_size_t]
        L.ndt_source_size.restype = C.c_int64
        L.ndt_source_size.argtypes = [vp]
        L.ndt_filter_source_device.argtypes = [vp, fp, C.c_double, C.c_int, vp, vp, vp, vp, C.c_size_t,
                                               C.POINTER(C.c_size_t)]
        L.ndt_filter_source.argtypes = [vp, fp, C.c_double, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_newton_align_batch.argtypes = [C.POINTER(Params), C.c_int64, fp, C.c_int, fp, EVAL_BATCH_FN, vp,
                                             C.POINTER(Result)]
        L.ndt_get_grid_info.argtypes = [vp, C.POINTER(GridInfo)]
        L.ndt_export_leaves.restype = C.c_int64
        L.ndt_export_leaves.argtypes = [vp, C.POINTER(Leaf), C.c_size_t]
        L.ndt_newton_align.argtypes = [C.POINTER(Params), C.c_int64, fp, fp, EVAL_FN, vp,
                                       C.POINTER(Result)]
        L.ndt_shard_range.restype = None
        L.ndt_shard_range.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t)]
        L.ndt_comm_unique_id.argtypes = [vp]
        L.ndt_comm_init_rccl.argtypes = [vp, vp, C.c_int, C.c_int]
        L.ndt_comm_init_shm.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.ndt_comm_init_hook.argtypes = [vp, ALLREDUCE_FN, vp, C.c_int, C.c_int]
        L.ndt_comm_destroy.argtypes = [vp]
        L.ndt_set_global_source_size.argtypes = [vp, C.c_int64]
        L.ndt_enable_kernel_timing.argtypes = [vp, C.c_int]
        L.ndt_get_timing.argtypes = [vp, C.POINTER(Timing)]
        L.ndt_multigrid_add_target.argtypes = [vp, C.c_int64, vp, C.c_size_t, C.c_size_t]
        L.ndt_multigrid_remove_target.argtypes = [vp, C.c_int64]
        L.ndt_multigrid_count.restype = C.c_int64
        L.ndt_multigrid_count.argtypes = [vp]
        L.ndt_multigrid_create_kdtree.argtypes = [vp]
        L.ndt_keyframe_put.argtypes = [vp, C.c_int64, vp, C.c_size_t, C.c_size_t]
        L.ndt_keyframe_erase.argtypes = [vp, C.c_int64]
        L.ndt_keyframe_count.restype = C.c_int64
        L.ndt_keyframe_count.argtypes = [vp]
        L.ndt_set_target_from_keyframes.argtypes = [vp, C.POINTER(C.c_int64), dp, C.c_int]
        L.ndt_set_source_from_keyframe.argtypes = [vp, C.c_int64]
        L.ndt_svn_default_params.restype = None
        L.ndt_svn_default_params.argtypes = [C.POINTER(SvnParams)]
        L.ndt_svn_sample_particles.argtypes = [dp, C.c_int, C.c_uint64, dp]
        L.ndt_svn_align.argtypes = [vp, C.POINTER(SvnParams), dp, dp, C.POINTER(SvnResult)]
        L.ndt_result_covariance.argtypes = [dp, C.c_double, C.c_int, dp]
        L.ndt_params_preset.argtypes = [C.POINTER(Params), C.c_int]
        L.ndt_score_transform.argtypes = [vp, fp, C.POINTER(Score)]
        L.ndt_comm_info.argtypes = [C.c_char_p, C.c_size_t]
        L.ndt_comm_rank_count.argtypes = [vp]
        L.ndt_comm_p2p_handle.argtypes = [vp, vp]
        L.ndt_comm_init_p2p.argtypes = [vp, vp, C.c_int, C.c_int]
        L.ndt_score_transforms.argtypes = [vp, fp, C.c_int, C.POINTER(Score)]
        L.ndt_xy_covariance_laplace.argtypes = [dp, dp]
        L.ndt_propose_poses_to_search.argtypes = [C.POINTER(Result), dp, dp, C.c_int, fp]
        L.ndt_xy_covariance_multi_ndt.argtypes = [vp, C.POINTER(Result), fp, C.c_int, dp, dp]
        L.ndt_xy_covariance_multi_ndt_score.argtypes = [vp, C.POINTER(Result), fp, C.c_int, C.c_double, dp, dp]
        L.ndt_voxel_downsample_device.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_float, vp, vp, vp, vp, C.c_size_t,
                                                  C.POINTER(C.c_size_t)]
        L.ndt_voxel_downsample.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_long, C.c_float, vp, C.c_size_t,
                                           C.POINTER(C.c_size_t)]
        L.ndt_get_iteration_history.argtypes = [vp, fp, dp, dp, C.c_int]
        L.ndt_map_reset.argtypes = [vp, C.c_float, C.c_int, C.c_int64]
        L.ndt_map_clear.argtypes = [vp]
        L.ndt_map_add.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_long, dp]
        L.ndt_map_add_device.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, dp]
        L.ndt_map_add_keyframe.argtypes = [vp, C.c_int64, dp]
        L.ndt_map_get_info.argtypes = [vp, C.POINTER(MapInfo)]
        L.ndt_map_export_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_map_export.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_long, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_set_target_from_map.argtypes = [vp, C.c_int]
        L.ndt_map_enable_moments.argtypes = [vp]
        L.ndt_map_has_moments.argtypes = [vp]
        L.ndt_map_export_moments.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_set_target_from_map_moments.argtypes = [vp, fp, fp]
        L.ndt_map_crop.argtypes = [vp, fp, fp, C.c_int, C.POINTER(C.c_int64)]
        L.ndt_map_export_state.argtypes = [vp, fp, fp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_map_export_state_device.argtypes = [vp, fp, fp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_map_import_state.argtypes = [vp, C.c_float, vp, vp, vp, vp, C.c_size_t]
        L.ndt_map_import_state_device.argtypes = [vp, C.c_float, vp, vp, vp, vp, C.c_size_t]
        L.ndt_map_transform.argtypes = [vp, dp, C.POINTER(C.c_int64)]
        L.ndt_map_import_state_posed.argtypes = [vp, C.c_float, vp, vp, vp, vp, C.c_size_t, dp]
        L.ndt_map_import_state_posed_device.argtypes = [vp, C.c_float, vp, vp, vp, vp, C.c_size_t, dp]
        L.ndt_map_level_info.argtypes = [vp, C.c_int, C.POINTER(MapInfo)]
        L.ndt_map_export_state_level.argtypes = [vp, C.c_int, fp, fp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_map_export_state_level_device.argtypes = [vp, C.c_int, fp, fp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_set_target_from_map_level.argtypes = [vp, C.c_int, fp, fp]
        L.ndt_map_coarsen.argtypes = [vp, C.c_int]
        L.ndt_map_levels_drop.argtypes = [vp]
        L.ndt_align_map_levels.argtypes = [vp, C.POINTER(MapLevelStep), C.c_int, fp, fp, C.POINTER(Result)]
        L.ndt_set_source_distributions.argtypes = [vp, vp, vp, C.c_size_t]
        L.ndt_set_source_distributions_device.argtypes = [vp, vp, vp, C.c_size_t]
        L.ndt_source_distributions_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ndt_export_source_distributions.argtypes = [vp, dp, dp, vp, vp, C.c_size_t]
        L.ndt_export_source_distributions.restype = C.c_int64
        L.ndt_eval_derivatives_d2d.argtypes = [vp, dp, C.c_int, C.c_int, dp]
        L.ndt_align_d2d.argtypes = [vp, fp, C.POINTER(Result)]
        L.ndt_set_source_times.argtypes = [vp, vp, C.c_size_t]
        L.ndt_set_source_times_device.argtypes = [vp, vp, C.c_size_t]
        L.ndt_source_times_info.restype = C.c_int64
        L.ndt_source_times_info.argtypes = [vp]
        L.ndt_eval_derivatives_ct.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp]
        L.ndt_align_ct.argtypes = [vp, dp, fp, C.POINTER(Result)]
        L.ndt_transform_source_ct.argtypes = [vp, dp, dp, C.c_int, vp, C.c_size_t]
        L.ndt_transform_source_ct_device.argtypes = [vp, dp, dp, C.c_int, vp, vp, vp, C.c_size_t]
        gpp = C.POINTER(GicpParams)
        L.ndt_gicp_default_params.restype = None
        L.ndt_gicp_default_params.argtypes = [gpp]
        L.ndt_gicp_set_params.argtypes = [vp, gpp]
        L.ndt_gicp_get_params.argtypes = [vp, gpp]
        L.ndt_gicp_export_neighbours.argtypes = [vp, C.c_int, vp, vp, C.c_size_t]
        L.ndt_gicp_export_neighbours.restype = C.c_int64
        L.ndt_gicp_export_covariances.argtypes = [vp, C.c_int, dp, dp, dp, C.c_size_t]
        L.ndt_gicp_export_covariances.restype = C.c_int64
        L.ndt_gicp_pair.argtypes = [vp, dp, C.POINTER(C.c_int64)]
        L.ndt_gicp_export_pairs.argtypes = [vp, vp, vp, C.c_size_t]
        L.ndt_gicp_export_pairs.restype = C.c_int64
        L.ndt_eval_derivatives_gicp.argtypes = [vp, dp, C.c_int, C.c_int, dp]
        L.ndt_align_gicp.argtypes = [vp, fp, C.POINTER(Result), C.POINTER(GicpInfo)]
        L.ndt_vgicp_export_voxels.argtypes = [vp, vp, dp, dp, C.c_size_t]
        L.ndt_vgicp_export_voxels.restype = C.c_int64
        L.ndt_vgicp_get_info.argtypes = [vp, C.POINTER(VgicpInfo)]
        L.ndt_eval_derivatives_vgicp.argtypes = [vp, dp, C.c_int, C.c_int, dp]
        L.ndt_align_vgicp.argtypes = [vp, fp, C.POINTER(Result), C.POINTER(VgicpInfo)]
        scp, i64 = C.POINTER(ScanContextParams), C.c_int64
        L.ndt_scan_context_default_params.restype = None
        L.ndt_scan_context_default_params.argtypes = [scp]
        L.ndt_scan_context_set_params.argtypes = [vp, scp]
        L.ndt_scan_context_get_params.argtypes = [vp, scp]
        L.ndt_scan_context_sector_table.argtypes = [C.c_int, fp]
        L.ndt_scan_context.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, vp]
        L.ndt_scan_context_device.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp]
        L.ndt_scan_context_keyframe.argtypes = [vp, i64, fp, vp]
        L.ndt_scan_context_bank_put.argtypes = [vp, i64, fp]
        L.ndt_scan_context_bank_get.argtypes = [vp, i64, fp]
        L.ndt_scan_context_bank_erase.argtypes = [vp, i64]
        L.ndt_scan_context_bank_clear.argtypes = [vp]
        L.ndt_scan_context_bank_count.argtypes = [vp]
        L.ndt_scan_context_bank_count.restype = i64
        L.ndt_scan_context_match.argtypes = [vp, fp, vp, dp, vp, vp, C.c_size_t]
        L.ndt_scan_context_match.restype = i64
        L.ndt_scan_context_match_keyframe.argtypes = [vp, i64, vp, dp, vp, vp, C.c_size_t]
        L.ndt_scan_context_match_keyframe.restype = i64
        L.ndt_map_carve_default_params.restype = None
        L.ndt_map_carve_default_params.argtypes = [C.POINTER(MapCarveParams)]
        L.ndt_map_carve_device.argtypes = [vp, vp, vp, vp, C.c_size_t, fp, dp, C.POINTER(MapCarveParams),
                                           C.POINTER(MapCarveResult)]
        L.ndt_map_carve.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, dp, C.POINTER(MapCarveParams),
                                    C.POINTER(MapCarveResult)]
        L.ndt_map_carve_keyframe.argtypes = [vp, C.c_int64, fp, dp, C.POINTER(MapCarveParams), C.POINTER(MapCarveResult)]
        ccp, szp = C.POINTER(MapComponentsParams), C.POINTER(C.c_size_t)
        L.ndt_map_components_default_params.restype = None
        L.ndt_map_components_default_params.argtypes = [ccp]
        L.ndt_map_component_filter_default_params.restype = None
        L.ndt_map_component_filter_default_params.argtypes = [C.POINTER(MapComponentFilter)]
        L.ndt_map_components.argtypes = [vp, ccp, C.POINTER(MapComponentsInfo)]
        L.ndt_map_export_components.argtypes = [vp, ccp, C.POINTER(MapComponent), C.c_size_t, szp]
        L.ndt_map_export_labels.argtypes = [vp, ccp, vp, vp, C.c_size_t, szp]
        L.ndt_map_export_labels_device.argtypes = [vp, ccp, vp, vp, C.c_size_t, szp]
        L.ndt_map_label_points.argtypes = [vp, ccp, vp, C.c_size_t, C.c_size_t, dp, vp, C.POINTER(C.c_int64)]
        L.ndt_map_label_points_device.argtypes = [vp, ccp, vp, vp, vp, C.c_size_t, dp, vp, C.POINTER(C.c_int64)]
        L.ndt_map_remove_components.argtypes = [vp, ccp, C.POINTER(MapComponentFilter), C.POINTER(MapRemoveComponentsResult)]
        L.ndt_trajectory_pose.argtypes = [dp, dp, C.c_int, dp, C.c_double, dp]
        traj = [dp, dp, C.c_int, dp, C.POINTER(ScanFilter)]
        L.ndt_deskew_device.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t] + traj + [vp, vp, vp, vp, vp, C.c_size_t,
                                                                                      C.POINTER(C.c_size_t)]
        L.ndt_deskew.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_long, vp] + traj + [vp, vp, C.c_size_t,
                                                                                         C.POINTER(C.c_size_t)]
        L.ndt_keyframe_put_deskewed.argtypes = [vp, C.c_int64, vp, C.c_size_t, C.c_size_t, C.c_long, vp] + traj + [
            C.POINTER(C.c_size_t)]
        L.ndt_scan_model_set.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp]
        L.ndt_scan_model_clear.argtypes = [vp]
        L.ndt_scan_model_get_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ndt_scan_model_from_beams.argtypes = [C.c_int, C.c_int, fp, fp, C.c_double, dp, fp, fp, fp, fp, fp, fp]
        ranges = [vp, vp, vp, C.POINTER(RangeGate)] + traj
        L.ndt_unproject_device.argtypes = [vp] + ranges + [vp, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_unproject.argtypes = [vp] + ranges + [vp, C.c_size_t, C.c_long, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_keyframe_put_from_ranges.argtypes = [vp, C.c_int64] + ranges + [C.POINTER(C.c_size_t)]
        L.ndt_packet_columns.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, C.c_size_t, C.c_double, vp, vp,
                                         C.POINTER(PacketFrameInfo)]
        L.ndt_packet_format_set.argtypes = [vp, C.c_int, C.c_int]
        L.ndt_packet_format_get.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ndt_packet_size.argtypes = [vp]
        L.ndt_packet_size.restype = C.c_size_t
        L.ndt_packet_frame_begin.argtypes = [vp]
        L.ndt_packet_frame_push.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_packet_frame_get_info.argtypes = [vp, C.POINTER(PacketFrameInfo)]
        L.ndt_decode_packet_frame_device.argtypes = [vp, vp, vp, vp, vp, vp]
        gated = [C.POINTER(RangeGate)] + traj
        L.ndt_unproject_packet_frame_device.argtypes = [vp] + gated + [vp] * 8 + [C.c_size_t, C.POINTER(C.c_size_t)]
        L.ndt_unproject_packet_frame.argtypes = [vp] + gated + [vp, C.c_size_t, C.c_long, vp, vp, vp, vp, C.c_size_t,
                                                                 C.POINTER(C.c_size_t)]
        L.ndt_keyframe_put_from_packets.argtypes = [vp, C.c_int64] + gated + [vp, vp, C.POINTER(C.c_size_t)]
        L.ndt_set_handoff_mode.argtypes = [vp, C.c_int]
        L.ndt_get_handoff_mode.argtypes = [vp]
        L.ndt_wait.argtypes = [vp]
        L.ndt_get_handoff_timing.argtypes = [vp, C.POINTER(HandoffTiming)]
        L.ndt_debug_prelaunch_counters.argtypes = [vp, C.POINTER(C.c_int64)]  # test seam, not in the header
        L.ndt_debug_build_counters.argtypes = [vp, C.POINTER(C.c_int64)]  # test seam, not in the header
        L.ndt_debug_speculation_counters.argtypes = [vp, C.POINTER(C.c_int64)]  # test seam, not in the header
        if hasattr(L, "ndt_debug_handoff_counters"):   # (a library of an earlier round under NDT_HIP_LIB has none)
            L.ndt_debug_handoff_counters.argtypes = [vp, C.POINTER(C.c_int64)]  # test seam, not in the header
        L.ndt_debug_set_speculation.argtypes = [vp, C.c_int]  # tuning aid, not in the header
        L.ndt_debug_sort_pairs.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, vp]  # test seam, not in the header
        # test seams, not in the header: launch plans of k_derivatives, the XCD chunk map, the evaluation log
        L.ndt_debug_launch_shape.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.ndt_debug_launch_plan.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.ndt_debug_xcd_chunk.argtypes = [C.c_int] * 5
        L.ndt_debug_xcd_chunk_map.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
        L.ndt_debug_eval_log.argtypes = [vp, C.c_int]
        L.ndt_debug_eval_log_read.argtypes = [vp, vp, C.c_int]
        L.ndt_debug_eval_log_read.restype = C.c_int64
        _lib = L
    return _lib


# DerivLaunchPlan (csrc/ndt_kernels.h): the shape of one k_derivatives launch, 16 ints in this order
EVAL_DESC_FIELDS = ("batch", "mode", "nb", "mbox", "threads", "blocks", "point_blocks", "summers", "doubling_split",
                    "xcd_count", "xcd_stripe", "two_level", "safe_sum", "dyn_lds", "cus", "spec")
# EvalLogEntry (csrc/ndt_engine.h): one logged evaluation
EVAL_LOG_DTYPE = np.dtype([("pose6", "<f8", 6), ("words", "<f8", EVAL_WORDS), ("T", "<f4", 16), ("launch", "<i8"),
                           ("k", "<i4"), ("K", "<i4"), ("need_h", "<i4"), ("score_only", "<i4"), ("prelaunched", "<i4"),
                           ("pad", "<i4"), ("plan", "<i4", len(EVAL_DESC_FIELDS))])
assert EVAL_LOG_DTYPE.itemsize == 464


def debug_launch_plan(n_src, K=1, cus=256, nb=1, mode=1, batched=None, mbox=False, safe_sum=False):
    """Test seam: the plan of a k_derivatives launch (dict over EVAL_DESC_FIELDS) for n_src points and K poses on a
    single-rank handle of `cus` compute units under the current ndt_tuning -- nb / mode: the template axes (NB 0 DIRECT1,
    1 DIRECT7, 2 KDTREE, 3 DIRECT26, 4 multi-grid, 5 / 6 packed DIRECT1 / DIRECT7; MODE 0 gradient, 1 Hessian, 2 Gauss-
    Newton, 3 score only).  batched defaults to K > 1."""
    out = (C.c_int * len(EVAL_DESC_FIELDS))()
    flags = (1 if (K > 1 if batched is None else batched) else 0) | (2 if mbox else 0) | (4 if safe_sum else 0)
    rc = lib().ndt_debug_launch_plan(int(n_src), int(K), int(cus), int(nb), int(mode), flags, out)
    if rc:
        raise NdtError(rc, "ndt_debug_launch_plan")
    return dict(zip(EVAL_DESC_FIELDS, out))


def debug_launch_shape(n_src, K=1, cus=256):
    """Test seam: (threads per block, point blocks, summing blocks, grid blocks per pose) of a k_derivatives launch."""
    out = (C.c_int * 4)()
    rc = lib().ndt_debug_launch_shape(int(n_src), int(K), int(cus), out)
    if rc:
        raise NdtError(rc, "ndt_debug_launch_shape")
    return tuple(out)


def debug_xcd_chunk(p, L, off, X, m):
    """Test seam: xcd_chunk(p, L, off, X, m) of csrc/ndt_device.h, called on the host."""
    r = lib().ndt_debug_xcd_chunk(int(p), int(L), int(off), int(X), int(m))
    if r < 0:
        raise NdtError(r, "ndt_debug_xcd_chunk")
    return r


def debug_xcd_chunk_map(L, off, X, m):
    """Test seam: [xcd_chunk(p, L, off, X, m) for p in range(L)] in one call."""
    out = np.zeros(int(L), np.int32)
    rc = lib().ndt_debug_xcd_chunk_map(int(L), int(off), int(X), int(m), out.ctypes.data_as(C.POINTER(C.c_int)))
    if rc:
        raise NdtError(rc, "ndt_debug_xcd_chunk_map")
    return out


def default_params(preset=None, **kw):
    p = Params()
    lib().ndt_default_params(C.byref(p))
    if preset is not None:
        rc = lib().ndt_params_preset(C.byref(p), int(preset))
        if rc != 0:
            raise NdtError(rc, "ndt_params_preset")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def comm_info():
    """(ncclGetVersion code, path of the shared object serving the nccl* symbols of the engine)."""
    buf = C.create_string_buffer(512)
    v = lib().ndt_comm_info(buf, 512)
    return v, buf.value.decode()


def backend_info():
    buf = C.create_string_buffer(256)
    n = lib().ndt_backend_info(buf, 256)
    return n, buf.value.decode()


def _trajectory_args(knot_t, knot_poses, ref_pose):
    """(knot_t [n] f64, poses [n * 16] f64 column-major, n, ref [16] f64 or None) as the C-ABI takes a trajectory"""
    kt = np.ascontiguousarray(knot_t, dtype=np.float64).ravel()
    kp = np.asarray(knot_poses, dtype=np.float64)
    if kp.ndim == 2 and kp.shape == (4, 4):
        kp = kp[None]
    if kp.ndim != 3 or kp.shape[1:] != (4, 4) or len(kp) != len(kt):
        raise ValueError("knot_poses must be n_knots x 4 x 4, one pose per knot time")
    poses = np.ascontiguousarray(np.transpose(kp, (0, 2, 1))).ravel()
    ref = None
    if ref_pose is not None:
        r = np.asarray(ref_pose, dtype=np.float64)
        if r.shape != (4, 4):
            raise ValueError("ref_pose must be 4 x 4")
        ref = np.ascontiguousarray(r.T).ravel()
    return kt, poses, len(kt), ref


def trajectory_pose(knot_t, knot_poses, t, ref_pose=None):
    """D(t) = ref^-1 T(t) of the deskew model as a 4 x 4 float64 matrix (host only, no device): knot poses body -> map,
    position blended linearly, attitude by slerp, t clamped to the knots; ref_pose None = the last knot."""
    kt, poses, n, ref = _trajectory_args(knot_t, knot_poses, ref_pose)
    out = np.zeros(16, np.float64)
    rc = lib().ndt_trajectory_pose(_dp(kt), _dp(poses), n, None if ref is None else _dp(ref), float(t), _dp(out))
    if rc != 0:
        raise NdtError(rc, "ndt_trajectory_pose")
    return out.reshape(4, 4).T.copy()


def scan_model_from_beams(n_cols, beam_azimuth_deg, beam_altitude_deg, lidar_origin_to_beam_origin_mm, lidar_to_body=None):
    """The unprojection tables of a spinning lidar as the drivers' lidar callback computes them (host only, no device):
    p = range_m * (x1, y1, z1)[col, row] + (x2, y2, z2)[col].  One azimuth and one altitude angle per row, in degrees;
    lidar_to_body: 4 x 4 (None: the identity).  Returns (x1, y1, z1 [n_cols, n_rows], x2, y2, z2 [n_cols]) float32, what
    setScanModel takes."""
    az = np.ascontiguousarray(beam_azimuth_deg, dtype=np.float32).ravel()
    alt = np.ascontiguousarray(beam_altitude_deg, dtype=np.float32).ravel()
    if len(az) != len(alt):
        raise ValueError("one azimuth and one altitude angle per row")
    n_cols, n_rows = int(n_cols), len(az)
    T = np.eye(4) if lidar_to_body is None else np.asarray(lidar_to_body, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("lidar_to_body must be 4 x 4")
    T16 = np.ascontiguousarray(T.T).ravel()
    shape = (max(n_cols, 0), n_rows)
    x1, y1, z1 = (np.zeros(shape, np.float32) for _ in range(3))
    x2, y2, z2 = (np.zeros(shape[0], np.float32) for _ in range(3))
    rc = lib().ndt_scan_model_from_beams(n_cols, n_rows, _fp(az), _fp(alt), float(lidar_origin_to_beam_origin_mm), _dp(T16),
                                         _fp(x1), _fp(y1), _fp(z1), _fp(x2), _fp(y2), _fp(z2))
    if rc != 0:
        raise NdtError(rc, "ndt_scan_model_from_beams")
    return x1, y1, z1, x2, y2, z2


def _packet_array(packets):
    """(uint8 array [k, stride], sizes [k] size_t, stride) of a 2-D uint8 array (every packet as long as a row) or of a
    sequence of bytes-like payloads of any lengths (padded with zeros to the longest)"""
    if isinstance(packets, np.ndarray) and packets.ndim == 2:
        a = np.ascontiguousarray(packets, dtype=np.uint8)
        return a, np.full(len(a), a.shape[1], np.uintp), a.shape[1]
    rows = [np.frombuffer(bytes(p), np.uint8) for p in packets]
    stride = max([len(r) for r in rows] + [1])
    a = np.zeros((len(rows), stride), np.uint8)
    for k, r in enumerate(rows):
        a[k, :len(r)] = r
    return a, np.array([len(r) for r in rows], np.uintp), stride


def packet_columns(profile, columns_per_packet, n_cols, n_rows, packets, t_ref=None):
    """The host pre-pass over a frame's UDP payloads (host only, no device; ndt_packet_columns): packets as a uint8 array
    [k, bytes] or a sequence of bytes-like payloads, t_ref None: the first accepted column's time.  Returns (col_src int32
    [n_cols]: dword offset of the column's first pixel in the packed packet buffer, -1: none; col_t float32 [n_cols], NaN:
    none; info dict)."""
    a, sizes, stride = _packet_array(packets)
    src, col_t = np.full(max(int(n_cols), 0), -1, np.int32), np.full(max(int(n_cols), 0), np.nan, np.float32)
    info = PacketFrameInfo()
    rc = lib().ndt_packet_columns(int(profile), int(columns_per_packet), int(n_cols), int(n_rows), a.ctypes.data, sizes.ctypes.data,
                                  len(a), stride, float("nan") if t_ref is None else float(t_ref), src.ctypes.data,
                                  col_t.ctypes.data, C.byref(info))
    if rc != 0:
        raise NdtError(rc, "ndt_packet_columns")
    return src, col_t, info.as_dict()


def shard_range(n, rank, nranks):
    b, c = C.c_size_t(), C.c_size_t()
    lib().ndt_shard_range(n, rank, nranks, C.byref(b), C.byref(c))
    return b.value, c.value


def _colmajor(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).T).ravel()


class ColMajor4f:
    """A 4x4 transform already converted to the ABI's 16 column-major floats (what
    Eigen::Matrix4f::data() is for the C++ callers): lets a loop convert its guess once."""

    def __init__(self, T):
        self.a = _colmajor(T)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _host_cloud(cloud, intensity_column=None):
    """A host cloud as the C ABI takes it: (the N x >= 3 contiguous float32 array, stride_bytes, intensity_offset_bytes;
    -1: none).  NumPy reports strides of 0 for an empty array, and the calls that accept n = 0 still check the stride."""
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be N x >=3 float32")
    if intensity_column is not None and not 3 <= int(intensity_column) < a.shape[1]:
        raise ValueError("intensity_column outside the cloud's columns")
    off = -1 if intensity_column is None else 4 * int(intensity_column)
    return a, (a.strides[0] if len(a) else a.itemsize * a.shape[1]), off


def unpack_eval(words):
    """32 packed doubles -> dict(score, gradient[6], hessian[6,6], nvtl_sum, n_with, n_pairs)."""
    w = np.ascontiguousarray(words, dtype=np.float64)
    g = np.zeros(6)
    H = np.zeros(36)
    s = C.c_double()
    lib().ndt_unpack_eval(_dp(w), C.byref(s), _dp(g), _dp(H))
    return dict(score=s.value, gradient=g, hessian=H.reshape(6, 6), nvtl_sum=w[28],
                n_with_neighbors=int(w[29]), n_pairs=int(w[30]))


def result_to_dict(r):
    return dict(T=np.array(r.final_transformation[:], dtype=np.float64).reshape(4, 4).T.copy(),
                pose=np.array(r.final_pose[:]), converged=bool(r.converged),
                iterations=r.iterations, n_evaluations=r.n_evaluations,
                hessian=np.array(r.hessian[:]).reshape(6, 6), score=r.score,
                transform_probability=r.transform_probability,
                nvtl=r.nearest_voxel_transformation_likelihood, n_pairs=r.n_pairs,
                n_points_with_neighbors=r.n_points_with_neighbors, ms_total=r.ms_total,
                ms_device=r.ms_device, n_evaluations_reused=r.n_evaluations_reused)


class NormalDistributionsTransform:
    """pclomp::NormalDistributionsTransform-shaped engine on one MI355X."""

    def __init__(self, device_id=-1, **params):
        self._p = default_params(device_id=device_id, **params)
        self._h = C.c_void_p()
        rc = lib().ndt_create(C.byref(self._p), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise NdtError(rc, "ndt_create failed (a gfx950 device is required; no CPU fallback)")
        self._raw, self._cooked = None, None
        self._keep = []
        self.last_unproject_count = 0      # *n_out of the last unprojectDevice call, also when it was refused

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ndt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise NdtError(rc, lib().ndt_last_error(self._h).decode())

    def _push(self):
        self._check(lib().ndt_set_params(self._h, C.byref(self._p)))

    # --- setters the drivers call (ref: run/pipeline.cpp:467-480) ---
    def setNumThreads(self, n): self._p.num_threads = int(n); self._push()
    def getNumThreads(self): return self._p.num_threads
    def setResolution(self, r): self._p.resolution = float(r); self._push()
    def getResolution(self): return self._p.resolution
    def setStepSize(self, s): self._p.step_size = float(s); self._push()
    def setTransformationEpsilon(self, e): self._p.trans_epsilon = float(e); self._push()
    def setMaximumIterations(self, n): self._p.max_iterations = int(n); self._push()
    def setOutlierRatio(self, o): self._p.outlier_ratio = float(o); self._push()
    def setNeighborhoodSearchMethod(self, m): self._p.search_method = int(m); self._push()
    def setMinPointPerVoxel(self, n): self._p.min_points_per_voxel = int(n); self._push()
    def setRegularizationScaleFactor(self, k): self._p.regularization_scale_factor = float(k); self._push()

    def setParams(self, **kw):
        for k, v in kw.items():
            if not hasattr(self._p, k):
                raise AttributeError(k)
            setattr(self._p, k, v)
        self._push()

    def setRegularizationPose(self, T):
        a = _colmajor(T)
        self._check(lib().ndt_set_regularization_pose(self._h, _fp(a)))

    def unsetRegularizationPose(self):
        self._check(lib().ndt_clear_regularization_pose(self._h))

    # --- clouds ---
    @staticmethod
    def _xyz(a):
        return _host_cloud(a)[0]

    def debugSortPairs(self, keys, end_bit):
        """Test seam: the voxel build's stable radix sort on caller keys -> (sorted keys, permutation)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        ko, vo = np.empty_like(k), np.empty_like(k)
        self._check(lib().ndt_debug_sort_pairs(self._h, k.ctypes.data, len(k), int(end_bit), ko.ctypes.data,
                                               vo.ctypes.data))
        return ko, vo

    def setInputTarget(self, cloud):
        a = self._xyz(cloud)
        self._check(lib().ndt_set_target(self._h, a.ctypes.data, len(a), a.strides[0]))

    def setInputSource(self, cloud):
        a = self._xyz(cloud)
        self._check(lib().ndt_set_source(self._h, a.ctypes.data, len(a), a.strides[0]))

    def setInputTargetSoA(self, x, y, z):
        x, y, z = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, z))
        self._check(lib().ndt_set_target_soa(self._h, x.ctypes.data, y.ctypes.data, z.ctypes.data, len(x)))

    def setInputSourceSoA(self, x, y, z):
        x, y, z = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, z))
        self._check(lib().ndt_set_source_soa(self._h, x.ctypes.data, y.ctypes.data, z.ctypes.data, len(x)))

    def setInputTargetDevice(self, dx, dy, dz, n):
        """dx/dy/dz: integer device addresses of SoA float32 arrays already in HBM."""
        self._check(lib().ndt_set_target_device(self._h, dx, dy, dz, n))

    def setInputTargetDeviceDeferred(self, dx, dy, dz, n):
        """As setInputTargetDevice, but the voxel-grid build is only ENQUEUED (a steady-state build under the
        asynchronous hand-off): the arrays must stay valid and unchanged until the first call that needs the grid --
        align(), getGridInfo(), wait() ... -- has returned; a failed build is reported by that call."""
        self._check(lib().ndt_set_target_device_deferred(self._h, dx, dy, dz, n))

    def setInputSourceDevice(self, dx, dy, dz, n):
        self._check(lib().ndt_set_source_device(self._h, dx, dy, dz, n))

    def setInputSourceDeviceView(self, dx, dy, dz, n):
        """No copy: the device arrays must stay valid and unchanged until the source is replaced
        (pcl::Registration::setInputSource keeps the caller's shared_ptr the same way)."""
        self._check(lib().ndt_set_source_device_view(self._h, dx, dy, dz, n))

    def sourceChanged(self):
        """The arrays of a viewed source were rewritten in place: drop whatever the engine cached of them."""
        self._check(lib().ndt_source_changed(self._h))

    def setHandoffMode(self, mode):
        """HANDOFF_ASYNC (default): setInputTarget / setInputSource return once the host cloud has been consumed; the
        copies and the voxel-grid build finish behind, and a failing steady-state build is reported by the first call
        that needs the grid (or by wait()).  HANDOFF_SYNC: both block until the device has everything."""
        self._check(lib().ndt_set_handoff_mode(self._h, int(mode)))

    def getHandoffMode(self):
        return int(lib().ndt_get_handoff_mode(self._h))

    def wait(self):
        """Blocks until every hand-off in flight is complete; raises what a deferred build failed with."""
        self._check(lib().ndt_wait(self._h))

    def getHandoffTiming(self):
        t = HandoffTiming()
        self._check(lib().ndt_get_handoff_timing(self._h, C.byref(t)))
        lane = lambda l: {k: getattr(l, k) for k, _ in HandoffLaneTiming._fields_}  # noqa: E731
        return dict(target=lane(t.target), source=lane(t.source), ms_build_wait=t.ms_build_wait, mode=t.mode,
                    cpu_budget=t.cpu_budget, repack_workers=t.repack_workers)

    def setRecordFormat(self, fmt):
        """RECORDS_F64 (80-byte voxel records, default) or RECORDS_PACKED48 (f64 mean + f32 inverse covariance,
        three 16-byte loads per neighbour instead of five; ndt_hip.h)."""
        self._check(lib().ndt_set_record_format(self._h, int(fmt)))

    def getRecordFormat(self):
        return int(lib().ndt_get_record_format(self._h))

    # --- multi-grid target [RECALLED: tier4 MultiGridNormalDistributionsTransform] ---
    def addTarget(self, cloud, target_id):
        """Voxelises `cloud` on its own and keeps its leaves under `target_id`."""
        a, stride, _ = _host_cloud(cloud)
        self._check(lib().ndt_multigrid_add_target(self._h, int(target_id), a.ctypes.data, len(a), stride))

    def removeTarget(self, target_id):
        self._check(lib().ndt_multigrid_remove_target(self._h, int(target_id)))

    def targetCount(self):
        return int(lib().ndt_multigrid_count(self._h))

    def createVoxelKdtree(self):
        """The union of all stored grids becomes the target (radius search over every grid's leaves)."""
        self._check(lib().ndt_multigrid_create_kdtree(self._h))

    # --- device-resident keyframe archive (ref: run/pipeline.cpp:784, run/pipeline_ligo_tc.cpp:519-529) ---
    def putKeyframe(self, kf_id, cloud):
        a, stride, _ = _host_cloud(cloud)
        self._check(lib().ndt_keyframe_put(self._h, int(kf_id), a.ctypes.data, len(a), stride))

    # --- deskew: per-point times + a pose trajectory, the acquisition filter in the same pass ---
    @staticmethod
    def _filter_ref(filter):
        if filter is None:
            return None
        if not isinstance(filter, ScanFilter):
            raise TypeError("filter must be a ScanFilter")
        return C.byref(filter)

    @staticmethod
    def _scan(cloud, t, intensity_column):
        a, stride, off = _host_cloud(cloud, intensity_column)
        tt = np.ascontiguousarray(t, dtype=np.float32).ravel()
        if len(tt) != len(a):
            raise ValueError("t must hold one time per point")
        return a, tt, stride, off

    def deskew(self, cloud, t, knot_t, knot_poses, ref_pose=None, filter=None, intensity_column=None, with_index=False):
        """The scan (N x >= 3 float32, one time per point in the units of knot_t) expressed in ref_pose (None: the last
        knot) -- see trajectory_pose for the model.  filter None: N points out, a non-finite point as NaN; a ScanFilter:
        the kept points in input order.  Returns a cloud of the same layout (x, y, z and the intensity column written,
        other columns zero), with_index: (cloud, index [m] int32)."""
        a, tt, stride, off = self._scan(cloud, t, intensity_column)
        kt, poses, n, ref = _trajectory_args(knot_t, knot_poses, ref_pose)
        out = np.zeros_like(a)
        idx = np.zeros(len(a), np.int32) if with_index else None
        m = C.c_size_t(0)
        self._check(lib().ndt_deskew(self._h, a.ctypes.data, len(a), stride, off, tt.ctypes.data, _dp(kt), _dp(poses), n,
                                     None if ref is None else _dp(ref), self._filter_ref(filter), out.ctypes.data,
                                     None if idx is None else idx.ctypes.data, len(a), C.byref(m)))
        out = out[:m.value].copy()
        return (out, idx[:m.value].copy()) if with_index else out

    def deskewDevice(self, dx, dy, dz, d_t, n, knot_t, knot_poses, ox, oy, oz, cap, ref_pose=None, filter=None,
                     d_intensity=None, o_intensity=None, d_index=None):
        """deskew on device SoA arrays (integer device addresses as setInputTargetDevice takes them; the intensity and
        index arrays may be None); returns the number of points written.  Without a filter the outputs may be the inputs."""
        kt, poses, nk, ref = _trajectory_args(knot_t, knot_poses, ref_pose)
        m = C.c_size_t(0)
        rc = lib().ndt_deskew_device(self._h, dx, dy, dz, d_intensity, d_t, int(n), _dp(kt), _dp(poses), nk,
                                     None if ref is None else _dp(ref), self._filter_ref(filter), ox, oy, oz, o_intensity,
                                     d_index, int(cap), C.byref(m))
        self.last_deskew_count = int(m.value)
        self._check(rc)
        return int(m.value)

    def putKeyframeDeskewed(self, kf_id, cloud, t, knot_t, knot_poses, ref_pose=None, filter=None, intensity_column=None):
        """putKeyframe(kf_id, deskew(cloud, ...)) with one upload: the archived scan is expressed in ref_pose (None: the
        last knot), which is then the frame's pose.  Returns the number of points archived."""
        a, tt, stride, off = self._scan(cloud, t, intensity_column)
        kt, poses, n, ref = _trajectory_args(knot_t, knot_poses, ref_pose)
        m = C.c_size_t(0)
        self._check(lib().ndt_keyframe_put_deskewed(self._h, int(kf_id), a.ctypes.data, len(a), stride, off, tt.ctypes.data,
                                                    _dp(kt), _dp(poses), n, None if ref is None else _dp(ref),
                                                    self._filter_ref(filter), C.byref(m)))
        return int(m.value)

    # --- unprojection: a range image through the scan model's tables, gate + filter + deskew in the same pass ---
    def setScanModel(self, x1, y1, z1, x2, y2, z2):
        """The unprojection tables (scan_model_from_beams returns them): x1, y1, z1 [n_cols, n_rows], x2, y2, z2 [n_cols];
        copied to the device and kept until replaced or cleared."""
        d = [np.ascontiguousarray(a, dtype=np.float32) for a in (x1, y1, z1)]
        o = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in (x2, y2, z2)]
        if d[0].ndim != 2 or any(a.shape != d[0].shape for a in d) or any(len(a) != d[0].shape[0] for a in o):
            raise ValueError("x1, y1, z1 must be n_cols x n_rows and x2, y2, z2 n_cols long")
        self._check(lib().ndt_scan_model_set(self._h, d[0].shape[0], d[0].shape[1], _fp(d[0]), _fp(d[1]), _fp(d[2]), _fp(o[0]),
                                             _fp(o[1]), _fp(o[2])))

    def clearScanModel(self):
        self._check(lib().ndt_scan_model_clear(self._h))

    def scanModelInfo(self):
        """(n_cols, n_rows) of the scan model, (0, 0) when none is set"""
        c, r = C.c_int(0), C.c_int(0)
        self._check(lib().ndt_scan_model_get_info(self._h, C.byref(c), C.byref(r)))
        return c.value, r.value

    @staticmethod
    def _gate_ref(gate):
        if gate is None:
            return None
        if not isinstance(gate, RangeGate):
            raise TypeError("gate must be a RangeGate")
        return C.byref(gate)

    @staticmethod
    def _trajectory_or_none(knot_t, knot_poses, ref_pose):
        """the C-ABI's trajectory arguments; no knots at all = no motion"""
        if knot_t is None and knot_poses is None and ref_pose is None:
            return None, None, 0, None
        kt, poses, n, ref = _trajectory_args(knot_t, knot_poses, ref_pose)
        return _dp(kt), _dp(poses), n, None if ref is None else _dp(ref)

    def _range_image(self, range_mm, reflectivity, col_t):
        n_cols, n_rows = self.scanModelInfo()
        r = np.ascontiguousarray(range_mm, dtype=np.uint32).ravel()
        t = np.ascontiguousarray(col_t, dtype=np.float32).ravel()
        refl = None if reflectivity is None else np.ascontiguousarray(reflectivity, dtype=np.uint8).ravel()
        if n_cols and (len(r) != n_cols * n_rows or len(t) != n_cols or (refl is not None and len(refl) != len(r))):
            raise ValueError("the range image must hold n_cols x n_rows pixels and one time per column of the scan model")
        return r, refl, t, n_cols * n_rows

    def unproject(self, range_mm, reflectivity, col_t, knot_t=None, knot_poses=None, ref_pose=None, gate=None, filter=None,
                  with_t=False, with_index=False):
        """The range image (uint32 millimetres [n_cols, n_rows], uint8 reflectivity or None, one float32 time per column)
        as points through the scan model: filter None: the organised cloud, every pixel, an invalid one as NaN; a
        ScanFilter: the valid, kept points in pixel order.  With knots the points are deskewed as deskew() does it.
        Returns a cloud [m, 4] (x, y, z, intensity) -- [m, 3] without reflectivity --, then the times and the pixel
        indices if asked for."""
        r, refl, t, n = self._range_image(range_mm, reflectivity, col_t)
        kt, poses, nk, ref = self._trajectory_or_none(knot_t, knot_poses, ref_pose)
        cols = 3 if refl is None else 4
        out = np.zeros((n, cols), np.float32)
        tt = np.zeros(n, np.float32) if with_t else None
        idx = np.zeros(n, np.int32) if with_index else None
        m = C.c_size_t(0)
        self._check(lib().ndt_unproject(self._h, r.ctypes.data, None if refl is None else refl.ctypes.data, t.ctypes.data,
                                        self._gate_ref(gate), kt, poses, nk, ref, self._filter_ref(filter), out.ctypes.data,
                                        4 * cols, -1 if refl is None else 12, None if tt is None else tt.ctypes.data,
                                        None if idx is None else idx.ctypes.data, n, C.byref(m)))
        res = [out[:m.value].copy()]
        if with_t:
            res.append(tt[:m.value].copy())
        if with_index:
            res.append(idx[:m.value].copy())
        return res[0] if len(res) == 1 else tuple(res)

    def unprojectDevice(self, d_range_mm, d_reflectivity, d_col_t, ox, oy, oz, cap, knot_t=None, knot_poses=None, ref_pose=None,
                        gate=None, filter=None, o_intensity=None, o_t=None, d_index=None):
        """unproject on device arrays (integer device addresses; the reflectivity and the intensity, time and index outputs
        may be None); returns the number of points written."""
        kt, poses, nk, ref = self._trajectory_or_none(knot_t, knot_poses, ref_pose)
        m = C.c_size_t(0)
        rc = lib().ndt_unproject_device(self._h, d_range_mm, d_reflectivity, d_col_t, self._gate_ref(gate), kt, poses, nk, ref,
                                        self._filter_ref(filter), ox, oy, oz, o_intensity, o_t, d_index, int(cap), C.byref(m))
        self.last_unproject_count = int(m.value)
        self._check(rc)
        return int(m.value)

    def putKeyframeFromRanges(self, kf_id, range_mm, reflectivity, col_t, knot_t=None, knot_poses=None, ref_pose=None, gate=None,
                              filter=None):
        """putKeyframe(kf_id, unproject(...)) with one upload of the range image (filter None: the zeroed filter -- an
        archive holds no NaN points).  Returns the number of points archived."""
        r, refl, t, _ = self._range_image(range_mm, reflectivity, col_t)
        kt, poses, nk, ref = self._trajectory_or_none(knot_t, knot_poses, ref_pose)
        m = C.c_size_t(0)
        self._check(lib().ndt_keyframe_put_from_ranges(self._h, int(kf_id), r.ctypes.data, None if refl is None else refl.ctypes.data,
                                                       t.ctypes.data, self._gate_ref(gate), kt, poses, nk, ref,
                                                       self._filter_ref(filter), C.byref(m)))
        return int(m.value)

    # --- lidar packets: the UDP payloads of a frame decoded on the device, then the calls above on the decoded image ---
    def setPacketFormat(self, profile, columns_per_packet):
        """LIDAR_PROFILE_RNG19 or LIDAR_PROFILE_LEGACY and the columns a packet carries; needs the scan model (setScanModel
        and clearScanModel drop the format and the frame in progress)."""
        self._check(lib().ndt_packet_format_set(self._h, int(profile), int(columns_per_packet)))

    def packetFormat(self):
        """(profile, columns_per_packet, packet bytes); (-1, 0, 0) when none is set"""
        p, c = C.c_int(0), C.c_int(0)
        self._check(lib().ndt_packet_format_get(self._h, C.byref(p), C.byref(c)))
        return p.value, c.value, int(lib().ndt_packet_size(self._h))

    def beginPacketFrame(self):
        self._check(lib().ndt_packet_frame_begin(self._h))

    def pushPackets(self, packets):
        """Packets in arrival order (a uint8 array [k, bytes] or a sequence of bytes-like payloads); returns the number
        taken -- fewer than given when a packet of the next frame stopped the call (packetFrameInfo()
        ["next_frame_pending"]): finish the frame, beginPacketFrame(), push the rest."""
        a, sizes, stride = _packet_array(packets)
        taken = C.c_size_t(0)
        self._check(lib().ndt_packet_frame_push(self._h, a.ctypes.data, sizes.ctypes.data, len(a), stride, C.byref(taken)))
        return int(taken.value)

    def packetFrameInfo(self):
        info = PacketFrameInfo()
        self._check(lib().ndt_packet_frame_get_info(self._h, C.byref(info)))
        return info.as_dict()

    def decodePacketFrameDevice(self, d_range_mm, d_reflectivity, d_signal, d_nir, d_col_t):
        """The range image of the frame in progress into device arrays (integer device addresses; reflectivity, signal and
        nir may be None)."""
        self._check(lib().ndt_decode_packet_frame_device(self._h, d_range_mm, d_reflectivity, d_signal, d_nir, d_col_t))

    def unprojectPacketFrame(self, knot_t=None, knot_poses=None, ref_pose=None, gate=None, filter=None, with_t=False,
                             with_index=False, with_signal=False, with_nir=False):
        """unproject() of the frame in progress: a cloud [m, 4] (x, y, z, intensity), then the times, the pixel indices,
        the signal and the nir values (uint16) of its points if asked for."""
        n_cols, n_rows = self.scanModelInfo()
        n = n_cols * n_rows
        kt, poses, nk, ref = self._trajectory_or_none(knot_t, knot_poses, ref_pose)
        out = np.zeros((max(n, 1), 4), np.float32)
        tt = np.zeros(max(n, 1), np.float32) if with_t else None
        idx = np.zeros(max(n, 1), np.int32) if with_index else None
        sig = np.zeros(max(n, 1), np.uint16) if with_signal else None
        nir = np.zeros(max(n, 1), np.uint16) if with_nir else None
        m = C.c_size_t(0)
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        self._check(lib().ndt_unproject_packet_frame(self._h, self._gate_ref(gate), kt, poses, nk, ref, self._filter_ref(filter),
                                                     out.ctypes.data, 16, 12, ptr(tt), ptr(idx), ptr(sig), ptr(nir), n, C.byref(m)))
        res = [out[:m.value].copy()] + [a[:m.value].copy() for a in (tt, idx, sig, nir) if a is not None]
        return res[0] if len(res) == 1 else tuple(res)

    def unprojectPacketFrameDevice(self, ox, oy, oz, cap, knot_t=None, knot_poses=None, ref_pose=None, gate=None, filter=None,
                                   o_intensity=None, o_t=None, d_index=None, d_signal=None, d_nir=None):
        """unprojectDevice() of the frame in progress (integer device addresses); returns the number of points written."""
        kt, poses, nk, ref = self._trajectory_or_none(knot_t, knot_poses, ref_pose)
        m = C.c_size_t(0)
        rc = lib().ndt_unproject_packet_frame_device(self._h, self._gate_ref(gate), kt, poses, nk, ref, self._filter_ref(filter), ox, oy,
                                                     oz, o_intensity, o_t, d_index, d_signal, d_nir, int(cap), C.byref(m))
        self.last_unproject_count = int(m.value)
        self._check(rc)
        return int(m.value)

    def putKeyframeFromPackets(self, kf_id, knot_t=None, knot_poses=None, ref_pose=None, gate=None, filter=None, with_signal=False,
                               with_nir=False):
        """putKeyframeFromRanges() of the frame in progress; returns the number of points archived, then their signal and
        nir values if asked for."""
        n_cols, n_rows = self.scanModelInfo()
        kt, poses, nk, ref = self._trajectory_or_none(knot_t, knot_poses, ref_pose)
        sig = np.zeros(max(n_cols * n_rows, 1), np.uint16) if with_signal else None
        nir = np.zeros(max(n_cols * n_rows, 1), np.uint16) if with_nir else None
        m = C.c_size_t(0)
        self._check(lib().ndt_keyframe_put_from_packets(self._h, int(kf_id), self._gate_ref(gate), kt, poses, nk, ref,
                                                        self._filter_ref(filter), None if sig is None else sig.ctypes.data,
                                                        None if nir is None else nir.ctypes.data, C.byref(m)))
        res = [int(m.value)] + [a[:m.value].copy() for a in (sig, nir) if a is not None]
        return res[0] if len(res) == 1 else tuple(res)

    def setInputSourceFromKeyframe(self, kf_id):
        self._check(lib().ndt_set_source_from_keyframe(self._h, int(kf_id)))

    def eraseKeyframe(self, kf_id):
        self._check(lib().ndt_keyframe_erase(self._h, int(kf_id)))

    def keyframeCount(self):
        return int(lib().ndt_keyframe_count(self._h))

    def setInputTargetFromKeyframes(self, ids, poses):
        """target = sum of archived scans, each moved by its 4x4 double pose, built on the device."""
        ids_a = (C.c_int64 * len(ids))(*[int(i) for i in ids])
        p = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float64).T for T in poses])).ravel()
        self._check(lib().ndt_set_target_from_keyframes(self._h, ids_a, _dp(p), len(ids)))

    # --- pcl::VoxelGrid downsample (ref: run/pipeline_ins_map_distribution.cpp:324-340) ---
    def voxelDownsampleDevice(self, dx, dy, dz, n, leaf, ox, oy, oz, cap, d_intensity=None, o_intensity=None):
        """SoA device arrays in, centroids of the occupied voxels (ascending voxel index) out; returns their number.
        The output arrays can be handed to setInputTargetDevice as they are."""
        m = C.c_size_t(0)
        self._check(lib().ndt_voxel_downsample_device(self._h, dx, dy, dz, d_intensity, int(n), float(leaf), ox, oy, oz,
                                                      o_intensity, int(cap), C.byref(m)))
        return int(m.value)

    def voxelDownsample(self, cloud, leaf, intensity_column=None):
        """Host cloud (N x >= 3 float32; intensity_column: index of the intensity field, 4 for pcl::PointXYZI's
        8-float layout) -> the filtered cloud in the same layout (other columns zero)."""
        a, stride, off = _host_cloud(cloud, intensity_column)
        out = np.zeros_like(a)
        if len(a) == 0:
            return out
        m = C.c_size_t(0)
        self._check(lib().ndt_voxel_downsample(self._h, a.ctypes.data, len(a), stride, off, float(leaf),
                                               out.ctypes.data, len(out), C.byref(m)))
        return out[:m.value]

    # --- sparse voxel map accumulated scan by scan (ref: run/pipeline_ins_map_distribution.cpp:281-377) ---
    @staticmethod
    def _pose16_or_none(pose):
        if pose is None:
            return None
        p = np.asarray(pose, dtype=np.float64)
        if p.shape != (4, 4):
            raise ValueError("pose must be 4 x 4")
        return np.ascontiguousarray(p.T).ravel()

    def mapReset(self, leaf, with_intensity=False, initial_capacity=0):
        """A new, empty voxel map of this leaf size (an existing one is freed)."""
        self._check(lib().ndt_map_reset(self._h, float(leaf), int(bool(with_intensity)), int(initial_capacity)))

    def mapClear(self):
        self._check(lib().ndt_map_clear(self._h))

    def mapAdd(self, cloud, intensity_column=None, pose=None):
        """Host cloud (N x >= 3 float32; intensity_column as for voxelDownsample), moved by the 4x4 double `pose` if
        one is given, accumulated into the map."""
        a, stride, off = _host_cloud(cloud, intensity_column)
        p = self._pose16_or_none(pose)
        self._check(lib().ndt_map_add(self._h, a.ctypes.data, len(a), stride, off, None if p is None else _dp(p)))

    def mapAddDevice(self, dx, dy, dz, n, d_intensity=None, pose=None):
        """SoA float32 arrays in device memory (integer addresses), as mapAdd."""
        p = self._pose16_or_none(pose)
        self._check(lib().ndt_map_add_device(self._h, dx, dy, dz, d_intensity, int(n), None if p is None else _dp(p)))

    def mapAddKeyframe(self, kf_id, pose):
        """An archived keyframe (putKeyframe) moved by its 4x4 double pose."""
        p = self._pose16_or_none(pose)
        if p is None:
            raise ValueError("a keyframe is added under a pose")
        self._check(lib().ndt_map_add_keyframe(self._h, int(kf_id), _dp(p)))

    def mapInfo(self):
        mi = MapInfo()
        self._check(lib().ndt_map_get_info(self._h, C.byref(mi)))
        return dict(leaf=mi.leaf, with_intensity=bool(mi.with_intensity), n_voxels=mi.n_voxels, n_points=mi.n_points,
                    n_points_dropped=mi.n_points_dropped, capacity=mi.capacity, min_ijk=tuple(mi.min_ijk),
                    max_ijk=tuple(mi.max_ijk), n_adds=mi.n_adds, n_grows=mi.n_grows)

    def mapExport(self, min_points=1, columns=3, intensity_column=None, with_counts=False):
        """The map's centroids (ascending (k, j, i)) as an M x `columns` float32 cloud in the layout mapAdd takes (other
        columns zero); with_counts: (cloud, int32 counts)."""
        columns = int(columns)
        if columns < 3 or (intensity_column is not None and not 3 <= int(intensity_column) < columns):
            raise ValueError("columns >= 3 and 3 <= intensity_column < columns")
        off = -1 if intensity_column is None else 4 * int(intensity_column)
        cap = self.mapInfo()["n_voxels"]              # (no selection holds more)
        out = np.zeros((cap, columns), dtype=np.float32)
        cnt = np.zeros(cap, dtype=np.int32)
        m = C.c_size_t(0)
        self._check(lib().ndt_map_export(self._h, int(min_points), out.ctypes.data if cap else None, 4 * columns, off,
                                         cnt.ctypes.data if cap else None, cap, C.byref(m)))
        out, cnt = out[:m.value], cnt[:m.value]
        return (out, cnt) if with_counts else out

    def mapExportDevice(self, ox, oy, oz, cap, min_points=1, o_intensity=None, o_count=None):
        """Into SoA device arrays of `cap` elements (o_count: int32); returns the number of voxels.  The arrays can be
        handed to setInputTargetDevice as they are."""
        m = C.c_size_t(0)
        self._check(lib().ndt_map_export_device(self._h, int(min_points), ox, oy, oz, o_intensity, o_count, int(cap),
                                                C.byref(m)))
        return int(m.value)

    def setInputTargetFromMap(self, min_points=1):
        """The map's centroids (voxels with >= min_points points) become the target, without leaving the device."""
        self._check(lib().ndt_set_target_from_map(self._h, int(min_points)))

    def mapEnableMoments(self):
        """From now on the map also keeps, per voxel, the nine f64 moment sums the target build reduces to (allowed on
        a map that has accumulated no point yet)."""
        self._check(lib().ndt_map_enable_moments(self._h))

    def mapHasMoments(self):
        rc = lib().ndt_map_has_moments(self._h)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def mapExportMoments(self, min_points=1):
        """(ijk [m, 3] int32, count [m] int32, sums [m, 9] float64: sum x, y, z, then xx xy xz yy yz zz) of the voxels
        with >= min_points points, ascending (k, j, i): what a caller saves to disk."""
        cap = self.mapInfo()["n_voxels"]              # (no selection holds more)
        ijk = np.zeros((cap, 3), dtype=np.int32)
        cnt = np.zeros(cap, dtype=np.int32)
        sums = np.zeros((cap, 9), dtype=np.float64)
        m = C.c_size_t(0)
        self._check(lib().ndt_map_export_moments(self._h, int(min_points), ijk.ctypes.data if cap else None,
                                                 cnt.ctypes.data if cap else None, sums.ctypes.data if cap else None, cap,
                                                 C.byref(m)))
        return ijk[:m.value], cnt[:m.value], sums[:m.value]

    @staticmethod
    def _box_corner(v, name):
        a = np.ascontiguousarray(v, dtype=np.float32)
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError("%s must be three finite numbers" % name)
        return a

    def setInputTargetFromMapMoments(self, box_min=None, box_max=None):
        """The NDT target made directly from the map's per-voxel moments: what setInputTarget would build from every
        finite point ever added whose voxel lies inside the box (both corners None: the whole map)."""
        if (box_min is None) != (box_max is None):
            raise ValueError("box_min and box_max go together (both None: the whole map)")
        if box_min is None:
            self._check(lib().ndt_set_target_from_map_moments(self._h, None, None))
            return
        lo, hi = self._box_corner(box_min, "box_min"), self._box_corner(box_max, "box_max")
        self._check(lib().ndt_set_target_from_map_moments(self._h, _fp(lo), _fp(hi)))

    # --- the map bounded, kept and combined: crop to a box, the full per-voxel state out and back in ---
    def _box_or_none(self, box_min, box_max):
        """(lo, hi) float32 corners, or (None, None) for the whole map; ValueError on half a box or a non-finite one."""
        if (box_min is None) != (box_max is None):
            raise ValueError("box_min and box_max go together (both None: the whole map)")
        if box_min is None:
            return None, None
        return self._box_corner(box_min, "box_min"), self._box_corner(box_max, "box_max")

    def mapCrop(self, box_min, box_max, remove_inside=False):
        """Keep the voxels inside the box and drop the rest (remove_inside: the other way round); returns the number of
        voxels dropped.  box_min > box_max on an axis is an empty box."""
        if box_min is None or box_max is None:
            raise ValueError("a crop needs both corners of its box")
        lo, hi = self._box_or_none(box_min, box_max)
        removed = C.c_int64(0)
        self._check(lib().ndt_map_crop(self._h, _fp(lo), _fp(hi), int(bool(remove_inside)), C.byref(removed)))
        return int(removed.value)

    def mapExportState(self, box_min=None, box_max=None):
        """The complete state of the occupied voxels (of the box, if one is given) in ascending (k, j, i) order:
        dict(leaf, with_intensity, ijk [m, 3] int32, count [m] int32, sums [m, 4] float32 -- the sums as the map holds
        them, not divided -- and moments [m, 9] float64, None for a map without moments).  mapImportState takes it."""
        lo, hi = self._box_or_none(box_min, box_max)
        info = self.mapInfo()
        cap = info["n_voxels"]                        # (no selection holds more)
        with_mom = self.mapHasMoments()
        ijk = np.zeros((cap, 3), dtype=np.int32)
        cnt = np.zeros(cap, dtype=np.int32)
        sums = np.zeros((cap, 4), dtype=np.float32)
        mom = np.zeros((cap, 9), dtype=np.float64) if with_mom else None
        m = C.c_size_t(0)
        self._check(lib().ndt_map_export_state(self._h, None if lo is None else _fp(lo), None if hi is None else _fp(hi),
                                               ijk.ctypes.data if cap else None, cnt.ctypes.data if cap else None,
                                               sums.ctypes.data if cap else None,
                                               mom.ctypes.data if with_mom and cap else None, cap, C.byref(m)))
        k = m.value
        return dict(leaf=info["leaf"], with_intensity=info["with_intensity"], ijk=ijk[:k], count=cnt[:k], sums=sums[:k],
                    moments=None if mom is None else mom[:k])

    def mapExportStateDevice(self, d_ijk, d_count, d_sums, d_moments, cap, box_min=None, box_max=None):
        """Into device arrays of `cap` records (integer addresses, any may be None); returns the number of voxels."""
        lo, hi = self._box_or_none(box_min, box_max)
        m = C.c_size_t(0)
        self._check(lib().ndt_map_export_state_device(self._h, None if lo is None else _fp(lo), None if hi is None else _fp(hi),
                                                      d_ijk, d_count, d_sums, d_moments, int(cap), C.byref(m)))
        return int(m.value)

    @staticmethod
    def _state_arrays(state, leaf, ijk, count, sums, moments):
        """(leaf, ijk int32 [n, 3], count int32 [n], sums float32 [n, 4], moments float64 [n, 9] or None, n) of a state
        given as a dict or as its arrays; ValueError on a missing or ragged one"""
        if state is not None:
            leaf, ijk, count, sums, moments = state["leaf"], state["ijk"], state["count"], state["sums"], state.get("moments")
        if leaf is None or ijk is None or count is None or sums is None:
            raise ValueError("a state needs leaf, ijk, count and sums")
        ijk = np.ascontiguousarray(ijk, dtype=np.int32)
        count = np.ascontiguousarray(count, dtype=np.int32)
        sums = np.ascontiguousarray(sums, dtype=np.float32)
        n = len(count)
        if count.ndim != 1 or ijk.shape != (n, 3) or sums.shape != (n, 4):
            raise ValueError("ijk must be n x 3 and sums n x 4 for the n counts")
        if moments is not None:
            moments = np.ascontiguousarray(moments, dtype=np.float64)
            if moments.shape != (n, 9):
                raise ValueError("moments must be n x 9")
        return float(leaf), ijk, count, sums, moments, n

    def mapImportState(self, state=None, leaf=None, ijk=None, count=None, sums=None, moments=None):
        """Merge voxel records into the map: a dict as mapExportState returns it, or leaf and the arrays themselves
        (ijk [n, 3], count [n], sums [n, 4], moments [n, 9] or None)."""
        leaf, ijk, count, sums, moments, n = self._state_arrays(state, leaf, ijk, count, sums, moments)
        self._check(lib().ndt_map_import_state(self._h, leaf, ijk.ctypes.data if n else None, count.ctypes.data if n else None,
                                               sums.ctypes.data if n else None,
                                               moments.ctypes.data if moments is not None and n else None, n))

    def mapImportStateDevice(self, leaf, d_ijk, d_count, d_sums, d_moments, n):
        """As mapImportState, from device arrays (integer addresses; d_moments None for a map without moments)."""
        self._check(lib().ndt_map_import_state_device(self._h, float(leaf), d_ijk, d_count, d_sums, d_moments, int(n)))

    # --- free-space carving: the voxels that the rays of a scan pass through, and none ends in, leave the map ---
    @staticmethod
    def _carve_args(origin, min_misses, keep_last, max_steps, protect_min_count, dry_run):
        """(origin float32[3], MapCarveParams); ValueError on what the library would refuse"""
        o = np.ascontiguousarray(origin, dtype=np.float32)
        if o.shape != (3,) or not np.isfinite(o).all():
            raise ValueError("origin must be three finite numbers")
        prm = MapCarveParams()
        lib().ndt_map_carve_default_params(C.byref(prm))
        for name, v in (("min_misses", min_misses), ("keep_last", keep_last), ("max_steps", max_steps),
                        ("protect_min_count", protect_min_count)):
            if v is not None:
                setattr(prm, name, int(v))
        prm.dry_run = int(bool(dry_run))
        if prm.min_misses < 1 or prm.keep_last < 0 or not 1 <= prm.max_steps <= 65536 or prm.protect_min_count < 0:
            raise ValueError("min_misses >= 1, keep_last >= 0, 1 <= max_steps <= 65536, protect_min_count >= 0")
        return o, prm

    @staticmethod
    def _carve_result(r):
        return {name: int(getattr(r, name)) for name, _ in MapCarveResult._fields_}

    def mapCarve(self, cloud, origin, pose=None, min_misses=None, keep_last=None, max_steps=None, protect_min_count=None,
                 dry_run=False):
        """One scan as a host cloud (N x >= 3 float32) seen from `origin` (the sensor position in the cloud's own frame;
        `pose`, 4x4 double, moves both): every voxel at least min_misses rays pass through and none ends in is removed.
        keep_last voxels before a ray's end are never counted, a ray is followed for max_steps voxels, a voxel with
        protect_min_count points or more stays (0: off), dry_run only counts.  None: the library's default.  Returns
        dict(n_rays, n_rays_skipped, n_steps, n_voxels_crossed, n_voxels_hit, n_removed, n_points_removed)."""
        o, prm = self._carve_args(origin, min_misses, keep_last, max_steps, protect_min_count, dry_run)
        a, stride, _ = _host_cloud(cloud)
        p = self._pose16_or_none(pose)
        r = MapCarveResult()
        self._check(lib().ndt_map_carve(self._h, a.ctypes.data if len(a) else None, len(a), stride, _fp(o),
                                        None if p is None else _dp(p), C.byref(prm), C.byref(r)))
        return self._carve_result(r)

    def mapCarveDevice(self, dx, dy, dz, n, origin, pose=None, min_misses=None, keep_last=None, max_steps=None,
                       protect_min_count=None, dry_run=False):
        """SoA float32 arrays in device memory (integer addresses), as mapCarve."""
        o, prm = self._carve_args(origin, min_misses, keep_last, max_steps, protect_min_count, dry_run)
        p = self._pose16_or_none(pose)
        r = MapCarveResult()
        self._check(lib().ndt_map_carve_device(self._h, dx, dy, dz, int(n), _fp(o), None if p is None else _dp(p),
                                               C.byref(prm), C.byref(r)))
        return self._carve_result(r)

    def mapCarveKeyframe(self, kf_id, origin, pose, min_misses=None, keep_last=None, max_steps=None, protect_min_count=None,
                         dry_run=False):
        """An archived keyframe (putKeyframe) under its 4x4 double pose, as mapCarve."""
        o, prm = self._carve_args(origin, min_misses, keep_last, max_steps, protect_min_count, dry_run)
        p = self._pose16_or_none(pose)
        if p is None:
            raise ValueError("a keyframe is carved under a pose")
        r = MapCarveResult()
        self._check(lib().ndt_map_carve_keyframe(self._h, int(kf_id), _fp(o), _dp(p), C.byref(prm), C.byref(r)))
        return self._carve_result(r)

    def setGlobalSourceSize(self, n):
        self._check(lib().ndt_set_global_source_size(self._h, int(n)))

    # --- registration ---
    def align(self, guess=None, return_transform=True):
        """align(guess) -> final 4x4.  return_transform=False skips building the NumPy result
        (a tight loop reads the few scalars it needs through the getters below)."""
        if guess is None:
            g = _colmajor(np.eye(4))
        elif isinstance(guess, ColMajor4f):
            g = guess.a
        else:
            g = _colmajor(guess)
        r = Result()
        self._check(lib().ndt_align(self._h, _fp(g), C.byref(r)))
        self._raw, self._cooked = r, None
        return self._result["T"] if return_transform else None

    computeTransformation = align

    def alignMany(self, guesses):
        """align() from each of K guesses (1 <= K <= 256) in shared launches (ndt_align_batch): a list of
        (final 4x4, result dict as getResult() gives it).  getResult() / getFinalTransformation() keep reporting the
        last align()."""
        g = np.ascontiguousarray(np.stack([x.a if isinstance(x, ColMajor4f) else _colmajor(x) for x in guesses]),
                                 dtype=np.float32) if len(guesses) else np.zeros((0, 16), np.float32)
        K = len(g)
        out = (Result * max(K, 1))()
        self._check(lib().ndt_align_batch(self._h, _fp(g), K, out))
        res = []
        for k in range(K):
            d = result_to_dict(out[k])
            d["iteration_num"] = d["iterations"]
            res.append((d["T"], d))
        return res

    @property
    def _result(self):
        if self._cooked is None and self._raw is not None:
            self._cooked = result_to_dict(self._raw)
        return self._cooked

    def getFinalTransformation(self): return self._result["T"]
    def hasConverged(self): return bool(self._raw.converged)
    def getFinalNumIteration(self): return self._raw.iterations
    def getNumEvaluations(self): return self._raw.n_evaluations
    def getTransformationProbability(self): return self._raw.transform_probability
    def getNearestVoxelTransformationLikelihood(self): return self._raw.nearest_voxel_transformation_likelihood

    def scoreTransform(self, T=None):
        """Scoring-only evaluation of the current source under T (default identity): dict(score,
        transform_probability, nvtl, n_pairs, n_points_with_neighbors)."""
        g = _colmajor(np.eye(4) if T is None else T)
        sc = Score()
        self._check(lib().ndt_score_transform(self._h, _fp(g), C.byref(sc)))
        return dict(score=sc.score, transform_probability=sc.transform_probability,
                    nvtl=sc.nearest_voxel_transformation_likelihood, n_pairs=sc.n_pairs,
                    n_points_with_neighbors=sc.n_points_with_neighbors)

    def scoreTransforms(self, transforms):
        """K transforms scored in one launch: list of dicts like scoreTransform()."""
        t = np.ascontiguousarray(np.stack([_colmajor(T) for T in transforms]), dtype=np.float32)
        K = len(t)
        out = (Score * K)()
        self._check(lib().ndt_score_transforms(self._h, _fp(t), K, out))
        return [dict(score=o.score, transform_probability=o.transform_probability,
                     nvtl=o.nearest_voxel_transformation_likelihood, n_pairs=o.n_pairs,
                     n_points_with_neighbors=o.n_points_with_neighbors) for o in out]

    # --- getFitnessScore [RECALLED: PCL Registration::getFitnessScore] ---
    def fitness(self, T, max_range=DBL_MAX, per_point=False):
        """Nearest-point fitness of the current source under T against the raw target points: dict(fitness_score,
        sum_sq_dist, n_inliers, n_points); with per_point=True also `sq_dists` (d^2 per source point, NaN for a
        non-finite point, +inf where d^2 > max_range).  max_range is a SQUARED distance, as in PCL."""
        a = _colmajor(T)
        out = Fitness()
        sq = None
        if per_point:
            sq = np.zeros(self.sourceSize(), np.float32)
        self._check(lib().ndt_fitness_score(self._h, _fp(a), float(max_range), C.byref(out),
                                            _fp(sq) if sq is not None else None, 0 if sq is None else len(sq)))
        d = dict(fitness_score=out.fitness_score, sum_sq_dist=out.sum_sq_dist, n_inliers=out.n_inliers,
                 n_points=out.n_points)
        if sq is not None:
            d["sq_dists"] = sq
        return d

    def fitnessMany(self, transforms, max_range=DBL_MAX):
        """K transforms in one query launch: list of dicts like fitness()."""
        t = np.ascontiguousarray(np.stack([_colmajor(T) for T in transforms]), dtype=np.float32)
        K = len(t)
        out = (Fitness * K)()
        self._check(lib().ndt_fitness_scores(self._h, _fp(t), K, float(max_range), out))
        return [dict(fitness_score=o.fitness_score, sum_sq_dist=o.sum_sq_dist, n_inliers=o.n_inliers,
                     n_points=o.n_points) for o in out]

    def getFitnessScore(self, max_range=DBL_MAX):
        """PCL's getFitnessScore(max_range): the fitness at the last align's final transformation (identity before
        any align)."""
        T = self._result["T"] if self._raw is not None else np.eye(4)
        return self.fitness(T, max_range)["fitness_score"]

    # --- per-point scores [RECALLED: tier4 ndt_omp calculateNearestVoxelScoreEachPoint] and the score-based filter ---
    POINT_SCORE_FIELDS = (("score", np.float64), ("nearest_voxel_score", np.float64), ("n_neighbors", np.int32),
                          ("best_voxel", np.int64))

    def sourceSize(self):
        """Points of the current (local) source, whichever call set it."""
        n = int(lib().ndt_source_size(self._h))
        if n < 0:
            raise NdtError(n, "ndt_source_size")
        return n

    @staticmethod
    def _T16(T):
        a = _colmajor(T)
        if a.shape != (16,) or not np.all(np.isfinite(a)):
            raise ValueError("T must be a finite 4 x 4 transform")
        return a

    def scorePoints(self, T, fields=None):
        """What scoreTransform(T) adds up, per source point in hand-over order: dict(score, nearest_voxel_score,
        n_neighbors, best_voxel) of NumPy arrays (`fields`: a subset of those names -- the others are not computed back)."""
        names = [f for f, _ in self.POINT_SCORE_FIELDS]
        want = names if fields is None else list(fields)
        for f in want:
            if f not in names:
                raise ValueError("unknown per-point field %r (one of %s)" % (f, ", ".join(names)))
        a = self._T16(T)
        n = self.sourceSize()
        out = {f: np.zeros(n, dt) for f, dt in self.POINT_SCORE_FIELDS if f in want}
        ptr = [out[f].ctypes.data if f in out else None for f in names]
        self._check(lib().ndt_score_points(self._h, _fp(a), ptr[0], ptr[1], ptr[2], ptr[3], n))
        return out

    def scorePointsDevice(self, T, d_score, d_nearest_voxel_score, d_n_neighbors, d_best_voxel, cap):
        """scorePoints into caller-owned device arrays (integer device addresses, None to skip one)."""
        a = self._T16(T)
        self._check(lib().ndt_score_points_device(self._h, _fp(a), d_score, d_nearest_voxel_score, d_n_neighbors,
                                                  d_best_voxel, int(cap)))

    def filterSource(self, T, min_score, keep_below=False):
        """The source points (as handed over, not transformed) whose nearest_voxel_score under T is >= min_score
        (keep_below: those below it), in input order: (xyz [m, 3] float32, index [m] int32)."""
        a = self._T16(T)
        if np.isnan(min_score):
            raise ValueError("min_score must not be NaN")
        n = self.sourceSize()
        xyz, idx = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        m = C.c_size_t(0)
        self._check(lib().ndt_filter_source(self._h, _fp(a), float(min_score), int(bool(keep_below)), xyz.ctypes.data,
                                            idx.ctypes.data, n, C.byref(m)))
        return xyz[:m.value].copy(), idx[:m.value].copy()

    def filterSourceDevice(self, T, min_score, keep_below, ox, oy, oz, d_index, cap):
        """filterSource into device SoA arrays (integer device addresses as setInputTargetDevice takes them; d_index may
        be None); returns the number selected.  The arrays can go into setInputTargetDevice / setInputSourceDevice."""
        a = self._T16(T)
        m = C.c_size_t(0)
        rc = lib().ndt_filter_source_device(self._h, _fp(a), float(min_score), int(bool(keep_below)), ox, oy, oz, d_index,
                                            int(cap), C.byref(m))
        self.last_filter_count = int(m.value)
        self._check(rc)
        return int(m.value)

    # --- 2-D covariance estimators of tier4 ndt_omp [RECALLED] ---
    def proposePosesToSearch(self, offsets_x, offsets_y):
        """Offsets rotated onto the principal axes of the Laplace covariance of the LAST result."""
        ox = np.ascontiguousarray(offsets_x, dtype=np.float64)
        oy = np.ascontiguousarray(offsets_y, dtype=np.float64)
        out = np.zeros((len(ox), 16), np.float32)
        self._check(lib().ndt_propose_poses_to_search(C.byref(self._raw), _dp(ox), _dp(oy), len(ox), _fp(out)))
        return [out[i].reshape(4, 4).T.astype(np.float64) for i in range(len(ox))]

    def estimateXYCovarianceMultiNdt(self, poses):
        main = Result.from_buffer_copy(self._raw)
        t = np.ascontiguousarray(np.stack([_colmajor(T) for T in poses]), dtype=np.float32)
        mean, cov = np.zeros(2), np.zeros(4)
        self._check(lib().ndt_xy_covariance_multi_ndt(self._h, C.byref(main), _fp(t), len(t), _dp(mean), _dp(cov)))
        return mean, cov.reshape(2, 2)

    def estimateXYCovarianceMultiNdtScore(self, poses, temperature):
        main = Result.from_buffer_copy(self._raw)
        t = np.ascontiguousarray(np.stack([_colmajor(T) for T in poses]), dtype=np.float32)
        mean, cov = np.zeros(2), np.zeros(4)
        self._check(lib().ndt_xy_covariance_multi_ndt_score(self._h, C.byref(main), _fp(t), len(t), float(temperature),
                                                            _dp(mean), _dp(cov)))
        return mean, cov.reshape(2, 2)

    def calculateTransformationProbability(self, cloud, T=None):
        """pclomp's scoring-only call [RECALLED]: score / #points of `cloud` (already transformed,
        or moved by T) against the current target."""
        self.setInputSource(cloud)
        return self.scoreTransform(T)["transform_probability"]

    def calculateNearestVoxelTransformationLikelihood(self, cloud, T=None):
        self.setInputSource(cloud)
        return self.scoreTransform(T)["nvtl"]

    def getResult(self):
        """pclomp::NdtResult: iteration_num, hessian, pose, transform_probability, nvtl."""
        r = dict(self._result)
        r["iteration_num"] = r["iterations"]
        return r

    def getIterationHistory(self):
        """pclomp::NdtResult's per-iteration arrays [RECALLED] of the last align: (transformation_array [n,4,4],
        transform_probability_array [n], nearest_voxel_transformation_likelihood_array [n]); entry 0 = the guess."""
        n = lib().ndt_get_iteration_history(self._h, None, None, None, 0)
        if n < 0:
            raise NdtError(n, "ndt_get_iteration_history")
        T = np.zeros((n, 16), np.float32)
        tp, nv = np.zeros(n), np.zeros(n)
        if n:
            lib().ndt_get_iteration_history(self._h, _fp(T), _dp(tp), _dp(nv), n)
        return T.reshape(n, 4, 4).transpose(0, 2, 1).astype(np.float64), tp, nv

    def evalDerivatives(self, poses6, transforms=None, compute_hessian=True):
        """computeDerivatives at K poses (K x 6); returns a list of dicts."""
        p = np.ascontiguousarray(np.atleast_2d(poses6), dtype=np.float64)
        K = p.shape[0]
        t = None
        if transforms is not None:
            t = np.ascontiguousarray(np.stack([_colmajor(T) for T in transforms]), dtype=np.float32)
        out = np.zeros((K, EVAL_WORDS))
        self._check(lib().ndt_eval_derivatives(self._h, _dp(p), _fp(t) if t is not None else None, K,
                                               int(compute_hessian), _dp(out)))
        return [unpack_eval(out[k]) for k in range(K)]

    def transformSource(self, T):
        """The `output` cloud of align(): the source transformed by T on the device."""
        n = self.sourceSize()
        out = np.zeros((n, 3), np.float32)
        a = _colmajor(T)
        self._check(lib().ndt_transform_source(self._h, _fp(a), _fp(out), n))
        return out

    # --- voxel grid accessors (ref: include/pipeline.hpp:175-206) ---
    def getGridInfo(self):
        gi = GridInfo()
        self._check(lib().ndt_get_grid_info(self._h, C.byref(gi)))
        return dict(min_b=np.array(gi.min_b[:]), max_b=np.array(gi.max_b[:]), div_b=np.array(gi.div_b[:]),
                    leaf_size=gi.leaf_size, n_leaves=gi.n_leaves, n_cells=gi.n_cells,
                    n_target_points=gi.n_target_points, ms_build=gi.ms_build)

    def getLeaves(self):
        """getTargetCells().getLeaves(): dict of arrays, valid leaves, ascending voxel index."""
        n = int(self.getGridInfo()["n_leaves"])
        buf = (Leaf * max(n, 1))()
        got = lib().ndt_export_leaves(self._h, buf, n)
        if got < 0:
            raise NdtError(int(got), lib().ndt_last_error(self._h).decode())
        a = np.frombuffer(buf, dtype=np.dtype(Leaf), count=got) if got else None
        if a is None:
            return dict(cell=np.zeros(0, np.int64), count=np.zeros(0, np.int32), center=np.zeros((0, 3), np.float32),
                        mean=np.zeros((0, 3)), cov=np.zeros((0, 3, 3)), icov=np.zeros((0, 3, 3)),
                        evecs=np.zeros((0, 3, 3)), evals=np.zeros((0, 3)))
        return dict(cell=a["index"].copy(), count=a["point_count"].copy(), center=a["center"].copy(),
                    mean=a["mean"].copy(), cov=a["cov"].reshape(-1, 3, 3).copy(),
                    icov=a["icov"].reshape(-1, 3, 3).copy(), evecs=a["evecs"].reshape(-1, 3, 3).copy(),
                    evals=a["evals"].copy())

    def getMinPointPerVoxel(self): return max(3, self._p.min_points_per_voxel)

    # --- multi-GPU ---
    def commInitRccl(self, id128, rank, nranks):
        buf = C.create_string_buffer(bytes(id128), 128)
        self._check(lib().ndt_comm_init_rccl(self._h, buf, rank, nranks))

    def commInitShm(self, name, rank, nranks):
        self._check(lib().ndt_comm_init_shm(self._h, name.encode(), rank, nranks))

    def commP2pHandle(self):
        """This rank's exchange area of the peer-write reducer as a 64-byte IPC handle (all-gather them)."""
        buf = C.create_string_buffer(64)
        self._check(lib().ndt_comm_p2p_handle(self._h, buf))
        return buf.raw

    def commInitP2p(self, handles, rank, nranks):
        """handles: the nranks x 64 bytes of every rank's commP2pHandle(), in rank order."""
        b = bytes(handles)
        if len(b) != 64 * nranks:
            raise ValueError("need %d handle bytes" % (64 * nranks))
        buf = C.create_string_buffer(b, len(b))
        self._check(lib().ndt_comm_init_p2p(self._h, buf, rank, nranks))

    def commInitHook(self, fn, rank, nranks):
        cb = ALLREDUCE_FN(fn)
        self._keep.append(cb)
        self._check(lib().ndt_comm_init_hook(self._h, cb, None, rank, nranks))

    def commRankCount(self):
        """Ranks of the live reducer as the transport reports them (RCCL: ncclCommCount)."""
        n = lib().ndt_comm_rank_count(self._h)
        if n < 0:
            raise NdtError(n, "ndt_comm_rank_count")
        return n

    def commP2pSelftest(self, rounds=10000):
        """COLLECTIVE slot-integrity pass of the peer-write reducer: dict(rounds, torn, missed, longest_us)."""
        out = (C.c_int64 * 4)()
        self._check(lib().ndt_comm_p2p_selftest(self._h, int(rounds), out))
        return dict(rounds=int(out[0]), torn=int(out[1]), missed=int(out[2]), longest_us=out[3] * 0.01)

    def commP2pStats(self, reset=False):
        """In-kernel exchanges since init / the last reset: dict(exchanges, mean_us, max_us, late)."""
        out = (C.c_int64 * 4)()
        self._check(lib().ndt_comm_p2p_stats(self._h, out, int(reset)))
        n = int(out[0])
        return dict(exchanges=n, mean_us=(out[1] * 0.01 / n) if n else 0.0, max_us=out[2] * 0.01, late=int(out[3]))

    def commDestroy(self):
        self._check(lib().ndt_comm_destroy(self._h))

    # --- instrumentation ---
    def setKeepWarm(self, period_us):
        """ndt_set_keepwarm: an idle-time heartbeat every period_us (0: off, the default)."""
        self._check(lib().ndt_set_keepwarm(self._h, int(period_us)))

    def keepWarm(self):
        """(period_us, beats launched so far)."""
        b = C.c_longlong(0)
        return lib().ndt_get_keepwarm(self._h, C.byref(b)), b.value

    def enableKernelTiming(self, on=True):
        self._check(lib().ndt_enable_kernel_timing(self._h, int(on)))

    def debugEvalLog(self, cap):
        """Test seam: clear the evaluation log and keep the next `cap` evaluations (0: off)."""
        rc = lib().ndt_debug_eval_log(self._h, int(cap))
        if rc < 0:
            raise NdtError(rc, "ndt_debug_eval_log")
        assert rc == EVAL_LOG_DTYPE.itemsize, "EvalLogEntry layout differs from EVAL_LOG_DTYPE"

    def debugEvalLogRead(self):
        """Test seam: the logged evaluations as a list of dicts (pose6, T as a 4x4, words, need_h, score_only, prelaunched,
        launch, k, K, desc: the launch's plan over EVAL_DESC_FIELDS).  Raises if the log overflowed."""
        n = lib().ndt_debug_eval_log_read(self._h, None, 0)
        if n < 0:
            raise NdtError(int(n), "ndt_debug_eval_log_read")
        a = np.zeros(n, EVAL_LOG_DTYPE)
        kept = lib().ndt_debug_eval_log_read(self._h, a.ctypes.data if n else None, int(n))
        assert kept == n
        return [dict(pose6=e["pose6"].copy(), T=e["T"].reshape(4, 4).T.astype(np.float64), T32=e["T"].copy(),
                     words=e["words"].copy(), need_h=bool(e["need_h"]), score_only=bool(e["score_only"]),
                     prelaunched=bool(e["prelaunched"]), launch=int(e["launch"]), k=int(e["k"]), K=int(e["K"]),
                     desc=dict(zip(EVAL_DESC_FIELDS, (int(v) for v in e["plan"])))) for e in a]

    def prelaunchCounters(self):
        """(evaluations served by a pre-launched kernel, pre-launched kernels told to leave, time-outs)."""
        out = (C.c_int64 * 8)()
        self._check(lib().ndt_debug_prelaunch_counters(self._h, out))
        return tuple(out)[:3]

    def autoStreamPlacement(self):
        """(1 if NDT_PRELAUNCH_AUTO has settled on the one-stream placement of waiting kernels, switches so far)."""
        out = (C.c_int64 * 8)()
        self._check(lib().ndt_debug_prelaunch_counters(self._h, out))
        return int(out[6]), int(out[7])

    def speculationCounters(self):
        """First evaluations of an align enqueued behind a build still in flight: (kept, discarded)."""
        out = (C.c_int64 * 2)()
        self._check(lib().ndt_debug_speculation_counters(self._h, out))
        return int(out[0]), int(out[1])

    def setSpeculation(self, on):
        """Tuning aid: the first-evaluation-behind-the-build short cut on / off for this handle."""
        self._check(lib().ndt_debug_set_speculation(self._h, 1 if on else 0))

    def lostRowRetries(self):
        """Evaluations repeated through the ticketed final sum after the summing block had given up waiting for a row."""
        out = (C.c_int64 * 8)()
        self._check(lib().ndt_debug_prelaunch_counters(self._h, out))
        return int(out[5])

    def prelaunchOverlapped(self):
        """Pre-launched kernels that were enqueued on the other stream (resident before their predecessor ended)."""
        out = (C.c_int64 * 8)()
        self._check(lib().ndt_debug_prelaunch_counters(self._h, out))
        return int(out[3])

    def p2pHostFinishes(self):
        """Peer-write evaluations whose cross-rank exchange the host had to finish (a peer's row was > 20 ms late)."""
        out = (C.c_int64 * 8)()
        self._check(lib().ndt_debug_prelaunch_counters(self._h, out))
        return int(out[4])

    def handoffCounters(self):
        """(host hand-offs of a target whose partition launch ran under the transfer, launches of tile ranges they made)."""
        out = (C.c_int64 * 2)()
        self._check(lib().ndt_debug_handoff_counters(self._h, out))
        return int(out[0]), int(out[1])

    def buildCounters(self):
        """(builds that fell back from the fused sort passes to the classic ones, two-launch bucketed builds
        that were declined and repeated sort-based, builds that went through in two launches)."""
        out = (C.c_int64 * 3)()
        self._check(lib().ndt_debug_build_counters(self._h, out))
        return tuple(out)

    def getTiming(self):
        t = Timing()
        self._check(lib().ndt_get_timing(self._h, C.byref(t)))
        return dict(ms_last_eval_kernel=t.ms_last_eval_kernel, ms_last_reduce_kernel=t.ms_last_reduce_kernel,
                    ms_last_build=t.ms_last_build, n_eval_launches=t.n_eval_launches,
                    ms_eval_kernel_total=t.ms_eval_kernel_total,
                    ms_reduce_kernel_total=t.ms_reduce_kernel_total, n_timed_evals=t.n_timed_evals)


# --- the map under a changed pose: every voxel's sums moved as the sums of its points would be (ndt_map_transform,
# ndt_map_import_state_posed).  Functions on an engine, not methods of it: `ndt` is a
# NormalDistributionsTransform that holds a map. ---
def _finite_pose16(pose):
    """a 4x4 double pose as 16 column-major doubles; ValueError on another shape or a non-finite value"""
    if pose is None:
        raise ValueError("a pose is needed")
    p = np.asarray(pose, dtype=np.float64)
    if p.shape != (4, 4) or not np.isfinite(p).all():
        raise ValueError("pose must be 4 x 4 and finite")
    return np.ascontiguousarray(p.T).ravel()


def mapTransform(ndt, pose):
    """Move the whole map of `ndt` by the 4x4 double `pose` (its upper 3 x 4 as given): every voxel's sums are moved
    exactly and re-binned by the moved float centroid, voxels that meet are merged in ascending (k, j, i) order.
    Returns the number of voxels afterwards."""
    p = _finite_pose16(pose)
    after = C.c_int64(0)
    ndt._check(lib().ndt_map_transform(ndt._h, _dp(p), C.byref(after)))
    return int(after.value)


def mapImportStatePosed(ndt, state=None, pose=None, leaf=None, ijk=None, count=None, sums=None, moments=None):
    """ndt.mapImportState of records accumulated in another frame: `pose` (4x4 double) takes that frame to the map's."""
    leaf, ijk, count, sums, moments, n = ndt._state_arrays(state, leaf, ijk, count, sums, moments)
    p = _finite_pose16(pose)
    ndt._check(lib().ndt_map_import_state_posed(ndt._h, leaf, ijk.ctypes.data if n else None,
                                                count.ctypes.data if n else None, sums.ctypes.data if n else None,
                                                moments.ctypes.data if moments is not None and n else None, n, _dp(p)))


def mapImportStatePosedDevice(ndt, leaf, d_ijk, d_count, d_sums, d_moments, n, pose):
    """As mapImportStatePosed, from device arrays (integer addresses; d_moments None for a map without moments)."""
    p = _finite_pose16(pose)
    ndt._check(lib().ndt_map_import_state_posed_device(ndt._h, float(leaf), d_ijk, d_count, d_sums, d_moments, int(n), _dp(p)))


# --- connected components of the map: which voxels belong together (ndt_map_components*, ndt_map_export_labels*,
# ndt_map_label_points*, ndt_map_remove_components).  Functions on an engine, as above; `engine` is a
# NormalDistributionsTransform that holds a map. ---
def _components_params(connectivity, min_count):
    """MapComponentsParams; ValueError on what the library would refuse.  None: the library's default (26, 1)."""
    prm = MapComponentsParams()
    lib().ndt_map_components_default_params(C.byref(prm))
    if connectivity is not None:
        prm.connectivity = int(connectivity)
    if min_count is not None:
        prm.min_count = int(min_count)
    if prm.connectivity not in (6, 18, 26) or prm.min_count < 1:
        raise ValueError("connectivity is 6, 18 or 26 and min_count >= 1")
    return prm


def _finite_pose16_or_none(pose):
    return None if pose is None else _finite_pose16(pose)


def mapComponents(engine, connectivity=None, min_count=None):
    """Label the map of `engine`: dict(n_components, n_voxels_labelled, n_voxels_unlabelled, largest, largest_n_voxels,
    largest_n_points).  Voxels with fewer than min_count points take no part; connectivity is 6, 18 or 26."""
    prm = _components_params(connectivity, min_count)
    info = MapComponentsInfo()
    engine._check(lib().ndt_map_components(engine._h, C.byref(prm), C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in MapComponentsInfo._fields_}


def mapExportComponents(engine, connectivity=None, min_count=None):
    """The component table in index order: dict(root_ijk [C, 3], n_voxels [C], n_points [C] int64, min_ijk [C, 3],
    max_ijk [C, 3]), int32 unless said otherwise."""
    prm = _components_params(connectivity, min_count)
    cap = mapComponents(engine, prm.connectivity, prm.min_count)["n_components"]
    rec = (MapComponent * max(cap, 1))()
    m = C.c_size_t(0)
    engine._check(lib().ndt_map_export_components(engine._h, C.byref(prm), rec if cap else None, cap, C.byref(m)))
    dt = np.dtype([("root_ijk", np.int32, 3), ("n_voxels", np.int32), ("n_points", np.int64), ("min_ijk", np.int32, 3),
                   ("max_ijk", np.int32, 3)])
    a = np.frombuffer(rec, dtype=dt, count=max(cap, 1))[:m.value].copy()
    return {k: a[k] for k in dt.names}


def mapExportLabels(engine, connectivity=None, min_count=None):
    """Every occupied voxel of the map in mapExportState()'s order: dict(ijk [m, 3] int32, label [m] int32; -1 for a
    voxel with fewer than min_count points)."""
    prm = _components_params(connectivity, min_count)
    cap = engine.mapInfo()["n_voxels"]
    ijk = np.zeros((cap, 3), dtype=np.int32)
    label = np.zeros(cap, dtype=np.int32)
    m = C.c_size_t(0)
    engine._check(lib().ndt_map_export_labels(engine._h, C.byref(prm), ijk.ctypes.data if cap else None,
                                           label.ctypes.data if cap else None, cap, C.byref(m)))
    return dict(ijk=ijk[:m.value], label=label[:m.value])


def mapExportLabelsDevice(engine, d_ijk, d_label, cap, connectivity=None, min_count=None):
    """Into device arrays of `cap` rows (integer addresses, either may be None); returns the number of voxels."""
    prm = _components_params(connectivity, min_count)
    m = C.c_size_t(0)
    engine._check(lib().ndt_map_export_labels_device(engine._h, C.byref(prm), d_ijk, d_label, int(cap), C.byref(m)))
    return int(m.value)


def mapLabelPoints(engine, cloud, pose=None, connectivity=None, min_count=None):
    """The label of the map voxel each point of a host cloud (N x >= 3 float32) falls in once moved by `pose` (4x4 double,
    as mapAdd moves it): int32 [N], -1 where there is none.  Returns (labels, n_labelled)."""
    prm = _components_params(connectivity, min_count)
    a, stride, _ = _host_cloud(cloud)
    p = _finite_pose16_or_none(pose)
    out = np.full(len(a), -1, dtype=np.int32)
    k = C.c_int64(0)
    engine._check(lib().ndt_map_label_points(engine._h, C.byref(prm), a.ctypes.data if len(a) else None, len(a), stride,
                                          None if p is None else _dp(p), out.ctypes.data if len(a) else None, C.byref(k)))
    return out, int(k.value)


def mapLabelPointsDevice(engine, dx, dy, dz, n, d_label, pose=None, connectivity=None, min_count=None):
    """SoA float32 arrays and an int32 output in device memory (integer addresses), as mapLabelPoints; returns n_labelled."""
    prm = _components_params(connectivity, min_count)
    p = _finite_pose16_or_none(pose)
    if int(n) > 0 and not (dx and dy and dz and d_label):
        raise ValueError("the cloud and the label output are needed")
    k = C.c_int64(0)
    engine._check(lib().ndt_map_label_points_device(engine._h, C.byref(prm), dx, dy, dz, int(n), None if p is None else _dp(p),
                                                 d_label, C.byref(k)))
    return int(k.value)


def mapRemoveComponents(engine, connectivity=None, min_count=None, min_voxels=1, min_points=0, keep_largest=0,
                        remove_unlabelled=False, dry_run=False):
    """Remove the components that do not survive: fewer than min_voxels voxels, fewer than min_points points, or not
    among the keep_largest largest (0: off); remove_unlabelled also takes the voxels with fewer than min_count points;
    dry_run only counts.  Returns dict(n_components, n_components_removed, n_removed, n_points_removed)."""
    prm = _components_params(connectivity, min_count)
    f = MapComponentFilter()
    lib().ndt_map_component_filter_default_params(C.byref(f))
    if int(min_voxels) < 1 or int(min_points) < 0 or int(keep_largest) < 0:
        raise ValueError("min_voxels >= 1, min_points >= 0, keep_largest >= 0")
    if int(min_voxels) > 2 ** 31 - 1 or int(keep_largest) > 2 ** 31 - 1 or int(min_points) > 2 ** 63 - 1:
        raise ValueError("a filter field is out of range")
    f.min_voxels, f.min_points, f.keep_largest = int(min_voxels), int(min_points), int(keep_largest)
    f.remove_unlabelled, f.dry_run = int(bool(remove_unlabelled)), int(bool(dry_run))
    r = MapRemoveComponentsResult()
    engine._check(lib().ndt_map_remove_components(engine._h, C.byref(prm), C.byref(f), C.byref(r)))
    return {name: int(getattr(r, name)) for name, _ in MapRemoveComponentsResult._fields_}


# --- levels: the map at leaf * 2^L made from its own sums, and coarse-to-fine alignment over them (ndt_map_level_*,
# ndt_set_target_from_map_level, ndt_map_coarsen, ndt_align_map_levels).  Functions on an engine, as above.
# level 0 is the map itself in every one of them. ---
MAP_MAX_LEVEL = 6
MAP_LEVEL_STEPS_MAX = 8


def mapLevelInfo(ndt, level):
    """mapInfo() of the map's level (derived if stale): leaf, n_voxels, n_points, capacity and the tight ijk box are the
    level's, the other counters the map's."""
    mi = MapInfo()
    ndt._check(lib().ndt_map_level_info(ndt._h, int(level), C.byref(mi)))
    return dict(leaf=mi.leaf, with_intensity=bool(mi.with_intensity), n_voxels=mi.n_voxels, n_points=mi.n_points,
                n_points_dropped=mi.n_points_dropped, capacity=mi.capacity, min_ijk=tuple(mi.min_ijk),
                max_ijk=tuple(mi.max_ijk), n_adds=mi.n_adds, n_grows=mi.n_grows)


def mapExportStateLevel(ndt, level, box_min=None, box_max=None):
    """ndt.mapExportState of the map's level: the same dict, leaf being the level's; the box selects level voxels."""
    lo, hi = ndt._box_or_none(box_min, box_max)
    info = mapLevelInfo(ndt, level)
    cap = info["n_voxels"]                        # (no selection holds more)
    with_mom = ndt.mapHasMoments()
    ijk = np.zeros((cap, 3), dtype=np.int32)
    cnt = np.zeros(cap, dtype=np.int32)
    sums = np.zeros((cap, 4), dtype=np.float32)
    mom = np.zeros((cap, 9), dtype=np.float64) if with_mom else None
    m = C.c_size_t(0)
    ndt._check(lib().ndt_map_export_state_level(ndt._h, int(level), None if lo is None else _fp(lo),
                                                None if hi is None else _fp(hi), ijk.ctypes.data if cap else None,
                                                cnt.ctypes.data if cap else None, sums.ctypes.data if cap else None,
                                                mom.ctypes.data if with_mom and cap else None, cap, C.byref(m)))
    k = m.value
    return dict(leaf=info["leaf"], with_intensity=info["with_intensity"], ijk=ijk[:k], count=cnt[:k], sums=sums[:k],
                moments=None if mom is None else mom[:k])


def mapExportStateLevelDevice(ndt, level, d_ijk, d_count, d_sums, d_moments, cap, box_min=None, box_max=None):
    """Into device arrays of `cap` records (integer addresses, any may be None); returns the number of level voxels."""
    lo, hi = ndt._box_or_none(box_min, box_max)
    m = C.c_size_t(0)
    ndt._check(lib().ndt_map_export_state_level_device(ndt._h, int(level), None if lo is None else _fp(lo),
                                                       None if hi is None else _fp(hi), d_ijk, d_count, d_sums, d_moments,
                                                       int(cap), C.byref(m)))
    return int(m.value)


def setInputTargetFromMapLevel(ndt, level, box_min=None, box_max=None):
    """ndt.setInputTargetFromMapMoments of the map's level; the engine's resolution must be the level's leaf."""
    lo, hi = ndt._box_or_none(box_min, box_max)
    ndt._check(lib().ndt_set_target_from_map_level(ndt._h, int(level), None if lo is None else _fp(lo),
                                                   None if hi is None else _fp(hi)))


def mapCoarsen(ndt, level):
    """The map becomes its level: leaf * 2^level, the level's voxels; the counters of its history are kept."""
    ndt._check(lib().ndt_map_coarsen(ndt._h, int(level)))


def mapLevelsDrop(ndt):
    """Free the cached levels; the map is untouched (the next use derives them again)."""
    ndt._check(lib().ndt_map_levels_drop(ndt._h))


def alignMapLevels(ndt, steps, guess=None, half_extent=None):
    """ndt_align_map_levels: coarse-to-fine align()s against the map's levels.  `steps`: a sequence of levels, or of
    (level, max_iterations, step_size) / dict(level=, max_iterations=, step_size=) with 0 for the engine's value; every
    step sets resolution to its level's leaf, makes the level (the box guess translation +- half_extent, or all of it)
    the target and aligns from the previous step's result.  Returns the list of result dicts, one per step; raises at
    the first step that fails.  The engine's parameters are the caller's again afterwards."""
    arr = (MapLevelStep * max(len(steps), 1))()
    for i, st in enumerate(steps):
        if isinstance(st, dict):
            st = (st["level"], st.get("max_iterations", 0), st.get("step_size", 0.0))
        elif np.isscalar(st):
            st = (st, 0, 0.0)
        arr[i].level, arr[i].max_iterations, arr[i].step_size = int(st[0]), int(st[1]), float(st[2])
    if guess is not None and np.shape(guess) != (4, 4):
        raise ValueError("guess must be 4 x 4")
    if not 1 <= len(steps) <= MAP_LEVEL_STEPS_MAX:
        raise ValueError("1 to %d steps" % MAP_LEVEL_STEPS_MAX)
    g = _colmajor(np.eye(4) if guess is None else guess)
    he = None
    if half_extent is not None:
        he = np.ascontiguousarray(half_extent, dtype=np.float32)
        if he.shape != (3,):
            raise ValueError("half_extent must be three numbers")
    res = (Result * max(len(steps), 1))()
    ndt._check(lib().ndt_align_map_levels(ndt._h, arr, len(steps), None if he is None else _fp(he), _fp(g), res))
    out = []
    for i in range(len(steps)):
        d = result_to_dict(res[i])
        d["iteration_num"] = d["iterations"]
        out.append(d)
    return out


# --- distribution-to-distribution NDT: a submap's voxels (mapExportState's records) registered to the target's leaves
# (ndt_set_source_distributions, ndt_eval_derivatives_d2d, ndt_align_d2d).  Functions on an engine, as above. ---
def setSourceDistributions(ndt, state=None, count=None, moments=None):
    """The distribution source of `ndt`: the records of mapExportState (its dict as `state`, or `count` [n] and
    `moments` [n, 9]).  Each record that passes the target build's leaf rule becomes a source Gaussian.  n = 0 clears
    the source.  Returns (records, accepted)."""
    if state is not None:
        count, moments = state.get("count"), state.get("moments")
    if count is None or moments is None:
        raise ValueError("count and moments (the state of a map with moments) are needed")
    count = np.ascontiguousarray(count, dtype=np.int32)
    moments = np.ascontiguousarray(moments, dtype=np.float64)
    n = len(count)
    if count.ndim != 1 or moments.shape != (n, 9):
        raise ValueError("count must be [n] and moments [n, 9]")
    ndt._check(lib().ndt_set_source_distributions(ndt._h, count.ctypes.data if n else None, moments.ctypes.data if n else None, n))
    return sourceDistributionsInfo(ndt)


def setSourceDistributionsDevice(ndt, d_count, d_moments, n):
    """As setSourceDistributions, from device arrays (integer addresses) as mapExportStateDevice wrote them."""
    if int(n) and (not d_count or not d_moments):
        raise ValueError("device pointers are needed")
    ndt._check(lib().ndt_set_source_distributions_device(ndt._h, d_count, d_moments, int(n)))
    return sourceDistributionsInfo(ndt)


def sourceDistributionsInfo(ndt):
    """(records handed over, Gaussians accepted) of the distribution source"""
    a, b = C.c_int64(0), C.c_int64(0)
    ndt._check(lib().ndt_source_distributions_info(ndt._h, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def getSourceDistributions(ndt):
    """The accepted source Gaussians in input order: dict(mean [m, 3], cov6 [m, 6] (xx, xy, xz, yy, yz, zz), cov
    [m, 3, 3], count [m], record_index [m])."""
    m = sourceDistributionsInfo(ndt)[1]
    mean, cov6 = np.zeros((m, 3)), np.zeros((m, 6))
    count, index = np.zeros(m, np.int32), np.zeros(m, np.int32)
    got = lib().ndt_export_source_distributions(ndt._h, _dp(mean), _dp(cov6), count.ctypes.data, index.ctypes.data, m) if m else 0
    if got < 0:
        ndt._check(int(got))
    cov = cov6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(m, 3, 3)
    return dict(mean=mean, cov6=cov6, cov=cov, count=count, record_index=index)


def evalDerivativesD2D(ndt, poses6, compute_hessian=True, raw=False):
    """The D2D score, gradient and Hessian at K poses [x, y, z, roll, pitch, yaw] (K x 6): a list of dicts as
    evalDerivatives gives them; raw=True: the K x 32 packed words."""
    p = np.ascontiguousarray(np.atleast_2d(poses6), dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 6 or not np.isfinite(p).all():
        raise ValueError("poses6 must be K x 6 and finite")
    K = p.shape[0]
    out = np.zeros((K, EVAL_WORDS))
    ndt._check(lib().ndt_eval_derivatives_d2d(ndt._h, _dp(p), K, int(bool(compute_hessian)), _dp(out)))
    return out if raw else [unpack_eval(out[k]) for k in range(K)]


computeDerivativesD2D = evalDerivativesD2D


def alignDistributions(ndt, guess=None):
    """ndt_align_d2d: the distribution source registered to the target from `guess` (4x4, default identity).  Returns
    (final 4x4, result dict as getResult() gives it); getResult() keeps reporting the last align()."""
    g = _colmajor(np.eye(4) if guess is None else guess)
    r = Result()
    ndt._check(lib().ndt_align_d2d(ndt._h, _fp(g), C.byref(r)))
    d = result_to_dict(r)
    d["iteration_num"] = d["iterations"]
    return d["T"], d


# --- continuous-time NDT: a scan captured in motion, one pose per point blended between the begin pose and the end pose by
# the point's time factor (ndt_set_source_times, ndt_eval_derivatives_ct, ndt_align_ct, ndt_transform_source_ct).
# Functions on an engine, as above.  `begin`, `end`: [x, y, z, roll, pitch, yaw]. ---
def _pose6(p, what):
    a = np.ascontiguousarray(p, dtype=np.float64)
    if a.shape != (6,) or not np.isfinite(a).all():
        raise ValueError("%s must be 6 finite numbers [x, y, z, roll, pitch, yaw]" % what)
    return a


def setSourceTimes(ndt, alpha):
    """One time factor per point of the current source, in the source's order (0: start of the frame, 1: its end; the
    reference's pointsAlpha).  An empty array clears the times.  Returns the number attached."""
    a = np.ascontiguousarray(alpha, dtype=np.float32)
    if a.ndim != 1:
        raise ValueError("alpha must be [n]")
    ndt._check(lib().ndt_set_source_times(ndt._h, a.ctypes.data if len(a) else None, len(a)))
    return sourceTimesInfo(ndt)


def setSourceTimesDevice(ndt, d_alpha, n):
    """As setSourceTimes, from a device array of n floats (integer address); copied during the call."""
    if int(n) < 0 or (int(n) and not d_alpha):
        raise ValueError("a device pointer is needed")
    ndt._check(lib().ndt_set_source_times_device(ndt._h, d_alpha, int(n)))
    return sourceTimesInfo(ndt)


def sourceTimesInfo(ndt):
    """The number of times attached to the source, 0 = none"""
    n = int(lib().ndt_source_times_info(ndt._h))
    if n < 0:
        ndt._check(n)
    return n


def evalDerivativesCT(ndt, begin, poses6, compute_hessian=True, raw=False):
    """The continuous-time score, gradient and Hessian at K END poses (K x 6) with the begin pose `begin`: a list of
    dicts as evalDerivatives gives them; raw=True: the K x 32 packed words."""
    b = _pose6(begin, "begin")
    p = np.ascontiguousarray(np.atleast_2d(poses6), dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 6 or not np.isfinite(p).all():
        raise ValueError("poses6 must be K x 6 and finite")
    K = p.shape[0]
    out = np.zeros((K, EVAL_WORDS))
    ndt._check(lib().ndt_eval_derivatives_ct(ndt._h, _dp(b), _dp(p), K, int(bool(compute_hessian)), _dp(out)))
    return out if raw else [unpack_eval(out[k]) for k in range(K)]


computeDerivativesCT = evalDerivativesCT


def alignContinuousTime(ndt, begin, guess=None):
    """ndt_align_ct: the END pose of the source captured in motion, from `guess` (4x4, default identity), the begin pose
    being known.  Returns (final 4x4, result dict as getResult() gives it -- its `pose` is the end pose to hand on as
    the next scan's begin); getResult() keeps reporting the last align()."""
    b = _pose6(begin, "begin")
    g = np.asarray(np.eye(4) if guess is None else guess, dtype=np.float64)
    if g.shape != (4, 4) or not np.isfinite(g).all():
        raise ValueError("guess must be a finite 4 x 4 matrix")
    g = _colmajor(g)
    r = Result()
    ndt._check(lib().ndt_align_ct(ndt._h, _dp(b), _fp(g), C.byref(r)))
    d = result_to_dict(r)
    d["iteration_num"] = d["iterations"]
    return d["T"], d


def transformSourceCT(ndt, begin, end, frame=0):
    """The deskewed scan under begin pose `begin` and end pose `end` [n, 3] float32: frame 0 in the end pose's frame (what
    keyframePut / mapAdd take with the result), frame 1 in the target's frame.  NaN rows for non-finite points or times."""
    b, e = _pose6(begin, "begin"), _pose6(end, "end")
    if frame not in (0, 1):
        raise ValueError("frame must be 0 (the end pose's frame) or 1 (the target's frame)")
    n = ndt.sourceSize()
    out = np.zeros((n, 3), np.float32)
    ndt._check(lib().ndt_transform_source_ct(ndt._h, _dp(b), _dp(e), int(frame), out.ctypes.data, n))
    return out


def transformSourceCTDevice(ndt, begin, end, d_x, d_y, d_z, cap, frame=0):
    """As transformSourceCT, into three device arrays of `cap` floats (integer addresses)."""
    b, e = _pose6(begin, "begin"), _pose6(end, "end")
    if frame not in (0, 1) or not d_x or not d_y or not d_z or int(cap) < 0:
        raise ValueError("frame must be 0 or 1 and the three device pointers are needed")
    ndt._check(lib().ndt_transform_source_ct_device(ndt._h, _dp(b), _dp(e), int(frame), d_x, d_y, d_z, int(cap)))


# --- GICP: the point source registered to the target's kept points, plane to plane (ndt_gicp_*, ndt_eval_derivatives_gicp,
# ndt_align_gicp).  Functions on an engine, as above; their first parameter is named `engine`, not `ndt`: the API
# fuzz's vocabulary (tests/test_api_sequences_cpu.py) is every function whose first parameter is `ndt`, and these join it
# in the change that extends the fuzz.  `which`: "source" / "target" (or GICP_SOURCE / GICP_TARGET). ---
def _gicp_which(which):
    w = {"source": GICP_SOURCE, "target": GICP_TARGET, GICP_SOURCE: GICP_SOURCE, GICP_TARGET: GICP_TARGET}.get(which)
    if w is None:
        raise ValueError("which must be 'source' or 'target'")
    return w


def _gicp_cloud_size(engine, which):
    n = lib().ndt_gicp_export_neighbours(engine._h, which, None, None, 1 << 62)   # (no output: the size alone)
    if n < 0:
        engine._check(int(n))
    return int(n)


def gicpDefaultParams():
    p = GicpParams()
    lib().ndt_gicp_default_params(C.byref(p))
    return p


def gicpGetParams(engine):
    """dict of the engine's ndt_gicp_params"""
    p = GicpParams()
    engine._check(lib().ndt_gicp_get_params(engine._h, C.byref(p)))
    return {k: getattr(p, k) for k, _ in GicpParams._fields_}


def gicpSetParams(engine, **kw):
    """Changes the named fields of the engine's ndt_gicp_params (k_neighbours, max_neighbour_distance, covariance_epsilon,
    max_correspondence_distance, transformation_epsilon, max_iterations, max_inner_iterations); returns them all."""
    names = [k for k, _ in GicpParams._fields_]
    for k in kw:
        if k not in names:
            raise ValueError("unknown GICP parameter %r" % k)
    ints = ("k_neighbours", "max_iterations", "max_inner_iterations")
    for k, v in kw.items():
        if k in ints and (isinstance(v, bool) or int(v) != v):
            raise ValueError("%s must be an integer" % k)
        if np.ndim(v) != 0 or np.isnan(float(v)):
            raise ValueError("%s must be a number" % k)
    p = GicpParams()
    if engine._h is None:
        raise ValueError("the engine has no handle")
    engine._check(lib().ndt_gicp_get_params(engine._h, C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, int(v) if k in ints else float(v))
    engine._check(lib().ndt_gicp_set_params(engine._h, C.byref(p)))
    return gicpGetParams(engine)


def gicpNeighbours(engine, which="source"):
    """(idx [n, k] int32 in (d2, index) order, -1 padded; n_found [n] int32) of the source's or the target's points"""
    w = _gicp_which(which)
    n, k = _gicp_cloud_size(engine, w), gicpGetParams(engine)["k_neighbours"]
    idx, found = np.full((n, k), -1, np.int32), np.zeros(n, np.int32)
    got = lib().ndt_gicp_export_neighbours(engine._h, w, idx.ctypes.data, found.ctypes.data, n)
    if got < 0:
        engine._check(int(got))
    return idx[:got], found[:got]


def gicpCovariances(engine, which="source"):
    """dict(mean [n, 3], raw_cov6 [n, 6], cov6 [n, 6] (xx, xy, xz, yy, yz, zz), cov [n, 3, 3]); NaN rows for points
    without a covariance"""
    w = _gicp_which(which)
    n = _gicp_cloud_size(engine, w)
    mean, raw, cov6 = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 6))
    got = lib().ndt_gicp_export_covariances(engine._h, w, _dp(mean), _dp(raw), _dp(cov6), n)
    if got < 0:
        engine._check(int(got))
    mean, raw, cov6 = mean[:got], raw[:got], cov6[:got]
    return dict(mean=mean, raw_cov6=raw, cov6=cov6, cov=cov6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3))


def gicpPair(engine, pose6):
    """ndt_gicp_pair: freezes the nearest-point pairs at `pose6` [x, y, z, roll, pitch, yaw]; returns their number"""
    p = _pose6(pose6, "pose6")
    n = C.c_int64(0)
    engine._check(lib().ndt_gicp_pair(engine._h, _dp(p), C.byref(n)))
    return int(n.value)


def gicpPairs(engine):
    """(target_index [n] int32, -1 = none; d2 [n] float32, +inf for none) of the frozen pairs, in source order"""
    n = engine.sourceSize()
    idx, d2 = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    got = lib().ndt_gicp_export_pairs(engine._h, idx.ctypes.data, d2.ctypes.data, n)
    if got < 0:
        engine._check(int(got))
    return idx[:got], d2[:got]


def evalDerivativesGICP(engine, poses6, compute_hessian=True, raw=False):
    """The GICP score (-sum q / 2), gradient and Hessian over the frozen pairs at K poses (K x 6): a list of dicts as
    evalDerivatives gives them; raw=True: the K x 32 packed words."""
    p = np.ascontiguousarray(np.atleast_2d(poses6), dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 6 or not np.isfinite(p).all():
        raise ValueError("poses6 must be K x 6 and finite")
    K = p.shape[0]
    out = np.zeros((K, EVAL_WORDS))
    engine._check(lib().ndt_eval_derivatives_gicp(engine._h, _dp(p), K, int(bool(compute_hessian)), _dp(out)))
    return out if raw else [unpack_eval(out[k]) for k in range(K)]


def alignGICP(engine, guess=None):
    """ndt_align_gicp from `guess` (4x4, default identity).  Returns (final 4x4, result dict as getResult() gives it with
    `gicp`: outer / inner iterations, evaluations, pairs, points without a covariance); getResult() keeps reporting the
    last align()."""
    g = np.asarray(np.eye(4) if guess is None else guess, dtype=np.float64)
    if g.shape != (4, 4) or not np.isfinite(g).all():
        raise ValueError("guess must be a finite 4 x 4 matrix")
    g = _colmajor(g)
    r, info = Result(), GicpInfo()
    engine._check(lib().ndt_align_gicp(engine._h, _fp(g), C.byref(r), C.byref(info)))
    d = result_to_dict(r)
    d["iteration_num"] = d["iterations"]
    d["gicp"] = {k: getattr(info, k) for k, _ in GicpInfo._fields_}
    return d["T"], d


# --- Voxelised GICP: the point source against one aggregate per target leaf (ndt_vgicp_*, ndt_eval_derivatives_vgicp,
# ndt_align_vgicp).  Functions on an engine with `engine` as their first parameter, as GICP's and for the same
# reason.  The covariance rule is GICP's (gicpSetParams). ---
def vgicpVoxels(engine):
    """dict(count [L] int32, mean [L, 3], cov6 [L, 6] (xx, xy, xz, yy, yz, zz), cov [L, 3, 3]) of the target's leaves in
    getLeaves() order; NaN rows with count 0 for a leaf none of whose points contributes"""
    n = lib().ndt_vgicp_export_voxels(engine._h, None, None, None, 1 << 62)   # (no output: the size alone)
    if n < 0:
        engine._check(int(n))
    n = int(n)
    count, mean, cov6 = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros((n, 6))
    got = lib().ndt_vgicp_export_voxels(engine._h, count.ctypes.data, _dp(mean), _dp(cov6), n)
    if got < 0:
        engine._check(int(got))
    count, mean, cov6 = count[:got], mean[:got], cov6[:got]
    return dict(count=count, mean=mean, cov6=cov6, cov=cov6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3))


def vgicpInfo(engine):
    """dict of ndt_vgicp_info (the table is derived if needed; the pair fields are 0)"""
    info = VgicpInfo()
    engine._check(lib().ndt_vgicp_get_info(engine._h, C.byref(info)))
    return {k: getattr(info, k) for k, _ in VgicpInfo._fields_}


def evalDerivativesVGICP(engine, poses6, compute_hessian=True, raw=False):
    """The VGICP score (-sum N q / 2 over the voxels of every source point), gradient and Hessian at K poses (K x 6): a list
    of dicts as evalDerivatives gives them; raw=True: the K x 32 packed words."""
    p = np.ascontiguousarray(np.atleast_2d(poses6), dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 6 or not np.isfinite(p).all():
        raise ValueError("poses6 must be K x 6 and finite")
    K = p.shape[0]
    out = np.zeros((K, EVAL_WORDS))
    engine._check(lib().ndt_eval_derivatives_vgicp(engine._h, _dp(p), K, int(bool(compute_hessian)), _dp(out)))
    return out if raw else [unpack_eval(out[k]) for k in range(K)]


def alignVGICP(engine, guess=None):
    """ndt_align_vgicp from `guess` (4x4, default identity).  Returns (final 4x4, result dict as getResult() gives it with
    `vgicp`: the fields of ndt_vgicp_info); getResult() keeps reporting the last align()."""
    g = np.asarray(np.eye(4) if guess is None else guess, dtype=np.float64)
    if g.shape != (4, 4) or not np.isfinite(g).all():
        raise ValueError("guess must be a finite 4 x 4 matrix")
    g = _colmajor(g)
    r, info = Result(), VgicpInfo()
    engine._check(lib().ndt_align_vgicp(engine._h, _fp(g), C.byref(r), C.byref(info)))
    d = result_to_dict(r)
    d["iteration_num"] = d["iterations"]
    d["vgicp"] = {k: getattr(info, k) for k, _ in VgicpInfo._fields_}
    return d["T"], d


# --- Scan Context place recognition over the keyframe archive (ndt_scan_context*).  Functions on an engine, as
# above.  A descriptor is [n_rings, n_sectors] float32, its counts int32 of the same shape. ---
def scanContextDefaultParams():
    p = ScanContextParams()
    lib().ndt_scan_context_default_params(C.byref(p))
    return p


def getScanContextParams(ndt):
    """dict(n_rings, n_sectors, max_radius, z_sign, lift, min_points_per_bin) of the engine"""
    p = ScanContextParams()
    ndt._check(lib().ndt_scan_context_get_params(ndt._h, C.byref(p)))
    return {k: getattr(p, k) for k, _ in ScanContextParams._fields_}


def setScanContextParams(ndt, **kw):
    """Changes the named parameters (the others stay); a change clears the descriptor bank."""
    unknown = set(kw) - {k for k, _ in ScanContextParams._fields_}
    if unknown:
        raise ValueError("unknown Scan Context parameter(s): %s" % sorted(unknown))
    for k in ("n_rings", "n_sectors", "min_points_per_bin"):
        if k in kw and int(kw[k]) != kw[k]:
            raise ValueError("%s must be an integer" % k)
    p = ScanContextParams(**{k: (float(v) if k in ("max_radius", "z_sign", "lift") else int(v))
                             for k, v in dict(getScanContextParams(ndt), **kw).items()})
    ndt._check(lib().ndt_scan_context_set_params(ndt._h, C.byref(p)))


def scanContextSectorTable(n_sectors):
    """dir [S, 2] float32: ((float)cos(2 pi k / S), (float)sin(2 pi k / S)) as the engine uploads it (host only)"""
    if int(n_sectors) != n_sectors or not 3 <= int(n_sectors) <= 128:
        raise ValueError("n_sectors must be an integer in 3 .. 128")
    d = np.zeros((int(n_sectors), 2), np.float32)
    rc = lib().ndt_scan_context_sector_table(int(n_sectors), _fp(d))
    if rc != 0:
        raise NdtError(rc, "ndt_scan_context_sector_table")
    return d


def scanContextYaw(shift, n_sectors):
    """yaw = shift * 2 pi / S wrapped to (-pi, pi]: Rz(yaw) is the guess that aligns the query scan to the candidate"""
    s, S = int(shift), int(n_sectors)
    if S < 3 or not 0 <= s < S:
        raise ValueError("shift must lie in 0 .. n_sectors - 1")
    return (s - S if 2 * s > S else s) * (2.0 * np.pi / S)


def _sc_shape(ndt):
    p = getScanContextParams(ndt)
    return p["n_rings"], p["n_sectors"]


def _sc_desc(ndt, desc):
    d = np.asarray(desc)
    if d.ndim != 2 or d.dtype.kind not in "fiu":
        raise ValueError("a descriptor must be a [n_rings, n_sectors] array of numbers")
    d = np.ascontiguousarray(d, dtype=np.float32)
    if d.shape != _sc_shape(ndt):
        raise ValueError("the descriptor is %s, the engine's parameters say %s" % (d.shape, _sc_shape(ndt)))
    return d


def scanContext(ndt, cloud, with_count=False):
    """The Scan Context descriptor of a host cloud (N x >= 3 float32, the sensor at the origin): desc [R, S] float32, with
    with_count also the points per bin [R, S] int32."""
    a, stride, _ = _host_cloud(cloud)
    R, S = _sc_shape(ndt)
    desc, count = np.zeros((R, S), np.float32), np.zeros((R, S), np.int32)
    ndt._check(lib().ndt_scan_context(ndt._h, a.ctypes.data if len(a) else None, len(a), stride, _fp(desc),
                                      count.ctypes.data if with_count else None))
    return (desc, count) if with_count else desc


def scanContextDevice(ndt, dx, dy, dz, n, d_desc, d_count=None):
    """As scanContext from three device arrays (integer addresses) into device memory of R x S words."""
    if int(n) < 0 or not d_desc or (int(n) and (not dx or not dy or not dz)):
        raise ValueError("device pointers are needed")
    ndt._check(lib().ndt_scan_context_device(ndt._h, dx, dy, dz, int(n), d_desc, d_count))


def scanContextKeyframe(ndt, kf_id, with_count=False):
    """The descriptor of the archived scan `kf_id`, stored in the bank under the same id and returned."""
    kf_id = _sc_id(kf_id)
    R, S = _sc_shape(ndt)
    desc, count = np.zeros((R, S), np.float32), np.zeros((R, S), np.int32)
    ndt._check(lib().ndt_scan_context_keyframe(ndt._h, kf_id, _fp(desc), count.ctypes.data if with_count else None))
    return (desc, count) if with_count else desc


def _sc_id(i):
    if isinstance(i, (bool, float)) or int(i) != i:
        raise ValueError("an id must be an integer")
    return int(i)


def scanContextBankPut(ndt, bank_id, desc):
    bank_id = _sc_id(bank_id)
    d = _sc_desc(ndt, desc)
    ndt._check(lib().ndt_scan_context_bank_put(ndt._h, bank_id, _fp(d)))


def scanContextBankGet(ndt, bank_id):
    bank_id = _sc_id(bank_id)
    d = np.zeros(_sc_shape(ndt), np.float32)
    ndt._check(lib().ndt_scan_context_bank_get(ndt._h, bank_id, _fp(d)))
    return d


def scanContextBankErase(ndt, bank_id):
    ndt._check(lib().ndt_scan_context_bank_erase(ndt._h, _sc_id(bank_id)))


def scanContextBankClear(ndt):
    ndt._check(lib().ndt_scan_context_bank_clear(ndt._h))


def scanContextBankCount(ndt):
    return int(lib().ndt_scan_context_bank_count(ndt._h))


def _sc_match(ndt, call):
    m = scanContextBankCount(ndt)
    ids, dist = np.zeros(m, np.int64), np.zeros(m, np.float64)
    shift, cols = np.zeros(m, np.int32), np.zeros(m, np.int32)
    got = call(ids.ctypes.data, _dp(dist), shift.ctypes.data, cols.ctypes.data, m)
    if got < 0:
        ndt._check(int(got))
    assert got == m
    return dict(ids=ids, distance=dist, shift=shift, columns=cols)


def scanContextMatch(ndt, desc):
    """The query descriptor against every bank entry at every column shift: dict(ids, distance, shift, columns), one
    element per entry in ascending id order."""
    d = _sc_desc(ndt, desc)
    return _sc_match(ndt, lambda *a: lib().ndt_scan_context_match(ndt._h, _fp(d), *a))


def scanContextMatchKeyframe(ndt, bank_id):
    """As scanContextMatch with the bank entry `bank_id` as the query (read on the device; it is among the results)."""
    bank_id = _sc_id(bank_id)
    return _sc_match(ndt, lambda *a: lib().ndt_scan_context_match_keyframe(ndt._h, bank_id, *a))


def comm_unique_id():
    buf = C.create_string_buffer(128)
    rc = lib().ndt_comm_unique_id(buf)
    if rc != 0:
        raise NdtError(rc, "ndt_comm_unique_id")
    return buf.raw


def xy_covariance_laplace(hessian):
    """-(H[0:2,0:2])^-1 [RECALLED tier4 estimate_xy_covariance_by_Laplace_approximation]."""
    H = np.ascontiguousarray(hessian, dtype=np.float64).reshape(36)
    out = np.zeros(4)
    rc = lib().ndt_xy_covariance_laplace(_dp(H), _dp(out))
    if rc != 0:
        raise NdtError(rc, "xy block of the Hessian is singular or not finite")
    return out.reshape(2, 2)


def result_covariance(hessian, eps=1e-6, gtsam_order=True):
    """-(H + eps I)^-1 of an align() Hessian, optionally in the block order the drivers hand to
    GTSAM (ref: run/pipeline.cpp:594-603, src/registercallback.cpp:170-186)."""
    H = np.ascontiguousarray(hessian, dtype=np.float64).reshape(36)
    out = np.zeros(36)
    rc = lib().ndt_result_covariance(_dp(H), float(eps), 1 if gtsam_order else 0, _dp(out))
    if rc != 0:
        raise NdtError(rc, "Hessian + eps I is singular or not finite")
    return out.reshape(6, 6)


def newton_align(params, n_source_total, guess, eval_fn, regularization_pose=None):
    """Host Newton/More-Thuente driver with an external evaluator.

    eval_fn(pose6 ndarray, T 4x4 ndarray, compute_hessian bool) -> 32 packed doubles.
    """
    def _cb(_ctx, pose_p, T_p, need_h, out_p):
        try:
            pose = np.array([pose_p[i] for i in range(6)])
            T = np.array([T_p[i] for i in range(16)], dtype=np.float32).reshape(4, 4).T
            w = np.asarray(eval_fn(pose, T, bool(need_h)), dtype=np.float64)
            for i in range(EVAL_WORDS):
                out_p[i] = float(w[i])
            return 0
        except Exception:  # never let an exception cross the C boundary
            import traceback
            traceback.print_exc()
            return -1
    cb = EVAL_FN(_cb)
    g = _colmajor(guess)
    reg = _colmajor(regularization_pose) if regularization_pose is not None else None
    r = Result()
    rc = lib().ndt_newton_align(C.byref(params), int(n_source_total), _fp(g),
                                _fp(reg) if reg is not None else None, cb, None, C.byref(r))
    if rc != 0:
        raise NdtError(rc, "ndt_newton_align")
    return result_to_dict(r)


def newton_align_batch(params, n_source_total, guesses, batch_eval_fn, regularization_pose=None):
    """K host Newton/More-Thuente loops in lockstep with an external batched evaluator (ndt_newton_align_batch).

    batch_eval_fn(poses [n, 6], T [n, 4, 4], need_h [n] bool) -> [n, 32] packed doubles, called once per round with
    the requests of the hypotheses still running.  Returns one result dict per guess, as newton_align() does.
    """
    def _cb(_ctx, n, pose_p, T_p, need_p, out_p):
        try:
            poses = np.ctypeslib.as_array(pose_p, shape=(n * 6,)).reshape(n, 6).copy()
            T = np.ctypeslib.as_array(T_p, shape=(n * 16,)).reshape(n, 4, 4).transpose(0, 2, 1).copy()
            need = np.ctypeslib.as_array(need_p, shape=(n,)).astype(bool)
            w = np.asarray(batch_eval_fn(poses, T, need), dtype=np.float64).reshape(n, EVAL_WORDS)
            np.ctypeslib.as_array(out_p, shape=(n * EVAL_WORDS,))[:] = w.ravel()
            return 0
        except Exception:  # never let an exception cross the C boundary
            import traceback
            traceback.print_exc()
            return -1
    cb = EVAL_BATCH_FN(_cb)
    g = np.ascontiguousarray(np.stack([_colmajor(x) for x in guesses]), dtype=np.float32) if len(guesses) \
        else np.zeros((0, 16), np.float32)
    K = len(g)
    reg = _colmajor(regularization_pose) if regularization_pose is not None else None
    out = (Result * max(K, 1))()
    rc = lib().ndt_newton_align_batch(C.byref(params), int(n_source_total), _fp(g), K,
                                      _fp(reg) if reg is not None else None, cb, None, out)
    if rc != 0:
        raise NdtError(rc, "ndt_newton_align_batch")
    return [result_to_dict(out[k]) for k in range(K)]


def pack_eval(score, gradient, hessian, nvtl_sum=0.0, n_with=0, n_pairs=0):
    """Inverse of unpack_eval (for external evaluators)."""
    w = np.zeros(EVAL_WORDS)
    w[0] = score
    w[1:7] = gradient
    H = np.asarray(hessian).reshape(6, 6)
    k = 7
    for i in range(6):
        for j in range(i, 6):
            w[k] = H[i, j]
            k += 1
    w[28], w[29], w[30] = nvtl_sum, n_with, n_pairs
    return w


def _pose16d(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).T).ravel()


def svn_sample_particles(prior, K, seed=0):
    """K x 4 x 4 initial particles around `prior` (ref: svn_ndt_impl.hpp:708-716, seed explicit)."""
    out = np.zeros(16 * K)
    rc = lib().ndt_svn_sample_particles(_dp(_pose16d(prior)), K, seed, _dp(out))
    if rc != 0:
        raise NdtError(rc, "ndt_svn_sample_particles")
    return out.reshape(K, 4, 4).transpose(0, 2, 1).copy()


class SvnNormalDistributionsTransform(NormalDistributionsTransform):
    """svn_ndt::SvnNormalDistributionsTransform-shaped engine (ref: extern/svn_ndt/include/
    svn_ndt.h:100-182; driver run/pipeline_lo_svn.cpp:301-319,387-388): K pose particles,
    Stage 1 as one batched kernel launch."""

    def __init__(self, device_id=-1, **params):
        base = dict(hessian_mode=HESSIAN_GAUSS_NEWTON, add_ridge=1)  # svn_ndt.h:314, impl :650-653
        base.update(params)
        super().__init__(device_id=device_id, **base)
        self._sp = SvnParams()
        lib().ndt_svn_default_params(C.byref(self._sp))

    def setParticleCount(self, k): self._sp.particle_count = int(k)
    def setMaxIterations(self, n): self._sp.max_iterations = int(n)
    def setKernelBandwidth(self, h): self._sp.kernel_bandwidth = float(h)
    def setStepSize(self, s): self._sp.step_size = float(s)
    def setEarlyStopThreshold(self, t): self._sp.stop_threshold = float(t)
    def setUseGaussNewtonHessian(self, on):
        self._p.hessian_mode = HESSIAN_GAUSS_NEWTON if on else HESSIAN_FULL
        self._push()

    def align(self, source_cloud, prior_pose, particles=None, seed=0):
        """SvnNdtResult as a dict: final_pose, final_covariance ([rot, trans] order), converged,
        iterations (+ the final particles and stage timings)."""
        self.setInputSource(source_cloud)
        K = self._sp.particle_count
        if particles is None:
            particles = svn_sample_particles(prior_pose, K, seed)
        part = np.ascontiguousarray(np.asarray(particles, dtype=np.float64).transpose(0, 2, 1)).ravel().copy()
        if len(part) != 16 * K:
            raise ValueError("need %d particles" % K)
        r = SvnResult()
        self._check(lib().ndt_svn_align(self._h, C.byref(self._sp), _dp(_pose16d(prior_pose)), _dp(part),
                                        C.byref(r)))
        return dict(final_pose=np.array(r.final_pose[:]).reshape(4, 4).T.copy(),
                    final_covariance=np.array(r.final_covariance[:]).reshape(6, 6),
                    converged=bool(r.converged), iterations=r.iterations,
                    last_mean_update=r.last_mean_update, ms_total=r.ms_total, ms_stage1=r.ms_stage1,
                    ms_stage2=r.ms_stage2, ms_stage3=r.ms_stage3,
                    particles=part.reshape(K, 4, 4).transpose(0, 2, 1).copy())
