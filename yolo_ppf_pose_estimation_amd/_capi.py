"""ctypes declarations for libppf_hip.so (include/ppf_hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950)
into ``yolo_ppf_pose_estimation_amd/csrc/libppf_hip.so``.  Loading fails loudly when it is missing:
there is no Python or CPU fallback for the engine.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPF_HIP_LIB") or os.path.join(HERE, "csrc", "libppf_hip.so")  # override: diagnostic builds only

PPF_OPT_HIT_FRACTION, PPF_OPT_GROUP_ROUND_BUCKETS, PPF_OPT_CLUSTER_SERIAL, PPF_OPT_ACC32, PPF_OPT_TABLE_FRACTION, PPF_OPT_BATCH_REFS, PPF_OPT_RUN_STAGING = 1, 2, 3, 4, 5, 6, 7
PPF_ICP_NO_SMALL_LEVELS, PPF_ICP_ONE_STREAM, PPF_ICP_LEGACY, PPF_ICP_GRID_ALWAYS = 1, 2, 4, 8  # the first three: accepted and ignored
PPF_OK, PPF_ERR_INVALID, PPF_ERR_NOT_TRAINED, PPF_ERR_HIP, PPF_ERR_NOMEM, PPF_ERR_IO, PPF_ERR_CAPACITY = range(7)
STATUS_NAMES = {0: "PPF_OK", 1: "PPF_ERR_INVALID", 2: "PPF_ERR_NOT_TRAINED", 3: "PPF_ERR_HIP", 4: "PPF_ERR_NOMEM",
                5: "PPF_ERR_IO", 6: "PPF_ERR_CAPACITY"}


class PPFError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class TrainParams(C.Structure):
    _fields_ = [("relative_sampling_step", C.c_double), ("relative_distance_step", C.c_double),
                ("num_angles", C.c_double), ("presampled", C.c_int32), ("distance_from_distance_step", C.c_int32),
                ("max_tile_refs", C.c_int32), ("key_equality", C.c_int32), ("feature", C.c_int32),
                ("reserved", C.c_int32)]


class MatchParams(C.Structure):
    _fields_ = [("relative_scene_sample_step", C.c_double), ("relative_scene_distance", C.c_double),
                ("position_threshold", C.c_double), ("rotation_threshold", C.c_double),
                ("use_weighted_avg", C.c_int32), ("presampled", C.c_int32), ("ref_offset", C.c_int32),
                ("ref_stride", C.c_int32), ("skip_clustering", C.c_int32), ("vote_mode", C.c_int32),
                ("pair_radius", C.c_double), ("rot_metric_relative", C.c_int32), ("alpha_range_2pi", C.c_int32)]


class IcpParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("tolerance", C.c_float), ("rejection_scale", C.c_float),
                ("num_levels", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class Pose(C.Structure):
    _fields_ = [("pose", C.c_double * 16), ("q", C.c_double * 4), ("t", C.c_double * 3), ("angle", C.c_double),
                ("alpha", C.c_double), ("residual", C.c_double), ("model_index", C.c_uint32),
                ("num_votes", C.c_uint32)]


class Vote(C.Structure):
    _fields_ = [("ref_ind_max", C.c_uint32), ("alpha_ind_max", C.c_uint32), ("max_votes", C.c_uint32)]


class ModelInfo(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("num_angles", C.c_int32), ("slots", C.c_uint32), ("n_buckets", C.c_uint32),
                ("n_entries", C.c_uint64), ("n_tiles", C.c_int32), ("tile_refs", C.c_int32),
                ("angle_step", C.c_double), ("distance_step", C.c_double), ("diameter", C.c_double),
                ("position_threshold_default", C.c_double), ("rotation_threshold_default", C.c_double),
                ("device_bytes", C.c_uint64)]


class MatchStats(C.Structure):
    _fields_ = [("n_scene_sampled", C.c_int32), ("n_paired", C.c_int32), ("n_ref", C.c_int32),
                ("n_poses", C.c_int32), ("n_pairs", C.c_uint64), ("n_votes", C.c_uint64),
                ("ms_vote_kernel", C.c_float), ("ms_pair_kernel", C.c_float), ("ms_total_device", C.c_float),
                ("ms_group_kernel", C.c_float), ("n_hits", C.c_uint64), ("n_lds_atomics", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("n_batches", C.c_int32), ("n_retries", C.c_int32),
                ("n_acc32_items", C.c_uint64), ("n_tables", C.c_uint64), ("phase_clocks", C.c_uint64 * 8)]


class PoolViolation(C.Structure):
    _fields_ = [("requested_bytes", C.c_uint64), ("first_offset", C.c_int64), ("n_bytes_damaged", C.c_uint64)]


class PoolReport(C.Structure):
    _fields_ = [("n_blocks_live", C.c_uint64), ("n_blocks_checked", C.c_uint64), ("n_violations", C.c_uint64),
                ("first", PoolViolation * 8)]


class MatchPlanIn(C.Structure):
    """ppf_debug_match_plan_in: what the sizing of a match call depends on"""
    _fields_ = [("n_ref", C.c_int32), ("n_paired", C.c_int32), ("hit_frac", C.c_double), ("run_frac", C.c_double),
                ("tbl_frac", C.c_double), ("count_tables", C.c_int32), ("batch_refs_cap", C.c_int32),
                ("round_buckets_cap", C.c_int32), ("run_seg_cap", C.c_int32), ("n_buckets", C.c_uint32),
                ("tile_refs", C.c_int32), ("num_angles", C.c_int32)]


class MatchPlanOut(C.Structure):
    """ppf_debug_match_plan_out: batches, pool capacities, LDS sizes"""
    _fields_ = [("pair_chunks", C.c_int32), ("n_rounds", C.c_int32), ("round_buckets", C.c_int32), ("batch", C.c_int32),
                ("n_batches", C.c_int32), ("stripe_bits", C.c_int32), ("stripe_cap", C.c_uint32), ("sorted_cap", C.c_uint32),
                ("run_cap", C.c_uint32), ("table_cap", C.c_uint32), ("run_seg", C.c_int32), ("vote_lds", C.c_uint64),
                ("group_lds", C.c_uint64)]


class IcpPlanIn(C.Structure):
    """ppf_debug_icp_plan_in: the jobs' row counts and the four parameters the planning of a launch sequence reads"""
    _fields_ = [("n", C.c_int32 * 8), ("nd_all", C.c_int32 * 8), ("jobs", C.c_int32), ("uniform", C.c_int32),
                ("iterations", C.c_int32), ("tolerance", C.c_float), ("rejection_scale", C.c_float), ("num_levels", C.c_int32)]


class IcpPlanOut(C.Structure):
    """ppf_debug_icp_plan_out: scratch totals, table and pinned-block layout, launch shapes per level"""
    _fields_ = [(f, C.c_uint64) for f in ("t_src", "t_dst", "t_sel", "t_parts", "t_sums", "t_sumd", "g_start", "g_cur", "g_box2",
                                          "g_box1u", "state", "bb_parts", "table_bytes", "levels_off", "h_done_off",
                                          "h_state_off", "h_tables_off", "pinned_bytes")] + \
               [("first_off", C.c_uint64 * 8), ("last_off", C.c_uint64 * 8), ("max_chunks", C.c_int32),
                ("max_rows_blocks", C.c_int32), ("max_dst_blocks", C.c_int32), ("robust", C.c_int32), ("n_levels", C.c_int32),
                ("pad0", C.c_int32), ("tol_p", C.c_double * 8), ("sum_ns", C.c_int64 * 8), ("tail_lds", C.c_uint64 * 8),
                ("max_iter", C.c_int32 * 8), ("max_ns", C.c_int32 * 8), ("nn_rows", C.c_int32 * 8), ("nn_blocks", C.c_uint32 * 8),
                ("begin_blocks", C.c_uint32 * 8), ("first_level", C.c_int32 * 5 * 8), ("last_level", C.c_int32 * 5 * 8),
                ("uni", C.c_int32 * 7 * 8), ("uni_p_sel", C.c_uint64 * 8), ("uni_p_parts", C.c_uint64 * 8)]


def stats_dict(st):
    """A stats structure as a plain dict (array fields as lists)."""
    out = {}
    for name, _ in st._fields_:
        v = getattr(st, name)
        out[name] = list(v) if isinstance(v, C.Array) else v
    return out


class BatchStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_votes", C.c_uint64), ("n_hits", C.c_uint64), ("n_lds_atomics", C.c_uint64),
                ("n_matches", C.c_int32), ("n_retries", C.c_int32), ("lanes", C.c_int32), ("ms_wall", C.c_float),
                ("ms_vote_kernel", C.c_float), ("ms_pair_kernel", C.c_float), ("ms_group_kernel", C.c_float),
                ("reserved", C.c_int32)]


class FrameParams(C.Structure):
    _fields_ = [("leaf", C.c_double), ("mean_k", C.c_int32), ("stddev_mul", C.c_double), ("normal_k", C.c_int32),
                ("curvature_threshold", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class FrameStats(C.Structure):
    _fields_ = [("n_boxes", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float),
                ("reserved", C.c_int32 * 4)]


class FrameDetection(C.Structure):
    _fields_ = [("model", C.c_void_p), ("model_cloud", C.c_void_p), ("scene", C.c_void_p), ("edge", C.c_void_p)]


class MatchFrameStats(C.Structure):
    _fields_ = [("n_dets", C.c_int32), ("n_matched", C.c_int32), ("n_icp_jobs", C.c_int32), ("n_icp_launches", C.c_int32),
                ("n_icp_passes", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("ms_match", C.c_float),
                ("ms_icp", C.c_float), ("reserved", C.c_int32 * 4)]


class DepthParams(C.Structure):
    _fields_ = [("format", C.c_int32), ("flags", C.c_int32), ("depth_scale", C.c_double), ("z_min", C.c_float),
                ("z_max", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_DEPTH_F32, PPF_DEPTH_U16 = 0, 1
PPF_DEPTH_FP64 = 1  # DepthParams.flags bit


class DepthNormalParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("max_depth_change", C.c_float), ("min_neighbours", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


PPF_DEPTH_NORMALS_DROP = 1  # DepthNormalParams.flags bit
PPF_DEPTH_NORMALS_MAX_RADIUS = 8


class DepthFilterParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("range_abs", C.c_float), ("range_quad", C.c_float), ("support_abs", C.c_float),
                ("support_quad", C.c_float), ("min_support", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthFilterStats(C.Structure):
    _fields_ = [("n_kept", C.c_int32), ("n_unsupported", C.c_int32), ("n_written", C.c_int32), ("n_launches", C.c_int32),
                ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_DEPTH_FILTER_MAX_RADIUS = 8


class DepthHistoryParams(C.Structure):
    _fields_ = [("window", C.c_int32), ("range_abs", C.c_float), ("range_quad", C.c_float), ("min_support", C.c_int32),
                ("max_age", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthHistoryStats(C.Structure):
    _fields_ = [("n_kept", C.c_int32), ("n_measured", C.c_int32), ("n_filled", C.c_int32), ("n_unsupported", C.c_int32),
                ("n_empty", C.c_int32), ("n_changed", C.c_int32), ("frame", C.c_int64), ("n_launches", C.c_int32),
                ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


class DepthHistoryDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("window", C.c_int32), ("reserved0", C.c_int32), ("frames", C.c_int64),
                ("device_bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]


PPF_HISTORY_MEAN = 1  # DepthHistoryParams.flags bit
PPF_HISTORY_MAX_WINDOW = 16
PPF_HISTORY_MAX_AGE = 15
PPF_HISTORY_MEASURED, PPF_HISTORY_FILLED, PPF_HISTORY_UNSUPPORTED, PPF_HISTORY_CHANGED = 1, 2, 3, 16  # the state image


class DepthMotionParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("iters", C.c_int32 * 4), ("pyr_gate", C.c_float), ("normal_gate", C.c_float),
                ("dist_gate", C.c_float), ("normal_cos", C.c_float), ("max_step_rot", C.c_float), ("max_step_trans", C.c_float),
                ("eps_rot", C.c_float), ("eps_trans", C.c_float), ("min_pair_share", C.c_float), ("min_pairs", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthMotionLevel(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("n_source", C.c_int32),
                ("n_pairs_first", C.c_int32), ("n_pairs_last", C.c_int32), ("rmse_first", C.c_float), ("rmse_last", C.c_float),
                ("reserved", C.c_int32 * 3)]


class DepthMotionStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_evaluations", C.c_int32), ("n_enqueued", C.c_int32), ("n_launches", C.c_int32),
                ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_MOTION_MAX_LEVELS, PPF_MOTION_MAX_ITERS = 4, 64
(PPF_MOTION_NONE, PPF_MOTION_CONVERGED, PPF_MOTION_MAX_ITERS_REACHED, PPF_MOTION_LOST, PPF_MOTION_STEP,
 PPF_MOTION_SKIPPED) = range(6)  # DepthMotionLevel.status


class DepthVolumeParams(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("voxel", C.c_float), ("origin", C.c_double * 3), ("trunc", C.c_float),
                ("max_weight", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthVolumeDesc(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("voxel", C.c_float), ("origin", C.c_double * 3), ("trunc", C.c_float),
                ("max_weight", C.c_int32), ("integrations", C.c_int64), ("device_bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]


class DepthVolumeIntegrateStats(C.Structure):
    _fields_ = [("n_updated", C.c_int64), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float),
                ("reserved", C.c_int32 * 4)]


class DepthVolumeRaycastParams(C.Structure):
    _fields_ = [("z_near", C.c_float), ("z_far", C.c_float), ("ray_step", C.c_float), ("min_weight", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class DepthVolumeRaycastStats(C.Structure):
    _fields_ = [("n_hits", C.c_int32), ("n_interpolated", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


class DepthVolumeExtractParams(C.Structure):
    _fields_ = [("min_weight", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthVolumeExtractStats(C.Structure):
    _fields_ = [("n_crossings", C.c_int64), ("n_rows", C.c_int64), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


class DepthVolumeMeshParams(C.Structure):
    _fields_ = [("min_weight", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthVolumeMeshStats(C.Structure):
    _fields_ = [("n_cells", C.c_int64), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("n_no_normal", C.c_int64),
                ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


class VolumeMeshDesc(C.Structure):
    _fields_ = [("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("device_bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]


class MeshComponentParams(C.Structure):
    _fields_ = [("min_triangles", C.c_int32), ("min_area", C.c_float), ("rank_lo", C.c_int32), ("rank_hi", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class MeshComponentInfo(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("n_degenerate", C.c_int32), ("n_edges", C.c_int32),
                ("n_boundary_edges", C.c_int32), ("n_nonmanifold_edges", C.c_int32), ("first_vertex", C.c_int32), ("kept", C.c_int32),
                ("area", C.c_double), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("reserved", C.c_int32 * 2)]


class MeshComponentStats(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("n_kept", C.c_int64), ("n_unreferenced", C.c_int64), ("n_bad_area", C.c_int64),
                ("n_vertices_out", C.c_int64), ("n_triangles_out", C.c_int64), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 5)]


PPF_VOLUME_MAX_DIM, PPF_VOLUME_MAX_WEIGHT, PPF_VOLUME_MAX_STEPS, PPF_VOLUME_MAX_TILES = 1024, 65535, 4096, 16777215


class MeshSampleParams(C.Structure):
    _fields_ = [("spacing", C.c_float), ("seed", C.c_uint32), ("normals", C.c_int32), ("visibility", C.c_int32), ("map_size", C.c_int32),
                ("min_views", C.c_int32), ("depth_tol", C.c_float), ("orient", C.c_int32), ("max_rows", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class MeshSampleStats(C.Structure):
    _fields_ = [("n_triangles", C.c_int64), ("n_degenerate", C.c_int64), ("n_sampled", C.c_int64), ("n_hidden", C.c_int64),
                ("n_flipped", C.c_int64), ("n_rows", C.c_int64), ("n_large", C.c_int64), ("n_launches", C.c_int32),
                ("n_host_syncs", C.c_int32), ("area", C.c_double), ("reserved", C.c_int32 * 4)]


PPF_MESH_NORMALS_FACE, PPF_MESH_NORMALS_VERTEX, PPF_MESH_VIEWS, PPF_MESH_HOST_COUNT = 0, 1, 26, 1024


class SegmentParams(C.Structure):
    _fields_ = [("depth_abs", C.c_float), ("depth_quad", C.c_float), ("normal_cos", C.c_float), ("curvature_threshold", C.c_float),
                ("min_size", C.c_int32), ("max_size", C.c_int32), ("max_segments", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class SegmentInfo(C.Structure):
    _fields_ = [("n_pixels", C.c_int32), ("n_border", C.c_int32), ("first_pixel", C.c_int32), ("box_xywh", C.c_int32 * 4),
                ("z_lo", C.c_float), ("z_hi", C.c_float), ("reserved", C.c_int32 * 3)]


class SegmentStats(C.Structure):
    _fields_ = [("n_kept", C.c_int32), ("n_eligible", C.c_int32), ("n_smooth", C.c_int32), ("n_attached", C.c_int32),
                ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_SEGMENT_EIGHT, PPF_SEGMENT_UNORIENTED = 1, 2  # SegmentParams.flags bits


class DepthEdgeParams(C.Structure):
    _fields_ = [("depth_abs", C.c_float), ("depth_quad", C.c_float), ("max_gap", C.c_int32), ("curvature_threshold", C.c_float),
                ("select", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class DepthEdgeStats(C.Structure):
    _fields_ = [("n_kept", C.c_int32), ("n_occluding", C.c_int32), ("n_occluded", C.c_int32), ("n_boundary", C.c_int32),
                ("n_curvature", C.c_int32), ("n_edge", C.c_int32), ("n_selected", C.c_int32), ("n_no_normal", C.c_int32),
                ("n_rows", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float),
                ("reserved", C.c_int32 * 4)]


PPF_EDGE_OCCLUDING, PPF_EDGE_OCCLUDED, PPF_EDGE_BOUNDARY, PPF_EDGE_CURVATURE = 1, 2, 4, 8  # the edge mask's bits
PPF_DEPTH_EDGE_MAX_GAP = 8


class RecognizerInfo(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_bins", C.c_int32 * 4), ("in_lds", C.c_int32), ("n_keys", C.c_uint64),
                ("bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]


class RecognizeParams(C.Structure):
    _fields_ = [("max_rows", C.c_int32), ("top", C.c_int32), ("min_score", C.c_double), ("min_precision", C.c_double),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class RecognizeScore(C.Structure):
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("n_known", C.c_uint64), ("n_keys_hit", C.c_uint64),
                ("precision", C.c_double), ("recall", C.c_double), ("score", C.c_double)]


class RecognizeStats(C.Structure):
    _fields_ = [("n_clouds", C.c_int32), ("n_models", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_RECOGNIZE_MAX_MODELS, PPF_RECOGNIZE_MAX_CLOUDS, PPF_RECOGNIZE_MAX_ROWS, PPF_RECOGNIZE_MAX_TOP = 64, 256, 2048, 16


class VerifyParams(C.Structure):
    _fields_ = [("inlier_dist", C.c_float), ("normal_cos", C.c_float), ("depth_tol", C.c_float), ("model_step", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class PoseScore(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_considered", C.c_int32), ("n_inliers", C.c_int32), ("n_visible", C.c_int32),
                ("n_supported", C.c_int32), ("n_occluded", C.c_int32), ("n_violations", C.c_int32), ("inlier_rmse", C.c_float),
                ("fitness", C.c_float), ("support", C.c_float), ("score", C.c_float), ("reserved", C.c_int32 * 3)]


class VerifyStats(C.Structure):
    _fields_ = [("n_dets", C.c_int32), ("n_jobs", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_VERIFY_ALL_ROWS, PPF_VERIFY_NORMALS = 1, 2  # VerifyParams.flags bits


class RenderParams(C.Structure):
    _fields_ = [("splat_radius", C.c_float), ("visible_tol", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class RenderStats(C.Structure):
    _fields_ = [("n_dets", C.c_int32), ("n_jobs", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_RENDER_MAX_SPLAT = 8  # include/ppf_hip.h


class SelectParams(C.Structure):
    _fields_ = [("depth_tol", C.c_float), ("max_overlap", C.c_float), ("min_score", C.c_float), ("min_pixels", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class SelectInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("rank", C.c_int32), ("suppressed_by", C.c_int32), ("n_drawn", C.c_int32),
                ("n_supported", C.c_int32), ("n_overlap", C.c_int32), ("explained", C.c_float), ("key", C.c_float),
                ("reserved", C.c_int32 * 4)]


class SelectStats(C.Structure):
    _fields_ = [("n_dets", C.c_int32), ("n_jobs", C.c_int32), ("n_eligible", C.c_int32), ("n_selected", C.c_int32),
                ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


PPF_SELECT_NONE, PPF_SELECT_SELECTED, PPF_SELECT_GATED, PPF_SELECT_SUPPRESSED = 0, 1, 2, 3  # SelectInfo.status


class RefineParams(C.Structure):
    _fields_ = [("depth_gate", C.c_float), ("max_step_rot", C.c_float), ("max_step_trans", C.c_float), ("eps_rot", C.c_float),
                ("eps_trans", C.c_float), ("min_pair_share", C.c_float), ("min_pairs", C.c_int32), ("max_iters", C.c_int32),
                ("model_step", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class RefineInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("n_rows", C.c_int32), ("n_considered", C.c_int32),
                ("n_pairs_first", C.c_int32), ("n_pairs_last", C.c_int32), ("rmse_first", C.c_float), ("rmse_last", C.c_float),
                ("reserved", C.c_int32 * 4)]


class RefineStats(C.Structure):
    _fields_ = [("n_dets", C.c_int32), ("n_jobs", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32),
                ("ms_wall", C.c_float), ("reserved", C.c_int32 * 4)]


# RefineInfo.status
PPF_REFINE_NONE, PPF_REFINE_CONVERGED, PPF_REFINE_MAX_ITERS, PPF_REFINE_LOST, PPF_REFINE_STEP = 0, 1, 2, 3, 4


class Camera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k1", C.c_double),
                ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double), ("k4", C.c_double),
                ("k5", C.c_double), ("k6", C.c_double), ("max_r", C.c_double), ("reserved", C.c_double * 3)]


class RegisterParams(C.Structure):
    _fields_ = [("quad_dz_abs", C.c_float), ("quad_dz_rel", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class RegisterStats(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("n_quads", C.c_int32), ("n_quads_cut", C.c_int32), ("n_quads_oversize", C.c_int32),
                ("n_filled", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float),
                ("reserved", C.c_int32 * 4)]


PPF_CAMERA_NEWTON_ITERS, PPF_REGISTER_MAX_QUAD_PX = 7, 16  # include/ppf_hip.h


class PlaneParams(C.Structure):
    _fields_ = [("distance_threshold", C.c_float), ("n_hypotheses", C.c_int32), ("seed", C.c_uint32), ("max_planes", C.c_int32),
                ("min_inliers", C.c_int32), ("min_inlier_share", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class PlaneInfo(C.Structure):
    _fields_ = [("n", C.c_double * 3), ("d", C.c_double), ("status", C.c_int32), ("hypothesis", C.c_int32), ("n_rows", C.c_int32),
                ("n_hyp_inliers", C.c_int32), ("n_inliers", C.c_int32), ("n_behind", C.c_int32), ("refit", C.c_int32),
                ("reserved", C.c_int32)]


class PlaneStats(C.Structure):
    _fields_ = [("n_clouds", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float),
                ("reserved", C.c_int32 * 4)]


PPF_PLANE_NONE, PPF_PLANE_REMOVED, PPF_PLANE_REJECTED = 0, 1, 2  # PlaneInfo.status
PPF_PLANE_NO_REFIT, PPF_PLANE_REMOVE_BEHIND = 1, 2  # PlaneParams.flags bits
PPF_PLANE_MAX_PLANES, PPF_PLANE_MAX_HYPOTHESES = 4, 4096


class ClusterParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("min_size", C.c_int32), ("max_size", C.c_int32), ("max_clusters", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class ClusterInfo(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("first_row", C.c_int32), ("lo", C.c_float * 3), ("hi", C.c_float * 3),
                ("box_xywh", C.c_int32 * 4), ("reserved", C.c_int32 * 4)]


class ClusterStats(C.Structure):
    _fields_ = [("n_clouds", C.c_int32), ("n_launches", C.c_int32), ("n_host_syncs", C.c_int32), ("ms_wall", C.c_float),
                ("reserved", C.c_int32 * 4)]


PPF_CLUSTER_MAX_CLUSTERS = 256


class RegionParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("normal_cos", C.c_float), ("curvature_threshold", C.c_float), ("min_size", C.c_int32),
                ("max_size", C.c_int32), ("max_regions", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


PPF_REGION_UNORIENTED = 1  # RegionParams.flags bit


# every symbol include/ppf_hip.h declares (tests/test_capi_symbols.py checks the header against this)
_SIGNATURES = {
    "ppf_default_train_params": (None, [C.POINTER(TrainParams)]),
    "ppf_default_match_params": (None, [C.POINTER(MatchParams)]),
    "ppf_default_icp_params": (None, [C.POINTER(IcpParams)]),
    "ppf_abi_version": (C.c_int, []),
    "ppf_last_error": (C.c_int, [C.c_char_p, C.c_int]),
    "ppf_device_count": (C.c_int, []),
    "ppf_model_train": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(TrainParams), C.POINTER(C.c_void_p)]),
    "ppf_pair_features": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "ppf_model_retain": (C.c_int, [C.c_void_p]),
    "ppf_model_release": (C.c_int, [C.c_void_p]),
    "ppf_model_get_info": (C.c_int, [C.c_void_p, C.POINTER(ModelInfo)]),
    "ppf_model_get_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "ppf_model_trim_contexts": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "ppf_model_nearest_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int)]),
    "ppf_model_get_sampled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "ppf_model_get_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ppf_model_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "ppf_model_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "ppf_model_check_file": (C.c_int, [C.c_char_p]),
    "ppf_model_save_mem": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ppf_model_load_mem": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "ppf_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                            C.POINTER(MatchParams), C.POINTER(Pose), C.c_int, C.POINTER(C.c_int)]),
    "ppf_match_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                                  C.c_int, C.POINTER(MatchParams), C.POINTER(Pose), C.c_int, C.POINTER(C.c_int)]),
    "ppf_batch_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "ppf_batch_destroy": (C.c_int, [C.c_void_p]),
    "ppf_batch_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "ppf_batch_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int,
                                C.c_int, C.c_int, C.c_int, C.POINTER(MatchParams), C.POINTER(Pose), C.c_int, C.POINTER(C.c_int),
                                C.POINTER(BatchStats)]),
    "ppf_batch_device_block": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "ppf_batch_copy_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ppf_raw_votes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.POINTER(MatchParams), C.POINTER(Vote), C.POINTER(Pose), C.c_int,
                                C.POINTER(C.c_int), C.POINTER(MatchStats)]),
    "ppf_workspace_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "ppf_workspace_destroy": (C.c_int, [C.c_void_p]),
    "ppf_workspace_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "ppf_workspace_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "ppf_match_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.POINTER(MatchParams), C.c_void_p]),
    "ppf_workspace_results": (C.c_int, [C.c_void_p, C.POINTER(Vote), C.POINTER(Pose), C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(Pose), C.c_int, C.POINTER(C.c_int), C.POINTER(MatchStats)]),
    "ppf_workspace_ref_counters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ppf_debug_accumulators": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(MatchParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "ppf_debug_accumulators_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_int, C.POINTER(MatchParams), C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "ppf_debug_block_size": (C.c_size_t, [C.c_size_t]),
    "ppf_debug_match_plan": (C.c_int, [C.POINTER(MatchPlanIn), C.POINTER(MatchPlanOut)]),
    "ppf_debug_icp_plan": (C.c_int, [C.POINTER(IcpPlanIn), C.POINTER(IcpPlanOut)]),
    "ppf_debug_model_row_groups": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ppf_debug_device_math": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ppf_debug_pool_guard": (C.c_int, [C.c_int]),
    "ppf_debug_pool_check": (C.c_int, [C.POINTER(PoolReport)]),
    "ppf_workspace_device_poses": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "ppf_workspace_copy_top_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ppf_workspace_copy_raw_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ppf_cluster_poses_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(MatchParams),
                                           C.c_void_p]),
    "ppf_cluster_poses": (C.c_int, [C.c_void_p, C.POINTER(Pose), C.c_int, C.c_int, C.POINTER(MatchParams),
                                    C.POINTER(Pose), C.c_int, C.POINTER(C.c_int)]),
    "ppf_sample_cloud": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_int)]),
    "ppf_transform_pc_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "ppf_icp_refine": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams),
                                 C.POINTER(Pose), C.c_int, C.POINTER(C.c_int)]),
    "ppf_icp_refine_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams),
                                        C.POINTER(Pose), C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "ppf_cloud_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "ppf_cloud_set_curvature": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "ppf_cloud_release": (C.c_int, [C.c_void_p]),
    "ppf_cloud_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "ppf_cloud_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ppf_cloud_device_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "ppf_prep_crop": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                C.POINTER(C.c_void_p)]),
    "ppf_prep_voxel_grid": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_void_p)]),
    "ppf_prep_outlier_removal": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_void_p)]),
    "ppf_prep_normals": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "ppf_prep_edges": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_void_p)]),
    "ppf_prep_to_mat": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ppf_match_clouds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MatchParams), C.POINTER(Pose), C.c_int,
                                   C.POINTER(C.c_int)]),
    "ppf_icp_refine_clouds": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(IcpParams), C.POINTER(Pose), C.c_int,
                                        C.POINTER(C.c_int)]),
    "ppf_prep_knn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ppf_default_frame_params": (None, [C.POINTER(FrameParams)]),
    "ppf_match_frame": (C.c_int, [C.POINTER(FrameDetection), C.c_int, C.POINTER(MatchParams), C.POINTER(IcpParams), C.c_int,
                                  C.POINTER(Pose), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(MatchFrameStats)]),
    "ppf_prep_frame": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                 C.POINTER(FrameParams), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                 C.POINTER(FrameStats)]),
    "ppf_default_depth_params": (None, [C.POINTER(DepthParams)]),
    "ppf_cloud_from_depth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double), C.POINTER(DepthParams),
                                       C.POINTER(C.c_void_p)]),
    "ppf_cloud_from_depth_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double),
                                              C.POINTER(DepthParams), C.c_void_p, C.POINTER(C.c_void_p)]),
    "ppf_default_depth_normal_params": (None, [C.POINTER(DepthNormalParams)]),
    "ppf_cloud_from_depth_normals": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double), C.POINTER(DepthParams),
                                               C.POINTER(DepthNormalParams), C.POINTER(C.c_void_p)]),
    "ppf_cloud_from_depth_normals_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double),
                                                      C.POINTER(DepthParams), C.POINTER(DepthNormalParams), C.c_void_p,
                                                      C.POINTER(C.c_void_p)]),
    "ppf_default_depth_filter_params": (None, [C.POINTER(DepthFilterParams)]),
    "ppf_depth_filter": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(DepthParams), C.POINTER(DepthFilterParams),
                                   C.c_void_p, C.POINTER(DepthFilterStats)]),
    "ppf_depth_filter_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(DepthParams),
                                          C.POINTER(DepthFilterParams), C.c_void_p, C.c_void_p, C.POINTER(DepthFilterStats)]),
    "ppf_default_depth_history_params": (None, [C.POINTER(DepthHistoryParams)]),
    "ppf_depth_history_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(DepthParams), C.POINTER(DepthHistoryParams), C.POINTER(C.c_void_p)]),
    "ppf_depth_history_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(DepthHistoryStats)]),
    "ppf_depth_history_push_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(DepthHistoryStats)]),
    "ppf_depth_history_reset": (C.c_int, [C.c_void_p]),
    "ppf_depth_history_info": (C.c_int, [C.c_void_p, C.POINTER(DepthHistoryDesc)]),
    "ppf_depth_history_release": (C.c_int, [C.c_void_p]),
    "ppf_default_depth_motion_params": (None, [C.POINTER(DepthMotionParams)]),
    "ppf_depth_motion": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double),
                                   C.POINTER(DepthParams), C.POINTER(DepthMotionParams), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(DepthMotionLevel), C.POINTER(DepthMotionStats)]),
    "ppf_depth_motion_device": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(DepthParams), C.POINTER(DepthMotionParams), C.POINTER(C.c_double), C.c_void_p,
                                          C.POINTER(C.c_double), C.POINTER(DepthMotionLevel), C.POINTER(DepthMotionStats)]),
    "ppf_default_depth_volume_params": (None, [C.POINTER(DepthVolumeParams)]),
    "ppf_default_depth_volume_raycast_params": (None, [C.POINTER(DepthVolumeRaycastParams)]),
    "ppf_default_depth_volume_extract_params": (None, [C.POINTER(DepthVolumeExtractParams)]),
    "ppf_depth_volume_create": (C.c_int, [C.POINTER(DepthVolumeParams), C.POINTER(C.c_void_p)]),
    "ppf_debug_depth_volume_shell": (C.c_int, [C.POINTER(DepthVolumeParams), C.POINTER(C.c_void_p)]),
    "ppf_depth_volume_release": (C.c_int, [C.c_void_p]),
    "ppf_depth_volume_reset": (C.c_int, [C.c_void_p]),
    "ppf_depth_volume_info": (C.c_int, [C.c_void_p, C.POINTER(DepthVolumeDesc)]),
    "ppf_depth_volume_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ppf_depth_volume_integrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double),
                                             C.POINTER(DepthParams), C.POINTER(C.c_double), C.POINTER(DepthVolumeIntegrateStats)]),
    "ppf_depth_volume_integrate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double),
                                                    C.POINTER(DepthParams), C.POINTER(C.c_double), C.c_void_p,
                                                    C.POINTER(DepthVolumeIntegrateStats)]),
    "ppf_depth_volume_raycast": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(DepthVolumeRaycastParams), C.c_void_p, C.c_void_p, C.POINTER(DepthVolumeRaycastStats)]),
    "ppf_depth_volume_raycast_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                  C.POINTER(DepthVolumeRaycastParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(DepthVolumeRaycastStats)]),
    "ppf_depth_volume_extract": (C.c_int, [C.c_void_p, C.POINTER(DepthVolumeExtractParams), C.POINTER(C.c_void_p),
                                           C.POINTER(DepthVolumeExtractStats)]),
    "ppf_depth_volume_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ppf_default_depth_volume_mesh_params": (None, [C.POINTER(DepthVolumeMeshParams)]),
    "ppf_depth_volume_mesh": (C.c_int, [C.c_void_p, C.POINTER(DepthVolumeMeshParams), C.POINTER(C.c_void_p),
                                        C.POINTER(DepthVolumeMeshStats)]),
    "ppf_volume_mesh_info": (C.c_int, [C.c_void_p, C.POINTER(VolumeMeshDesc)]),
    "ppf_volume_mesh_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "ppf_volume_mesh_release": (C.c_int, [C.c_void_p]),
    "ppf_volume_mesh_upload": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "ppf_debug_volume_mesh_shell": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "ppf_default_mesh_component_params": (None, [C.POINTER(MeshComponentParams)]),
    "ppf_volume_mesh_components": (C.c_int, [C.c_void_p, C.POINTER(MeshComponentParams), C.POINTER(C.c_void_p), C.c_void_p,
                                             C.POINTER(MeshComponentInfo), C.c_int, C.POINTER(MeshComponentStats)]),
    "ppf_default_mesh_sample_params": (None, [C.POINTER(MeshSampleParams)]),
    "ppf_cloud_from_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(MeshSampleParams),
                                      C.POINTER(C.c_void_p), C.POINTER(MeshSampleStats)]),
    "ppf_default_segment_params": (None, [C.POINTER(SegmentParams)]),
    "ppf_depth_segments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(DepthParams), C.c_void_p,
                                     C.POINTER(SegmentParams), C.c_void_p, C.POINTER(SegmentInfo), C.POINTER(C.c_int32),
                                     C.POINTER(SegmentStats)]),
    "ppf_depth_segments_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(DepthParams), C.c_void_p,
                                            C.POINTER(SegmentParams), C.c_void_p, C.c_void_p, C.POINTER(SegmentInfo),
                                            C.POINTER(C.c_int32), C.POINTER(SegmentStats)]),
    "ppf_default_depth_edge_params": (None, [C.POINTER(DepthEdgeParams)]),
    "ppf_depth_edges": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double), C.POINTER(DepthParams), C.c_void_p,
                                  C.POINTER(DepthEdgeParams), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(DepthEdgeStats)]),
    "ppf_depth_edges_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_double), C.POINTER(DepthParams),
                                         C.c_void_p, C.POINTER(DepthEdgeParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                         C.POINTER(DepthEdgeStats)]),
    "ppf_recognizer_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "ppf_recognizer_retain": (C.c_int, [C.c_void_p]),
    "ppf_recognizer_release": (C.c_int, [C.c_void_p]),
    "ppf_recognizer_model_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RecognizerInfo)]),
    "ppf_recognizer_keys": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "ppf_default_recognize_params": (None, [C.POINTER(RecognizeParams)]),
    "ppf_recognize_frame": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(RecognizeParams), C.c_void_p, C.c_void_p,
                                      C.POINTER(RecognizeScore), C.POINTER(C.c_int32), C.POINTER(RecognizeStats)]),
    "ppf_default_verify_params": (None, [C.POINTER(VerifyParams)]),
    "ppf_verify_frame": (C.c_int, [C.POINTER(FrameDetection), C.c_int, C.POINTER(Pose), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int,
                                   C.c_int, C.POINTER(C.c_double), C.POINTER(VerifyParams), C.POINTER(PoseScore), C.POINTER(C.c_int),
                                   C.POINTER(VerifyStats)]),
    "ppf_default_render_params": (None, [C.POINTER(RenderParams)]),
    "ppf_verify_frame_rendered": (C.c_int, [C.POINTER(FrameDetection), C.c_int, C.POINTER(Pose), C.POINTER(C.c_int), C.c_int, C.c_void_p,
                                            C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(VerifyParams), C.POINTER(RenderParams),
                                            C.POINTER(PoseScore), C.POINTER(C.c_int), C.POINTER(VerifyStats)]),
    "ppf_render_frame": (C.c_int, [C.POINTER(FrameDetection), C.c_int, C.POINTER(Pose), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_double), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.POINTER(RenderStats)]),
    "ppf_default_select_params": (None, [C.POINTER(SelectParams)]),
    "ppf_select_frame": (C.c_int, [C.POINTER(FrameDetection), C.c_int, C.POINTER(Pose), C.POINTER(C.c_int), C.c_int, C.POINTER(PoseScore),
                                   C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(RenderParams), C.POINTER(SelectParams),
                                   C.POINTER(SelectInfo), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                   C.POINTER(SelectStats)]),
    "ppf_default_refine_params": (None, [C.POINTER(RefineParams)]),
    "ppf_refine_frame": (C.c_int, [C.POINTER(FrameDetection), C.c_int, C.POINTER(Pose), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int,
                                   C.c_int, C.POINTER(C.c_double), C.POINTER(RefineParams), C.POINTER(Pose), C.POINTER(RefineInfo),
                                   C.POINTER(RefineStats)]),
    "ppf_default_camera": (None, [C.POINTER(Camera), C.c_double, C.c_double, C.c_double, C.c_double]),
    "ppf_camera_project": (C.c_int, [C.POINTER(Camera), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ppf_camera_unproject": (C.c_int, [C.POINTER(Camera), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ppf_camera_map_boxes": (C.c_int, [C.POINTER(Camera), C.POINTER(Camera), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ppf_depth_map_create": (C.c_int, [C.POINTER(Camera), C.c_int, C.c_int, C.POINTER(Camera), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_void_p)]),
    "ppf_depth_map_release": (C.c_int, [C.c_void_p]),
    "ppf_depth_map_rays": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ppf_default_register_params": (None, [C.POINTER(RegisterParams)]),
    "ppf_depth_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(DepthParams), C.POINTER(RegisterParams), C.c_void_p,
                                     C.POINTER(RegisterStats)]),
    "ppf_depth_register_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(DepthParams), C.POINTER(RegisterParams),
                                            C.c_void_p, C.c_void_p, C.POINTER(RegisterStats)]),
    "ppf_default_plane_params": (None, [C.POINTER(PlaneParams)]),
    "ppf_prep_planes": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(PlaneParams), C.POINTER(C.c_void_p), C.POINTER(PlaneInfo),
                                  C.POINTER(C.c_void_p), C.POINTER(PlaneStats)]),
    "ppf_prep_planes_apply": (C.c_int, [C.c_void_p, C.POINTER(PlaneInfo), C.c_int, C.POINTER(PlaneParams), C.POINTER(C.c_void_p)]),
    "ppf_default_cluster_params": (None, [C.POINTER(ClusterParams)]),
    "ppf_prep_clusters": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(ClusterParams), C.POINTER(C.c_double), C.c_int, C.c_int,
                                    C.POINTER(C.c_void_p), C.POINTER(ClusterInfo), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                    C.POINTER(ClusterStats)]),
    "ppf_default_region_params": (None, [C.POINTER(RegionParams)]),
    "ppf_prep_regions": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(RegionParams), C.POINTER(C.c_double), C.c_int, C.c_int,
                                   C.POINTER(C.c_void_p), C.POINTER(ClusterInfo), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                   C.POINTER(ClusterStats)]),
    "ppf_icp_register": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
}

PPF_FEATURE_PPF, PPF_FEATURE_DARBOUX = 0, 1
PPF_ABI_VERSION = 4   # include/ppf_hip.h
PPF_NOFF_MAT = 3      # x y z nx ny nz rows (the N x 6 Mat of CloudProcessing.h:163-190)
PPF_NOFF_PCL = 4      # pcl::PointNormal rows: x y z 1 | nx ny nz 0 | curvature pad pad pad (stride 12)

_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as the system
    one libppf_hip.so is linked against).  Whichever copy is loaded first serves every later user of that SONAME -- but
    torch opens its copy by path, so when the system runtime came first the process ends up with two runtimes and
    torch sees "No HIP GPUs".  Loading torch's copy first (by path, without importing torch) makes both agree,
    whatever the import order.  Without torch installed nothing happens and the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libppf_hip.so; raises (never falls back) when the extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()').  There is no CPU fallback.")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if L.ppf_abi_version() != PPF_ABI_VERSION:
            raise ImportError("libppf_hip.so ABI version mismatch")
        _lib = L
    return _lib


def last_error() -> str:
    buf = C.create_string_buffer(1024)
    lib().ppf_last_error(buf, 1024)
    return buf.value.decode("utf-8", "replace")


def check(status: int):
    if status != PPF_OK:
        raise PPFError(status, last_error())
