"""ctypes loader of the C-ABI library (include/elimaloc_hip.h -> elimaloc_amd/libelimaloc_hip.so).

There is no CPU fallback: a missing library or a missing gfx950 device raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ELM_LIB") or os.path.join(_HERE, "libelimaloc_hip.so")  # ELM_LIB: developer A/B of prebuilt variants

ELM_OK = 0
P2P, GICP, VGICP, AVGICP = 0, 1, 2, 3
MAX_ITER_TRACE = 64
PACKED_SUMS = 32
COMM_ID_BYTES = 128


class ElmError(RuntimeError):
    pass


class RegConfig(C.Structure):
    """POD mirror of RegistrationConfig (reg.hpp:62-85)."""
    _fields_ = [
        ("i_max_thread", C.c_int32),
        ("icp_method", C.c_int32),
        ("voxel_search_method", C.c_int32),
        ("use_radar_cov", C.c_int32),
        ("max_iteration", C.c_int32),
        ("b_debug_print", C.c_int32),
        ("gicp_cov_search_dist", C.c_double),
        ("max_search_dist", C.c_double),
        ("lm_lambda", C.c_double),
        ("icp_termination_threshold_m", C.c_double),
        ("min_overlap_ratio", C.c_double),
        ("max_fitness_score", C.c_double),
        ("doppler_trans_lambda", C.c_double),
        ("range_variance_m", C.c_double),
        ("azimuth_variance_deg", C.c_double),
        ("elevation_variance_deg", C.c_double),
        ("ego_to_lidar_trans", C.c_double * 3),
        ("ego_to_lidar_rot", C.c_double * 9),
        ("ego_to_imu_rot", C.c_double * 9),
    ]


class IterTrace(C.Structure):
    _fields_ = [
        ("JTJ", C.c_double * 36),
        ("JTr", C.c_double * 6),
        ("residual_sum", C.c_double),
        ("n_corr", C.c_double),
        ("x", C.c_double * 6),
        ("step_norm", C.c_double),
        ("T", C.c_double * 16),
    ]


class RegResult(C.Structure):
    _fields_ = [
        ("T", C.c_double * 16),
        ("fitness_score", C.c_double),
        ("d_fitness", C.c_double),
        ("local_cov", C.c_double * 36),
        ("is_success", C.c_int32),
        ("iterations", C.c_int32),
        ("gate", C.c_int32),
        ("path", C.c_int32),
        ("n_corr_last", C.c_double),
        ("point_iterations", C.c_double),
        ("n_cand_total", C.c_double),
        ("n_occ_total", C.c_double),
        ("fallback_blocks", C.c_double),
        ("n_tested_total", C.c_double),
    ]


class Profile(C.Structure):
    _fields_ = [
        ("accumulate_launches", C.c_uint64),
        ("solve_steps", C.c_uint64),
        ("accumulate_ms", C.c_double),
        ("solve_ms", C.c_double),
    ]


class MapInfo(C.Structure):
    _fields_ = [
        ("n_input_points", C.c_uint64),
        ("n_points", C.c_uint64),
        ("n_voxels", C.c_uint64),
        ("hash_capacity", C.c_uint64),
        ("voxel_size", C.c_double),
        ("max_points_per_voxel", C.c_int32),
        ("has_voxel_cov", C.c_int32),
        ("has_point_cov", C.c_int32),
        ("layout_flags", C.c_int32),
        ("device_bytes", C.c_uint64),
        ("n_query_voxels", C.c_uint64),
        ("nbr_entries", C.c_uint64),
        ("index_bytes", C.c_uint64),
        ("index_part_bytes", C.c_uint64 * 4),
        ("n_list_voxels", C.c_uint64),
    ]


class DeskewTables(C.Structure):
    _fields_ = [
        ("d_time_scan_cur", C.c_double),
        ("d_time_scan_end", C.c_double),
        ("i_imu_pointer_cur", C.c_int32),
        ("b_run_deskew", C.c_int32),
        ("b_is_imu_available", C.c_int32),
        ("b_is_odom_available", C.c_int32),
        ("f_odom_incre_x", C.c_float),
        ("f_odom_incre_y", C.c_float),
        ("f_odom_incre_z", C.c_float),
        ("_pad", C.c_float),
        ("vec_d_imu_time", C.POINTER(C.c_double)),
        ("vec_d_imu_rot_x", C.POINTER(C.c_double)),
        ("vec_d_imu_rot_y", C.POINTER(C.c_double)),
        ("vec_d_imu_rot_z", C.POINTER(C.c_double)),
    ]


class RelocConfigC(C.Structure):
    """elm_reloc_config (include/elimaloc_hip.h, relocalization)."""
    _fields_ = [("radius_xy_m", C.c_double), ("step_xy_m", C.c_double), ("yaw_range_deg", C.c_double), ("step_yaw_deg", C.c_double),
                ("score_max_range_m", C.c_double), ("max_score_points", C.c_int32), ("top_k", C.c_int32), ("nms_xy_m", C.c_double),
                ("nms_yaw_deg", C.c_double), ("lds_budget_bytes", C.c_int64), ("bitmap_max_bytes", C.c_int64)]


class RelocCandidate(C.Structure):
    """elm_reloc_candidate: a kept hypothesis (T0) and its ICP result (T), column-major."""
    _fields_ = [("T0", C.c_double * 16), ("T", C.c_double * 16), ("score", C.c_uint32), ("hyp_index", C.c_int32),
                ("is_success", C.c_int32), ("iterations", C.c_int32), ("fitness_score", C.c_double)]


class GlobalRelocConfigC(C.Structure):
    """elm_reloc_global_config (include/elimaloc_hip.h, global relocalization)."""
    _fields_ = [("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double), ("step_xy_m", C.c_double),
                ("step_yaw_deg", C.c_double), ("score_max_range_m", C.c_double), ("score_min_height_m", C.c_double),
                ("max_score_points", C.c_int32), ("top_k", C.c_int32), ("nms_xy_m", C.c_double), ("nms_yaw_deg", C.c_double),
                ("pool_min", C.c_int32), ("max_kz_span", C.c_int32), ("bitmap_max_bytes", C.c_int64)]


class GlobalRelocStats(C.Structure):
    """elm_reloc_global_stats: lattice size, pruning per level, leaves scored, timings of one elm_relocalize_global."""
    _fields_ = [("lattice_poses", C.c_int64), ("valid_leaves", C.c_int64), ("nx", C.c_int32), ("ny", C.c_int32), ("n_yaw", C.c_int32),
                ("levels", C.c_int32), ("n_counted", C.c_int32), ("passes", C.c_int32), ("tau", C.c_uint32), ("_pad", C.c_uint32),
                ("nodes_bounded", C.c_int64 * 24), ("nodes_kept", C.c_int64 * 24), ("leaves_scored", C.c_int64), ("point_evals", C.c_int64),
                ("ms_ground", C.c_double), ("ms_search", C.c_double), ("ms_refine", C.c_double)]


class FreeSpaceConfigC(C.Structure):
    """elm_freespace_config (include/elimaloc_hip.h, free-space check)."""
    _fields_ = [("sub", C.c_int32), ("min_hits", C.c_int32), ("max_samples", C.c_int32), ("_pad", C.c_int32), ("step_m", C.c_double),
                ("start_m", C.c_double), ("min_range_m", C.c_double), ("max_range_m", C.c_double), ("end_margin_m", C.c_double),
                ("end_margin_frac", C.c_double), ("origin", C.c_double * 3)]


class FreeSpaceStatsC(C.Structure):
    """elm_freespace_stats: the counts of one pose."""
    _fields_ = [("n_counted", C.c_uint32), ("n_pierced", C.c_uint32), ("n_end_occupied", C.c_uint32), ("n_supported", C.c_uint32),
                ("n_samples", C.c_uint64), ("n_hit_samples", C.c_uint64)]


class RayCastConfigC(C.Structure):
    """elm_raycast_config (include/elimaloc_hip.h, ray casting)."""
    _fields_ = [("sub", C.c_int32), ("max_steps", C.c_int32), ("min_range_m", C.c_double), ("max_range_m", C.c_double),
                ("cmp_min_range_m", C.c_double), ("cmp_max_range_m", C.c_double), ("tol_m", C.c_double), ("tol_frac", C.c_double),
                ("origin", C.c_double * 3)]


class RayCastStatsC(C.Structure):
    """elm_raycast_stats: the counts of one pose."""
    _fields_ = [("n_cast", C.c_uint32), ("n_hit", C.c_uint32), ("n_miss", C.c_uint32), ("n_truncated", C.c_uint32),
                ("n_compared", C.c_uint32), ("n_match", C.c_uint32), ("n_through", C.c_uint32), ("n_front", C.c_uint32),
                ("n_steps", C.c_uint64)]


class EvidenceConfigC(C.Structure):
    """elm_evidence_config (include/elimaloc_hip.h, map evidence)."""
    _fields_ = [("sub", C.c_int32), ("max_steps", C.c_int32), ("min_range_m", C.c_double), ("obs_min_range_m", C.c_double),
                ("obs_max_range_m", C.c_double), ("end_margin_m", C.c_double), ("end_margin_frac", C.c_double), ("origin", C.c_double * 3)]


class EvidenceStatsC(C.Structure):
    """elm_evidence_stats: the counts of one observation."""
    _fields_ = [("n_cast", C.c_uint32), ("n_observing", C.c_uint32), ("n_walked", C.c_uint32), ("n_truncated", C.c_uint32),
                ("n_through_beams", C.c_uint32), ("n_end_hit", C.c_uint32), ("n_end_free", C.c_uint32), ("_pad", C.c_uint32),
                ("n_through_events", C.c_uint64), ("n_steps", C.c_uint64)]


class EvidenceRuleC(C.Structure):
    """elm_evidence_rule: when a cell's counters make it stale."""
    _fields_ = [("min_through", C.c_uint32), ("through_per_hit", C.c_uint32)]


class GrowthConfigC(C.Structure):
    """elm_growth_config (include/elimaloc_hip.h, map growth): the evidence config's fields plus clearance_cells."""
    _fields_ = [("sub", C.c_int32), ("max_steps", C.c_int32), ("min_range_m", C.c_double), ("obs_min_range_m", C.c_double),
                ("obs_max_range_m", C.c_double), ("end_margin_m", C.c_double), ("end_margin_frac", C.c_double), ("origin", C.c_double * 3),
                ("clearance_cells", C.c_int32), ("_pad", C.c_int32)]


class GrowthStatsC(C.Structure):
    """elm_growth_stats: the counts of one observation."""
    _fields_ = [("n_cast", C.c_uint32), ("n_observing", C.c_uint32), ("n_walked", C.c_uint32), ("n_truncated", C.c_uint32),
                ("n_end_hit", C.c_uint32), ("n_end_near", C.c_uint32), ("n_end_new", C.c_uint32), ("n_end_out", C.c_uint32),
                ("n_through_beams", C.c_uint32), ("n_dropped", C.c_uint32), ("n_through_events", C.c_uint64), ("n_steps", C.c_uint64)]


class GrowthRuleC(C.Structure):
    """elm_growth_rule: when a candidate cell's counters make it appeared."""
    _fields_ = [("min_hit", C.c_uint32), ("hit_per_through", C.c_uint32)]


class GrowthObjectRuleC(C.Structure):
    """elm_growth_object_rule (include/elimaloc_hip.h, map growth: objects): the member rule, the connectivity, the smallest object."""
    _fields_ = [("min_hit", C.c_uint32), ("hit_per_through", C.c_uint32), ("connectivity", C.c_uint32), ("min_cells", C.c_uint32)]


class GrowthObjectC(C.Structure):
    """elm_growth_object: one listed component."""
    _fields_ = [("label", C.c_int32 * 3), ("n_cells", C.c_uint32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("hit", C.c_uint64),
                ("through", C.c_uint64), ("cell_sum", C.c_uint64 * 3)]


class GrowthObjectStatsC(C.Structure):
    """elm_growth_object_stats: the counts of one labelling."""
    _fields_ = [("n_members", C.c_uint32), ("n_objects", C.c_uint32), ("n_small", C.c_uint32), ("n_small_cells", C.c_uint32),
                ("max_cells", C.c_uint32), ("_pad", C.c_uint32)]


class CellGridDesc(C.Structure):
    """elm_cell_grid_desc: the cell grid's fields of the map's view and the counts of its arrays."""
    _fields_ = [(n, C.c_int32) for n in ("gx0", "gy0", "gz0", "gnx", "gny", "gnz", "vx0", "vy0", "vz0", "vnx", "vny", "vnz", "gtny",
                                          "grid_tiled", "grid_wide")] + [("grid_nslots", C.c_uint32), ("n_start_words", C.c_uint64),
                                                                         ("n_blocks", C.c_uint64), ("n_tiles", C.c_uint64)]


INDEX_BUILD_HOST, INDEX_BUILD_DEVICE, INDEX_STAGES = 0, 1, 5


class BuildSourcesC(C.Structure):
    """elm_build_sources (include/elimaloc_hip.h, device map build from resident sources)."""
    _fields_ = [("base", C.c_void_p), ("keep_within", C.c_int32), ("keep_center", C.c_double * 3), ("keep_radius_m", C.c_double),
                ("scans", C.POINTER(C.c_void_p)), ("poses16", C.POINTER(C.c_double)), ("n_jobs", C.c_int32)]


class BuildSourcesStatsC(C.Structure):
    """elm_build_sources_stats: the counts of one elm_map_build_device_from."""
    _fields_ = [(n, C.c_uint64) for n in ("n_base_kept", "n_base_dropped", "n_scan_points", "n_points", "n_voxels")]


class OdometryConfigC(C.Structure):
    """elm_odometry_config (include/elimaloc_hip.h, LiDAR odometry on a rolling local map)."""
    _fields_ = [("voxel_size", C.c_double), ("max_points_per_voxel", C.c_int32), ("max_range_m", C.c_double),
                ("key_min_trans_m", C.c_double), ("key_min_rot_rad", C.c_double), ("reg", RegConfig)]


class OdometryStepC(C.Structure):
    """elm_odometry_step: what one elm_odometry_step_scan did."""
    _fields_ = [("T", C.c_double * 16), ("registered", C.c_int32), ("is_success", C.c_int32), ("inserted", C.c_int32), ("reg", RegResult),
                ("build", BuildSourcesStatsC)]

class PlacesConfigC(C.Structure):
    """elm_places_config (include/elimaloc_hip.h, place recognition)."""
    _fields_ = [("n_rings", C.c_int32), ("n_layers", C.c_int32), ("r_min_m", C.c_double), ("r_max_m", C.c_double),
                ("z_min_m", C.c_double), ("z_max_m", C.c_double)]


class PlacesStatsC(C.Structure):
    """elm_places_stats: the counts of one described scan."""
    _fields_ = [("n_points", C.c_uint32), ("n_used", C.c_uint32), ("n_bits", C.c_uint32)]


class PlacesQueryConfigC(C.Structure):
    """elm_places_query_config: the selection of one query."""
    _fields_ = [("top_k", C.c_int32), ("min_dice_q16", C.c_uint32), ("exclude_id_lo", C.c_int64), ("exclude_id_hi", C.c_int64)]


class PlaceMatchC(C.Structure):
    """elm_place_match: one (query, entry) pair."""
    _fields_ = [("dice_q16", C.c_uint32), ("inter", C.c_uint16), ("shift", C.c_uint16)]


class PlaceCandidateC(C.Structure):
    """elm_place_candidate: one selected entry of a query."""
    _fields_ = [("entry", C.c_uint32), ("dice_q16", C.c_uint32), ("id", C.c_int64), ("inter", C.c_uint16), ("shift", C.c_uint16),
                ("_pad", C.c_uint32), ("yaw_rad", C.c_double)]


PLACES_SECTORS, PLACES_MAX_TOP_K = 64, 16


class PoseGraphConfigC(C.Structure):
    """elm_posegraph_config (include/elimaloc_hip.h, pose graph)."""
    _fields_ = [("max_iterations", C.c_int32), ("pcg_max_iterations", C.c_int32), ("pcg_check_every", C.c_int32), ("_pad", C.c_int32),
                ("lambda_init", C.c_double), ("lambda_up", C.c_double), ("lambda_down", C.c_double), ("lambda_min", C.c_double),
                ("lambda_max", C.c_double), ("cost_rel_tol", C.c_double), ("step_tol", C.c_double), ("pcg_rel_tol", C.c_double),
                ("huber_k", C.c_double)]


class PoseGraphLinearizeStatsC(C.Structure):
    """elm_posegraph_linearize_stats."""
    _fields_ = [("chi2", C.c_double), ("cost", C.c_double), ("grad_inf_norm", C.c_double), ("n_outliers", C.c_int64)]


class PoseGraphSolveStatsC(C.Structure):
    """elm_posegraph_solve_stats."""
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("rel_residual", C.c_double)]


class PoseGraphResultC(C.Structure):
    """elm_posegraph_result."""
    _fields_ = [("solves", C.c_int32), ("accepted", C.c_int32), ("rejected", C.c_int32), ("stop_reason", C.c_int32),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("lambda_final", C.c_double), ("pcg_iterations_total", C.c_int64)]


class PoseGraphTraceC(C.Structure):
    """elm_posegraph_trace: one solve of an optimize call."""
    _fields_ = [("cost", C.c_double), ("lambda_", C.c_double), ("accepted", C.c_int32), ("pcg_iterations", C.c_int32)]


class PoseGraphInitConfigC(C.Structure):
    """elm_posegraph_init_config (include/elimaloc_hip_posegraph_init.h)."""
    _fields_ = [("pcg_rel_tol", C.c_double), ("pcg_max_iterations", C.c_int32), ("pcg_check_every", C.c_int32), ("stages", C.c_int32),
                ("reserved", C.c_int32)]


class PoseGraphInitResultC(C.Structure):
    """elm_posegraph_init_result."""
    _fields_ = [("cost_before", C.c_double), ("cost_after", C.c_double), ("rot_rel_residual", C.c_double), ("trans_rel_residual", C.c_double),
                ("rot_iterations", C.c_int32), ("trans_iterations", C.c_int32), ("rot_converged", C.c_int32), ("trans_converged", C.c_int32),
                ("degenerate_nodes", C.c_int32), ("applied", C.c_int32)]


class PoseGraphInitPriorConfigC(C.Structure):
    """elm_posegraph_init_prior_config (include/elimaloc_hip_posegraph_init_prior.h)."""
    _fields_ = [("base", PoseGraphInitConfigC), ("align_min_ratio", C.c_double)]


class PoseGraphInitPriorResultC(C.Structure):
    """elm_posegraph_init_prior_result."""
    _fields_ = [("base", PoseGraphInitResultC), ("pre_rel_residual", C.c_double), ("pre_iterations", C.c_int32), ("pre_converged", C.c_int32),
                ("aligned_components", C.c_int32), ("rank_deficient_components", C.c_int32), ("min_align_ratio", C.c_double)]


PG_INIT_ALIGN_ROW = 28  # ELM_PG_INIT_ALIGN_ROW: c_a[3], c_b[3], S[9], W, G[9], sigma[3]


class LoopsConfigC(C.Structure):
    """elm_loops_config (include/elimaloc_hip_loops.h)."""
    _fields_ = [("q_t", C.c_double), ("q_r", C.c_double), ("gamma", C.c_double), ("steps_per_batch", C.c_int32), ("reserved", C.c_int32)]


class LoopsResultC(C.Structure):
    """elm_loops_result."""
    _fields_ = [("size", C.c_int32), ("steps", C.c_int32), ("adjacent_pairs", C.c_int64), ("adjacency_ms", C.c_double),
                ("greedy_ms", C.c_double)]


class LoopCovResultC(C.Structure):
    """elm_loopcov_result (include/elimaloc_hip_loopcov.h)."""
    _fields_ = [("size", C.c_int32), ("steps", C.c_int32), ("adjacent_pairs", C.c_int64), ("non_finite_pairs", C.c_int64),
                ("chain_ms", C.c_double), ("adjacency_ms", C.c_double), ("greedy_ms", C.c_double)]


class PoseGraphCovConfigC(C.Structure):
    """elm_posegraph_cov_config (include/elimaloc_hip_posegraph_cov.h)."""
    _fields_ = [("lambda_", C.c_double), ("pcg_rel_tol", C.c_double), ("pcg_max_iterations", C.c_int32), ("pcg_check_every", C.c_int32),
                ("scratch_bytes", C.c_uint64)]


class PoseGraphCovStatsC(C.Structure):
    """elm_posegraph_cov_stats."""
    _fields_ = [("n_columns", C.c_int32), ("n_converged", C.c_int32), ("passes", C.c_int32), ("iterations_max", C.c_int32),
                ("rel_residual_max", C.c_double), ("ms_device", C.c_double), ("scratch_bytes", C.c_uint64)]


class RegInfoConfigC(C.Structure):
    """elm_reginfo_config (include/elimaloc_hip_reginfo.h)."""
    _fields_ = [("metric", C.c_int32), ("_pad", C.c_int32), ("sigma2", C.c_double), ("length_scale_m", C.c_double),
                ("min_eigen_ratio", C.c_double)]


class RegInfoResultC(C.Structure):
    """elm_reginfo_result."""
    _fields_ = [("information", C.c_double * 36), ("H", C.c_double * 36), ("g", C.c_double * 6), ("chi2", C.c_double), ("sigma2", C.c_double),
                ("length_scale", C.c_double), ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36), ("n_points", C.c_int32),
                ("n_pairs", C.c_int32), ("n_default", C.c_int32), ("dof", C.c_int32), ("rank", C.c_int32), ("status", C.c_int32)]


REGINFO_MAX_JOBS = 4096
REGINFO_METRIC_METHOD, REGINFO_METRIC_PLANE = 0, 1
REGINFO_NO_PAIRS, REGINFO_NO_DOF, REGINFO_DEGENERATE, REGINFO_NON_FINITE = 1, 2, 4, 8
LOOPS_MAX, LOOPS_MAX_S = 16384, 2048
POSEGRAPH_MAX_NODES, POSEGRAPH_MAX_EDGES = 1 << 20, 1 << 22
POSEGRAPH_MAX_PRIORS = 1 << 22
PG_STOP = {1: "max_iterations", 2: "cost_tol", 3: "step_tol", 4: "lambda_max", 5: "cost_zero"}

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)

PG_PRECOND = {0: "block_jacobi", 1: "chain"}
PG_INIT_ROT, PG_INIT_TRANS = 1, 2


class PcmNodeConfig(C.Structure):
    """elm_pcm_node_config (include/elimaloc_hip.h)."""
    _fields_ = [("lidar_type", C.c_char * 32), ("lidar_scan_time_end", C.c_int32), ("pcm_voxel_max_point", C.c_int32),
                ("run_deskew", C.c_int32), ("input_index_sampling", C.c_int32), ("lidar_time_delay", C.c_double),
                ("pcm_voxel_size", C.c_double), ("input_max_dist", C.c_double), ("input_voxel_ds_m", C.c_double),
                ("tf_ego_to_lidar", C.c_double * 16)]


class PcmScanOutput(C.Structure):
    """elm_pcm_scan_output (include/elimaloc_hip.h)."""
    _fields_ = [("pose_ego", C.c_double * 16), ("pose_lidar", C.c_double * 16), ("covariance", C.c_double * 36),
                ("fitness_score", C.c_double), ("time_scan_end", C.c_double), ("n_filtered", C.c_uint64), ("n_source", C.c_uint64),
                ("result", RegResult)]


class CloudField(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("offset", C.c_uint32), ("datatype", C.c_int32)]


FIELD_UINT16, FIELD_UINT32, FIELD_FLOAT32 = 4, 6, 7


class EkfConfig(C.Structure):
    """elm_ekf_config (include/elimaloc_hip.h)."""
    _fields_ = [("imu_gravity", C.c_double)] + [(n, C.c_int32) for n in (
        "imu_estimate_gravity", "imu_estimate_calibration", "use_zupt", "use_complementary_filter", "gps_type", "_pad")] + [
        (n, C.c_double) for n in (
            "ekf_init_x_m", "ekf_init_y_m", "ekf_init_z_m", "ekf_init_roll_deg", "ekf_init_pitch_deg", "ekf_init_yaw_deg",
            "state_std_pos_m", "state_std_rot_deg", "state_std_vel_mps", "state_std_gyro_dps", "state_std_acc_mps",
            "imu_std_gyro_dps", "imu_std_acc_mps", "ekf_imu_bias_cov_gyro", "ekf_imu_bias_cov_acc",
            "gnss_min_cov_x_m", "gnss_min_cov_y_m", "gnss_min_cov_z_m", "gnss_min_cov_roll_deg", "gnss_min_cov_pitch_deg",
            "gnss_min_cov_yaw_deg", "can_vel_scale_factor", "ekf_can_meas_uncertainty_vel_mps",
            "ekf_can_meas_uncertainty_yaw_rate_deg")]


class EkfStateC(C.Structure):
    _fields_ = [("x", C.c_double * 27), ("rot_xyzw", C.c_double * 4), ("imu_rot_xyzw", C.c_double * 4),
                ("P", C.c_double * 729), ("timestamp", C.c_double)] + [(n, C.c_int32) for n in (
                    "b_state_initialized", "b_yaw_initialized", "b_rotation_stabilized", "b_state_stabilized",
                    "b_pcm_init_on_going", "_pad")]


class EgoStateC(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "timestamp", "x_m", "y_m", "z_m", "roll_rad", "pitch_rad", "yaw_rad", "roll_vel", "pitch_vel", "yaw_vel",
        "vx", "vy", "vz", "ax", "ay", "az", "x_cov_m", "y_cov_m", "z_cov_m", "roll_cov_rad", "pitch_cov_rad", "yaw_cov_rad")]


def _sig(*argtypes, ret=C.c_int):
    return ret, list(argtypes)


P, i, d, f, szt = C.POINTER, C.c_int, C.c_double, C.c_float, C.c_size_t
vp, cp, dp, fp, ip, szp = C.c_void_p, C.c_char_p, P(d), P(f), P(i), P(szt)
u8p, u16p, u32p, u64p, i32p, i64p = P(C.c_uint8), P(C.c_uint16), P(C.c_uint32), P(C.c_uint64), P(C.c_int32), P(C.c_int64)
pqc = P(PlacesQueryConfigC)

# One table per header: name -> (restype, [argtypes]) of every function it declares.  lib() applies them; the CPU test-suite holds them
# against the headers' prototypes.
DECLS = {  # include/elimaloc_hip.h
    "elm_reg_config_default": _sig(P(RegConfig), ret=None),
    "elm_ctx_create": _sig(i, P(vp)),
    "elm_ctx_create_multi": _sig(ip, i, P(vp)),
    "elm_ctx_group_info": _sig(vp, ip, ip, ip, i),
    "elm_register_shard": _sig(vp, vp, fp, szt, szt, dp, P(RegConfig), P(RegResult), P(IterTrace), i),
    "elm_ctx_destroy": _sig(vp, ret=None),
    "elm_last_error": _sig(vp, ret=cp),
    "elm_strerror": _sig(i, ret=cp),
    "elm_ctx_synchronize": _sig(vp),
    "elm_ctx_stream": _sig(vp, ret=vp),
    "elm_ctx_set_profiling": _sig(vp, i),
    "elm_ctx_set_work_counters": _sig(vp, i),
    "elm_ctx_get_profile": _sig(vp, P(Profile), i),
    "elm_map_build": _sig(vp, fp, szt, d, i, P(vp)),
    "elm_map_destroy": _sig(vp, ret=None),
    "elm_map_cal_voxel_cov_all": _sig(vp),
    "elm_map_cal_point_cov_all": _sig(vp, d),
    "elm_map_build_neighbourhoods": _sig(vp),
    "elm_map_get_info": _sig(vp, P(MapInfo)),
    "elm_map_empty": _sig(vp),
    "elm_map_download_points": _sig(vp, dp, dp, dp, szt),
    "elm_map_download_voxels": _sig(vp, i32p, i32p, dp, dp, szt),
    "elm_map_find_ground_height": _sig(vp, d, d, dp, ip),
    "elm_map_get_correspondences": _sig(vp, vp, i, dp, szt, d, u32p, i32p, szt, szp),
    "elm_align_clouds_local": _sig(vp, i, dp, dp, dp, dp, szt, dp, d, P(RegConfig), dp, dp, dp),
    "elm_scan_upload": _sig(vp, fp, szt, szt, P(vp)),
    "elm_scan_destroy": _sig(vp, ret=None),
    "elm_scan_size": _sig(vp, ret=szt),
    "elm_scan_download": _sig(vp, fp, szt),
    "elm_register": _sig(vp, vp, fp, szt, dp, P(RegConfig), dp, ip, dp, dp, P(RegResult), P(IterTrace)),
    "elm_format_register_log": _sig(P(RegConfig), P(RegResult), szt, P(IterTrace), dp, d, cp, szt, ret=szt),
    "elm_register_batch": _sig(vp, vp, P(vp), i, dp, P(RegConfig), P(RegResult), P(IterTrace)),
    "elm_register_stream": _sig(vp, vp, P(vp), i, dp, P(RegConfig), i, P(RegResult), P(IterTrace)),
    "elm_register_stream_host": _sig(vp, vp, P(vp), u32p, i, dp, P(RegConfig), i, P(RegResult), P(IterTrace)),
    "elm_host_alloc": _sig(szt, ret=vp),
    "elm_host_free": _sig(vp, ret=None),
    "elm_ctx_measure_h2d": _sig(vp, vp, szt, i, dp),
    "elm_register_batch_enqueue": _sig(vp, vp, P(vp), i, dp, P(RegConfig), i),
    "elm_register_batch_finish": _sig(vp, P(RegResult), P(IterTrace)),
    "elm_deskew": _sig(vp, fp, fp, szt, P(DeskewTables), fp, ip),
    "elm_deskew_downsample": _sig(vp, fp, fp, szt, P(DeskewTables), d, P(vp), ip),
    "elm_deskew_prepare": _sig(dp, szt, dp, szt, d, f, f, i, i, dp, dp, dp, dp, szt, P(DeskewTables)),
    "elm_comm_get_unique_id": _sig(vp),
    "elm_comm_init": _sig(vp, i, i, vp),
    "elm_comm_destroy": _sig(vp),
    "elm_comm_info": _sig(vp, ip, ip),
    "elm_comm_set_hook": _sig(vp, ALLREDUCE_FN, vp),
    "elm_filter_points_by_distance": _sig(fp, fp, szt, d, fp, fp, szp),
    "elm_voxel_downsample": _sig(fp, szt, d, i64p, szp),
    "elm_get_interpolated_pose": _sig(dp, szt, d, fp, ip),
    "elm_shape_odom_covariance": _sig(dp, dp, d, dp),
    "elm_cal_frame_point_cov": _sig(dp, szt, d, d, d, dp),
    "elm_ekf_config_default": _sig(P(EkfConfig), ret=None),
    "elm_ekf_create": _sig(P(EkfConfig), P(vp)),
    "elm_ekf_destroy": _sig(vp, ret=None),
    "elm_ekf_predict_imu": _sig(vp, d, dp, dp, ip),
    "elm_ekf_predict": _sig(vp, d, ip),
    "elm_ekf_update_can": _sig(vp, d, dp, dp, ip),
    "elm_gps_project": _sig(d, d, d, d, d, d, dp),
    "elm_ekf_update_navsatfix": _sig(vp, d, d, d, d, dp, d, d, d, i, d, dp, ip),
    "elm_ekf_update_pose": _sig(vp, d, dp, dp, dp, dp, i, ip),
    "elm_ekf_update_pcm_odom": _sig(vp, d, dp, dp, dp, i, ip),
    "elm_ekf_get_state": _sig(vp, P(EkfStateC)),
    "elm_ekf_publish": _sig(vp, P(EgoStateC)),
    "elm_ini_load": _sig(cp, P(vp)),
    "elm_ini_destroy": _sig(vp, ret=None),
    "elm_ini_get_string": _sig(vp, cp, cp, cp, szt),
    "elm_ini_get_int": _sig(vp, cp, cp, ip),
    "elm_ini_get_bool": _sig(vp, cp, cp, ip),
    "elm_ini_get_double": _sig(vp, cp, cp, dp),
    "elm_ini_get_array": _sig(vp, cp, cp, dp, szt, szp),
    "elm_pcm_node_config_default": _sig(P(PcmNodeConfig), ret=None),
    "elm_load_pcm_config": _sig(cp, cp, P(PcmNodeConfig), P(RegConfig)),
    "elm_load_ekf_config": _sig(cp, P(EkfConfig)),
    "elm_pcd_load_xyz": _sig(cp, P(fp), szp),
    "elm_free": _sig(vp, ret=None),
    "elm_scan_from_cloud": _sig(vp, szt, szt, P(CloudField), i, i, i, fp, fp, fp, szt, szp),
    "elm_pcm_callback_point_cloud": _sig(vp, vp, P(PcmNodeConfig), P(RegConfig), fp, fp, szt, d, dp, szt, dp, szt, P(PcmScanOutput), ip),
    "elm_reloc_config_default": _sig(P(RelocConfigC), ret=None),
    "elm_reloc_make_hypotheses": _sig(dp, P(RelocConfigC), dp, szt, szp),
    "elm_map_score_poses": _sig(vp, vp, vp, dp, i, P(RelocConfigC), u32p),
    "elm_relocalize": _sig(vp, vp, fp, szt, dp, P(RelocConfigC), P(RegConfig), dp, P(RegResult), P(RelocCandidate), i, ip),
    "elm_reloc_global_config_default": _sig(P(GlobalRelocConfigC), ret=None),
    "elm_map_ground_heights": _sig(vp, vp, dp, szt, dp, i32p),
    "elm_reloc_global_hypotheses": _sig(vp, vp, dp, P(GlobalRelocConfigC), dp, i32p, szt, szp),
    "elm_relocalize_global": _sig(vp, vp, fp, szt, dp, P(GlobalRelocConfigC), P(RegConfig), dp, P(RegResult), P(RelocCandidate), i, ip,
                                  P(GlobalRelocStats)),
    "elm_freespace_config_default": _sig(P(FreeSpaceConfigC), ret=None),
    "elm_map_fine_cells": _sig(vp, vp, i, i32p, szt, szp),
    "elm_map_check_free_space": _sig(vp, vp, vp, dp, i, P(FreeSpaceConfigC), P(FreeSpaceStatsC), u16p),
    "elm_raycast_config_default": _sig(P(RayCastConfigC), ret=None),
    "elm_map_raycast": _sig(vp, vp, vp, dp, i, P(RayCastConfigC), P(RayCastStatsC), dp, dp, i32p, u8p),
    "elm_evidence_config_default": _sig(P(EvidenceConfigC), ret=None),
    "elm_evidence_rule_default": _sig(P(EvidenceRuleC), ret=None),
    "elm_evidence_create": _sig(vp, vp, i, P(vp)),
    "elm_evidence_destroy": _sig(vp, ret=None),
    "elm_evidence_reset": _sig(vp, vp),
    "elm_evidence_accumulate": _sig(vp, vp, vp, dp, P(EvidenceConfigC), P(EvidenceStatsC), u16p),
    "elm_evidence_accumulate_batch": _sig(vp, vp, P(vp), dp, i, P(EvidenceConfigC), P(EvidenceStatsC)),
    "elm_evidence_counts": _sig(vp, vp, u32p, u32p, szt, szp),
    "elm_evidence_stale_points": _sig(vp, vp, P(EvidenceRuleC), u8p, szt, szp),
    "elm_growth_config_default": _sig(P(GrowthConfigC), ret=None),
    "elm_growth_rule_default": _sig(P(GrowthRuleC), ret=None),
    "elm_growth_create": _sig(vp, vp, i, szt, P(vp)),
    "elm_growth_destroy": _sig(vp, ret=None),
    "elm_growth_reset": _sig(vp, vp),
    "elm_growth_accumulate": _sig(vp, vp, vp, dp, P(GrowthConfigC), P(GrowthStatsC), u16p),
    "elm_growth_accumulate_batch": _sig(vp, vp, P(vp), dp, i, P(GrowthConfigC), P(GrowthStatsC)),
    "elm_growth_cells": _sig(vp, vp, i32p, u32p, u32p, u64p, szt, szp),
    "elm_growth_appeared_points": _sig(vp, vp, P(GrowthRuleC), dp, szt, szp),
    "elm_growth_object_rule_default": _sig(P(GrowthObjectRuleC), ret=None),
    "elm_growth_find_objects": _sig(vp, vp, P(GrowthObjectRuleC), P(GrowthObjectStatsC)),
    "elm_growth_objects": _sig(vp, vp, P(GrowthObjectC), szt, szp),
    "elm_growth_cell_objects": _sig(vp, vp, i32p, szt, szp),
    "elm_growth_beam_objects": _sig(vp, vp, vp, dp, P(GrowthConfigC), i32p),
    "elm_map_build_device": _sig(vp, vp, u8p, fp, szt, d, i, P(vp)),
    "elm_map_build_device_stages": _sig(vp, dp),
    "elm_map_build_device_from": _sig(vp, P(BuildSourcesC), d, i, P(vp), P(BuildSourcesStatsC)),
    "elm_odometry_config_default": _sig(P(OdometryConfigC), ret=None),
    "elm_odometry_create": _sig(vp, P(OdometryConfigC), P(vp)),
    "elm_odometry_destroy": _sig(vp, ret=None),
    "elm_odometry_reset": _sig(vp),
    "elm_odometry_predict": _sig(vp, dp),
    "elm_odometry_step_scan": _sig(vp, vp, dp, P(OdometryStepC)),
    "elm_odometry_map": _sig(vp, ret=vp),
    "elm_places_config_default": _sig(P(PlacesConfigC), ret=None),
    "elm_places_tables": _sig(P(PlacesConfigC), dp, dp, dp),
    "elm_places_create": _sig(vp, P(PlacesConfigC), i, P(vp)),
    "elm_places_destroy": _sig(vp, ret=None),
    "elm_places_reset": _sig(vp, vp),
    "elm_places_size": _sig(vp, vp, szp),
    "elm_places_describe": _sig(vp, vp, P(vp), dp, i, u64p, P(PlacesStatsC)),
    "elm_places_add": _sig(vp, vp, P(vp), dp, i64p, i, P(PlacesStatsC)),
    "elm_places_add_words": _sig(vp, vp, u64p, i64p, szt),
    "elm_places_download": _sig(vp, vp, szt, szt, u64p, i64p, u32p),
    "elm_places_match_words": _sig(vp, vp, u64p, i, pqc, P(PlaceCandidateC), i32p, P(PlaceMatchC)),
    "elm_places_query": _sig(vp, vp, P(vp), dp, i, pqc, P(PlaceCandidateC), i32p, P(PlaceMatchC), P(PlacesStatsC)),
    "elm_map_set_index_build": _sig(vp, i),
    "elm_map_index_build_stages": _sig(vp, dp),
    "elm_map_download_cell_grid": _sig(vp, P(CellGridDesc), u32p, szt, fp, szt, u32p, szt, u32p, szt),
    "elm_posegraph_config_default": _sig(P(PoseGraphConfigC), ret=None),
    "elm_posegraph_create": _sig(vp, i, i, P(vp)),
    "elm_posegraph_destroy": _sig(vp, ret=None),
    "elm_posegraph_reset": _sig(vp, vp),
    "elm_posegraph_size": _sig(vp, vp, szp, szp),
    "elm_posegraph_add_nodes": _sig(vp, vp, dp, u8p, szt),
    "elm_posegraph_set_poses": _sig(vp, vp, szt, szt, dp),
    "elm_posegraph_get_poses": _sig(vp, vp, szt, szt, dp),
    "elm_posegraph_set_fixed": _sig(vp, vp, szt, szt, u8p),
    "elm_posegraph_add_edges": _sig(vp, vp, i32p, i32p, dp, dp, szt),
    "elm_posegraph_linearize": _sig(vp, vp, d, P(PoseGraphLinearizeStatsC)),
    "elm_posegraph_download_linearization": _sig(vp, vp, dp, dp, dp, dp, dp, dp, dp),
    "elm_posegraph_solve": _sig(vp, vp, d, d, i, dp, P(PoseGraphSolveStatsC)),
    "elm_posegraph_optimize": _sig(vp, vp, P(PoseGraphConfigC), P(PoseGraphResultC), P(PoseGraphTraceC), i),
    "elm_posegraph_edge_terms": _sig(dp, dp, dp, dp, dp, dp),
}
DECLS_PRECOND = {  # include/elimaloc_hip_posegraph_precond.h (the pose graph's preconditioner)
    "elm_posegraph_set_preconditioner": _sig(vp, vp, i),
    "elm_posegraph_get_preconditioner": _sig(vp, vp, ip),
}
DECLS_INIT = {  # include/elimaloc_hip_posegraph_init.h (the pose graph's linear initialization)
    "elm_posegraph_init_config_default": _sig(P(PoseGraphInitConfigC), ret=None),
    "elm_posegraph_initialize": _sig(vp, vp, P(PoseGraphInitConfigC), P(PoseGraphInitResultC), dp, dp),
}
DECLS_LOOPS = {  # include/elimaloc_hip_loops.h (loop closing: pairwise consistency of loop measurements)
    "elm_loops_config_default": _sig(P(LoopsConfigC), ret=None),
    "elm_loops_pair_terms": _sig(dp, dp, dp, dp, dp, dp, dp),
    "elm_loops_consistency": _sig(vp, dp, szt, i32p, i32p, dp, dp, dp, szt, P(LoopsConfigC), P(LoopsResultC), u8p, i32p, u64p, dp),
}
DECLS_LOOPCOV = {  # include/elimaloc_hip_loopcov.h (loop closing: pairwise consistency with a propagated 6 x 6 covariance)
    "elm_loopcov_chain": _sig(vp, dp, szt, dp, szt, dp, dp),
    "elm_loopcov_pair_terms": _sig(dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp),
    "elm_loopcov_consistency": _sig(vp, dp, szt, i32p, i32p, dp, dp, szt, dp, szt, P(LoopsConfigC), P(LoopCovResultC), u8p, i32p, u64p, dp),
}
DECLS_PGCOV = {  # include/elimaloc_hip_posegraph_cov.h (the pose graph's marginal and relative covariances)
    "elm_posegraph_cov_config_default": _sig(P(PoseGraphCovConfigC), ret=None),
    "elm_posegraph_covariance": _sig(vp, vp, i32p, szt, i32p, szt, P(PoseGraphCovConfigC), dp, dp, i32p, u8p, P(PoseGraphCovStatsC)),
    "elm_posegraph_relative_covariance": _sig(vp, vp, i32p, i32p, szt, P(PoseGraphCovConfigC), dp, P(PoseGraphCovStatsC)),
}
DECLS_PGPRIOR = {  # include/elimaloc_hip_posegraph_prior.h (the pose graph's absolute pose and position factors)
    "elm_posegraph_reserve_priors": _sig(vp, vp, i),
    "elm_posegraph_add_priors": _sig(vp, vp, i32p, dp, dp, dp, szt),
    "elm_posegraph_prior_count": _sig(vp, vp, szp),
    "elm_posegraph_get_priors": _sig(vp, vp, szt, szt, i32p, dp, dp, dp),
    "elm_posegraph_clear_priors": _sig(vp, vp),
    "elm_posegraph_set_prior_huber": _sig(vp, vp, d),
    "elm_posegraph_get_prior_huber": _sig(vp, vp, dp),
    "elm_posegraph_download_prior_linearization": _sig(vp, vp, dp, dp, dp, dp),
    "elm_posegraph_prior_terms": _sig(dp, dp, dp, dp, dp),
}
DECLS_PGINITP = {  # include/elimaloc_hip_posegraph_init_prior.h (the pose graph's linear initialization with the priors in it)
    "elm_posegraph_init_prior_config_default": _sig(P(PoseGraphInitPriorConfigC), ret=None),
    "elm_posegraph_initialize_priors": _sig(vp, vp, P(PoseGraphInitPriorConfigC), P(PoseGraphInitPriorResultC), dp, dp, dp, dp, i),
}
DECLS_REGINFO = {  # include/elimaloc_hip_reginfo.h (registration information: 6 x 6 pose information and degeneracy)
    "elm_reginfo_config_default": _sig(P(RegInfoConfigC), ret=None),
    "elm_register_information": _sig(vp, vp, P(vp), dp, i, P(RegConfig), P(RegInfoConfigC), P(RegInfoResultC)),
    "elm_reginfo_pair_terms": _sig(dp, dp, dp, dp, dp, d, i, i, dp, dp, dp, dp),
}
# the names alone, as __graft_entry__ and the ABI tests read them
EXPORTS, EXPORTS_PRECOND, EXPORTS_INIT, EXPORTS_LOOPS = list(DECLS), list(DECLS_PRECOND), list(DECLS_INIT), list(DECLS_LOOPS)
EXPORTS_LOOPCOV = list(DECLS_LOOPCOV)
EXPORTS_PGCOV = list(DECLS_PGCOV)
EXPORTS_PGPRIOR = list(DECLS_PGPRIOR)
EXPORTS_PGINITP = list(DECLS_PGINITP)
EXPORTS_REGINFO = list(DECLS_REGINFO)

_LIB = None


def lib():
    """Load libelimaloc_hip.so (fails loudly when it has not been built) and give every declared function its signature."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ElmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for table in (DECLS, DECLS_PRECOND, DECLS_INIT, DECLS_LOOPS, DECLS_LOOPCOV, DECLS_PGCOV, DECLS_PGPRIOR, DECLS_PGINITP, DECLS_REGINFO):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


def check(status, ctx=None, what=""):
    if status != ELM_OK:
        L = lib()
        msg = L.elm_strerror(status).decode()
        if ctx is not None:
            detail = L.elm_last_error(ctx)
            if detail:
                msg += ": " + detail.decode()
        raise ElmError(f"{what} failed ({status}): {msg}")
