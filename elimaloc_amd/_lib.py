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


POSEGRAPH_MAX_NODES, POSEGRAPH_MAX_EDGES = 1 << 20, 1 << 22
PG_STOP = {1: "max_iterations", 2: "cost_tol", 3: "step_tol", 4: "lambda_max", 5: "cost_zero"}

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)

# every symbol include/elimaloc_hip.h declares (checked by the CPU test-suite)
EXPORTS = [
    "elm_reg_config_default", "elm_ctx_create", "elm_ctx_create_multi", "elm_ctx_group_info", "elm_register_shard", "elm_ctx_destroy", "elm_last_error", "elm_strerror",
    "elm_ctx_synchronize", "elm_ctx_stream", "elm_ctx_set_profiling", "elm_ctx_set_work_counters", "elm_ctx_get_profile", "elm_map_build", "elm_map_destroy", "elm_map_cal_voxel_cov_all",
    "elm_map_cal_point_cov_all", "elm_map_build_neighbourhoods", "elm_map_get_info", "elm_map_empty", "elm_map_download_points",
    "elm_map_download_voxels", "elm_map_find_ground_height", "elm_map_get_correspondences", "elm_align_clouds_local", "elm_scan_upload", "elm_scan_destroy",
    "elm_scan_size", "elm_scan_download", "elm_register", "elm_format_register_log", "elm_register_batch", "elm_register_stream", "elm_register_stream_host", "elm_host_alloc", "elm_host_free", "elm_ctx_measure_h2d", "elm_register_batch_enqueue",
    "elm_register_batch_finish", "elm_deskew", "elm_deskew_downsample", "elm_deskew_prepare", "elm_comm_get_unique_id", "elm_comm_init",
    "elm_comm_destroy", "elm_comm_info", "elm_comm_set_hook", "elm_filter_points_by_distance", "elm_voxel_downsample",
    "elm_get_interpolated_pose", "elm_shape_odom_covariance", "elm_cal_frame_point_cov",
    "elm_ekf_config_default", "elm_ekf_create", "elm_ekf_destroy", "elm_ekf_predict_imu", "elm_ekf_predict", "elm_ekf_update_can", "elm_gps_project", "elm_ekf_update_navsatfix",
    "elm_ekf_update_pose", "elm_ekf_update_pcm_odom", "elm_ekf_get_state", "elm_ekf_publish",
    "elm_ini_load", "elm_ini_destroy", "elm_ini_get_string", "elm_ini_get_int", "elm_ini_get_bool", "elm_ini_get_double",
    "elm_ini_get_array", "elm_pcm_node_config_default", "elm_load_pcm_config", "elm_load_ekf_config", "elm_pcd_load_xyz",
    "elm_free", "elm_scan_from_cloud", "elm_pcm_callback_point_cloud",
    "elm_reloc_config_default", "elm_reloc_make_hypotheses", "elm_map_score_poses", "elm_relocalize",
    "elm_reloc_global_config_default", "elm_map_ground_heights", "elm_reloc_global_hypotheses", "elm_relocalize_global",
    "elm_freespace_config_default", "elm_map_fine_cells", "elm_map_check_free_space",
    "elm_raycast_config_default", "elm_map_raycast",
    "elm_evidence_config_default", "elm_evidence_rule_default", "elm_evidence_create", "elm_evidence_destroy", "elm_evidence_reset",
    "elm_evidence_accumulate", "elm_evidence_accumulate_batch", "elm_evidence_counts", "elm_evidence_stale_points",
    "elm_growth_config_default", "elm_growth_rule_default", "elm_growth_create", "elm_growth_destroy", "elm_growth_reset",
    "elm_growth_accumulate", "elm_growth_accumulate_batch", "elm_growth_cells", "elm_growth_appeared_points",
    "elm_growth_object_rule_default", "elm_growth_find_objects", "elm_growth_objects", "elm_growth_cell_objects", "elm_growth_beam_objects",
    "elm_map_build_device", "elm_map_build_device_stages", "elm_map_build_device_from",
    "elm_odometry_config_default", "elm_odometry_create", "elm_odometry_destroy", "elm_odometry_reset", "elm_odometry_predict",
    "elm_odometry_step_scan", "elm_odometry_map",
    "elm_places_config_default", "elm_places_tables", "elm_places_create", "elm_places_destroy", "elm_places_reset", "elm_places_size",
    "elm_places_describe", "elm_places_add", "elm_places_add_words", "elm_places_download", "elm_places_match_words", "elm_places_query",
    "elm_map_set_index_build", "elm_map_index_build_stages", "elm_map_download_cell_grid",
    "elm_posegraph_config_default", "elm_posegraph_create", "elm_posegraph_destroy", "elm_posegraph_reset", "elm_posegraph_size",
    "elm_posegraph_add_nodes", "elm_posegraph_set_poses", "elm_posegraph_get_poses", "elm_posegraph_set_fixed", "elm_posegraph_add_edges",
    "elm_posegraph_linearize", "elm_posegraph_download_linearization", "elm_posegraph_solve", "elm_posegraph_optimize",
    "elm_posegraph_edge_terms",
]
# every symbol include/elimaloc_hip_posegraph_precond.h declares (the header elimaloc_hip.h includes for the pose graph's preconditioner)
EXPORTS_PRECOND = ["elm_posegraph_set_preconditioner", "elm_posegraph_get_preconditioner"]
PG_PRECOND = {0: "block_jacobi", 1: "chain"}
# every symbol include/elimaloc_hip_posegraph_init.h declares (the header elimaloc_hip.h includes for the pose graph's linear initialization)
EXPORTS_INIT = ["elm_posegraph_init_config_default", "elm_posegraph_initialize"]
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


_LIB = None


def lib():
    """Load libelimaloc_hip.so (fails loudly when it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ElmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, dp, fp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.elm_reg_config_default.argtypes = [C.POINTER(RegConfig)]
    L.elm_reg_config_default.restype = None
    L.elm_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.elm_ctx_destroy.argtypes = [vp]
    L.elm_ctx_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.elm_ctx_group_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.elm_register_shard.argtypes = [vp, vp, fp, C.c_size_t, C.c_size_t, dp, C.POINTER(RegConfig), C.POINTER(RegResult), C.POINTER(IterTrace), C.c_int]
    L.elm_ctx_destroy.restype = None
    L.elm_last_error.argtypes = [vp]
    L.elm_last_error.restype = C.c_char_p
    L.elm_strerror.argtypes = [C.c_int]
    L.elm_strerror.restype = C.c_char_p
    L.elm_ctx_synchronize.argtypes = [vp]
    L.elm_ctx_stream.argtypes = [vp]
    L.elm_ctx_stream.restype = vp
    L.elm_format_register_log.argtypes = [C.POINTER(RegConfig), C.POINTER(RegResult), C.c_size_t, C.POINTER(IterTrace), C.POINTER(C.c_double),
                                          C.c_double, C.c_char_p, C.c_size_t]
    L.elm_format_register_log.restype = C.c_size_t
    L.elm_ctx_set_profiling.argtypes = [vp, C.c_int]
    L.elm_ctx_set_work_counters.argtypes = [vp, C.c_int]
    L.elm_ctx_get_profile.argtypes = [vp, C.POINTER(Profile), C.c_int]
    L.elm_map_build.argtypes = [vp, fp, C.c_size_t, C.c_double, C.c_int, C.POINTER(vp)]
    L.elm_map_build_device.argtypes = [vp, vp, C.POINTER(C.c_uint8), fp, C.c_size_t, C.c_double, C.c_int, C.POINTER(vp)]
    L.elm_map_build_device_stages.argtypes = [vp, dp]
    L.elm_map_build_device_from.argtypes = [vp, C.POINTER(BuildSourcesC), C.c_double, C.c_int, C.POINTER(vp), C.POINTER(BuildSourcesStatsC)]
    L.elm_odometry_config_default.argtypes = [C.POINTER(OdometryConfigC)]
    L.elm_odometry_config_default.restype = None
    L.elm_odometry_create.argtypes = [vp, C.POINTER(OdometryConfigC), C.POINTER(vp)]
    L.elm_odometry_destroy.argtypes = [vp]
    L.elm_odometry_destroy.restype = None
    L.elm_odometry_reset.argtypes = [vp]
    L.elm_odometry_predict.argtypes = [vp, dp]
    L.elm_odometry_step_scan.argtypes = [vp, vp, dp, C.POINTER(OdometryStepC)]
    L.elm_odometry_map.argtypes = [vp]
    L.elm_odometry_map.restype = vp
    u32p = C.POINTER(C.c_uint32)
    L.elm_map_set_index_build.argtypes = [vp, C.c_int]
    L.elm_map_index_build_stages.argtypes = [vp, dp]
    L.elm_map_download_cell_grid.argtypes = [vp, C.POINTER(CellGridDesc), u32p, C.c_size_t, fp, C.c_size_t, u32p, C.c_size_t, u32p, C.c_size_t]
    L.elm_map_destroy.argtypes = [vp]
    L.elm_map_destroy.restype = None
    L.elm_map_cal_voxel_cov_all.argtypes = [vp]
    L.elm_map_cal_point_cov_all.argtypes = [vp, C.c_double]
    L.elm_map_build_neighbourhoods.argtypes = [vp]
    L.elm_map_get_info.argtypes = [vp, C.POINTER(MapInfo)]
    L.elm_map_empty.argtypes = [vp]
    L.elm_map_download_points.argtypes = [vp, dp, dp, dp, C.c_size_t]
    L.elm_map_download_voxels.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp, C.c_size_t]
    L.elm_map_find_ground_height.argtypes = [vp, C.c_double, C.c_double, dp, ip]
    L.elm_cal_frame_point_cov.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, C.c_double, dp]
    L.elm_align_clouds_local.argtypes = [vp, C.c_int, dp, dp, dp, dp, C.c_size_t, dp, C.c_double, C.POINTER(RegConfig), dp, dp, dp]
    L.elm_map_get_correspondences.argtypes = [vp, vp, C.c_int, dp, C.c_size_t, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_scan_upload.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.elm_scan_destroy.argtypes = [vp]
    L.elm_scan_destroy.restype = None
    L.elm_scan_size.argtypes = [vp]
    L.elm_scan_size.restype = C.c_size_t
    L.elm_scan_download.argtypes = [vp, fp, C.c_size_t]
    L.elm_deskew_downsample.argtypes = [vp, fp, fp, C.c_size_t, C.POINTER(DeskewTables), C.c_double, C.POINTER(vp), ip]
    L.elm_register.argtypes = [vp, vp, fp, C.c_size_t, dp, C.POINTER(RegConfig), dp, ip, dp, dp,
                               C.POINTER(RegResult), C.POINTER(IterTrace)]
    L.elm_register_stream.argtypes = [vp, vp, C.POINTER(vp), C.c_int, dp, C.POINTER(RegConfig), C.c_int, C.POINTER(RegResult),
                                      C.POINTER(IterTrace)]
    L.elm_register_stream_host.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.c_int, dp, C.POINTER(RegConfig), C.c_int,
                                           C.POINTER(RegResult), C.POINTER(IterTrace)]
    L.elm_ctx_measure_h2d.argtypes = [vp, vp, C.c_size_t, C.c_int, dp]
    L.elm_host_alloc.argtypes = [C.c_size_t]
    L.elm_host_alloc.restype = vp
    L.elm_host_free.argtypes = [vp]
    L.elm_host_free.restype = None
    L.elm_register_batch.argtypes = [vp, vp, C.POINTER(vp), C.c_int, dp, C.POINTER(RegConfig),
                                     C.POINTER(RegResult), C.POINTER(IterTrace)]
    L.elm_register_batch_enqueue.argtypes = [vp, vp, C.POINTER(vp), C.c_int, dp, C.POINTER(RegConfig), C.c_int]
    L.elm_register_batch_finish.argtypes = [vp, C.POINTER(RegResult), C.POINTER(IterTrace)]
    L.elm_deskew.argtypes = [vp, fp, fp, C.c_size_t, C.POINTER(DeskewTables), fp, ip]
    L.elm_deskew_prepare.argtypes = [dp, C.c_size_t, dp, C.c_size_t, C.c_double, C.c_float, C.c_float, C.c_int,
                                     C.c_int, dp, dp, dp, dp, C.c_size_t, C.POINTER(DeskewTables)]
    L.elm_filter_points_by_distance.argtypes = [fp, fp, C.c_size_t, C.c_double, fp, fp, C.POINTER(C.c_size_t)]
    L.elm_voxel_downsample.argtypes = [fp, C.c_size_t, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]
    L.elm_get_interpolated_pose.argtypes = [dp, C.c_size_t, C.c_double, fp, ip]
    L.elm_shape_odom_covariance.argtypes = [dp, dp, C.c_double, dp]
    L.elm_ekf_config_default.argtypes = [C.POINTER(EkfConfig)]
    L.elm_ekf_config_default.restype = None
    L.elm_ekf_create.argtypes = [C.POINTER(EkfConfig), C.POINTER(vp)]
    L.elm_ekf_destroy.argtypes = [vp]
    L.elm_ekf_destroy.restype = None
    L.elm_ekf_predict_imu.argtypes = [vp, C.c_double, dp, dp, ip]
    L.elm_ekf_predict.argtypes = [vp, C.c_double, ip]
    L.elm_ekf_update_can.argtypes = [vp, C.c_double, dp, dp, ip]
    L.elm_gps_project.argtypes = [C.c_double] * 6 + [dp]
    L.elm_ekf_update_navsatfix.argtypes = [vp] + [C.c_double] * 4 + [dp] + [C.c_double] * 3 + [C.c_int, C.c_double, dp, ip]
    L.elm_ekf_update_pose.argtypes = [vp, C.c_double, dp, dp, dp, dp, C.c_int, ip]
    L.elm_ekf_update_pcm_odom.argtypes = [vp, C.c_double, dp, dp, dp, C.c_int, ip]
    L.elm_ekf_get_state.argtypes = [vp, C.POINTER(EkfStateC)]
    L.elm_ekf_publish.argtypes = [vp, C.POINTER(EgoStateC)]
    cp, szp = C.c_char_p, C.POINTER(C.c_size_t)
    L.elm_ini_load.argtypes = [cp, C.POINTER(vp)]
    L.elm_ini_destroy.argtypes = [vp]
    L.elm_ini_destroy.restype = None
    L.elm_ini_get_string.argtypes = [vp, cp, cp, C.c_char_p, C.c_size_t]
    L.elm_ini_get_int.argtypes = [vp, cp, cp, ip]
    L.elm_ini_get_bool.argtypes = [vp, cp, cp, ip]
    L.elm_ini_get_double.argtypes = [vp, cp, cp, dp]
    L.elm_ini_get_array.argtypes = [vp, cp, cp, dp, C.c_size_t, szp]
    L.elm_pcm_node_config_default.argtypes = [C.POINTER(PcmNodeConfig)]
    L.elm_pcm_node_config_default.restype = None
    L.elm_load_pcm_config.argtypes = [cp, cp, C.POINTER(PcmNodeConfig), C.POINTER(RegConfig)]
    L.elm_load_ekf_config.argtypes = [cp, C.POINTER(EkfConfig)]
    L.elm_pcd_load_xyz.argtypes = [cp, C.POINTER(fp), szp]
    L.elm_free.argtypes = [vp]
    L.elm_free.restype = None
    L.elm_scan_from_cloud.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(CloudField), C.c_int, C.c_int, C.c_int, fp, fp, fp,
                                      C.c_size_t, szp]
    L.elm_pcm_callback_point_cloud.argtypes = [vp, vp, C.POINTER(PcmNodeConfig), C.POINTER(RegConfig), fp, fp, C.c_size_t, C.c_double,
                                               dp, C.c_size_t, dp, C.c_size_t, C.POINTER(PcmScanOutput), ip]
    L.elm_reloc_config_default.argtypes = [C.POINTER(RelocConfigC)]
    L.elm_reloc_config_default.restype = None
    L.elm_reloc_make_hypotheses.argtypes = [dp, C.POINTER(RelocConfigC), dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_map_score_poses.argtypes = [vp, vp, vp, dp, C.c_int, C.POINTER(RelocConfigC), C.POINTER(C.c_uint32)]
    L.elm_relocalize.argtypes = [vp, vp, fp, C.c_size_t, dp, C.POINTER(RelocConfigC), C.POINTER(RegConfig), dp, C.POINTER(RegResult),
                                 C.POINTER(RelocCandidate), C.c_int, ip]
    L.elm_freespace_config_default.argtypes = [C.POINTER(FreeSpaceConfigC)]
    L.elm_freespace_config_default.restype = None
    L.elm_map_fine_cells.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_map_check_free_space.argtypes = [vp, vp, vp, dp, C.c_int, C.POINTER(FreeSpaceConfigC), C.POINTER(FreeSpaceStatsC),
                                           C.POINTER(C.c_uint16)]
    L.elm_raycast_config_default.argtypes = [C.POINTER(RayCastConfigC)]
    L.elm_raycast_config_default.restype = None
    L.elm_map_raycast.argtypes = [vp, vp, vp, dp, C.c_int, C.POINTER(RayCastConfigC), C.POINTER(RayCastStatsC), dp, dp,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]
    L.elm_evidence_config_default.argtypes = [C.POINTER(EvidenceConfigC)]
    L.elm_evidence_config_default.restype = None
    L.elm_evidence_rule_default.argtypes = [C.POINTER(EvidenceRuleC)]
    L.elm_evidence_rule_default.restype = None
    L.elm_evidence_create.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.elm_evidence_destroy.argtypes = [vp]
    L.elm_evidence_destroy.restype = None
    L.elm_evidence_reset.argtypes = [vp, vp]
    L.elm_evidence_accumulate.argtypes = [vp, vp, vp, dp, C.POINTER(EvidenceConfigC), C.POINTER(EvidenceStatsC), C.POINTER(C.c_uint16)]
    L.elm_evidence_accumulate_batch.argtypes = [vp, vp, C.POINTER(vp), dp, C.c_int, C.POINTER(EvidenceConfigC), C.POINTER(EvidenceStatsC)]
    L.elm_evidence_counts.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_evidence_stale_points.argtypes = [vp, vp, C.POINTER(EvidenceRuleC), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_growth_config_default.argtypes = [C.POINTER(GrowthConfigC)]
    L.elm_growth_config_default.restype = None
    L.elm_growth_rule_default.argtypes = [C.POINTER(GrowthRuleC)]
    L.elm_growth_rule_default.restype = None
    L.elm_growth_create.argtypes = [vp, vp, C.c_int, C.c_size_t, C.POINTER(vp)]
    L.elm_growth_destroy.argtypes = [vp]
    L.elm_growth_destroy.restype = None
    L.elm_growth_reset.argtypes = [vp, vp]
    L.elm_growth_accumulate.argtypes = [vp, vp, vp, dp, C.POINTER(GrowthConfigC), C.POINTER(GrowthStatsC), C.POINTER(C.c_uint16)]
    L.elm_growth_accumulate_batch.argtypes = [vp, vp, C.POINTER(vp), dp, C.c_int, C.POINTER(GrowthConfigC), C.POINTER(GrowthStatsC)]
    L.elm_growth_cells.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    L.elm_growth_appeared_points.argtypes = [vp, vp, C.POINTER(GrowthRuleC), dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_growth_object_rule_default.argtypes = [C.POINTER(GrowthObjectRuleC)]
    L.elm_growth_object_rule_default.restype = None
    L.elm_growth_find_objects.argtypes = [vp, vp, C.POINTER(GrowthObjectRuleC), C.POINTER(GrowthObjectStatsC)]
    L.elm_growth_objects.argtypes = [vp, vp, C.POINTER(GrowthObjectC), C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_growth_cell_objects.argtypes = [vp, vp, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.elm_growth_beam_objects.argtypes = [vp, vp, vp, dp, C.POINTER(GrowthConfigC), C.POINTER(C.c_int32)]
    L.elm_reloc_global_config_default.argtypes = [C.POINTER(GlobalRelocConfigC)]
    L.elm_reloc_global_config_default.restype = None
    L.elm_map_ground_heights.argtypes = [vp, vp, dp, C.c_size_t, dp, C.POINTER(C.c_int32)]
    L.elm_reloc_global_hypotheses.argtypes = [vp, vp, dp, C.POINTER(GlobalRelocConfigC), dp, C.POINTER(C.c_int32), C.c_size_t,
                                              C.POINTER(C.c_size_t)]
    L.elm_relocalize_global.argtypes = [vp, vp, fp, C.c_size_t, dp, C.POINTER(GlobalRelocConfigC), C.POINTER(RegConfig), dp,
                                        C.POINTER(RegResult), C.POINTER(RelocCandidate), C.c_int, ip, C.POINTER(GlobalRelocStats)]
    u64p, i64p, pqc = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(PlacesQueryConfigC)
    L.elm_places_config_default.argtypes = [C.POINTER(PlacesConfigC)]
    L.elm_places_config_default.restype = None
    L.elm_places_tables.argtypes = [C.POINTER(PlacesConfigC), dp, dp, dp]
    L.elm_places_create.argtypes = [vp, C.POINTER(PlacesConfigC), C.c_int, C.POINTER(vp)]
    L.elm_places_destroy.argtypes = [vp]
    L.elm_places_destroy.restype = None
    L.elm_places_reset.argtypes = [vp, vp]
    L.elm_places_size.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    L.elm_places_describe.argtypes = [vp, vp, C.POINTER(vp), dp, C.c_int, u64p, C.POINTER(PlacesStatsC)]
    L.elm_places_add.argtypes = [vp, vp, C.POINTER(vp), dp, i64p, C.c_int, C.POINTER(PlacesStatsC)]
    L.elm_places_add_words.argtypes = [vp, vp, u64p, i64p, C.c_size_t]
    L.elm_places_download.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p, i64p, C.POINTER(C.c_uint32)]
    L.elm_places_match_words.argtypes = [vp, vp, u64p, C.c_int, pqc, C.POINTER(PlaceCandidateC), C.POINTER(C.c_int32), C.POINTER(PlaceMatchC)]
    L.elm_places_query.argtypes = [vp, vp, C.POINTER(vp), dp, C.c_int, pqc, C.POINTER(PlaceCandidateC), C.POINTER(C.c_int32),
                                   C.POINTER(PlaceMatchC), C.POINTER(PlacesStatsC)]
    u8p, i32p, szt = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_size_t
    L.elm_posegraph_config_default.argtypes = [C.POINTER(PoseGraphConfigC)]
    L.elm_posegraph_config_default.restype = None
    L.elm_posegraph_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.elm_posegraph_destroy.argtypes = [vp]
    L.elm_posegraph_destroy.restype = None
    L.elm_posegraph_reset.argtypes = [vp, vp]
    L.elm_posegraph_size.argtypes = [vp, vp, C.POINTER(szt), C.POINTER(szt)]
    L.elm_posegraph_add_nodes.argtypes = [vp, vp, dp, u8p, szt]
    L.elm_posegraph_set_poses.argtypes = [vp, vp, szt, szt, dp]
    L.elm_posegraph_get_poses.argtypes = [vp, vp, szt, szt, dp]
    L.elm_posegraph_set_fixed.argtypes = [vp, vp, szt, szt, u8p]
    L.elm_posegraph_add_edges.argtypes = [vp, vp, i32p, i32p, dp, dp, szt]
    L.elm_posegraph_linearize.argtypes = [vp, vp, C.c_double, C.POINTER(PoseGraphLinearizeStatsC)]
    L.elm_posegraph_download_linearization.argtypes = [vp, vp, dp, dp, dp, dp, dp, dp, dp]
    L.elm_posegraph_solve.argtypes = [vp, vp, C.c_double, C.c_double, C.c_int, dp, C.POINTER(PoseGraphSolveStatsC)]
    L.elm_posegraph_optimize.argtypes = [vp, vp, C.POINTER(PoseGraphConfigC), C.POINTER(PoseGraphResultC), C.POINTER(PoseGraphTraceC), C.c_int]
    L.elm_posegraph_edge_terms.argtypes = [dp, dp, dp, dp, dp, dp]
    L.elm_posegraph_set_preconditioner.argtypes = [vp, vp, C.c_int]
    L.elm_posegraph_get_preconditioner.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.elm_posegraph_init_config_default.argtypes = [C.POINTER(PoseGraphInitConfigC)]
    L.elm_posegraph_init_config_default.restype = None
    L.elm_posegraph_initialize.argtypes = [vp, vp, C.POINTER(PoseGraphInitConfigC), C.POINTER(PoseGraphInitResultC), dp, dp]
    L.elm_comm_get_unique_id.argtypes = [vp]
    L.elm_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.elm_comm_destroy.argtypes = [vp]
    L.elm_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.elm_comm_set_hook.argtypes = [vp, ALLREDUCE_FN, vp]
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
