"""ctypes binding of libpcm_amd.so (the C ABI declared in include/pcm_amd.h)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/pcm_amd.h declares (tests check the .so exports each one)
SYMBOLS = [
    "pcm_abi_version", "pcm_default_config", "pcm_create", "pcm_destroy", "pcm_last_error",
    "pcm_get_config", "pcm_set_config", "pcm_set_stream", "pcm_set_target", "pcm_set_source",
    "pcm_swap_source_and_target", "pcm_clear_source", "pcm_clear_target", "pcm_align",
    "pcm_linearize", "pcm_compute_error", "pcm_get_planes", "pcm_get_neighbour_lists", "pcm_get_lio_members", "pcm_obs_model", "pcm_target_insert", "pcm_map_incremental", "pcm_get_target", "pcm_get_covariances", "pcm_set_covariances", "pcm_ndt_derivatives", "pcm_ndt_score", "pcm_fitness_score", "pcm_undistort", "pcm_voxel_downsample", "pcm_voxel_downsample_large", "pcm_approx_voxel_downsample", "pcm_livox_filter", "pcm_gicp_bfgs_set_correspondences", "pcm_gicp_bfgs_fdf", "pcm_gicp_bfgs_update_correspondences", "pcm_gicp_bfgs_get_correspondences", "pcm_align_batch", "pcm_set_profiling", "pcm_debug_phase_cycles",
    "pcm_get_stats", "pcm_reset_stats", "pcm_lio_frame_begin", "pcm_lio_frame_end", "pcm_get_source",
    "pcm_loam_default_params", "pcm_loam_set_target", "pcm_loam_set_source", "pcm_loam_align", "pcm_loam_align_batch",
    "pcm_loam_coefficients", "pcm_loam_neighbours",
    "pcm_loam_default_feature_params", "pcm_loam_extract_features", "pcm_loam_frame_begin", "pcm_loam_frame_begin_batch",
    "pcm_loam_feature_info",
    "pcm_loam_deskew_tables", "pcm_loam_extract_features_deskew", "pcm_loam_frame_begin_deskew", "pcm_loam_frame_begin_batch_deskew",
    "pcm_loam_cloud_default_desc", "pcm_loam_cloud_prepare", "pcm_loam_cloud_cached", "pcm_loam_frame_begin_cloud", "pcm_loam_frame_begin_cloud_batch",
    "pcm_loam_default_submap_params", "pcm_loam_keyframe_add", "pcm_loam_keyframe_set_poses", "pcm_loam_keyframe_count", "pcm_loam_keyframe_clear",
    "pcm_loam_keyframe_get", "pcm_loam_submap_update", "pcm_loam_submap_near", "pcm_loam_submap_info",
    "pcm_loam_default_sc_params", "pcm_loam_sc_add", "pcm_loam_sc_put", "pcm_loam_sc_get", "pcm_loam_sc_count", "pcm_loam_sc_shape", "pcm_loam_sc_clear",
    "pcm_loam_sc_detect", "pcm_loam_sc_distance", "pcm_loam_loop_detect_distance", "pcm_loam_sc_add_near",
    "pcm_loam_submap_near_dev", "pcm_loam_default_loop_params", "pcm_loam_loop_verify", "pcm_loam_loop_closure", "pcm_loam_loop_verifier_exists",
    "pcm_loam_default_global_params", "pcm_loam_global_keys", "pcm_loam_global_map", "pcm_loam_map_export", "pcm_loam_global_gather_ms",
    "pcm_loam_default_dynmap_params", "pcm_loam_tile_add", "pcm_loam_tile_count", "pcm_loam_tile_clear", "pcm_loam_dynmap_need_load",
    "pcm_loam_dynmap_load", "pcm_loam_dynmap_crop", "pcm_loam_dynmap_info", "pcm_loam_dynmap_global",
    "pcm_loam_default_tiles_params", "pcm_loam_tiles_build", "pcm_loam_tile_info", "pcm_loam_tile_get", "pcm_loam_tiles_build_ms",
    "pcm_loam_tile_share", "pcm_loam_tile_share_count", "pcm_loam_dynmap_crop_batch",
    "pcm_occ_default_params", "pcm_occ_reset", "pcm_occ_insert_scans", "pcm_occ_insert_keyframes", "pcm_occ_get_scan", "pcm_occ_status",
    "pcm_occ_info", "pcm_occ_get_map", "pcm_occ_get_pgm", "pcm_occ_get_counts",
    "pcm_scan_default_fuse_params", "pcm_scan_fuse", "pcm_scan_fused",
    "pcm_lidar_default_desc", "pcm_lidar_filter", "pcm_lio_frame_begin_cloud",
    "pcm_lio_default_update_params", "pcm_lio_update", "pcm_lio_update_trace",
    "pcm_lio_default_imu_state", "pcm_lio_imu_init", "pcm_lio_propagate",
    "pcm_share_target", "pcm_target_share_count",
    "pcm_neighbour_list_info", "pcm_neighbour_list_headroom", "pcm_neighbour_list_update_ms",
    "pcm_lio_frame_world", "pcm_lio_frame_body", "pcm_lio_frame_effect", "pcm_lio_map_append", "pcm_lio_map_info_get", "pcm_lio_map_get",
    "pcm_lio_map_clear", "pcm_lio_map_export",
    "pcm_lio_search_path",
    "pcm_icp_default_params", "pcm_icp_set_params", "pcm_icp_get_params", "pcm_icp_last", "pcm_icp_trace",
    "pcm_loam_default_sc_loop_params", "pcm_loam_sc_loop_verify", "pcm_loam_sc_loop_closure", "pcm_loam_sc_loop_verifier_exists",
    "pcm_octo_default_params", "pcm_octo_reset", "pcm_octo_insert_scan", "pcm_octo_insert_keyframes", "pcm_octo_info", "pcm_octo_get_cells",
    "pcm_octo_get_occupied", "pcm_octo_project", "pcm_octo_get_pgm", "pcm_octo_debug", "pcm_octo_phase_ms",
]

PCM_ABI_VERSION = 3   # include/pcm_amd.h
PCM_OK = 0
PCM_FLAG_NO_LDS_STAGING = 1
PCM_FLAG_FUSED_STEP = 2
PCM_FLAG_COUNTED_SEARCH = 8           # k_linearize_counted instead of k_linearize (A/B; same results, measured slower)
PCM_FLAG_NEIGHBOUR_LISTS = 16           # static targets: per-voxel candidate lists built with the map (default: from the 2nd registration on), same results
PCM_FLAG_FOLLOWING_LISTS = 128          # P2PLANE: the lists follow a target that grows (target_insert / map_incremental): touched runs are rewritten, same results
PCM_FLAG_NO_NEIGHBOUR_LISTS = 64        # never: the tile kernel serves every pass
PCM_FLAG_REFERENCE_KNN_ORDER = 32      # neighbours in the order of libstdc++'s std::nth_element (the reference's), slower kernel
PCM_FLAG_LIO_REFERENCE_SEMANTICS = 4   # pcm_obs_model keeps LaserMapping's per-point members across calls and scans
PCM_ERR_INVALID_ARGUMENT = -1
PCM_ERR_NO_INPUT = -2
PCM_ERR_UNSUPPORTED = -4
PCM_ERR_OUT_OF_RANGE = -5
PCM_ERR_NOT_CONVERGED = -6
PCM_ERR_INTERNAL = -7
PCM_ERR_TOO_FEW_FEATURES = -8          # LOAM: not enough corner / surf features, pose left as given
MEM_HOST, MEM_DEVICE = 0, 1
MODEL = {"P2PLANE": 0, "GICP": 1, "VGICP": 2, "NDT_P2D": 3, "NDT_D2D": 4, "NDT_OMP": 5, "VGICP_CUDA": 6, "LOAM": 7, "ICP": 8}
OPTIMIZER = {"GN": 0, "LM": 1}
REGULARIZATION = {"NONE": 0, "MIN_EIG": 1, "NORMALIZED_MIN_EIG": 2, "PLANE": 3, "FROBENIUS": 4, "PCLOMP": 5}


class PcmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pcm error %d: %s" % (code, msg))
        self.code = code


class PcmConfig(C.Structure):
    _fields_ = [("model", C.c_int32), ("optimizer", C.c_int32), ("max_iterations", C.c_int32),
                ("lm_max_iterations", C.c_int32), ("rotation_eps", C.c_double),
                ("translation_eps", C.c_double), ("lm_init_lambda_factor", C.c_double),
                ("voxel_resolution", C.c_float), ("num_neighbors", C.c_int32), ("knn", C.c_int32),
                ("min_knn", C.c_int32), ("max_range", C.c_float), ("plane_threshold", C.c_float),
                ("max_corr_dist", C.c_float), ("k_correspondences", C.c_int32),
                ("regularization", C.c_int32), ("sort_source", C.c_int32), ("flags", C.c_int32),
                ("map_capacity", C.c_int32), ("ndt_step_size", C.c_float), ("ndt_outlier_ratio", C.c_float),
                ("batch_window", C.c_int32), ("voxel_mode", C.c_int32), ("neighbor_search_radius", C.c_float),
                ("covariance_method", C.c_int32), ("rbf_kernel_width", C.c_float), ("rbf_max_dist", C.c_float)]


class PcmResult(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("T64", C.c_double * 16), ("H", C.c_double * 36),
                ("cost", C.c_double), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("num_linearize", C.c_int32), ("num_compute_error", C.c_int32),
                ("num_inliers", C.c_int32), ("status", C.c_int32)]


class PcmLioState(C.Structure):
    _fields_ = [("rot", C.c_double * 4), ("pos", C.c_double * 3), ("off_R", C.c_double * 4), ("off_T", C.c_double * 3)]


class PcmLioMapInfo(C.Structure):   # pcm_lio_map_info
    _fields_ = [("points", C.c_uint64), ("capacity", C.c_uint64), ("frames_appended", C.c_uint64), ("growths", C.c_uint64),
                ("scan_wait_num", C.c_int32), ("pcd_index", C.c_int32), ("chunk_ready", C.c_int32), ("reserved", C.c_int32)]


class PcmObsResult(C.Structure):
    _fields_ = [("HTH", C.c_double * 144), ("HTh", C.c_double * 12), ("sum_h2", C.c_double), ("n_eff", C.c_int32), ("valid", C.c_int32)]


class PcmLioFilterState(C.Structure):   # state_ikfom, DOF 23 in this order
    _fields_ = [("pos", C.c_double * 3), ("rot", C.c_double * 4), ("off_R", C.c_double * 4), ("off_T", C.c_double * 3), ("vel", C.c_double * 3),
                ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("grav", C.c_double * 3)]


class PcmLioUpdateParams(C.Structure):
    _fields_ = [("R", C.c_double), ("max_iter", C.c_int32), ("extrinsic_est_en", C.c_int32), ("limit", C.c_double * 23), ("reserved", C.c_int32 * 8)]


class PcmLioUpdateResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("rematches", C.c_int32), ("valid_calls", C.c_int32), ("t", C.c_int32), ("n_eff_last", C.c_int32),
                ("status", C.c_int32), ("sum_h2_last", C.c_double), ("reserved", C.c_int32 * 8)]


class PcmImuSample(C.Structure):   # sensor_msgs::Imu: stamp, linear_acceleration, angular_velocity
    _fields_ = [("t", C.c_double), ("acc", C.c_double * 3), ("gyr", C.c_double * 3)]


class PcmLioImuState(C.Structure):   # the members of ImuProcess
    _fields_ = [("mean_acc", C.c_double * 3), ("mean_gyr", C.c_double * 3), ("cov_acc", C.c_double * 3), ("cov_gyr", C.c_double * 3),
                ("cov_bias_gyr", C.c_double * 3), ("cov_bias_acc", C.c_double * 3), ("cov_acc_scale", C.c_double * 3), ("cov_gyr_scale", C.c_double * 3),
                ("lidar_T_wrt_imu", C.c_double * 3), ("lidar_R_wrt_imu", C.c_double * 4), ("angvel_last", C.c_double * 3), ("acc_s_last", C.c_double * 3),
                ("last_lidar_end_time", C.c_double), ("last_imu", PcmImuSample), ("init_iter_num", C.c_int32), ("first_frame", C.c_int32),
                ("need_init", C.c_int32), ("reserved", C.c_int32 * 5)]


class PcmLioFrameParams(C.Structure):
    _fields_ = [("num_scans", C.c_int32), ("point_filter_num", C.c_int32), ("blind", C.c_double), ("leaf_size", C.c_float), ("reserved", C.c_int32)]


class PcmStats(C.Structure):
    _fields_ = [("linearize_launches", C.c_uint64), ("point_passes", C.c_uint64),
                ("candidates", C.c_uint64), ("slots_probed", C.c_uint64), ("linearize_ms", C.c_double),
                ("target_voxels", C.c_uint64), ("target_slots", C.c_uint64), ("tiles", C.c_uint64),
                ("tiles_lds_grid", C.c_uint64), ("tiles_lds_points", C.c_uint64), ("residual_ms", C.c_double),
                ("timed_launches", C.c_uint64), ("timed_pair_slots", C.c_uint64), ("launched_pair_slots", C.c_uint64),
                ("lru_batch_hazards", C.c_uint64)]


class PcmLoamParams(C.Structure):
    _fields_ = [("iter_num", C.c_int32), ("edge_min_valid", C.c_int32), ("surf_min_valid", C.c_int32), ("reserved0", C.c_int32),
                ("rot_conv_deg", C.c_double), ("trans_conv_cm", C.c_double), ("degeneracy_threshold", C.c_double),
                ("search_cell", C.c_float), ("reserved", C.c_int32 * 7)]


class PcmLoamResult(C.Structure):
    _fields_ = [("x", C.c_float * 6), ("iterations", C.c_int32), ("converged", C.c_int32), ("degenerate", C.c_int32),
                ("status", C.c_int32), ("eigenvalues", C.c_double * 6), ("num_corner", C.c_int32), ("num_surf", C.c_int32),
                ("corner_fitness", C.c_double), ("surf_fitness", C.c_double), ("maps_built", C.c_int32), ("reserved", C.c_int32)]


PCM_LOAM_FEATURES_FORCE_SERIAL_SORT = 1


class PcmLoamFeatureParams(C.Structure):
    _fields_ = [("n_scan", C.c_int32), ("horizon_scan", C.c_int32), ("downsample_rate", C.c_int32), ("area_num", C.c_int32),
                ("min_range", C.c_float), ("max_range", C.c_float), ("edge_threshold", C.c_float), ("surf_threshold", C.c_float),
                ("odometry_surf_leaf", C.c_float), ("mapping_corner_leaf", C.c_float), ("mapping_surf_leaf", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_int32 * 8)]


class PcmLoamFeaturesResult(C.Structure):
    _fields_ = [("num_extracted", C.c_int32), ("num_corner_scan", C.c_int32), ("num_surf_scan", C.c_int32), ("num_corner", C.c_int32),
                ("num_surf", C.c_int32), ("sectors", C.c_int32), ("sectors_serial", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32 * 8)]


PCM_LOAM_TIME_DOUBLE, PCM_LOAM_TIME_FLOAT = 0, 1
PCM_LOAM_DESKEW_READY, PCM_LOAM_DESKEW_WAITING = 0, 1


class PcmLoamDeskew(C.Structure):
    _fields_ = [("time_scan_cur", C.c_double), ("imu_time", C.c_void_p), ("imu_rot_x", C.c_void_p), ("imu_rot_y", C.c_void_p), ("imu_rot_z", C.c_void_p),
                ("odom_time", C.c_void_p), ("odom_incre_x", C.c_void_p), ("odom_incre_y", C.c_void_p), ("odom_incre_z", C.c_void_p),
                ("n_imu", C.c_int32), ("n_odom", C.c_int32), ("imu_available", C.c_int32), ("time_kind", C.c_int32),
                ("time_offset_bytes", C.c_size_t), ("reserved", C.c_int32 * 8)]


class PcmLoamImuSample(C.Structure):   # sensor_msgs::Imu through imuConverter: stamp, angular_velocity
    _fields_ = [("t", C.c_double), ("gyro", C.c_double * 3)]


class PcmLoamOdomSample(C.Structure):   # nav_msgs::Odometry: stamp, pose.pose.position
    _fields_ = [("t", C.c_double), ("xyz", C.c_double * 3)]


class PcmLoamDeskewInput(C.Structure):
    _fields_ = [("time_scan_cur", C.c_double), ("time_scan_next", C.c_double), ("imu", C.c_void_p), ("odom", C.c_void_p),
                ("n_imu", C.c_int32), ("n_odom", C.c_int32), ("reserved", C.c_int32 * 4)]


class PcmLoamDeskewResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("imu_skipped", C.c_int32), ("odom_skipped", C.c_int32), ("n_imu", C.c_int32), ("n_odom", C.c_int32),
                ("imu_available", C.c_int32), ("odom_available", C.c_int32), ("odom_deskew", C.c_int32), ("start_odom_index", C.c_int32),
                ("reserved", C.c_int32 * 7)]


PCM_LOAM_LIDAR_VELODYNE, PCM_LOAM_LIDAR_RSLIDAR_RUBY, PCM_LOAM_LIDAR_RSLIDAR_16, PCM_LOAM_LIDAR_RSLIDAR_32 = 0, 1, 2, 3   # utility.h:116-121
PCM_LOAM_CLOUD_MAPPING, PCM_LOAM_CLOUD_LOCALIZATION = 0, 1
PCM_LOAM_INTENSITY_UINT8, PCM_LOAM_INTENSITY_FLOAT = 0, 1
PCM_LOAM_RING_UINT16 = 0
PCM_LOAM_FIELD_ABSENT = C.c_size_t(-1).value


class PcmLoamCloudDesc(C.Structure):
    _fields_ = [("height", C.c_uint32), ("width", C.c_uint32), ("point_step", C.c_size_t), ("xyz_offset_bytes", C.c_size_t),
                ("intensity_offset_bytes", C.c_size_t), ("ring_offset_bytes", C.c_size_t), ("time_offset_bytes", C.c_size_t),
                ("intensity_kind", C.c_int32), ("ring_kind", C.c_int32), ("time_kind", C.c_int32), ("is_dense", C.c_int32),
                ("lidar_type", C.c_int32), ("record_kind", C.c_int32), ("synth_ring", C.c_int32), ("synth_time", C.c_int32),
                ("reserved", C.c_int32 * 8)]


class PcmLoamCloudResult(C.Structure):
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_nonfinite", C.c_uint64), ("ring_synthesised", C.c_int32),
                ("time_synthesised", C.c_int32), ("time_available", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32 * 8)]


class PcmLoamSubmapParams(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("keypose_density", C.c_float), ("corner_leaf", C.c_float), ("surf_leaf", C.c_float),
                ("recent_window_s", C.c_double), ("reserved", C.c_int32 * 8)]


class PcmLoamSubmapResult(C.Structure):
    _fields_ = [("num_keyframes", C.c_int32), ("num_near", C.c_int32), ("num_pose_leaves", C.c_int32), ("num_selected", C.c_int32),
                ("num_skipped", C.c_int32), ("num_corner_in", C.c_int32), ("num_surf_in", C.c_int32), ("num_corner_map", C.c_int32),
                ("num_surf_map", C.c_int32), ("rebuilt", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32 * 5)]


PCM_LOAM_SC_POINTS, PCM_LOAM_SC_KEYFRAME_SURF, PCM_LOAM_SC_KEYFRAME_NEAR = 0, 1, 2


class PcmLoamScParams(C.Structure):
    _fields_ = [("lidar_height", C.c_double), ("max_radius", C.c_double), ("search_ratio", C.c_double), ("dist_threshold", C.c_double),
                ("num_ring", C.c_int32), ("num_sector", C.c_int32), ("num_exclude_recent", C.c_int32), ("num_candidates", C.c_int32),
                ("tree_making_period", C.c_int32), ("leaf", C.c_float), ("reserved", C.c_int32 * 8)]


class PcmLoamScAddResult(C.Structure):
    _fields_ = [("index", C.c_int32), ("num_points_in", C.c_int32), ("num_points", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32 * 4)]


class PcmLoamScResult(C.Structure):
    _fields_ = [("loop_id", C.c_int32), ("yaw_diff_rad", C.c_float), ("min_dist", C.c_double), ("nn_idx", C.c_int32), ("nn_align", C.c_int32),
                ("num_descriptors", C.c_int32), ("tree_size", C.c_int32), ("tree_rebuilt", C.c_int32), ("num_evaluated", C.c_int32),
                ("status", C.c_int32), ("reserved0", C.c_int32), ("cand_index", C.c_int32 * 64), ("cand_d2", C.c_float * 64),
                ("cand_dist", C.c_double * 64), ("cand_shift", C.c_int32 * 64), ("reserved", C.c_int32 * 8)]


PCM_LOAM_LOOP_ACCEPTED, PCM_LOAM_LOOP_REJECTED_SIZE, PCM_LOAM_LOOP_REJECTED_NOT_CONVERGED, PCM_LOAM_LOOP_REJECTED_FITNESS, PCM_LOAM_LOOP_NONE = 0, 1, 2, 3, 4


class PcmLoamLoopParams(C.Structure):
    _fields_ = [("history_search_num", C.c_int32), ("min_cur_points", C.c_int32), ("min_prev_points", C.c_int32), ("wrt_key", C.c_int32),
                ("fitness_threshold", C.c_float), ("near_leaf", C.c_float), ("ndt_epsilon", C.c_double), ("ndt_resolution", C.c_float),
                ("ndt_num_neighbors", C.c_int32), ("reserved", C.c_int32 * 8)]


class PcmLoamLoopResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("key_cur", C.c_int32), ("key_pre", C.c_int32), ("num_cur_points", C.c_int32), ("num_prev_points", C.c_int32),
                ("ndt_iterations", C.c_int32), ("ndt_converged", C.c_int32), ("noise_variance", C.c_float), ("fitness", C.c_double),
                ("correction", C.c_float * 16), ("pose_from", C.c_double * 6), ("pose_to", C.c_double * 6), ("between", C.c_double * 16),
                ("between6", C.c_double * 6), ("reserved", C.c_int32 * 8)]


class PcmLoamScLoopParams(C.Structure):
    _fields_ = [("history_search_num", C.c_int32), ("min_cur_points", C.c_int32), ("min_prev_points", C.c_int32), ("icp_max_iterations", C.c_int32),
                ("fitness_threshold", C.c_float), ("near_leaf", C.c_float), ("icp_max_correspondence_distance", C.c_double),
                ("icp_transformation_epsilon", C.c_double), ("icp_euclidean_fitness_epsilon", C.c_double), ("icp_voxel_resolution", C.c_float),
                ("reserved", C.c_int32 * 9)]


class PcmLoamScLoopResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("key_cur", C.c_int32), ("key_pre", C.c_int32), ("num_cur_points", C.c_int32), ("num_prev_points", C.c_int32),
                ("icp_iterations", C.c_int32), ("icp_converged", C.c_int32), ("icp_stop_reason", C.c_int32), ("yaw_diff_rad", C.c_float),
                ("noise_variance", C.c_float), ("cauchy_k", C.c_double), ("fitness", C.c_double), ("correction", C.c_float * 16),
                ("pose_from", C.c_double * 6), ("pose_to", C.c_double * 6), ("between", C.c_double * 16), ("between6", C.c_double * 6),
                ("reserved", C.c_int32 * 8)]


PCM_MODEL_ICP = 8
PCM_ICP_STOP_NONE, PCM_ICP_STOP_ITERATIONS, PCM_ICP_STOP_TRANSFORM, PCM_ICP_STOP_ABS_MSE, PCM_ICP_STOP_REL_MSE, PCM_ICP_STOP_NO_CORRESPONDENCES = 0, 1, 2, 3, 4, 5
PCM_ICP_CHUNK_ITERATIONS = 8


class PcmIcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("rotation_epsilon", C.c_double), ("euclidean_fitness_epsilon", C.c_double), ("mse_absolute", C.c_double), ("reserved", C.c_int32 * 8)]


class PcmIcpInfo(C.Structure):
    _fields_ = [("stop_reason", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32), ("reserved0", C.c_int32), ("num_pairs", C.c_uint64),
                ("mse", C.c_double), ("reserved", C.c_int32 * 8)]


class PcmLoamGlobalParams(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("keypose_density", C.c_float), ("leaf", C.c_float)]


class PcmLoamGlobalResult(C.Structure):
    _fields_ = [("num_near", C.c_int32), ("num_pose_leaves", C.c_int32), ("num_skipped", C.c_int32), ("num_used", C.c_int32),
                ("points_in", C.c_uint64), ("points_out", C.c_uint64)]


class PcmVoxelLargeResult(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("finite_points", C.c_uint64), ("pieces", C.c_uint64), ("depth", C.c_uint32), ("levels", C.c_uint32),
                ("host_waits", C.c_uint32), ("reserved", C.c_uint32), ("workspace_bytes", C.c_uint64)]


class PcmLoamDynmapParams(C.Structure):
    _fields_ = [("max_range", C.c_float), ("margin", C.c_int32), ("area_size", C.c_int32), ("crop_x", C.c_int32), ("reserved", C.c_int32 * 8)]


class PcmLoamDynmapLoadResult(C.Structure):
    _fields_ = [("num_corner_tiles", C.c_int32), ("num_surf_tiles", C.c_int32), ("num_corner_selected", C.c_int32), ("num_surf_selected", C.c_int32),
                ("num_corner_points", C.c_int64), ("num_surf_points", C.c_int64), ("generation", C.c_uint64), ("changed", C.c_int32),
                ("reserved", C.c_int32 * 5)]


class PcmLoamDynmapCropResult(C.Structure):
    _fields_ = [("num_corner_in", C.c_int32), ("num_surf_in", C.c_int32), ("num_corner", C.c_int32), ("num_surf", C.c_int32),
                ("num_nonfinite", C.c_int32), ("rebuilt", C.c_int32), ("x_lo", C.c_float), ("x_hi", C.c_float), ("y_lo", C.c_float),
                ("y_hi", C.c_float), ("status", C.c_int32), ("reserved", C.c_int32 * 5)]


PCM_LOAM_TILES_STAGES = 9
TILES_STAGE_NAMES = ("workspace_host", "tile_keys", "key_sort", "distinct_keys", "rank", "tile_minmax", "cell_sort", "means_scatter", "tile_stats")


class PcmLoamTilesParams(C.Structure):
    _fields_ = [("tile_size", C.c_float), ("leaf_corner", C.c_float), ("leaf_surf", C.c_float), ("reserved", C.c_int32 * 9)]


class PcmLoamTilesResult(C.Structure):
    _fields_ = [("num_corner_tiles", C.c_int32), ("num_surf_tiles", C.c_int32), ("corner_points_in", C.c_uint64), ("surf_points_in", C.c_uint64),
                ("corner_points_out", C.c_uint64), ("surf_points_out", C.c_uint64), ("num_nonfinite", C.c_uint64), ("reserved", C.c_int32 * 6)]


class PcmOccParams(C.Structure):
    _fields_ = [("min_z", C.c_double), ("max_z", C.c_double), ("angle_increment", C.c_double), ("min_range", C.c_double),
                ("max_range", C.c_double), ("log_occ", C.c_double), ("log_free", C.c_double), ("resolution", C.c_double),
                ("max_radius", C.c_double), ("fill_with_white", C.c_int32), ("use_nan", C.c_int32), ("reserved", C.c_int32 * 8)]


class PcmOctoParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("prob_hit", C.c_double), ("prob_miss", C.c_double), ("clamp_min", C.c_double), ("clamp_max", C.c_double),
                ("max_range", C.c_double), ("min_range", C.c_double), ("pointcloud_min_x", C.c_double), ("pointcloud_max_x", C.c_double),
                ("pointcloud_min_y", C.c_double), ("pointcloud_max_y", C.c_double), ("pointcloud_min_z", C.c_double), ("pointcloud_max_z", C.c_double),
                ("occupancy_min_z", C.c_double), ("occupancy_max_z", C.c_double), ("min_x_size", C.c_double), ("min_y_size", C.c_double),
                ("filter_speckles", C.c_int32), ("reserved0", C.c_int32), ("initial_cells", C.c_uint64), ("max_cells", C.c_uint64),
                ("reserved", C.c_int32 * 8)]


class PcmOctoInsertResult(C.Structure):
    _fields_ = [("points_in", C.c_uint64), ("dropped_nonfinite", C.c_uint64), ("skipped_window", C.c_uint64), ("skipped_min_range", C.c_uint64),
                ("truncated", C.c_uint64), ("rejected_rays", C.c_uint64), ("cells_touched", C.c_uint64), ("new_cells", C.c_uint64),
                ("table_growths", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_int32 * 8)]


class PcmOctoMapInfo(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("occupied", C.c_uint64), ("free_cells", C.c_uint64), ("capacity", C.c_uint64), ("epoch", C.c_uint64),
                ("key_min", C.c_int32 * 3), ("key_max", C.c_int32 * 3), ("metric_min", C.c_double * 3), ("metric_max", C.c_double * 3),
                ("resolution", C.c_double), ("hit", C.c_float), ("miss", C.c_float), ("clamp_min", C.c_float), ("clamp_max", C.c_float),
                ("reserved", C.c_int32 * 8)]


class PcmOctoGridInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("min_key_x", C.c_int32), ("min_key_y", C.c_int32), ("resolution", C.c_double),
                ("origin_x", C.c_double), ("origin_y", C.c_double), ("reserved", C.c_int32 * 8)]


PCM_SCAN_MAX_SEGMENTS = 8
PCM_SCAN_LIDAR_XYZIRT, PCM_SCAN_LIDAR_XYZI, PCM_SCAN_DEPTH = 0, 1, 2
PCM_SCAN_INTENSITY_FLOAT, PCM_SCAN_INTENSITY_UINT8 = 0, 1
PCM_SCAN_RING_BY_HEIGHT, PCM_SCAN_RING_DIV_WIDTH, PCM_SCAN_RING_MOD_HEIGHT = 0, 1, 2
PCM_SCAN_OUT_XYZI, PCM_SCAN_OUT_XYZIR, PCM_SCAN_OUT_XYZIRT = 0, 1, 2


class PcmScanSegment(C.Structure):
    _fields_ = [("kind", C.c_int32), ("memory", C.c_int32), ("points", C.c_void_p), ("n", C.c_size_t), ("stride_bytes", C.c_size_t),
                ("intensity_offset_bytes", C.c_size_t), ("ring_offset_bytes", C.c_size_t), ("timestamp_offset_bytes", C.c_size_t),
                ("intensity_type", C.c_int32), ("ring_rule", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("ring_table", C.c_void_p), ("ring_table_len", C.c_int32), ("dt_sec", C.c_int32), ("dt_nsec", C.c_int32),
                ("reserved", C.c_int32), ("T", C.c_double * 16)]


class PcmScanFuseParams(C.Structure):
    _fields_ = [("depth_filter", C.c_double), ("pitch_scale", C.c_double), ("pitch_min", C.c_double), ("pitch_max", C.c_double),
                ("pitch_offset", C.c_double), ("pitch_ring_table", C.c_void_p), ("pitch_ring_table_len", C.c_int32),
                ("ring_below", C.c_int32), ("ring_otherwise", C.c_int32), ("depth_intensity", C.c_float), ("output_layout", C.c_int32),
                ("reserved", C.c_int32 * 9)]


class PcmScanSegmentCounts(C.Structure):
    _fields_ = [("n_in", C.c_uint32), ("n_nan", C.c_uint32), ("n_depth_filtered", C.c_uint32), ("n_kept", C.c_uint32),
                ("out_offset", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class PcmScanFuseResult(C.Structure):
    _fields_ = [("seg", PcmScanSegmentCounts * PCM_SCAN_MAX_SEGMENTS), ("n_out", C.c_uint32), ("n_pitch_index_clamped", C.c_uint32),
                ("status", C.c_int32), ("reserved", C.c_int32 * 5)]


PCM_LIDAR_VELODYNE, PCM_LIDAR_OUSTER, PCM_LIDAR_RSLIDAR, PCM_LIDAR_LIVOX_STD = 2, 3, 4, 5   # the reference's LidarType values
PCM_LIDAR_TIME_FLOAT, PCM_LIDAR_TIME_DOUBLE, PCM_LIDAR_TIME_UINT32 = 0, 1, 2
PCM_LIDAR_RING_UINT8, PCM_LIDAR_RING_UINT16 = 0, 1
PCM_LIDAR_MAX_SCANS = 256


class PcmLidarDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("time_kind", C.c_int32), ("ring_kind", C.c_int32), ("num_scans", C.c_int32), ("point_filter_num", C.c_int32),
                ("time_scale", C.c_float), ("stride_bytes", C.c_size_t), ("xyz_offset_bytes", C.c_size_t), ("intensity_offset_bytes", C.c_size_t),
                ("time_offset_bytes", C.c_size_t), ("ring_offset_bytes", C.c_size_t), ("blind", C.c_double), ("reserved", C.c_int32 * 8)]


def library_path() -> str:
    """The in-tree build; PCM_AMD_LIBRARY names another build of the same ABI (A/B measurements of two builds on one box)."""
    return os.environ.get("PCM_AMD_LIBRARY") or os.path.join(_HERE, "libpcm_amd.so")


def build_library(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    so = library_path()
    src_dir = os.path.join(_HERE, "csrc")
    inc = os.path.join(os.path.dirname(_HERE), "include", "pcm_amd.h")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if f.endswith((".hip", ".h"))] + [inc]
    stale = force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", src_dir, "-s", "-j4"])
    return so


def load_library():
    """Load libpcm_amd.so.  Raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # One HIP runtime per process: the torch wheel bundles its own libamdhip64.so.7
    # (same SONAME as /opt/rocm's).  If libpcm_amd.so pulled in the system copy
    # first, a later `import torch` would load a second runtime that finds no GPU;
    # importing torch first lets the dynamic loader reuse torch's copy for us.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    so = library_path()
    if not os.path.exists(so):
        raise PcmError(-3, "libpcm_amd.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(so)
    vp, i32, u64, sz = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
    L.pcm_abi_version.restype = i32
    L.pcm_default_config.argtypes = [C.POINTER(PcmConfig)]
    L.pcm_default_config.restype = None
    L.pcm_create.argtypes = [i32, C.POINTER(PcmConfig)]
    L.pcm_create.restype = vp
    L.pcm_destroy.argtypes = [vp]
    L.pcm_destroy.restype = None
    L.pcm_last_error.argtypes = [vp]
    L.pcm_last_error.restype = C.c_char_p
    L.pcm_get_config.argtypes = [vp, C.POINTER(PcmConfig)]
    L.pcm_set_config.argtypes = [vp, C.POINTER(PcmConfig)]
    L.pcm_set_stream.argtypes = [vp, vp]
    for f in (L.pcm_set_target, L.pcm_set_source):
        f.argtypes = [vp, vp, sz, sz, i32, u64]
    for f in (L.pcm_swap_source_and_target, L.pcm_clear_source, L.pcm_clear_target, L.pcm_reset_stats):
        f.argtypes = [vp]
    L.pcm_share_target.argtypes = [vp, vp]
    L.pcm_target_share_count.argtypes = [vp]
    L.pcm_align.argtypes = [vp, vp, C.POINTER(PcmResult)]
    L.pcm_linearize.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.pcm_compute_error.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.pcm_get_planes.argtypes = [vp, vp, sz]
    L.pcm_get_neighbour_lists.argtypes = [vp, vp, vp, vp, vp]
    L.pcm_neighbour_list_info.argtypes = [vp, vp]
    L.pcm_neighbour_list_update_ms.argtypes = [vp, vp]
    L.pcm_lio_search_path.argtypes = [vp, vp]
    L.pcm_neighbour_list_headroom.argtypes = [vp, C.c_float, u64]
    L.pcm_get_lio_members.argtypes = [vp, vp, vp, sz]
    L.pcm_obs_model.argtypes = [vp, C.POINTER(PcmLioState), i32, i32, C.POINTER(PcmObsResult)]
    L.pcm_target_insert.argtypes = [vp, vp, sz, sz, i32]
    L.pcm_map_incremental.argtypes = [vp, C.POINTER(PcmLioState), C.c_float, i32, C.POINTER(sz)]
    L.pcm_get_target.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.pcm_get_covariances.argtypes = [vp, C.c_int, vp, sz, C.POINTER(sz)]
    L.pcm_livox_filter.argtypes = [vp, vp, sz, C.c_int, C.c_int, C.c_int, C.c_double, vp, sz, C.POINTER(sz)]
    L.pcm_set_covariances.argtypes = [vp, C.c_int, vp, sz, C.c_int]
    L.pcm_ndt_derivatives.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_double), vp, vp]
    L.pcm_ndt_score.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.pcm_fitness_score.argtypes = [vp, vp, C.c_double, C.POINTER(C.c_double)]
    L.pcm_voxel_downsample.argtypes = [vp, vp, sz, sz, C.c_int, C.c_float, vp, sz, C.POINTER(sz)]
    L.pcm_voxel_downsample_large.argtypes = [vp, vp, sz, sz, C.c_int, C.c_float, vp, sz, C.POINTER(PcmVoxelLargeResult)]
    L.pcm_approx_voxel_downsample.argtypes = [vp, vp, sz, sz, C.c_int, C.c_float, vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.pcm_gicp_bfgs_set_correspondences.argtypes = [vp, vp, sz, vp, sz, sz, vp, vp, sz, vp, C.c_int]
    L.pcm_gicp_bfgs_fdf.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_double), vp]
    L.pcm_gicp_bfgs_update_correspondences.argtypes = [vp, vp, vp, C.POINTER(sz)]
    L.pcm_gicp_bfgs_get_correspondences.argtypes = [vp, vp, vp, vp, sz]
    L.pcm_undistort.argtypes = [vp, vp, sz, sz, sz, C.c_int, vp, C.c_int, C.POINTER(PcmLioState)]
    L.pcm_align_batch.argtypes = [C.POINTER(vp), i32, vp, vp, vp]
    L.pcm_set_profiling.argtypes = [vp, i32]
    L.pcm_debug_phase_cycles.argtypes = [vp, vp]
    L.pcm_get_stats.argtypes = [vp, C.POINTER(PcmStats)]
    L.pcm_lio_frame_begin.argtypes = [vp, vp, sz, C.c_int, C.POINTER(PcmLioFrameParams), vp, C.c_int, C.POINTER(PcmLioState), C.POINTER(sz)]
    L.pcm_lio_frame_end.argtypes = [vp, C.POINTER(PcmLioState), C.c_float, i32, C.POINTER(sz)]
    L.pcm_get_source.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.pcm_loam_default_params.argtypes = [C.POINTER(PcmLoamParams)]
    L.pcm_loam_default_params.restype = None
    for f in (L.pcm_loam_set_target, L.pcm_loam_set_source):
        f.argtypes = [vp, vp, sz, vp, sz, sz, i32, u64]
    L.pcm_loam_align.argtypes = [vp, C.POINTER(PcmLoamParams), vp, C.POINTER(PcmLoamResult)]
    L.pcm_loam_align_batch.argtypes = [C.POINTER(vp), i32, C.POINTER(PcmLoamParams), vp, C.POINTER(PcmLoamResult)]
    L.pcm_loam_coefficients.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.pcm_loam_neighbours.argtypes = [vp, vp, vp, vp]
    L.pcm_loam_default_feature_params.argtypes = [C.POINTER(PcmLoamFeatureParams)]
    L.pcm_loam_default_feature_params.restype = None
    L.pcm_loam_extract_features.argtypes = [vp, vp, sz, sz, sz, sz, i32, C.POINTER(PcmLoamFeatureParams), vp, sz, vp, sz, C.POINTER(PcmLoamFeaturesResult)]
    L.pcm_loam_frame_begin.argtypes = [vp, vp, sz, sz, sz, sz, i32, C.POINTER(PcmLoamFeatureParams), C.POINTER(PcmLoamFeaturesResult)]
    L.pcm_loam_frame_begin_batch.argtypes = [C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(sz), sz, sz, sz, i32, C.POINTER(PcmLoamFeatureParams),
                                             C.POINTER(PcmLoamFeaturesResult)]
    L.pcm_loam_feature_info.argtypes = [vp] * 12
    L.pcm_loam_deskew_tables.argtypes = [C.POINTER(PcmLoamDeskewInput), vp, sz, vp, sz, C.POINTER(PcmLoamDeskew), C.POINTER(PcmLoamDeskewResult)]
    L.pcm_loam_extract_features_deskew.argtypes = L.pcm_loam_extract_features.argtypes + [C.POINTER(PcmLoamDeskew)]
    L.pcm_loam_frame_begin_deskew.argtypes = L.pcm_loam_frame_begin.argtypes + [C.POINTER(PcmLoamDeskew)]
    L.pcm_loam_frame_begin_batch_deskew.argtypes = L.pcm_loam_frame_begin_batch.argtypes + [C.POINTER(C.POINTER(PcmLoamDeskew))]
    L.pcm_loam_cloud_default_desc.argtypes = [i32, i32, C.POINTER(PcmLoamCloudDesc)]
    L.pcm_loam_cloud_prepare.argtypes = [vp, vp, C.POINTER(PcmLoamCloudDesc), i32, vp, sz, i32, C.POINTER(PcmLoamCloudResult)]
    L.pcm_loam_cloud_cached.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.pcm_loam_frame_begin_cloud.argtypes = [vp, vp, C.POINTER(PcmLoamCloudDesc), i32, C.POINTER(PcmLoamFeatureParams), C.POINTER(PcmLoamFeaturesResult),
                                             C.POINTER(PcmLoamDeskew), C.POINTER(PcmLoamCloudResult)]
    L.pcm_loam_frame_begin_cloud_batch.argtypes = [C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(PcmLoamCloudDesc), i32, C.POINTER(PcmLoamFeatureParams),
                                                   C.POINTER(PcmLoamFeaturesResult), C.POINTER(C.POINTER(PcmLoamDeskew)), C.POINTER(PcmLoamCloudResult)]
    L.pcm_loam_default_submap_params.argtypes = [C.POINTER(PcmLoamSubmapParams)]
    L.pcm_loam_default_submap_params.restype = None
    L.pcm_loam_keyframe_add.argtypes = [vp, vp, C.c_double, vp, sz, vp, sz, sz, i32]
    L.pcm_loam_keyframe_set_poses.argtypes = [vp, i32, i32, vp]
    L.pcm_loam_keyframe_count.argtypes = [vp]
    L.pcm_loam_keyframe_clear.argtypes = [vp]
    L.pcm_loam_keyframe_get.argtypes = [vp, i32, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.pcm_loam_submap_update.argtypes = [vp, C.POINTER(PcmLoamSubmapParams), C.c_double, C.POINTER(PcmLoamSubmapResult)]
    L.pcm_loam_submap_near.argtypes = [vp, i32, i32, i32, C.c_float, vp, sz, C.POINTER(sz)]
    L.pcm_loam_submap_info.argtypes = [vp] * 6
    L.pcm_loam_default_sc_params.argtypes = [C.POINTER(PcmLoamScParams)]
    L.pcm_loam_default_sc_params.restype = None
    L.pcm_loam_sc_add.argtypes = [vp, C.POINTER(PcmLoamScParams), i32, i32, vp, sz, sz, i32, C.POINTER(PcmLoamScAddResult)]
    L.pcm_loam_sc_add_near.argtypes = [vp, C.POINTER(PcmLoamScParams), i32, i32, i32, C.c_float, C.POINTER(PcmLoamScAddResult)]
    L.pcm_loam_sc_put.argtypes = [vp, vp, i32, i32]
    L.pcm_loam_sc_get.argtypes = [vp, i32, vp, vp, vp]
    L.pcm_loam_sc_count.argtypes = [vp]
    L.pcm_loam_sc_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pcm_loam_sc_clear.argtypes = [vp]
    L.pcm_loam_sc_detect.argtypes = [vp, C.POINTER(PcmLoamScParams), C.POINTER(PcmLoamScResult)]
    L.pcm_loam_sc_distance.argtypes = [vp, C.POINTER(PcmLoamScParams), i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.pcm_loam_loop_detect_distance.argtypes = [vp, C.c_float, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.pcm_loam_submap_near_dev.argtypes = [vp, i32, i32, i32, C.c_float, vp, sz, i32, C.POINTER(sz)]
    L.pcm_loam_default_loop_params.argtypes = [C.POINTER(PcmLoamLoopParams)]
    L.pcm_loam_default_loop_params.restype = None
    L.pcm_loam_loop_verify.argtypes = [vp, C.POINTER(PcmLoamLoopParams), i32, i32, C.POINTER(PcmLoamLoopResult)]
    L.pcm_loam_loop_closure.argtypes = [vp, C.POINTER(PcmLoamLoopParams), C.c_float, C.c_double, C.c_double, C.POINTER(PcmLoamLoopResult)]
    L.pcm_loam_loop_verifier_exists.argtypes = [vp]
    L.pcm_loam_default_global_params.argtypes = [C.POINTER(PcmLoamGlobalParams)]
    L.pcm_loam_default_global_params.restype = None
    L.pcm_loam_global_keys.argtypes = [vp, C.POINTER(PcmLoamGlobalParams), vp, sz, C.POINTER(sz)]
    L.pcm_loam_global_map.argtypes = [vp, C.POINTER(PcmLoamGlobalParams), vp, sz, i32, C.POINTER(PcmLoamGlobalResult)]
    L.pcm_loam_map_export.argtypes = [vp, i32, i32, i32, vp, sz, i32, C.POINTER(sz)]
    L.pcm_loam_global_gather_ms.argtypes = [vp, C.POINTER(PcmLoamGlobalParams), i32, C.POINTER(C.c_float), vp, C.POINTER(sz), C.POINTER(C.c_float)]
    L.pcm_loam_default_dynmap_params.argtypes = [C.POINTER(PcmLoamDynmapParams)]
    L.pcm_loam_default_dynmap_params.restype = None
    L.pcm_loam_tile_add.argtypes = [vp, i32, vp, vp, sz, sz, i32]
    L.pcm_loam_tile_count.argtypes = [vp, i32]
    L.pcm_loam_tile_clear.argtypes = [vp]
    L.pcm_loam_dynmap_need_load.argtypes = [vp, C.POINTER(PcmLoamDynmapParams), vp]
    L.pcm_loam_dynmap_load.argtypes = [vp, C.POINTER(PcmLoamDynmapParams), vp, C.POINTER(PcmLoamDynmapLoadResult)]
    L.pcm_loam_dynmap_crop.argtypes = [vp, C.POINTER(PcmLoamDynmapParams), vp, C.POINTER(PcmLoamDynmapCropResult)]
    L.pcm_loam_dynmap_crop_batch.argtypes = [C.POINTER(vp), i32, C.POINTER(PcmLoamDynmapParams), vp, C.POINTER(PcmLoamDynmapCropResult)]
    L.pcm_loam_tile_share.argtypes = [vp, vp]
    L.pcm_loam_tile_share_count.argtypes = [vp]
    L.pcm_loam_dynmap_info.argtypes = [vp] * 5
    L.pcm_loam_dynmap_global.argtypes = [vp, vp, sz, C.POINTER(sz), i32]
    L.pcm_loam_default_tiles_params.argtypes = [C.POINTER(PcmLoamTilesParams)]
    L.pcm_loam_default_tiles_params.restype = None
    L.pcm_loam_tiles_build.argtypes = [vp, C.POINTER(PcmLoamTilesParams), i32, i32, C.POINTER(PcmLoamTilesResult)]
    L.pcm_loam_tiles_build_ms.argtypes = [vp, C.POINTER(PcmLoamTilesParams), i32, i32, C.POINTER(PcmLoamTilesResult), vp]
    L.pcm_loam_tile_info.argtypes = [vp, i32, i32, vp, vp, C.POINTER(sz)]
    L.pcm_loam_tile_get.argtypes = [vp, i32, i32, vp, sz, i32, C.POINTER(sz)]
    L.pcm_occ_default_params.argtypes = [C.POINTER(PcmOccParams)]
    L.pcm_occ_default_params.restype = None
    L.pcm_occ_reset.argtypes = [vp, C.POINTER(PcmOccParams)]
    L.pcm_occ_insert_scans.argtypes = [vp, vp, vp, vp, i32, sz, i32]
    L.pcm_occ_insert_keyframes.argtypes = [vp, i32, i32]
    L.pcm_occ_get_scan.argtypes = [vp, i32, vp, vp]
    L.pcm_occ_status.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int64)]
    L.pcm_occ_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_int64)]
    L.pcm_occ_get_map.argtypes = [vp, vp, sz]
    L.pcm_occ_get_pgm.argtypes = [vp, vp, sz]
    L.pcm_occ_get_counts.argtypes = [vp, vp, vp, sz]
    L.pcm_octo_default_params.argtypes = [C.POINTER(PcmOctoParams)]
    L.pcm_octo_default_params.restype = None
    L.pcm_octo_reset.argtypes = [vp, C.POINTER(PcmOctoParams)]
    L.pcm_octo_insert_scan.argtypes = [vp, vp, sz, vp, sz, sz, i32, vp, vp, C.POINTER(PcmOctoInsertResult)]
    L.pcm_octo_insert_keyframes.argtypes = [vp, i32, i32]
    L.pcm_octo_info.argtypes = [vp, C.POINTER(PcmOctoMapInfo)]
    L.pcm_octo_get_cells.argtypes = [vp, vp, sz, i32, C.POINTER(sz)]
    L.pcm_octo_get_occupied.argtypes = [vp, vp, sz, i32, C.POINTER(sz)]
    L.pcm_octo_project.argtypes = [vp, C.POINTER(PcmOctoGridInfo), vp, sz, i32]
    L.pcm_octo_get_pgm.argtypes = [vp, vp, sz, i32]
    L.pcm_octo_debug.argtypes = [vp, i32, i32]
    L.pcm_octo_phase_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.pcm_scan_default_fuse_params.argtypes = [C.POINTER(PcmScanFuseParams)]
    L.pcm_scan_default_fuse_params.restype = None
    L.pcm_scan_fuse.argtypes = [vp, C.POINTER(PcmScanSegment), i32, C.POINTER(PcmScanFuseParams), vp, sz, i32, C.POINTER(PcmScanFuseResult)]
    L.pcm_scan_fused.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.pcm_lidar_default_desc.argtypes = [i32, C.POINTER(PcmLidarDesc)]
    L.pcm_lidar_filter.argtypes = [vp, vp, sz, i32, C.POINTER(PcmLidarDesc), vp, sz, i32, C.POINTER(sz), C.POINTER(C.c_int)]
    L.pcm_lio_frame_begin_cloud.argtypes = [vp, vp, sz, i32, C.POINTER(PcmLidarDesc), C.c_float, vp, i32, C.POINTER(PcmLioState), C.POINTER(sz)]
    L.pcm_lio_default_update_params.argtypes = [C.POINTER(PcmLioUpdateParams)]
    L.pcm_lio_default_update_params.restype = None
    L.pcm_lio_update.argtypes = [vp, C.POINTER(PcmLioUpdateParams), C.POINTER(PcmLioFilterState), vp, C.POINTER(PcmLioUpdateResult)]
    L.pcm_lio_update_trace.argtypes = [vp, i32, C.POINTER(PcmLioFilterState), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp]
    L.pcm_lio_default_imu_state.argtypes = [C.POINTER(PcmLioImuState)]
    L.pcm_lio_default_imu_state.restype = None
    L.pcm_lio_imu_init.argtypes = [C.POINTER(PcmLioImuState), vp, i32, C.POINTER(PcmLioFilterState), vp]
    L.pcm_lio_propagate.argtypes = [vp, C.POINTER(PcmLioImuState), vp, i32, C.c_double, C.c_double, C.POINTER(PcmLioFilterState), vp, vp, i32, C.POINTER(C.c_int32)]
    L.pcm_lio_frame_world.argtypes = [vp, C.POINTER(PcmLioState), i32, vp, sz, i32, C.POINTER(sz)]
    L.pcm_lio_frame_body.argtypes = [vp, C.POINTER(PcmLioState), vp, sz, i32, C.POINTER(sz)]
    L.pcm_lio_frame_effect.argtypes = [vp, C.POINTER(PcmLioState), vp, sz, i32, C.POINTER(sz)]
    L.pcm_lio_map_append.argtypes = [vp, C.POINTER(PcmLioState), i32, i32, C.POINTER(PcmLioMapInfo)]
    L.pcm_lio_map_info_get.argtypes = [vp, C.POINTER(PcmLioMapInfo)]
    L.pcm_lio_map_get.argtypes = [vp, sz, sz, vp, i32]
    L.pcm_lio_map_clear.argtypes = [vp]
    L.pcm_lio_map_export.argtypes = [vp, C.c_float, C.c_double, C.c_double, vp, sz, i32, C.POINTER(sz)]
    L.pcm_icp_default_params.argtypes = [C.POINTER(PcmIcpParams)]
    L.pcm_icp_default_params.restype = None
    L.pcm_icp_set_params.argtypes = [vp, C.POINTER(PcmIcpParams)]
    L.pcm_icp_get_params.argtypes = [vp, C.POINTER(PcmIcpParams)]
    L.pcm_icp_last.argtypes = [vp, C.POINTER(PcmIcpInfo)]
    L.pcm_icp_trace.argtypes = [vp, i32, vp, vp, C.POINTER(C.c_int32)]
    L.pcm_loam_default_sc_loop_params.argtypes = [C.POINTER(PcmLoamScLoopParams)]
    L.pcm_loam_default_sc_loop_params.restype = None
    L.pcm_loam_sc_loop_verify.argtypes = [vp, C.POINTER(PcmLoamScLoopParams), i32, i32, C.POINTER(PcmLoamScLoopResult)]
    L.pcm_loam_sc_loop_closure.argtypes = [vp, C.POINTER(PcmLoamScLoopParams), C.POINTER(PcmLoamScLoopResult)]
    L.pcm_loam_sc_loop_verifier_exists.argtypes = [vp]
    _LIB = L
    return L
