"""ctypes binding of include/omni_hip.h plus thin numpy-friendly wrappers that mirror the reference classes.

Fails loudly: a missing ``lib/libomni_hip.so`` raises ImportError-like OSError from ``lib()``, a missing GPU raises
``OmniError`` from ``Context()``.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMNI_LIB") or os.path.join(_HERE, "lib", "libomni_hip.so")   # OMNI_LIB: A/B a second build of the same ABI

OK, ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_CAPACITY = 0, 1, 2, 3, 4
PREC_F32, PREC_F16, PREC_SPLIT = 0, 1, 2
STORE_F32, STORE_F16 = 0, 1
SCAN_F32, SCAN_F32_ROWS, SCAN_T16, SCAN_MQ, SCAN_MQ_MIRROR = range(5)      # omni_index_debug_scan
BF_OPENCV, BF_MUTUAL = 0, 1
ABI_VERSION = 2               # include/omni_hip.h OMNI_ABI_VERSION: checked when the library is loaded
SP_NUM_LAYERS = 12
SP_NUM_STAGES = 16
SP_LAYER_NAMES = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b",
                  "convPa", "convPb", "convDa", "convDb"]
VB_NAMES = ["hblock", "sblock", "mblock", "pw_mfma3", "valu"]      # include/omni_hip.h OMNI_VB_*
VLAD_STEM_NAMES = ["stem", "stem_b0", "layers"]                     # OMNI_VLAD_STEM_*
VLAD_KINDS = {"conv3x3": 0, "pw_relu6": 1, "dw3x3_relu6": 2, "pw_linear": 3, "pw_linear_res": 4}

# every symbol include/omni_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "omni_abi_version", "omni_last_error", "omni_ctx_create", "omni_ctx_create_priority", "omni_ctx_order_after", "omni_memcpy_d2h_async", "omni_ctx_destroy", "omni_ctx_sync", "omni_ctx_stream",
    "omni_ctx_device_info", "omni_ctx_mfma_ceiling", "omni_dev_alloc", "omni_dev_free", "omni_host_alloc", "omni_host_free", "omni_memcpy_h2d", "omni_memcpy_d2h", "omni_timer_start",
    "omni_timer_stop", "omni_sp_create", "omni_sp_destroy", "omni_sp_desc_dim", "omni_sp_image_size", "omni_sp_infer", "omni_sp_enqueue_dev",
    "omni_sp_fetch", "omni_sp_dev_outputs", "omni_sp_get_dense", "omni_sp_postprocess_dense", "omni_sp_debug_layer", "omni_sp_last_plan",
    "omni_sp_profile", "omni_sp_stage_name", "omni_sp_stage_flops", "omni_sp_stage_tiles_left_out", "omni_sp_mask_skip_plan", "omni_sp_mask_band_plan", "omni_vlad_create", "omni_vlad_destroy", "omni_vlad_set_precision", "omni_vlad_pack_block", "omni_sp_pack_constants",
    "omni_vlad_infer", "omni_vlad_enqueue_dev", "omni_vlad_fetch", "omni_vlad_dev_output", "omni_vlad_mask_skip_layers", "omni_vlad_debug_taps", "omni_vlad_debug_layer", "omni_vlad_block_paths", "omni_index_create",
    "omni_index_destroy", "omni_index_add", "omni_index_add_dev", "omni_index_ntotal", "omni_index_dim", "omni_index_reset", "omni_index_truncate", "omni_index_cert_stats",
    "omni_index_search", "omni_index_search_dev", "omni_index_search_prefix_dev", "omni_index_search_batch_prefix_dev", "omni_index_set_shard", "omni_topk_merge", "omni_index_last_scan_ms", "omni_index_debug_scan",
    "omni_index_save", "omni_index_load",
    "omni_trace_push", "omni_trace_pop", "omni_sp_set_perf", "omni_sp_last_stage_ms", "omni_bf_match", "omni_bf_match_multi", "omni_bf_match_batched_dev", "omni_config_count", "omni_config_describe", "omni_config_value", "omni_config_is_process_wide", "omni_cam_create", "omni_cam_create_mono", "omni_cam_destroy", "omni_cam_enqueue_dev", "omni_cam_enqueue_host", "omni_cam_enqueue_host_parts", "omni_cam_enqueue_fisheye_dev", "omni_cam_enqueue_fisheye_host", "omni_cam_get_input", "omni_cam_wait", "omni_cam_order_after", "omni_cam_set_active", "omni_cam_ready",
    "omni_shard_unique_id", "omni_shard_library_path", "omni_shard_create", "omni_shard_destroy", "omni_shard_ntotal", "omni_shard_preload_local", "omni_shard_step_batch_dev", "omni_shard_step_enqueue", "omni_shard_rows_consumed", "omni_shard_step_wait", "omni_shard_last_exchange_us",
    "omni_shard_search", "omni_flatten_create", "omni_flatten_destroy", "omni_flatten_out_bytes", "omni_flatten_enqueue_dev",
    "omni_resize_create", "omni_resize_destroy", "omni_resize_mode", "omni_resize_enqueue_dev", "omni_cam_enqueue_raw_dev", "omni_cam_enqueue_raw_host", "omni_cam_enqueue_raw_host_parts",
    "omni_landmarks_enqueue_dev", "omni_cam_set_stereo_model", "omni_cam_set_poses", "omni_cam_landmarks",
    "omni_landmarks_enqueue_dev_camera", "omni_cam_set_camera_model", "omni_camera_lift_host", "omni_camera_project_host",
    "omni_depth_landmarks_enqueue_dev", "omni_depth_landmarks_host", "omni_cam_set_depth_model", "omni_cam_set_depth_host", "omni_cam_set_depth_dev",
    "omni_homography_ransac_multi", "omni_bf_match_homography_multi", "omni_pnp_ransac_multi",
    "omni_jpeg_create", "omni_jpeg_destroy", "omni_jpeg_enqueue_dev", "omni_jpeg_header", "omni_jpeg_encode_host", "omni_cam_set_jpeg", "omni_cam_jpeg",
    "omni_jpegdec_create", "omni_jpegdec_destroy", "omni_jpegdec_enqueue_host", "omni_jpegdec_last_stats", "omni_jpegdec_last_ms", "omni_jpegdec_debug_buffers", "omni_jpegdec_classify",
    "omni_jpeg_decode_host", "omni_jpeg_decode_parallel_host", "omni_jpeg_decode_restart_parallel_host", "omni_jpegdec_last_chunks", "omni_jpeg_decode_plain_parallel_host", "omni_jpegdec_last_seam", "omni_jpegdec_debug_state_buffer",
    "omni_jpegdec_last_unstuff", "omni_jpegdec_debug_in_buffer", "omni_jpegdec_unstuff_dev", "omni_jpeg_unstuff_tile_bytes", "omni_jpeg_unstuff_host", "omni_jpeg_unstuff_tiled_host", "omni_jpeg_scan_end",
    "omni_cam_enqueue_jpeg_host", "omni_cam_jpegdec_status", "omni_cam_enqueue_fisheye_jpeg_host",
    "omni_pcafit_create", "omni_pcafit_destroy", "omni_pcafit_reset", "omni_pcafit_enqueue_rows_dev", "omni_sp_set_pcafit", "omni_pcafit_stats", "omni_pcafit_moments",
    "omni_pcafit_merge_host", "omni_pca_solve_host", "omni_pcafit_solve", "omni_pca_moments_host", "omni_pca_write_csv",
    "omni_wire_packet_capacity", "omni_wire_table_ints", "omni_wire_pack_enqueue_dev", "omni_wire_pack_host", "omni_cam_set_wire", "omni_cam_set_wire_meta", "omni_cam_wire",
    "omni_wire_image_capacity", "omni_wire_pack_image_enqueue_dev", "omni_wire_pack_image_host", "omni_cam_set_wire_image", "omni_cam_wire_image",
    "omni_rows_assemble_enqueue_dev", "omni_rows_assemble_host", "omni_memcpy_h2d_async",
    "omni_corr_assemble_host", "omni_corr_assemble_multi", "omni_bf_match_homography_corr_multi",
    "omni_pcm_create", "omni_pcm_destroy", "omni_pcm_size", "omni_pcm_capacity", "omni_pcm_add", "omni_pcm_adjacency", "omni_pcm_rows_host", "omni_pcm_max_clique_host", "omni_pcm_atan2",
    "omni_pgo_default_params", "omni_pgo_create", "omni_pgo_destroy", "omni_pgo_solve_multi", "omni_pgo_solve_host", "omni_pgo_residuals_host", "omni_pgo_plan_graph_host",
    "omni_pgo_sincos", "omni_pgo_normalize_angle", "omni_pgo_sum_host",
]
PGO_CONVERGED, PGO_MAX_ITERATIONS, PGO_NONFINITE, PGO_EMPTY = 0, 1, 2, 3      # include/omni_hip.h OMNI_PGO_*
PGO_MAX_POSES, PGO_MAX_EDGES, PGO_MAX_STARTS = 4096, 16384, 64
# include/omni_hip.h omni_pgo_edge and omni_pgo_stats as numpy records: a pose is x y z yaw
PGO_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("z", "<f8", (4,)), ("sqrt_inf", "<f8", (4,)), ("robust", "<i4"), ("reserved", "<i4")])
PGO_STATS_DTYPE = np.dtype([("initial_cost", "<f8"), ("final_cost", "<f8"), ("iterations", "<i4"), ("cg_iterations", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
PCM_FULL, PCM_MAX_ADD, PCM_DEFAULT_CAPACITY = 100, 64, 4096      # include/omni_hip.h OMNI_PCM_*
# include/omni_hip.h omni_pcm_edge as a numpy record: poses are xyz + quaternion wxyz
PCM_EDGE_DTYPE = np.dtype([("id", "<i8"), ("drone_a", "<i4"), ("drone_b", "<i4"), ("relative_pose", "<f8", (7,)), ("self_pose_a", "<f8", (7,)), ("self_pose_b", "<f8", (7,)),
                           ("arc_a", "<f8"), ("arc_b", "<f8"), ("pos_cov", "<f8", (3,)), ("ang_cov", "<f8", (3,))])
ROW_UNIT, ROW_STAGED, ROW_ZERO = 0, 1, 2      # include/omni_hip.h OMNI_ROW_*: where a row of a mixed detector batch comes from
WIRE_HEADER_BYTES, WIRE_LANDMARK_BYTES, WIRE_HEADER_OFFSET = 16545, 324, 3      # include/omni_hip.h OMNI_WIRE_*
WIRE_CHANNELS = ("VIOKF_HEADER", "VIOKF_LANDMARKS")                            # packet 0 of an image / every other packet
WIRE_IMAGE_CHANNEL, WIRE_IMAGE_HEAD_BYTES, WIRE_IMAGE_OFFSET = "SWARM_LOOP_IMG_DES", 177, 3      # the whole descriptor (csrc/wire_plan.h whole_*)
JPEGDEC_OK, JPEGDEC_HOST, JPEGDEC_UNSUPPORTED, JPEGDEC_CORRUPT = 0, 1, 2, 3      # include/omni_hip.h OMNI_JPEGDEC_*
JPEGDEC_GUARD_BYTES = 256
JPEG_OK, JPEG_TRUNCATED, JPEG_HEADER_BYTES = 0, 1, 328      # include/omni_hip.h OMNI_JPEG_*
HG_UNFILTERED, HG_OK, HG_NO_MODEL, HG_HOST = 0, 1, 2, 3     # include/omni_hip.h OMNI_HG_*: the status of one pair's homography RANSAC
PNP_SKIPPED, PNP_OK, PNP_NO_MODEL, PNP_HOST = 0, 1, 2, 3    # include/omni_hip.h OMNI_PNP_*: the status of one candidate's PnP RANSAC
PNP_MAX_POINTS, PNP_MAX_ITERS = 2048, 1000


class OmniError(RuntimeError):
    pass


class _SpWeights(C.Structure):
    _fields_ = [("weight", C.POINTER(C.c_float) * SP_NUM_LAYERS), ("bias", C.POINTER(C.c_float) * SP_NUM_LAYERS)]


class _VladLayer(C.Structure):
    _fields_ = [("kind", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("stride", C.c_int),
                ("weight", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float))]


class PcmParams(C.Structure):     # include/omni_hip.h omni_pcm_params
    _fields_ = [("pcm_thres", C.c_double), ("pos_covariance_per_meter", C.c_double), ("yaw_covariance_per_meter", C.c_double)]


class PgoParams(C.Structure):     # include/omni_hip.h omni_pgo_params
    _fields_ = [("max_iterations", C.c_int32), ("max_cg_iterations", C.c_int32), ("max_lambda_retries", C.c_int32), ("reserved", C.c_int32),
                ("initial_lambda", C.c_double), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double), ("cg_tolerance", C.c_double)]


class CorrCand(C.Structure):      # include/omni_hip.h omni_corr_cand
    _fields_ = [(n, C.c_int32) for n in ("pair_first", "pair_count", "min_match_pre_dir", "min_direction_loop", "min_loop_num", "init_mode_min_loop_num", "init_mode", "reserved")]


class CorrIO(C.Structure):        # include/omni_hip.h omni_corr_io
    _fields_ = [(n, C.c_int32) for n in ("n_cands", "n_pairs", "max_n", "cap")] + \
               [(n, C.c_void_p) for n in ("cands", "q_idx", "t_idx", "n_matches", "q_flags", "n_flags", "nq", "nt", "mask", "hg_status", "q_3d", "t_norm", "dq_old", "X", "u",
                                          "n_corr", "matched_dir_count", "gate", "new_idx", "old_idx", "n_pair_corr")]


class _CamResult(C.Structure):
    _fields_ = [("n_dirs", C.c_int), ("max_num", C.c_int), ("desc_dim", C.c_int), ("global_dim", C.c_int),
                ("kps_xy", C.POINTER(C.c_float)), ("n_kps", C.POINTER(C.c_int)), ("desc", C.POINTER(C.c_float)),
                ("scores", C.POINTER(C.c_float)), ("global_desc", C.POINTER(C.c_float)), ("match_up", C.POINTER(C.c_int)),
                ("match_down", C.POINTER(C.c_int)), ("match_dist", C.POINTER(C.c_float)), ("n_matches", C.POINTER(C.c_int)), ("n_images", C.c_int)]


STEREO_MAX_DIRS = 8           # OMNI_STEREO_MAX_DIRS


class StereoModel(C.Structure):
    """omni_stereo_model: the pinhole model, the accept rule and the per-direction extrinsics (xyz + quaternion wxyz) of the stereo-landmark stage"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("triangle_thres", C.c_double),
                ("accept_min_3d_pts", C.c_int), ("dirs_per_keyframe", C.c_int),
                ("up_extrinsic", (C.c_double * 7) * STEREO_MAX_DIRS), ("down_extrinsic", (C.c_double * 7) * STEREO_MAX_DIRS)]


def stereo_model(fx, fy, cx, cy, triangle_thres, accept_min_3d_pts, up_extrinsics, down_extrinsics) -> StereoModel:
    """up_extrinsics / down_extrinsics: [dirs][7] (body -> camera of every direction of a key frame)"""
    up, down = np.asarray(up_extrinsics, np.float64).reshape(-1, 7), np.asarray(down_extrinsics, np.float64).reshape(-1, 7)
    if not (1 <= len(up) <= STEREO_MAX_DIRS and len(down) == len(up)):
        raise ValueError(f"stereo_model: {len(up)} up and {len(down)} down extrinsics, 1..{STEREO_MAX_DIRS} of each")
    m = StereoModel(fx, fy, cx, cy, triangle_thres, int(accept_min_3d_pts), len(up))
    for d in range(len(up)):
        m.up_extrinsic[d][:] = up[d].tolist()
        m.down_extrinsic[d][:] = down[d].tolist()
    return m


CAMERA_PINHOLE, CAMERA_MEI = 0, 1      # OMNI_CAMERA_*
CAMERA_TYPES = {"PINHOLE": CAMERA_PINHOLE, "MEI": CAMERA_MEI}


class CameraModel(C.Structure):
    """omni_camera_model: the lens of the lift (csrc/camera_plan.h) -- camodocal's PINHOLE with distortion coefficients, or MEI (xi; the stereo model's
    fx fy cx cy then hold gamma1 gamma2 u0 v0).  All zeros: the ideal pinhole."""
    _fields_ = [("type", C.c_int), ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("xi", C.c_double)]


def camera_model(type=CAMERA_PINHOLE, k1=0.0, k2=0.0, p1=0.0, p2=0.0, xi=0.0) -> CameraModel:
    """type: CAMERA_PINHOLE / CAMERA_MEI or their names; nothing is checked here -- the entry points refuse what csrc/camera_plan.h's check refuses"""
    if isinstance(type, str):
        if type.upper() not in CAMERA_TYPES:
            raise ValueError(f"camera_model: type {type!r}, one of {sorted(CAMERA_TYPES)}")
        type = CAMERA_TYPES[type.upper()]
    return CameraModel(int(type), float(k1), float(k2), float(p1), float(p2), float(xi))


def camera_lift_host(camera, intrinsics4, xy) -> np.ndarray:
    """omni_camera_lift_host (no GPU): pixels xy [n][2] float32 -> lifted and divided by z, [n][2] float64; camera None: the ideal pinhole"""
    xy = _f32(xy).reshape(-1, 2)
    k = np.ascontiguousarray(intrinsics4, np.float64).reshape(4)
    out = np.zeros((len(xy), 2), np.float64)
    _check(lib().omni_camera_lift_host(C.byref(camera) if camera is not None else None, k.ctypes.data, xy.ctypes.data, len(xy), out.ctypes.data))
    return out


def camera_project_host(camera, intrinsics4, xyz) -> np.ndarray:
    """omni_camera_project_host (no GPU): the forward model, points xyz [n][3] in the camera's frame -> pixels [n][2] float64"""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    k = np.ascontiguousarray(intrinsics4, np.float64).reshape(4)
    out = np.zeros((len(xyz), 2), np.float64)
    _check(lib().omni_camera_project_host(C.byref(camera) if camera is not None else None, k.ctypes.data, xyz.ctypes.data, len(xyz), out.ctypes.data))
    return out


class DepthModel(C.Structure):
    """omni_depth_model: the intrinsics, the depth window, the accept rule, the depth images' size and the extrinsic (xyz + quaternion wxyz) of the depth-landmark stage"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("depth_near", C.c_double), ("depth_far", C.c_double),
                ("accept_min_3d_pts", C.c_int), ("depth_width", C.c_int), ("depth_height", C.c_int), ("extrinsic", C.c_double * 7)]


def depth_model(fx, fy, cx, cy, depth_near, depth_far, accept_min_3d_pts, depth_width, depth_height, extrinsic=(0, 0, 0, 1, 0, 0, 0)) -> DepthModel:
    e = np.asarray(extrinsic, np.float64).reshape(-1)
    if e.shape != (7,):
        raise ValueError(f"depth_model: an extrinsic of {e.size} numbers, xyz + quaternion wxyz")
    m = DepthModel()
    m.fx, m.fy, m.cx, m.cy, m.depth_near, m.depth_far = float(fx), float(fy), float(cx), float(cy), float(depth_near), float(depth_far)
    m.accept_min_3d_pts, m.depth_width, m.depth_height = int(accept_min_3d_pts), int(depth_width), int(depth_height)
    m.extrinsic[:] = [float(v) for v in e]
    return m


def depth_landmarks_host(model: DepthModel, poses7, kps_xy, n_kps, depth, have=None, camera=None, depth_stride: int = 0) -> dict:
    """omni_depth_landmarks_host: csrc/depth_plan.h on the host, no GPU.  kps_xy [N][M][2], n_kps [N], poses7 [N][7], depth [N][depth_height][stride] u16
    (depth_stride 0: the array's last dimension), have [N] or None (all)"""
    kps_xy, n_kps = _f32(kps_xy), np.ascontiguousarray(n_kps, np.int32)
    N, M = n_kps.shape[0], kps_xy.shape[1]
    p = np.ascontiguousarray(poses7, np.float64).reshape(-1, 7)
    d = np.ascontiguousarray(depth, np.uint16)
    hv = np.ascontiguousarray(have, np.uint8) if have is not None else None
    assert p.shape == (N, 7) and kps_xy.shape == (N, M, 2) and (hv is None or hv.shape == (N,))
    outs = np.zeros((N, M, 2), np.float32), np.zeros((N, M, 3), np.float32), np.zeros((N, M), np.uint8), np.zeros(N, np.int32)
    _check(lib().omni_depth_landmarks_host(C.byref(model), C.byref(camera) if camera is not None else None, p.ctypes.data, N, M, kps_xy.ctypes.data, n_kps.ctypes.data,
                                           d.ctypes.data, depth_stride or d.shape[-1], hv.ctypes.data if hv is not None else None, *[o.ctypes.data for o in outs]))
    return dict(zip(("norm2d", "landmarks_3d", "landmarks_flag", "count_3d"), outs))


class WireImageMeta(C.Structure):
    """omni_wire_image_meta: what a key frame's image sends besides the unit's arrays (stamp, ids, direction, the two poses as xyz + quaternion wxyz)"""
    _fields_ = [("timestamp", C.c_double), ("frame_id", C.c_int64), ("drone_id", C.c_int32), ("direction", C.c_int32), ("prevent_adding_db", C.c_int32),
                ("reserved", C.c_int32), ("pose_drone", C.c_double * 7), ("camera_extrinsic", C.c_double * 7)]


WIRE_META_DTYPE = np.dtype([("timestamp", "<f8"), ("frame_id", "<i8"), ("drone_id", "<i4"), ("direction", "<i4"), ("prevent_adding_db", "<i4"), ("reserved", "<i4"),
                            ("pose_drone", "<f8", (7,)), ("camera_extrinsic", "<f8", (7,))])      # the same 144 bytes as a numpy record


def wire_packet_capacity(max_num: int) -> int:
    return int(lib().omni_wire_packet_capacity(max_num))


def wire_table_ints(max_num: int) -> int:
    return int(lib().omni_wire_table_ints(max_num))


def _wire_inputs(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta):
    kps_xy, n_kps = _f32(kps_xy), np.ascontiguousarray(n_kps, np.int32)
    N, M = n_kps.shape[0], kps_xy.shape[1]
    ins = [kps_xy, n_kps, _f32(desc), _f32(norm2d), _f32(l3d), np.ascontiguousarray(flag, np.uint8), _f32(global_desc), np.ascontiguousarray(meta, WIRE_META_DTYPE)]
    assert kps_xy.shape == (N, M, 2) and ins[2].shape[:2] == (N, M) and ins[3].shape == (N, M, 2) and ins[4].shape == (N, M, 3) and ins[5].shape == (N, M)
    assert ins[6].shape[0] == N and ins[7].shape == (N,)
    return N, M, ins


def wire_pack_host(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta, send_all_features: bool = False, fill: int = 0):
    """omni_wire_pack_host: csrc/wire_plan.h on the host, no GPU.  kps_xy [N][M][2], n_kps [N], desc [N][M][64], norm2d [N][M][2], l3d [N][M][3], flag [N][M] u8,
    global_desc [N][4096], meta [N] records of WIRE_META_DTYPE -> (packets [N][capacity] u8 pre-filled with `fill`, table [N][table_ints] i32)"""
    N, M, ins = _wire_inputs(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta)
    out = np.full((N, wire_packet_capacity(M)), fill, np.uint8)
    table = np.zeros((N, wire_table_ints(M)), np.int32)
    _check(lib().omni_wire_pack_host(N, M, ins[2].shape[2], ins[6].shape[1], int(bool(send_all_features)), *[a.ctypes.data for a in ins], out.ctypes.data, table.ctypes.data))
    return out, table


def wire_image_capacity(max_num: int, jpeg_capacity: int = 0) -> int:
    return int(lib().omni_wire_image_capacity(max_num, jpeg_capacity))


def _wire_jpeg_inputs(N, jpeg, jpeg_sizes, jpeg_status):
    """the JPEG rows of a whole descriptor: (with_image, [jpeg [N][capacity] u8, sizes [N] i32, status [N] i32] or [], capacity)"""
    if jpeg is None:
        assert jpeg_sizes is None and jpeg_status is None
        return 0, [], 0
    jp = np.ascontiguousarray(jpeg, np.uint8)
    js, jt = np.ascontiguousarray(jpeg_sizes, np.int32), np.ascontiguousarray(jpeg_status, np.int32)
    assert jp.ndim == 2 and jp.shape[0] == N and js.shape == (N,) and jt.shape == (N,)
    return 1, [jp, js, jt], jp.shape[1]


def wire_pack_image_host(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta, jpeg=None, jpeg_sizes=None, jpeg_status=None, width: int = 0, height: int = 0,
                         with_features: bool = True, fill: int = 0):
    """omni_wire_pack_image_host: the whole descriptor of csrc/wire_plan.h on the host, no GPU.  The arrays of wire_pack_host plus jpeg [N][capacity] u8, jpeg_sizes [N],
    jpeg_status [N] (all three None: with_image 0) -> (packets [N][wire_image_capacity] u8 pre-filled with `fill`, sizes [N][2] i32 = (offset, size))"""
    N, M, ins = _wire_inputs(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta)
    with_image, jp, cap = _wire_jpeg_inputs(N, jpeg, jpeg_sizes, jpeg_status)
    out = np.full((N, wire_image_capacity(M, cap)), fill, np.uint8)
    sizes = np.full((N, 2), -1, np.int32)
    _check(lib().omni_wire_pack_image_host(N, M, ins[2].shape[2], ins[6].shape[1], int(bool(with_features)), with_image, *[a.ctypes.data for a in ins],
                                           *([a.ctypes.data for a in jp] or [None] * 3), cap, width, height, out.ctypes.data, sizes.ctypes.data))
    return out, sizes


def _rows_inputs(table, unit_rows, staged_rows, dim):
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 2)      # omni_row_source: (source, index) per output row
    unit_rows, staged_rows = _f32(unit_rows).reshape(-1, dim if dim > 0 else 1), _f32(staged_rows).reshape(-1, dim if dim > 0 else 1)
    return table, unit_rows, staged_rows


def rows_assemble_host(table, unit_rows, staged_rows, dim: int, n_rows: int = None) -> np.ndarray:
    """omni_rows_assemble_host: csrc/rows_plan.h on the host, no GPU.  table [n_rows][2] i32 = (ROW_*, index), unit_rows [U][dim], staged_rows [S][dim]
    -> [n_rows][dim] f32, bit for bit"""
    table, unit_rows, staged_rows = _rows_inputs(table, unit_rows, staged_rows, dim)
    n_rows = len(table) if n_rows is None else n_rows
    out = np.empty((max(n_rows, 0), max(dim, 0)), np.float32)
    _check(lib().omni_rows_assemble_host(n_rows, dim, table.ctypes.data, unit_rows.ctypes.data if len(unit_rows) else None, len(unit_rows),
                                         staged_rows.ctypes.data if len(staged_rows) else None, len(staged_rows), out.ctypes.data))
    return out


def wire_packets(packets_row: np.ndarray, table_row: np.ndarray):
    """one image's packets as (channel, bytes) in sending order, cut out of its buffer through its table"""
    return [(WIRE_CHANNELS[min(k, 1)], packets_row[table_row[2 + 2 * k]:table_row[2 + 2 * k] + table_row[3 + 2 * k]].tobytes()) for k in range(int(table_row[0]))]


class _CamLandmarks(C.Structure):
    _fields_ = [("n_images", C.c_int), ("n_dirs", C.c_int), ("max_num", C.c_int), ("norm2d", C.POINTER(C.c_float)), ("landmarks_3d", C.POINTER(C.c_float)),
                ("landmarks_flag", C.POINTER(C.c_uint8)), ("count_3d", C.POINTER(C.c_int))]


class _CamJpeg(C.Structure):
    _fields_ = [("n_images", C.c_int), ("capacity", C.c_int64), ("bytes", C.POINTER(C.c_uint8)), ("sizes", C.POINTER(C.c_int)), ("status", C.POINTER(C.c_int))]


class _CamWire(C.Structure):
    _fields_ = [("n_images", C.c_int), ("max_num", C.c_int), ("table_ints", C.c_int), ("capacity", C.c_int64), ("packets", C.POINTER(C.c_uint8)), ("table", C.POINTER(C.c_int))]


class _CamWireImage(C.Structure):
    _fields_ = [("n_images", C.c_int), ("with_features", C.c_int), ("with_image", C.c_int), ("capacity", C.c_int64), ("packets", C.POINTER(C.c_uint8)), ("sizes", C.POINTER(C.c_int))]


class _VladWeights(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("layers", C.POINTER(_VladLayer)), ("n_clusters", C.c_int), ("feat_dim", C.c_int),
                ("out_dim", C.c_int), ("assign_w", C.POINTER(C.c_float)), ("assign_b", C.POINTER(C.c_float)),
                ("clusters", C.POINTER(C.c_float)), ("fc_w", C.POINTER(C.c_float)), ("fc_b", C.POINTER(C.c_float))]


_lib = None
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_i64p = C.POINTER(C.c_int64)
_u8p = C.POINTER(C.c_uint8)
_vp = C.c_void_p


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"(or `make -C omni-swarm_amd`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)

    def sig(name, res, args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args

    sig("omni_abi_version", C.c_int, [])
    sig("omni_last_error", C.c_char_p, [])
    sig("omni_ctx_create", _vp, [C.c_int])
    sig("omni_ctx_create_priority", _vp, [C.c_int, C.c_int])
    sig("omni_ctx_order_after", C.c_int, [_vp, _vp])
    sig("omni_memcpy_d2h_async", C.c_int, [_vp, _vp, _vp, C.c_size_t])
    sig("omni_ctx_destroy", None, [_vp])
    sig("omni_ctx_sync", C.c_int, [_vp])
    sig("omni_ctx_stream", _vp, [_vp])
    sig("omni_ctx_device_info", C.c_int, [_vp, C.c_char_p, C.c_int, _ip, _ip, C.POINTER(C.c_size_t)])
    sig("omni_ctx_mfma_ceiling", C.c_int, [_vp, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)])
    sig("omni_dev_alloc", _vp, [_vp, C.c_size_t])
    sig("omni_dev_free", C.c_int, [_vp, _vp])
    sig("omni_host_alloc", _vp, [C.c_size_t])
    sig("omni_host_free", C.c_int, [_vp])
    sig("omni_memcpy_h2d", C.c_int, [_vp, _vp, _vp, C.c_size_t])
    sig("omni_memcpy_d2h", C.c_int, [_vp, _vp, _vp, C.c_size_t])
    sig("omni_timer_start", C.c_int, [_vp])
    sig("omni_timer_stop", C.c_int, [_vp, _fp])
    sig("omni_sp_create", _vp, [_vp, C.POINTER(_SpWeights), _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                C.c_int, C.c_int])
    sig("omni_sp_destroy", None, [_vp])
    sig("omni_sp_desc_dim", C.c_int, [_vp])
    sig("omni_sp_infer", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _fp, _ip, _fp, _fp])
    sig("omni_sp_enqueue_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int])
    sig("omni_sp_fetch", C.c_int, [_vp, C.c_int, _fp, _ip, _fp, _fp])
    sig("omni_sp_dev_outputs", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)])
    sig("omni_sp_get_dense", C.c_int, [_vp, C.c_int, _fp, _fp])
    sig("omni_sp_postprocess_dense", C.c_int, [_vp, _fp, _fp, C.c_int, _fp, _ip, _fp, _fp])
    sig("omni_sp_debug_layer", C.c_int, [_vp, C.c_char_p, C.c_int, _fp, _ip, _ip, _ip])
    sig("omni_sp_last_plan", C.c_int, [_vp])
    sig("omni_sp_profile", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _fp])
    sig("omni_sp_stage_name", C.c_char_p, [C.c_int])
    sig("omni_sp_stage_flops", C.c_double, [_vp, C.c_int])
    sig("omni_sp_stage_tiles_left_out", C.c_double, [_vp, C.c_int])
    sig("omni_sp_mask_skip_plan", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)])
    sig("omni_sp_mask_band_plan", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)])
    sig("omni_vlad_create", _vp, [_vp, C.POINTER(_VladWeights), C.c_int, C.c_int, C.c_int])
    sig("omni_vlad_destroy", None, [_vp])
    sig("omni_vlad_set_precision", C.c_int, [_vp, C.c_int])
    sig("omni_sp_pack_constants", C.c_int64, [C.c_int, _fp, _fp, C.c_int, _vp, C.c_int64, C.POINTER(C.c_float)])
    sig("omni_vlad_pack_block", C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _vp, C.c_int64])
    sig("omni_vlad_infer", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _fp])
    sig("omni_vlad_enqueue_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int])
    sig("omni_vlad_fetch", C.c_int, [_vp, C.c_int, _fp])
    sig("omni_vlad_dev_output", C.c_int, [_vp, C.POINTER(_vp)])
    sig("omni_vlad_mask_skip_layers", C.c_int, [_vp, C.POINTER(C.c_double), C.c_int])
    sig("omni_vlad_debug_taps", C.c_int, [_vp, C.c_int])
    sig("omni_vlad_debug_layer", C.c_int, [_vp, C.c_char_p, C.c_int, _fp, _ip, _ip, _ip])
    sig("omni_vlad_block_paths", C.c_int, [_vp, _ip, C.c_int])
    sig("omni_index_create", _vp, [_vp, C.c_int, C.c_int, C.c_int64])
    sig("omni_index_destroy", None, [_vp])
    sig("omni_index_add", C.c_int, [_vp, C.c_int64, _fp])
    sig("omni_index_add_dev", C.c_int, [_vp, C.c_int64, _vp])
    sig("omni_index_ntotal", C.c_int64, [_vp])
    sig("omni_index_reset", C.c_int, [_vp])
    sig("omni_index_truncate", C.c_int, [_vp, C.c_int64])
    sig("omni_index_cert_stats", C.c_int, [_vp, _i64p, _i64p])
    sig("omni_index_dim", C.c_int, [_vp])
    sig("omni_sp_image_size", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)])
    sig("omni_index_search", C.c_int, [_vp, C.c_int, _fp, C.c_int, _fp, _i64p])
    sig("omni_index_search_dev", C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp])
    sig("omni_index_search_prefix_dev", C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int64, _vp, _vp])
    sig("omni_index_search_batch_prefix_dev", C.c_int, [_vp, C.c_int, _vp, _i64p, C.c_int, _i64p, _vp, _vp])
    sig("omni_index_set_shard", C.c_int, [_vp, C.c_int, C.c_int])
    sig("omni_topk_merge", C.c_int, [C.c_int, C.c_int, C.c_int, _fp, _i64p, C.c_int, _fp, _i64p])
    sig("omni_index_last_scan_ms", C.c_int, [_vp, _fp])
    sig("omni_index_debug_scan", C.c_int, [_vp, C.c_int, C.c_int, _fp, C.c_int64, _i64p, C.c_int, C.c_void_p])
    sig("omni_index_save", C.c_int, [_vp, C.c_char_p])
    sig("omni_index_load", C.c_int, [_vp, C.c_char_p])
    sig("omni_bf_match", C.c_int, [_vp, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _ip, _ip, _fp, _ip])
    sig("omni_bf_match_multi", C.c_int, [_vp, C.c_int, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, C.c_int, C.c_int, C.c_int, _ip, _ip, _fp, _ip])
    sig("omni_bf_match_batched_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp, C.c_int64,
                                               _vp, _vp, _vp, _vp, _vp])
    sig("omni_cam_create", _vp, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("omni_cam_create_mono", _vp, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int])
    sig("omni_cam_destroy", None, [_vp])
    sig("omni_cam_enqueue_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int])
    sig("omni_trace_push", None, [C.c_char_p])
    sig("omni_config_is_process_wide", C.c_int, [C.c_int])
    sig("omni_sp_set_perf", C.c_int, [_vp, C.c_int])
    sig("omni_sp_last_stage_ms", C.c_int, [_vp, _vp])
    sig("omni_trace_pop", None, [])
    sig("omni_cam_enqueue_host", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("omni_cam_enqueue_host_parts", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("omni_cam_enqueue_fisheye_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("omni_cam_enqueue_fisheye_host", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("omni_cam_get_input", C.c_int, [_vp, _vp, C.c_int64])
    sig("omni_cam_enqueue_raw_dev", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int])
    sig("omni_cam_enqueue_raw_host", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int])
    sig("omni_cam_enqueue_raw_host_parts", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int])
    sig("omni_cam_wait", C.c_int, [_vp, C.POINTER(_CamResult)])
    sig("omni_homography_ransac_multi", C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, _ip, _ip, _vp, C.POINTER(C.c_double), _ip])
    sig("omni_pnp_ransac_multi", C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, _ip, _ip, _ip, _vp, C.POINTER(C.c_double), _ip])
    sig("omni_bf_match_homography_multi", C.c_int, [_vp, C.c_int, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, C.c_int, C.c_int, C.c_int, C.POINTER(_fp), C.POINTER(_fp),
                                                  C.POINTER(_vp), _ip, _ip, _ip, _fp, _ip, _ip, _ip, _vp, C.POINTER(C.c_double), _ip, _ip])
    sig("omni_landmarks_enqueue_dev", C.c_int, [_vp, C.POINTER(StereoModel), _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    sig("omni_cam_set_stereo_model", C.c_int, [_vp, C.POINTER(StereoModel)])
    sig("omni_landmarks_enqueue_dev_camera", C.c_int, [_vp, C.POINTER(StereoModel), C.POINTER(CameraModel), _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    sig("omni_cam_set_camera_model", C.c_int, [_vp, C.POINTER(CameraModel)])
    sig("omni_camera_lift_host", C.c_int, [C.POINTER(CameraModel), _vp, _vp, C.c_int, _vp])
    sig("omni_camera_project_host", C.c_int, [C.POINTER(CameraModel), _vp, _vp, C.c_int, _vp])
    sig("omni_depth_landmarks_enqueue_dev", C.c_int, [_vp, C.POINTER(DepthModel), C.POINTER(CameraModel), _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp])
    sig("omni_depth_landmarks_host", C.c_int, [C.POINTER(DepthModel), C.POINTER(CameraModel), _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp])
    sig("omni_cam_set_depth_model", C.c_int, [_vp, C.POINTER(DepthModel), C.POINTER(CameraModel)])
    sig("omni_cam_set_depth_host", C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int])
    sig("omni_cam_set_depth_dev", C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int])
    sig("omni_cam_set_poses", C.c_int, [_vp, C.POINTER(C.c_double), C.c_int])
    sig("omni_cam_landmarks", C.c_int, [_vp, C.POINTER(_CamLandmarks)])
    sig("omni_rows_assemble_enqueue_dev", C.c_int, [_vp, C.c_int64, C.c_int, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp])
    sig("omni_rows_assemble_host", C.c_int, [C.c_int64, C.c_int, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp])
    sig("omni_memcpy_h2d_async", C.c_int, [_vp, _vp, _vp, C.c_size_t])
    sig("omni_corr_assemble_host", C.c_int, [C.POINTER(CorrIO)])
    sig("omni_corr_assemble_multi", C.c_int, [_vp, C.POINTER(CorrIO), _fp])
    sig("omni_bf_match_homography_corr_multi", C.c_int, [_vp, C.c_int, C.POINTER(_fp), _ip, C.POINTER(_fp), _ip, C.c_int, C.c_int, C.c_int, C.POINTER(_fp), C.POINTER(_fp),
                                                       C.POINTER(_vp), _ip, C.c_int, _vp, C.c_int, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(C.c_double),
                                                       _ip, _ip, _fp, _ip, _ip, _ip, _vp, C.POINTER(C.c_double), _ip, _ip, _fp, _fp, _ip, _ip, _ip, _ip, _ip, _ip])
    sig("omni_wire_packet_capacity", C.c_int64, [C.c_int])
    sig("omni_wire_table_ints", C.c_int, [C.c_int])
    sig("omni_wire_pack_enqueue_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    sig("omni_wire_pack_host", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    sig("omni_wire_image_capacity", C.c_int64, [C.c_int, C.c_int64])
    sig("omni_wire_pack_image_enqueue_dev", C.c_int, [_vp] + [C.c_int] * 6 + [_vp] * 11 + [C.c_int64, C.c_int, C.c_int, _vp, _vp])
    sig("omni_wire_pack_image_host", C.c_int, [C.c_int] * 6 + [_vp] * 11 + [C.c_int64, C.c_int, C.c_int, _vp, _vp])
    sig("omni_jpeg_create", _vp, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64])
    sig("omni_jpeg_destroy", None, [_vp])
    sig("omni_jpeg_enqueue_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp])
    sig("omni_jpeg_header", C.c_int, [C.c_int, C.c_int, C.c_int, _vp])
    sig("omni_jpeg_encode_host", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _i64p, _ip])
    sig("omni_cam_set_jpeg", C.c_int, [_vp, C.c_int, C.c_int64])
    sig("omni_cam_jpeg", C.c_int, [_vp, C.POINTER(_CamJpeg)])
    sig("omni_cam_set_wire", C.c_int, [_vp, C.c_int, C.c_int])
    sig("omni_cam_set_wire_meta", C.c_int, [_vp, _vp, C.c_int])
    sig("omni_cam_wire", C.c_int, [_vp, C.POINTER(_CamWire)])
    sig("omni_cam_set_wire_image", C.c_int, [_vp, C.c_int, C.c_int])
    sig("omni_cam_wire_image", C.c_int, [_vp, C.POINTER(_CamWireImage)])
    sig("omni_jpegdec_create", _vp, [_vp, C.c_int, C.c_int, C.c_int, C.c_int64])
    sig("omni_jpegdec_destroy", None, [_vp])
    sig("omni_jpegdec_enqueue_host", C.c_int, [_vp, C.POINTER(_vp), _i64p, C.c_int, _vp, C.c_int, _vp])
    sig("omni_jpegdec_last_stats", C.c_int, [_vp, _ip, _ip, _ip])
    sig("omni_jpegdec_last_ms", C.c_int, [_vp, _fp, _fp, _i64p])
    sig("omni_jpegdec_debug_buffers", C.c_int, [_vp, C.POINTER(_vp), _i64p, C.POINTER(_vp), _i64p])
    sig("omni_jpegdec_classify", C.c_int, [_vp, C.c_int64, _ip, _ip])
    sig("omni_jpeg_decode_host", C.c_int, [_vp, C.c_int64, _vp, C.c_int, _ip, _ip, _ip])
    sig("omni_cam_enqueue_jpeg_host", C.c_int, [_vp, _vp, C.POINTER(_vp), _i64p, C.POINTER(_vp), _i64p, C.c_int])
    sig("omni_cam_jpegdec_status", C.c_int, [_vp, _ip, C.c_int])
    sig("omni_cam_enqueue_fisheye_jpeg_host", C.c_int, [_vp, _vp, _vp, C.POINTER(_vp), _i64p, C.POINTER(_vp), _i64p, C.c_int, C.c_int, C.c_int])
    sig("omni_jpeg_decode_parallel_host", C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, _ip, _ip, _ip, _ip])
    sig("omni_jpeg_decode_restart_parallel_host", C.c_int, [_vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _ip, _ip, _ip, _ip])
    sig("omni_jpegdec_last_chunks", C.c_int, [_vp, _ip])
    sig("omni_jpeg_decode_plain_parallel_host", C.c_int, [_vp, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _ip, _ip, _ip, _ip])
    sig("omni_jpegdec_last_seam", C.c_int, [_vp, _ip, _ip])
    sig("omni_jpegdec_debug_state_buffer", C.c_int, [_vp, C.POINTER(_vp), _i64p])
    sig("omni_jpegdec_last_unstuff", C.c_int, [_vp, _ip, _i64p, _i64p])
    sig("omni_jpegdec_debug_in_buffer", C.c_int, [_vp, C.POINTER(_vp), _i64p])
    sig("omni_jpegdec_unstuff_dev", C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _i64p])
    sig("omni_jpeg_unstuff_tile_bytes", C.c_int, [])
    sig("omni_jpeg_unstuff_host", C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _i64p, _i64p, C.c_int64, _i64p])
    sig("omni_jpeg_unstuff_tiled_host", C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _i64p, _i64p, C.c_int64, _i64p, _i64p, _i64p, _vp, C.c_int64, _i64p])
    sig("omni_jpeg_scan_end", C.c_int64, [_vp, C.c_int64, C.c_int64])
    sig("omni_cam_order_after", C.c_int, [_vp, _vp, C.c_int])
    sig("omni_cam_set_active", C.c_int, [_vp, C.c_int])
    sig("omni_cam_ready", C.c_int, [_vp, C.POINTER(C.c_int)])
    sig("omni_flatten_create", _vp, [_vp, C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(_fp)])
    sig("omni_flatten_destroy", None, [_vp])
    sig("omni_flatten_out_bytes", C.c_int64, [_vp])
    sig("omni_flatten_enqueue_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp])
    sig("omni_resize_create", _vp, [_vp, C.c_int, C.c_int, C.c_int, C.c_int])
    sig("omni_resize_destroy", None, [_vp])
    sig("omni_resize_mode", C.c_int, [_vp])
    sig("omni_resize_enqueue_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp])
    sig("omni_config_count", C.c_int, [])
    sig("omni_config_describe", C.c_int, [C.c_int, C.POINTER(C.c_char_p), _ip, _ip, _ip, _ip, C.POINTER(C.c_char_p)])
    sig("omni_config_value", C.c_int, [C.c_char_p, _ip])
    sig("omni_shard_unique_id", C.c_int, [C.c_char_p])
    sig("omni_shard_library_path", C.c_int, [C.c_char_p, C.c_int])
    sig("omni_shard_create", _vp, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_char_p])
    sig("omni_shard_destroy", None, [_vp])
    sig("omni_shard_ntotal", C.c_int64, [_vp])
    sig("omni_shard_preload_local", C.c_int, [_vp, _fp, C.c_int64, C.c_int64])
    sig("omni_shard_step_batch_dev", C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _fp, _i64p])
    sig("omni_shard_step_enqueue", C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int])
    sig("omni_shard_rows_consumed", C.c_int, [_vp])
    sig("omni_shard_step_wait", C.c_int, [_vp, _fp, _i64p])
    sig("omni_shard_last_exchange_us", C.c_int, [_vp, _fp, _fp])
    sig("omni_shard_search", C.c_int, [_vp, C.c_int, _fp, C.c_int, _fp, _i64p])
    _dp = C.POINTER(C.c_double)
    sig("omni_pcafit_create", _vp, [_vp])
    sig("omni_pcafit_destroy", None, [_vp])
    sig("omni_pcafit_reset", C.c_int, [_vp])
    sig("omni_pcafit_enqueue_rows_dev", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int])
    sig("omni_sp_set_pcafit", C.c_int, [_vp, _vp])
    sig("omni_pcafit_stats", C.c_int, [_vp, _i64p, _i64p])
    sig("omni_pcafit_moments", C.c_int, [_vp, _dp, _dp])
    sig("omni_pcafit_merge_host", C.c_int, [_i64p, _dp, _dp, C.c_int64, _dp, _dp])
    sig("omni_pca_solve_host", C.c_int, [C.c_int64, _dp, _dp, C.c_int, _dp, _fp, _dp, _fp, _dp, _dp])
    sig("omni_pcafit_solve", C.c_int, [_vp, C.c_int, _dp, _fp, _dp, _fp, _dp, _dp])
    sig("omni_pca_moments_host", C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _i64p, _i64p, _dp, _dp])
    sig("omni_pca_write_csv", C.c_int, [C.c_char_p, C.c_char_p, _fp, _fp, C.c_int])
    sig("omni_pcm_create", C.c_int, [_vp, C.c_int, C.POINTER(PcmParams), C.POINTER(_vp)])
    sig("omni_pcm_destroy", None, [_vp])
    sig("omni_pcm_size", C.c_int, [_vp])
    sig("omni_pcm_capacity", C.c_int, [_vp])
    sig("omni_pcm_add", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _fp])
    sig("omni_pcm_adjacency", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp])
    sig("omni_pcm_rows_host", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(PcmParams), C.c_int, _vp, _vp, _vp])
    sig("omni_pcm_max_clique_host", C.c_int, [_vp, C.c_int, C.c_int, _vp, _ip])
    sig("omni_pcm_atan2", C.c_double, [C.c_double, C.c_double])
    sig("omni_pgo_default_params", C.c_int, [C.POINTER(PgoParams)])
    sig("omni_pgo_create", C.c_int, [_vp, C.POINTER(_vp)])
    sig("omni_pgo_destroy", None, [_vp])
    sig("omni_pgo_solve_multi", C.c_int, [_vp, C.POINTER(PgoParams), _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _ip, _fp])
    sig("omni_pgo_solve_host", C.c_int, [C.POINTER(PgoParams), _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _ip])
    sig("omni_pgo_residuals_host", C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp])
    sig("omni_pgo_plan_graph_host", C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _ip])
    sig("omni_pgo_sincos", None, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    sig("omni_pgo_normalize_angle", C.c_double, [C.c_double])
    sig("omni_pgo_sum_host", C.c_double, [_vp, C.c_int])
    if L.omni_abi_version() != ABI_VERSION:
        raise OmniError("libomni_hip.so ABI version mismatch")
    _lib = L
    return L


def _check(rc):
    if rc != OK:
        raise OmniError(f"omni error {rc}: {lib().omni_last_error().decode()}")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _pf(a):
    return a.ctypes.data_as(_fp)


class Context:
    """One HIP stream + scratch on one GPU (omni_ctx)."""

    def __init__(self, device_id: int = 0, high_priority: bool = False):
        import weakref
        self.device_id = device_id
        self._children = weakref.WeakSet()      # handles created on this context: closed before the context is (their destroy uses its stream)
        self.h = lib().omni_ctx_create_priority(device_id, 1) if high_priority else lib().omni_ctx_create(device_id)
        if not self.h:
            raise OmniError(f"omni_ctx_create failed: {lib().omni_last_error().decode()}")

    def _adopt(self, child):
        self._children.add(child)

    def close(self):
        if self.h:
            for kind in ("Cam", "Shard", None):     # omni_cam / omni_shard borrow other handles: they go first
                for ch in list(self._children):
                    if kind is None or type(ch).__name__ == kind:   # noqa: E721
                        try:
                            ch.close()
                        except Exception:
                            pass
            lib().omni_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(lib().omni_ctx_sync(self.h))

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu, mhz, mem = C.c_int(), C.c_int(), C.c_size_t()
        _check(lib().omni_ctx_device_info(self.h, name, 256, C.byref(ncu), C.byref(mhz), C.byref(mem)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "clock_mhz": mhz.value, "hbm_bytes": mem.value}

    def mfma_ceiling(self, ms: float = 100.0):
        """what the fp16 matrix cores of this board sustain (calibration: back-to-back MFMAs on every SIMD for ~ms milliseconds)"""
        tf, ghz = C.c_float(), C.c_float()
        _check(lib().omni_ctx_mfma_ceiling(self.h, C.c_float(ms), C.byref(tf), C.byref(ghz)))
        return {"tflops": tf.value, "sclk_ghz": ghz.value}

    def alloc(self, nbytes: int) -> int:
        p = lib().omni_dev_alloc(self.h, nbytes)
        if not p:
            raise OmniError(f"omni_dev_alloc({nbytes}) failed: {lib().omni_last_error().decode()}")
        return p

    def free(self, p):
        _check(lib().omni_dev_free(self.h, p))

    def to_device(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.alloc(max(arr.nbytes, 1))
        _check(lib().omni_memcpy_h2d(self.h, p, arr.ctypes.data_as(_vp), arr.nbytes))
        return p

    def from_device(self, p: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        _check(lib().omni_memcpy_d2h(self.h, out.ctypes.data_as(_vp), p, out.nbytes))
        return out

    def host_alloc(self, shape, dtype=np.uint8) -> np.ndarray:
        """Pinned host array (hipHostMalloc): the source of asynchronous uploads (omni_cam_enqueue_host).  The array keeps no
        reference to this context; free with host_free()."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = lib().omni_host_alloc(n)
        if not p:
            raise OmniError(f"omni_host_alloc({n}) failed: {lib().omni_last_error().decode()}")
        buf = (C.c_uint8 * n).from_address(p)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            _check(lib().omni_host_free(p))

    def timer_start(self):
        _check(lib().omni_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        _check(lib().omni_timer_stop(self.h, C.byref(ms)))
        return ms.value


class SuperPoint:
    """SuperPointTensorRT(engine, pca_comp, pca_mean, width, height, thres, max_num) -- weights replace the engine file."""

    def __init__(self, ctx: Context, weights: dict, pca_comp, pca_mean, width: int, height: int, thres: float = 0.015,
                 max_num: int = 200, precision: int = PREC_F32, max_batch: int = 1):
        self.ctx, self.W, self.H, self.max_num, self.max_batch, self.precision = ctx, width, height, max_num, max_batch, precision
        self._keep = []
        w = _SpWeights()
        for i, n in enumerate(SP_LAYER_NAMES):
            wt, bs = _f32(weights[n + ".weight"]), _f32(weights[n + ".bias"])
            self._keep += [wt, bs]
            w.weight[i], w.bias[i] = _pf(wt), _pf(bs)
        pc = pm = None
        pca_dim = 0
        if pca_comp is not None:
            pc, pm = _f32(pca_comp), _f32(pca_mean)
            pca_dim = pc.shape[0]
        self.h = lib().omni_sp_create(ctx.h, C.byref(w), _pf(pc) if pc is not None else None,
                                      _pf(pm) if pm is not None else None, pca_dim, width, height, thres, max_num,
                                      precision, max_batch)
        if not self.h:
            raise OmniError(f"omni_sp_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)
        self.desc_dim = lib().omni_sp_desc_dim(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_sp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _outs(self, batch):
        return (np.zeros((batch, self.max_num, 2), np.float32), np.zeros(batch, np.int32),
                np.zeros((batch, self.max_num, self.desc_dim), np.float32), np.zeros((batch, self.max_num), np.float32))

    @staticmethod
    def _split(kps, n, desc, sc):
        return [(kps[b, :n[b]].copy(), desc[b, :n[b]].copy(), sc[b, :n[b]].copy()) for b in range(len(n))]

    def inference(self, gray_u8: np.ndarray, fisheye_mask: bool = False):
        """[H,W] or [B,H,W] uint8 -> list of (kps [n,2] (x,y), desc [n,D], scores [n]) per image."""
        g = np.ascontiguousarray(gray_u8, np.uint8)
        if g.ndim == 2:
            g = g[None]
        b = g.shape[0]
        kps, n, desc, sc = self._outs(b)
        _check(lib().omni_sp_infer(self.h, g.ctypes.data_as(_vp), g.shape[2], b, int(fisheye_mask), _pf(kps),
                                   n.ctypes.data_as(_ip), _pf(desc), _pf(sc)))
        return self._split(kps, n, desc, sc)

    def enqueue_dev(self, gray_dev: int, stride: int, batch: int, fisheye_mask: bool = False):
        _check(lib().omni_sp_enqueue_dev(self.h, gray_dev, stride, batch, int(fisheye_mask)))

    def fetch(self, batch: int):
        kps, n, desc, sc = self._outs(batch)
        _check(lib().omni_sp_fetch(self.h, batch, _pf(kps), n.ctypes.data_as(_ip), _pf(desc), _pf(sc)))
        return self._split(kps, n, desc, sc)

    def dev_outputs(self):
        k, n, d, s = _vp(), _vp(), _vp(), _vp()
        _check(lib().omni_sp_dev_outputs(self.h, C.byref(k), C.byref(n), C.byref(d), C.byref(s)))
        return k.value, n.value, d.value, s.value

    def get_dense(self, batch: int):
        semi = np.empty((batch, self.H, self.W), np.float32)
        desc = np.empty((batch, 256, self.H // 8, self.W // 8), np.float32)
        _check(lib().omni_sp_get_dense(self.h, batch, _pf(semi), _pf(desc)))
        return semi, desc

    def postprocess_dense(self, semi: np.ndarray, desc: np.ndarray):
        semi, desc = _f32(semi), _f32(desc)
        if semi.ndim == 2:
            semi, desc = semi[None], desc[None]
        b = semi.shape[0]
        kps, n, d, sc = self._outs(b)
        _check(lib().omni_sp_postprocess_dense(self.h, _pf(semi), _pf(desc), b, _pf(kps), n.ctypes.data_as(_ip), _pf(d), _pf(sc)))
        return self._split(kps, n, d, sc)

    def debug_layer(self, name: str, batch: int = 1) -> np.ndarray:
        """omni_sp_debug_layer: [batch, C, H, W] float32.  name: "conv1a" .. "conv4b", "heads", "desc" (an activation of the last forward pass, NCHW); "desc_rows_in" /
        "desc_rows_out" (the sparse fp32 descriptor tail's compact rows, C = 4 max_num, H = 256, W = 1); "desc_raw" (the sampled descriptors before the channel
        normalisation, C = max_num, H = 256, W = 1; rows beyond n_kps are not meaningful) / "desc_norm_partial" (their per-channel sums of squares in 8 key-point
        segments, C = 8, H = 256, W = 1): after any pass that ran the post-processing (inference, fetch, postprocess_dense), batch <= that pass's"""
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        _check(lib().omni_sp_debug_layer(self.h, name.encode(), batch, None, C.byref(c), C.byref(h), C.byref(w)))
        out = np.empty((batch, c.value, h.value, w.value), np.float32)
        _check(lib().omni_sp_debug_layer(self.h, name.encode(), batch, _pf(out), C.byref(c), C.byref(h), C.byref(w)))
        return out

    def set_pcafit(self, fit: "PcaFit | None"):
        """omni_sp_set_pcafit: every pass of this handle adds its rows to `fit` (None: detach).  `fit` must have been made on this handle's Context and serves one
        handle at a time; closing either of the two detaches"""
        _check(lib().omni_sp_set_pcafit(self.h, fit.h if fit is not None else None))
        self._pcafit = fit

    def last_plan(self) -> int:
        """The kernel forms of the last pass as bits (include/omni_hip.h omni_sp_last_plan)."""
        return lib().omni_sp_last_plan(self.h)

    def profile(self, gray_dev: int, stride: int, batch: int, reps: int = 5):
        ms = np.zeros(SP_NUM_STAGES, np.float32)
        _check(lib().omni_sp_profile(self.h, gray_dev, stride, batch, reps, _pf(ms)))
        out = []
        for i in range(SP_NUM_STAGES):
            name = lib().omni_sp_stage_name(i).decode()
            if name:
                out.append({"stage": name, "ms": float(ms[i]), "flops_per_image": lib().omni_sp_stage_flops(self.h, i),
                            "tiles_left_out": lib().omni_sp_stage_tiles_left_out(self.h, i)})
        return out


PCA_DIM_IN = 256      # csrc/pca_plan.h kDim


class PcaMoments:
    """The accumulator of a PCA fit on the host (csrc/pca_plan.h): n, skipped, s [256], S [256][256] (symmetric), float64"""

    def __init__(self, n=0, skipped=0, s=None, S=None):
        self.n, self.skipped = int(n), int(skipped)
        self.s = np.zeros(PCA_DIM_IN, np.float64) if s is None else np.ascontiguousarray(s, np.float64).reshape(PCA_DIM_IN).copy()
        self.S = np.zeros((PCA_DIM_IN, PCA_DIM_IN), np.float64) if S is None else np.ascontiguousarray(S, np.float64).reshape(PCA_DIM_IN, PCA_DIM_IN).copy()

    def add_rows(self, raw_desc, norm_partial, n_kps) -> "PcaMoments":
        """omni_pca_moments_host (no GPU): the stand-in of PcaFit.enqueue_rows_dev.  raw_desc [B][M][256], norm_partial [B][8][256] float32, n_kps [B] int32"""
        raw, part, n_kps = _f32(raw_desc), _f32(norm_partial), np.ascontiguousarray(n_kps, np.int32)
        if raw.ndim != 3 or raw.shape[2] != PCA_DIM_IN or part.shape != (raw.shape[0], 8, PCA_DIM_IN) or n_kps.shape != (raw.shape[0],):
            raise ValueError(f"PcaMoments.add_rows: raw_desc {raw.shape}, norm_partial {part.shape}, n_kps {n_kps.shape}")
        n, sk = C.c_int64(self.n), C.c_int64(self.skipped)
        _check(lib().omni_pca_moments_host(raw.ctypes.data, part.ctypes.data, n_kps.ctypes.data, raw.shape[0], raw.shape[1], C.byref(n), C.byref(sk),
                                           self.s.ctypes.data_as(C.POINTER(C.c_double)), self.S.ctypes.data_as(C.POINTER(C.c_double))))
        self.n, self.skipped = n.value, sk.value
        return self

    def add_descriptors(self, descs) -> "PcaMoments":
        """rows given as the 256-d descriptors of one image each (what a handle without PCA returns, [n][256] float32): raw = the descriptor, norm = 1"""
        for d in descs:
            d = _f32(d).reshape(-1, PCA_DIM_IN)
            if len(d) == 0:
                continue
            part = np.zeros((1, 8, PCA_DIM_IN), np.float32)
            part[0, 0] = 1.0
            self.add_rows(d[None], part, np.array([len(d)], np.int32))
        return self

    def merge(self, right: "PcaMoments") -> "PcaMoments":
        """omni_pcafit_merge_host: n, s, S += right's (skipped too)"""
        n = C.c_int64(self.n)
        dp = C.POINTER(C.c_double)
        _check(lib().omni_pcafit_merge_host(C.byref(n), self.s.ctypes.data_as(dp), self.S.ctypes.data_as(dp), right.n, right.s.ctypes.data_as(dp), right.S.ctypes.data_as(dp)))
        self.n, self.skipped = n.value, self.skipped + right.skipped
        return self

    def solve(self, pca_dim: int = 64) -> dict:
        return pca_solve_host(self.n, self.s, self.S, pca_dim)


def _pca_outputs(pca_dim: int):
    k = max(1, min(int(pca_dim), PCA_DIM_IN))
    return {"components": np.zeros((k, PCA_DIM_IN), np.float64), "components_f32": np.zeros((k, PCA_DIM_IN), np.float32), "mean": np.zeros(PCA_DIM_IN, np.float64),
            "mean_f32": np.zeros(PCA_DIM_IN, np.float32), "explained_variance": np.zeros(k, np.float64)}


def _pca_out_args(o, tv):
    dp = C.POINTER(C.c_double)
    return (o["components"].ctypes.data_as(dp), _pf(o["components_f32"]), o["mean"].ctypes.data_as(dp), _pf(o["mean_f32"]), o["explained_variance"].ctypes.data_as(dp), C.byref(tv))


def pca_solve_host(n: int, s, S, pca_dim: int = 64) -> dict:
    """omni_pca_solve_host (no GPU): components [pca_dim][256] and mean [256] in float64 and float32, explained_variance [pca_dim], total_variance"""
    s, S = np.ascontiguousarray(s, np.float64).reshape(PCA_DIM_IN), np.ascontiguousarray(S, np.float64).reshape(PCA_DIM_IN, PCA_DIM_IN)
    o, tv = _pca_outputs(pca_dim), C.c_double()
    dp = C.POINTER(C.c_double)
    _check(lib().omni_pca_solve_host(int(n), s.ctypes.data_as(dp), S.ctypes.data_as(dp), int(pca_dim), *_pca_out_args(o, tv)))
    o["total_variance"] = tv.value
    return o


def pca_write_csv(comp_path: str, mean_path: str, components_f32, mean_f32):
    """omni_pca_write_csv: components_.csv / mean_.csv as every SuperPoint handle here loads them"""
    comp, mean = _f32(components_f32), _f32(mean_f32).reshape(-1)
    if comp.ndim != 2 or comp.shape[1] != PCA_DIM_IN or mean.shape != (PCA_DIM_IN,):
        raise ValueError(f"pca_write_csv: components {comp.shape}, mean {mean.shape}")
    _check(lib().omni_pca_write_csv(os.fsencode(comp_path), os.fsencode(mean_path), _pf(comp), _pf(mean), comp.shape[0]))


class PcaFit:
    """omni_pcafit: the moments of a PCA fit accumulated in HBM (csrc/pca_fit.hip); attach with SuperPoint.set_pcafit or feed rows with enqueue_rows_dev"""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.h = lib().omni_pcafit_create(ctx.h)
        if not self.h:
            raise OmniError(f"omni_pcafit_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_pcafit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _check(lib().omni_pcafit_reset(self.h))

    def enqueue_rows_dev(self, raw_desc_dev: int, norm_partial_dev: int, n_kps_dev: int, batch: int, max_num: int):
        _check(lib().omni_pcafit_enqueue_rows_dev(self.h, raw_desc_dev, norm_partial_dev, n_kps_dev, batch, max_num))

    def stats(self):
        n, sk = C.c_int64(), C.c_int64()
        _check(lib().omni_pcafit_stats(self.h, C.byref(n), C.byref(sk)))
        return n.value, sk.value

    def moments(self) -> PcaMoments:
        m = PcaMoments()
        dp = C.POINTER(C.c_double)
        m.n, m.skipped = self.stats()
        _check(lib().omni_pcafit_moments(self.h, m.s.ctypes.data_as(dp), m.S.ctypes.data_as(dp)))
        return m

    def solve(self, pca_dim: int = 64) -> dict:
        o, tv = _pca_outputs(pca_dim), C.c_double()
        _check(lib().omni_pcafit_solve(self.h, int(pca_dim), *_pca_out_args(o, tv)))
        o["total_variance"] = tv.value
        return o


class MobileNetVLAD:
    """MobileNetVLADTensorRT(engine, width, height); weights (ASSUMED architecture) replace the engine file."""

    def __init__(self, ctx: Context, weights: dict, layer_specs, n_clusters: int, feat_dim: int, out_dim: int,
                 width: int, height: int, max_batch: int = 1):
        self.ctx, self.W, self.H, self.out_dim, self.max_batch = ctx, width, height, out_dim, max_batch
        self._keep = []
        layers = (_VladLayer * len(layer_specs))()
        for i, (name, kind, cin, cout, stride) in enumerate(layer_specs):
            wt, bs = _f32(weights[name + ".weight"]), _f32(weights[name + ".bias"])
            self._keep += [wt, bs]
            layers[i] = _VladLayer(VLAD_KINDS[kind], cin, cout, stride, _pf(wt), _pf(bs))
        aw, ab = _f32(weights["vlad.assign.weight"]).reshape(n_clusters, feat_dim), _f32(weights["vlad.assign.bias"])
        cl, fw, fb = _f32(weights["vlad.clusters"]), _f32(weights["fc.weight"]), _f32(weights["fc.bias"])
        self._keep += [aw, ab, cl, fw, fb, layers]
        vw = _VladWeights(len(layer_specs), layers, n_clusters, feat_dim, out_dim, _pf(aw), _pf(ab), _pf(cl), _pf(fw), _pf(fb))
        self.h = lib().omni_vlad_create(ctx.h, C.byref(vw), width, height, max_batch)
        if not self.h:
            raise OmniError(f"omni_vlad_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_vlad_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_precision(self, precision: int):
        """PREC_F32 (default, parity mode) or PREC_F16 (fp16 matrix-core operands in the inverted-residual blocks)."""
        _check(lib().omni_vlad_set_precision(self.h, int(precision)))

    def inference(self, gray_u8: np.ndarray, fisheye_mask: bool = False) -> np.ndarray:
        g = np.ascontiguousarray(gray_u8, np.uint8)
        if g.ndim == 2:
            g = g[None]
        out = np.empty((g.shape[0], self.out_dim), np.float32)
        _check(lib().omni_vlad_infer(self.h, g.ctypes.data_as(_vp), g.shape[2], g.shape[0], int(fisheye_mask), _pf(out)))
        return out

    def enqueue_dev(self, gray_dev: int, stride: int, batch: int, fisheye_mask: bool = False):
        _check(lib().omni_vlad_enqueue_dev(self.h, gray_dev, stride, batch, int(fisheye_mask)))

    def fetch(self, batch: int) -> np.ndarray:
        out = np.empty((batch, self.out_dim), np.float32)
        _check(lib().omni_vlad_fetch(self.h, batch, _pf(out)))
        return out

    def dev_output(self) -> int:
        p = _vp()
        _check(lib().omni_vlad_dev_output(self.h, C.byref(p)))
        return p.value

    def mask_skip_layers(self) -> list:
        """Share of the tiles of the stem (+ block 0) and of blocks 1, 2, ... that a fisheye-masked pass leaves out (the mask's constant region)."""
        f = (C.c_double * 32)()
        n = lib().omni_vlad_mask_skip_layers(self.h, f, 32)
        return [f[i] for i in range(min(n, 32))]

    def debug_taps(self, on: bool = True):
        """Test hook: from now on a pass keeps a copy of the stem's (where it runs on its own) and every block's output for ``debug_layer``."""
        _check(lib().omni_vlad_debug_taps(self.h, int(on)))

    def debug_layer(self, name: str, batch: int = 1) -> np.ndarray:
        """One layer of the last pass with the taps on, NCHW float32: "stem", "b0" .. "b16", "assign", "vlad", "out"."""
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        _check(lib().omni_vlad_debug_layer(self.h, name.encode(), batch, None, C.byref(c), C.byref(h), C.byref(w)))
        out = np.empty((batch, c.value, h.value, w.value), np.float32)
        _check(lib().omni_vlad_debug_layer(self.h, name.encode(), batch, _pf(out), C.byref(c), C.byref(h), C.byref(w)))
        return out

    def block_paths(self) -> dict:
        """The kernels of the current plan: {"stem": "stem" | "stem_b0" | "layers", "blocks": [VB_NAMES entry per block; None = inside the stem kernel]}."""
        p = (C.c_int * 64)()
        n = lib().omni_vlad_block_paths(self.h, p, 64)
        return {"stem": VLAD_STEM_NAMES[p[0]], "blocks": [VB_NAMES[p[i]] if p[i] >= 0 else None for i in range(1, min(n, 64))]}


def sp_pack_constants(which, w, bias=None, cout=64):
    """Host-only test hook: (halfs as uint16, scale) of conv1a's byte-operand fragments (which = 0), a cin = 64 layer's Winograd fragments (which = 1),
    a direct split layer's fragments (which = 2: w [cout][cin][3][3], cin = 64 or 128) or convDb's split fragments (which = 3: hi, then lo)."""
    w = _f32(w)
    b = _f32(bias) if bias is not None else None
    n_out = {0: 2048, 1: 64 * cout * 32, 2: w.size * 2, 3: 2 * 65536}[which]
    out = np.zeros(n_out, np.uint16)
    sc = C.c_float(0)
    n = lib().omni_sp_pack_constants(which, _pf(w), _pf(b) if b is not None else None, cout, out.ctypes.data_as(_vp), out.size, C.byref(sc))
    if n != out.size:
        raise OmniError(f"omni_sp_pack_constants failed: {lib().omni_last_error().decode()}")
    return out, float(sc.value)


def vlad_pack_block(cin, hid, cout, stride, we, be, wd, bd, wp):
    """Host-only test hook: the split-fp16 weight blob of one inverted-residual block (bytes), or None when no kernel covers the shape."""
    we, be, wd, bd, wp = (_f32(x) for x in (we, be, wd, bd, wp))
    need = lib().omni_vlad_pack_block(cin, hid, cout, stride, None, None, None, None, None, None, 0)
    if need < 0:
        return None
    out = np.zeros(need, np.uint8)
    got = lib().omni_vlad_pack_block(cin, hid, cout, stride, _pf(we), _pf(be), _pf(wd), _pf(bd), _pf(wp), out.ctypes.data_as(_vp), need)
    if got != need:
        raise OmniError(f"omni_vlad_pack_block failed: {lib().omni_last_error().decode()}")
    return out


class IndexFlatIP:
    """faiss::IndexFlatIP(d): add / search / ntotal (+ row sharding)."""

    def __init__(self, ctx: Context, d: int = 4096, storage: int = STORE_F32, capacity: int = 0):
        self.ctx, self.d = ctx, d
        self.h = lib().omni_index_create(ctx.h, d, storage, capacity)
        if not self.h:
            raise OmniError(f"omni_index_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ntotal(self) -> int:
        return lib().omni_index_ntotal(self.h)

    def add(self, x: np.ndarray):
        x = _f32(np.atleast_2d(x))
        assert x.shape[1] == self.d
        _check(lib().omni_index_add(self.h, x.shape[0], _pf(x)))

    def add_dev(self, n: int, x_dev: int):
        _check(lib().omni_index_add_dev(self.h, n, x_dev))

    def reset(self):
        _check(lib().omni_index_reset(self.h))

    def cert_stats(self):
        """(queries answered through the fp16 mirror + exact refinement, of those the ones re-run with the exact scan)"""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(lib().omni_index_cert_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def truncate(self, n_rows: int):
        _check(lib().omni_index_truncate(self.h, n_rows))

    def save(self, path: str):
        """Shard checkpoint (OMNX1): header + the raw row matrix as stored."""
        _check(lib().omni_index_save(self.h, path.encode()))

    def load(self, path: str):
        _check(lib().omni_index_load(self.h, path.encode()))

    def set_shard(self, rank: int, world: int):
        _check(lib().omni_index_set_shard(self.h, rank, world))

    def search(self, q: np.ndarray, k: int):
        q = _f32(np.atleast_2d(q))
        D = np.empty((q.shape[0], k), np.float32)
        I = np.empty((q.shape[0], k), np.int64)
        _check(lib().omni_index_search(self.h, q.shape[0], _pf(q), k, _pf(D), I.ctypes.data_as(_i64p)))
        return D, I

    def search_dev(self, nq: int, q_dev: int, k: int, D_dev: int, I_dev: int):
        _check(lib().omni_index_search_dev(self.h, nq, q_dev, k, D_dev, I_dev))

    def search_prefix_dev(self, nq: int, q_dev: int, k: int, n_limit: int, D_dev: int, I_dev: int):
        """search_dev over the first n_limit rows only (asynchronous; see include/omni_hip.h)."""
        _check(lib().omni_index_search_prefix_dev(self.h, nq, q_dev, k, n_limit, D_dev, I_dev))

    def search_batch_prefix_dev(self, rows_dev: int, row_idx, k: int, limits, D_dev: int, I_dev: int):
        """len(limits) <= 64 prefix searches in ONE pass over the shard: query j = row row_idx[j] of rows_dev (None: rows 0..), it sees
        local rows [0, limits[j]).  Asynchronous (see include/omni_hip.h)."""
        lim = np.ascontiguousarray(limits, np.int64)
        ri = None if row_idx is None else np.ascontiguousarray(row_idx, np.int64)
        _check(lib().omni_index_search_batch_prefix_dev(self.h, len(lim), rows_dev, None if ri is None else ri.ctypes.data_as(_i64p), k,
                                                        lim.ctypes.data_as(_i64p), D_dev, I_dev))

    def search_prefix_many(self, q: np.ndarray, k: int, limits) -> tuple:
        """q [F][nq][d], limits [F]: F searches, search f over this shard's first limits[f] rows only; all enqueued back to back,
        ONE host synchronisation.  Returns D [F][nq][k], I [F][nq][k] (global ids under set_shard)."""
        q = _f32(q)
        F, nq = q.shape[0], q.shape[1]
        D = np.full((F, nq, k), -3.4028235e38, np.float32)
        I = np.full((F, nq, k), -1, np.int64)
        live = [f for f in range(F) if int(limits[f]) > 0]
        if not live:
            return D, I
        qd = self.ctx.to_device(q)
        buf = self.ctx.alloc(F * nq * k * 12)
        try:
            for f in live:
                self.search_prefix_dev(nq, qd + f * nq * self.d * 4, k, int(limits[f]), buf + F * nq * k * 8 + f * nq * k * 4, buf + f * nq * k * 8)
            raw = self.ctx.from_device(buf, (F * nq * k * 12,), np.uint8)
        finally:
            self.ctx.free(qd)
            self.ctx.free(buf)
        Ia = raw[:F * nq * k * 8].view(np.int64).reshape(F, nq, k)
        Da = raw[F * nq * k * 8:].view(np.float32).reshape(F, nq, k)
        for f in live:
            D[f], I[f] = Da[f], Ia[f]
        return D, I

    def debug_scan(self, which: int, q: np.ndarray, n: int = None, limits=None, rotate: bool = True) -> np.ndarray:
        """Test hook (omni_index_debug_scan): ONE named scan kernel (SCAN_F32, SCAN_F32_ROWS, SCAN_T16, SCAN_MQ, SCAN_MQ_MIRROR) over rows [0, n) -> the
        raw 64-bit keys [nq][n] (uint64): high word = the order-preserving map of the fp32 score, low word = 0xFFFFFFFF - row, 0 = beyond the query's limit."""
        q = _f32(np.atleast_2d(q))
        assert q.shape[1] == self.d
        n = self.ntotal if n is None else int(n)
        lim = None if limits is None else np.ascontiguousarray(limits, np.int64)
        assert lim is None or len(lim) == q.shape[0]
        keys = np.empty((q.shape[0], max(n, 0)), np.uint64)
        _check(lib().omni_index_debug_scan(self.h, which, q.shape[0], _pf(q), n, None if lim is None else lim.ctypes.data_as(_i64p), int(bool(rotate)),
                                           keys.ctypes.data))
        return keys

    def last_scan_ms(self) -> float:
        ms = C.c_float()
        _check(lib().omni_index_last_scan_ms(self.h, C.byref(ms)))
        return ms.value


class Flatten:
    """omni_flatten: FisheyeUndist::undist_all_cuda -- one launch remaps fisheye images into all virtual pinhole views (maps from
    omni_swarm_amd.flatten.generate_undist_maps or host/fisheye_flatten.hpp)."""

    def __init__(self, ctx: Context, src_width: int, src_height: int, maps):
        self.ctx = ctx
        self.maps = [np.ascontiguousarray(m, np.float32) for m in maps]          # [h][w][2]
        self.shapes = [(m.shape[0], m.shape[1]) for m in self.maps]
        n = len(self.maps)
        vw = (C.c_int * n)(*[s[1] for s in self.shapes])
        vh = (C.c_int * n)(*[s[0] for s in self.shapes])
        ptrs = (_fp * n)(*[_pf(m) for m in self.maps])
        self.h = lib().omni_flatten_create(ctx.h, src_width, src_height, n, vw, vh, ptrs)
        if not self.h:
            raise OmniError(f"omni_flatten_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)
        self.out_bytes = lib().omni_flatten_out_bytes(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_flatten_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue_dev(self, src_dev: int, src_stride: int, batch: int, out_dev: int):
        _check(lib().omni_flatten_enqueue_dev(self.h, src_dev, src_stride, batch, out_dev))

    def __call__(self, fisheye_u8: np.ndarray):
        """[H,W] or [B,H,W] uint8 -> list over images of lists of views (host convenience: upload, remap, download)."""
        g = np.ascontiguousarray(fisheye_u8, np.uint8)
        if g.ndim == 2:
            g = g[None]
        src = self.ctx.to_device(g)
        out = self.ctx.alloc(self.out_bytes * g.shape[0])
        try:
            self.enqueue_dev(src, g.shape[2], g.shape[0], out)
            raw = self.ctx.from_device(out, (g.shape[0], self.out_bytes), np.uint8)
        finally:
            self.ctx.free(src)
            self.ctx.free(out)
        res = []
        for b in range(g.shape[0]):
            views, o = [], 0
            for (h, w) in self.shapes:
                views.append(raw[b, o:o + h * w].reshape(h, w).copy())
                o += h * w
            res.append(views)
        return res


class Resize:
    """omni_resize: camera-size frames -> network-size images, the cv::resize(INTER_LINEAR) both reference engines run in front of their networks, as the fixed
    integer spec of csrc/resize_plan.h (mode: RESIZE_COPY / RESIZE_AREA2 / RESIZE_LINEAR).  One object per source size -> destination size."""

    def __init__(self, ctx: Context, src_width: int, src_height: int, dst_width: int, dst_height: int):
        self.ctx = ctx
        self.src_w, self.src_h, self.dst_w, self.dst_h = src_width, src_height, dst_width, dst_height
        self.h = lib().omni_resize_create(ctx.h, src_width, src_height, dst_width, dst_height)
        if not self.h:
            raise OmniError(f"omni_resize_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)
        self.mode = lib().omni_resize_mode(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_resize_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue_dev(self, src_dev: int, src_stride: int, batch: int, out_dev: int):
        _check(lib().omni_resize_enqueue_dev(self.h, src_dev, src_stride, batch, out_dev))

    def __call__(self, frames_u8: np.ndarray, src_stride: int = 0) -> np.ndarray:
        """[h,w] or [B,h,w] uint8 -> [B][dst_h][dst_w] (host convenience: upload, resize, download).  src_stride > w: the rows are laid out with that pitch
        on the device (the padding bytes are 0xA5: a kernel that read them would show it)."""
        g = np.ascontiguousarray(frames_u8, np.uint8)
        if g.ndim == 2:
            g = g[None]
        assert g.shape[1:] == (self.src_h, self.src_w)
        stride = src_stride or self.src_w
        if stride != self.src_w:
            padded = np.full((g.shape[0], self.src_h, stride), 0xA5, np.uint8)
            padded[:, :, :self.src_w] = g
            g = padded
        src = self.ctx.to_device(g)
        out = self.ctx.alloc(g.shape[0] * self.dst_h * self.dst_w)
        try:
            self.enqueue_dev(src, stride, g.shape[0], out)
            return self.ctx.from_device(out, (g.shape[0], self.dst_h, self.dst_w), np.uint8)
        finally:
            self.ctx.free(src)
            self.ctx.free(out)


RESIZE_COPY, RESIZE_AREA2, RESIZE_LINEAR = 0, 1, 2


def pcm_params(pcm_thres: float = 0.6, pos_covariance_per_meter: float = 0.01, yaw_covariance_per_meter: float = 0.003) -> PcmParams:
    return PcmParams(pcm_thres, pos_covariance_per_meter, yaw_covariance_per_meter)


def _pcm_edges(edges) -> np.ndarray:
    e = np.ascontiguousarray(edges, dtype=PCM_EDGE_DTYPE).reshape(-1)
    assert PCM_EDGE_DTYPE.itemsize == 248
    return e


def pcm_rows_host(edges, first: int = 0, params: PcmParams | None = None, stride_words: int = 0, with_smd: bool = False):
    """csrc/pcm_plan.h under g++ (omni_pcm_rows_host): edges[first:] are the new vertices.  Returns (rows [n - first][stride_words] u64, degree_add [n] i32) and, with
    with_smd, the distance of every pair (i, j < i) as a third array [n - first][n]."""
    e = _pcm_edges(edges)
    n = len(e)
    stride = stride_words or max(1, (n + 63) // 64)
    pr = params or pcm_params()
    rows = np.zeros((max(n - first, 0), stride), np.uint64)
    deg = np.zeros(max(n, 1), np.int32)
    smd = np.zeros((max(n - first, 0), max(n, 1)), np.float64) if with_smd else None
    _check(lib().omni_pcm_rows_host(e.ctypes.data, n, first, C.byref(pr), stride, rows.ctypes.data, deg.ctypes.data, smd.ctypes.data if with_smd else None))
    return (rows, deg[:n], smd) if with_smd else (rows, deg[:n])


def pcm_max_clique_host(rows: np.ndarray, n: int | None = None) -> np.ndarray:
    """The clique heuristic of csrc/pcm_plan.h on bitset rows [>= n][stride_words] u64: the vertices of the clique found, the start vertex first."""
    r = np.ascontiguousarray(rows, np.uint64)
    n = r.shape[0] if n is None else n
    out = np.zeros(max(n, 1), np.int32)
    size = C.c_int(0)
    _check(lib().omni_pcm_max_clique_host(r.ctypes.data, n, r.shape[1] if r.ndim == 2 and r.shape[1] else 1, out.ctypes.data, C.byref(size)))
    return out[:size.value].copy()


def pcm_atan2(y: float, x: float) -> float:
    return lib().omni_pcm_atan2(y, x)


class Pcm:
    """omni_pcm: the pairwise-consistency graph of one drone pair's loop edges in HBM (csrc/pcm.hip; the arithmetic is csrc/pcm_plan.h's).  add() appends 1..64 edges
    and returns the degrees of all vertices and the new vertices' rows, or None when the handle is full (OMNI_PCM_FULL: nothing changed)."""

    def __init__(self, ctx: Context, capacity: int = PCM_DEFAULT_CAPACITY, params: PcmParams | None = None):
        self.ctx, self.capacity, self.params = ctx, capacity, params or pcm_params()
        h = _vp()
        _check(lib().omni_pcm_create(ctx.h, capacity, C.byref(self.params), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.last_kernel_us = 0.0

    def close(self):
        if getattr(self, "h", None):
            lib().omni_pcm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        return lib().omni_pcm_size(self.h)

    def add(self, edges, time_kernel: bool = False):
        e = _pcm_edges(edges)
        n, held, words = len(e), self.size, self.capacity // 64
        deg = np.zeros(held + max(n, 1), np.int32)
        rows = np.zeros((max(n, 1), words), np.uint64)
        us = C.c_float(0)
        rc = lib().omni_pcm_add(self.h, e.ctypes.data, n, deg.ctypes.data, rows.ctypes.data, C.byref(us) if time_kernel else None)
        if rc == PCM_FULL:
            return None
        _check(rc)
        self.last_kernel_us = us.value
        return deg[:held + n], rows[:n]

    def adjacency(self, first: int = 0, n_rows: int | None = None):
        """(rows [n_rows][capacity / 64] u64 as they lie in HBM, degrees [size] i32)"""
        n_rows = self.size - first if n_rows is None else n_rows
        rows = np.zeros((max(n_rows, 1), self.capacity // 64), np.uint64)
        deg = np.zeros(max(self.size, 1), np.int32)
        _check(lib().omni_pcm_adjacency(self.h, first, n_rows, rows.ctypes.data, deg.ctypes.data))
        return rows[:n_rows], deg[:self.size]


def pgo_params(**kw) -> PgoParams:
    """omni_pgo_default_params with the given fields replaced (max_iterations, max_cg_iterations, max_lambda_retries, initial_lambda, function_tolerance,
    parameter_tolerance, cg_tolerance)"""
    pr = PgoParams()
    _check(lib().omni_pgo_default_params(C.byref(pr)))
    for k, v in kw.items():
        assert k in dict(PgoParams._fields_) and k != "reserved", k
        setattr(pr, k, v)
    return pr


def pgo_edges(edges) -> np.ndarray:
    e = np.ascontiguousarray(edges, dtype=PGO_EDGE_DTYPE).reshape(-1)
    assert PGO_EDGE_DTYPE.itemsize == 80 and PGO_STATS_DTYPE.itemsize == 32
    return e


def pgo_sqrt_inf(pos_cov, yaw_cov) -> np.ndarray:
    """the diagonal square-root information of csrc/pgo_plan.h: 1 / sqrt(cov) over (pos_cov xyz, yaw_cov); a zero covariance gives inf, as IEEE does"""
    with np.errstate(divide="ignore"):
        return 1.0 / np.sqrt(np.concatenate([np.broadcast_to(np.asarray(pos_cov, np.float64), (3,)), [float(yaw_cov)]]))


def _pgo_args(poses, fixed, edges):
    x = np.ascontiguousarray(poses, np.float64)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 4:
        raise OmniError("pose graph: poses must be [n][4] or [starts][n][4]")
    f = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    if len(f) != x.shape[1]:
        raise OmniError("pose graph: fixed must have one byte per pose")
    return x, f, pgo_edges(edges)


def pgo_solve_host(poses, fixed, edges, params: PgoParams | None = None):
    """csrc/pgo_plan.h under g++ (omni_pgo_solve_host): poses [starts][n][4] (or [n][4]: one start).  Returns (poses_out [starts][n][4], stats [starts]
    PGO_STATS_DTYPE, best)."""
    x, f, e = _pgo_args(poses, fixed, edges)
    pr = params or pgo_params()
    out, st, best = np.zeros_like(x), np.zeros(max(x.shape[0], 1), PGO_STATS_DTYPE), C.c_int(-2)
    _check(lib().omni_pgo_solve_host(C.byref(pr), x.ctypes.data, f.ctypes.data, e.ctypes.data, x.shape[1], len(e), x.shape[0], out.ctypes.data, st.ctypes.data, C.byref(best)))
    return out, st[:x.shape[0]], best.value


def pgo_residuals_host(poses, edges):
    """(residuals [m][4], jac_i [m][4][4], jac_j [m][4][4], costs [m]) of csrc/pgo_plan.h at poses [n][4], the loss's correction applied"""
    x, e = np.ascontiguousarray(poses, np.float64), pgo_edges(edges)
    m = len(e)
    r, ji, jj, c = np.zeros((max(m, 1), 4)), np.zeros((max(m, 1), 4, 4)), np.zeros((max(m, 1), 4, 4)), np.zeros(max(m, 1))
    _check(lib().omni_pgo_residuals_host(x.ctypes.data, e.ctypes.data, x.shape[0], m, r.ctypes.data, ji.ctypes.data, jj.ctypes.data, c.ctypes.data))
    return r[:m], ji[:m], jj[:m], c[:m]


def pgo_plan_graph_host(fixed, edges):
    """(offsets [n + 1], incident [2 m] = 2 x edge + side, active [n], n_active) of pgo::plan_graph"""
    f, e = np.ascontiguousarray(fixed, np.uint8).reshape(-1), pgo_edges(edges)
    n, m = len(f), len(e)
    off, inc, act, na = np.zeros(n + 1, np.int32), np.zeros(max(2 * m, 1), np.int32), np.zeros(max(n, 1), np.uint8), C.c_int(0)
    _check(lib().omni_pgo_plan_graph_host(f.ctypes.data, e.ctypes.data, n, m, off.ctypes.data, inc.ctypes.data, act.ctypes.data, C.byref(na)))
    return off, inc[:2 * m], act[:n], na.value


def pgo_sincos(yaw: float):
    s, c = C.c_double(0), C.c_double(0)
    lib().omni_pgo_sincos(yaw, C.byref(s), C.byref(c))
    return s.value, c.value


def pgo_sum_host(v) -> float:
    a = np.ascontiguousarray(v, np.float64).reshape(-1)
    return lib().omni_pgo_sum_host(a.ctypes.data, len(a))


class Pgo:
    """omni_pgo: the 4-DoF pose graph solver on the GPU (csrc/pgo.hip; the arithmetic is csrc/pgo_plan.h's).  solve() takes one graph and 1..64 initial pose sets,
    one workgroup each, and returns what pgo_solve_host returns, bit for bit."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = _vp()
        _check(lib().omni_pgo_create(ctx.h, C.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.last_kernel_us = 0.0

    def close(self):
        if getattr(self, "h", None):
            lib().omni_pgo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, poses, fixed, edges, params: PgoParams | None = None, time_kernel: bool = False):
        x, f, e = _pgo_args(poses, fixed, edges)
        pr = params or pgo_params()
        out, st, best, us = np.zeros_like(x), np.zeros(max(x.shape[0], 1), PGO_STATS_DTYPE), C.c_int(-2), C.c_float(0)
        _check(lib().omni_pgo_solve_multi(self.h, C.byref(pr), x.ctypes.data, f.ctypes.data, e.ctypes.data, x.shape[1], len(e), x.shape[0], out.ctypes.data, st.ctypes.data,
                                          C.byref(best), C.byref(us) if time_kernel else None))
        self.last_kernel_us = us.value
        return out, st[:x.shape[0]], best.value


def jpeg_header(width: int, height: int, quality: int) -> bytes:
    """everything a file of this size and quality holds in front of its scan (csrc/jpeg_plan.h; no GPU)"""
    out = np.empty(JPEG_HEADER_BYTES, np.uint8)
    _check(lib().omni_jpeg_header(width, height, quality, out.ctypes.data_as(_vp)))
    return out.tobytes()


def jpeg_encode_host(gray: np.ndarray, quality: int, zero_from_row: int = -1, capacity: int = 0, width: int = 0):
    """csrc/jpeg_plan.h on the host (g++ inside the library; no GPU): gray [h][stride] u8 of which `width` columns (default all) are the picture ->
    (status, the file's bytes).  zero_from_row < 0: no row is blanked.  capacity 0: room for any file of this size."""
    g = np.ascontiguousarray(gray, np.uint8)
    h, stride = g.shape
    w = width or stride
    cap = capacity or JPEG_HEADER_BYTES + 2 + ((w + 7) // 8) * ((h + 7) // 8) * 416 + 8
    out = np.empty(cap, np.uint8)
    size, status = C.c_int64(0), C.c_int(0)
    _check(lib().omni_jpeg_encode_host(g.ctypes.data_as(_vp), stride, w, h, quality, h if zero_from_row < 0 else zero_from_row, out.ctypes.data_as(_vp), cap,
                                       C.byref(size), C.byref(status)))
    return status.value, out[:size.value].tobytes()


class Jpeg:
    """omni_jpeg: up to max_images images of width x height as baseline JPEG files on the GPU (send_img; csrc/jpeg.hip, the arithmetic: csrc/jpeg_plan.h)"""

    def __init__(self, ctx: Context, width: int, height: int, max_images: int, quality: int, capacity_per_image: int = 0):
        self.ctx, self.w, self.h_img, self.max_images = ctx, width, height, max_images
        self.capacity = capacity_per_image or max(width * height // 2, JPEG_HEADER_BYTES + 2)
        self.h = lib().omni_jpeg_create(ctx.h, width, height, max_images, quality, self.capacity)
        if not self.h:
            raise OmniError(f"omni_jpeg_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_jpeg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue_dev(self, gray_dev: int, stride: int, n_images: int, zero_from_row: int, out_dev: int, sizes_dev: int, status_dev: int):
        _check(lib().omni_jpeg_enqueue_dev(self.h, gray_dev, stride, n_images, zero_from_row, out_dev, sizes_dev, status_dev))

    def __call__(self, images_u8: np.ndarray, zero_from_row: int = -1, stride: int = 0):
        """[h,w] or [B,h,w] uint8 -> [(status, bytes)] per image (host convenience: upload, encode, download).  stride > w: the rows are laid out with that pitch on
        the device (the padding bytes are 0xA5).  The output block is 0xA5 before the call and has a guard behind it: `last_guard_ok` tells whether the stage kept
        to every image's capacity, `last_raw` is the block as it came back."""
        g = np.ascontiguousarray(images_u8, np.uint8)
        if g.ndim == 2:
            g = g[None]
        assert g.shape[1:] == (self.h_img, self.w)
        n, st = g.shape[0], stride or self.w
        if st != self.w:
            padded = np.full((n, self.h_img, st), 0xA5, np.uint8)
            padded[:, :, :self.w] = g
            g = padded
        guard = 64
        src = self.ctx.to_device(g)
        out = self.ctx.to_device(np.full(n * self.capacity + guard, 0xA5, np.uint8))
        meta = self.ctx.to_device(np.full(2 * n, -1, np.int32))
        try:
            self.enqueue_dev(src, st, n, self.h_img if zero_from_row < 0 else zero_from_row, out, meta, meta + 4 * n)
            raw = self.ctx.from_device(out, (n * self.capacity + guard,), np.uint8)
            m = self.ctx.from_device(meta, (2, n), np.int32)
        finally:
            for p in (src, out, meta):
                self.ctx.free(p)
        self.last_raw = raw[:n * self.capacity].reshape(n, self.capacity)
        self.last_guard_ok = bool((raw[n * self.capacity:] == 0xA5).all())
        self.last_sizes = m[0].copy()
        return [(int(m[1, i]), self.last_raw[i, :m[0, i]].tobytes()) for i in range(n)]

def jpegdec_classify(data: bytes):
    """(OMNI_JPEGDEC_* classification, width, height) of a JPEG file (csrc/jpeg_dec_plan.h's parser; no GPU).  0 x 0: no frame header could be read"""
    w, h = C.c_int(0), C.c_int(0)
    st = lib().omni_jpegdec_classify(data, len(data), C.byref(w), C.byref(h))
    return st, w.value, h.value


def _jpeg_decode(data: bytes, stride: int, call):
    cls, w, h = jpegdec_classify(data)
    st = stride or w
    out = np.full((max(h, 1), max(st, 1)), 0xA5, np.uint8)
    ww, hh, status = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(call(out.ctypes.data_as(_vp), st, C.byref(ww), C.byref(hh), C.byref(status)))
    return status.value, (out[:h] if stride else out[:h, :w].copy())


def jpeg_decode_host(data: bytes, stride: int = 0):
    """csrc/jpeg_dec_plan.h's sequential decoder on the host (g++ inside the library; no GPU): a JPEG file -> (status, gray [h][w] u8).  stride > w: the
    array returned is [h][stride], 0xA5 where nothing was written.  UNSUPPORTED: nothing is written"""
    return _jpeg_decode(data, stride, lambda o, st, w, h, s: lib().omni_jpeg_decode_host(data, len(data), o, st, w, h, s))


def jpeg_decode_parallel_host(data: bytes, subseq_bits: int):
    """the CPU stand-in for the kernels -> (status, gray, dict(n_sub, subseq_bits, rounds, wrong_after_first))"""
    stats = (C.c_int * 4)()
    status, pix = _jpeg_decode(data, 0, lambda o, st, w, h, s: lib().omni_jpeg_decode_parallel_host(data, len(data), subseq_bits, o, st, w, h, s, stats))
    return status, pix, dict(n_sub=stats[0], subseq_bits=stats[1], rounds=stats[2], wrong_after_first=stats[3])


JPEGDEC_MAX_SUBSEQ = 4096                     # csrc/jpeg_dec_plan.h JD_MAX_SUBSEQ: subsequences one workgroup of the entropy kernel holds


def jpeg_decode_restart_parallel_host(data: bytes, subseq_bits: int, restart_wgs: int, max_subseq: int = JPEGDEC_MAX_SUBSEQ):
    """the CPU stand-in for the kernels of a handle with OMNI_JPEGDEC_RESTART_WGS = restart_wgs -> (status, gray, dict(n_sub, subseq_bits, chunks, rounds)): a
    restart-interval file is planned into chunks and decoded by the phase functions (OK), or left to the sequential decoder when it cannot be planned (HOST)"""
    stats = (C.c_int * 4)()
    status, pix = _jpeg_decode(data, 0, lambda o, st, w, h, s: lib().omni_jpeg_decode_restart_parallel_host(data, len(data), subseq_bits, restart_wgs, max_subseq, o, st,
                                                                                                           w, h, s, stats))
    return status, pix, dict(n_sub=stats[0], subseq_bits=stats[1], chunks=stats[2], rounds=stats[3])


def jpeg_decode_plain_parallel_host(data: bytes, subseq_bits: int, plain_wgs: int, max_subseq: int = JPEGDEC_MAX_SUBSEQ):
    """the CPU stand-in for the kernels of a handle with OMNI_JPEGDEC_PLAIN_WGS = plain_wgs -> (status, gray, dict(n_sub, subseq_bits, chunks, chunk_rounds,
    seam_rounds, seam_changed, seam_chunks, rounds = chunk_rounds + seam_rounds: what omni_jpegdec_last_stats reports)): a file without a restart interval over
    min(plain_wgs, n_sub) chunks that relax on their own, then the seam relaxation over the whole picture"""
    stats = (C.c_int * 7)()
    status, pix = _jpeg_decode(data, 0, lambda o, st, w, h, s: lib().omni_jpeg_decode_plain_parallel_host(data, len(data), subseq_bits, plain_wgs, max_subseq, o, st,
                                                                                                         w, h, s, stats))
    return status, pix, dict(n_sub=stats[0], subseq_bits=stats[1], chunks=stats[2], chunk_rounds=stats[3], seam_rounds=stats[4], seam_changed=stats[5],
                             seam_chunks=stats[6], rounds=stats[3] + stats[4])


def jpeg_unstuff_tile_bytes() -> int:
    """csrc/jpeg_dec_plan.h JD_UNSTUFF_TILE: raw scan bytes per tile of the unstuffing by tiles"""
    return lib().omni_jpeg_unstuff_tile_bytes()


def jpeg_scan_end(data: bytes, start: int = 0) -> int:
    """csrc/jpeg_dec_plan.h scan_end: where the entropy-coded data that start at `start` end"""
    return lib().omni_jpeg_scan_end(data, len(data), start)


def jpeg_unstuff_host(scan: bytes):
    """the byte-wise pass (jd::unstuff; g++, no GPU) -> (clean bytes + the 16 bytes behind them u8, clean count, [clean offset behind every restart marker])"""
    n = len(scan)
    out = np.full(n + 16, 0xA5, np.uint8)
    rst = (C.c_int64 * (n // 2 + 1))()
    k, nr = C.c_int64(), C.c_int64()
    _check(lib().omni_jpeg_unstuff_host(scan, n, out.ctypes.data_as(_vp), out.size, C.byref(k), rst, len(rst), C.byref(nr)))
    return out[:k.value + 16].copy(), k.value, list(rst[:nr.value])


def jpeg_unstuff_tiled_host(scan: bytes):
    """survey + every tile compacted on its own into a buffer of 0xA5 (jd::survey, jd::unstuff_tiled_host: the CPU stand-in for jpegdec_unstuff_kernel) ->
    dict(out: the clean bytes + 16 u8, n_clean: the end of the last tile, rst, raw_end, surveyed_clean, tile_off [n_tiles])"""
    n = len(scan)
    out = np.zeros(n + 16, np.uint8)
    rst = (C.c_int64 * (n // 2 + 1))()
    tiles = np.zeros(n // jpeg_unstuff_tile_bytes() + 1, np.uint32)
    k, nr, re, sc, nt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _check(lib().omni_jpeg_unstuff_tiled_host(scan, n, out.ctypes.data_as(_vp), out.size, C.byref(k), rst, len(rst), C.byref(nr), C.byref(re), C.byref(sc),
                                              tiles.ctypes.data_as(_vp), tiles.size, C.byref(nt)))
    return dict(out=out[:max(k.value, 0) + 16].copy(), n_clean=k.value, rst=list(rst[:nr.value]), raw_end=re.value, surveyed_clean=sc.value,
                tile_off=[int(t) for t in tiles[:nt.value]])


def jpegdec_unstuff_dev(ctx: "Context", scan: bytes):
    """TEST INFRASTRUCTURE: jpegdec_unstuff_kernel alone on a byte string taken as a scan -> (clean bytes + the 16 bytes behind them u8, clean count)"""
    out = np.full(len(scan) + 16, 0xA5, np.uint8)
    k = C.c_int64()
    _check(lib().omni_jpegdec_unstuff_dev(ctx.h, scan, len(scan), out.ctypes.data_as(_vp), out.size, C.byref(k)))
    return out[:k.value + 16].copy(), k.value


class JpegDec:
    """omni_jpegdec: up to max_images JPEG files of at most capacity_per_image bytes -> gray images of width x height on the GPU (is_compressed_images;
    csrc/jpeg_dec.hip, the arithmetic: csrc/jpeg_dec_plan.h)"""

    def __init__(self, ctx: Context, width: int, height: int, max_images: int, capacity_per_image: int = 0):
        self.ctx, self.w, self.h_img, self.max_images = ctx, width, height, max_images
        self.capacity = capacity_per_image or max(width * height // 2, 1024)
        self.h = lib().omni_jpegdec_create(ctx.h, width, height, max_images, self.capacity)
        if not self.h:
            raise OmniError(f"omni_jpegdec_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_jpegdec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue_host(self, files, out_dev: int, out_stride: int, status_dev: int):
        """files: [bytes]; asynchronous on the context's stream (the files may go on return)"""
        n = len(files)
        ptrs = (_vp * n)(*[C.cast(C.c_char_p(f), _vp) for f in files])
        sizes = (C.c_int64 * n)(*[len(f) for f in files])
        _check(lib().omni_jpegdec_enqueue_host(self.h, ptrs, sizes, n, out_dev, out_stride, status_dev))

    def last_stats(self, n: int):
        """per image of the last call: (relaxation rounds that changed something, subsequences, bits per subsequence)"""
        r, s, b = (C.c_int * self.max_images)(), (C.c_int * self.max_images)(), (C.c_int * self.max_images)()
        _check(lib().omni_jpegdec_last_stats(self.h, r, s, b))
        return [(r[i], s[i], b[i]) for i in range(n)]

    def last_chunks(self, n: int):
        """per image of the last call: the entropy kernel's workgroups that decoded a share of it (the chunks of a restart-interval file)"""
        k = (C.c_int * self.max_images)()
        _check(lib().omni_jpegdec_last_chunks(self.h, k))
        return [k[i] for i in range(n)]

    def last_seam(self, n: int):
        """per image of the last call: (seam relaxation rounds that changed something, subsequences it changed) of a picture spread by OMNI_JPEGDEC_PLAIN_WGS;
        (0, 0) for every other image"""
        r, m = (C.c_int * self.max_images)(), (C.c_int * self.max_images)()
        _check(lib().omni_jpegdec_last_seam(self.h, r, m))
        return [(r[i], m[i]) for i in range(n)]

    def last_ms(self):
        """(upload ms, memsets + kernels ms, bytes uploaded) of the last call, on the GPU's clock"""
        u, k, b = C.c_float(), C.c_float(), C.c_int64()
        _check(lib().omni_jpegdec_last_ms(self.h, C.byref(u), C.byref(k), C.byref(b)))
        return u.value, k.value, b.value

    def guards_ok(self) -> bool:
        """the 0xA5 bytes behind the coefficient buffer, the DC buffer and (OMNI_JPEGDEC_PLAIN_WGS >= 2) the state arrays are as they were created"""
        cp, cb, dp, db, sp, sb = _vp(), C.c_int64(), _vp(), C.c_int64(), _vp(), C.c_int64()
        _check(lib().omni_jpegdec_debug_buffers(self.h, C.byref(cp), C.byref(cb), C.byref(dp), C.byref(db)))
        _check(lib().omni_jpegdec_debug_state_buffer(self.h, C.byref(sp), C.byref(sb)))
        self.ctx.sync()
        self.guarded = 2 + bool(sp.value)                      # the buffers whose guards were looked at
        return all(bool((self.ctx.from_device(p.value + b.value, (JPEGDEC_GUARD_BYTES,), np.uint8) == 0xA5).all()) for p, b in ((cp, cb), (dp, db), (sp, sb)) if p.value)

    def last_unstuff(self):
        """(pictures whose scan the device unstuffed, raw scan bytes uploaded for them, clean bytes they became) of the last call; (0, 0, 0) on a handle whose
        OMNI_JPEGDEC_UNSTUFF_DEV is 0"""
        n, r, k = C.c_int(), C.c_int64(), C.c_int64()
        _check(lib().omni_jpegdec_last_unstuff(self.h, C.byref(n), C.byref(r), C.byref(k)))
        return n.value, r.value, k.value

    def unstuff_guard_ok(self) -> bool:
        """the 0xA5 bytes behind the last clean area of the last call (OMNI_JPEGDEC_UNSTUFF_DEV = 1) are intact; `unstuff_guarded`: whether there was such a guard
        to look at (0 on a handle with the switch off: True)"""
        p, b = _vp(), C.c_int64()
        _check(lib().omni_jpegdec_debug_in_buffer(self.h, C.byref(p), C.byref(b)))
        self.unstuff_guarded = int(bool(p.value))
        if not p.value:
            return True
        self.ctx.sync()
        return bool((self.ctx.from_device(p.value, (b.value,), np.uint8) == 0xA5).all())

    def __call__(self, files, stride: int = 0):
        """[bytes] -> ([status], pictures [n][h][stride or w] u8) (host convenience: enqueue, download).  The output block is 0xA5 before the call and has a guard
        behind it: `last_guard_ok` tells whether the stage kept to it (and to its own buffers' guards)."""
        n, st = len(files), stride or self.w
        guard = 256
        out = self.ctx.to_device(np.full(n * self.h_img * st + guard, 0xA5, np.uint8))
        status = self.ctx.to_device(np.full(n, -1, np.int32))
        try:
            self.enqueue_host(files, out, st, status)
            raw = self.ctx.from_device(out, (n * self.h_img * st + guard,), np.uint8)
            stv = self.ctx.from_device(status, (n,), np.int32)
        finally:
            self.ctx.free(out)
            self.ctx.free(status)
        self.last_guard_ok = bool((raw[n * self.h_img * st:] == 0xA5).all()) and self.guards_ok()
        return [int(v) for v in stv], raw[:n * self.h_img * st].reshape(n, self.h_img, st)


SHARD_ID_BYTES = 128


def shard_unique_id() -> bytes:
    """ncclGetUniqueId through the library: call on rank 0, carry the 128 bytes to the other ranks by any channel."""
    buf = C.create_string_buffer(SHARD_ID_BYTES)
    _check(lib().omni_shard_unique_id(buf))
    return buf.raw


def sp_mask_band_plan(width: int, height: int, precision: int, layer: int):
    """(first tile row, tile rows, share of the layer's tiles) of the full-width band of tile rows a fisheye-masked pass leaves out of layer `layer`
    (1..5 = conv1b, conv2a, conv2b, conv3a, conv3b; first tile row == tile rows: no band): csrc/superpoint.hip, pure arithmetic (no device)."""
    ty0, tiles_y, frac = C.c_int(), C.c_int(), C.c_double()
    _check(lib().omni_sp_mask_band_plan(width, height, precision, layer, C.byref(ty0), C.byref(tiles_y), C.byref(frac)))
    return ty0.value, tiles_y.value, frac.value


def sp_mask_skip_plan(width: int, height: int, precision: int, layer: int):
    """((tile row 0, tile row 1, tile column 0, tile column 1), share of the layer's tiles) of the rectangle inside that band where layer `layer`'s output
    is one constant vector (0 = conv1a [split only], 1..5 = conv1b, conv2a, conv2b, conv3a, conv3b): csrc/superpoint.hip, pure arithmetic (no device)."""
    rect = (C.c_int * 4)()
    frac = C.c_double()
    _check(lib().omni_sp_mask_skip_plan(width, height, precision, layer, rect, C.byref(frac)))
    return tuple(rect), frac.value


def config_table() -> list:
    """csrc/config.h's table: [{env, default, lo, hi, cls, doc}] (cls: 0 variant, 1 tuning, 2 debug, 3 test, 4 string)"""
    out = []
    for i in range(lib().omni_config_count()):
        env, doc = C.c_char_p(), C.c_char_p()
        d, lo, hi, cls = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(lib().omni_config_describe(i, C.byref(env), C.byref(d), C.byref(lo), C.byref(hi), C.byref(cls), C.byref(doc)))
        out.append({"env": env.value.decode(), "default": d.value, "lo": lo.value, "hi": hi.value, "cls": cls.value, "doc": doc.value.decode()})
    return out


def config_value(env: str) -> int:
    """what a handle created now would see for this option"""
    v = C.c_int()
    _check(lib().omni_config_value(env.encode(), C.byref(v)))
    return v.value


def shard_library_path() -> str:
    """The file ncclAllGather & co. were resolved from (the process's librccl, or what OMNI_RCCL_LIB names)."""
    buf = C.create_string_buffer(1024)
    _check(lib().omni_shard_library_path(buf, 1024))
    return buf.value.decode()


class Shard:
    """omni_shard: this rank's part of the row-sharded key-frame database; collectives are RCCL inside libomni_hip.so (csrc/shard.hip)."""

    def __init__(self, ctx: Context, local: IndexFlatIP, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == SHARD_ID_BYTES
        self.ctx, self.local, self.rank, self.world = ctx, local, rank, world
        self.h = lib().omni_shard_create(ctx.h, local.h, local.d, rank, world, unique_id)
        if not self.h:
            raise OmniError(f"omni_shard_create failed: {lib().omni_last_error().decode()}")
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().omni_shard_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ntotal(self) -> int:
        return lib().omni_shard_ntotal(self.h)

    def preload_local(self, rows_local: np.ndarray, ntotal_global: int):
        rows_local = _f32(rows_local)
        _check(lib().omni_shard_preload_local(self.h, _pf(rows_local), rows_local.shape[0], ntotal_global))

    def step_batch_dev(self, F: int, m: int, rows_dev: int, query_row: int, k: int):
        D = np.empty((F, k), np.float32)
        I = np.empty((F, k), np.int64)
        _check(lib().omni_shard_step_batch_dev(self.h, F, m, rows_dev, query_row, k, _pf(D), I.ctypes.data_as(_i64p)))
        return D, I

    def step_enqueue(self, F: int, m: int, rows_dev: int, query_row: int, k: int):
        """asynchronous half of step_batch_dev: the whole exchange unit is put on the shard's stream, nothing is waited for"""
        self._pend = (F, k)
        _check(lib().omni_shard_step_enqueue(self.h, F, m, rows_dev, query_row, k))

    def rows_consumed(self):
        _check(lib().omni_shard_rows_consumed(self.h))

    def step_wait(self):
        F, k = self._pend
        D = np.empty((F, k), np.float32)
        I = np.empty((F, k), np.int64)
        _check(lib().omni_shard_step_wait(self.h, _pf(D), I.ctypes.data_as(_i64p)))
        return D, I

    def search(self, q: np.ndarray, k: int):
        q = _f32(np.atleast_2d(q))
        D = np.empty((q.shape[0], k), np.float32)
        I = np.empty((q.shape[0], k), np.int64)
        _check(lib().omni_shard_search(self.h, q.shape[0], _pf(q), k, _pf(D), I.ctypes.data_as(_i64p)))
        return D, I


def topk_merge(D_lists: np.ndarray, I_lists: np.ndarray, k_out: int):
    """[n_lists, nq, k_each] per-shard lists -> merged [nq, k_out] (score desc, id asc).  Host-side, no GPU needed."""
    D_lists, I_lists = _f32(D_lists), np.ascontiguousarray(I_lists, np.int64)
    n_lists, nq, k_each = D_lists.shape
    D = np.empty((nq, k_out), np.float32)
    I = np.empty((nq, k_out), np.int64)
    _check(lib().omni_topk_merge(n_lists, nq, k_each, _pf(D_lists), I_lists.ctypes.data_as(_i64p), k_out, _pf(D),
                                 I.ctypes.data_as(_i64p)))
    return D, I


def bf_match(ctx: Context, q: np.ndarray, t: np.ndarray, mode: int = BF_OPENCV):
    """cv::BFMatcher(NORM_L2, crossCheck=true).match(q, t) -> (query_idx, train_idx, distance)."""
    q, t = _f32(q), _f32(t)
    nq, nt = q.shape[0], t.shape[0]
    dim = q.shape[1] if q.ndim == 2 and nq else (t.shape[1] if t.ndim == 2 else 64)
    qi, ti, dd = np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.float32)
    n = C.c_int(0)
    _check(lib().omni_bf_match(ctx.h, _pf(q), nq, _pf(t), nt, dim, mode, qi.ctypes.data_as(_ip), ti.ctypes.data_as(_ip),
                               _pf(dd), C.byref(n)))
    return qi[:n.value].copy(), ti[:n.value].copy(), dd[:n.value].copy()


def bf_match_multi(ctx: Context, pairs, mode: int = BF_OPENCV):
    """[(q, t), ...] -> [(query_idx, train_idx, distance), ...]: bf_match of every pair in one GPU round trip."""
    P = len(pairs)
    qs, ts = [_f32(q) for q, _ in pairs], [_f32(t) for _, t in pairs]
    dim = next((a.shape[1] for a in qs + ts if a.ndim == 2 and a.shape[0]), 64)
    nq = np.array([q.shape[0] for q in qs], np.int32)
    nt = np.array([t.shape[0] for t in ts], np.int32)
    max_n = int(max(1, nq.max(), nt.max()))
    qp = (_fp * P)(*[_pf(q) if q.shape[0] else None for q in qs])
    tp = (_fp * P)(*[_pf(t) if t.shape[0] else None for t in ts])
    qi, ti, dd, n = np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.float32), np.zeros(P, np.int32)
    _check(lib().omni_bf_match_multi(ctx.h, P, qp, nq.ctypes.data_as(_ip), tp, nt.ctypes.data_as(_ip), dim, mode, max_n, qi.ctypes.data_as(_ip),
                                     ti.ctypes.data_as(_ip), _pf(dd), n.ctypes.data_as(_ip)))
    return [(qi[p, :n[p]].copy(), ti[p, :n[p]].copy(), dd[p, :n[p]].copy()) for p in range(P)]


def homography_ransac_multi(ctx: Context, pairs) -> list:
    """[(src_xy, dst_xy), ...] ([n][2] float pixels of the old / the new image) -> [{status, mask [n], H [9], info [4]}]: cv::findHomography(src, dst, RANSAC, 3, mask)
    of every pair in one GPU round trip (omni_homography_ransac_multi); status is one of HG_*"""
    P = len(pairs)
    count = np.array([len(a) for a, _ in pairs], np.int32)
    max_n = int(max(1, count.max()))
    src, dst = np.zeros((P, max_n, 2), np.float32), np.zeros((P, max_n, 2), np.float32)
    for p, (a, b) in enumerate(pairs):
        src[p, :count[p]], dst[p, :count[p]] = _f32(a).reshape(-1, 2), _f32(b).reshape(-1, 2)
    status, mask, H, info = np.zeros(P, np.int32), np.zeros((P, max_n), np.uint8), np.zeros((P, 9), np.float64), np.zeros((P, 4), np.int32)
    _check(lib().omni_homography_ransac_multi(ctx.h, P, max_n, _pf(src), _pf(dst), count.ctypes.data_as(_ip), status.ctypes.data_as(_ip), mask.ctypes.data,
                                              H.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(_ip)))
    return [{"status": int(status[p]), "mask": mask[p, :count[p]].copy(), "H": H[p].copy(), "info": info[p].copy()} for p in range(P)]


def pnp_ransac_multi(ctx: Context, cands) -> list:
    """[(X_xyz [n][3], u_xy [n][2], max_iters), ...] (float 3-D points and normalised image points) -> [{status, mask [n], Rt [12], info [4]}]: the RANSAC half of
    cv::solvePnPRansac(X, u, K = I, ..., max_iters, 3, 0.99, inliers) of every candidate in one GPU round trip (omni_pnp_ransac_multi); status is one of PNP_*"""
    P = len(cands)
    count = np.array([len(a) for a, _, _ in cands], np.int32)
    iters = np.array([it for _, _, it in cands], np.int32)
    max_n = int(max(1, count.max()))
    X, u = np.zeros((P, max_n, 3), np.float32), np.zeros((P, max_n, 2), np.float32)
    for p, (a, b, _) in enumerate(cands):
        X[p, :count[p]], u[p, :count[p]] = _f32(a).reshape(-1, 3), _f32(b).reshape(-1, 2)
    status, mask, Rt, info = np.zeros(P, np.int32), np.zeros((P, max_n), np.uint8), np.zeros((P, 12), np.float64), np.zeros((P, 4), np.int32)
    _check(lib().omni_pnp_ransac_multi(ctx.h, P, max_n, _pf(X), _pf(u), count.ctypes.data_as(_ip), iters.ctypes.data_as(_ip), status.ctypes.data_as(_ip), mask.ctypes.data,
                                       Rt.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(_ip)))
    return [{"status": int(status[p]), "mask": mask[p, :count[p]].copy(), "Rt": Rt[p].copy(), "info": info[p].copy()} for p in range(P)]


def bf_match_homography_multi(ctx: Context, pairs, mode: int = BF_OPENCV) -> list:
    """[(q_desc, t_desc, q_xy, t_xy, q_flags), ...] -> per pair {q_idx, t_idx, dist (bf_match's), kept (positions in the match list of the matches whose query key
    point is flagged), mask (over kept), H, info, status}: the matcher, the flag filter and the homography RANSAC of compute_correspond_features in one GPU round
    trip (omni_bf_match_homography_multi)"""
    P = len(pairs)
    qs, ts = [_f32(x[0]) for x in pairs], [_f32(x[1]) for x in pairs]
    qx, tx = [_f32(x[2]).reshape(-1, 2) for x in pairs], [_f32(x[3]).reshape(-1, 2) for x in pairs]
    fl = [np.ascontiguousarray(x[4], np.uint8) for x in pairs]
    dim = next((a.shape[1] for a in qs + ts if a.ndim == 2 and a.shape[0]), 64)
    nq, nt = np.array([q.shape[0] for q in qs], np.int32), np.array([t.shape[0] for t in ts], np.int32)
    nf = np.array([f.shape[0] for f in fl], np.int32)
    max_n = int(max(1, nq.max(), nt.max(), nf.max()))
    ptrs = lambda arrs: (_fp * P)(*[_pf(a) if a.shape[0] else None for a in arrs])
    fp = (_vp * P)(*[f.ctypes.data if f.shape[0] else None for f in fl])
    qi, ti, dd, n = np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.float32), np.zeros(P, np.int32)
    kept, nk, mask = np.zeros((P, max_n), np.int32), np.zeros(P, np.int32), np.zeros((P, max_n), np.uint8)
    H, info, status = np.zeros((P, 9), np.float64), np.zeros((P, 4), np.int32), np.zeros(P, np.int32)
    ip = lambda a: a.ctypes.data_as(_ip)
    _check(lib().omni_bf_match_homography_multi(ctx.h, P, ptrs(qs), ip(nq), ptrs(ts), ip(nt), dim, mode, max_n, ptrs(qx), ptrs(tx), fp, ip(nf), ip(qi), ip(ti), _pf(dd), ip(n),
                                                ip(kept), ip(nk), mask.ctypes.data, H.ctypes.data_as(C.POINTER(C.c_double)), ip(info), ip(status)))
    return [{"q_idx": qi[p, :n[p]].copy(), "t_idx": ti[p, :n[p]].copy(), "dist": dd[p, :n[p]].copy(), "kept": kept[p, :nk[p]].copy(), "mask": mask[p, :nk[p]].copy(),
             "H": H[p].copy(), "info": info[p].copy(), "status": int(status[p])} for p in range(P)]


CORR_OK, CORR_REJECT, CORR_HOST = 0, 1, 2      # include/omni_hip.h OMNI_CORR_*
HG_UNFILTERED, HG_OK, HG_NO_MODEL, HG_HOST = 0, 1, 2, 3


def _corr_cands(cands):
    """[(pair_first, pair_count, min_match_pre_dir, min_direction_loop, min_loop_num, init_mode_min_loop_num, init_mode), ...] -> omni_corr_cand[]"""
    out = (CorrCand * max(len(cands), 1))()
    for c, v in enumerate(cands):
        (out[c].pair_first, out[c].pair_count, out[c].min_match_pre_dir, out[c].min_direction_loop, out[c].min_loop_num, out[c].init_mode_min_loop_num,
         out[c].init_mode) = (int(x) for x in v)
    return out


def _corr_result(cands, P, n_corr, mdc, gate, X, u, new_idx, old_idx, npc):
    per_cand = [{"n_corr": int(n_corr[c]), "matched_dir_count": int(mdc[c]), "gate": int(gate[c]), "X": X[c, :max(0, n_corr[c])].copy(), "u": u[c, :max(0, n_corr[c])].copy()}
                for c in range(len(cands))]
    per_pair = [{"new_idx": new_idx[p, :max(0, npc[p])].copy(), "old_idx": old_idx[p, :max(0, npc[p])].copy()} for p in range(P)]
    return per_cand, per_pair


class CorrArrays:
    """omni_corr_io in host memory, built from per-pair dicts: q_idx, t_idx (the matcher's list), q_flags, nq, nt, mask (over the flagged matches), hg_status, q_3d
    [nq][3], t_norm [nt][2], dq_old (w, x, y, z); cands: see _corr_cands.  .io is the struct (the arrays live as long as this object)"""

    def __init__(self, cands, pairs, max_n: int | None = None, cap: int | None = None):
        P, Cn = len(pairs), len(cands)
        if max_n is None:
            max_n = int(max([1] + [max(len(p["q_idx"]), len(p["q_flags"]), p["nq"], p["nt"], len(p["mask"])) for p in pairs]))
        if cap is None:
            cap = max(1, max([c[1] for c in cands] + [0]) * max_n)
        Pn, Cc = max(P, 1), max(Cn, 1)
        self.cands, self.P, self.max_n, self.cap = cands, P, max_n, cap
        self.qi, self.ti = np.zeros((Pn, max_n), np.int32), np.zeros((Pn, max_n), np.int32)
        self.fl, self.mk = np.zeros((Pn, max_n), np.uint8), np.zeros((Pn, max_n), np.uint8)
        self.nm, self.nf, self.nq, self.nt, self.st = (np.zeros(Pn, np.int32) for _ in range(5))
        self.q3, self.tn, self.dq = np.zeros((Pn, max_n, 3), np.float32), np.zeros((Pn, max_n, 2), np.float32), np.zeros((Pn, 4), np.float64)
        for p, d in enumerate(pairs):
            n = len(d["q_idx"])
            self.qi[p, :n], self.ti[p, :n], self.nm[p] = d["q_idx"], d["t_idx"], d.get("n_matches", n)
            self.fl[p, :len(d["q_flags"])], self.nf[p] = d["q_flags"], len(d["q_flags"])
            self.mk[p, :len(d["mask"])] = d["mask"]
            self.nq[p], self.nt[p], self.st[p] = d["nq"], d["nt"], d["hg_status"]
            a, b = _f32(d["q_3d"]).reshape(-1, 3), _f32(d["t_norm"]).reshape(-1, 2)
            self.q3[p, :len(a)], self.tn[p, :len(b)], self.dq[p] = a, b, d["dq_old"]
        self.X, self.u = np.zeros((Cc, cap, 3), np.float32), np.zeros((Cc, cap, 2), np.float32)
        self.n_corr, self.mdc, self.gate = (np.full(Cc, -1, np.int32) for _ in range(3))
        self.new_idx, self.old_idx, self.npc = np.zeros((Pn, max_n), np.int32), np.zeros((Pn, max_n), np.int32), np.zeros(Pn, np.int32)
        self.cd = _corr_cands(cands)
        self.io = CorrIO(Cn, P, max_n, cap, C.cast(self.cd, _vp), *(a.ctypes.data for a in (
            self.qi, self.ti, self.nm, self.fl, self.nf, self.nq, self.nt, self.mk, self.st, self.q3, self.tn, self.dq, self.X, self.u, self.n_corr, self.mdc, self.gate,
            self.new_idx, self.old_idx, self.npc)))

    def result(self):
        return _corr_result(self.cands, self.P, self.n_corr, self.mdc, self.gate, self.X, self.u, self.new_idx, self.old_idx, self.npc)


def corr_assemble(cands, pairs, ctx: Context | None = None, max_n: int | None = None, cap: int | None = None, time_kernel: bool = False):
    """The correspondences of loop candidates (csrc/corr_plan.h): ctx None -> omni_corr_assemble_host, no GPU; a Context -> the kernel alone
    (omni_corr_assemble_multi).  cands, pairs: see CorrArrays.  -> (per candidate {n_corr, matched_dir_count, gate, X [n][3], u [n][2]}, per pair {new_idx,
    old_idx})[, the kernel's microseconds]"""
    a = CorrArrays(cands, pairs, max_n, cap)
    us = C.c_float(-1.0)
    if ctx is None:
        _check(lib().omni_corr_assemble_host(C.byref(a.io)))
    else:
        _check(lib().omni_corr_assemble_multi(ctx.h, C.byref(a.io), C.byref(us) if time_kernel else None))
    return a.result() + (float(us.value),) if time_kernel else a.result()


def bf_match_homography_corr_multi(ctx: Context, pairs, cands, mode: int = BF_OPENCV):
    """bf_match_homography_multi with the correspondence stage behind it in the same round trip (omni_bf_match_homography_corr_multi).  pairs:
    [(q_desc, t_desc, q_xy, t_xy, q_flags, q_3d [nq][3], t_norm [nt][2], dq_old (w, x, y, z)), ...]; cands: see _corr_cands.  -> (bf_match_homography_multi's
    list, per candidate {n_corr, matched_dir_count, gate, X, u}, per pair {new_idx, old_idx})"""
    P = len(pairs)
    qs, ts = [_f32(x[0]) for x in pairs], [_f32(x[1]) for x in pairs]
    qx, tx = [_f32(x[2]).reshape(-1, 2) for x in pairs], [_f32(x[3]).reshape(-1, 2) for x in pairs]
    fl = [np.ascontiguousarray(x[4], np.uint8) for x in pairs]
    q3, tn = [_f32(x[5]).reshape(-1, 3) for x in pairs], [_f32(x[6]).reshape(-1, 2) for x in pairs]
    dq = np.ascontiguousarray([x[7] for x in pairs], np.float64).reshape(P, 4)
    dim = next((a.shape[1] for a in qs + ts if a.ndim == 2 and a.shape[0]), 64)
    nq, nt = np.array([q.shape[0] for q in qs], np.int32), np.array([t.shape[0] for t in ts], np.int32)
    nf = np.array([f.shape[0] for f in fl], np.int32)
    max_n = int(max(1, nq.max(), nt.max(), nf.max()))
    cap = max(1, max(c[1] for c in cands) * max_n)
    ptrs = lambda arrs: (_fp * P)(*[_pf(a) if a.shape[0] else None for a in arrs])
    fp = (_vp * P)(*[f.ctypes.data if f.shape[0] else None for f in fl])
    qi, ti, dd, n = np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.float32), np.zeros(P, np.int32)
    kept, nk, mask = np.zeros((P, max_n), np.int32), np.zeros(P, np.int32), np.zeros((P, max_n), np.uint8)
    H, info, status = np.zeros((P, 9), np.float64), np.zeros((P, 4), np.int32), np.zeros(P, np.int32)
    Cn = len(cands)
    X, u = np.zeros((Cn, cap, 3), np.float32), np.zeros((Cn, cap, 2), np.float32)
    n_corr, mdc, gate = (np.full(Cn, -1, np.int32) for _ in range(3))
    new_idx, old_idx, npc = np.zeros((P, max_n), np.int32), np.zeros((P, max_n), np.int32), np.zeros(P, np.int32)
    ip = lambda a: a.ctypes.data_as(_ip)
    cd = _corr_cands(cands)
    _check(lib().omni_bf_match_homography_corr_multi(ctx.h, P, ptrs(qs), ip(nq), ptrs(ts), ip(nt), dim, mode, max_n, ptrs(qx), ptrs(tx), fp, ip(nf), Cn, C.cast(cd, _vp), cap,
                                                     ptrs(q3), ptrs(tn), dq.ctypes.data_as(C.POINTER(C.c_double)), ip(qi), ip(ti), _pf(dd), ip(n), ip(kept), ip(nk),
                                                     mask.ctypes.data, H.ctypes.data_as(C.POINTER(C.c_double)), ip(info), ip(status), _pf(X), _pf(u), ip(n_corr), ip(mdc),
                                                     ip(gate), ip(new_idx), ip(old_idx), ip(npc)))
    hg = [{"q_idx": qi[p, :n[p]].copy(), "t_idx": ti[p, :n[p]].copy(), "dist": dd[p, :n[p]].copy(), "kept": kept[p, :nk[p]].copy(), "mask": mask[p, :nk[p]].copy(),
           "H": H[p].copy(), "info": info[p].copy(), "status": int(status[p])} for p in range(P)]
    return (hg,) + _corr_result(cands, P, n_corr, mdc, gate, X, u, new_idx, old_idx, npc)


def bf_match_batched_dev(ctx: Context, n_pairs, max_n, dim, mode, q_dev, q_stride, nq_dev, t_dev, t_stride, nt_dev,
                         qidx_dev, tidx_dev, dist_dev, n_dev):
    _check(lib().omni_bf_match_batched_dev(ctx.h, n_pairs, max_n, dim, mode, q_dev, q_stride, nq_dev, t_dev, t_stride,
                                           nt_dev, qidx_dev, tidx_dev, dist_dev, n_dev))


def landmarks_dev(ctx: Context, model: StereoModel, poses7_dev, n_pairs, max_num, kps_xy_dev, n_kps_dev, match_up_dev, match_down_dev, n_matches_dev,
                  norm2d_out, l3d_out, flag_out, count_out, camera=None, camera_entry=False):
    """omni_landmarks_enqueue_dev: lifting + up/down triangulation on HBM-resident arrays laid out [up images | down images]; asynchronous on ctx.
    camera: a CameraModel -> omni_landmarks_enqueue_dev_camera (camera_entry=True takes that entry with camera None too: its NULL, the ideal pinhole)"""
    if camera is not None or camera_entry:
        _check(lib().omni_landmarks_enqueue_dev_camera(ctx.h, C.byref(model), C.byref(camera) if camera is not None else None, poses7_dev, n_pairs,
                                                       model.dirs_per_keyframe, max_num, kps_xy_dev, n_kps_dev, match_up_dev, match_down_dev, n_matches_dev, norm2d_out,
                                                       l3d_out, flag_out, count_out))
        return
    _check(lib().omni_landmarks_enqueue_dev(ctx.h, C.byref(model), poses7_dev, n_pairs, model.dirs_per_keyframe, max_num, kps_xy_dev, n_kps_dev, match_up_dev,
                                            match_down_dev, n_matches_dev, norm2d_out, l3d_out, flag_out, count_out))


def landmarks(ctx: Context, model: StereoModel, poses7, kps_xy, n_kps, match_up, match_down, n_matches, camera=None, camera_entry=False) -> dict:
    """host convenience around landmarks_dev (upload, run, download): kps_xy [2P][M][2], n_kps [2P], match_* [P][M], n_matches [P], poses7 [P / dirs][7]"""
    kps_xy, n_kps = _f32(kps_xy), np.ascontiguousarray(n_kps, np.int32)
    P, M = n_kps.shape[0] // 2, kps_xy.shape[1]
    ins = [np.ascontiguousarray(poses7, np.float64), kps_xy, n_kps, np.ascontiguousarray(match_up, np.int32), np.ascontiguousarray(match_down, np.int32),
           np.ascontiguousarray(n_matches, np.int32)]
    assert ins[0].shape == (P // model.dirs_per_keyframe, 7) and kps_xy.shape == (2 * P, M, 2) and ins[3].shape == ins[4].shape == (P, M) and ins[5].shape == (P,)
    outs = [((2 * P, M, 2), np.float32), ((2 * P, M, 3), np.float32), ((2 * P, M), np.uint8), ((P,), np.int32)]
    dev = []
    try:
        for a in ins:
            dev.append(ctx.to_device(a))
        for shape, dt in outs:
            dev.append(ctx.alloc(int(np.prod(shape)) * np.dtype(dt).itemsize))
        landmarks_dev(ctx, model, dev[0], P, M, *dev[1:], camera=camera, camera_entry=camera_entry)
        ctx.sync()
        res = [ctx.from_device(d, shape, dt) for d, (shape, dt) in zip(dev[6:], outs)]
    finally:
        for d in dev:
            ctx.free(d)
    return dict(zip(("norm2d", "landmarks_3d", "landmarks_flag", "count_3d"), res))


def depth_landmarks_dev(ctx: Context, model: DepthModel, poses7_dev, n_images, max_num, kps_xy_dev, n_kps_dev, depth_dev, depth_stride, have_dev, norm2d_out, l3d_out,
                        flag_out, count_out, camera=None):
    """omni_depth_landmarks_enqueue_dev: the depth landmarks of n_images images on HBM-resident arrays; asynchronous on ctx.  camera None: the ideal pinhole"""
    _check(lib().omni_depth_landmarks_enqueue_dev(ctx.h, C.byref(model), C.byref(camera) if camera is not None else None, poses7_dev, n_images, max_num, kps_xy_dev,
                                                  n_kps_dev, depth_dev, depth_stride, have_dev, norm2d_out, l3d_out, flag_out, count_out))


def depth_landmarks(ctx: Context, model: DepthModel, poses7, kps_xy, n_kps, depth, have=None, camera=None, depth_stride: int = 0) -> dict:
    """host convenience around depth_landmarks_dev (upload, run, download): the arguments of depth_landmarks_host"""
    kps_xy, n_kps = _f32(kps_xy), np.ascontiguousarray(n_kps, np.int32)
    N, M = n_kps.shape[0], kps_xy.shape[1]
    d = np.ascontiguousarray(depth, np.uint16)
    ins = [np.ascontiguousarray(poses7, np.float64).reshape(-1, 7), kps_xy, n_kps, d]
    if have is not None:
        ins.append(np.ascontiguousarray(have, np.uint8))
    assert ins[0].shape == (N, 7) and kps_xy.shape == (N, M, 2)
    outs = [((N, M, 2), np.float32), ((N, M, 3), np.float32), ((N, M), np.uint8), ((N,), np.int32)]
    dev, odev = [], []
    try:
        for a in ins:
            dev.append(ctx.to_device(a))
        for shape, dt in outs:
            odev.append(ctx.alloc(int(np.prod(shape)) * np.dtype(dt).itemsize))
        depth_landmarks_dev(ctx, model, dev[0], N, M, dev[1], dev[2], dev[3], depth_stride or d.shape[-1], dev[4] if have is not None else None, *odev, camera=camera)
        ctx.sync()
        res = [ctx.from_device(o, shape, dt) for o, (shape, dt) in zip(odev, outs)]
    finally:
        for x in dev + odev:
            ctx.free(x)
    return dict(zip(("norm2d", "landmarks_3d", "landmarks_flag", "count_3d"), res))


def wire_pack_dev(ctx: Context, n_images, max_num, kps_xy_dev, n_kps_dev, desc_dev, norm2d_dev, l3d_dev, flag_dev, global_dev, meta_dev, packets_out, table_out,
                  send_all_features: bool = False, desc_dim: int = 64, global_dim: int = 4096):
    """omni_wire_pack_enqueue_dev: a unit's HBM-resident arrays -> LoopNet packet buffers and tables (csrc/wire_pack.hip); asynchronous on ctx"""
    _check(lib().omni_wire_pack_enqueue_dev(ctx.h, n_images, max_num, desc_dim, global_dim, int(bool(send_all_features)), kps_xy_dev, n_kps_dev, desc_dev, norm2d_dev,
                                            l3d_dev, flag_dev, global_dev, meta_dev, packets_out, table_out))


def wire_pack_image_dev(ctx: Context, n_images, max_num, kps_xy_dev, n_kps_dev, desc_dev, norm2d_dev, l3d_dev, flag_dev, global_dev, meta_dev, jpeg_dev, jpeg_sizes_dev,
                        jpeg_status_dev, jpeg_capacity, width, height, packets_out, sizes_out, with_features: bool = True, with_image: bool = True, desc_dim: int = 64,
                        global_dim: int = 4096):
    """omni_wire_pack_image_enqueue_dev: a unit's HBM-resident arrays and JPEG files -> whole-descriptor packets (csrc/wire_pack.hip); asynchronous on ctx"""
    _check(lib().omni_wire_pack_image_enqueue_dev(ctx.h, n_images, max_num, desc_dim, global_dim, int(bool(with_features)), int(bool(with_image)), kps_xy_dev, n_kps_dev,
                                                  desc_dev, norm2d_dev, l3d_dev, flag_dev, global_dev, meta_dev, jpeg_dev, jpeg_sizes_dev, jpeg_status_dev, jpeg_capacity,
                                                  width, height, packets_out, sizes_out))


def wire_pack_image(ctx: Context, kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta, jpeg=None, jpeg_sizes=None, jpeg_status=None, width: int = 0, height: int = 0,
                    with_features: bool = True, fill: int = 0):
    """host convenience around wire_pack_image_dev (upload, run, download): the arguments and results of wire_pack_image_host"""
    N, M, ins = _wire_inputs(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta)
    with_image, jp, cap = _wire_jpeg_inputs(N, jpeg, jpeg_sizes, jpeg_status)
    outs = [np.full((N, wire_image_capacity(M, cap)), fill, np.uint8), np.full((N, 2), -1, np.int32)]
    dev = []
    try:
        for a in ins + jp + outs:
            dev.append(ctx.to_device(a.view(np.uint8) if a.dtype == WIRE_META_DTYPE else a))
        wire_pack_image_dev(ctx, N, M, *dev[:8], *(dev[8:11] if with_image else [None] * 3), cap, width, height, *dev[-2:], with_features=with_features,
                            with_image=bool(with_image), desc_dim=ins[2].shape[2], global_dim=ins[6].shape[1])
        ctx.sync()
        res = [ctx.from_device(d, o.shape, o.dtype) for d, o in zip(dev[-2:], outs)]
    finally:
        for x in dev:
            ctx.free(x)
    return res[0], res[1]


def rows_assemble_dev(ctx: Context, n_rows: int, dim: int, table_dev, unit_rows_dev, n_unit_rows: int, staged_rows_dev, n_staged_rows: int, out_dev):
    """omni_rows_assemble_enqueue_dev: the rows of a mixed detector batch gathered into one block (csrc/rows_assemble.hip); asynchronous on ctx"""
    _check(lib().omni_rows_assemble_enqueue_dev(ctx.h, n_rows, dim, table_dev, unit_rows_dev, n_unit_rows, staged_rows_dev, n_staged_rows, out_dev))


def rows_assemble(ctx: Context, table, unit_rows, staged_rows, dim: int, unit_offset_floats: int = 0) -> np.ndarray:
    """host convenience around rows_assemble_dev (upload, run, download): the arguments and result of rows_assemble_host.  The table and the staged rows go up
    through omni_memcpy_h2d_async out of one pinned block, as the detector sends them.  unit_offset_floats: the unit block starts that many floats into its
    allocation (an address off the 16-byte grid takes the dword path)."""
    table, unit_rows, staged_rows = _rows_inputs(table, unit_rows, staged_rows, dim)
    n_rows, tb = len(table), (table.nbytes + 255) // 256 * 256
    pinned = ctx.host_alloc((tb + max(staged_rows.nbytes, 1),), np.uint8)
    dev = []
    try:
        pinned[:table.nbytes] = table.view(np.uint8).reshape(-1)
        pinned[tb:tb + staged_rows.nbytes] = staged_rows.view(np.uint8).reshape(-1)
        dev.append(ctx.alloc(pinned.nbytes))
        _check(lib().omni_memcpy_h2d_async(ctx.h, dev[0], pinned.ctypes.data, pinned.nbytes))
        dev.append(ctx.to_device(np.concatenate([np.zeros(unit_offset_floats, np.float32), unit_rows.reshape(-1)])))
        dev.append(ctx.to_device(np.full((n_rows, dim), np.float32(-7.0))))
        rows_assemble_dev(ctx, n_rows, dim, dev[0], dev[1] + 4 * unit_offset_floats if len(unit_rows) else None, len(unit_rows),
                          dev[0] + tb if len(staged_rows) else None, len(staged_rows), dev[2])
        ctx.sync()
        return ctx.from_device(dev[2], (n_rows, dim), np.float32)
    finally:
        ctx.sync()
        for x in dev:
            ctx.free(x)
        ctx.host_free(pinned)


def wire_pack(ctx: Context, kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta, send_all_features: bool = False, fill: int = 0):
    """host convenience around wire_pack_dev (upload, run, download): the arguments and results of wire_pack_host"""
    N, M, ins = _wire_inputs(kps_xy, n_kps, desc, norm2d, l3d, flag, global_desc, meta)
    outs = [np.full((N, wire_packet_capacity(M)), fill, np.uint8), np.full((N, wire_table_ints(M)), -1, np.int32)]
    dev = []
    try:
        for a in ins + outs:
            dev.append(ctx.to_device(a.view(np.uint8) if a.dtype == WIRE_META_DTYPE else a))
        wire_pack_dev(ctx, N, M, *dev, send_all_features=send_all_features, desc_dim=ins[2].shape[2], global_dim=ins[6].shape[1])
        ctx.sync()
        res = [ctx.from_device(d, o.shape, o.dtype) for d, o in zip(dev[-2:], outs)]
    finally:
        for x in dev:
            ctx.free(x)
    return res[0], res[1]


class Cam:
    """omni_cam: one key frame's CNN + matching work as a single asynchronous unit (LoopCam::on_flattened_images,
    loop_cam.cpp:178-229).  wait() returns numpy VIEWS of the handle's pinned host block (valid until the next enqueue)."""

    def __init__(self, sp: SuperPoint, vlad, n_dirs: int, global_dim: int, bf_mode: int = BF_OPENCV, mono: bool = False):
        """mono: CameraConfig::PINHOLE_DEPTH -- one camera per image (omni_cam_create_mono): n_dirs images, no up/down match"""
        self.sp, self.vlad, self.n, self.cams = sp, vlad, n_dirs, (1 if mono else 2)
        self.n_active = n_dirs
        if mono:
            self.h = lib().omni_cam_create_mono(sp.ctx.h, sp.h, vlad.ctx.h, vlad.h, n_dirs, sp.max_num, global_dim)
        else:
            self.h = lib().omni_cam_create(sp.ctx.h, sp.h, vlad.ctx.h, vlad.h, n_dirs, sp.max_num, global_dim, bf_mode)
        if not self.h:
            raise OmniError(f"omni_cam_create failed: {lib().omni_last_error().decode()}")
        sp.ctx._adopt(self)
        vlad.ctx._adopt(self)
        self._res = _CamResult()

    def close(self):
        if getattr(self, "h", None):
            lib().omni_cam_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue_dev(self, gray_dev: int, stride: int, fisheye_mask: bool = True):
        _check(lib().omni_cam_enqueue_dev(self.h, gray_dev, stride, int(fisheye_mask)))

    def enqueue_host(self, gray_host: np.ndarray, fisheye_mask: bool = True):
        """gray_host [2*n_dirs][H][W] u8 ([n_dirs] for a mono handle), ideally pinned (Context.host_alloc); must stay untouched until wait() returns."""
        assert gray_host.dtype == np.uint8 and gray_host.ndim == 3 and gray_host.shape[0] == self.cams * self.n_active and gray_host.flags.c_contiguous
        _check(lib().omni_cam_enqueue_host(self.h, gray_host.ctypes.data_as(_vp), gray_host.shape[2], gray_host.shape[2], gray_host.shape[1],
                                           int(fisheye_mask)))

    def enqueue_fisheye_dev(self, up: "Flatten", down: "Flatten", up_dev: int, down_dev: int, src_stride: int, n_keyframes: int, first_view: int = 1,
                            fisheye_mask: bool = True):
        """raw fisheye frames in HBM, n_keyframes per camera: flattened inside the unit into views first_view.. of `up` / `down` (omni_cam_enqueue_fisheye_dev)"""
        _check(lib().omni_cam_enqueue_fisheye_dev(self.h, up.h, down.h, up_dev, down_dev, src_stride, n_keyframes, first_view, int(fisheye_mask)))

    def enqueue_fisheye_host(self, up: "Flatten", down: "Flatten", up_host: np.ndarray, down_host: np.ndarray, first_view: int = 1, fisheye_mask: bool = True):
        """up_host / down_host [n_keyframes][src_h][src_w] u8, ideally pinned (Context.host_alloc); must stay untouched until wait() returns."""
        for a in (up_host, down_host):
            assert a.dtype == np.uint8 and a.ndim == 3 and a.flags.c_contiguous and a.shape[0] == up_host.shape[0]
        _check(lib().omni_cam_enqueue_fisheye_host(self.h, up.h, down.h, up_host.ctypes.data_as(_vp), down_host.ctypes.data_as(_vp), up_host.shape[2],
                                                   up_host.shape[0], first_view, int(fisheye_mask)))

    def enqueue_raw_dev(self, resize: "Resize", left_dev: int, right_dev: int, src_stride: int, n_keyframes: int):
        """raw stereo-pinhole frames in HBM, n_keyframes per camera, of the camera's size: resized inside the unit (omni_cam_enqueue_raw_dev)"""
        _check(lib().omni_cam_enqueue_raw_dev(self.h, resize.h, left_dev, right_dev, src_stride, n_keyframes))

    def enqueue_raw_host(self, resize: "Resize", left_host: np.ndarray, right_host: np.ndarray):
        """left_host / right_host [n_keyframes][src_h][src_stride] u8, ideally pinned (Context.host_alloc); must stay untouched until wait() returns."""
        for a in (left_host, right_host):
            assert a.dtype == np.uint8 and a.ndim == 3 and a.flags.c_contiguous and a.shape == left_host.shape and a.shape[1] == resize.src_h
        _check(lib().omni_cam_enqueue_raw_host(self.h, resize.h, left_host.ctypes.data_as(_vp), right_host.ctypes.data_as(_vp), left_host.shape[2], left_host.shape[0]))

    def enqueue_raw_host_parts(self, resize: "Resize", left_parts, right_parts):
        """the same from lists of [k_i][src_h][src_w] arrays per camera (omni_cam_enqueue_raw_host_parts)"""
        def pack(parts):
            for a in parts:
                assert a.dtype == np.uint8 and a.ndim == 3 and a.flags.c_contiguous and a.shape[1:] == (resize.src_h, resize.src_w)
            return (_vp * len(parts))(*[a.ctypes.data for a in parts]), (C.c_int * len(parts))(*[a.shape[0] for a in parts]), len(parts)
        lp, ln, nl = pack(left_parts)
        rp, rn, nr = pack(right_parts)
        _check(lib().omni_cam_enqueue_raw_host_parts(self.h, resize.h, lp, ln, nl, rp, rn, nr, resize.src_w))

    def enqueue_jpeg_host(self, resize, left_files, right_files=None):
        """is_compressed_images: the unit's frames as JPEG files ([bytes] per camera; right_files None for a mono handle), decoded on the GPU inside the unit in
        front of `resize` (None: the files hold network-size pictures).  The files may go on return."""
        def pack(files):
            if files is None:
                return None, None
            return (_vp * len(files))(*[C.cast(C.c_char_p(f), _vp) for f in files]), (C.c_int64 * len(files))(*[len(f) for f in files])
        assert right_files is None or len(right_files) == len(left_files)
        lp, ls = pack(left_files)
        rp, rs = pack(right_files)
        _check(lib().omni_cam_enqueue_jpeg_host(self.h, resize.h if resize is not None else None, lp, ls, rp, rs, len(left_files)))
        self._jdec_frames = None

    def enqueue_fisheye_jpeg_host(self, up: "Flatten", down: "Flatten", up_files, down_files, first_view: int = 1, fisheye_mask: bool = True):
        """enqueue_fisheye_host with each camera's raw frames as JPEG files ([bytes] per camera): decoded and flattened inside the unit
        (omni_cam_enqueue_fisheye_jpeg_host).  The files may go on return; jpegdec_status() after wait() has 2 * len(up_files) entries."""
        assert len(up_files) == len(down_files)
        def pack(files):
            return (_vp * len(files))(*[C.cast(C.c_char_p(f), _vp) for f in files]), (C.c_int64 * len(files))(*[len(f) for f in files])
        up_p, up_s = pack(up_files)
        dn_p, dn_s = pack(down_files)
        _check(lib().omni_cam_enqueue_fisheye_jpeg_host(self.h, up.h, down.h, up_p, up_s, dn_p, dn_s, len(up_files), first_view, int(fisheye_mask)))
        self._jdec_frames = 2 * len(up_files)

    def jpegdec_status(self) -> list:
        """after wait(): the OMNI_JPEGDEC_* status of every frame of that unit, [left frames | right frames] ([up frames | down frames] of a fisheye unit)"""
        n = getattr(self, "_jdec_frames", None) or self.cams * self.n_active
        st = (C.c_int * n)()
        _check(lib().omni_cam_jpegdec_status(self.h, st, n))
        return list(st)

    def get_input(self) -> np.ndarray:
        """[cams * n_active][H][W] u8: the handle's own input block as the last enqueue_host / enqueue_fisheye_* / enqueue_raw_* unit left it (not after enqueue_dev)"""
        out = np.empty((self.cams * self.n_active, self.sp.H, self.sp.W), np.uint8)
        _check(lib().omni_cam_get_input(self.h, out.ctypes.data_as(_vp), out.nbytes))
        return out

    def set_active(self, n_dirs: int):
        """a unit of fewer directions than the handle was created for: the next enqueues read cams * n_dirs images (up cameras first, down right behind)"""
        _check(lib().omni_cam_set_active(self.h, n_dirs))
        self.n_active = n_dirs

    def set_stereo_model(self, model):
        """a StereoModel: every following unit lifts and triangulates its stereo landmarks on the GPU (landmarks() after wait()); None switches it off"""
        _check(lib().omni_cam_set_stereo_model(self.h, C.byref(model) if model is not None else None))
        self._model = model

    def set_poses(self, poses7):
        """pose_drone (xyz + quaternion wxyz) of the key frames of the NEXT unit: [n_keyframes][7]"""
        p = np.ascontiguousarray(poses7, np.float64).reshape(-1, 7)
        _check(lib().omni_cam_set_poses(self.h, p.ctypes.data_as(C.POINTER(C.c_double)), p.shape[0]))

    def set_camera_model(self, camera):
        """a CameraModel: the lens of the stage's lifts (csrc/camera_plan.h); None: the ideal pinhole again.  Kept over set_stereo_model."""
        _check(lib().omni_cam_set_camera_model(self.h, C.byref(camera) if camera is not None else None))

    def set_depth_model(self, model, camera=None):
        """a DepthModel (mono handles): every following unit lifts its key points and reads its depth landmarks on the GPU (landmarks() after wait()); the lens
        (a CameraModel; None: the ideal pinhole) travels with it.  model None switches the stage off.  set_poses and set_depth_host / _dev before every enqueue."""
        _check(lib().omni_cam_set_depth_model(self.h, C.byref(model) if model is not None else None, C.byref(camera) if camera is not None else None))

    def set_depth_host(self, frames, stride: int = 0):
        """the depth frames of the NEXT unit: a list of [H][stride] u16 arrays, None for a key frame without a depth image; copied before the call returns"""
        arrs = [np.ascontiguousarray(f, np.uint16) if f is not None else None for f in frames]
        ptrs = (_vp * len(arrs))(*[a.ctypes.data if a is not None else None for a in arrs])
        st = stride or next((a.shape[-1] for a in arrs if a is not None), 0)
        _check(lib().omni_cam_set_depth_host(self.h, ptrs, st, len(arrs)))

    def set_depth_dev(self, depth_dev: int, stride: int, n_images: int, have=None):
        """the same for frames already in HBM ([n_images][H][stride] u16), borrowed until wait(); have [n_images] or None (all)"""
        hv = np.ascontiguousarray(have, np.uint8) if have is not None else None
        _check(lib().omni_cam_set_depth_dev(self.h, depth_dev, stride, hv.ctypes.data if hv is not None else None, n_images))

    def landmarks(self) -> dict:
        """after wait(): numpy VIEWS of the unit's lifted key points, 3-D landmarks, flags and count_3d (valid until the next enqueue)"""
        r = _CamLandmarks()
        _check(lib().omni_cam_landmarks(self.h, C.byref(r)))
        A = np.ctypeslib.as_array
        ni, n, m = r.n_images, r.n_dirs, r.max_num
        return {"norm2d": A(r.norm2d, (ni, m, 2)), "landmarks_3d": A(r.landmarks_3d, (ni, m, 3)), "landmarks_flag": A(r.landmarks_flag, (ni, m)),
                "count_3d": A(r.count_3d, (n,))}          # (a mono unit with a depth model: n_images == n_dirs, one count per image)

    def set_jpeg(self, quality: int, capacity_per_image: int = 0):
        """send_img: every following unit also encodes its main images as JPEG files (jpeg() after wait()); quality 0 switches it off.
        capacity 0: width * height / 2 per image"""
        _check(lib().omni_cam_set_jpeg(self.h, quality, capacity_per_image or max(self.sp.W * self.sp.H // 2, JPEG_HEADER_BYTES + 2)))

    def jpeg(self) -> list:
        """after wait(): [(status, bytes)] of the unit's main images -- the up / left images of a stereo handle, every image of a mono handle"""
        r = _CamJpeg()
        _check(lib().omni_cam_jpeg(self.h, C.byref(r)))
        A = np.ctypeslib.as_array
        raw, sizes, status = A(r.bytes, (r.n_images, r.capacity)), A(r.sizes, (r.n_images,)), A(r.status, (r.n_images,))
        return [(int(status[i]), raw[i, :sizes[i]].tobytes()) for i in range(r.n_images)]

    def set_wire(self, on: bool, send_all_features: bool = False):
        """the LoopNet wire: every following unit also packs its main images as LoopNet packets (wire() after wait()); needs a landmark model on the handle"""
        _check(lib().omni_cam_set_wire(self.h, int(bool(on)), int(bool(send_all_features))))

    def set_wire_meta(self, records):
        """the records (WIRE_META_DTYPE) of the NEXT unit's main images; copied before the call returns"""
        m = np.ascontiguousarray(records, WIRE_META_DTYPE).reshape(-1)
        _check(lib().omni_cam_set_wire_meta(self.h, m.ctypes.data, len(m)))

    def wire(self):
        """after wait(): numpy VIEWS (packets [n][capacity] u8, table [n][table_ints] i32) of the unit's main images (valid until the next enqueue); wire_packets cuts
        an image's packets out"""
        r = _CamWire()
        _check(lib().omni_cam_wire(self.h, C.byref(r)))
        A = np.ctypeslib.as_array
        return A(r.packets, (r.n_images, r.capacity)), A(r.table, (r.n_images, r.table_ints))

    def jpeg_arrays(self):
        """after wait(): numpy VIEWS (bytes [n][capacity] u8, sizes [n] i32, status [n] i32) of the unit's JPEG stage, as omni_cam_jpeg serves them"""
        r = _CamJpeg()
        _check(lib().omni_cam_jpeg(self.h, C.byref(r)))
        A = np.ctypeslib.as_array
        return A(r.bytes, (r.n_images, r.capacity)), A(r.sizes, (r.n_images,)), A(r.status, (r.n_images,))

    def set_wire_image(self, with_features: bool, with_image: bool):
        """the whole descriptor behind the LoopNet packets of set_wire (wire_image() after wait()): with the 64-d descriptors, with the JPEG file of set_jpeg; both
        False switch it off"""
        _check(lib().omni_cam_set_wire_image(self.h, int(bool(with_features)), int(bool(with_image))))

    def wire_image(self):
        """after wait(): numpy VIEWS (packets [n][capacity] u8, sizes [n][2] i32 = (offset, size)) of the unit's main images (valid until the next enqueue)"""
        r = _CamWireImage()
        _check(lib().omni_cam_wire_image(self.h, C.byref(r)))
        A = np.ctypeslib.as_array
        return A(r.packets, (r.n_images, r.capacity)), A(r.sizes, (r.n_images, 2))

    def ready(self) -> bool:
        r = C.c_int(0)
        _check(lib().omni_cam_ready(self.h, C.byref(r)))
        return bool(r.value)

    def wait(self) -> dict:
        r = self._res
        _check(lib().omni_cam_wait(self.h, C.byref(r)))
        n, m, d, g, ni = r.n_dirs, r.max_num, r.desc_dim, r.global_dim, r.n_images
        A = np.ctypeslib.as_array
        return {"kps_xy": A(r.kps_xy, (ni, m, 2)), "n_kps": A(r.n_kps, (ni,)), "desc": A(r.desc, (ni, m, d)),
                "scores": A(r.scores, (ni, m)), "global_desc": A(r.global_desc, (n, g)), "match_up": A(r.match_up, (n, m)),
                "match_down": A(r.match_down, (n, m)), "match_dist": A(r.match_dist, (n, m)), "n_matches": A(r.n_matches, (n,))}
