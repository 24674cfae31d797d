"""ctypes launcher of the C++ key-frame host loop (host/keyframe_pipeline.hpp -> lib/libomni_host.so).

The loop itself -- SwarmLoop::VIOKF_callback's hot part, swarm_loop/src/swarm_loop.cpp:140-170: LoopCam::on_flattened_images followed
by LoopDetector::on_image_recv, for a stream of key frames -- runs in C++ (omni::KeyframePipeline over the adapters of
host/omni_swarm.hpp and the C ABI of libomni_hip.so).  Python only writes the weight files, owns the pinned input pool and starts the run.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libomni_host.so")
SYMBOLS = ["omni_pipeline_last_error", "omni_pipeline_create", "omni_pipeline_destroy", "omni_pipeline_preload", "omni_pipeline_db_rows",
           "omni_pipeline_run", "omni_pipeline_attach_shard", "omni_pipeline_prepare", "omni_pipeline_geometry_stats", "omni_pipeline_sync",
           "omni_pipeline_set_poses", "omni_pipeline_create_pinhole_depth", "omni_pipeline_set_depth", "omni_pipeline_push_keyframe", "omni_pipeline_flush", "omni_pipeline_host_times", "omni_pipeline_get_candidates", "omni_pipeline_get_edges", "omni_pipeline_get_latencies",
           "omni_pipeline_poll", "omni_pipeline_set_latency", "omni_pipeline_units", "omni_pipeline_get_exchange_us", "omni_swarm_params_from_launch", "omni_swarm_params_table", "omni_pipeline_apply_launch", "omni_pipeline_create_from_launch"]
# CameraConfig::STEREO_PINHOLE's entry points: include/omni_host_stereo.h, lib/libomni_host_stereo.so (the same handle)
STEREO_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_stereo.so")
STEREO_SYMBOLS = ["omni_stereo_last_error", "omni_pipeline_create_stereo_pinhole", "omni_pipeline_set_stereo_extrinsics"]
_lib = None
# where the pipeline computes its stereo landmarks: include/omni_host_landmarks.h, lib/libomni_host_landmarks.so (the same handle)
LANDMARKS_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_landmarks.so")
LANDMARKS_SYMBOLS = ["omni_landmarks_last_error", "omni_pipeline_set_device_landmarks"]
# where the pipeline runs the homography RANSAC of its loop candidates: include/omni_host_homography.h, lib/libomni_host_homography.so (the same handle)
HOMOGRAPHY_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_homography.so")
HOMOGRAPHY_SYMBOLS = ["omni_homography_last_error", "omni_pipeline_set_device_homography", "omni_pipeline_get_device_homography"]
# where the pipeline runs the PnP RANSAC of its loop candidates: include/omni_host_pnp.h, lib/libomni_host_pnp.so (the same handle)
PNP_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_pnp.so")
PNP_SYMBOLS = ["omni_pnp_last_error", "omni_pipeline_set_device_pnp", "omni_pipeline_get_device_pnp", "omni_pipeline_recv_copy_as_remote"]
_stereo_lib = None
_landmarks_lib = None
_homography_lib = None
_pnp_lib = None
JPEG_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_jpeg.so")
JPEG_SYMBOLS = ["omni_jpeg_host_last_error", "omni_pipeline_set_send_img", "omni_pipeline_get_send_img", "omni_pipeline_jpeg_truncated", "omni_pipeline_frame_image"]
_jpeg_lib = None
WIRE_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_wire.so")
WIRE_SYMBOLS = ["omni_wire_host_last_error", "omni_pipeline_set_wire", "omni_pipeline_get_wire", "omni_pipeline_wire_pending", "omni_pipeline_take_packets",
                "omni_pipeline_set_wire_recv", "omni_pipeline_recv_packet", "omni_pipeline_scan_recv", "omni_pipeline_remote_frames", "omni_pipeline_wire_host_ms"]
WIRE_CHANNELS = ("VIOKF_HEADER", "VIOKF_LANDMARKS", "SWARM_LOOP_IMG_DES", "SWARM_LOOP_CONN")      # include/omni_host_wire.h, omni_host_wire_messages.h OMNI_WIRE_CHANNEL_*
_wire_lib = None
WIREMSG_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_wiremsg.so")
WIREMSG_SYMBOLS = ["omni_wiremsg_last_error", "omni_pipeline_set_wire_messages", "omni_pipeline_get_wire_messages", "omni_pipeline_set_wire_accept_img_desc",
                   "omni_pipeline_get_remote_edges", "omni_pipeline_remote_image_pending", "omni_pipeline_take_remote_image"]
WIRE_IMG_OFF, WIRE_IMG_IMAGE, WIRE_IMG_WHOLE, WIRE_IMG_PC_REPLAY = range(4)      # include/omni_host_wire_messages.h OMNI_WIRE_IMG_*
WIRE_IMG_MODES = {"off": 0, "image": 1, "whole": 2, "pc_replay": 3}
WIRE_REMOTE_IMAGES_MAX = 64
REMOTE_EDGE_DTYPE = np.dtype([("id", "<i8"), ("keyframe_id_a", "<i8"), ("keyframe_id_b", "<i8"), ("drone_id_a", "<i4"), ("drone_id_b", "<i4"), ("pnp_inlier_num", "<i4"),
                              ("reserved", "<i4"), ("ts_a", "<f8"), ("ts_b", "<f8"), ("relative_pose", "<f8", (7,)), ("self_pose_a", "<f8", (7,)), ("self_pose_b", "<f8", (7,)),
                              ("pos_cov", "<f8", (3,)), ("ang_cov", "<f8", (3,))])      # omni_remote_edge
_wiremsg_lib = None
# remote key frames joining the unit stream: include/omni_host_remote.h, lib/libomni_host_remote.so (the same handle)
REMOTE_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_remote.so")
REMOTE_SYMBOLS = ["omni_remote_last_error", "omni_pipeline_set_remote_in_stream", "omni_pipeline_get_remote_in_stream", "omni_pipeline_remote_pending",
                  "omni_pipeline_remote_stats", "omni_pipeline_queue_copy_as_remote", "omni_remote_merge_plan"]
_remote_lib = None
# inter-drone loop candidates verified with their batch: include/omni_host_verify.h, lib/libomni_host_verify.so (the same handle)
VERIFY_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_verify.so")
VERIFY_SYMBOLS = ["omni_verify_last_error", "omni_pipeline_set_batch_verify", "omni_pipeline_get_batch_verify", "omni_pipeline_verify_stats", "omni_pipeline_edge_ids", "omni_pipeline_corr_stats", "omni_verify_correspond_host", "omni_verify_plan"]
_verify_lib = None
# pairwise-consistency outlier rejection of the loop edges: include/omni_host_pcm.h, lib/libomni_host_pcm.so (the same handle)
PCM_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_pcm.so")
PCM_SYMBOLS = ["omni_pcm_host_last_error", "omni_pipeline_set_pcm", "omni_pipeline_get_pcm", "omni_pipeline_good_edges", "omni_pipeline_pcm_stats", "omni_pipeline_pcm_records",
               "omni_pcm_filter_host"]
PCM_STATS = ("edges_entered", "pairs_evaluated", "consistent_pairs", "clique_runs", "unknown_frames", "full_handles")
_pcm_lib = None
# the 4-DoF pose graph of the window: include/omni_host_posegraph.h, lib/libomni_host_posegraph.so (the same handle)
POSEGRAPH_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_posegraph.so")
POSEGRAPH_SYMBOLS = ["omni_posegraph_host_last_error", "omni_pipeline_set_pose_graph", "omni_pipeline_get_pose_graph", "omni_pipeline_optimize",
                     "omni_pipeline_estimated_poses", "omni_pipeline_pose_graph_drift", "omni_pipeline_pose_graph_stats", "omni_pipeline_pose_graph_problem",
                     "omni_pose_graph_build_host"]
POSEGRAPH_STATS = ("optimize_calls", "poses", "ego_edges", "loop_edges", "loops_outside", "unreachable_drones", "merged", "best", "status", "iterations", "cg_iterations")
POSEGRAPH_COUNTS = ("ego_edges", "loop_edges", "loops_outside", "unreachable_drones", "merged")
# include/omni_host_posegraph.h omni_pose_graph_frame / omni_pose_graph_keyframe as numpy records
POSE_GRAPH_FRAME_DTYPE = np.dtype([("drone", "<i4"), ("pose_index", "<i4"), ("keyframe_id", "<i8"), ("odom", "<f8", (4,)), ("init", "<f8", (4,)), ("pose", "<f8", (4,))])
POSE_GRAPH_KEYFRAME_DTYPE = np.dtype([("drone", "<i4"), ("reserved", "<i4"), ("keyframe_id", "<i8"), ("pose", "<f8", (7,))])
_posegraph_lib = None
JPEGDEC_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_jpegdec.so")
JPEGDEC_SYMBOLS = ["omni_jpegdec_host_last_error", "omni_pipeline_set_compressed_images", "omni_pipeline_get_compressed_images", "omni_pipeline_jpeg_corrupt",
                   "omni_pipeline_push_keyframe_jpeg", "omni_pipeline_run_jpeg", "omni_swarm_vins_is_compressed_images", "omni_pipeline_apply_vins_settings"]
_jpegdec_lib = None
# STEREO_FISHEYE fed the fisheye camera's own frames: include/omni_host_fisheye.h, lib/libomni_host_fisheye.so (the same handle)
FISHEYE_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_fisheye.so")
FISHEYE_SYMBOLS = ["omni_fisheye_last_error", "omni_pipeline_create_stereo_fisheye_raw", "omni_pipeline_get_fisheye_raw"]
_fisheye_lib = None
# the lens model of the pipeline's lifts and the camodocal file reader: include/omni_host_camera.h, lib/libomni_host_camera.so (the same handle)
CAMERA_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_camera.so")
CAMERA_SYMBOLS = ["omni_camera_last_error", "omni_pipeline_set_camera_model", "omni_pipeline_get_camera_model", "omni_camera_from_yaml",
                  "omni_pipeline_create_from_launch_camera", "omni_pipeline_frame_landmarks"]
_camera_lib = None
# where the pipeline reads PINHOLE_DEPTH's depth landmarks: include/omni_host_depth.h, lib/libomni_host_depth.so (the same handle)
DEPTH_LIB_PATH = os.path.join(_HERE, "lib", "libomni_host_depth.so")
DEPTH_SYMBOLS = ["omni_depth_last_error", "omni_pipeline_set_device_depth_landmarks", "omni_pipeline_get_device_depth_landmarks"]
_depth_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        capi.lib()                                     # libomni_hip.so first (libomni_host.so links against it)
        L = C.CDLL(LIB_PATH)
        L.omni_pipeline_last_error.restype = C.c_char_p
        L.omni_pipeline_create.restype = C.c_void_p
        L.omni_pipeline_create.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        L.omni_pipeline_create_pinhole_depth.restype = C.c_void_p
        L.omni_pipeline_create_pinhole_depth.argtypes = L.omni_pipeline_create.argtypes + [C.c_double] * 6 + [C.c_int]
        L.omni_pipeline_set_depth.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.omni_pipeline_push_keyframe.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_double, C.POINTER(C.c_double), C.c_int, C.c_void_p,
                                                  C.POINTER(C.c_int)]
        L.omni_pipeline_flush.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_poll.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_set_latency.argtypes = [C.c_void_p, C.c_double, C.c_int]
        L.omni_pipeline_units.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_get_exchange_us.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int]
        L.omni_swarm_params_from_launch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.omni_pipeline_apply_launch.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.omni_swarm_params_table.argtypes = [C.c_char_p, C.c_int]
        L.omni_pipeline_create_from_launch.restype = C.c_void_p
        L.omni_pipeline_create_from_launch.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.omni_pipeline_host_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        L.omni_pipeline_geometry_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_destroy.argtypes = [C.c_void_p]
        L.omni_pipeline_destroy.restype = None
        L.omni_pipeline_preload.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
        L.omni_pipeline_db_rows.argtypes = [C.c_void_p]
        L.omni_pipeline_db_rows.restype = C.c_int64
        L.omni_pipeline_run.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int)]
        L.omni_pipeline_sync.argtypes = [C.c_void_p]
        L.omni_pipeline_attach_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
        L.omni_pipeline_prepare.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_set_poses.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_double)]
        L.omni_pipeline_get_candidates.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        L.omni_pipeline_get_edges.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        L.omni_pipeline_get_latencies.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int]
        _lib = L
    return _lib


def stereo_lib():
    global _stereo_lib
    if _stereo_lib is None:
        if not os.path.exists(STEREO_LIB_PATH):
            raise OSError(f"{STEREO_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        lib()
        L = C.CDLL(STEREO_LIB_PATH)
        L.omni_stereo_last_error.restype = C.c_char_p
        L.omni_pipeline_create_stereo_pinhole.restype = C.c_void_p
        L.omni_pipeline_create_stereo_pinhole.argtypes = lib().omni_pipeline_create.argtypes + [C.c_double] * 4 + [C.c_int, C.c_int, C.c_double, C.c_int]
        L.omni_pipeline_set_stereo_extrinsics.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _stereo_lib = L
    return _stereo_lib


def fisheye_lib():
    """libomni_host_fisheye.so (include/omni_host_fisheye.h): the raw-fisheye mode of the key-frame pipeline"""
    global _fisheye_lib
    if _fisheye_lib is None:
        if not os.path.exists(FISHEYE_LIB_PATH):
            raise OSError(f"{FISHEYE_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        lib()
        L = C.CDLL(FISHEYE_LIB_PATH)
        L.omni_fisheye_last_error.restype = C.c_char_p
        L.omni_pipeline_create_stereo_fisheye_raw.restype = C.c_void_p
        L.omni_pipeline_create_stereo_fisheye_raw.argtypes = lib().omni_pipeline_create.argtypes + [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                                                                  C.c_int]
        L.omni_pipeline_get_fisheye_raw.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _fisheye_lib = L
    return _fisheye_lib


def _err(what):
    return capi.OmniError(f"{what}: {lib().omni_pipeline_last_error().decode()}")


def swarm_params_from_launch(launch_xml: str, node_name: str = "swarm_loop", args: dict | None = None):
    """The node's parameters as one of the reference's launch files sets them (host/swarm_loop_params.hpp; no ROS): -> (dict name -> value text,
    names whose stored type nh.param<T> refuses (defaults kept), names the node never reads)."""
    buf = C.create_string_buffer(1 << 16)
    a = "\n".join(f"{k}:={v}" for k, v in (args or {}).items()).encode() or None
    if lib().omni_swarm_params_from_launch(launch_xml.encode(), node_name.encode(), a, buf, len(buf)):
        raise _err("omni_swarm_params_from_launch")
    vals, mism, unk = {}, [], []
    for line in buf.value.decode().splitlines():
        if line.startswith("#mismatch "):
            mism.append(line[10:])
        elif line.startswith("#unknown "):
            unk.append(line[9:])
        else:
            k, _, v = line.partition("=")
            vals[k] = v
    return vals, mism, unk


def swarm_params_table():
    """[(name, 'I' | 'B' | 'D' | 'S', default text)]: every parameter SwarmLoop::Init reads, in its order (host/swarm_loop_params.hpp)"""
    buf = C.create_string_buffer(1 << 16)
    if lib().omni_swarm_params_table(buf, len(buf)):
        raise _err("omni_swarm_params_table")
    return [tuple(l.split("\t")) if l.count("\t") == 2 else tuple(l.split("\t")) + ("",) for l in buf.value.decode().split("\n") if l]


def landmarks_lib():
    global _landmarks_lib
    if _landmarks_lib is None:
        lib()                                   # (libomni_hip.so / OMNI_LIB first, as for the other host libraries)
        if not os.path.exists(LANDMARKS_LIB_PATH):
            raise OSError(f"{LANDMARKS_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(LANDMARKS_LIB_PATH)
        L.omni_landmarks_last_error.restype = C.c_char_p
        L.omni_pipeline_set_device_landmarks.argtypes = [C.c_void_p, C.c_int]
        _landmarks_lib = L
    return _landmarks_lib


def depth_lib():
    global _depth_lib
    if _depth_lib is None:
        lib()                                   # (libomni_hip.so / OMNI_LIB first, as for the other host libraries)
        if not os.path.exists(DEPTH_LIB_PATH):
            raise OSError(f"{DEPTH_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(DEPTH_LIB_PATH)
        L.omni_depth_last_error.restype = C.c_char_p
        L.omni_pipeline_set_device_depth_landmarks.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_device_depth_landmarks.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        _depth_lib = L
    return _depth_lib


PCA_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libomni_host_pca.so")
PCA_SYMBOLS = ["omni_pca_host_last_error", "omni_pipeline_set_fit_pca", "omni_pipeline_get_fit_pca", "omni_pipeline_pca_fit_stats", "omni_pipeline_pca_fit_moments",
               "omni_pipeline_pca_fit_solve", "omni_pipeline_pca_fit_write", "omni_pipeline_pca_fit_reset"]
_pca_lib = None


def pca_lib():
    """libomni_host_pca.so (include/omni_host_pca.h): the PCA fit of the key-frame pipeline's descriptor stream"""
    global _pca_lib
    if _pca_lib is None:
        lib()
        if not os.path.exists(PCA_LIB_PATH):
            raise OSError(f"{PCA_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(PCA_LIB_PATH)
        dp, fp, ip64 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)
        L.omni_pca_host_last_error.restype = C.c_char_p
        L.omni_pipeline_set_fit_pca.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_fit_pca.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_pca_fit_stats.argtypes = [C.c_void_p, ip64, ip64]
        L.omni_pipeline_pca_fit_moments.argtypes = [C.c_void_p, ip64, ip64, dp, dp]
        L.omni_pipeline_pca_fit_solve.argtypes = [C.c_void_p, C.c_int, dp, fp, dp, fp, dp, dp]
        L.omni_pipeline_pca_fit_write.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
        L.omni_pipeline_pca_fit_reset.argtypes = [C.c_void_p]
        _pca_lib = L
    return _pca_lib


def camera_lib():
    """libomni_host_camera.so (include/omni_host_camera.h): the lens model of the key-frame pipeline, the camodocal file reader"""
    global _camera_lib
    if _camera_lib is None:
        lib()
        if not os.path.exists(CAMERA_LIB_PATH):
            raise OSError(f"{CAMERA_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(CAMERA_LIB_PATH)
        L.omni_camera_last_error.restype = C.c_char_p
        L.omni_pipeline_set_camera_model.argtypes = [C.c_void_p, C.POINTER(capi.CameraModel), C.POINTER(C.c_double)]
        L.omni_pipeline_get_camera_model.argtypes = [C.c_void_p, C.POINTER(capi.CameraModel), C.POINTER(C.c_double)]
        L.omni_camera_from_yaml.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(capi.CameraModel), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.omni_pipeline_create_from_launch_camera.restype = C.c_void_p
        L.omni_pipeline_create_from_launch_camera.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                              C.c_int, C.c_int, C.c_int, C.c_char_p]
        L.omni_pipeline_frame_landmarks.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _camera_lib = L
    return _camera_lib


_CAMERA_NAMES = {v: k for k, v in capi.CAMERA_TYPES.items()}


def _camera_struct(camera_model) -> capi.CameraModel:
    """a capi.CameraModel, or a dict(type=, k1=, k2=, p1=, p2=, xi=) with type "PINHOLE" / "MEI" (or 0 / 1)"""
    if isinstance(camera_model, capi.CameraModel):
        return camera_model
    d = dict(camera_model)
    extra = set(d) - {"type", "k1", "k2", "p1", "p2", "xi", "intrinsics", "image_size"}
    if extra:
        raise ValueError(f"camera_model: unknown entries {sorted(extra)}")
    return capi.camera_model(d.get("type", capi.CAMERA_PINHOLE), d.get("k1", 0.0), d.get("k2", 0.0), d.get("p1", 0.0), d.get("p2", 0.0), d.get("xi", 0.0))


def camera_from_yaml(text: str, width: int = 0, height: int = 0) -> dict:
    """the camodocal file the node's camera_config_path names (its TEXT): dict(type="PINHOLE" | "MEI", k1, k2, p1, p2, xi, intrinsics=[fx, fy, cx, cy] -- MEI:
    gamma1 gamma2 u0 v0 --, image_size=(image_width, image_height)).  width, height > 0: the intrinsics scaled to images of that size.  The dict is what
    KeyframePipeline(camera_model=) and set_camera_model take."""
    m, k, wh = capi.CameraModel(), (C.c_double * 4)(), (C.c_int * 2)()
    if camera_lib().omni_camera_from_yaml(text.encode(), int(width), int(height), C.byref(m), k, wh):
        raise capi.OmniError(f"omni_camera_from_yaml: {camera_lib().omni_camera_last_error().decode()}")
    return {"type": _CAMERA_NAMES[m.type], "k1": m.k1, "k2": m.k2, "p1": m.p1, "p2": m.p2, "xi": m.xi, "intrinsics": list(k), "image_size": (wh[0], wh[1])}


def homography_lib():
    global _homography_lib
    if _homography_lib is None:
        lib()
        if not os.path.exists(HOMOGRAPHY_LIB_PATH):
            raise OSError(f"{HOMOGRAPHY_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(HOMOGRAPHY_LIB_PATH)
        L.omni_homography_last_error.restype = C.c_char_p
        L.omni_pipeline_set_device_homography.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_device_homography.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _homography_lib = L
    return _homography_lib


def pnp_lib():
    global _pnp_lib
    if _pnp_lib is None:
        lib()
        if not os.path.exists(PNP_LIB_PATH):
            raise OSError(f"{PNP_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(PNP_LIB_PATH)
        L.omni_pnp_last_error.restype = C.c_char_p
        L.omni_pipeline_set_device_pnp.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_device_pnp.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_recv_copy_as_remote.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        _pnp_lib = L
    return _pnp_lib


def jpegdec_lib():
    """libomni_host_jpegdec.so (include/omni_host_jpegdec.h): is_compressed_images of the key-frame pipeline"""
    global _jpegdec_lib
    if _jpegdec_lib is None:
        lib()                                                    # (libomni_host.so first: the handle's type lives there)
        L = C.CDLL(JPEGDEC_LIB_PATH)
        L.omni_jpegdec_host_last_error.restype = C.c_char_p
        L.omni_pipeline_set_compressed_images.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_compressed_images.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_jpeg_corrupt.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_pipeline_push_keyframe_jpeg.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int64, C.c_double, C.POINTER(C.c_double), C.c_int,
                                                       C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_run_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.omni_swarm_vins_is_compressed_images.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        L.omni_pipeline_apply_vins_settings.argtypes = [C.c_void_p, C.c_char_p]
        _jpegdec_lib = L
    return _jpegdec_lib


def vins_is_compressed_images(vins_yaml_text: str) -> bool:
    """is_compressed_images of the VINS settings file the node's vins_config_path names (False when the key is absent)"""
    return bool(jpegdec_lib().omni_swarm_vins_is_compressed_images(vins_yaml_text.encode(), None))


def jpeg_lib():
    global _jpeg_lib
    if _jpeg_lib is None:
        lib()
        if not os.path.exists(JPEG_LIB_PATH):
            raise OSError(f"{JPEG_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(JPEG_LIB_PATH)
        L.omni_jpeg_host_last_error.restype = C.c_char_p
        L.omni_pipeline_set_send_img.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.omni_pipeline_get_send_img.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_jpeg_truncated.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_pipeline_frame_image.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        _jpeg_lib = L
    return _jpeg_lib


def wire_lib():
    global _wire_lib
    if _wire_lib is None:
        lib()
        if not os.path.exists(WIRE_LIB_PATH):
            raise OSError(f"{WIRE_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(WIRE_LIB_PATH)
        L.omni_wire_host_last_error.restype = C.c_char_p
        L.omni_pipeline_set_wire.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.omni_pipeline_get_wire.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_wire_pending.argtypes = [C.c_void_p]
        L.omni_pipeline_wire_pending.restype = C.c_int64
        L.omni_pipeline_take_packets.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.POINTER(C.c_int)]
        L.omni_pipeline_set_wire_recv.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
        L.omni_pipeline_recv_packet.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_double, C.POINTER(C.c_int)]
        L.omni_pipeline_scan_recv.argtypes = [C.c_void_p, C.c_double]
        L.omni_pipeline_remote_frames.argtypes = [C.c_void_p]
        L.omni_pipeline_remote_frames.restype = C.c_int64
        L.omni_pipeline_wire_host_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        _wire_lib = L
    return _wire_lib


def pcm_lib():
    global _pcm_lib
    if _pcm_lib is None:
        lib()
        if not os.path.exists(PCM_LIB_PATH):
            raise OSError(f"{PCM_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(PCM_LIB_PATH)
        L.omni_pcm_host_last_error.restype = C.c_char_p
        L.omni_pipeline_set_pcm.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int]
        L.omni_pipeline_get_pcm.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_good_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.omni_pipeline_pcm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_pipeline_pcm_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.omni_pcm_filter_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(capi.PcmParams), C.c_void_p, C.POINTER(C.c_int64)]
        _pcm_lib = L
    return _pcm_lib


def posegraph_lib():
    global _posegraph_lib
    if _posegraph_lib is None:
        lib()
        if not os.path.exists(POSEGRAPH_LIB_PATH):
            raise OSError(f"{POSEGRAPH_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(POSEGRAPH_LIB_PATH)
        ip = C.POINTER(C.c_int)
        L.omni_posegraph_host_last_error.restype = C.c_char_p
        L.omni_pipeline_set_pose_graph.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.omni_pipeline_get_pose_graph.argtypes = [C.c_void_p, ip, ip, ip]
        L.omni_pipeline_optimize.argtypes = [C.c_void_p, ip]
        L.omni_pipeline_estimated_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ip]
        L.omni_pipeline_pose_graph_drift.argtypes = [C.c_void_p, C.POINTER(C.c_double), ip]
        L.omni_pipeline_pose_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.omni_pipeline_pose_graph_problem.argtypes = [C.c_void_p, ip, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.PgoParams)]
        L.omni_pose_graph_build_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, ip,
                                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip]
        _posegraph_lib = L
    return _posegraph_lib


def pose_graph_build_host(keyframes, loops, self_id: int, window: int = 50, starts: int = 1, pos_covariance_per_meter: float = 0.01, yaw_covariance_per_meter: float = 0.003):
    """host/pose_graph.hpp without a pipeline and without a GPU: keyframes (POSE_GRAPH_KEYFRAME_DTYPE, in the order seen) and loops (REMOTE_EDGE_DTYPE, in order) ->
    dict(frames POSE_GRAPH_FRAME_DTYPE, poses [starts][n][4], fixed [n], edges capi.PGO_EDGE_DTYPE, and the counts of POSEGRAPH_COUNTS)"""
    kf = np.ascontiguousarray(keyframes, dtype=POSE_GRAPH_KEYFRAME_DTYPE).reshape(-1)
    lp = np.ascontiguousarray(loops, dtype=REMOTE_EDGE_DTYPE).reshape(-1)
    L = posegraph_lib()
    n_frames, sizes, counts = C.c_int(0), (C.c_int * 3)(), (C.c_int * 5)()

    def call(frames, poses, fixed, edges):
        rc = L.omni_pose_graph_build_host(self_id, window, starts, pos_covariance_per_meter, yaw_covariance_per_meter, kf.ctypes.data if len(kf) else None, len(kf),
                                          lp.ctypes.data if len(lp) else None, len(lp), frames.ctypes.data if frames is not None and len(frames) else None,
                                          0 if frames is None else len(frames), C.byref(n_frames), sizes, None if poses is None else poses.ctypes.data,
                                          None if fixed is None else fixed.ctypes.data, 0 if fixed is None else len(fixed), None if edges is None else edges.ctypes.data,
                                          0 if edges is None else len(edges), counts)
        if rc:
            raise capi.OmniError(f"omni_pose_graph_build_host: {L.omni_posegraph_host_last_error().decode()}")

    call(None, None, None, None)
    frames = np.zeros(n_frames.value, POSE_GRAPH_FRAME_DTYPE)
    poses, fixed, edges = np.zeros((sizes[2], sizes[0], 4)), np.zeros(max(sizes[0], 1), np.uint8), np.zeros(max(sizes[1], 1), capi.PGO_EDGE_DTYPE)
    call(frames, poses, fixed, edges)
    return dict(frames=frames, poses=poses, fixed=fixed[:sizes[0]], edges=edges[:sizes[1]], **dict(zip(POSEGRAPH_COUNTS, (int(v) for v in counts))))


def pcm_filter_host(edges, self_id: int, batches=None, redundant: bool = False, capacity: int = capi.PCM_DEFAULT_CAPACITY, params=None):
    """host/loop_outlier_rejection.hpp with its rows from omni_pcm_rows_host (no GPU): capi.PCM_EDGE_DTYPE records enter in calls of batches[0], batches[1], ..
    edges (None: one call).  Returns (good [n] bool: whether edge k passes afterwards, stats dict)."""
    e = np.ascontiguousarray(edges, dtype=capi.PCM_EDGE_DTYPE).reshape(-1)
    good = np.zeros(max(len(e), 1), np.uint8)
    st = (C.c_int64 * 6)()
    b = None if batches is None else np.ascontiguousarray(batches, np.int32)
    pr = params or capi.pcm_params()
    if pcm_lib().omni_pcm_filter_host(e.ctypes.data, len(e), None if b is None else b.ctypes.data, 0 if b is None else len(b), self_id, int(bool(redundant)), capacity,
                                      C.byref(pr), good.ctypes.data, st):
        raise capi.OmniError(f"omni_pcm_filter_host: {pcm_lib().omni_pcm_host_last_error().decode()}")
    return good[:len(e)].astype(bool), dict(zip(PCM_STATS, (int(v) for v in st)))


def wiremsg_lib():
    global _wiremsg_lib
    if _wiremsg_lib is None:
        lib()
        if not os.path.exists(WIREMSG_LIB_PATH):
            raise OSError(f"{WIREMSG_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(WIREMSG_LIB_PATH)
        L.omni_wiremsg_last_error.restype = C.c_char_p
        L.omni_pipeline_set_wire_messages.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.omni_pipeline_get_wire_messages.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.omni_pipeline_set_wire_accept_img_desc.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_remote_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.omni_pipeline_remote_image_pending.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_pipeline_remote_image_pending.restype = C.c_int64
        L.omni_pipeline_take_remote_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _wiremsg_lib = L
    return _wiremsg_lib


def remote_lib():
    global _remote_lib
    if _remote_lib is None:
        if not os.path.exists(REMOTE_LIB_PATH):
            raise OSError(f"{REMOTE_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(REMOTE_LIB_PATH)
        L.omni_remote_last_error.restype = C.c_char_p
        L.omni_pipeline_set_remote_in_stream.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_remote_in_stream.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_remote_pending.argtypes = [C.c_void_p]
        L.omni_pipeline_remote_pending.restype = C.c_int64
        L.omni_pipeline_remote_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_pipeline_queue_copy_as_remote.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64]
        L.omni_remote_merge_plan.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        _remote_lib = L
    return _remote_lib


def remote_merge_plan(a: int, b: int, queue_p):
    """host/remote_queue.hpp's order rule, no pipeline and no GPU: the detector batch of a unit that covers the local hand-over numbers [a, b), given p of the queued
    remote frames in arrival order -> ([(is_remote, index), ...] in detector order, queue entries taken from the front)"""
    p = np.ascontiguousarray(queue_p, np.int64)
    cap = max(b - a, 0) + len(p)
    rem, idx = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int64)
    n, taken = C.c_int64(0), C.c_int64(0)
    if remote_lib().omni_remote_merge_plan(a, b, p.ctypes.data if len(p) else None, len(p), rem.ctypes.data, idx.ctypes.data, cap, C.byref(n), C.byref(taken)):
        raise capi.OmniError(f"omni_remote_merge_plan: {remote_lib().omni_remote_last_error().decode()}")
    return [(bool(rem[s]), int(idx[s])) for s in range(n.value)], taken.value


def verify_lib():
    global _verify_lib
    if _verify_lib is None:
        if not os.path.exists(VERIFY_LIB_PATH):
            raise OSError(f"{VERIFY_LIB_PATH} is missing: run `make -C omni-swarm_amd`")
        L = C.CDLL(VERIFY_LIB_PATH)
        L.omni_verify_last_error.restype = C.c_char_p
        L.omni_pipeline_set_batch_verify.argtypes = [C.c_void_p, C.c_int]
        L.omni_pipeline_get_batch_verify.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.omni_pipeline_verify_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_pipeline_edge_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.omni_pipeline_edge_ids.restype = C.c_int64
        L.omni_pipeline_corr_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.omni_verify_correspond_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11
        L.omni_verify_plan.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int]
        _verify_lib = L
    return _verify_lib


def verify_plan(self_id: int, T: int, drone, partner, partner_init, verdict, batch_len, n_drones: int):
    """host/verify_plan.hpp's certainty rule over a stream of frames cut into detector batches, no pipeline and no GPU (include/omni_host_verify.h has the
    arguments) -> (init_mode per frame, resolved_before per frame, end_resolve per batch, inter_drone_loop_count[{x, self_id}] per drone x)"""
    dr, pa, pi = (np.ascontiguousarray(v, np.int32) for v in (drone, partner, partner_init))
    ve, bl = np.ascontiguousarray(verdict, np.uint8), np.ascontiguousarray(batch_len, np.int64)
    n, nb = len(dr), len(bl)
    if not (len(pa) == len(pi) == len(ve) == n):
        raise ValueError("verify_plan: one partner, partner_init and verdict per frame")
    im, rb, er, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(nb, 1), np.int32), np.zeros(max(n_drones, 1), np.int64)
    if verify_lib().omni_verify_plan(self_id, T, n, dr.ctypes.data, pa.ctypes.data, pi.ctypes.data, ve.ctypes.data, bl.ctypes.data, nb, im.ctypes.data, rb.ctypes.data,
                                     er.ctypes.data, cnt.ctypes.data, n_drones):
        raise capi.OmniError(f"omni_verify_plan: {verify_lib().omni_verify_last_error().decode()}")
    return [bool(v) for v in im[:n]], [bool(v) for v in rb[:n]], [bool(v) for v in er[:nb]], [int(v) for v in cnt[:n_drones]]


def verify_correspond_host(cands, pairs, cand: int, max_dirs: int, main_dir_new: int, main_dir_old: int, step_present, old_quat):
    """LoopGeometry::compute_correspond_features on two frames built from candidate `cand` (omni_verify_correspond_host; cands and pairs as capi.CorrArrays takes
    them, the pairs' dq_old ignored) -> {dq_old [pair_count][4], n_corr, result, size_gate, X [n][3], u [n][2], new_idx, old_idx (per pair)}"""
    a = capi.CorrArrays(cands, pairs)
    pc = cands[cand][1]
    sp, oq = np.ascontiguousarray(step_present, np.uint8), np.ascontiguousarray(old_quat, np.float64).reshape(max_dirs, 4)
    dq, X, u = np.zeros((max(pc, 1), 4), np.float64), np.zeros((a.cap, 3), np.float32), np.zeros((a.cap, 2), np.float32)
    n, res, gate = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    ni, oi, npc = np.zeros((max(pc, 1), a.max_n), np.int32), np.zeros((max(pc, 1), a.max_n), np.int32), np.zeros(max(pc, 1), np.int32)
    if verify_lib().omni_verify_correspond_host(C.addressof(a.io), cand, max_dirs, main_dir_new, main_dir_old, sp.ctypes.data, oq.ctypes.data, dq.ctypes.data, X.ctypes.data,
                                                u.ctypes.data, C.addressof(n), C.addressof(res), C.addressof(gate), ni.ctypes.data, oi.ctypes.data, npc.ctypes.data):
        raise capi.OmniError(f"omni_verify_correspond_host: {verify_lib().omni_verify_last_error().decode()}")
    return {"dq_old": dq[:pc], "n_corr": n.value, "result": bool(res.value), "size_gate": bool(gate.value), "X": X[:n.value].copy(), "u": u[:n.value].copy(),
            "new_idx": [ni[j, :npc[j]].copy() for j in range(pc)], "old_idx": [oi[j, :npc[j]].copy() for j in range(pc)]}


class KeyframePipeline:
    def __init__(self, device: int, sp_weights_path: str, pca_comp_csv: str, pca_mean_csv: str, vlad_weights_path: str, width=600, height=480,
                 thres=0.02, max_num=200, precision=capi.PREC_F16, microbatch=8, pipelines=0, storage=capi.STORE_F32, self_id=1,
                 inner_product_thres=0.3, init_mode_product_thres=0.2, match_index_dist=5, min_loop_num=30, min_direction_loop=3, geometry=False, pinhole_depth=None,
                 stereo_pinhole=None, device_landmarks=None, device_homography=None, send_img=False, jpg_quality=50, device_pnp=None, compressed_images=False, raw_fisheye=None, camera_model=None,
                 device_depth_landmarks=None, fit_pca=False, wire=False, device_wire=False, send_all_features=False, remote_in_stream=False, batch_verify=False,
                 wire_img_desc="off", wire_loop_conn=False, pcm=False, pcm_thres=0.6, pcm_redundant=False, pcm_capacity=capi.PCM_DEFAULT_CAPACITY,
                 pose_graph=False, pose_graph_window=50, pose_graph_starts=1):
        """pinhole_depth: None = CameraConfig::STEREO_FISHEYE (4 directions x up/down views per key frame); a dict(fx, fy, cx, cy, depth_near, depth_far,
        accept_min_3d_pts) = CameraConfig::PINHOLE_DEPTH (launch/realsense.launch): one gray image + one depth image (set_depth) per key frame.
        stereo_pinhole: a dict(fx, fy, cx, cy[, src_width, src_height, triangle_thres, accept_min_3d_pts]) = CameraConfig::STEREO_PINHOLE: a left and a right
        frame per key frame, of src_width x src_height (the camera's size: resized to width x height inside every unit, on the GPU) or, without them, of
        the networks' size; fx fy cx cy are those of the width x height image.  set_stereo_extrinsics gives the rig's two extrinsics.
        device_landmarks: True / False = the stereo landmarks of a `geometry` pipeline inside the key-frame unit on the GPU / on the host's geometry
        threads (the same bits either way); None: the library's default.
        device_homography: True / False = the homography RANSAC of a `geometry` pipeline's loop candidates on the GPU, in the round trip that matches their
        direction pairs / on the host's geometry threads (the same masks either way); None: the library's default.
        device_pnp: True / False = the EPnP RANSAC of a `geometry` pipeline's loop candidates on the GPU, one call per candidate / on the host's geometry
        threads (the same edges either way); None: the library's default, which is off.
        send_img / jpg_quality: the reference's switch of the same name (default off, quality 50): the main image of every direction goes into its message as a
        JPEG file, encoded inside the key-frame unit on the GPU (set_send_img).
        raw_fisheye: a dict(src_width, src_height, fov_deg, mei_up, mei_down[, first_view]) = CameraConfig::STEREO_FISHEYE fed the fisheye camera's own frames:
        ONE up frame and ONE down frame of src_width x src_height per key frame, flattened into the four side views (width x height) inside every unit, on the
        GPU; mei_up / mei_down: the cameras' nine MEI parameters as flatten.generate_undist_maps takes them.  With compressed_images the two frames are JPEG
        files (push_keyframe_jpeg, run_jpeg).  The reference has no such path: its upstream (VINS-Fisheye) flattens.
        camera_model: a dict(type="PINHOLE" | "MEI", k1=, k2=, p1=, p2=, xi=) (what camera_from_yaml returns; its "intrinsics", when present, replace fx fy cx cy)
        or a capi.CameraModel = the lens behind the intrinsics, as the reference's camodocal file describes it: every lift -- landmarks_2d_norm, the triangulation on
        either path, PINHOLE_DEPTH's depth landmarks -- undoes it (csrc/camera_plan.h).  None: the ideal pinhole.  Refused in the raw_fisheye mode.
        device_depth_landmarks: True / False = PINHOLE_DEPTH's lifted key points and depth landmarks of a `geometry` pipeline inside the key-frame unit on the GPU
        (every depth image is then copied at push_keyframe / read when run() enqueues its unit) / on the calling thread (the same bits either way); None: the
        library's default, which is off.  Refused for the stereo configurations.
        fit_pca: the reference's OUTPUT_RAW_SUPERPOINT_DESC as a calibration mode: the 256-d descriptors of every key point of the stream enter the moments of
        a PCA fit on the GPU (csrc/pca_fit.hip); pca_fit / pca_fit_write make components_.csv / mean_.csv of them.  Results do not depend on it.  Default off.
        wire / device_wire / send_all_features: the LoopNet wire (set_wire): every finished key frame leaves as LoopNet's packets (take_packets) and packets of
        other drones enter through recv_packet / scan_recv; device_wire packs the packets inside the key-frame unit on the GPU (the same bytes).  Default off.
        wire_img_desc / wire_loop_conn: LoopNet's other two message kinds on that wire (set_wire_messages).  "image" / "whole" / "pc_replay": an image's whole
        descriptor leaves behind its landmark packets without its 64-d descriptors and with its JPEG file (needs send_img) / with the descriptors, and with the
        file when send_img is on / alone; with device_wire it is packed inside the unit too.  wire_loop_conn: every accepted edge leaves as a packet of its own,
        and edges of other drones arrive in remote_edges().  Default off.
        remote_in_stream: key frames of other drones (the wire's, or queue_copy_as_remote's) are queued and join the next key-frame unit's detector batch at
        their place in the serial order, their rows gathered with the unit's on the GPU (csrc/rows_assemble.hip), instead of stopping the pipeline with a flush
        each; the same candidates, edges and rows (set_remote_in_stream).  Default off.
        batch_verify: loop candidates between a frame of another drone and a frame of this one are verified with their detector batch, in one GPU round trip,
        instead of one by one on the spot; earlier only where a remote frame's init mode depends on a pending verdict (host/verify_plan.hpp).  The same
        candidates, edges and counters (set_batch_verify, verify_stats).  Independent of remote_in_stream.  Default off.
        pcm / pcm_thres / pcm_redundant / pcm_capacity: pairwise-consistency outlier rejection of the loop edges of a `geometry` pipeline (set_pcm): every edge
        that enters edges() or remote_edges() is compared with every earlier edge of its drone pair on the GPU (csrc/pcm.hip), a clique heuristic picks each
        pair's inlier set, and good_edges() lists what is left; edges(), candidates, counters and rows are unchanged.  Default off.
        pipelines <= 0: the library's default number of units in flight for the precision (4 for fp16, 2 otherwise)"""
        self.microbatch = microbatch
        common = (device, sp_weights_path.encode(), pca_comp_csv.encode(), pca_mean_csv.encode(), vlad_weights_path.encode(), width, height, thres, max_num,
                  precision, microbatch, pipelines, storage, self_id, inner_product_thres, init_mode_product_thres, match_index_dist, min_loop_num,
                  min_direction_loop, int(geometry))
        if raw_fisheye is not None:
            if pinhole_depth is not None or stereo_pinhole is not None:
                raise ValueError("raw_fisheye belongs to STEREO_FISHEYE: neither pinhole_depth nor stereo_pinhole")
            d = raw_fisheye
            up9, down9 = ((C.c_double * 9)(*[float(v) for v in d[k]]) for k in ("mei_up", "mei_down"))
            self.h = fisheye_lib().omni_pipeline_create_stereo_fisheye_raw(*common, d["src_width"], d["src_height"], d["fov_deg"], up9, down9, d.get("first_view", 1))
            if not self.h:
                raise capi.OmniError(f"omni_pipeline_create_stereo_fisheye_raw: {fisheye_lib().omni_fisheye_last_error().decode()}")
        elif stereo_pinhole is not None:
            if pinhole_depth is not None:
                raise ValueError("pinhole_depth and stereo_pinhole are two camera configurations")
            d = stereo_pinhole
            self.h = stereo_lib().omni_pipeline_create_stereo_pinhole(*common, d["fx"], d["fy"], d["cx"], d["cy"], d.get("src_width", 0), d.get("src_height", 0),
                                                                      d.get("triangle_thres", 0.006), d.get("accept_min_3d_pts", 50))
            if not self.h:
                raise capi.OmniError(f"omni_pipeline_create_stereo_pinhole: {stereo_lib().omni_stereo_last_error().decode()}")
        elif pinhole_depth is None:
            self.h = lib().omni_pipeline_create(*common)
        else:
            d = pinhole_depth
            self.h = lib().omni_pipeline_create_pinhole_depth(*common, d["fx"], d["fy"], d["cx"], d["cy"], d.get("depth_near", 0.3), d.get("depth_far", 10.0),
                                                              d.get("accept_min_3d_pts", 50))
        self._depth = None
        if not self.h:
            raise _err("omni_pipeline_create")
        if camera_model is not None:
            self.set_camera_model(camera_model)
        if device_landmarks is not None:
            self.set_device_landmarks(device_landmarks)
        if device_homography is not None:
            self.set_device_homography(device_homography)
        if device_depth_landmarks is not None:
            self.set_device_depth_landmarks(device_depth_landmarks)
        if device_pnp is not None:
            self.set_device_pnp(device_pnp)
        if send_img:
            self.set_send_img(True, jpg_quality)
        if compressed_images:
            self.set_compressed_images(True)
        if fit_pca:
            self.set_fit_pca(True)
        if wire or device_wire:
            self.set_wire(wire, device_wire, send_all_features)
        if WIRE_IMG_MODES.get(wire_img_desc, wire_img_desc) or wire_loop_conn:
            self.set_wire_messages(wire_img_desc, wire_loop_conn)
        if remote_in_stream:
            self.set_remote_in_stream(True)
        if batch_verify:
            self.set_batch_verify(True)
        if pcm:
            self.set_pcm(True, pcm_thres, pcm_redundant, pcm_capacity)
        if pose_graph:
            self.set_pose_graph(True, pose_graph_window, pose_graph_starts)

    def _pg(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {posegraph_lib().omni_posegraph_host_last_error().decode()}")

    def set_pose_graph(self, on: bool, window: int = 50, starts: int = 1):
        """before the first key frame: the 4-DoF pose graph of the last `window` key frames per drone (2..256) over ego motion and good_edges(), solved by optimize()
        from `starts` initial pose sets (1..64); refused on the sharded database and without a geometry stage"""
        self._pg(posegraph_lib().omni_pipeline_set_pose_graph(self.h, int(bool(on)), int(window), int(starts)), "omni_pipeline_set_pose_graph")

    def pose_graph(self) -> dict:
        on, window, starts = C.c_int(0), C.c_int(0), C.c_int(0)
        self._pg(posegraph_lib().omni_pipeline_get_pose_graph(self.h, C.byref(on), C.byref(window), C.byref(starts)), "omni_pipeline_get_pose_graph")
        return dict(on=bool(on.value), window=window.value, starts=starts.value)

    def optimize(self) -> int:
        """solves the current window on the GPU (blocking); returns the kept start's status (capi.PGO_*)"""
        st = C.c_int(0)
        self._pg(posegraph_lib().omni_pipeline_optimize(self.h, C.byref(st)), "omni_pipeline_optimize")
        return st.value

    def estimated_poses(self) -> np.ndarray:
        """every window key frame of the last optimize() (POSE_GRAPH_FRAME_DTYPE): drone, key frame id, pose = the estimate x y z yaw, odom = the odometry pose"""
        n = C.c_int(0)
        self._pg(posegraph_lib().omni_pipeline_estimated_poses(self.h, None, 0, C.byref(n)), "omni_pipeline_estimated_poses")
        out = np.zeros(n.value, POSE_GRAPH_FRAME_DTYPE)
        if len(out):
            self._pg(posegraph_lib().omni_pipeline_estimated_poses(self.h, out.ctypes.data, len(out), C.byref(n)), "omni_pipeline_estimated_poses")
        return out

    def drift(self):
        """this drone's newest estimated pose . inverse(its odometry pose) as x y z yaw, or None when the last optimize() held no key frame of this drone"""
        out, valid = (C.c_double * 4)(), C.c_int(0)
        self._pg(posegraph_lib().omni_pipeline_pose_graph_drift(self.h, out, C.byref(valid)), "omni_pipeline_pose_graph_drift")
        return np.array(out[:]) if valid.value else None

    def pose_graph_stats(self) -> dict:
        st, cost = (C.c_int64 * 11)(), (C.c_double * 2)()
        self._pg(posegraph_lib().omni_pipeline_pose_graph_stats(self.h, st, cost), "omni_pipeline_pose_graph_stats")
        return dict(zip(POSEGRAPH_STATS, (int(v) for v in st)), initial_cost=cost[0], final_cost=cost[1])

    def pose_graph_problem(self) -> dict:
        """the exact problem the last optimize() solved: dict(poses [starts][n][4], fixed [n], edges capi.PGO_EDGE_DTYPE, params capi.PgoParams)"""
        sizes, pr = (C.c_int * 3)(), capi.PgoParams()
        self._pg(posegraph_lib().omni_pipeline_pose_graph_problem(self.h, sizes, None, None, 0, None, 0, None), "omni_pipeline_pose_graph_problem")
        poses, fixed, edges = np.zeros((sizes[2], sizes[0], 4)), np.zeros(max(sizes[0], 1), np.uint8), np.zeros(max(sizes[1], 1), capi.PGO_EDGE_DTYPE)
        self._pg(posegraph_lib().omni_pipeline_pose_graph_problem(self.h, sizes, poses.ctypes.data, fixed.ctypes.data, sizes[0], edges.ctypes.data, len(edges), C.byref(pr)),
                 "omni_pipeline_pose_graph_problem")
        return dict(poses=poses, fixed=fixed[:sizes[0]], edges=edges[:sizes[1]], params=pr)

    def _pcm(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {pcm_lib().omni_pcm_host_last_error().decode()}")

    def set_pcm(self, on: bool, pcm_thres: float = 0.6, redundant: bool = False, capacity: int = capi.PCM_DEFAULT_CAPACITY):
        """before the first key frame: pairwise-consistency outlier rejection of the loop edges (refused on the sharded database and without a geometry stage)"""
        self._pcm(pcm_lib().omni_pipeline_set_pcm(self.h, int(bool(on)), float(pcm_thres), int(bool(redundant)), int(capacity)), "omni_pipeline_set_pcm")

    def pcm(self) -> dict:
        on, thres, red, cap = C.c_int(0), C.c_double(0), C.c_int(0), C.c_int(0)
        self._pcm(pcm_lib().omni_pipeline_get_pcm(self.h, C.byref(on), C.byref(thres), C.byref(red), C.byref(cap)), "omni_pipeline_get_pcm")
        return dict(on=bool(on.value), pcm_thres=thres.value, redundant=bool(red.value), capacity=cap.value)

    def good_edges(self) -> np.ndarray:
        """edges() then remote_edges() without those the stage rejected (REMOTE_EDGE_DTYPE records); with the stage off: all of them"""
        n = C.c_int(0)
        self._pcm(pcm_lib().omni_pipeline_good_edges(self.h, None, 0, C.byref(n)), "omni_pipeline_good_edges")
        out = np.zeros(n.value, REMOTE_EDGE_DTYPE)
        if len(out):
            self._pcm(pcm_lib().omni_pipeline_good_edges(self.h, out.ctypes.data, len(out), C.byref(n)), "omni_pipeline_good_edges")
        return out

    def pcm_stats(self) -> dict:
        st = (C.c_int64 * 6)()
        self._pcm(pcm_lib().omni_pipeline_pcm_stats(self.h, st), "omni_pipeline_pcm_stats")
        return dict(zip(PCM_STATS, (int(v) for v in st)))

    def pcm_records(self) -> np.ndarray:
        """the records the stage entered so far, in the order they entered (capi.PCM_EDGE_DTYPE, path lengths included)"""
        n = C.c_int(0)
        self._pcm(pcm_lib().omni_pipeline_pcm_records(self.h, None, 0, C.byref(n)), "omni_pipeline_pcm_records")
        out = np.zeros(n.value, capi.PCM_EDGE_DTYPE)
        if len(out):
            self._pcm(pcm_lib().omni_pipeline_pcm_records(self.h, out.ctypes.data, len(out), C.byref(n)), "omni_pipeline_pcm_records")
        return out

    def _pca(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {pca_lib().omni_pca_host_last_error().decode()}")

    def set_fit_pca(self, on: bool):
        """before the first key frame: every lane accumulates the moments of a PCA fit of the stream's 256-d descriptors (refused on the sharded database)"""
        self._pca(pca_lib().omni_pipeline_set_fit_pca(self.h, int(bool(on))), "omni_pipeline_set_fit_pca")

    def fit_pca(self) -> bool:
        on = C.c_int(0)
        self._pca(pca_lib().omni_pipeline_get_fit_pca(self.h, C.byref(on)), "omni_pipeline_get_fit_pca")
        return bool(on.value)

    def pca_fit_moments(self) -> "capi.PcaMoments":
        """waits for the units in flight; the lanes' accumulators merged in a fixed order"""
        m, n, sk = capi.PcaMoments(), C.c_int64(), C.c_int64()
        dp = C.POINTER(C.c_double)
        self._pca(pca_lib().omni_pipeline_pca_fit_moments(self.h, C.byref(n), C.byref(sk), m.s.ctypes.data_as(dp), m.S.ctypes.data_as(dp)), "omni_pipeline_pca_fit_moments")
        m.n, m.skipped = n.value, sk.value
        return m

    def pca_fit(self, pca_dim: int = 64) -> dict:
        """components [pca_dim][256] and mean [256] (float64 and float32), explained_variance, total_variance of the stream so far"""
        o, tv = capi._pca_outputs(pca_dim), C.c_double()
        self._pca(pca_lib().omni_pipeline_pca_fit_solve(self.h, int(pca_dim), *capi._pca_out_args(o, tv)), "omni_pipeline_pca_fit_solve")
        o["total_variance"] = tv.value
        return o

    def pca_fit_write(self, comp_path: str, mean_path: str, pca_dim: int = 64):
        """components_.csv / mean_.csv of the stream so far: the files a pipeline is created with"""
        self._pca(pca_lib().omni_pipeline_pca_fit_write(self.h, os.fsencode(comp_path), os.fsencode(mean_path), int(pca_dim)), "omni_pipeline_pca_fit_write")

    def pca_fit_reset(self):
        self._pca(pca_lib().omni_pipeline_pca_fit_reset(self.h), "omni_pipeline_pca_fit_reset")

    def set_camera_model(self, camera_model, intrinsics=None):
        """before the first key frame: the lens of every lift (see __init__); None: the ideal pinhole.  intrinsics [fx, fy, cx, cy] of the network-size image
        (or the dict's own "intrinsics"): None keeps the pipeline's"""
        m = _camera_struct(camera_model) if camera_model is not None else None
        if intrinsics is None and isinstance(camera_model, dict):
            intrinsics = camera_model.get("intrinsics")
        k = (C.c_double * 4)(*[float(v) for v in intrinsics]) if intrinsics is not None else None
        if camera_lib().omni_pipeline_set_camera_model(self.h, C.byref(m) if m is not None else None, k):
            raise capi.OmniError(f"omni_pipeline_set_camera_model: {camera_lib().omni_camera_last_error().decode()}")

    def camera_model(self) -> dict:
        """the lens and the intrinsics the pipeline lifts with, as camera_from_yaml's dict (without image_size)"""
        m, k = capi.CameraModel(), (C.c_double * 4)()
        if camera_lib().omni_pipeline_get_camera_model(self.h, C.byref(m), k):
            raise capi.OmniError(f"omni_pipeline_get_camera_model: {camera_lib().omni_camera_last_error().decode()}")
        return {"type": _CAMERA_NAMES[m.type], "k1": m.k1, "k2": m.k2, "p1": m.p1, "p2": m.p2, "xi": m.xi, "intrinsics": list(k)}

    def frame_landmarks(self, msg_id: int, direction: int = 0, max_n: int = 1024) -> dict:
        """the landmarks of one image of a key frame in the database as its message carries them: landmarks_2d [n][2], landmarks_2d_norm [n][2] (the lifted
        floats), landmarks_3d [n][3], landmarks_flag [n]"""
        n = C.c_int(0)
        a2, an, a3, af = np.zeros((max_n, 2), np.float32), np.zeros((max_n, 2), np.float32), np.zeros((max_n, 3), np.float32), np.zeros(max_n, np.uint8)
        if camera_lib().omni_pipeline_frame_landmarks(self.h, msg_id, direction, max_n, C.byref(n), a2.ctypes.data, an.ctypes.data, a3.ctypes.data, af.ctypes.data):
            raise capi.OmniError(f"omni_pipeline_frame_landmarks: {camera_lib().omni_camera_last_error().decode()}")
        if n.value > max_n:
            raise ValueError(f"frame_landmarks: {n.value} key points, max_n = {max_n}")
        k = n.value
        return {"landmarks_2d": a2[:k].copy(), "landmarks_2d_norm": an[:k].copy(), "landmarks_3d": a3[:k].copy(), "landmarks_flag": af[:k].copy()}

    def set_device_landmarks(self, on: bool):
        """before the first key frame: stereo landmarks inside the key-frame unit (GPU) or on the host's geometry threads"""
        if landmarks_lib().omni_pipeline_set_device_landmarks(self.h, int(bool(on))):
            raise capi.OmniError(f"omni_pipeline_set_device_landmarks: {landmarks_lib().omni_landmarks_last_error().decode()}")

    def set_device_depth_landmarks(self, on: bool):
        """before the first key frame, PINHOLE_DEPTH only: the depth landmarks inside the key-frame unit (GPU) or on the calling thread"""
        if depth_lib().omni_pipeline_set_device_depth_landmarks(self.h, int(bool(on))):
            raise capi.OmniError(f"omni_pipeline_set_device_depth_landmarks: {depth_lib().omni_depth_last_error().decode()}")

    def device_depth_landmarks(self) -> bool:
        """the switch as it was set"""
        on = C.c_int(0)
        if depth_lib().omni_pipeline_get_device_depth_landmarks(self.h, C.byref(on)):
            raise capi.OmniError(f"omni_pipeline_get_device_depth_landmarks: {depth_lib().omni_depth_last_error().decode()}")
        return bool(on.value)

    def _jpegdec(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {jpegdec_lib().omni_jpegdec_host_last_error().decode()}")

    def set_compressed_images(self, on: bool):
        """is_compressed_images: every following key frame comes as JPEG files (push_keyframe with bytes, run_jpeg), decoded on the GPU inside the key-frame unit in
        front of the resize (csrc/jpeg_dec.hip; libjpeg-turbo's gray pixels, pinned against Pillow -- cv::imdecode's own parity is unpinned).  Before the first
        key frame.  STEREO_PINHOLE, PINHOLE_DEPTH and STEREO_FISHEYE in its raw-fisheye mode; ignored by a flattened-view STEREO_FISHEYE pipeline and under a
        sharded database."""
        self._jpegdec(jpegdec_lib().omni_pipeline_set_compressed_images(self.h, int(bool(on))), "omni_pipeline_set_compressed_images")

    def fisheye_raw(self):
        """(src_width, src_height) of a raw-fisheye pipeline, (0, 0) of every other"""
        w, h = C.c_int(0), C.c_int(0)
        if fisheye_lib().omni_pipeline_get_fisheye_raw(self.h, C.byref(w), C.byref(h)):
            raise capi.OmniError(f"omni_pipeline_get_fisheye_raw: {fisheye_lib().omni_fisheye_last_error().decode()}")
        return w.value, h.value

    def apply_vins_settings(self, vins_yaml_text: str):
        """sets the switch from the VINS settings file's is_compressed_images"""
        self._jpegdec(jpegdec_lib().omni_pipeline_apply_vins_settings(self.h, vins_yaml_text.encode()), "omni_pipeline_apply_vins_settings")

    def compressed_images(self):
        """(the switch as set, whether this pipeline's mode takes files at all)"""
        on, act = C.c_int(0), C.c_int(0)
        self._jpegdec(jpegdec_lib().omni_pipeline_get_compressed_images(self.h, C.byref(on), C.byref(act)), "omni_pipeline_get_compressed_images")
        return bool(on.value), bool(act.value)

    def jpeg_corrupt(self) -> int:
        """frames whose file could not be decoded so far (all-zero pictures: no key points)"""
        n = C.c_int64(0)
        self._jpegdec(jpegdec_lib().omni_pipeline_jpeg_corrupt(self.h, C.byref(n)), "omni_pipeline_jpeg_corrupt")
        return n.value

    @staticmethod
    def _files(files):
        keep = [bytes(f) for f in files]
        return keep, (C.c_void_p * len(keep))(*[C.cast(C.c_char_p(f), C.c_void_p) for f in keep]), (C.c_int64 * len(keep))(*[len(f) for f in keep])

    def push_keyframe_jpeg(self, files, msg_id: int, stamp: float, pose7=None, prevent_adding_db: bool = False, depth: np.ndarray = None) -> int:
        """push_keyframe for a key frame that comes as JPEG files: [left, right] (STEREO_PINHOLE) or [the gray image] (PINHOLE_DEPTH) as bytes; copied before the
        call returns"""
        keep, fp, fs = self._files(files)
        p7 = None
        if pose7 is not None:
            p7v = np.ascontiguousarray(pose7, np.float64).reshape(7)
            p7 = p7v.ctypes.data_as(C.POINTER(C.c_double))
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
            self._depths = getattr(self, "_depths", []) + [depth]
        hits = C.c_int(0)
        self._jpegdec(jpegdec_lib().omni_pipeline_push_keyframe_jpeg(self.h, fp, fs, msg_id, float(stamp), p7, int(prevent_adding_db),
                                                                     depth.ctypes.data if depth is not None else None, C.byref(hits)), "omni_pipeline_push_keyframe_jpeg")
        return hits.value

    def run_jpeg(self, keyframes, first_msg_id: int = 0) -> int:
        """run() for key frames that come as JPEG files: keyframes = [[left, right], ...] (PINHOLE_DEPTH: [[gray], ...]) as bytes"""
        flat = [f for kf in keyframes for f in kf]
        keep, fp, fs = self._files(flat)
        hits = C.c_int(0)
        self._jpegdec(jpegdec_lib().omni_pipeline_run_jpeg(self.h, len(keyframes), first_msg_id, fp, fs, C.byref(hits)), "omni_pipeline_run_jpeg")
        return hits.value

    def _wire(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {wire_lib().omni_wire_host_last_error().decode()}")

    def set_wire(self, wire: bool, device_wire: bool = False, send_all_features: bool = False):
        """the LoopNet wire (host/loop_net_wire.hpp): on, every finished key frame's packets are kept until take_packets; device_wire: packed on the GPU inside the
        key-frame unit (csrc/wire_pack.hip) instead of on the calling thread, the same bytes.  Before the first key frame; device_wire needs the landmarks made on
        the device (device_landmarks / device_depth_landmarks with geometry)"""
        self._wire(wire_lib().omni_pipeline_set_wire(self.h, int(bool(wire)), int(bool(device_wire)), int(bool(send_all_features))), "omni_pipeline_set_wire")

    def wire(self):
        """(wire, device_wire as in effect, send_all_features)"""
        v = [C.c_int(0) for _ in range(3)]
        self._wire(wire_lib().omni_pipeline_get_wire(self.h, *[C.byref(x) for x in v]), "omni_pipeline_get_wire")
        return tuple(bool(x.value) for x in v)

    @property
    def wire_pending(self) -> int:
        return int(wire_lib().omni_pipeline_wire_pending(self.h))

    def take_packets(self):
        """pops the oldest finished key frame's packets: (msg_id, [(channel name, bytes), ...]) in sending order"""
        L = wire_lib()
        nb, npk, mid = C.c_int64(0), C.c_int(0), C.c_int64(0)
        self._wire(L.omni_pipeline_take_packets(self.h, None, None, 0, C.byref(nb), None, None, None, 0, C.byref(npk)), "omni_pipeline_take_packets")
        buf = np.empty(max(nb.value, 1), np.uint8)
        off, size, ch = np.empty(max(npk.value, 1), np.int64), np.empty(max(npk.value, 1), np.int32), np.empty(max(npk.value, 1), np.int32)
        self._wire(L.omni_pipeline_take_packets(self.h, C.byref(mid), buf.ctypes.data, buf.size, C.byref(nb), off.ctypes.data, size.ctypes.data, ch.ctypes.data, len(off),
                                                C.byref(npk)), "omni_pipeline_take_packets")
        return int(mid.value), [(WIRE_CHANNELS[ch[k]], buf[off[k]:off[k] + size[k]].tobytes()) for k in range(npk.value)]

    def set_wire_recv(self, recv_period: float = 0.5, min_direction_loop: int = 3, group_by_frame_id: bool = False):
        self._wire(wire_lib().omni_pipeline_set_wire_recv(self.h, recv_period, min_direction_loop, int(bool(group_by_frame_id))), "omni_pipeline_set_wire_recv")

    def recv_packet(self, channel: str, data: bytes, now: float) -> bool:
        """one packet of another drone; frames it completes go through the detector (candidates(), edges()) before the call returns.  False: it did not parse"""
        ok = C.c_int(0)
        self._wire(wire_lib().omni_pipeline_recv_packet(self.h, channel.encode(), data, len(data), now, C.byref(ok)), "omni_pipeline_recv_packet")
        return bool(ok.value)

    def scan_recv(self, now: float):
        self._wire(wire_lib().omni_pipeline_scan_recv(self.h, now), "omni_pipeline_scan_recv")

    @property
    def remote_frames(self) -> int:
        return int(wire_lib().omni_pipeline_remote_frames(self.h))

    def wire_host_ms(self, reset: bool = False) -> float:
        ms = C.c_double(0)
        self._wire(wire_lib().omni_pipeline_wire_host_ms(self.h, C.byref(ms), int(reset)), "omni_pipeline_wire_host_ms")
        return ms.value

    def _wiremsg(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {wiremsg_lib().omni_wiremsg_last_error().decode()}")

    def set_wire_messages(self, wire_img_desc="off", wire_loop_conn: bool = False):
        """LoopNet's other two message kinds (include/omni_host_wire_messages.h).  wire_img_desc: "off" / "image" / "whole" / "pc_replay" (or WIRE_IMG_*).  Before the
        first key frame, with the wire on; "image" needs send_img"""
        mode = WIRE_IMG_MODES[wire_img_desc] if isinstance(wire_img_desc, str) else int(wire_img_desc)
        self._wiremsg(wiremsg_lib().omni_pipeline_set_wire_messages(self.h, mode, int(bool(wire_loop_conn))), "omni_pipeline_set_wire_messages")

    def wire_messages(self):
        """(wire_img_desc as WIRE_IMG_*, wire_loop_conn, accept_img_desc)"""
        v = [C.c_int(0) for _ in range(3)]
        self._wiremsg(wiremsg_lib().omni_pipeline_get_wire_messages(self.h, *[C.byref(x) for x in v]), "omni_pipeline_get_wire_messages")
        return v[0].value, bool(v[1].value), bool(v[2].value)

    def set_wire_accept_img_desc(self, on: bool):
        """received whole descriptors that carry their 64-d descriptors enter the frame flow (what a replay ground station sets); default off"""
        self._wiremsg(wiremsg_lib().omni_pipeline_set_wire_accept_img_desc(self.h, int(bool(on))), "omni_pipeline_set_wire_accept_img_desc")

    def remote_edges(self) -> np.ndarray:
        """the edges other drones sent so far (REMOTE_EDGE_DTYPE records, every field of a LoopEdge, the doubles bit for bit), in arrival order"""
        n = C.c_int(0)
        self._wiremsg(wiremsg_lib().omni_pipeline_get_remote_edges(self.h, None, 0, C.byref(n)), "omni_pipeline_get_remote_edges")
        out = np.zeros(n.value, REMOTE_EDGE_DTYPE)
        if n.value:
            self._wiremsg(wiremsg_lib().omni_pipeline_get_remote_edges(self.h, out.ctypes.data, len(out), C.byref(n)), "omni_pipeline_get_remote_edges")
        return out

    def remote_images_pending(self):
        """(images waiting for take_remote_image, images dropped so far because more than WIRE_REMOTE_IMAGES_MAX waited)"""
        dropped = C.c_int64(0)
        return int(wiremsg_lib().omni_pipeline_remote_image_pending(self.h, C.byref(dropped))), int(dropped.value)

    def take_remote_image(self):
        """pops the oldest JPEG file another drone sent inside a whole descriptor: dict(drone_id, frame_id, direction, width, height, bytes); None when none waits"""
        L = wiremsg_lib()
        if L.omni_pipeline_remote_image_pending(self.h, None) <= 0:
            return None
        nb = C.c_int64(0)
        self._wiremsg(L.omni_pipeline_take_remote_image(self.h, None, 0, C.byref(nb), None, None, None, None, None), "omni_pipeline_take_remote_image")
        buf = np.empty(max(nb.value, 1), np.uint8)
        drone, direction, w, h, frame = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        self._wiremsg(L.omni_pipeline_take_remote_image(self.h, buf.ctypes.data, buf.size, C.byref(nb), C.byref(drone), C.byref(frame), C.byref(direction), C.byref(w),
                                                        C.byref(h)), "omni_pipeline_take_remote_image")
        return {"drone_id": drone.value, "frame_id": frame.value, "direction": direction.value, "width": w.value, "height": h.value, "bytes": buf[:nb.value].tobytes()}

    def _remote(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {remote_lib().omni_remote_last_error().decode()}")

    def set_remote_in_stream(self, on: bool):
        """remote key frames join the unit stream instead of flushing it (host/remote_queue.hpp).  Before the first key frame; refused on a sharded database"""
        self._remote(remote_lib().omni_pipeline_set_remote_in_stream(self.h, int(bool(on))), "omni_pipeline_set_remote_in_stream")

    def remote_in_stream(self) -> bool:
        on = C.c_int(0)
        self._remote(remote_lib().omni_pipeline_get_remote_in_stream(self.h, C.byref(on)), "omni_pipeline_get_remote_in_stream")
        return bool(on.value)

    @property
    def remote_pending(self) -> int:
        """remote frames queued, or in a detector batch that poll() / the next unit / flush() has not collected yet"""
        return int(remote_lib().omni_pipeline_remote_pending(self.h))

    def remote_stats(self):
        """(frames queued, frames that joined a unit's batch, batches of remote frames alone, flushes a remote frame forced: the switch-off path)"""
        out = (C.c_int64 * 4)()
        self._remote(remote_lib().omni_pipeline_remote_stats(self.h, out), "omni_pipeline_remote_stats")
        return tuple(int(v) for v in out)

    def _verify(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {verify_lib().omni_verify_last_error().decode()}")

    def set_batch_verify(self, on: bool):
        """inter-drone loop candidates are verified with their detector batch (host/verify_plan.hpp).  While no detector batch is pending; refused without a
        geometry stage and on a sharded database"""
        self._verify(verify_lib().omni_pipeline_set_batch_verify(self.h, int(bool(on))), "omni_pipeline_set_batch_verify")

    def batch_verify(self) -> bool:
        on = C.c_int(0)
        self._verify(verify_lib().omni_pipeline_get_batch_verify(self.h, C.byref(on)), "omni_pipeline_get_batch_verify")
        return bool(on.value)

    def verify_stats(self):
        """(inter-drone candidates deferred, resolves at the end of a detector batch, early resolves forced by the rule, matcher round trips spent on both)"""
        out = (C.c_int64 * 4)()
        self._verify(verify_lib().omni_pipeline_verify_stats(self.h, out), "omni_pipeline_verify_stats")
        return tuple(int(v) for v in out)

    def corr_stats(self):
        """(candidates whose correspondences the matcher's round trip assembled on the GPU, candidates it handed back to the host functions)"""
        out = (C.c_int64 * 2)()
        self._verify(verify_lib().omni_pipeline_corr_stats(self.h, out), "omni_pipeline_corr_stats")
        return tuple(int(v) for v in out)

    def edge_ids(self) -> np.ndarray:
        """LoopEdge::id of every accepted edge, in the order of edges(): numbered in candidate order"""
        n = int(verify_lib().omni_pipeline_edge_ids(self.h, None, 0))
        out = np.zeros(max(n, 1), np.int64)
        verify_lib().omni_pipeline_edge_ids(self.h, out.ctypes.data, n)
        return out[:n]

    def queue_copy_as_remote(self, src_msg_id: int, drone_id: int, new_msg_id: int):
        """recv_copy_as_remote's twin: the copy of the stored key frame is queued (remote_in_stream) instead of handed to on_remote_frame"""
        self._remote(remote_lib().omni_pipeline_queue_copy_as_remote(self.h, src_msg_id, drone_id, new_msg_id), "omni_pipeline_queue_copy_as_remote")

    def _jpeg(self, rc, what):
        if rc:
            raise capi.OmniError(f"{what}: {jpeg_lib().omni_jpeg_host_last_error().decode()}")

    def set_send_img(self, on: bool, jpg_quality: int = 50):
        """send_img: every following key frame's main images go into their messages as JPEG files, encoded inside the key-frame unit on the GPU (csrc/jpeg.hip;
        libjpeg's defaults, pinned against Pillow -- cv::imencode's own parity is unpinned).  Before the first key frame.  Ignored under a sharded database."""
        self._jpeg(jpeg_lib().omni_pipeline_set_send_img(self.h, int(bool(on)), int(jpg_quality)), "omni_pipeline_set_send_img")

    def send_img(self):
        """(the switch as set, jpg_quality, whether this pipeline's mode encodes at all)"""
        on, q, act = C.c_int(), C.c_int(), C.c_int()
        self._jpeg(jpeg_lib().omni_pipeline_get_send_img(self.h, C.byref(on), C.byref(q), C.byref(act)), "omni_pipeline_get_send_img")
        return bool(on.value), q.value, bool(act.value)

    def jpeg_truncated(self) -> int:
        n = C.c_int64()
        self._jpeg(jpeg_lib().omni_pipeline_jpeg_truncated(self.h, C.byref(n)), "omni_pipeline_jpeg_truncated")
        return n.value

    def frame_image(self, msg_id: int, direction: int) -> bytes:
        """the JPEG file direction `direction` of key frame `msg_id` carries in the detector's database (b"": none); between two calls of run / push_keyframe / flush"""
        n = C.c_int64()
        self._jpeg(jpeg_lib().omni_pipeline_frame_image(self.h, msg_id, direction, None, 0, C.byref(n)), "omni_pipeline_frame_image")
        out = np.empty(max(n.value, 1), np.uint8)
        self._jpeg(jpeg_lib().omni_pipeline_frame_image(self.h, msg_id, direction, out.ctypes.data, n.value, C.byref(n)), "omni_pipeline_frame_image")
        return out[:n.value].tobytes()

    def set_device_homography(self, on: bool):
        """the homography RANSAC of the loop candidates on the GPU (next to the matcher) or on the host's geometry threads; between any two calls"""
        if homography_lib().omni_pipeline_set_device_homography(self.h, int(bool(on))):
            raise capi.OmniError(f"omni_pipeline_set_device_homography: {homography_lib().omni_homography_last_error().decode()}")

    def device_homography(self):
        """(the switch, direction pairs whose mask came from the GPU so far, pairs the device handed back to the host)"""
        on, dev, host = C.c_int(0), C.c_int(0), C.c_int(0)
        if homography_lib().omni_pipeline_get_device_homography(self.h, C.byref(on), C.byref(dev), C.byref(host)):
            raise capi.OmniError(f"omni_pipeline_get_device_homography: {homography_lib().omni_homography_last_error().decode()}")
        return bool(on.value), dev.value, host.value

    def set_device_pnp(self, on: bool):
        """the EPnP RANSAC of the loop candidates' relative pose on the GPU or on the host's geometry threads (the refit stays there); between any two calls"""
        if pnp_lib().omni_pipeline_set_device_pnp(self.h, int(bool(on))):
            raise capi.OmniError(f"omni_pipeline_set_device_pnp: {pnp_lib().omni_pnp_last_error().decode()}")

    def recv_copy_as_remote(self, src_msg_id: int, drone_id: int, new_msg_id: int):
        """a copy of the database's key frame src_msg_id, handed to the detector as key frame new_msg_id of ANOTHER drone: the on-the-spot, init_mode path of a
        frame received over the network (after a flush).  -> (msg_id of the database frame it was matched with or -1, whether the candidate became an edge)"""
        old, loop = C.c_int64(-1), C.c_int(0)
        if pnp_lib().omni_pipeline_recv_copy_as_remote(self.h, src_msg_id, drone_id, new_msg_id, C.byref(old), C.byref(loop)):
            raise capi.OmniError(f"omni_pipeline_recv_copy_as_remote: {pnp_lib().omni_pnp_last_error().decode()}")
        return old.value, bool(loop.value)

    def device_pnp(self):
        """(the switch, candidates whose RANSAC ran on the GPU so far, candidates that ran on the host although the switch was on)"""
        on, dev, host = C.c_int(0), C.c_int(0), C.c_int(0)
        if pnp_lib().omni_pipeline_get_device_pnp(self.h, C.byref(on), C.byref(dev), C.byref(host)):
            raise capi.OmniError(f"omni_pipeline_get_device_pnp: {pnp_lib().omni_pnp_last_error().decode()}")
        return bool(on.value), dev.value, host.value

    @classmethod
    def from_launch(cls, device: int, launch_xml: str, sp_weights_path: str, vlad_weights_path: str, pca_comp_csv: str | None = None, pca_mean_csv: str | None = None,
                    precision=capi.PREC_F16, microbatch=8, pipelines=0, storage=capi.STORE_F32, geometry=False, node_name="swarm_loop", args: dict | None = None,
                    intrinsics=None, camera_yaml: str | None = None):
        """A pipeline configured by one of the reference's launch files (omni_pipeline_create_from_launch): image size, thresholds, camera configuration and
        self_id come from the file; weights, precision and batching are this build's.  camera_yaml: the TEXT of the camodocal file the launch file's
        camera_config_path names (omni_pipeline_create_from_launch_camera): lens and intrinsics come from it, scaled to the launch file's image size, in the
        place of `intrinsics`."""
        self = cls.__new__(cls)
        a = "\n".join(f"{k}:={v}" for k, v in (args or {}).items()).encode() or None
        k4 = (C.c_double * 4)(*intrinsics) if intrinsics is not None else None
        self.microbatch = microbatch
        self._depth = None
        if camera_yaml is not None:
            if intrinsics is not None:
                raise ValueError("from_launch: camera_yaml carries the intrinsics; give one of the two")
            self.h = camera_lib().omni_pipeline_create_from_launch_camera(device, launch_xml.encode(), node_name.encode(), a, sp_weights_path.encode(), vlad_weights_path.encode(),
                                                                          pca_comp_csv.encode() if pca_comp_csv else None, pca_mean_csv.encode() if pca_mean_csv else None,
                                                                          precision, microbatch, pipelines, storage, int(geometry), camera_yaml.encode())
            if not self.h:
                raise capi.OmniError(f"omni_pipeline_create_from_launch_camera: {camera_lib().omni_camera_last_error().decode()}")
            return self
        self.h = lib().omni_pipeline_create_from_launch(device, launch_xml.encode(), node_name.encode(), a, sp_weights_path.encode(), vlad_weights_path.encode(),
                                                       pca_comp_csv.encode() if pca_comp_csv else None, pca_mean_csv.encode() if pca_mean_csv else None, precision,
                                                       microbatch, pipelines, storage, int(geometry), k4)
        if not self.h:
            raise _err("omni_pipeline_create_from_launch")
        return self

    def set_depth(self, first_msg_id: int, depth: np.ndarray):
        """depth [n][H][W] u16 millimetres of key frames first_msg_id .. first_msg_id + n - 1 (kept alive by this object)"""
        self._depth = np.ascontiguousarray(depth, np.uint16)
        if lib().omni_pipeline_set_depth(self.h, first_msg_id, self._depth.shape[0], self._depth.ctypes.data):
            raise _err("omni_pipeline_set_depth")

    def set_stereo_extrinsics(self, left7, right7):
        """STEREO_PINHOLE: body -> camera of the left and the right camera, xyz + quaternion wxyz each; before the first key frame"""
        a, b = (np.ascontiguousarray(v, np.float64).reshape(7) for v in (left7, right7))
        if stereo_lib().omni_pipeline_set_stereo_extrinsics(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double))):
            raise capi.OmniError(f"omni_pipeline_set_stereo_extrinsics: {stereo_lib().omni_stereo_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            lib().omni_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach_shard(self, rank: int, world: int, unique_id: bytes):
        """Collective: the database becomes the row-sharded index over `world` ranks (RCCL inside libomni_hip.so)."""
        if lib().omni_pipeline_attach_shard(self.h, rank, world, unique_id):
            raise _err("omni_pipeline_attach_shard")

    def preload(self, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, np.float32)
        if lib().omni_pipeline_preload(self.h, rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0]):
            raise _err("omni_pipeline_preload")

    @property
    def db_rows(self) -> int:
        return lib().omni_pipeline_db_rows(self.h)

    def run(self, n_keyframes: int, first_msg_id: int, pool_ptrs, first_slot: int = 0, tail_ptr=None, from_host: bool = True) -> int:
        """pool_ptrs: addresses (ints) of the micro-batch image blocks -- pinned host memory (from_host) or HBM."""
        arr = (C.c_void_p * len(pool_ptrs))(*pool_ptrs)
        hits = C.c_int(0)
        if lib().omni_pipeline_run(self.h, n_keyframes, first_msg_id, arr, len(pool_ptrs), first_slot, tail_ptr, int(from_host), C.byref(hits)):
            raise _err("omni_pipeline_run")
        return hits.value

    def push_keyframe(self, images, msg_id: int, stamp: float, pose7=None, prevent_adding_db: bool = False, depth: np.ndarray = None) -> int:
        """The streaming intake: one key frame (images: list of u8 arrays [H][W], up cameras then down cameras; PINHOLE_DEPTH: one; STEREO_PINHOLE: the left
        and the right frame, at the camera's size when the pipeline was given src_width / src_height) with its id, stamp,
        odometry pose and prevent_adding_db flag (swarm_loop.cpp:140-170); returns the loop candidates found by the units this call finished.  The
        images are copied before the call returns; a depth image must stay alive until flush()."""
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        arr = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
        p7 = None
        if pose7 is not None:
            p7v = np.ascontiguousarray(pose7, np.float64).reshape(7)
            p7 = p7v.ctypes.data_as(C.POINTER(C.c_double))
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
            self._depths = getattr(self, "_depths", []) + [depth]
        hits = C.c_int(0)
        if lib().omni_pipeline_push_keyframe(self.h, arr, imgs[0].shape[1], msg_id, float(stamp), p7, int(prevent_adding_db),
                                             depth.ctypes.data if depth is not None else None, C.byref(hits)):
            raise _err("omni_pipeline_push_keyframe")
        return hits.value

    def poll(self) -> int:
        """The streaming intake's latency bound (call from a timer or after every push; never waits for a CNN unit): sends a partly filled micro-batch
        older than max_wait_ms, finishes the units the GPU is done with, and -- with nothing left in flight -- collects the last detector step."""
        hits = C.c_int(0)
        if lib().omni_pipeline_poll(self.h, C.byref(hits)):
            raise _err("omni_pipeline_poll")
        return hits.value

    def set_latency(self, max_wait_ms: float = 50.0, dispatch_when_idle: bool = True):
        if lib().omni_pipeline_set_latency(self.h, float(max_wait_ms), int(dispatch_when_idle)):
            raise _err("omni_pipeline_set_latency")

    def units(self):
        """(units in flight, how the last run() ordered them: 0 = kernels take turns, 1 / 2 = oldest first)"""
        f = C.c_int(0)
        n = lib().omni_pipeline_units(self.h, C.byref(f))
        return n, f.value

    def flush(self) -> int:
        hits = C.c_int(0)
        if lib().omni_pipeline_flush(self.h, C.byref(hits)):
            raise _err("omni_pipeline_flush")
        self._depths = []
        return hits.value

    def host_times(self, reset: bool = True) -> dict:
        """the host thread's milliseconds per unit (micro-batch): enqueue, wait_gpu, messages, detector, geometry; `units` = how many were averaged"""
        out = (C.c_double * 5)()
        n = lib().omni_pipeline_host_times(self.h, out, int(reset))
        return dict(zip(("enqueue", "wait_gpu", "messages", "detector", "geometry"), [round(v, 4) for v in out]), units=n)

    def prepare(self, n_keyframes: int):
        if lib().omni_pipeline_prepare(self.h, n_keyframes):
            raise _err("omni_pipeline_prepare")

    def geometry_stats(self):
        """(candidates handed to compute_loop, loop edges accepted)"""
        a, b = C.c_int(0), C.c_int(0)
        lib().omni_pipeline_geometry_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def set_poses(self, first_msg_id: int, poses7: np.ndarray):
        """odometry poses [n][7] = position xyz + quaternion wxyz of key frames first_msg_id .. first_msg_id + n - 1"""
        p = np.ascontiguousarray(poses7, np.float64).reshape(-1, 7)
        if lib().omni_pipeline_set_poses(self.h, first_msg_id, len(p), p.ctypes.data_as(C.POINTER(C.c_double))):
            raise _err("omni_pipeline_set_poses")

    def candidates(self) -> np.ndarray:
        """[n][4] = (new key frame, old key frame, direction_new, direction_old) of every loop candidate so far"""
        n = lib().omni_pipeline_get_candidates(self.h, None, 0)
        out = np.zeros((max(n, 1), 4), np.int64)
        lib().omni_pipeline_get_candidates(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), n)
        return out[:n]

    def edges(self) -> np.ndarray:
        """[n][12] = (keyframe_id_a, keyframe_id_b, drone_id_a, drone_id_b, pnp inliers, relative position xyz, relative quaternion wxyz)"""
        n = lib().omni_pipeline_get_edges(self.h, None, 0)
        out = np.zeros((max(n, 1), 12), np.float64)
        lib().omni_pipeline_get_edges(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out[:n]

    def latencies_ms(self, reset: bool = True) -> np.ndarray:
        """latency of every micro-batch since the last reset: upload start -> detector (+ geometry) done, milliseconds"""
        n = lib().omni_pipeline_get_latencies(self.h, None, 0, 0)
        out = np.zeros(max(n, 1), np.float64)
        lib().omni_pipeline_get_latencies(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), n, int(reset))
        return out[:n]

    def apply_launch(self, launch_xml: str, node_name: str = "swarm_loop"):
        """the detector's and the geometry stage's thresholds from one of the reference's launch files (omni_pipeline_apply_launch)"""
        if lib().omni_pipeline_apply_launch(self.h, launch_xml.encode(), node_name.encode()):
            raise _err("omni_pipeline_apply_launch")

    def exchange_us(self, reset: bool = True) -> np.ndarray:
        """sharded mode: [n][2] device microseconds of the two all-gathers (new rows, per-shard top-k lists) of every exchange unit since the last reset"""
        n = lib().omni_pipeline_get_exchange_us(self.h, None, 0, 0)
        out = np.zeros((max(n, 1), 2), np.float32)
        lib().omni_pipeline_get_exchange_us(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), n, int(reset))
        return out[:n]

    def sync(self):
        if lib().omni_pipeline_sync(self.h):
            raise _err("omni_pipeline_sync")
