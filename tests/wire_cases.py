"""Synthetic key-frame arrays for the LoopNet wire's pack stage (csrc/wire_plan.h), shared by the CPU and the GPU tests: the shapes and edges of the issue, each a dict
of the arguments of capi.wire_pack_host / capi.wire_pack plus send_all_features.  Also an independent reader of the two packets (struct, big-endian), so that the
layout is stated once more outside C++."""
import struct

import numpy as np

ODD_BITS = np.array([0x7fc12345, 0xffc00001, 0x7f812345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32)      # NaNs with payloads, infs, -0.0, denormals


def frame(capi, seed, n_images, max_num, send_all=False):
    rng = np.random.default_rng(seed)
    N, M = n_images, max_num
    meta = np.zeros(N, capi.WIRE_META_DTYPE)
    meta["timestamp"] = 1.6e9 + rng.uniform(-10, 10, N)
    meta["frame_id"] = rng.integers(-2**62, 2**62, N)
    meta["drone_id"] = 2
    meta["direction"] = np.arange(N) % 4
    meta["prevent_adding_db"] = rng.integers(0, 2, N)
    meta["pose_drone"] = rng.uniform(-10, 10, (N, 7))
    meta["camera_extrinsic"] = rng.uniform(-10, 10, (N, 7))
    return {"kps_xy": rng.uniform(0, 600, (N, M, 2)).astype(np.float32), "n_kps": rng.integers(1, M + 1, N).astype(np.int32),
            "desc": rng.uniform(-1, 1, (N, M, 64)).astype(np.float32), "norm2d": rng.uniform(-1, 1, (N, M, 2)).astype(np.float32),
            "l3d": rng.uniform(-5, 5, (N, M, 3)).astype(np.float32), "flag": (rng.integers(0, 3, (N, M)) != 0).astype(np.uint8),
            "global_desc": rng.uniform(-1, 1, (N, 4096)).astype(np.float32), "meta": meta, "send_all_features": send_all}


def flag_exactly(f, g, n_kps, count):
    """image g: n_kps key points, `count` of them flagged, spread over even then odd slots"""
    f["n_kps"][g] = n_kps
    f["flag"][g] = 0
    slots = (list(range(0, n_kps, 2)) + list(range(1, n_kps, 2)))[:count]
    assert len(slots) == count
    f["flag"][g, slots] = 1
    return f


def cases(capi):
    """name -> frame.  Shapes: n_images 1 and 8, max_num 200 and 65; every edge of the issue; more than one compaction pass (max_num 600, 1024)"""
    out = {}
    for N in (1, 8):
        for M in (200, 65):
            out[f"random_{N}x{M}"] = frame(capi, 10 * N + M, N, M)
    out["send_all_8x65"] = frame(capi, 3, 8, 65, send_all=True)
    f = frame(capi, 4, 8, 200); f["n_kps"][[1, 7]] = 0; out["no_keypoints"] = f
    out["no_flag"] = flag_exactly(frame(capi, 5, 8, 200), 2, 120, 0)
    out["all_flagged"] = flag_exactly(frame(capi, 6, 8, 200), 3, 200, 200)
    for c in (63, 64, 65):
        out[f"flagged{c}_of_200"] = flag_exactly(frame(capi, 7 + c, 1, 200), 0, 200, c)
    out["send_all_counts_flags"] = flag_exactly(frame(capi, 8, 8, 200, send_all=True), 0, 150, 40)
    f = frame(capi, 9, 8, 65); f["n_kps"][0] = 9999; f["n_kps"][1] = -3; out["clamped_counts"] = f
    out["passes_3_1x600"] = frame(capi, 11, 1, 600)
    out["full_1x1024"] = flag_exactly(frame(capi, 12, 1, 1024), 0, 1024, 1024)
    f = flag_exactly(frame(capi, 13, 1, 65), 0, 65, 65)
    for key, step in (("desc", 5), ("global_desc", 7), ("norm2d", 1), ("kps_xy", 1), ("l3d", 1)):
        v = f[key].view(np.uint32).reshape(-1)
        idx = np.arange(0, v.size, step)
        v[idx] = ODD_BITS[(idx // step) % 8]
    f["meta"]["pose_drone"].view(np.uint64)[0, 1] = 0x7ff8000000abcdef
    f["meta"]["camera_extrinsic"].view(np.uint64)[0, 6] = 0x8000000000000000
    f["meta"]["drone_id"][0] = -5
    out["payload_bits"] = f
    return out


def args(f):
    return (f["kps_xy"], f["n_kps"], f["desc"], f["norm2d"], f["l3d"], f["flag"], f["global_desc"], f["meta"])


def parse_header(b: bytes) -> dict:
    assert len(b) == 161 + 4 * 4096
    fp, ts, drone, msg_id, frame_id, feature_num, direction, prevent = struct.unpack(">8sdiqqiiB", b[:45])
    assert fp == b"OMNIHDR1" and struct.unpack(">i", b[157:161])[0] == 4096
    return {"timestamp_bits": b[8:16], "drone_id": drone, "msg_id": msg_id, "frame_id": frame_id, "feature_num": feature_num, "direction": direction, "prevent": prevent,
            "pose_bits": b[45:101], "extrinsic_bits": b[101:157], "image_desc_bits": np.frombuffer(b[161:], ">u4")}


def parse_landmark(b: bytes) -> dict:
    assert len(b) == 324
    fp, msg_id, header_id, drone, lid, flag = struct.unpack(">8sqqiii", b[:36])
    assert fp == b"OMNILMK1" and struct.unpack(">i", b[64:68])[0] == 64
    return {"msg_id": msg_id, "header_id": header_id, "drone_id": drone, "landmark_id": lid, "flag": flag, "floats_bits": np.frombuffer(b[36:64], ">u4"),
            "desc_bits": np.frombuffer(b[68:], ">u4")}
