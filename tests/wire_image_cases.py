"""Cases and an independent reader of the LoopNet wire's other two packets: the whole descriptor (SWARM_LOOP_IMG_DES; csrc/wire_plan.h whole_*, packed by
capi.wire_pack_image_host / capi.wire_pack_image) and the loop edge (SWARM_LOOP_CONN).  The cases are tests/wire_cases.py's synthetic key-frame arrays plus JPEG rows,
sizes and statuses, shared by the CPU and the GPU tests; the reader and the writer below state both layouts once more outside C++ (struct, big-endian)."""
import struct

import numpy as np

from tests import wire_cases as WC

JPEG_OK, JPEG_TRUNCATED = 0, 1
SMALLEST_FILE = 328 + 2                  # OMNI_JPEG_HEADER_BYTES + 2
CAP = 1024                               # jpeg_capacity of most cases: a multiple of 4, a few output dwords per lane
HEAD = ">8sdiqqiiB7d7diiiii"             # fingerprint .. prevent_adding_db, the two poses, width, height, image_desc_size, feature_descriptor_size, image_size
assert struct.calcsize(HEAD) == 177
EDGE = ">8sqqqiii2d7d7d7d3d3d"
assert struct.calcsize(EDGE) == 276
TAIL_N_KPS = [0, 1, 2, 3, 4, 65, 200, 9999]      # every alignment of the byte tail (landmark_num mod 4), no packet, the two sizes, a clamped count


def with_jpeg(f, seed, cap=CAP, sizes=None, status=None, width=640, height=480, with_features=True, with_image=True):
    rng = np.random.default_rng(1000 + seed)
    N = f["n_kps"].shape[0]
    f = dict(f)
    f["jpeg"] = rng.integers(1, 256, (N, cap)).astype(np.uint8)          # (no zero byte: a file byte that is dropped shows)
    f["jpeg_sizes"] = np.asarray(sizes if sizes is not None else rng.integers(SMALLEST_FILE, cap + 1, N), np.int32)
    f["jpeg_status"] = np.asarray(status if status is not None else np.zeros(N), np.int32)
    f.update(width=width, height=height, with_features=with_features, with_image=with_image)
    return f


def cases(capi):
    """name -> case.  n_images 1 and 8, max_num 65 and 200, n_kps 0..4 / 65 / 200 / clamped, file sizes of every residue mod 4 against every alignment of the tail,
    no file (truncated), the smallest file, exactly the capacity, above it, all four (with_features, with_image) combinations, NaN / inf / -0.0 payload bits"""
    out = {}
    for N in (1, 8):
        for M in (200, 65):
            for wf in (False, True):
                for wi in (False, True):
                    out[f"random_{N}x{M}_f{int(wf)}i{int(wi)}"] = with_jpeg(WC.frame(capi, 10 * N + M, N, M), N + M, with_features=wf, with_image=wi)
    for r in range(4):
        for M in (200, 65):
            f = WC.frame(capi, 20 + r, 8, M)
            f["n_kps"][:] = TAIL_N_KPS
            out[f"tail{r}_8x{M}"] = with_jpeg(f, r, sizes=[SMALLEST_FILE + ((g + r) & 3) for g in range(8)], with_features=bool(r & 1))
    f = WC.frame(capi, 30, 8, 65)
    st = [JPEG_TRUNCATED] + [JPEG_OK] * 7
    out["file_sizes"] = with_jpeg(f, 30, sizes=[0, SMALLEST_FILE, CAP, CAP + 7, -5, 1, 2, 3], status=st)
    out["truncated_with_size"] = with_jpeg(f, 31, sizes=[500, 331, 332, 333, 334, 335, 336, 337], status=st, with_features=False)
    f = WC.frame(capi, 32, 1, 65); f["n_kps"][0] = 1
    out["one_landmark_full_file"] = with_jpeg(f, 32, cap=332, sizes=[332])
    f = WC.frame(capi, 33, 8, 65); f["n_kps"][0] = 9999; f["n_kps"][1] = -3
    out["clamped_counts"] = with_jpeg(f, 33)
    out["payload_bits"] = with_jpeg(WC.cases(capi)["payload_bits"], 34, cap=332, sizes=[331], width=-1, height=2**31 - 1)
    return out


def args(f):
    return WC.args(f) + ((f["jpeg"], f["jpeg_sizes"], f["jpeg_status"]) if f["with_image"] else (None, None, None))


def kwargs(f):
    return {"width": f["width"], "height": f["height"], "with_features": f["with_features"]}


def capacity(M, jpeg_capacity):
    return 180 + 4 * (4096 + 71 * M) + (M + jpeg_capacity + 3) // 4 * 4


def image_size(f, g):
    if not f["with_image"] or f["jpeg_status"][g] != JPEG_OK:
        return 0
    return int(np.clip(f["jpeg_sizes"][g], 0, f["jpeg"].shape[1]))


def expected_packet(f, g, msg_id=0):
    """image g's whole descriptor written with struct and numpy alone; None when the image is not sent"""
    M = f["flag"].shape[1]
    n = int(np.clip(f["n_kps"][g], 0, M))
    if n == 0:
        return None
    m, isz = f["meta"][g], image_size(f, g)
    fds = 64 * n if f["with_features"] else 0
    w, h = (np.array([f["width"], f["height"]], np.int64).astype(np.int32))
    head = struct.pack(HEAD, b"OMNIIMG1", m["timestamp"], m["drone_id"], msg_id, m["frame_id"], n, m["direction"], int(m["prevent_adding_db"] != 0),
                       *m["pose_drone"], *m["camera_extrinsic"], int(w), int(h), 4096, fds, isz)
    # (struct packs a double from its value: NaN payloads must go through the bits)
    head = bytearray(head)
    head[8:16] = np.array([m["timestamp"]]).view(np.uint64).astype(">u8").tobytes()
    head[45:101] = m["pose_drone"].view(np.uint64).astype(">u8").tobytes()
    head[101:157] = m["camera_extrinsic"].view(np.uint64).astype(">u8").tobytes()
    be = lambda a: np.ascontiguousarray(a).view(np.uint32).astype(">u4").tobytes()
    floats = be(f["global_desc"][g]) + (be(f["desc"][g, :n]) if fds else b"") + be(f["norm2d"][g, :n]) + be(f["kps_xy"][g, :n]) + be(f["l3d"][g, :n])
    return bytes(head) + floats + f["flag"][g, :n].tobytes() + (f["jpeg"][g, :isz].tobytes() if isz else b"")


def parse_image(b: bytes) -> dict:
    """the whole descriptor read back: the head's fields, the float arrays as bits, flags and file"""
    v = struct.unpack(HEAD, b[:177])
    assert v[0] == b"OMNIIMG1"
    n, ids, fds, isz = v[5], v[24], v[25], v[26]
    assert len(b) == 177 + 4 * (ids + fds + 7 * n) + n + isz
    fl = np.frombuffer(b[177:177 + 4 * (ids + fds + 7 * n)], ">u4")
    cut = np.cumsum([0, ids, fds, 2 * n, 2 * n, 3 * n])
    parts = [fl[cut[i]:cut[i + 1]] for i in range(5)]
    t = 177 + 4 * len(fl)
    return {"timestamp_bits": b[8:16], "drone_id": v[2], "msg_id": v[3], "frame_id": v[4], "landmark_num": n, "direction": v[6], "prevent": v[7], "pose_bits": b[45:101],
            "extrinsic_bits": b[101:157], "width": v[22], "height": v[23], "image_desc_bits": parts[0], "desc_bits": parts[1], "norm2d_bits": parts[2], "kps_bits": parts[3],
            "l3d_bits": parts[4], "flag": np.frombuffer(b[t:t + n], np.uint8), "image": b[t + n:]}


def parse_edge(b: bytes) -> dict:
    assert len(b) == 276
    v = struct.unpack(EDGE, b)
    assert v[0] == b"OMNILCN1"
    return {"id": v[1], "keyframe_id_a": v[2], "keyframe_id_b": v[3], "drone_id_a": v[4], "drone_id_b": v[5], "pnp_inlier_num": v[6], "ts_a": v[7], "ts_b": v[8],
            "relative_pose": v[9:16], "self_pose_a": v[16:23], "self_pose_b": v[23:30], "pos_cov": v[30:33], "ang_cov": v[33:36], "bits": np.frombuffer(b[44:], ">u8")}
