"""Seeded inputs of the depth-landmark stage (csrc/depth_plan.h: PINHOLE_DEPTH's lifted key points and depth landmarks) and the protocol of
tests/cpp/depth_plan_pin.cpp, shared by the CPU and GPU tests.  The lenses are tests/camera_cases.py's (imported, not restated).

Every case has 3 images; what the cases cover between them:
  gate and rounding   half-integer coordinates both ways (2.5 -> 2, 3.5 -> 4), x = 640.0 on a 640-wide depth image (passes the gate, no landmark), x = 640.4 and
                      x = -0.25 (the gate drops them, although -0.25 rounds to 0), the same in y with 480;
  depth values        0, 299, 300 (300 / 1000.0 is not > 0.3), 301, 9999, 10000, 65535 under the first key points, 200 .. 12000 elsewhere;
  depth images        640 x 480 and one smaller than the gate (64 x 48); a stride larger than the width;
  key-point counts    0, accept_min, accept_min + 1, 257 (the kernel's lane loop wraps), max_num = 300, a raw count above max_num;
  poses               un-normalised quaternions in pose_drone and in the extrinsic;
  lenses              the ideal pinhole, PINHOLE with k1 k2 p1 p2, MEI;
  one image without a depth frame."""
import ctypes
import os
import subprocess

import numpy as np

from tests import camera_cases as CC

ROOT = CC.ROOT
ACCEPT_MIN = 5
NEAR, FAR = 0.3, 10.0
DEPTH_VALUES = (0, 299, 300, 301, 9999, 10000, 65535)
# (x, y): the gate, the rounding and the guard against this depth image; on a 640 x 480 depth image unless noted
SPECIAL_POINTS = ((2.5, 3.5), (3.5, 2.5), (640.0, 10.0), (640.4, 10.0), (-0.25, 5.0), (10.0, 480.0), (10.0, 480.4), (10.0, -0.25), (639.5, 479.5), (638.5, 478.5),
                  (0.0, 0.0), (0.5, 0.5), (63.5, 47.5), (62.5, 46.5), (64.0, 10.0), (10.0, 48.0), (639.0, 479.0), (0.49, 0.51))


def make_case(omni, lens, seed, max_num, depth_w, depth_h, stride, counts, have, accept_min=ACCEPT_MIN, near=NEAR, far=FAR) -> dict:
    rng = np.random.default_rng(seed)
    N = len(counts)
    fx, fy, cx, cy = CC.intrinsics(lens)
    ext = np.r_[rng.uniform(-0.2, 0.2, 3), rng.normal(size=4) * 1.7]                  # un-normalised
    model = omni.capi.depth_model(fx, fy, cx, cy, near, far, accept_min, depth_w, depth_h, ext)
    poses = np.concatenate([rng.uniform(-5, 5, (N, 3)), rng.normal(size=(N, 4)) * rng.uniform(0.3, 3.0, (N, 1))], 1)
    kps = np.zeros((N, max_num, 2), np.float32)
    depth = rng.integers(200, 12000, (N, depth_h, stride)).astype(np.uint16)
    for i, n in enumerate(counts):
        live = min(max(n, 0), max_num)
        # whole pixels, half pixels and arbitrary fractions, over the gate's range and a little beyond; every third point inside a small depth image
        xy = np.stack([rng.uniform(-3, 644, max_num), rng.uniform(-3, 484, max_num)], 1)
        small = rng.random(max_num) < (0.5 if depth_w < 640 else 0.0)
        xy[small] = np.stack([rng.uniform(0, depth_w + 1, small.sum()), rng.uniform(0, depth_h + 1, small.sum())], 1)
        kind = rng.integers(0, 3, max_num)
        xy[kind == 0] = np.rint(xy[kind == 0])
        xy[kind == 1] = np.floor(xy[kind == 1]) + 0.5
        sp = np.array(SPECIAL_POINTS)[: min(len(SPECIAL_POINTS), max_num)]
        xy[: len(sp)] = sp
        kps[i] = xy.astype(np.float32)                                                   # (slots behind the live ones hold values too: they must not be read)
        # the special depth values under the key points that can see the image, cyclically
        at = 0
        for k in range(live):
            x, y = kps[i, k]
            if not (0 <= x <= 640 and 0 <= y <= 480):
                continue
            px, py = int(np.rint(np.float64(x))), int(np.rint(np.float64(y)))
            if px < depth_w and py < depth_h and k % 2 == 0:
                depth[i, py, px] = DEPTH_VALUES[at % len(DEPTH_VALUES)]
                at += 1
    return {"lens": lens, "camera": CC.camera(omni, lens), "model": model, "n_images": N, "max_num": max_num, "stride": stride, "poses": poses, "kps_xy": kps,
            "n_kps": np.array(counts, np.int32), "have": np.array(have, np.uint8), "depth": depth}


def gate_cases(omni) -> list:
    """three lenses x 3 images x max_num 300, and a 7-slot case"""
    return [
        make_case(omni, "ideal", 1, 300, 640, 480, 640, [0, ACCEPT_MIN, ACCEPT_MIN + 1], [1, 1, 1]),
        make_case(omni, "euroc", 2, 300, 640, 480, 656, [257, 300, 350], [1, 0, 1]),
        make_case(omni, "mei", 3, 300, 64, 48, 80, [300, 40, 257], [1, 1, 1]),
        make_case(omni, "ideal", 4, 7, 640, 480, 640, [7, 6, 9], [1, 1, 1]),
        make_case(omni, "mild", 5, 300, 640, 480, 640, [300, 300, 120], [1, 1, 0], accept_min=50),
    ]


# ---- tests/cpp/depth_plan_pin.cpp ---------------------------------------------------------------------------------------------------------------------------
def build_pin(tmp_dir) -> str:
    """a stand-alone program with its own main, built with ASan + UBSan (as tests/cpp/landmark_plan_pin.cpp is by its sanitizer run)"""
    exe = os.path.join(str(tmp_dir), "depth_plan_pin_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "depth_plan_pin.cpp")])
    return exe


def _struct_bytes(s) -> bytes:
    return bytes(ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s)))


def pack(c) -> bytes:
    hdr = np.array([c["n_images"], c["max_num"], c["stride"], 0], np.int32)
    parts = [hdr.tobytes(), _struct_bytes(c["model"]), _struct_bytes(c["camera"])]
    parts += [np.ascontiguousarray(c[k], dt).tobytes() for k, dt in (("poses", np.float64), ("kps_xy", np.float32), ("n_kps", np.int32), ("have", np.uint8), ("depth", np.uint16))]
    return b"".join(parts)


def run_pin(exe, mode, cases) -> list:
    """[{norm2d, landmarks_3d, landmarks_flag, count_3d}] per case"""
    raw = subprocess.run([exe, mode], input=b"".join(pack(c) for c in cases), capture_output=True, check=True).stdout
    out, at = [], 0
    for c in cases:
        N, M = c["n_images"], c["max_num"]
        r = {}
        for key, shape, dt in (("norm2d", (N, M, 2), np.float32), ("landmarks_3d", (N, M, 3), np.float32), ("landmarks_flag", (N, M), np.uint8), ("count_3d", (N,), np.int32)):
            a = np.frombuffer(raw, dt, int(np.prod(shape)), at).reshape(shape)
            at += a.nbytes
            r[key] = a
        out.append(r)
    assert at == len(raw)
    return out


def same_bits(a, b) -> list:
    """names of the outputs whose BITS differ (floats compared as integers: NaN payloads and the sign of zero count)"""
    bad = []
    for k in ("norm2d", "landmarks_3d", "landmarks_flag", "count_3d"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad.append(k)
    return bad
