"""Seeded inputs of the stereo-landmark stage (csrc/landmark_plan.h, csrc/landmarks.hip) and the protocol of tests/cpp/landmark_plan_pin.cpp, shared by the CPU
and GPU tests: synthetic rigs (the fisheye rig's four directions, a stereo-pinhole pair), random drone poses (key frame 0: identity) with un-normalised
quaternions, scene points in front of both cameras seen at integer pixels (+- 1 pixel of noise), and injected matches: zero disparity (the point at infinity),
reversed disparity (a point behind the up camera), offsets across the epipolar line on both sides of triangle_thres, indices outside the images."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, FY, CX, CY, THRES, BASELINE = 300.0, 299.5, 300.25, 239.75, 0.006, 0.10
IMG_W, IMG_H = 600, 480
KINDS = ("good", "infinity", "behind", "offset")


def build_pin(tmp_dir) -> str:
    exe = os.path.join(str(tmp_dir), "landmark_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "landmark_plan_pin.cpp")])
    return exe


def quat_from_R(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2          # (a half turn: the directions looking backwards)
    if x > 1e-6:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)])
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    return np.array([(R[0, 2] - R[2, 0]) / (4 * y), (R[0, 1] + R[1, 0]) / (4 * y), y, (R[1, 2] + R[2, 1]) / (4 * y)])


def quat_R(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rig(dirs):
    """[dirs][7] up, [dirs][7] down: body -> camera (camera axes: x right, y down, z forward).  dirs = 4: the flattened fisheye pair, direction d looks along the
    body x axis turned by 90 deg * d, the cameras +- baseline / 2 along body z; dirs = 1: the forward stereo pair, the right camera a baseline to the right"""
    up, down = [], []
    for d in range(dirs):
        yaw = np.pi / 2 * d
        c, s = np.cos(yaw), np.sin(yaw)
        q = quat_from_R(np.array([[s, 0, c], [-c, 0, s], [0, -1, 0]]))
        if dirs == 1:
            up.append(np.r_[0, 0, 0, q]); down.append(np.r_[0, -BASELINE, 0, q])
        else:
            up.append(np.r_[0, 0, BASELINE / 2, q]); down.append(np.r_[0, 0, -BASELINE / 2, 1.7 * q])      # (an un-normalised quaternion)
    return np.array(up), np.array(down)


def model(omni, dirs, accept_min):
    up, down = rig(dirs)
    return omni.capi.stereo_model(FX, FY, CX, CY, THRES, accept_min, up, down)


def make_case(omni, seed, dirs, n_keyframes, max_num, accept_min, n_kps, n_matches, bad_indices=False):
    """n_kps [(up, down)] and n_matches per pair (n_matches[p] <= min of the pair's counts).  The returned dict holds the arrays of omni_landmarks_enqueue_dev and
    `kind` [P][M]: what each match was made as (index into KINDS), `offset` [P][M]: the pixels an "offset" match was moved across the epipolar line"""
    rng = np.random.default_rng(seed)
    P, M = dirs * n_keyframes, max_num
    assert len(n_kps) == len(n_matches) == P
    up7, down7 = rig(dirs)
    poses = np.zeros((n_keyframes, 7))
    for k in range(n_keyframes):
        q = rng.standard_normal(4)
        poses[k] = np.r_[rng.uniform(-5, 5, 3), q * rng.uniform(0.5, 2.0)] if k else np.r_[0, 0, 0, 1, 0, 0, 0]
    kps = np.zeros((2 * P, M, 2), np.float32)
    nk = np.zeros(2 * P, np.int32)
    mu, md = np.zeros((P, M), np.int32), np.zeros((P, M), np.int32)
    nm = np.asarray(n_matches, np.int32).copy()
    kind, offset = np.full((P, M), -1, np.int32), np.zeros((P, M), np.int32)
    for p in range(P):
        d = p % dirs
        n_up, n_down = n_kps[p]
        nk[p], nk[P + p] = n_up, n_down
        Ru, Rd = quat_R(up7[d, 3:]), quat_R(down7[d, 3:])
        step = (Rd.T @ (up7[d, :3] - down7[d, :3]))                # the up camera's centre in the down camera's frame: along x (pinhole pair) or y (fisheye pair)
        axis = int(np.argmax(np.abs(step)))                        # the image axis of the epipolar lines
        n = max(n_up, n_down)
        z = rng.uniform(1.0, 8.0, n)
        px = np.stack([rng.integers(40, IMG_W - 40, n), rng.integers(40, IMG_H - 40, n)], 1).astype(np.float64)
        Xu = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1)            # in the up camera's frame
        Xd = (Rd.T @ (Ru @ Xu.T + (up7[d, :3] - down7[d, :3])[:, None])).T
        pd = np.stack([Xd[:, 0] / Xd[:, 2] * FX + CX, Xd[:, 1] / Xd[:, 2] * FY + CY], 1)
        pu_i = px + rng.integers(-1, 2, px.shape)
        pd_i = np.rint(pd) + rng.integers(-1, 2, pd.shape)
        perm = rng.permutation(n_down) if n_down else np.zeros(0, np.int64)                   # scene point j is key point j of the up image, perm[j] of the down image
        m = int(nm[p])
        assert m <= min(n_up, n_down)
        q_idx = np.sort(rng.choice(min(n_up, n_down), m, replace=False)) if m else np.zeros(0, np.int64)
        for i, j in enumerate(q_idx):
            k = (0, 0, 0, 1, 2, 3, 3, 3)[int(rng.integers(0, 8))] if m > 3 else 0
            if k == 1:
                pd_i[j] = pu_i[j]
            elif k == 2:
                pd_i[j] = pu_i[j]
                pd_i[j, axis] -= np.sign(pd[j, axis] - px[j, axis]) * rng.integers(3, 12)      # the disparity of a point behind the cameras
            elif k == 3:
                offset[p, i] = rng.integers(1, 16)
                pd_i[j, 1 - axis] += offset[p, i] * (1 if rng.integers(0, 2) else -1)
            kind[p, i] = k
            mu[p, i], md[p, i] = j, perm[j]
        kps[p, :n_up] = pu_i[:n_up]
        if n_down:
            kps[P + p, perm[:n_down]] = pd_i[:n_down]
        if bad_indices and m >= 4:                                 # indices outside the images: skipped, nothing written through them
            for i, (a, b) in zip(rng.choice(m, 4, replace=False), ((-1, 0), (n_up, 0), (0, n_down), (1 << 30, -(1 << 30)))):
                mu[p, i] = a if a else mu[p, i]
                md[p, i] = b if b else md[p, i]
                kind[p, i] = -2
    return {"model": model(omni, dirs, accept_min), "n_pairs": P, "max_num": M, "poses": poses, "kps_xy": kps, "n_kps": nk, "match_up": mu, "match_down": md,
            "n_matches": nm, "kind": kind, "offset": offset}


def pack(case) -> bytes:
    hdr = np.array([case["n_pairs"], case["max_num"], case["poses"].shape[0], 0], np.int32)
    parts = [hdr.tobytes(), bytes(ctypes.string_at(ctypes.addressof(case["model"]), ctypes.sizeof(case["model"])))]
    parts += [np.ascontiguousarray(case[k], dt).tobytes() for k, dt in (("poses", np.float64), ("kps_xy", np.float32), ("n_kps", np.int32), ("match_up", np.int32),
                                                                       ("match_down", np.int32), ("n_matches", np.int32))]
    return b"".join(parts)


def run_pin(exe, mode, cases) -> list:
    """[{norm2d, landmarks_3d, landmarks_flag, count_3d, ties}] per case"""
    raw = subprocess.run([exe, mode], input=b"".join(pack(c) for c in cases), capture_output=True, check=True).stdout
    out, at = [], 0
    for c in cases:
        P, M = c["n_pairs"], c["max_num"]
        r = {}
        for name, shape, dt in (("norm2d", (2 * P, M, 2), np.float32), ("landmarks_3d", (2 * P, M, 3), np.float32), ("landmarks_flag", (2 * P, M), np.uint8),
                                ("count_3d", (P,), np.int32), ("ties", (1,), np.int32)):
            a = np.frombuffer(raw, dt, int(np.prod(shape)), at).reshape(shape)
            at += a.nbytes
            r[name] = a
        out.append(r)
    assert at == len(raw)
    return out


def same_bits(a, b) -> list:
    """names of the outputs whose BITS differ (floats compared as integers: NaN payloads and the sign of zero count)"""
    bad = []
    for k in ("norm2d", "landmarks_3d", "landmarks_flag", "count_3d"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad.append(k)
    return bad


def gate_cases(omni) -> list:
    """The shapes both gates run (CPU: header against the host functions; GPU: kernel against the header): one and five pairs of one direction, eight pairs of
    four directions (two key frames with poses of their own), max_num 7 / 100 / 200, images with 0, accept_min, accept_min + 1 and max_num key points,
    match lists of 0, 1, 63, 64, 65 (the wave boundary) and n_kps entries, accept_min_3d_pts 3 and the reference's 50, indices outside the images"""
    mk = make_case
    return [
        mk(omni, 1, 1, 1, 7, 3, [(7, 7)], [7]),
        mk(omni, 2, 1, 1, 7, 3, [(7, 5)], [0]),
        mk(omni, 3, 1, 5, 100, 3, [(0, 0), (3, 10), (4, 100), (100, 100), (100, 70)], [0, 3, 1, 100, 65]),
        mk(omni, 4, 1, 5, 100, 3, [(100, 64), (64, 100), (100, 0), (100, 100), (4, 4)], [64, 63, 0, 65, 4], bad_indices=True),
        mk(omni, 5, 1, 5, 200, 50, [(50, 200), (51, 200), (200, 200), (200, 150), (200, 100)], [50, 51, 200, 64, 63]),
        mk(omni, 6, 4, 2, 200, 50, [(200, 200), (200, 180), (51, 60), (50, 60), (200, 200), (0, 0), (170, 200), (200, 1)], [200, 65, 51, 50, 1, 0, 170, 1], bad_indices=True),
        mk(omni, 7, 4, 2, 100, 3, [(100, 100), (3, 3), (4, 4), (100, 90), (63, 64), (64, 65), (65, 63), (100, 100)], [100, 3, 4, 64, 63, 64, 63, 0], bad_indices=True),
    ]
