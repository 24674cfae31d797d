"""Seeded inputs of the lens model (csrc/camera_plan.h) and of the stereo-landmark stage with a camera, and the protocol of tests/cpp/camera_plan_pin.cpp,
shared by the CPU and GPU tests.  Everything about rigs, poses, kinds of injected matches and the seven gate shapes is tests/landmark_cases.py's, imported as
it is: a case is made there for the ideal pinhole and its key points are then moved to where THIS case's camera sees the same rays (cam::project's formulas,
restated in numpy), rounded to whole pixels as a detector reports them -- so the "good" matches are good under the camera, the "behind" ones stay behind.

The restatement of csrc/camera_plan.h in Python (lift_py, project_py) follows the header's specification expression for expression on float64 scalars."""
import ctypes
import math
import os
import subprocess

import numpy as np

from tests import landmark_cases as L

ROOT = L.ROOT
PIXEL_RANGE = (40, 560, 40, 440)          # x0, x1, y0, y1: where landmark_cases draws its pixels from

# name -> (type, k1, k2, p1, p2, xi, fx, fy, cx, cy); the intrinsics are landmark_cases' unless noted
_K = (L.FX, L.FY, L.CX, L.CY)
CAMERAS = {
    "ideal": ("PINHOLE", 0.0, 0.0, 0.0, 0.0, 0.0) + _K,              # passed as NULL / through the entry points without a camera
    "zero": ("PINHOLE", 0.0, 0.0, 0.0, 0.0, 0.0) + _K,               # passed as a model whose coefficients are all 0
    "mild": ("PINHOLE", -0.05, 0.01, 1e-3, -1e-3, 0.0) + _K,
    "barrel": ("PINHOLE", -0.12, 0.02, -4e-4, 7e-4, 0.0) + _K,
    "euroc": ("PINHOLE", -0.2917, 0.08228, 5.333e-5, -1.578e-4, 0.0) + _K,
    # gamma 620: at gamma 300 the rays of this xi pass 90 degrees inside the picture -- the test's concern, not the stage's
    "mei": ("MEI", -0.05, 0.01, 1e-3, -1e-3, 1.2, 620.0, 620.0, L.CX, L.CY),
    # the fixed-point rounds diverge near the picture's corners: inf and NaN flow on (tests' rule for non-finite values)
    "diverging": ("PINHOLE", 0.1, -0.2, 1e-3, 5e-4, 0.0) + _K,
}
GATED = ("mild", "barrel", "euroc", "mei")      # the non-ideal cameras whose outputs are finite over PIXEL_RANGE


def intrinsics(name):
    return np.array(CAMERAS[name][6:], np.float64)


def camera(omni, name):
    t, k1, k2, p1, p2, xi = CAMERAS[name][:6]
    return omni.capi.camera_model(t, k1, k2, p1, p2, xi)


# ---- csrc/camera_plan.h restated ------------------------------------------------------------------------------------------------------------------------------
def _distortion(c, mx, my):
    k1, k2, p1, p2 = (np.float64(v) for v in c[1:5])
    mx2 = mx * mx; my2 = my * my; mxy = mx * my; rho2 = mx2 + my2; rad = k1 * rho2 + k2 * rho2 * rho2
    dx = mx * rad + 2 * p1 * mxy + p2 * (rho2 + 2 * mx2)
    dy = my * rad + 2 * p2 * mxy + p1 * (rho2 + 2 * my2)
    return dx, dy


def lift_py(name, x, y):
    """section 1 of the specification on float64 scalars: x, y float32 pixels -> (x / z, y / z)"""
    c = CAMERAS[name]
    fx, fy, cx, cy = (np.float64(v) for v in c[6:])
    with np.errstate(all="ignore"):
        mx_d = (np.float64(np.float32(x)) - cx) / fx
        my_d = (np.float64(np.float32(y)) - cy) / fy
        mei = c[0] == "MEI"
        mx_u, my_u = mx_d, my_d
        if mei or any(v != 0 for v in c[1:5]):
            dx, dy = _distortion(c, mx_d, my_d)
            mx_u, my_u = mx_d - dx, my_d - dy
            for _ in range((6 if mei else 8) - 1):
                dx, dy = _distortion(c, mx_u, my_u)
                mx_u, my_u = mx_d - dx, my_d - dy
        if not mei:
            return mx_u, my_u
        xi = np.float64(c[5])
        rho2 = mx_u * mx_u + my_u * my_u
        if xi == 1.0:
            z = (1.0 - rho2) / 2.0
        else:
            rad = 1.0 + (1.0 - xi * xi) * rho2
            z = 1.0 - xi * (rho2 + 1.0) / (xi + (np.float64(math.sqrt(rad)) if rad >= 0 else np.float64("nan")))
        return mx_u / z, my_u / z


def project_np(name, X):
    """the forward model on arrays: X [n][3] in the camera's frame -> pixels [n][2] (float64)"""
    c = CAMERAS[name]
    fx, fy, cx, cy = c[6:]
    X = np.asarray(X, np.float64)
    if c[0] == "MEI":
        n = np.sqrt((X * X).sum(1))
        x, y, z = X[:, 0] / n, X[:, 1] / n, X[:, 2] / n + c[5]
        mx, my = x / z, y / z
    else:
        mx, my = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    dx, dy = _distortion(c, mx, my)
    return np.stack([fx * (mx + dx) + cx, fy * (my + dy) + cy], 1)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------
def with_camera(omni, case, name):
    """landmark_cases' case seen through camera `name`: every live key point moved from its ideal-pinhole pixel to the pixel where the camera sees that ray
    (rounded to a whole pixel), the stereo model's intrinsics the camera's"""
    c = dict(case)
    m = type(case["model"]).from_buffer_copy(case["model"])
    m.fx, m.fy, m.cx, m.cy = CAMERAS[name][6:]
    c["model"], c["camera"], c["camera_name"] = m, camera(omni, name), name
    kps = case["kps_xy"].copy()
    if name not in ("ideal", "zero"):
        for img in range(kps.shape[0]):
            n = int(case["n_kps"][img])
            if n:
                p = kps[img, :n].astype(np.float64)
                rays = np.stack([(p[:, 0] - L.CX) / L.FX, (p[:, 1] - L.CY) / L.FY, np.ones(n)], 1)
                kps[img, :n] = np.rint(project_np(name, rays)).astype(np.float32)
    c["kps_xy"] = kps
    return c


def infinity_keypoints(case) -> np.ndarray:
    """[2P][M] bool: the key points of the matches landmark_cases made with zero disparity (kind "infinity").  Their rays are parallel, so the triangulated
    point is a finite direction over a homogeneous coordinate that may round to 0: landmark_cases' own gate cases, ideal pinhole, hold such +-inf landmarks at
    these key points already (its cases 5 and 6) and compare them by their bits."""
    P, M = case["n_pairs"], case["max_num"]
    mask = np.zeros((2 * P, M), bool)
    for p in range(P):
        for i in range(int(case["n_matches"][p])):
            if case["kind"][p, i] == 1:
                mask[p, case["match_up"][p, i]] = mask[P + p, case["match_down"][p, i]] = True
    return mask


def gate_cases(omni, name) -> list:
    """landmark_cases.gate_cases (1, 5 and 8 pairs; max_num 7 / 100 / 200; 0, accept_min, accept_min + 1 and max_num key points; 0, 1, 63, 64, 65 and n_kps
    matches; 1 and 4 directions) through camera `name`"""
    return [with_camera(omni, c, name) for c in L.gate_cases(omni)]


def diverging_pixels(pin):
    """whole pixels of PIXEL_RANGE where the `diverging` camera's lift is not finite, by the g++ build"""
    x0, x1, y0, y1 = PIXEL_RANGE
    xs, ys = np.meshgrid(np.arange(x0, x1 + 1, 2, dtype=np.float32), np.arange(y0, y1 + 1, 2, dtype=np.float32))
    grid = np.stack([xs.ravel(), ys.ravel()], 1)
    out = run_points(pin, "lift", "diverging", grid)
    return grid[~np.isfinite(out).all(1)], len(grid)


def diverging_cases(omni, pin) -> list:
    """two gate shapes (5 pairs of one direction; 8 pairs of four) through the `diverging` camera, with every third key point of every image put on a pixel
    where that camera's lift is inf or NaN"""
    bad, _ = diverging_pixels(pin)
    assert len(bad) >= 50
    rng = np.random.default_rng(99)
    out = []
    for base in (L.gate_cases(omni)[3], L.gate_cases(omni)[6]):
        c = with_camera(omni, base, "diverging")
        for img in range(c["kps_xy"].shape[0]):
            n = int(c["n_kps"][img])
            idx = np.arange(0, n, 3)
            c["kps_xy"][img, idx] = bad[rng.integers(0, len(bad), len(idx))]
        out.append(c)
    return out


# ---- tests/cpp/camera_plan_pin.cpp ----------------------------------------------------------------------------------------------------------------------------
def build_pin(tmp_dir, sanitize=False) -> str:
    exe = os.path.join(str(tmp_dir), "camera_plan_pin" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "cpp", "camera_plan_pin.cpp")])
    return exe


def _struct_bytes(s) -> bytes:
    return bytes(ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s)))


def run_points(exe, mode, name, pts, omni=None) -> np.ndarray:
    """mode lift / lmlift (pts [n][2] float32 pixels) or project (pts [n][3] float64): [n][2] float64"""
    import omni_loader
    omni = omni or omni_loader.load()
    pts = np.ascontiguousarray(pts, np.float64 if mode == "project" else np.float32)
    rec = np.array([len(pts), 0], np.int32).tobytes() + _struct_bytes(camera(omni, name)) + intrinsics(name).tobytes() + pts.tobytes()
    raw = subprocess.run([exe, mode], input=rec, capture_output=True, check=True).stdout
    return np.frombuffer(raw, np.float64).reshape(len(pts), 2)


def pack(case) -> bytes:
    hdr = np.array([case["n_pairs"], case["max_num"], case["poses"].shape[0], 0], np.int32)
    parts = [hdr.tobytes(), _struct_bytes(case["model"]), _struct_bytes(case["camera"])]
    parts += [np.ascontiguousarray(case[k], dt).tobytes() for k, dt in (("poses", np.float64), ("kps_xy", np.float32), ("n_kps", np.int32), ("match_up", np.int32),
                                                                       ("match_down", np.int32), ("n_matches", np.int32))]
    return b"".join(parts)


def run_pin(exe, mode, cases) -> list:
    """[{norm2d, landmarks_3d, landmarks_flag, count_3d, ties}] per case (landmark_cases.run_pin's output)"""
    raw = subprocess.run([exe, mode], input=b"".join(pack(c) for c in cases), capture_output=True, check=True).stdout
    out, at = [], 0
    for c in cases:
        P, M = c["n_pairs"], c["max_num"]
        r = {}
        for key, shape, dt in (("norm2d", (2 * P, M, 2), np.float32), ("landmarks_3d", (2 * P, M, 3), np.float32), ("landmarks_flag", (2 * P, M), np.uint8),
                               ("count_3d", (P,), np.int32), ("ties", (1,), np.int32)):
            a = np.frombuffer(raw, dt, int(np.prod(shape)), at).reshape(shape)
            at += a.nbytes
            r[key] = a
        out.append(r)
    assert at == len(raw)
    return out


def run_depth(exe, omni, name, intr, near, far, accept_min, pose7, ext7, kps, depth) -> dict:
    """PINHOLE_DEPTH's host path (fill_image_descriptor + fill_depth_landmarks with the model's lift) on one image's key points [n][2] and depth image u16 [H][W]"""
    kps, depth = np.ascontiguousarray(kps, np.float32).reshape(-1, 2), np.ascontiguousarray(depth, np.uint16)
    n = len(kps)
    rec = (np.array([n, depth.shape[1], depth.shape[0], accept_min], np.int32).tobytes() + _struct_bytes(camera(omni, name)) +
           np.array(list(intr) + [near, far], np.float64).tobytes() + np.ascontiguousarray(pose7, np.float64).tobytes() + np.ascontiguousarray(ext7, np.float64).tobytes() +
           kps.tobytes() + depth.tobytes())
    raw = subprocess.run([exe, "depth"], input=rec, capture_output=True, check=True).stdout
    assert len(raw) == n * (8 + 12 + 1) + 4
    return {"norm2d": np.frombuffer(raw, np.float32, 2 * n, 0).reshape(n, 2), "landmarks_3d": np.frombuffer(raw, np.float32, 3 * n, 8 * n).reshape(n, 3),
            "landmarks_flag": np.frombuffer(raw, np.uint8, n, 20 * n), "count_3d": int(np.frombuffer(raw, np.int32, 1, 21 * n)[0])}


def same_where_finite(a, b) -> list:
    """the rule for a camera that diverges: flags and counts equal, the isnan and isinf masks equal, every finite value equal in its bits; returns what is not"""
    bad = []
    for k in ("landmarks_flag", "count_3d"):
        if not np.array_equal(a[k], b[k]):
            bad.append(k)
    for k in ("norm2d", "landmarks_3d"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)) or not np.array_equal(np.isinf(x), np.isinf(y)):
            bad.append(k + " masks")
            continue
        fin = np.isfinite(x)
        if not np.array_equal(x.view(np.uint32)[fin], y.view(np.uint32)[fin]):
            bad.append(k)
    return bad
