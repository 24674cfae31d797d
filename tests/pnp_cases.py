"""Seeded inputs of the loop-verification PnP RANSAC (csrc/pnp_plan.h, csrc/pnp.hip) and the protocol of tests/cpp/pnp_plan_pin.cpp, shared by the CPU and GPU
tests.  A case is what compute_relative_pose hands to solvePnPRansac: `count` float-valued 3-D points in front of a camera with a seeded pose and as many
float-valued normalised image points.  A planted share of the image points are the points' projections (+- 1e-3 of noise); the rest are unrelated, spread over
+- 8 normalised units: the reference's threshold is 3 NORMALISED units, so some unrelated points do fall inside a chance model's band, but at share 0 too few for the
stop rule to end a run of 100 iterations early (at 1 000 iterations counts of 65 and more run them all)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIPPED, OK, NO_MODEL, HOST = 0, 1, 2, 3
MAX_N = 2048                                                     # pnp::kMaxN, the entry's cap
COUNTS = (0, 5, 6, 7, 16, 63, 64, 65, 200, 300, 1500, MAX_N)      # 300 lies above the workgroup's 256 lanes, 1500 above 1 024
SHARES = (0.0, 0.3, 0.6, 0.9, 1.0)
HEAD = ("status", "count", "iters_run", "best_iter", "max_good", "ret", "n_inliers")


def build_pin(tmp_dir, sanitize=False) -> str:
    exe = os.path.join(str(tmp_dir), "pnp_plan_pin" + ("_san" if sanitize else ""))
    flags = ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pnp_plan_pin.cpp")])
    return exe


def rotation(rv):
    th = np.linalg.norm(rv)
    if th < 1e-12:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_case(seed, count, share, max_iters, kind="random"):
    """kind: "random" | "coplanar" (every point in one plane of the world) | "duplicated" (every correspondence is one of four)"""
    rng = np.random.default_rng(seed)
    R, t = rotation(rng.uniform(-0.3, 0.3, 3)), rng.uniform(-0.5, 0.5, 3)
    cam = np.stack([rng.uniform(-2, 2, count), rng.uniform(-2, 2, count), rng.uniform(2, 8, count)], 1)      # in front of the camera
    if kind == "coplanar":
        cam[:, 2] = 4.0 + 0.25 * cam[:, 0]
    X = ((cam - t) @ R).astype(np.float32)                                                                  # X_cam = R X + t
    c = X.astype(np.float64) @ R.T + t
    u = rng.uniform(-8, 8, (count, 2))
    inl = rng.permutation(count)[:int(round(share * count))]
    u[inl] = c[inl, :2] / c[inl, 2:] + rng.uniform(-1e-3, 1e-3, (len(inl), 2))
    u = u.astype(np.float32)
    if kind == "duplicated" and count:
        pick = rng.integers(0, 4, count)
        X, u = X[inl[:4]][pick], u[inl[:4]][pick]
    return {"X": np.ascontiguousarray(X), "u": np.ascontiguousarray(u), "count": count, "share": share, "max_iters": max_iters, "seed": seed, "kind": kind,
            "n_inliers_planted": len(inl)}


def pack(c) -> bytes:
    return b"".join([np.array([c["count"], c["max_iters"]], np.int32).tobytes(), c["X"].tobytes(), c["u"].tobytes()])


def run_pin(exe, mode, cases, env=None) -> list:
    """mode: ("plan", R) or ("host",).  [{status, count, iters_run, best_iter, max_good, ret, n_inliers, Rt, pose, mask, inliers}] per case"""
    raw = subprocess.run([exe] + [str(m) for m in mode], input=b"".join(pack(c) for c in cases), capture_output=True, check=True, env=env).stdout
    out, at = [], 0
    for c in cases:
        n = c["count"]
        r = dict(zip(HEAD, (int(v) for v in np.frombuffer(raw, np.int32, 7, at)))); at += 28
        r["Rt"] = np.frombuffer(raw, np.float64, 12, at); at += 96
        r["pose"] = np.frombuffer(raw, np.float64, 12, at); at += 96
        r["mask"] = np.frombuffer(raw, np.uint8, n, at); at += n
        r["inliers"] = np.frombuffer(raw, np.int32, n, at); at += 4 * n
        out.append(r)
    assert at == len(raw)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def differing(a, b) -> list:
    """names of the outputs that differ; Rt and pose are compared by their BITS"""
    bad = [k for k in HEAD if a[k] != b[k]]
    bad += [k for k in ("mask", "inliers") if not np.array_equal(a[k], b[k])]
    bad += [k for k in ("Rt", "pose") if not np.array_equal(bits(a[k]), bits(b[k]))]
    return bad


DEGENERATE = 2              # the last two gate cases are the deliberately degenerate ones


def gate_cases() -> list:
    """Both gates run these (CPU: header against the host functions; GPU: kernel against the header).  100 iterations: every count x planted share.  1 000
    iterations (init_mode): seven counts x shares 0 / 0.3 / 0.9.  7 iterations: three counts x three shares.  Then a coplanar and a duplicated set."""
    cases = [make_case(100 + 10 * i + j, n, s, 100) for i, n in enumerate(COUNTS) for j, s in enumerate(SHARES)]
    cases += [make_case(300 + 10 * i + j, n, s, 1000) for i, n in enumerate((6, 16, 65, 200, 300, 1500, MAX_N)) for j, s in enumerate((0.0, 0.3, 0.9))]
    cases += [make_case(400 + 10 * i + j, n, s, 7) for i, n in enumerate((7, 64, 200)) for j, s in enumerate((0.0, 0.6, 1.0))]
    cases += [make_case(500, 60, 1.0, 100, kind="coplanar"), make_case(501, 40, 1.0, 100, kind="duplicated")]
    return cases


def index_of(cases, count, share, max_iters) -> int:
    return next(i for i, c in enumerate(cases) if (c["count"], c["share"], c["max_iters"], c["kind"]) == (count, share, max_iters, "random"))
