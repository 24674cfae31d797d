"""Seeded inputs of the loop-verification RANSAC (csrc/ransac_plan.h, csrc/homography.hip) and the protocol of tests/cpp/ransac_plan_pin.cpp, shared by the CPU
and GPU tests.  A case is what the image-pair compute_correspond_features sees behind its matcher: the new and the old image's key points (float pixels of a
600 x 480 image), the new image's landmark flags and a cross-checked match list.  `count` matches are flagged; a planted share of them follows one homography
(+- 0.5 pixel), the rest are unrelated points; further matches whose key point has no flag (or lies behind the flag array's end) are mixed in where asked."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_W, IMG_H = 600, 480
UNFILTERED, OK, NO_MODEL, HOST = 0, 1, 2, 3
COUNTS = (0, 3, 4, 5, 6, 30, 63, 64, 65, 200)
SHARES = (0.0, 0.3, 0.6, 0.9, 1.0)
HEAD = ("status", "n_kept", "count", "iters_run", "best_iter", "max_good", "ties", "ret", "n_reduced")


def build_pin(tmp_dir) -> str:
    exe = os.path.join(str(tmp_dir), "ransac_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ransac_plan_pin.cpp")])
    return exe


def make_case(seed, count, share, dropped=0, short_flags=False, kind="random"):
    """count flagged matches + `dropped` unflagged ones, in ascending query order.  short_flags: the flag array ends in front of the last key points, so some
    matches are dropped by `queryIdx >= n_flags`.  kind: "random" | "duplicated" (every point is one of three places) | "collinear" (all on one line)."""
    rng = np.random.default_rng(seed)
    n = count + dropped
    nq, nt = n + int(rng.integers(0, 5)), n + int(rng.integers(0, 5))
    q_idx = np.sort(rng.choice(nq, n, replace=False)).astype(np.int32) if n else np.zeros(0, np.int32)
    t_idx = rng.choice(nt, n, replace=False).astype(np.int32) if n else np.zeros(0, np.int32)
    old = np.stack([rng.uniform(20, IMG_W - 20, nt), rng.uniform(20, IMG_H - 20, nt)], 1)
    new = np.stack([rng.uniform(20, IMG_W - 20, nq), rng.uniform(20, IMG_H - 20, nq)], 1)
    a = rng.uniform(-0.2, 0.2)
    H = np.array([[np.cos(a), -np.sin(a), rng.uniform(-30, 30)], [np.sin(a), np.cos(a), rng.uniform(-30, 30)], [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])
    H[:2, :2] *= rng.uniform(0.9, 1.1)
    is_drop = np.zeros(n, bool)
    if dropped:
        is_drop[rng.choice(n, dropped, replace=False)] = True
    kept = np.flatnonzero(~is_drop)
    inl = kept[rng.permutation(len(kept))[:int(round(share * len(kept)))]]
    if kind == "duplicated":
        places = np.stack([rng.uniform(50, IMG_W - 50, 3), rng.uniform(50, IMG_H - 50, 3)], 1)
        old[t_idx] = places[rng.integers(0, 3, n)]
        new[q_idx] = old[t_idx] + 2.0
    elif kind == "collinear":
        k = rng.choice(200, n, replace=False).astype(np.float64)      # whole pixels: the cross products are exactly 0
        old[t_idx] = np.stack([40 + 2 * k, 60 + k], 1)
        new[q_idx] = np.stack([500 - 2 * k, 50 + 2 * k], 1)
    else:
        p = np.c_[old[t_idx[inl]], np.ones(len(inl))] @ H.T
        new[q_idx[inl]] = p[:, :2] / p[:, 2:] + rng.uniform(-0.5, 0.5, (len(inl), 2))
    flags = np.zeros(nq, np.uint8)
    flags[q_idx[kept]] = 1
    n_flags = nq
    if short_flags and n:                                    # cut the array behind a flagged key point: the matches above it are dropped by the length test
        n_flags = int(q_idx[kept[len(kept) * 2 // 3]]) + 1 if len(kept) else 0
    return {"q_idx": q_idx, "t_idx": t_idx, "q_xy": new.astype(np.float32), "t_xy": old.astype(np.float32), "flags": flags[:n_flags].copy(), "seed": seed, "count": count,
            "share": share, "kind": kind, "n_inliers_planted": len(inl)}


def pack(c) -> bytes:
    hdr = np.array([len(c["q_idx"]), len(c["q_xy"]), len(c["t_xy"]), len(c["flags"])], np.int32)
    return b"".join([hdr.tobytes(), c["q_idx"].tobytes(), c["t_idx"].tobytes(), np.ascontiguousarray(c["q_xy"], np.float32).tobytes(),
                     np.ascontiguousarray(c["t_xy"], np.float32).tobytes(), np.ascontiguousarray(c["flags"], np.uint8).tobytes()])


def run_pin(exe, mode, cases) -> list:
    """mode: ("plan", R) or ("host",).  [{status, n_kept, count, iters_run, best_iter, max_good, ties, ret, n_reduced, H, kept, new_idx, old_idx, mask}] per case"""
    raw = subprocess.run([exe] + [str(m) for m in mode], input=b"".join(pack(c) for c in cases), capture_output=True, check=True).stdout
    out, at = [], 0
    for c in cases:
        n = len(c["q_idx"])
        head = np.frombuffer(raw, np.int32, 9, at); at += 36
        r = dict(zip(HEAD, (int(v) for v in head)))
        r["H"] = np.frombuffer(raw, np.float64, 9, at); at += 72
        for name in ("kept", "new_idx", "old_idx"):
            r[name] = np.frombuffer(raw, np.int32, n, at); at += 4 * n
        r["mask"] = np.frombuffer(raw, np.uint8, n, at); at += n
        out.append(r)
    assert at == len(raw)
    return out


def differing(a, b) -> list:
    """names of the outputs that differ; H is compared by its BITS"""
    bad = [k for k in HEAD if k != "ties" and a[k] != b[k]]
    bad += [k for k in ("kept", "new_idx", "old_idx", "mask") if not np.array_equal(a[k], b[k])]
    if not np.array_equal(np.ascontiguousarray(a["H"]).view(np.uint64), np.ascontiguousarray(b["H"]).view(np.uint64)):
        bad.append("H")
    return bad


def point_lists(c, r):
    """the RANSAC's own input of a case: src (old image) / dst (new image) [n_kept][2] of the matches the pin kept"""
    k = r["kept"][:r["n_kept"]]
    return c["t_xy"][c["t_idx"][k]], c["q_xy"][c["q_idx"][k]]


def find_no_subset_seed(exe, first=1000, n=400) -> int:
    """a count-5 pair with no valid subset: unrelated points, none of whose 120 ordered subsets keeps its orientation"""
    cases = [make_case(s, 5, 0.0) for s in range(first, first + n)]
    for s, r in zip(range(first, first + n), run_pin(exe, ("plan", 64), cases)):
        if r["status"] == NO_MODEL and r["iters_run"] == 0:
            return s
    raise AssertionError("no count-5 pair without a valid subset among the seeds searched")


NO_SUBSET_SEED = 1010       # (find_no_subset_seed's answer; tests/test_ransac_plan_cpu.py checks that it still is one)
DEGENERATE = 2              # the last two gate cases are the deliberately degenerate ones


def gate_cases() -> list:
    """Both gates run these (CPU: header against the host functions; GPU: kernels against the header): every count x planted share, no match dropped; counts
    with matches dropped by a zero flag and by the flag array's length; all matches dropped; the count-5 pair without a valid subset; duplicated and collinear
    points (LAST: they come back HOST)"""
    cases = [make_case(100 + 10 * i + j, n, s) for i, n in enumerate(COUNTS) for j, s in enumerate(SHARES)]
    cases += [make_case(300 + i, n, 0.6, dropped=d) for i, (n, d) in enumerate(((3, 5), (4, 2), (5, 40), (30, 30), (64, 1), (200, 56)))]
    cases += [make_case(320 + i, n, 0.9, dropped=d, short_flags=True) for i, (n, d) in enumerate(((6, 3), (30, 10), (65, 65)))]
    cases += [make_case(330, 0, 0.0, dropped=30), make_case(331, 0, 0.0, dropped=1)]
    cases.append(make_case(NO_SUBSET_SEED, 5, 0.0))
    cases += [make_case(340, 30, 0.0, kind="duplicated"), make_case(341, 64, 0.0, kind="collinear")]
    return cases
