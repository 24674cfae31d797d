"""SwarmPoseGraph (host/pose_graph.hpp) through omni_pose_graph_build_host of libomni_host_posegraph.so, without a GPU and without a pipeline: the window cut, merged
zero-length steps, ego-motion edges, loop edges inside and outside the window, the breadth-first initial values against the restatement of tests/pgo_cases.py
(4 x 4 matrices), an unreachable drone counted and left out, the constant pose, the further starts, the refusals -- and, the conventions taken together, that a
problem built from exact odometry and exact loops has no cost at its initial values and is solved by omni_pgo_solve_host once this drone's odometry drifts.

The scene: drones 1 (this one, 60 key frames, two of them identical), 2 (30), 3 (20) and 4 (10; no edge reaches it) fly random walks; drone d's odometry frame sits at
G_d in the world, so its odometry pose is inverse(G_d) . truth.  Loops: 1 -> 2, 3 -> 2 (it reaches drone 3 against its direction), 2 -> 1, one to a frame of drone 1
older than the window, one of drone 4 with itself, one between the two identical frames."""
import numpy as np
import pytest

from tests import pgo_cases as PC

SELF, WINDOW = 1, 50
LENGTHS = {1: 60, 2: 30, 3: 20, 4: 10}
SAME = (55, 56)                       # key frames of drone 1 with one pose


def quat7(p):
    return np.array([p[0], p[1], p[2], np.cos(p[3] / 2), 0.0, 0.0, np.sin(p[3] / 2)])


def inv_restated(a):
    return PC.unmat(np.linalg.inv(PC.mat(a)))


@pytest.fixture(scope="module")
def scene(omni):
    from omni_swarm_amd import pipeline as P
    rng = np.random.default_rng(12)
    G = {d: np.array([3.0 * d * rng.normal(), 3.0 * d * rng.normal(), 0.2 * d, rng.uniform(-3, 3)]) for d in LENGTHS}
    G[SELF] = np.zeros(4)
    truth, odom = {}, {}
    for d, n in LENGTHS.items():
        truth[d] = PC.walk(rng, n, np.array([rng.normal(), rng.normal(), 0.1, rng.uniform(-3, 3)]))
        if d == SELF:
            truth[d][SAME[1]] = truth[d][SAME[0]]
        odom[d] = np.array([PC.delta_restated(G[d], t) for t in truth[d]])
    kf = []
    for k in range(max(LENGTHS.values())):          # interleaved arrival, as a pipeline sees them
        for d, n in LENGTHS.items():
            if k < n:
                kf.append((d, 0, 1000 * d + k, quat7(odom[d][k])))
    kf = np.array(kf, P.POSE_GRAPH_KEYFRAME_DTYPE)

    def loop(i, da, ka, db, kb):
        e = np.zeros((), P.REMOTE_EDGE_DTYPE)
        e["id"], e["drone_id_a"], e["drone_id_b"], e["keyframe_id_a"], e["keyframe_id_b"] = i, da, db, 1000 * da + ka, 1000 * db + kb
        e["relative_pose"] = quat7(PC.delta_restated(truth[da][ka], truth[db][kb]))
        e["pos_cov"], e["ang_cov"] = [0.01, 0.04, 0.0025], [0.5, 0.5, 0.0001]
        return e

    loops = np.array([loop(0, 1, 3, 2, 4), loop(1, 1, 30, 2, 5), loop(2, 3, 7, 2, 20), loop(3, 2, 25, 1, 58), loop(4, 4, 1, 4, 8), loop(5, 1, SAME[0], 1, SAME[1]),
                      loop(6, 3, 15, 1, 40)], P.REMOTE_EDGE_DTYPE)
    return P, kf, loops, truth, odom, G


def test_window_merge_edges_and_the_constant_pose(omni, scene):
    c = omni.capi
    P, kf, loops, truth, odom, G = scene
    b = P.pose_graph_build_host(kf, loops, SELF, WINDOW, 1, 0.01, 0.003)
    f = b["frames"]
    assert [int((f["drone"] == d).sum()) for d in (1, 2, 3, 4)] == [50, 30, 20, 0] and b["unreachable_drones"] == 1
    assert list(f["keyframe_id"][f["drone"] == 1]) == [1000 + k for k in range(10, 60)]          # the window cut: the last 50, oldest first
    assert list(f["drone"]) == sorted(f["drone"])
    # the two identical key frames share a pose; every other frame has its own, in order
    i0, i1 = (int(np.flatnonzero(f["keyframe_id"] == 1000 + k)[0]) for k in SAME)
    assert b["merged"] == 1 and f["pose_index"][i0] == f["pose_index"][i1] and len(b["fixed"]) == 99
    assert np.array_equal(np.unique(f["pose_index"]), np.arange(99)) and (np.diff(f["pose_index"]) >= 0).all()
    for r in f:
        assert np.abs(r["odom"] - odom[int(r["drone"])][int(r["keyframe_id"]) % 1000] + 0).max() < 1e-12
    # the constant pose: the oldest window pose of this drone and no other
    assert list(np.flatnonzero(b["fixed"])) == [int(f["pose_index"][0])] and f["keyframe_id"][0] == 1010
    # ego-motion edges: consecutive poses of a drone, DeltaPose of the odometry, covariance = step length x per-metre, no loss
    e = b["edges"]
    assert b["ego_edges"] == 99 - 3 and not e["robust"][:96].any() and e["robust"][96:].all()
    first = {}
    for r in f:
        first.setdefault(int(r["pose_index"]), r)
    for k in range(96):
        a, bb = first[int(e["i"][k])], first[int(e["j"][k])]
        assert e["j"][k] == e["i"][k] + 1 and a["drone"] == bb["drone"]
        assert np.abs(e["z"][k] - PC.delta_restated(a["odom"], bb["odom"])).max() < 1e-12
        step = np.linalg.norm(bb["odom"][:3] - a["odom"][:3])
        assert np.allclose(e["sqrt_inf"][k], 1 / np.sqrt(step * np.array([0.01, 0.01, 0.01, 0.003])), rtol=1e-12)
    # loop edges: those with both frames in the window, in order; the one to an old frame, drone 4's and the one inside a merged pose are outside
    assert b["loop_edges"] == 4 and b["loops_outside"] == 3 and len(e) == 100
    pose_of = {(int(r["drone"]), int(r["keyframe_id"])): int(r["pose_index"]) for r in f}
    for k, l in zip(range(96, 100), loops[[1, 2, 3, 6]]):
        assert e["i"][k] == pose_of[int(l["drone_id_a"]), int(l["keyframe_id_a"])] and e["j"][k] == pose_of[int(l["drone_id_b"]), int(l["keyframe_id_b"])]
        want = PC.delta_restated(truth[int(l["drone_id_a"])][int(l["keyframe_id_a"]) % 1000], truth[int(l["drone_id_b"])][int(l["keyframe_id_b"]) % 1000])
        assert np.abs(e["z"][k] - want).max() < 1e-12
        assert np.allclose(e["sqrt_inf"][k], [10.0, 5.0, 20.0, 100.0], rtol=1e-12)               # 1 / sqrt(pos_cov xyz, ang_cov[2])


def test_breadth_first_initial_values_equal_the_restatement(omni, scene):
    c = omni.capi
    P, kf, loops, truth, odom, G = scene
    b = P.pose_graph_build_host(kf, loops, SELF, WINDOW, 1)
    f = b["frames"]
    # the restatement: drone 2 through loop 1 (1 -> 2; loop 0's frame of drone 1 is older than the window), drone 3 through loop 2 against its direction
    off1 = np.zeros(4)
    rel = PC.delta_restated(truth[1][30], truth[2][5])
    off2 = PC.mul_restated(PC.mul_restated(PC.mul_restated(off1, odom[1][30]), rel), inv_restated(odom[2][5]))
    rel = inv_restated(PC.delta_restated(truth[3][7], truth[2][20]))
    off3 = PC.mul_restated(PC.mul_restated(PC.mul_restated(off2, odom[2][20]), rel), inv_restated(odom[3][7]))
    off = {1: off1, 2: off2, 3: off3}
    worst = 0.0
    for r in f:
        want = PC.mul_restated(off[int(r["drone"])], r["odom"])
        d = r["init"] - want
        worst = max(worst, np.abs(d[:3]).max(), abs(PC.wrap(d[3])))
        assert np.array_equal(r["init"], r["pose"])
    print(f"initial values: largest difference from the restatement {worst:.2e}")
    assert worst < 1e-9               # poses of ~30 m through four compositions, each rounded at 1e-16 relative: 1e-13 expected
    assert np.array_equal(b["poses"][0][f["pose_index"]], f["init"])
    # exact odometry and exact loops: the offsets are the drones' frames in this drone's, the initial values are the truth, and the problem has no cost there
    for r in f:
        t = truth[int(r["drone"])][int(r["keyframe_id"]) % 1000]
        assert np.abs(r["init"][:3] - t[:3]).max() < 1e-9 and abs(PC.wrap(r["init"][3] - t[3])) < 1e-9
    _, _, _, cost = c.pgo_residuals_host(b["poses"][0], b["edges"])
    assert cost.sum() < 1e-18


def test_a_drifting_odometry_is_corrected_by_the_host_solver(omni, scene):
    c = omni.capi
    P, kf, loops, truth, odom, G = scene
    kf2 = kf.copy()
    drift = np.array([1.5, -1.0, 0.3, 0.2])
    for r in kf2:
        if r["drone"] == SELF and r["keyframe_id"] >= 1035:
            x, y, z, w, _, _, s = r["pose"]
            r["pose"] = quat7(PC.mul_restated(drift, np.array([x, y, z, 2 * np.arctan2(s, w)])))
    b = P.pose_graph_build_host(kf2, loops, SELF, WINDOW, 1)
    out, st, best = c.pgo_solve_host(b["poses"], b["fixed"], b["edges"])
    f = b["frames"]
    me = f["drone"] == SELF
    t = np.array([truth[SELF][int(k) % 1000] for k in f["keyframe_id"][me]])
    rms_odom = np.sqrt(((f["odom"][me][:, :3] - t[:, :3]) ** 2).sum(1).mean())
    rms_est = np.sqrt(((out[0][f["pose_index"][me]][:, :3] - t[:, :3]) ** 2).sum(1).mean())
    print(f"RMS position error of this drone: odometry {rms_odom:.3f} m, estimate {rms_est:.3f} m; status {st[0]}")
    assert best == 0 and st[0]["status"] == c.PGO_CONVERGED and rms_est < rms_odom and rms_odom > 1.0


def test_further_starts_turn_the_other_drones_about_their_oldest_pose(omni, scene):
    P, kf, loops, truth, odom, G = scene
    b = P.pose_graph_build_host(kf, loops, SELF, WINDOW, 3)
    f, x = b["frames"], b["poses"]
    assert x.shape == (3, 99, 4) and np.array_equal(x[0][f["pose_index"]], f["init"])
    for s in (1, 2):
        for d in (1, 2, 3):
            idx = f["pose_index"][f["drone"] == d]
            if d == SELF:
                assert np.array_equal(x[s][idx], x[0][idx])
                continue
            turn = np.array([0, 0, 0, 2 * np.pi * s / 3])
            piv = x[0][idx[0]]
            for v in idx:
                want = PC.mul_restated(piv, PC.mul_restated(turn, PC.mul_restated(inv_restated(piv), x[0][v])))
                dd = x[s][v] - want
                assert np.abs(dd[:3]).max() < 1e-9 and abs(PC.wrap(dd[3])) < 1e-9
            assert np.abs(x[s][idx[0]][:3] - piv[:3]).max() < 1e-9


def test_no_frame_of_this_drone_and_the_refusals(omni, scene):
    c = omni.capi
    P, kf, loops, truth, odom, G = scene
    b = P.pose_graph_build_host(kf[kf["drone"] != SELF], loops, SELF, WINDOW, 1)
    assert len(b["frames"]) == 0 and b["unreachable_drones"] == 3 and len(b["fixed"]) == 0 and len(b["edges"]) == 0
    b = P.pose_graph_build_host(kf, loops[:0], SELF, 2, 1)
    assert len(b["frames"]) == 2 and b["unreachable_drones"] == 3 and b["ego_edges"] == 1 and list(b["fixed"]) == [1, 0]
    for kw, word in ((dict(window=1), "window"), (dict(window=257), "window"), (dict(starts=0), "starts"), (dict(starts=65), "starts")):
        with pytest.raises(c.OmniError, match=word):
            P.pose_graph_build_host(kf, loops, SELF, **kw)
    L = P.posegraph_lib()
    assert L.omni_pipeline_set_pose_graph(None, 1, 50, 1) == 1 and b"null pipeline" in L.omni_posegraph_host_last_error()
    assert L.omni_pipeline_optimize(None, None) == 1 and L.omni_pipeline_estimated_poses(None, None, 0, None) == 1
    assert L.omni_pipeline_pose_graph_stats(None, None, None) == 1 and L.omni_pipeline_pose_graph_problem(None, None, None, None, 0, None, 0, None) == 1


def test_library_exports_what_its_c_header_declares(omni):
    import os
    import re
    import subprocess
    from omni_swarm_amd import pipeline as P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, "include", "omni_host_posegraph.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", P.POSEGRAPH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("omni_")}
    assert declared == exported == set(P.POSEGRAPH_SYMBOLS)
    assert P.POSE_GRAPH_FRAME_DTYPE.itemsize == 112 and P.POSE_GRAPH_KEYFRAME_DTYPE.itemsize == 72
    mk = open(os.path.join(root, "omni-swarm_amd", "Makefile")).read()
    assert "lib/libomni_host_posegraph.so" in mk.split("all:")[1].splitlines()[0]
