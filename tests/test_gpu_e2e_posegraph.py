"""The 4-DoF pose graph through the key-frame pipeline (KeyframePipeline(..., pose_graph=True): include/omni_host_posegraph.h, host/pose_graph.hpp, csrc/pgo.hip) on
the STEREO_PINHOLE scene of tests/test_gpu_e2e_pcm.py, imported and unchanged: run() of key frames 0..7, drone 2's eight key frames through the wire, run() of key
frames 8..15, then optimize().

The stage only adds outputs.  With the switch off the run is the parent's (RS.check_scene); with it on, the returned hits, candidates, every field of every edge with
its id, the counters, the database's rows and good_edges() equal the switch-off run's: no tolerance.  estimated_poses() equals omni_pgo_solve_host (the g++ build of
the header the kernel runs) on the problem omni_pipeline_pose_graph_problem exports, bit for bit.

Once more with a synthetic drift composed onto the pose_drone of key frames 8..15 of this drone.  The drift is max(10 x the scene's median loop-edge position error,
which the test measures first from the edges of the drift-free run against the scene's true poses; 0.5 m) along x, -0.6 of it along y, and 0.1 rad of yaw.  After
optimize() the RMS position error of this drone's estimated poses against the scene's ground truth is strictly below the odometry's -- no number beyond the drift's
choice."""
import numpy as np
import pytest

from tests import pcm_cases as PC
from tests import test_gpu_e2e_batch_verify as BV
from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_pcm as EP
from tests import test_gpu_e2e_remote_stream as RS
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests import test_gpu_e2e_wire as WT
from tests.test_gpu_e2e_landmarks import files, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the scene)
from tests.test_gpu_e2e_remote_stream import packets               # noqa: F401  (drone 2's key frames 1008..1015 as packets)

pytestmark = pytest.mark.gpu
MB = LM.MB


def true_pose(scene, drone, kf):
    """the scene's pose of a key frame: drone 1's frame k is scene[k]; drone 2's frames 1008.. carry the poses of key frames 8.."""
    return np.asarray(scene[int(kf) if drone == 1 else int(kf) - 1000][1], np.float64)


def run(omni, ctx, files, scene, packets, pose_graph, drift=None, starts=1):
    n = len(scene)
    half = n // 2
    pins = WT.stereo_blocks(ctx, scene, list(range(n)))
    pl, clock = BV.drone1(omni, files, True, False, True, False), RS.Clock()
    try:
        assert pl.pose_graph() == dict(on=False, window=50, starts=1)
        if pose_graph:
            pl.set_pose_graph(True, 50, starts)
            assert pl.pose_graph() == dict(on=True, window=50, starts=starts)
        poses = np.array([pose for _, pose in scene], np.float64)
        if drift is not None:
            for k in range(half, n):
                poses[k] = PC.pmul(drift, poses[k])
        pl.set_poses(0, poses)
        ptrs = [p.ctypes.data for p in pins]
        hits = pl.run(half, 0, ptrs[:half // MB], 0, None, True)
        for frame in packets:
            RS.receive(pl, frame, clock)
        hits += pl.run(half, half, ptrs[half // MB:], 0, None, True)
        assert pl.remote_pending == 0
        out = dict(full=BV.full(pl, hits), good=pl.good_edges(), odom=poses)
        if pose_graph:
            out["status"] = pl.optimize()
            out["est"], out["problem"], out["stats"], out["drift"] = pl.estimated_poses(), pl.pose_graph_problem(), pl.pose_graph_stats(), pl.drift()
            out["full_after"], out["good_after"] = BV.full(pl, 0), pl.good_edges()
        return out
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


def check_against_the_host(omni, r):
    """estimated_poses() == omni_pgo_solve_host on the exported problem, bit for bit; the stats say the same"""
    c = omni.capi
    pr, est, st = r["problem"], r["est"], r["stats"]
    out, hs, best = c.pgo_solve_host(pr["poses"], pr["fixed"], pr["edges"], pr["params"])
    assert best == st["best"] >= 0 and hs[best]["status"] == st["status"] == r["status"]
    assert (hs[best]["iterations"], hs[best]["cg_iterations"]) == (st["iterations"], st["cg_iterations"])
    assert hs[best]["initial_cost"] == st["initial_cost"] and hs[best]["final_cost"] == st["final_cost"]
    assert est["pose"].tobytes() == np.ascontiguousarray(out[best][est["pose_index"]]).tobytes()
    assert np.array_equal(pr["poses"][0][est["pose_index"]], est["init"])
    assert st["poses"] == len(pr["fixed"]) and st["ego_edges"] + st["loop_edges"] == len(pr["edges"]) and st["optimize_calls"] == 1


def test_the_switch_only_adds_outputs_and_the_estimate_equals_the_host(omni, ctx, files, pinhole_scene, packets):
    c = omni.capi
    half = len(pinhole_scene) // 2
    off = run(omni, ctx, files, pinhole_scene, packets, False)
    on = run(omni, ctx, files, pinhole_scene, packets, True)
    RS.check_scene(off["full"], half)
    BV.assert_same(on["full"], off["full"])
    assert on["good"].tobytes() == off["good"].tobytes() == on["good_after"].tobytes() and len(on["good"]) >= 2
    assert np.array_equal(on["full_after"][7], on["full"][7])                       # optimize() adds no edge and takes none
    check_against_the_host(omni, on)
    est, st = on["est"], on["stats"]
    assert list(est["drone"]) == [1] * (2 * half) + [2] * half and list(est["keyframe_id"][:2 * half]) == list(range(2 * half))
    assert st["unreachable_drones"] == 0 and st["loop_edges"] + st["loops_outside"] == len(on["good"]) and st["status"] in (c.PGO_CONVERGED, c.PGO_MAX_ITERATIONS)
    for r in est:                                                                  # the odometry poses are the pose_drone the pipeline was given
        p7 = true_pose(pinhole_scene, int(r["drone"]), r["keyframe_id"])
        assert np.abs(r["odom"][:3] - p7[:3]).max() == 0
    assert list(np.flatnonzero(on["problem"]["fixed"])) == [0] and on["drift"] is not None
    print(f"pose graph on: stats {st}; drift {on['drift']}")


def test_a_synthetic_drift_is_taken_out(omni, ctx, files, pinhole_scene, packets):
    c = omni.capi
    scene, half = pinhole_scene, len(pinhole_scene) // 2
    plain = run(omni, ctx, files, scene, packets, True)
    errs = []
    for e in plain["good"]:
        A, B = true_pose(scene, int(e["drone_id_a"]), e["keyframe_id_a"]), true_pose(scene, int(e["drone_id_b"]), e["keyframe_id_b"])
        errs.append(np.linalg.norm(e["relative_pose"][:3] - PC.pmul(PC.pinv(A), B)[:3]))
    median = float(np.median(errs))
    size = max(10.0 * median, 0.5)
    drift = np.array([size, -0.6 * size, 0.0, np.cos(0.05), 0.0, 0.0, np.sin(0.05)])
    r = run(omni, ctx, files, scene, packets, True, drift)
    check_against_the_host(omni, r)
    est = r["est"]
    me = est["drone"] == 1
    truth = np.array([true_pose(scene, 1, k)[:3] for k in est["keyframe_id"][me]])
    rms_odom = float(np.sqrt(((est["odom"][me][:, :3] - truth) ** 2).sum(1).mean()))
    rms_est = float(np.sqrt(((est["pose"][me][:, :3] - truth) ** 2).sum(1).mean()))
    print(f"median loop-edge position error {median:.4f} m over {len(errs)} edges; drift {size:.3f} m; RMS position error of this drone: odometry {rms_odom:.4f} m, "
          f"estimate {rms_est:.4f} m; stats {r['stats']}; drift() {r['drift']}")
    assert np.linalg.norm(drift[:3]) >= 10.0 * median and len(errs) >= 2
    assert r["stats"]["loop_edges"] >= 1 and r["status"] in (c.PGO_CONVERGED, c.PGO_MAX_ITERATIONS)
    assert rms_est < rms_odom


def test_refusals_and_the_constructor_switch(omni, ctx, files, pinhole_scene):
    from omni_swarm_amd import pipeline
    c, P = omni.capi, SP.PARAMS
    views, pose = pinhole_scene[0]
    pl = LM.make(omni, files, "pinhole", True)
    try:
        for kw, word in ((dict(window=1), "pose_graph_window"), (dict(window=257), "pose_graph_window"), (dict(starts=0), "pose_graph_starts"), (dict(starts=65), "pose_graph_starts")):
            with pytest.raises(c.OmniError, match=word):
                pl.set_pose_graph(True, **kw)
        with pytest.raises(c.OmniError, match="the pose graph is off"):
            pl.optimize()
        pl.set_pose_graph(True, 20, 4)
        assert pl.pose_graph() == dict(on=True, window=20, starts=4)
        assert pl.optimize() == c.PGO_EMPTY and len(pl.estimated_poses()) == 0 and pl.drift() is None        # before any key frame
        pl.set_pose_graph(False)
        assert pl.pose_graph()["on"] is False
        pl.push_keyframe(list(views), 0, 0.0, pose, False)
        pl.flush()
        with pytest.raises(c.OmniError, match="after the first key frame"):
            pl.set_pose_graph(True)
    finally:
        pl.close()
    common = (0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1, P["inner_product_thres"],
              P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"])
    pl = pipeline.KeyframePipeline(*common, geometry=True, stereo_pinhole=SP.STEREO, pose_graph=True, pose_graph_window=30, pose_graph_starts=2)
    try:
        assert pl.pose_graph() == dict(on=True, window=30, starts=2)
    finally:
        pl.close()
    pl = pipeline.KeyframePipeline(*common, geometry=False, stereo_pinhole=SP.STEREO)
    try:
        with pytest.raises(c.OmniError, match="no geometry stage"):
            pl.set_pose_graph(True)
    finally:
        pl.close()
