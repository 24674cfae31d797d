"""The key-frame pipeline with the PnP RANSAC of its loop candidates on the GPU (KeyframePipeline(..., device_pnp=True): one omni_pnp_ransac_multi call per
candidate from its geometry task, csrc/pnp.hip; the refit stays on the host) against the same pipeline running geom::solve_pnp_ransac whole on the host's geometry
threads (device_pnp=False, the default), on the rendered scenes of tests/test_gpu_e2e_landmarks.py (STEREO_FISHEYE, 600 x 480, eight places and their revisits;
STEREO_PINHOLE, raw 750 x 600 pairs): candidates, EVERY field of every edge and the geometry counters are identical -- the mask and the best model are the same,
so the refit and everything downstream are -- both through run() and through push_keyframe / flush; no candidate is handed back to the host.  The pipeline's own
key frames are the self drone's and run compute_relative_pose's 100-iteration limit; init_mode (1 000 iterations, the lower gates) is what a frame of ANOTHER
drone gets, verified on the spot by the detector's callback: the last test hands stored key frames to the detector again as another drone's
(omni_pipeline_recv_copy_as_remote) with the switch on and off."""
import numpy as np
import pytest

from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_scene as FE
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests.test_gpu_e2e_landmarks import files, fisheye_scene, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the two scenes)

pytestmark = pytest.mark.gpu
MB = LM.MB


def make(omni, files, scene_kind, device_pnp):
    from omni_swarm_amd import pipeline
    c = omni.capi
    E, extra = (FE, {}) if scene_kind == "fisheye" else (SP, {"stereo_pinhole": SP.STEREO})
    P = E.PARAMS
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], E.W, E.H, E.THR, E.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, device_pnp=device_pnp, **extra)
    if scene_kind != "fisheye":
        pl.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
    return pl


def through(omni, ctx, files, scene_kind, scene, device_pnp, streaming):
    """-> (hits, candidates, edges, geometry stats, database rows, (switch, pairs from the device, pairs handed back))"""
    n, dirs = len(scene), scene[0][0].shape[0] // 2
    pl = make(omni, files, scene_kind, device_pnp)
    pins = []
    try:
        assert pl.device_pnp() == (device_pnp, 0, 0)
        if streaming:
            hits = 0
            for i, (views, pose) in enumerate(scene):
                hits += pl.push_keyframe(list(views), i, float(i), pose, False)
            hits += pl.flush()
        else:
            for s in range(0, n, MB):
                kf = [scene[s + m][0] for m in range(MB)]
                p = ctx.host_alloc((2 * dirs * MB,) + kf[0].shape[1:], np.uint8)
                p[:] = np.stack([kf[m][i] for m in range(MB) for i in range(dirs)] + [kf[m][dirs + i] for m in range(MB) for i in range(dirs)])
                pins.append(p)
            pl.set_poses(0, np.array([pose for _, pose in scene]))
            hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
        return hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows, pl.device_pnp()
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


@pytest.mark.parametrize("streaming", [False, True], ids=["run", "push_keyframe"])
@pytest.mark.parametrize("scene_kind", ["fisheye", "pinhole"])
def test_device_pnp_changes_nothing_downstream(omni, ctx, files, fisheye_scene, pinhole_scene, scene_kind, streaming):
    scene = fisheye_scene if scene_kind == "fisheye" else pinhole_scene
    assert len(scene) % MB == 0
    host = through(omni, ctx, files, scene_kind, scene, False, streaming)
    dev = through(omni, ctx, files, scene_kind, scene, True, streaming)
    print(f"{scene_kind}, {'push_keyframe' if streaming else 'run'}: {len(scene)} key frames, hits {host[0]} / {dev[0]}, candidates {len(host[1])}, edges {len(host[2])} / {len(dev[2])}, "
          f"geometry (calls, edges) {host[3]} / {dev[3]}, rows {host[4]}; candidates served by the device {dev[5][1]}, handed back to the host {dev[5][2]}")
    assert len(host[1]) >= 4 and len(host[2]) >= 2 and len(host[1]) > len(host[2])      # not vacuous: accepted edges AND rejected candidates
    assert dev[0] == host[0] and dev[3] == host[3] and dev[4] == host[4]
    assert np.array_equal(dev[1], host[1])
    assert dev[2].shape == host[2].shape and np.array_equal(dev[2], host[2])            # every field of every edge, bit for bit
    assert host[5] == (False, 0, 0)
    assert dev[5][0] is True and dev[5][1] >= len(host[2]) and dev[5][2] == 0           # every accepted edge went through the device; no candidate fell back to the host


def test_the_switch_can_be_turned_between_calls(omni, ctx, files, pinhole_scene):
    """omni_pipeline_set_device_pnp between two runs: the second half of the scene with the switch on gives the edges of a run with it off throughout; then off
    again through the C entry, which the getter reports"""
    scene = pinhole_scene
    ref = through(omni, ctx, files, "pinhole", scene, False, False)
    pl = make(omni, files, "pinhole", False)
    pins = []
    try:
        half = len(scene) // 2
        assert half % MB == 0
        for s in range(0, len(scene), MB):
            kf = [scene[s + m][0] for m in range(MB)]
            p = ctx.host_alloc((2 * MB,) + kf[0].shape[1:], np.uint8)
            p[:] = np.stack([kf[m][0] for m in range(MB)] + [kf[m][1] for m in range(MB)])
            pins.append(p)
        pl.set_poses(0, np.array([pose for _, pose in scene]))
        hits = pl.run(half, 0, [p.ctypes.data for p in pins[:half // MB]], 0, None, True)
        pl.set_device_pnp(True)
        hits += pl.run(half, half, [p.ctypes.data for p in pins[half // MB:]], 0, None, True)
        on, served, back = pl.device_pnp()
        assert on and served > 0 and back == 0
        pl.set_device_pnp(False)
        assert pl.device_pnp() == (False, served, 0)
        assert hits == ref[0] and np.array_equal(np.array(pl.candidates()), ref[1]) and np.array_equal(np.array(pl.edges()), ref[2])
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


def test_init_mode_candidates_of_another_drone_are_verified_on_the_spot_with_the_same_result(omni, ctx, files, fisheye_scene):
    """KeyframePipeline::on_remote_frame: after the scene, copies of eight stored key frames arrive as key frames of drone 2.  No loop connects the two drones
    yet, so every one is an init_mode candidate (the hook is given 1 000 iterations), verified inside the detector's call through collect_geometry(): the verdicts,
    the candidates and every field of every edge are those of the pipeline with the switch off, the device served every candidate that reached the PnP stage"""
    scene, got = fisheye_scene, {}
    dirs = scene[0][0].shape[0] // 2
    for on in (False, True):
        pl = make(omni, files, "fisheye", on)
        pins = []
        try:
            for s in range(0, len(scene), MB):
                kf = [scene[s + m][0] for m in range(MB)]
                p = ctx.host_alloc((2 * dirs * MB,) + kf[0].shape[1:], np.uint8)
                p[:] = np.stack([kf[m][i] for m in range(MB) for i in range(dirs)] + [kf[m][dirs + i] for m in range(MB) for i in range(dirs)])
                pins.append(p)
            pl.set_poses(0, np.array([pose for _, pose in scene]))
            pl.run(len(scene), 0, [p.ctypes.data for p in pins], 0, None, True)
            n_self_cand, n_self_edges, served0 = len(pl.candidates()), len(pl.edges()), pl.device_pnp()[1]
            verdicts = [pl.recv_copy_as_remote(src, 2, 1000 + src) for src in range(4, 12)]
            got[on] = (verdicts, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.device_pnp(), n_self_cand, n_self_edges, served0)
        finally:
            pl.close()
            for p in pins:
                ctx.host_free(p)
    host, dev = got[False], got[True]
    print(f"remote frames: verdicts {host[0]} / {dev[0]}; candidates {host[5]} -> {len(host[1])}, edges {host[6]} -> {len(host[2])}; geometry {host[3]} / {dev[3]}; "
          f"device_pnp {host[4]} / {dev[4]} (served before the remote frames: {dev[7]})")
    assert all(old >= 0 for old, _ in host[0]) and sum(loop for _, loop in host[0]) >= 4            # not vacuous: every remote frame is a candidate, most become edges
    assert len(host[1]) == host[5] + 8 and len(host[2]) == host[6] + sum(loop for _, loop in host[0])
    assert dev[0] == host[0] and dev[3] == host[3]
    assert np.array_equal(dev[1], host[1]) and dev[2].shape == host[2].shape and np.array_equal(dev[2], host[2])
    assert set(host[2][host[6]:, 2]) | set(host[2][host[6]:, 3]) == {1.0, 2.0}                         # the new edges connect drone 2 with the self drone
    assert host[4] == (False, 0, 0)
    assert dev[4][0] is True and dev[4][2] == 0 and dev[4][1] - dev[7] >= sum(loop for _, loop in host[0])      # every remote edge went through the device
