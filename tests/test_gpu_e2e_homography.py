"""The key-frame pipeline with the homography RANSAC of its loop candidates on the GPU (KeyframePipeline(..., device_homography=True): the fused matcher entry,
csrc/homography.hip) against the same pipeline running geom::find_homography_ransac on the host's geometry threads (device_homography=False), on the rendered scenes
of tests/test_gpu_e2e_landmarks.py (STEREO_FISHEYE, 600 x 480, eight places and their revisits; STEREO_PINHOLE, raw 750 x 600 pairs): candidates, EVERY field of
every edge and the geometry counters are identical -- the masks are the same, so everything downstream is -- both through run() and through push_keyframe / flush;
no direction pair is handed back to the host.  The candidates that are rejected are the pairs that run all 2 000 iterations."""
import numpy as np
import pytest

from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_scene as FE
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests.test_gpu_e2e_landmarks import files, fisheye_scene, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the two scenes)

pytestmark = pytest.mark.gpu
MB = LM.MB


def make(omni, files, scene_kind, device_homography):
    from omni_swarm_amd import pipeline
    c = omni.capi
    E, extra = (FE, {}) if scene_kind == "fisheye" else (SP, {"stereo_pinhole": SP.STEREO})
    P = E.PARAMS
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], E.W, E.H, E.THR, E.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, device_homography=device_homography, **extra)
    if scene_kind != "fisheye":
        pl.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
    return pl


def through(omni, ctx, files, scene_kind, scene, device_homography, streaming):
    """-> (hits, candidates, edges, geometry stats, database rows, (switch, pairs from the device, pairs handed back))"""
    n, dirs = len(scene), scene[0][0].shape[0] // 2
    pl = make(omni, files, scene_kind, device_homography)
    pins = []
    try:
        assert pl.device_homography() == (device_homography, 0, 0)
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
        return hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows, pl.device_homography()
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


@pytest.mark.parametrize("streaming", [False, True], ids=["run", "push_keyframe"])
@pytest.mark.parametrize("scene_kind", ["fisheye", "pinhole"])
def test_device_homography_changes_nothing_downstream(omni, ctx, files, fisheye_scene, pinhole_scene, scene_kind, streaming):
    scene = fisheye_scene if scene_kind == "fisheye" else pinhole_scene
    assert len(scene) % MB == 0
    host = through(omni, ctx, files, scene_kind, scene, False, streaming)
    dev = through(omni, ctx, files, scene_kind, scene, True, streaming)
    print(f"{scene_kind}, {'push_keyframe' if streaming else 'run'}: {len(scene)} key frames, hits {host[0]} / {dev[0]}, candidates {len(host[1])}, edges {len(host[2])} / {len(dev[2])}, "
          f"geometry (calls, edges) {host[3]} / {dev[3]}, rows {host[4]}; direction pairs served by the device {dev[5][1]}, handed back to the host {dev[5][2]}")
    assert len(host[1]) >= 4 and len(host[2]) >= 2 and len(host[1]) > len(host[2])      # not vacuous: accepted edges AND rejected candidates (the 2 000-iteration case)
    assert dev[0] == host[0] and dev[3] == host[3] and dev[4] == host[4]
    assert np.array_equal(dev[1], host[1])
    assert dev[2].shape == host[2].shape and np.array_equal(dev[2], host[2])            # every field of every edge, bit for bit
    assert host[5] == (False, 0, 0)
    assert dev[5][0] is True and dev[5][1] >= len(host[2]) and dev[5][2] == 0           # no pair fell back to the host


def test_the_switch_can_be_turned_between_calls(omni, ctx, files, pinhole_scene):
    """omni_pipeline_set_device_homography between two runs: the second half of the scene with the switch on gives the edges of a run with it off throughout"""
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
        pl.set_device_homography(True)
        hits += pl.run(half, half, [p.ctypes.data for p in pins[half // MB:]], 0, None, True)
        on, served, back = pl.device_homography()
        assert on and served > 0 and back == 0
        assert hits == ref[0] and np.array_equal(np.array(pl.candidates()), ref[1]) and np.array_equal(np.array(pl.edges()), ref[2])
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)
