"""The key-frame pipeline with its stereo landmarks computed inside the unit on the GPU (KeyframePipeline(..., device_landmarks=True): csrc/landmarks.hip) against
the same pipeline computing them on the host's geometry threads (device_landmarks=False: fill_stereo_landmarks), on the rendered scenes of
tests/test_gpu_e2e_scene.py (STEREO_FISHEYE, 600 x 480; eight places and their revisits) and tests/test_gpu_e2e_stereo_pinhole.py (STEREO_PINHOLE, raw 750 x 600
pairs): candidates, EVERY field of every edge and the geometry counters are identical -- the landmarks are the same bits, so everything downstream is -- both
through run() and through push_keyframe / flush.  The front end runs in fp16: what is compared does not depend on the networks' precision."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import test_gpu_e2e_scene as FE
from tests import test_gpu_e2e_stereo_pinhole as SP

pytestmark = pytest.mark.gpu
MB = 4


@pytest.fixture(scope="module")
def files(omni, tmp_path_factory):
    from omni_swarm_amd import weights
    comp, mean = synth.pca()
    return weights.write_pipeline_files(str(tmp_path_factory.mktemp("e2e_landmarks")), S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), omni.capi.VLAD_KINDS)


@pytest.fixture(scope="module")
def fisheye_scene():
    """places 0..7 of the scene's schedule and their revisits, the first visits first: [(8 views, pose7)]"""
    plan = FE.schedule()
    first = [q for q in plan[:FE.N_PLACES] if q[0] < 8]
    again = [q for q in plan[FE.N_PLACES:] if q[0] < 8]
    return [(synth.room_keyframe(p, FE.H, FE.W, rv, sg), np.concatenate([pose[0], pose[1]])) for (p, rv, sg, pose) in first + again]


@pytest.fixture(scope="module")
def pinhole_scene():
    plan = SP.schedule()
    return [(np.stack(pair), np.concatenate([q[3][0], q[3][1]])) for pair, q in zip(SP.raw_frames(plan), plan)]


def make(omni, files, scene_kind, device_landmarks):
    from omni_swarm_amd import pipeline
    c = omni.capi
    if scene_kind == "fisheye":
        P = FE.PARAMS
        return pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], FE.W, FE.H, FE.THR, FE.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                         P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                         geometry=True, device_landmarks=device_landmarks)
    P = SP.PARAMS
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, stereo_pinhole=SP.STEREO, device_landmarks=device_landmarks)
    pl.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
    return pl


def through(omni, ctx, files, scene_kind, scene, device_landmarks, streaming):
    """-> (hits, candidates, edges, geometry stats, database rows)"""
    n, dirs = len(scene), scene[0][0].shape[0] // 2
    pl = make(omni, files, scene_kind, device_landmarks)
    pins = []
    try:
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
        out = (hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows)
        with pytest.raises(omni.capi.OmniError, match="after the first key frame"):
            pl.set_device_landmarks(not device_landmarks)
        return out
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


@pytest.mark.parametrize("streaming", [False, True], ids=["run", "push_keyframe"])
@pytest.mark.parametrize("scene_kind", ["fisheye", "pinhole"])
def test_device_landmarks_change_nothing_downstream(omni, ctx, files, fisheye_scene, pinhole_scene, scene_kind, streaming):
    scene = fisheye_scene if scene_kind == "fisheye" else pinhole_scene
    assert len(scene) % MB == 0
    host = through(omni, ctx, files, scene_kind, scene, False, streaming)
    dev = through(omni, ctx, files, scene_kind, scene, True, streaming)
    print(f"{scene_kind}, {'push_keyframe' if streaming else 'run'}: {len(scene)} key frames, hits {host[0]} / {dev[0]}, candidates {len(host[1])}, edges {len(host[2])} / {len(dev[2])}, "
          f"geometry (calls, edges) {host[3]} / {dev[3]}, rows {host[4]}")
    assert len(host[1]) >= 4 and len(host[2]) >= 2                              # not vacuous: loop candidates and accepted edges (they need the landmarks)
    assert dev[0] == host[0] and dev[3] == host[3] and dev[4] == host[4]
    assert np.array_equal(dev[1], host[1])
    assert dev[2].shape == host[2].shape and np.array_equal(dev[2], host[2])    # every field of every edge, bit for bit
