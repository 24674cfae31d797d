"""The key-frame pipeline with a lens model (KeyframePipeline(..., camera_model=): host/camera_model.hpp, csrc/camera_plan.h), end to end.

STEREO_PINHOLE: the scene of tests/test_gpu_e2e_stereo_pinhole.py (raw 750 x 600 pairs, resized to 600 x 480 inside the unit) with every frame WARPED in numpy
so that the `mild` camera of tests/camera_cases.py is true for it: the pixel a lens with those coefficients would have recorded each ray at (the forward model
of csrc/camera_plan.h, inverted per output pixel by a long fixed-point iteration that shares nothing with the lift's eight rounds).  The pipeline with its stereo
landmarks inside the unit on the GPU against the same pipeline lifting and triangulating on the host: candidates, EVERY field of every edge and the geometry
counters identical, through run() and through push_keyframe + flush.  Condition: the host path alone finds loop edges on the warped frames.

PINHOLE_DEPTH: the scene of tests/test_gpu_e2e_depth.py warped the same way: every landmark of every message equals fill_depth_landmarks with the model's lift
(tests/cpp/camera_plan_pin.cpp `depth`, the g++ build of the host functions, on the message's own key points).

A pipeline with no model set is a pipeline with the all-zero model: the same rows, candidates and edges.  The front end runs in fp16: nothing compared here
depends on the networks' precision."""
import functools

import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import camera_cases as K
from tests import test_gpu_e2e_depth as DP
from tests import test_gpu_e2e_stereo_pinhole as SP

pytestmark = pytest.mark.gpu
MB = 4
MILD = dict(zip(("type", "k1", "k2", "p1", "p2", "xi"), K.CAMERAS["mild"][:6]))
ZERO = dict(type="PINHOLE", k1=0.0, k2=0.0, p1=0.0, p2=0.0, xi=0.0)


@functools.lru_cache(maxsize=None)
def warp_map(h, w, fx, fy, cx, cy):
    """where output pixel (u, v) of the `mild` lens looks in the ideal-pinhole picture: the ray m_u with m_u + d(m_u) = m_d(u, v), as ideal pixels (x, y)"""
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    mx_d, my_d = (u - cx) / fx, (v - cy) / fy
    mx, my = mx_d, my_d
    for _ in range(40):
        dx, dy = K._distortion(K.CAMERAS["mild"], mx, my)
        mx, my = mx_d - dx, my_d - dy
    dx, dy = K._distortion(K.CAMERAS["mild"], mx, my)
    assert max(np.abs(mx + dx - mx_d).max() * fx, np.abs(my + dy - my_d).max() * fy) < 1e-9          # converged: the forward model lands on the output pixel
    return np.clip(fx * mx + cx, 0, w - 1), np.clip(fy * my + cy, 0, h - 1)


def warp(img, fx, fy, cx, cy, nearest=False):
    """the picture the `mild` lens records of the scene whose ideal-pinhole picture is img (bilinear; nearest for a depth image)"""
    h, w = img.shape
    x, y = warp_map(h, w, fx, fy, cx, cy)
    if nearest:
        return img[np.rint(y).astype(int), np.rint(x).astype(int)]
    x0, y0 = np.minimum(np.floor(x).astype(int), w - 2), np.minimum(np.floor(y).astype(int), h - 2)
    ax, ay = x - x0, y - y0
    f = img.astype(np.float64)
    out = (f[y0, x0] * (1 - ax) + f[y0, x0 + 1] * ax) * (1 - ay) + (f[y0 + 1, x0] * (1 - ax) + f[y0 + 1, x0 + 1] * ax) * ay
    return np.rint(out).astype(img.dtype)


@pytest.fixture(scope="module")
def files(omni, tmp_path_factory):
    from omni_swarm_amd import weights
    comp, mean = synth.pca()
    return weights.write_pipeline_files(str(tmp_path_factory.mktemp("e2e_camera")), S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), omni.capi.VLAD_KINDS)


@pytest.fixture(scope="module")
def pinhole_scene():
    """[(left | right at the camera's size, warped; pose7)]: the camera-size frames have fx = 375 (300 at the networks' 0.8 scale), the coefficients are the same"""
    plan = SP.schedule()
    s = SP.SRC_W / SP.W
    k = (SP.FX * s, SP.FY * s, SP.CX * s, SP.CY * s)
    return [(np.stack([warp(f, *k) for f in pair]), np.concatenate([q[3][0], q[3][1]])) for pair, q in zip(SP.raw_frames(plan), plan)]


def make_stereo(omni, files, device_landmarks, camera_model):
    from omni_swarm_amd import pipeline
    c, P = omni.capi, SP.PARAMS
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, stereo_pinhole=SP.STEREO, device_landmarks=device_landmarks, camera_model=camera_model)
    pl.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
    return pl


def through(omni, ctx, files, scene, device_landmarks, streaming, camera_model):
    """-> (hits, candidates, edges, geometry stats, database rows)"""
    n = len(scene)
    pl = make_stereo(omni, files, device_landmarks, camera_model)
    pins = []
    try:
        if streaming:
            hits = 0
            for i, (views, pose) in enumerate(scene):
                hits += pl.push_keyframe(list(views), i, float(i), pose, False)
            hits += pl.flush()
        else:
            for s in range(0, n, MB):
                p = ctx.host_alloc((2 * MB,) + scene[0][0].shape[1:], np.uint8)
                p[:] = np.stack([scene[s + m][0][0] for m in range(MB)] + [scene[s + m][0][1] for m in range(MB)])
                pins.append(p)
            pl.set_poses(0, np.array([pose for _, pose in scene]))
            hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
        out = (hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows)
        with pytest.raises(omni.capi.OmniError, match="after the first key frame"):
            pl.set_camera_model(None)
        return out
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


@pytest.fixture(scope="module")
def host_runs(omni, ctx, files, pinhole_scene):
    """the host path with the lens, by run() and by push_keyframe: computed once"""
    return {streaming: through(omni, ctx, files, pinhole_scene, False, streaming, MILD) for streaming in (False, True)}


@pytest.mark.parametrize("streaming", [False, True], ids=["run", "push_keyframe"])
def test_device_landmarks_with_a_lens_change_nothing_downstream(omni, ctx, files, pinhole_scene, host_runs, streaming):
    host = host_runs[streaming]
    dev = through(omni, ctx, files, pinhole_scene, True, streaming, MILD)
    print(f"mild, {'push_keyframe' if streaming else 'run'}: {len(pinhole_scene)} key frames, hits {host[0]} / {dev[0]}, candidates {len(host[1])}, edges {len(host[2])} / {len(dev[2])}, "
          f"geometry (calls, edges) {host[3]} / {dev[3]}, rows {host[4]}")
    assert len(host[1]) >= 4 and len(host[2]) >= 1                              # the condition: the host path alone finds loop edges on the warped frames
    assert dev[0] == host[0] and dev[3] == host[3] and dev[4] == host[4]
    assert np.array_equal(dev[1], host[1])
    assert dev[2].shape == host[2].shape and np.array_equal(dev[2], host[2])    # every field of every edge, bit for bit


def test_the_lens_is_in_the_path_and_no_model_is_the_zero_model(omni, ctx, files, pinhole_scene, host_runs):
    """on the warped frames: no camera_model, the all-zero model and an explicit None give the same rows, candidates and edges (the ideal pinhole, as before);
    the edges found with the true lens differ from those -- the model reaches the geometry"""
    none = through(omni, ctx, files, pinhole_scene, True, False, None)
    zero = through(omni, ctx, files, pinhole_scene, True, False, ZERO)
    for a, b in zip(none, zero):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    mild = host_runs[False]
    print(f"edges with the lens {len(mild[2])}, with the ideal pinhole on the same frames {len(none[2])}")
    assert none[4] == mild[4] and not (none[2].shape == mild[2].shape and np.array_equal(none[2], mild[2]))
    pl = make_stereo(omni, files, True, None)
    try:
        got = pl.camera_model()
        assert got["type"] == "PINHOLE" and [got[k] for k in ("k1", "k2", "p1", "p2", "xi")] == [0.0] * 5 and got["intrinsics"] == [SP.FX, SP.FY, SP.CX, SP.CY]
        pl.set_camera_model(MILD, intrinsics=[301.0, 299.0, 300.5, 239.5])
        got = pl.camera_model()
        assert got["k1"] == MILD["k1"] and got["p2"] == MILD["p2"] and got["intrinsics"] == [301.0, 299.0, 300.5, 239.5]
        with pytest.raises(omni.capi.OmniError, match="xi > 0"):
            pl.set_camera_model(dict(type="MEI", xi=0.0))
        with pytest.raises(omni.capi.OmniError, match="not finite"):
            pl.set_camera_model(dict(type="PINHOLE", k1=float("nan")))
        assert pl.camera_model()["k1"] == MILD["k1"]                               # the refused calls changed nothing
    finally:
        pl.close()


def test_depth_landmarks_are_fill_depth_landmarks_with_the_models_lift(omni, ctx, files, tmp_path):
    from omni_swarm_amd import pipeline
    c, P = omni.capi, DP.PARAMS
    plan = DP.schedule()[:8]
    k = (DP.FX, DP.FY, DP.CX, DP.CY)
    frames = [(warp(g, *k), warp(d, *k, nearest=True)) for g, d in (synth.depth_keyframe(p, DP.H, DP.W, rv, sg) for (p, rv, sg, _) in plan)]
    poses = np.array([np.concatenate([q[3][0], q[3][1]]) for q in plan])
    pin = K.build_pin(tmp_path)
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], DP.W, DP.H, DP.THR, DP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"], geometry=True,
                                   pinhole_depth=dict(fx=DP.FX, fy=DP.FY, cx=DP.CX, cy=DP.CY, depth_near=DP.NEAR, depth_far=DP.FAR, accept_min_3d_pts=DP.ACCEPT_MIN),
                                   camera_model=MILD)
    try:
        for i, (gray, depth) in enumerate(frames):
            pl.push_keyframe([gray], i, float(i), poses[i], False, depth=depth)
        pl.flush()
        assert pl.db_rows == len(frames)
        total = 0
        for i, (gray, depth) in enumerate(frames):
            got = pl.frame_landmarks(i, 0)
            ref = K.run_depth(pin, omni, "mild", k, DP.NEAR, DP.FAR, DP.ACCEPT_MIN, poses[i], np.concatenate(DP.EXT), got["landmarks_2d"], depth)
            ideal = K.run_depth(pin, omni, "zero", k, DP.NEAR, DP.FAR, DP.ACCEPT_MIN, poses[i], np.concatenate(DP.EXT), got["landmarks_2d"], depth)
            n = len(got["landmarks_2d"])
            assert n > DP.ACCEPT_MIN and ref["count_3d"] == int(got["landmarks_flag"].sum()) > 0
            for key in ("norm2d", "landmarks_3d", "landmarks_flag"):
                mine = got["landmarks_2d_norm"] if key == "norm2d" else got[key]
                assert np.array_equal(np.ascontiguousarray(mine).view(np.uint8), np.ascontiguousarray(ref[key]).view(np.uint8)), (i, key)
            assert not np.array_equal(got["landmarks_3d"], ideal["landmarks_3d"])       # the lens is in the path
            total += ref["count_3d"]
        print(f"{len(frames)} PINHOLE_DEPTH key frames, {total} depth landmarks, every one the host function's with the model's lift")
    finally:
        pl.close()
