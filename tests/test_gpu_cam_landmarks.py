"""The key-frame unit with a stereo model (omni_cam_set_stereo_model / omni_cam_set_poses / omni_cam_landmarks: csrc/landmarks.hip behind the unit's up <-> down
match) against the CPU build of the same arithmetic (tests/cpp/landmark_plan_pin.cpp) fed the unit's OWN key points and match lists: bit for bit.  Networks at
128 x 96, max_num 100, a four-direction handle with room for two key frames; the down views are the up views moved up by three rows (a scene about two metres
away for a 0.1 m vertical baseline at f = 64), so the matcher finds pairs and the triangulation keeps some."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import landmark_cases as L

pytestmark = pytest.mark.gpu

W, H, DIRS, N_KF, MAX_NUM, ACCEPT_MIN = 128, 96, 4, 2, 100, 3
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")
LM_KEYS = ("norm2d", "landmarks_3d", "landmarks_flag", "count_3d")


def stereo_model(omni):
    up, down = L.rig(DIRS)
    return omni.capi.stereo_model(64.0, 64.0, 63.5, 47.5, L.THRES, ACCEPT_MIN, up, down)


def poses(seed, n):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.standard_normal((n, 4)) * rng.uniform(0.5, 2.0, (n, 1))], 1)


@pytest.fixture(scope="module")
def rig(omni, ctx, tmp_path_factory):
    """two handles on streams of their own (as in the key-frame pipeline), two different units of pinned images, the pin program"""
    from omni_swarm_amd import frontend
    c = omni.capi
    ctx_b = c.Context(0)
    comp, mean = synth.pca()
    cams = [frontend.LoopCam(x, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, c.PREC_F16,
                             n_dirs=DIRS * N_KF) for x in (ctx, ctx_b)]
    units = []
    for u in range(2):
        a = ctx.host_alloc((2 * DIRS * N_KF, H, W), np.uint8)
        up = np.stack([synth.image_u8(8200 + 16 * u + k, H, W, n_shapes=60) for k in range(DIRS * N_KF)])
        a[:] = np.concatenate([up, np.roll(up, -3, axis=1)])
        units.append(a)
    r = {"cams": cams, "units": units, "model": stereo_model(omni), "pin": L.build_pin(tmp_path_factory.mktemp("landmark_plan"))}
    yield r
    for lc in cams:
        lc.close()
    ctx_b.close()
    for a in units:
        ctx.host_free(a)


def part(unit, n):
    """the first n directions of a unit's block as a unit of its own: [up 0..n | down 0..n]"""
    return np.ascontiguousarray(np.concatenate([unit[:n], unit[DIRS * N_KF:DIRS * N_KF + n]]))


def wait(lc, with_landmarks):
    res = {k: v.copy() for k, v in lc.cam.wait().items()}
    if with_landmarks:
        res.update({k: v.copy() for k, v in lc.cam.landmarks().items()})
    return res


def pinned(rig, res, model, p7):
    """the pin program on the unit's own results"""
    n = res["n_matches"].shape[0]
    case = {"model": model, "n_pairs": n, "max_num": MAX_NUM, "poses": np.asarray(p7, np.float64).reshape(-1, 7), "kps_xy": res["kps_xy"], "n_kps": res["n_kps"],
            "match_up": res["match_up"], "match_down": res["match_down"], "n_matches": res["n_matches"]}
    (r,) = L.run_pin(rig["pin"], "plan", [case])
    return r


def test_unit_landmarks_equal_the_cpu_build_and_nothing_else_changes(omni, ctx, rig):
    lc, unit, model = rig["cams"][0], rig["units"][0], rig["model"]
    p7 = poses(1, N_KF)
    lc.cam.set_active(DIRS * N_KF)
    lc.cam.set_stereo_model(None)
    lc.cam.enqueue_host(unit, True)
    plain = wait(lc, False)
    with pytest.raises(omni.capi.OmniError, match="without a stereo model"):
        lc.cam.landmarks()
    lc.cam.set_stereo_model(model)
    lc.cam.set_poses(p7)
    lc.cam.enqueue_host(unit, True)
    got = wait(lc, True)
    ref = pinned(rig, got, model, p7)
    print("key points per image:", got["n_kps"].tolist(), "matches:", got["n_matches"].tolist(), "count_3d GPU:", got["count_3d"].tolist(), "CPU:", ref["count_3d"].tolist(),
          "ties:", int(ref["ties"][0]))
    assert [k for k in KEYS if not np.array_equal(got[k], plain[k])] == []
    assert (got["n_kps"] > ACCEPT_MIN).all() and (got["n_matches"] > 0).all() and got["count_3d"].sum() > 0          # not vacuous
    assert int(ref["ties"][0]) == 0 and L.same_bits(got, ref) == []
    lc.cam.set_stereo_model(None)


def test_partly_filled_unit_and_device_entry(omni, ctx, rig):
    """omni_cam_set_active(4): one key frame of four directions in a handle made for two; fed through omni_cam_enqueue_dev"""
    lc, model = rig["cams"][0], rig["model"]
    small = part(rig["units"][0], DIRS)
    p7 = poses(2, 1)
    lc.cam.set_stereo_model(model)
    lc.cam.set_active(DIRS)
    dev = ctx.to_device(small)
    try:
        lc.cam.set_poses(p7)
        lc.cam.enqueue_dev(dev, W, True)
        got = wait(lc, True)
    finally:
        ctx.free(dev)
        lc.cam.set_active(DIRS * N_KF)
        lc.cam.set_stereo_model(None)
    assert got["norm2d"].shape == (2 * DIRS, MAX_NUM, 2) and got["count_3d"].shape == (DIRS,) and got["count_3d"].sum() > 0
    assert L.same_bits(got, pinned(rig, got, model, p7)) == []


def test_two_units_in_flight_with_poses_of_their_own(omni, ctx, rig):
    model = rig["model"]
    p7 = [poses(3, N_KF), poses(4, N_KF)]
    for lc in rig["cams"]:
        lc.cam.set_active(DIRS * N_KF)
        lc.cam.set_stereo_model(model)
    try:
        for lc, unit, p in zip(rig["cams"], rig["units"], p7):
            lc.cam.set_poses(p)
            lc.cam.enqueue_host(unit, True)
        got = [wait(rig["cams"][1], True), wait(rig["cams"][0], True)][::-1]
    finally:
        for lc in rig["cams"]:
            lc.cam.set_stereo_model(None)
    for g, p in zip(got, p7):
        assert g["count_3d"].sum() > 0 and L.same_bits(g, pinned(rig, g, model, p)) == []
    assert not np.array_equal(got[0]["landmarks_3d"], got[1]["landmarks_3d"])


def test_refusals(omni, ctx, rig):
    """each before anything is enqueued; the handle stays usable"""
    c = omni.capi
    lc, unit, model = rig["cams"][0], rig["units"][0], rig["model"]
    mono = c.Cam(lc.sp, lc.vlad, DIRS * N_KF, V.OUT_DIM, mono=True)
    try:
        with pytest.raises(c.OmniError, match="mono"):
            mono.set_stereo_model(model)
    finally:
        mono.close()
    up, down = L.rig(DIRS)
    with pytest.raises(c.OmniError, match="do not divide"):
        lc.cam.set_stereo_model(c.stereo_model(64.0, 64.0, 63.5, 47.5, L.THRES, ACCEPT_MIN, up[:3], down[:3]))
    with pytest.raises(c.OmniError, match="without a stereo model"):
        lc.cam.set_poses(poses(5, N_KF))
    lc.cam.set_active(DIRS * N_KF)
    lc.cam.set_stereo_model(model)
    try:
        with pytest.raises(c.OmniError, match="poses are not"):
            lc.cam.enqueue_host(unit, True)
        lc.cam.set_poses(poses(5, 1))                                          # one key frame's pose for a unit of two
        with pytest.raises(c.OmniError, match="poses of 1 key frames x 4 directions for a unit of 8"):
            lc.cam.enqueue_host(unit, True)
        with pytest.raises(c.OmniError, match="poses of 1 key frames"):
            lc.cam.enqueue_dev(16, W, True)                                    # (refused before the pointer is used)
        with pytest.raises(c.OmniError, match="without a pending"):            # nothing was enqueued by any of them
            lc.cam.wait()
        lc.cam.set_poses(poses(5, N_KF))
        lc.cam.enqueue_host(unit, True)
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.set_poses(poses(6, N_KF))
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.set_stereo_model(None)
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.landmarks()
        first = wait(lc, True)
        with pytest.raises(c.OmniError, match="poses are not"):                # the poses were that unit's: the next one needs its own
            lc.cam.enqueue_host(unit, True)
        lc.cam.set_poses(poses(5, N_KF))
        lc.cam.enqueue_host(unit, True)                                        # and the handle still works
        again = wait(lc, True)
        assert L.same_bits(first, again) == [] and first["count_3d"].sum() > 0
    finally:
        lc.cam.set_stereo_model(None)
