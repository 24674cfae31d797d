"""The key-frame unit with a lens model (omni_cam_set_camera_model next to omni_cam_set_stereo_model: csrc/landmarks.hip lifting through csrc/camera_plan.h behind
the unit's up <-> down match) against the CPU build of the same arithmetic (tests/cpp/camera_plan_pin.cpp `plan`) fed the unit's OWN key points and match lists:
bit for bit.  The rig of tests/test_gpu_cam_landmarks.py: networks at 128 x 96, max_num 100, a four-direction handle with room for two key frames, down views =
up views moved up by three rows.  Cameras: `mild` (PINHOLE with distortion) on f = 64 and `mei` (xi 1.2) on gamma = 140, which sees about the same field."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import camera_cases as K
from tests import landmark_cases as L

pytestmark = pytest.mark.gpu

W, H, DIRS, N_KF, MAX_NUM, ACCEPT_MIN = 128, 96, 4, 2, 100, 3
LM_KEYS = ("norm2d", "landmarks_3d", "landmarks_flag", "count_3d")
FOCAL = {"mild": 64.0, "mei": 140.0}


def stereo_model(omni, name):
    up, down = L.rig(DIRS)
    return omni.capi.stereo_model(FOCAL[name], FOCAL[name], 63.5, 47.5, L.THRES, ACCEPT_MIN, up, down)


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
    r = {"cams": cams, "units": units, "pin": K.build_pin(tmp_path_factory.mktemp("camera_plan"))}
    yield r
    for lc in cams:
        lc.close()
    ctx_b.close()
    for a in units:
        ctx.host_free(a)


def wait(lc):
    res = {k: v.copy() for k, v in lc.cam.wait().items()}
    res.update({k: v.copy() for k, v in lc.cam.landmarks().items()})
    return res


def pinned(rig, res, model, camera, p7):
    """the pin program on the unit's own results"""
    n = res["n_matches"].shape[0]
    case = {"model": model, "camera": camera, "n_pairs": n, "max_num": MAX_NUM, "poses": np.asarray(p7, np.float64).reshape(-1, 7), "kps_xy": res["kps_xy"],
            "n_kps": res["n_kps"], "match_up": res["match_up"], "match_down": res["match_down"], "n_matches": res["n_matches"]}
    (r,) = K.run_pin(rig["pin"], "plan", [case])
    return r


def reset(lc):
    lc.cam.set_active(DIRS * N_KF)
    lc.cam.set_stereo_model(None)
    lc.cam.set_camera_model(None)


@pytest.mark.parametrize("name", ("mild", "mei"))
def test_whole_unit_and_partly_filled_unit(omni, ctx, rig, name):
    lc, unit = rig["cams"][0], rig["units"][0]
    model, camera = stereo_model(omni, name), K.camera(omni, name)
    try:
        lc.cam.set_stereo_model(model)
        lc.cam.set_camera_model(camera)
        p7 = poses(1, N_KF)
        lc.cam.set_poses(p7)
        lc.cam.enqueue_host(unit, True)
        got = wait(lc)
        ref = pinned(rig, got, model, camera, p7)
        ideal = pinned(rig, got, model, K.camera(omni, "zero"), p7)
        print(f"{name}: key points per image {got['n_kps'].tolist()}, matches {got['n_matches'].tolist()}, count_3d GPU {got['count_3d'].tolist()} CPU {ref['count_3d'].tolist()} "
              f"(ideal pinhole on the same arrays: {ideal['count_3d'].tolist()}), ties {int(ref['ties'][0])}")
        assert (got["n_kps"] > ACCEPT_MIN).all() and (got["n_matches"] > 0).all() and got["count_3d"].sum() > 0          # not vacuous
        assert int(ref["ties"][0]) == 0 and L.same_bits(got, ref) == []
        assert "norm2d" in L.same_bits(got, ideal)                                                                  # the lens is in the unit's path
        # omni_cam_set_active(4): one key frame of four directions in a handle made for two
        small = np.ascontiguousarray(np.concatenate([unit[:DIRS], unit[DIRS * N_KF:DIRS * N_KF + DIRS]]))
        lc.cam.set_active(DIRS)
        p7 = poses(2, 1)
        lc.cam.set_poses(p7)
        lc.cam.enqueue_host(small, True)
        part = wait(lc)
        assert part["norm2d"].shape == (2 * DIRS, MAX_NUM, 2) and part["count_3d"].shape == (DIRS,) and part["count_3d"].sum() > 0
        assert L.same_bits(part, pinned(rig, part, model, camera, p7)) == []
    finally:
        reset(lc)


@pytest.mark.parametrize("name", ("mild", "mei"))
def test_two_units_in_flight(omni, ctx, rig, name):
    model, camera = stereo_model(omni, name), K.camera(omni, name)
    p7 = [poses(3, N_KF), poses(4, N_KF)]
    try:
        for lc in rig["cams"]:
            lc.cam.set_active(DIRS * N_KF)
            lc.cam.set_stereo_model(model)
            lc.cam.set_camera_model(camera)
        for lc, unit, p in zip(rig["cams"], rig["units"], p7):
            lc.cam.set_poses(p)
            lc.cam.enqueue_host(unit, True)
        got = [wait(rig["cams"][1]), wait(rig["cams"][0])][::-1]
    finally:
        for lc in rig["cams"]:
            reset(lc)
    for g, p in zip(got, p7):
        assert g["count_3d"].sum() > 0 and L.same_bits(g, pinned(rig, g, model, camera, p)) == []
    assert not np.array_equal(got[0]["landmarks_3d"], got[1]["landmarks_3d"])


def test_the_model_survives_set_stereo_model_and_null_is_ideal(omni, ctx, rig):
    lc, unit = rig["cams"][0], rig["units"][0]
    model, camera = stereo_model(omni, "mild"), K.camera(omni, "mild")
    p7 = poses(5, N_KF)

    def run():
        lc.cam.set_poses(p7)
        lc.cam.enqueue_host(unit, True)
        return wait(lc)
    try:
        lc.cam.set_camera_model(camera)                       # before any stereo model
        lc.cam.set_stereo_model(model)
        first = run()
        lc.cam.set_stereo_model(None)                         # off and on again, with another threshold: the lens stays
        other = stereo_model(omni, "mild")
        other.triangle_thres = 2 * L.THRES
        lc.cam.set_stereo_model(other)
        second = run()
        assert L.same_bits(first, pinned(rig, first, model, camera, p7)) == []
        assert L.same_bits(second, pinned(rig, second, other, camera, p7)) == []
        assert np.array_equal(first["norm2d"], second["norm2d"])
        lc.cam.set_camera_model(None)                         # NULL: the ideal pinhole again = a handle that never had a lens
        plain = run()
        assert L.same_bits(plain, pinned(rig, plain, other, K.camera(omni, "zero"), p7)) == []
        (old,) = L.run_pin(L.build_pin(rig["pin"].rsplit("/", 1)[0]), "plan", [{"model": other, "n_pairs": DIRS * N_KF, "max_num": MAX_NUM, "poses": p7, "kps_xy": plain["kps_xy"],
                                                                               "n_kps": plain["n_kps"], "match_up": plain["match_up"], "match_down": plain["match_down"],
                                                                               "n_matches": plain["n_matches"]}])
        assert L.same_bits(plain, old) == []                  # ... the earlier pin program, which knows no camera
    finally:
        reset(lc)


def test_refusals(omni, ctx, rig):
    """each before anything is enqueued; the handle stays usable"""
    c = omni.capi
    lc, unit = rig["cams"][0], rig["units"][0]
    model, camera = stereo_model(omni, "mild"), K.camera(omni, "mild")
    mono = c.Cam(lc.sp, lc.vlad, DIRS * N_KF, V.OUT_DIM, mono=True)
    try:
        with pytest.raises(c.OmniError, match="mono"):
            mono.set_camera_model(camera)
    finally:
        mono.close()
    for bad, what in ((c.camera_model(7), "unknown type"), (c.camera_model("MEI", xi=0.0), "xi > 0"), (c.camera_model("PINHOLE", k1=float("inf")), "not finite")):
        with pytest.raises(c.OmniError, match=what):
            lc.cam.set_camera_model(bad)
    try:
        lc.cam.set_stereo_model(model)
        lc.cam.set_camera_model(camera)
        lc.cam.set_poses(poses(6, N_KF))
        lc.cam.enqueue_host(unit, True)
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.set_camera_model(None)
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.set_camera_model(K.camera(omni, "mei"))
        first = wait(lc)
        assert L.same_bits(first, pinned(rig, first, model, camera, poses(6, N_KF))) == []      # the refused calls changed nothing
    finally:
        reset(lc)
