"""A MONO key-frame unit with a depth model (omni_cam_set_depth_model / omni_cam_set_poses / omni_cam_set_depth_host / _dev / omni_cam_landmarks:
csrc/depth_landmarks.hip behind the unit's key points) against the host path (omni_depth_landmarks_host, which tests/test_depth_capi_cpu.py holds to
fill_image_descriptor + fill_depth_landmarks) fed the unit's OWN key points: bit for bit.  Networks at 128 x 96, max_num 100, a handle of 2 images, a distorted
PINHOLE lens; the depth images have the networks' size."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import camera_cases as CC
from tests import depth_cases as D

pytestmark = pytest.mark.gpu

W, H, N, MAX_NUM, ACCEPT_MIN = 128, 96, 2, 100, 3
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")
LENS = "mild"


def poses(seed, n):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.standard_normal((n, 4)) * rng.uniform(0.5, 2.0, (n, 1))], 1)


def depth_frames(seed, n=N, stride=W):
    rng = np.random.default_rng(seed)
    d = rng.integers(200, 12000, (n, H, stride)).astype(np.uint16)
    d[:, ::7, ::5] = np.array(D.DEPTH_VALUES + (5000,), np.uint16)[rng.integers(0, 8, d[:, ::7, ::5].shape)]
    return d


@pytest.fixture(scope="module")
def rig(omni, ctx):
    c = omni.capi
    comp, mean = synth.pca()
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, S.synth_weights(0), comp, mean, W, H, 0.015, MAX_NUM, c.PREC_F16, N)
    vlad = c.MobileNetVLAD(vctx, V.synth_weights(), V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, W, H, N)
    cam = c.Cam(sp, vlad, N, V.OUT_DIM, mono=True)
    unit = ctx.host_alloc((N, H, W), np.uint8)
    unit[:] = np.stack([synth.image_u8(8300 + k, H, W, n_shapes=60) for k in range(N)])
    ext = np.array([0.05, -0.02, 0.1, 0.5, -0.5, 0.5, -0.5]) * 1.3                     # un-normalised
    model = c.depth_model(64.0, 64.0, 63.5, 47.5, D.NEAR, D.FAR, ACCEPT_MIN, W, H, ext)
    r = {"cam": cam, "sp": sp, "vlad": vlad, "unit": unit, "model": model, "camera": CC.camera(omni, LENS)}
    yield r
    cam.close()
    sp.close()
    vlad.close()
    vctx.close()
    ctx.host_free(unit)


def wait(cam, with_landmarks):
    res = {k: v.copy() for k, v in cam.wait().items()}
    if with_landmarks:
        res.update({k: v.copy() for k, v in cam.landmarks().items()})
    return res


def host_path(omni, rig, res, p7, depth, have=None, stride=0):
    """the host path on the unit's own key points"""
    return omni.capi.depth_landmarks_host(rig["model"], p7, res["kps_xy"], res["n_kps"], depth, have=have, camera=rig["camera"], depth_stride=stride)


def run_unit(rig, p7, set_depth, enqueue=None):
    cam = rig["cam"]
    cam.set_poses(p7)
    set_depth(cam)
    (enqueue or (lambda: cam.enqueue_host(rig["unit"], False)))()
    return wait(cam, True)


def test_unit_landmarks_equal_the_host_path_and_nothing_else_changes(omni, ctx, rig):
    cam, unit = rig["cam"], rig["unit"]
    p7, depth = poses(1, N), depth_frames(1)
    cam.set_depth_model(None)
    cam.enqueue_host(unit, False)
    plain = wait(cam, False)
    with pytest.raises(omni.capi.OmniError, match="without a stereo model"):      # a mono handle without a depth model: the error it was
        cam.landmarks()
    cam.set_depth_model(rig["model"], rig["camera"])
    try:
        got = run_unit(rig, p7, lambda cm: cm.set_depth_host(list(depth)))
        ref = host_path(omni, rig, got, p7, depth)
        print("key points per image:", got["n_kps"].tolist(), "count_3d GPU:", got["count_3d"].tolist(), "host:", ref["count_3d"].tolist())
        assert [k for k in KEYS if not np.array_equal(got[k], plain[k])] == []     # every field of omni_cam_result, bit for bit
        assert got["norm2d"].shape == (N, MAX_NUM, 2) and got["count_3d"].shape == (N,)      # n_images == n_dirs, count_3d per image
        assert (got["n_kps"] > ACCEPT_MIN).all() and (got["count_3d"] > 5).all()             # not vacuous
        assert D.same_bits(got, ref) == []
        # a NULL depth frame: zeros for that image (its lifted key points are still there), the other image as before
        nul = run_unit(rig, p7, lambda cm: cm.set_depth_host([depth[0], None]))
        assert D.same_bits(nul, host_path(omni, rig, nul, p7, depth, have=[1, 0])) == []
        assert nul["count_3d"].tolist() == [int(got["count_3d"][0]), 0] and not nul["landmarks_3d"][1].any() and not nul["landmarks_flag"][1].any()
        assert np.array_equal(nul["norm2d"], got["norm2d"]) and nul["norm2d"][1].any()
    finally:
        cam.set_depth_model(None)


def test_depth_in_hbm_a_wider_stride_and_a_smaller_unit(omni, ctx, rig):
    """set_depth_dev gives what set_depth_host gives, also with a stride above the width on both; omni_cam_set_active(1): one image in a handle made for two"""
    cam = rig["cam"]
    p7, wide = poses(2, N), depth_frames(2, stride=W + 8)
    packed = np.ascontiguousarray(wide[:, :, :W])
    cam.set_depth_model(rig["model"], rig["camera"])
    dev = ctx.to_device(wide)
    small = ctx.to_device(np.ascontiguousarray(rig["unit"][:1]))
    try:
        a = run_unit(rig, p7, lambda cm: cm.set_depth_host(list(packed)))
        b = run_unit(rig, p7, lambda cm: cm.set_depth_host(list(wide), W + 8))
        d = run_unit(rig, p7, lambda cm: cm.set_depth_dev(dev, W + 8, N))
        e = run_unit(rig, p7, lambda cm: cm.set_depth_dev(dev, W + 8, N, have=[0, 1]))
        assert a["count_3d"].sum() > 10 and D.same_bits(a, host_path(omni, rig, a, p7, packed)) == []
        assert D.same_bits(b, a) == [] and D.same_bits(d, a) == []
        assert D.same_bits(e, host_path(omni, rig, e, p7, wide, have=[0, 1], stride=W + 8)) == [] and e["count_3d"][0] == 0 and e["count_3d"][1] == a["count_3d"][1]
        cam.set_active(1)
        one = run_unit(rig, p7[:1], lambda cm: cm.set_depth_host([packed[0]]), lambda: cam.enqueue_dev(small, W, False))
        assert one["norm2d"].shape == (1, MAX_NUM, 2) and one["count_3d"].shape == (1,)
        assert D.same_bits(one, {k: a[k][:1] for k in ("norm2d", "landmarks_3d", "landmarks_flag", "count_3d")}) == []
    finally:
        ctx.free(dev)
        ctx.free(small)
        cam.set_active(N)
        cam.set_depth_model(None)


def test_jpeg_and_parts_entries_give_what_the_host_entry_gives(omni, ctx, rig):
    """the unit's frames as JPEG files (omni_cam_enqueue_jpeg_host, right_files = NULL) and as parts (omni_cam_enqueue_host_parts) against omni_cam_enqueue_host
    on the same pixels"""
    c = omni.capi
    cam = rig["cam"]
    files = [c.jpeg_encode_host(np.ascontiguousarray(g), 85)[1] for g in rig["unit"]]
    pixels = ctx.host_alloc((N, H, W), np.uint8)
    pixels[:] = np.stack([c.jpeg_decode_host(f)[1] for f in files])
    p7, depth = poses(3, N), depth_frames(3)
    cam.set_depth_model(rig["model"], rig["camera"])
    try:
        sd = lambda cm: cm.set_depth_host(list(depth))
        ref = run_unit(rig, p7, sd, lambda: cam.enqueue_host(pixels, False))
        got = run_unit(rig, p7, sd, lambda: cam.enqueue_jpeg_host(None, files))
        assert ref["count_3d"].sum() > 10 and D.same_bits(ref, host_path(omni, rig, ref, p7, depth)) == []
        assert [k for k in KEYS if not np.array_equal(got[k], ref[k])] == [] and D.same_bits(got, ref) == []
        lib = c.lib()
        import ctypes
        cam.set_poses(p7)
        sd(cam)
        ups = (ctypes.c_void_p * 2)(pixels[0].ctypes.data, pixels[1].ctypes.data)
        cnt = (ctypes.c_int * 2)(1, 1)
        assert lib.omni_cam_enqueue_host_parts(cam.h, ups, cnt, 2, None, None, 0, W, H, 0) == 0, lib.omni_last_error()
        parts = wait(cam, True)
        assert D.same_bits(parts, ref) == []
    finally:
        ctx.host_free(pixels)
        cam.set_depth_model(None)


def test_frontend_loopcam_with_a_depth_model(omni, ctx, rig):
    """frontend.LoopCam(depth_model=): a mono unit whose fetch() carries the lifted key points and the depth landmarks of every image"""
    from omni_swarm_amd import frontend
    c = omni.capi
    comp, mean = synth.pca()
    with pytest.raises(ValueError, match="two camera configurations"):
        frontend.LoopCam(ctx, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, c.PREC_F16, n_dirs=N,
                         depth_model=rig["model"], stereo_model=c.StereoModel())
    lc = frontend.LoopCam(ctx, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, c.PREC_F16, n_dirs=N,
                          depth_model=rig["model"], camera_model=rig["camera"])
    p7, depth = poses(7, N), depth_frames(7)
    try:
        lc.set_poses(p7)
        lc.set_depth([depth[0], depth[1]])
        lc.enqueue_host(rig["unit"])
        kf = lc.fetch()
    finally:
        lc.close()
    rig["cam"].set_depth_model(rig["model"], rig["camera"])                   # the same unit through the C-ABI wrapper, which the tests above hold to the host path
    try:
        ref = run_unit(rig, p7, lambda cm: cm.set_depth_host(list(depth)))
    finally:
        rig["cam"].set_depth_model(None)
    assert len(kf["images"]) == N and kf["landmark_num"] == int(ref["n_kps"].sum())
    for d, im in enumerate(kf["images"]):
        n = im["landmark_num"]
        assert n == ref["n_kps"][d] and im["count_3d"] == ref["count_3d"][d] > 5 and "landmarks_2d_down" not in im
        for key, arr in (("landmarks_2d", ref["kps_xy"]), ("landmarks_2d_norm", ref["norm2d"]), ("landmarks_3d", ref["landmarks_3d"]), ("landmarks_flag", ref["landmarks_flag"])):
            assert np.array_equal(im[key].view(np.uint8), np.ascontiguousarray(arr[d, :n]).view(np.uint8)), (d, key)


def test_refusals(omni, ctx, rig):
    """each before anything is enqueued; the handle stays usable"""
    c = omni.capi
    cam, unit, model = rig["cam"], rig["unit"], rig["model"]
    depth = depth_frames(4)
    # a stereo handle takes no depth model; a mono handle still takes neither a stereo model nor set_camera_model, with the messages it had
    sp2 = c.SuperPoint(ctx, S.synth_weights(0), *synth.pca(), W, H, 0.015, MAX_NUM, c.PREC_F16, 2)
    stereo = c.Cam(sp2, rig["vlad"], 1, V.OUT_DIM)
    try:
        with pytest.raises(c.OmniError, match="stereo handle"):
            stereo.set_depth_model(model)
        with pytest.raises(c.OmniError, match="stereo handle"):
            stereo.set_depth_model(None)
    finally:
        stereo.close()
        sp2.close()
    from tests import landmark_cases as L
    up, down = L.rig(1)
    with pytest.raises(c.OmniError, match="a mono handle has no up / down camera pair to triangulate from"):
        cam.set_stereo_model(c.stereo_model(64.0, 64.0, 63.5, 47.5, L.THRES, ACCEPT_MIN, up, down))
    with pytest.raises(c.OmniError, match="a mono handle runs no stereo-landmark stage to lift in"):
        cam.set_camera_model(rig["camera"])
    cam.set_depth_model(None)
    with pytest.raises(c.OmniError, match="without a stereo model"):
        cam.set_poses(poses(5, N))
    with pytest.raises(c.OmniError, match="without a depth model"):
        cam.set_depth_host(list(depth))
    with pytest.raises(c.OmniError, match="without a depth model"):
        cam.set_depth_dev(16, W, N)
    bad = type(model).from_buffer_copy(model)
    bad.depth_width = 0
    with pytest.raises(c.OmniError, match="depth_width"):
        cam.set_depth_model(bad)
    with pytest.raises(c.OmniError, match="MEI needs xi"):
        cam.set_depth_model(model, c.CameraModel(type=c.CAMERA_MEI, xi=0.0))
    cam.set_active(N)
    cam.set_depth_model(model, rig["camera"])
    try:
        with pytest.raises(c.OmniError, match="stride"):
            cam.set_depth_host(list(depth), W - 1)
        with pytest.raises(c.OmniError, match="images, the handle holds"):
            cam.set_depth_host(list(depth) + [None])
        with pytest.raises(c.OmniError, match="poses are not"):
            cam.enqueue_host(unit, False)
        cam.set_poses(poses(5, N))
        with pytest.raises(c.OmniError, match="depth frames are not"):
            cam.enqueue_host(unit, False)
        cam.set_depth_host([depth[0]])                                         # one image's frame for a unit of two
        with pytest.raises(c.OmniError, match="depth frames of 1 images for a unit of 2"):
            cam.enqueue_host(unit, False)
        with pytest.raises(c.OmniError, match="depth frames of 1 images"):
            cam.enqueue_dev(16, W, False)                                      # (refused before the pointer is used)
        with pytest.raises(c.OmniError, match="depth frames of 1 images"):
            cam.enqueue_jpeg_host(None, [b"\xff\xd8", b"\xff\xd8"])            # (... before the files are read)
        cam.set_depth_host(list(depth))
        cam.set_poses(poses(5, 1))                                             # one key frame's pose for a unit of two
        with pytest.raises(c.OmniError, match="poses of 1 key frames for a unit of 2"):
            cam.enqueue_host(unit, False)
        with pytest.raises(c.OmniError, match="without a pending"):            # nothing was enqueued by any of them
            cam.wait()
        cam.set_poses(poses(5, N))
        cam.enqueue_host(unit, False)
        for call in (lambda: cam.set_poses(poses(6, N)), lambda: cam.set_depth_host(list(depth)), lambda: cam.set_depth_dev(16, W, N), lambda: cam.set_depth_model(None),
                     lambda: cam.set_depth_model(model), lambda: cam.landmarks()):
            with pytest.raises(c.OmniError, match="in flight"):
                call()
        first = wait(cam, True)
        with pytest.raises(c.OmniError, match="poses are not"):                # the poses and the frames were that unit's: the next one needs its own
            cam.enqueue_host(unit, False)
        cam.set_poses(poses(5, N))
        with pytest.raises(c.OmniError, match="depth frames are not"):
            cam.enqueue_host(unit, False)
        cam.set_depth_host(list(depth))
        cam.enqueue_host(unit, False)                                          # and the handle still works
        again = wait(cam, True)
        assert D.same_bits(first, again) == [] and first["count_3d"].sum() > 0
    finally:
        cam.set_depth_model(None)
