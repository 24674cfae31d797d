"""The key-frame unit fed RAW stereo-pinhole pairs (omni_cam_enqueue_raw_host / _dev: the resize kernel inside the unit) against the existing path -- the numpy
restatement of the resize (tests/resize_ref.py), [resized left | resized right], omni_cam_enqueue_host with fisheye_mask = 0.  Networks at 128 x 96, raw frames
188 x 120, 3 key frames in a unit created for 4 (one direction: the unit's size counts key frames).  Both paths run the same network kernels on the same bytes:
every comparison is exact."""
import contextlib

import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import resize_ref as R

pytestmark = pytest.mark.gpu

SRC_W, SRC_H, W, H, N_KF, N_KF_CAP, MAX_NUM = 188, 120, 128, 96, 3, 4, 100
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")


@pytest.fixture(scope="module")
def rig(omni, ctx):
    c = omni.capi
    r = {"rs": c.Resize(ctx, SRC_W, SRC_H, W, H), "raw": []}
    for cam in range(2):                                                      # pinned: the source of the unit's asynchronous uploads
        a = ctx.host_alloc((N_KF + 1, SRC_H, SRC_W), np.uint8)                # (the fourth pair: a second unit for the in-flight test)
        # the right camera sees the left camera's scene a few columns over: the up / down matcher has pairs to find
        a[:] = np.stack([np.roll(synth.image_u8(7100 + k, SRC_H, SRC_W, n_shapes=80), -3 * cam, axis=1) for k in range(N_KF + 1)])
        r["raw"].append(a)
    small = [R.resize(a, W, H) for a in r["raw"]]                             # computed once, never written again
    r["resized"] = lambda kfs: np.stack([small[cam][k] for cam in range(2) for k in kfs])
    r["weights"] = (S.synth_weights(0), synth.pca(), V.synth_weights())
    yield r
    r["rs"].close()
    for a in r["raw"]:
        ctx.host_free(a)


@contextlib.contextmanager
def make_cam(omni, ctx, rig, prec, active=N_KF):
    """a unit created for 4 key frames with 3 active; closed whatever the test does"""
    from omni_swarm_amd import frontend
    sp_w, (comp, mean), vw = rig["weights"]
    lc = frontend.LoopCam(ctx, sp_w, comp, mean, vw, V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, prec, n_dirs=N_KF_CAP, fisheye=False)
    try:
        lc.cam.set_active(active)
        yield lc
    finally:
        lc.close()


def wait(lc):
    return {k: v.copy() for k, v in lc.cam.wait().items()}


def same(a, b):
    return [k for k in KEYS if not np.array_equal(a[k], b[k])]


def test_unit_input_bytes_equal_the_restatement(omni, ctx, rig):
    """(a) omni_cam_get_input after a raw unit: [resized left kf 0..2 | resized right kf 0..2], no row blanked."""
    c = omni.capi
    ref = rig["resized"](range(N_KF))
    with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
        lc.cam.enqueue_raw_host(rig["rs"], rig["raw"][0][:N_KF], rig["raw"][1][:N_KF])
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.get_input()
        lc.cam.wait()
        got = lc.cam.get_input()
    diff = int((got != ref).sum())
    print(f"{diff} of {ref.size} bytes of the unit's input block differ from the restatement")
    assert got.shape == ref.shape == (2 * N_KF, H, W) and ref[:, H * 3 // 4:].std() > 5
    assert diff == 0


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT"])
def test_results_equal_the_unit_fed_resized_images(omni, ctx, rig, prec):
    """(b) every field of omni_cam_result, bit for bit"""
    c = omni.capi
    small = ctx.host_alloc((2 * N_KF, H, W), np.uint8)
    small[:] = rig["resized"](range(N_KF))
    try:
        with make_cam(omni, ctx, rig, getattr(c, prec)) as lc:
            lc.cam.enqueue_host(small, False)
            ref = wait(lc)
            lc.cam.enqueue_raw_host(rig["rs"], rig["raw"][0][:N_KF], rig["raw"][1][:N_KF])
            got = wait(lc)
    finally:
        ctx.host_free(small)
    print(prec, "key points per left image:", ref["n_kps"][:N_KF].tolist(), "right:", ref["n_kps"][N_KF:].tolist(), "matches:", ref["n_matches"].tolist())
    assert ref["n_kps"].shape == (2 * N_KF,) and ref["global_desc"].shape == (N_KF, V.OUT_DIM)
    assert (ref["n_kps"] >= 20).all() and (ref["n_matches"] > 0).all()                          # not vacuous
    assert same(got, ref) == []


def test_host_entry_equals_device_entry_and_two_units_in_flight(omni, ctx, rig):
    """(c), and the parts form and the frontend's blocking call"""
    c = omni.capi
    rs = rig["rs"]
    units = [[a[:N_KF] for a in rig["raw"]], [a[1:N_KF + 1] for a in rig["raw"]]]                # two different units of three key frames
    ctx_b = c.Context(0)                                                                        # the second handle on streams of its own, as in the key-frame pipeline
    try:
        with make_cam(omni, ctx, rig, c.PREC_F16) as a, make_cam(omni, ctx_b, rig, c.PREC_F16) as b:
            one_by_one = []
            for lc, (left, right) in zip((a, b), units):
                lc.cam.enqueue_raw_host(rs, left, right)
                one_by_one.append(wait(lc))
            assert same(one_by_one[0], one_by_one[1]) != []                                     # different key frames, different results
            # raw frames already in HBM, rows at a pitch of their own
            pitch = SRC_W + 4
            padded = [np.zeros((N_KF, SRC_H, pitch), np.uint8) for _ in range(2)]
            for p, u in zip(padded, units[0]):
                p[:, :, :SRC_W] = u
            left_dev, right_dev = ctx.to_device(padded[0]), ctx.to_device(padded[1])
            try:
                a.cam.enqueue_raw_dev(rs, left_dev, right_dev, pitch, N_KF)
                assert same(wait(a), one_by_one[0]) == []
                assert np.array_equal(a.cam.get_input(), rig["resized"](range(N_KF)))
            finally:
                ctx.free(left_dev); ctx.free(right_dev)
            # both units enqueued before either is waited for
            for lc, (left, right) in zip((a, b), units):
                lc.cam.enqueue_raw_host(rs, left, right)
            together = [wait(b), wait(a)][::-1]
            assert same(together[0], one_by_one[0]) == [] and same(together[1], one_by_one[1]) == []
            # the unit's frames as segments of host memory: 1 + 2 left, 2 + 1 right
            (left, right) = units[1]
            b.cam.enqueue_raw_host_parts(rs, [left[:1], left[1:]], [right[:2], right[2:]])
            assert same(wait(b), one_by_one[1]) == []
            # the blocking call of the Python frontend: one raw pair = one key frame
            a.cam.set_active(1)
            kf = a.on_stereo_images(rig["raw"][0][0], rig["raw"][1][0], rs)
            v = rig["resized"]([0])
            ref = a.on_flattened_images(v[:1], v[1:])
            assert len(kf["images"]) == 1 and kf["landmark_num"] == ref["landmark_num"] > 0
            for x, y in zip(kf["images"], ref["images"]):
                assert all(np.array_equal(x[k], y[k]) for k in x)
    finally:
        ctx_b.close()


def test_a_resize_object_of_equal_sizes_is_the_host_entry(omni, ctx, rig):
    """(d) source = destination: the copy mode feeds the networks the frames themselves"""
    c = omni.capi
    frames = ctx.host_alloc((2 * N_KF, H, W), np.uint8)
    frames[:] = rig["resized"](range(N_KF))[::-1]
    rs = c.Resize(ctx, W, H, W, H)
    try:
        assert rs.mode == c.RESIZE_COPY
        with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
            lc.cam.enqueue_host(frames, False)
            ref = wait(lc)
            lc.cam.enqueue_raw_host(rs, frames[:N_KF], frames[N_KF:])
            got = wait(lc)
            assert np.array_equal(lc.cam.get_input(), frames)
        assert (ref["n_kps"] >= 20).all() and same(got, ref) == []
    finally:
        rs.close()
        ctx.host_free(frames)


def test_refusals(omni, ctx, rig):
    """(e) each refused before the device is touched; the handle stays usable"""
    c = omni.capi
    rs = rig["rs"]
    left, right = (a[:N_KF] for a in rig["raw"])
    with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
        with pytest.raises(c.OmniError, match="2 key frames for a unit of 3"):
            lc.cam.enqueue_raw_host(rs, left[:2], right[:2])
        with pytest.raises(c.OmniError, match="stride"):
            lc.cam.enqueue_raw_dev(rs, 16, 16, SRC_W - 1, N_KF)                             # (refused before the pointers are used)
        other = c.Resize(ctx, SRC_W, SRC_H, 96, 64)
        mono = c.Cam(lc.sp, lc.vlad, N_KF, V.OUT_DIM, mono=True)
        try:
            with pytest.raises(c.OmniError, match="96x64 images but the networks were created for 128x96"):
                lc.cam.enqueue_raw_host(other, left, right)
            with pytest.raises(c.OmniError, match="mono"):
                mono.enqueue_raw_host(rs, left, right)
        finally:
            mono.close(); other.close()
        with pytest.raises(c.OmniError, match="without a pending"):                         # nothing was enqueued by any of them
            lc.cam.wait()
        lc.cam.enqueue_raw_host(rs, left, right)
        with pytest.raises(c.OmniError, match="in flight"):                                 # a second unit on a busy handle
            lc.cam.enqueue_raw_host(rs, left, right)
        first = wait(lc)
        lc.cam.enqueue_raw_host(rs, left, right)                                            # and the handle still works
        assert same(wait(lc), first) == [] and (first["n_kps"] >= 20).all()
    import torch
    if torch.cuda.device_count() > 1:                                                       # tables on another device (needs a second GPU to exist)
        ctx_1 = c.Context(1)
        far = c.Resize(ctx_1, SRC_W, SRC_H, W, H)
        try:
            with make_cam(omni, ctx, rig, c.PREC_F16) as lc, pytest.raises(c.OmniError, match="device"):
                lc.cam.enqueue_raw_host(far, left, right)
        finally:
            far.close(); ctx_1.close()
