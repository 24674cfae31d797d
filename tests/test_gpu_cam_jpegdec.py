"""The key-frame unit fed JPEG FILES (omni_cam_enqueue_jpeg_host: the decode kernels of csrc/jpeg_dec.hip inside the unit, on its SuperPoint stream, in front of the
resize) against the same unit fed the host-decoded pixels of the same files (omni_jpeg_decode_host, the g++ build of csrc/jpeg_dec_plan.h) through the existing
entries: omni_cam_get_input and EVERY field of omni_cam_result bit-identical.  Frames 160 x 120 -> networks at 128 x 96, encoded at test time with the project's
own omni_jpeg_encode_host: a stereo handle created for 4 key frames with 3 active (omni_cam_enqueue_raw_host is the other side), a mono handle with and without a
resize (omni_cam_enqueue_host is the other side); a frame above the decoder's capacity (decoded on the calling thread), a truncated frame (all zeros, no key
points), the refusals."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import resize_ref as R

pytestmark = pytest.mark.gpu

SRC_W, SRC_H, W, H, N_KF, N_KF_CAP, MAX_NUM = 160, 120, 128, 96, 3, 4, 100
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")


@pytest.fixture(scope="module")
def rig(omni, ctx):
    """files and their host-decoded pixels (pinned: the source of the other side's uploads); computed once"""
    c = omni.capi
    r = {"rs": c.Resize(ctx, SRC_W, SRC_H, W, H), "files": [], "raw": [], "weights": (S.synth_weights(0), synth.pca(), V.synth_weights())}
    for cam in range(2):
        frames = [np.roll(synth.image_u8(8100 + k, SRC_H, SRC_W, n_shapes=80), -3 * cam, axis=1) for k in range(N_KF)]
        files = []
        for k, g in enumerate(frames):
            st, data = c.jpeg_encode_host(np.ascontiguousarray(g), (75, 90, 60)[k])
            assert st == c.JPEG_OK and len(data) <= SRC_W * SRC_H // 2
            files.append(data)
        a = ctx.host_alloc((N_KF, SRC_H, SRC_W), np.uint8)
        for k, f in enumerate(files):
            st, pix = c.jpeg_decode_host(f)
            assert st == c.JPEGDEC_OK
            a[k] = pix
        r["files"].append(files)
        r["raw"].append(a)
    small = [synth.image_u8(8200 + k, H, W, n_shapes=60) for k in range(N_KF)]                 # network-size pictures for the mono handle without a resize
    r["small_files"] = [c.jpeg_encode_host(g, 80)[1] for g in small]
    r["small"] = ctx.host_alloc((N_KF, H, W), np.uint8)
    r["small"][:] = np.stack([c.jpeg_decode_host(f)[1] for f in r["small_files"]])
    yield r
    r["rs"].close()
    for a in r["raw"] + [r["small"]]:
        ctx.host_free(a)


def stereo_cam(omni, ctx, rig, prec):
    from omni_swarm_amd import frontend
    sp_w, (comp, mean), vw = rig["weights"]
    lc = frontend.LoopCam(ctx, sp_w, comp, mean, vw, V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, prec, n_dirs=N_KF_CAP, fisheye=False)
    lc.cam.set_active(N_KF)
    return lc


def wait(cam):
    return {k: v.copy() for k, v in cam.wait().items()}


def moved(a, b):
    return [k for k in KEYS if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT"])
def test_stereo_unit_equals_the_unit_fed_the_host_decoded_frames(omni, ctx, rig, prec):
    c = omni.capi
    lc = stereo_cam(omni, ctx, rig, getattr(c, prec))
    try:
        cam = lc.cam
        cam.enqueue_raw_host(rig["rs"], rig["raw"][0], rig["raw"][1])
        ref, ref_in = wait(cam), cam.get_input()
        cam.enqueue_jpeg_host(rig["rs"], rig["files"][0], rig["files"][1])
        with pytest.raises(c.OmniError, match="in flight"):
            cam.jpegdec_status()
        got, got_in, status = wait(cam), cam.get_input(), cam.jpegdec_status()
    finally:
        lc.close()
    diff = int((got_in != ref_in).sum())
    print(f"{prec}: input block {diff} of {ref_in.size} bytes differ; fields with other bits: {moved(got, ref)}; key points {ref['n_kps'].tolist()}, matches {ref['n_matches'].tolist()}")
    assert status == [c.JPEGDEC_OK] * (2 * N_KF)
    assert got_in.shape == ref_in.shape == (2 * N_KF, H, W) and diff == 0
    assert np.array_equal(ref_in, np.concatenate([R.resize(rig["raw"][0], W, H), R.resize(rig["raw"][1], W, H)]))
    assert (ref["n_kps"] >= 20).all() and (ref["n_matches"] > 0).all()                           # not vacuous
    assert moved(got, ref) == []


@pytest.mark.parametrize("resize", [False, True])
def test_mono_unit_equals_the_unit_fed_the_host_decoded_frames(omni, ctx, rig, resize):
    """PINHOLE_DEPTH's gray image: right = NULL.  Without a resize the files hold network-size pictures and are decoded straight into the unit's input block"""
    c = omni.capi
    sp_w, (comp, mean), vw = rig["weights"]
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, sp_w, comp, mean, W, H, 0.015, MAX_NUM, c.PREC_F16, N_KF_CAP)
    vlad = c.MobileNetVLAD(vctx, vw, V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, W, H, N_KF_CAP)
    cam = c.Cam(sp, vlad, N_KF_CAP, V.OUT_DIM, mono=True)
    pixels = ctx.host_alloc((N_KF, H, W), np.uint8)
    try:
        cam.set_active(N_KF)
        pixels[:] = R.resize(rig["raw"][0], W, H) if resize else rig["small"]
        want_in = pixels.copy()                                                                  # (the pinned block is gone when the asserts run)
        cam.enqueue_host(pixels, False)
        ref, ref_in = wait(cam), cam.get_input()
        cam.enqueue_jpeg_host(rig["rs"] if resize else None, rig["files"][0] if resize else rig["small_files"])
        got, got_in, status = wait(cam), cam.get_input(), cam.jpegdec_status()
        cam.enqueue_host(pixels, False)
        cam.wait()
        with pytest.raises(c.OmniError, match="did not come as JPEG files"):
            cam.jpegdec_status()
    finally:
        ctx.host_free(pixels)
        cam.close()
        sp.close()
        vlad.close()
        vctx.close()
    print(f"mono, resize {resize}: input block {int((got_in != ref_in).sum())} bytes differ; fields with other bits: {moved(got, ref)}; key points {ref['n_kps'].tolist()}")
    assert status == [c.JPEGDEC_OK] * N_KF and np.array_equal(got_in, ref_in) and np.array_equal(ref_in, want_in)
    assert (ref["n_kps"] >= 20).all() and moved(got, ref) == []


def test_a_frame_for_the_host_and_a_truncated_frame(omni, ctx, rig):
    """left frame 1 is above the decoder's capacity (width x height / 2 bytes): decoded on the calling thread, same unit.  Right frame 2 ends inside its scan:
    CORRUPT, its picture all zeros, no key points and no matches for that key frame"""
    c = omni.capi
    noise = np.random.default_rng(5).integers(0, 256, (SRC_H, SRC_W)).astype(np.uint8)
    st, big = c.jpeg_encode_host(noise, 100)
    assert st == c.JPEG_OK and len(big) > SRC_W * SRC_H // 2
    left = [rig["files"][0][0], big, rig["files"][0][2]]
    right = rig["files"][1][:2] + [rig["files"][1][2][:len(rig["files"][1][2]) // 2]]
    raw = [ctx.host_alloc((N_KF, SRC_H, SRC_W), np.uint8) for _ in range(2)]
    want = []
    for a, files in zip(raw, (left, right)):
        for k, f in enumerate(files):
            st, pix = c.jpeg_decode_host(f)
            want.append(c.JPEGDEC_HOST if f is big else st)
            a[k] = pix
    lc = stereo_cam(omni, ctx, rig, c.PREC_F16)
    try:
        cam = lc.cam
        cam.enqueue_raw_host(rig["rs"], raw[0], raw[1])
        ref, ref_in = wait(cam), cam.get_input()
        cam.enqueue_jpeg_host(rig["rs"], left, right)
        got, got_in, status = wait(cam), cam.get_input(), cam.jpegdec_status()
    finally:
        lc.close()
        for a in raw:
            ctx.host_free(a)
    assert want == [c.JPEGDEC_OK, c.JPEGDEC_HOST, c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_CORRUPT] == status
    assert np.array_equal(got_in, ref_in) and not got_in[2 * N_KF - 1].any() and got_in[N_KF - 1].any()
    assert got["n_kps"][2 * N_KF - 1] == 0 and got["n_matches"][N_KF - 1] == 0 and moved(got, ref) == []


def test_refusals_enqueue_nothing(omni, ctx, rig):
    c = omni.capi
    lc = stereo_cam(omni, ctx, rig, c.PREC_F16)
    try:
        cam = lc.cam
        lf, rf = rig["files"]
        prog = bytearray(lf[0])
        prog[prog.index(b"\xff\xc0") + 1] = 0xC2                                                  # a progressive frame header: UNSUPPORTED
        for args, word in (((rig["rs"], lf, None), "left and right"), ((rig["rs"], lf[:2], rf[:2]), "key frames"), ((None, lf, rf), "160x120"),
                           ((rig["rs"], lf, rig["small_files"]), "128x96"), ((rig["rs"], [bytes(prog)] + lf[1:], rf), "UNSUPPORTED")):
            with pytest.raises(c.OmniError, match=word):
                cam.enqueue_jpeg_host(*args)
        cam.enqueue_jpeg_host(rig["rs"], lf, rf)                                                   # (nothing is pending: the next enqueue is accepted)
        with pytest.raises(c.OmniError, match="in flight"):
            cam.enqueue_jpeg_host(rig["rs"], lf, rf)
        cam.wait()
        assert cam.jpegdec_status() == [c.JPEGDEC_OK] * (2 * N_KF)
    finally:
        lc.close()
