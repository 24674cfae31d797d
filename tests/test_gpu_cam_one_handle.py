"""Every arrival form of a key-frame unit goes through one body (cam_input_run, csrc/cam.hip) and shares the handle's two staging buffers: what the per-entry tests
do not see is ONE handle taking the forms one after another -- the buffers grow, change roles (uploaded raw frames, decoded frames, the input block decoded into
directly) and are read at other offsets.  The rig of tests/test_gpu_cam_jpegdec.py: frames 160 x 120, networks at 128 x 96, 3 key frames in a handle made for 4,
PREC_F16; the raw frames are the host-decoded pixels of the files, so every form of one sequence feeds the networks the same bytes and every comparison is exact."""
import ctypes

import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from tests import resize_ref as R
from tests.test_gpu_cam_jpegdec import H, KEYS, MAX_NUM, N_KF, N_KF_CAP, SRC_W, W, moved, rig, stereo_cam, wait  # noqa: F401  (rig: the module's fixture)

pytestmark = pytest.mark.gpu


def host_parts(c, cam, up, down):
    """omni_cam_enqueue_host_parts from lists of [k][H][W] arrays (down: [] for a mono handle)"""
    def pack(parts):
        return (ctypes.c_void_p * len(parts))(*[a.ctypes.data for a in parts]), (ctypes.c_int * len(parts))(*[a.shape[0] for a in parts]), len(parts)
    u, d = pack(up), pack(down) if down else (None, None, 0)
    assert c.lib().omni_cam_enqueue_host_parts(cam.h, *u, *d, W, H, 0) == 0, c.lib().omni_last_error()


def valid(res):
    """a unit's result with the rows behind each image's key points cleared: the pinned block keeps there what an EARLIER unit of this handle left (the networks
    write n_kps rows), and these sequences put units of other pictures between two units of the same ones"""
    for i, n in enumerate(res["n_kps"]):
        for k in ("kps_xy", "desc", "scores"):
            res[k][i, n:] = 0
    return res


def check(c, cam, what, want_in, ref, files=0):
    got, got_in = valid(wait(cam)), cam.get_input()
    assert np.array_equal(got_in, want_in), what
    assert ref is None or moved(got, ref) == [], (what, moved(got, ref))
    if files:
        assert cam.jpegdec_status() == [c.JPEGDEC_OK] * files, what
    else:
        with pytest.raises(c.OmniError, match="did not come as JPEG files"):
            cam.jpegdec_status()
    return got


def test_a_stereo_handle_takes_every_form_in_turn(omni, ctx, rig):
    c = omni.capi
    rs, (lf, rf), (left, right) = rig["rs"], rig["files"], rig["raw"]
    small_r = rig["small_files"][1:] + rig["small_files"][:1]                                    # network-size files for the right camera: the left one's, rotated
    pix = ctx.host_alloc((2 * N_KF, H, W), np.uint8)                                              # what the host forms upload
    lc = stereo_cam(omni, ctx, rig, c.PREC_F16)
    dev = []
    try:
        cam = lc.cam
        for n in (N_KF, 2):                                                                       # the unit the handle was set up for, then a smaller one
            cam.set_active(n)
            want = np.concatenate([R.resize(left[:n], W, H), R.resize(right[:n], W, H)])
            pix[:2 * n] = want
            cam.enqueue_host(pix[:2 * n], False)
            ref = check(c, cam, ("host", n), want, None)
            assert (ref["n_kps"] >= 20).all() and (ref["n_matches"] > 0).all()                    # not vacuous
            cam.enqueue_raw_host(rs, left[:n], right[:n])
            check(c, cam, ("raw_host", n), want, ref)
            cam.enqueue_jpeg_host(rs, lf[:n], rf[:n])
            check(c, cam, ("jpeg_host + resize", n), want, ref, 2 * n)
            cam.enqueue_raw_host_parts(rs, [left[:n - 1], left[n - 1:n]], [right[:n - 1], right[n - 1:n]])
            check(c, cam, ("raw_host_parts", n), want, ref)
            dev = [ctx.to_device(np.ascontiguousarray(a[:n])) for a in (left, right)]
            cam.enqueue_raw_dev(rs, dev[0], dev[1], SRC_W, n)
            check(c, cam, ("raw_dev", n), want, ref)
            while dev:
                ctx.free(dev.pop())
            host_parts(c, cam, [pix[:1], pix[1:n]], [pix[n:2 * n - 1], pix[2 * n - 1:2 * n]])
            check(c, cam, ("host_parts", n), want, ref)
            # files of network-size pictures, decoded straight into the input block -- against the host form fed the host-decoded pictures
            want_small = np.concatenate([rig["small"][:n], np.roll(rig["small"], -1, axis=0)[:n]])
            cam.enqueue_jpeg_host(None, rig["small_files"][:n], small_r[:n])
            got = check(c, cam, ("jpeg_host", n), want_small, None, 2 * n)
            pix[:2 * n] = want_small
            cam.enqueue_host(pix[:2 * n], False)
            check(c, cam, ("host, decoded pictures", n), want_small, got)
            assert moved(got, ref) != []                                                          # other pictures, another result
    finally:
        lc.close()
        for p in dev:
            ctx.free(p)
        ctx.host_free(pix)


def test_a_mono_handle_takes_every_form_in_turn(omni, ctx, rig):
    c = omni.capi
    sp_w, (comp, mean), vw = rig["weights"]
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, sp_w, comp, mean, W, H, 0.015, MAX_NUM, c.PREC_F16, N_KF_CAP)
    vlad = c.MobileNetVLAD(vctx, vw, V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, W, H, N_KF_CAP)
    cam = c.Cam(sp, vlad, N_KF_CAP, V.OUT_DIM, mono=True)
    pix = ctx.host_alloc((N_KF, H, W), np.uint8)
    try:
        cam.set_active(N_KF)
        want = R.resize(rig["raw"][0], W, H)
        pix[:] = want
        cam.enqueue_host(pix, False)
        ref = check(c, cam, "host", want, None)
        assert (ref["n_kps"] >= 20).all()
        cam.enqueue_jpeg_host(rig["rs"], rig["files"][0])
        check(c, cam, "jpeg_host + resize", want, ref, N_KF)
        cam.enqueue_jpeg_host(None, rig["small_files"])
        small = check(c, cam, "jpeg_host", rig["small"].copy(), None, N_KF)
        host_parts(c, cam, [pix[:2], pix[2:]], [])
        check(c, cam, "host_parts", want, ref)
        pix[:] = rig["small"]
        cam.enqueue_host(pix, False)
        check(c, cam, "host, decoded pictures", rig["small"].copy(), small)
    finally:
        ctx.host_free(pix)
        cam.close()
        sp.close()
        vlad.close()
        vctx.close()
