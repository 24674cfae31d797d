"""The key-frame unit fed RAW fisheye pairs as JPEG FILES (omni_cam_enqueue_fisheye_jpeg_host: the decode kernels of csrc/jpeg_dec.hip, then flatten_unit_kernel,
inside the unit on its SuperPoint stream) against the same unit fed the host-decoded pixels of the same files (omni_jpeg_decode_host) through
omni_cam_enqueue_fisheye_host: omni_cam_get_input and EVERY field of omni_cam_result bit-identical.  The reference has no such path (its upstream, VINS-Fisheye,
decodes and flattens): parity is against this project's own decode and flatten stages.
Rig: the one of tests/test_gpu_cam_fisheye.py scaled by about a third -- 432 x 352 frames, its MEI intrinsics scaled with the frame, fov 235 at width 200: four
side views of 200 x 104 per camera, the smallest multiple-of-8 views whose masked band SuperPoint's plan leaves out of its tile walks (csrc/sp_plan.h: the fused
conv1a, use_skip) and that still give 50 key points -- 3 key frames in a unit created for 4.  Files are made at test time with omni_jpeg_encode_host."""
import contextlib

import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth

pytestmark = pytest.mark.gpu

SRC_W, SRC_H, FOV, VW, VH, DIRS, N_KF, N_KF_CAP, MAX_NUM = 432, 352, 235.0, 200, 104, 4, 3, 4, 200
ODD_W, ODD_H = 427, 341                                                       # no multiple of 16 (nor of 8) in either dimension
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")


def mei(src_w, src_h):
    """the MEI camera of tests/test_gpu_cam_fisheye.py (1280 x 1024), its intrinsics scaled with the frame"""
    sx, sy = src_w / 1280.0, src_h / 1024.0
    return (1.8, -0.2, 0.05, 0.001, -0.002, 1100.0 * sx, 1098.0 * sy, 640.0 * sx, 512.0 * sy)


def coded(c, gray, quality=75):
    """-> (the file, its host decode)"""
    st, data = c.jpeg_encode_host(np.ascontiguousarray(gray), quality)
    assert st == c.JPEG_OK
    st, pix = c.jpeg_decode_host(data)
    assert st == c.JPEGDEC_OK and pix.shape == gray.shape
    return data, pix


def make_side(c, ctx, src_w, src_h, seed):
    """two flatten objects, N_KF files per camera and their host-decoded pixels in pinned memory"""
    from omni_swarm_amd import flatten
    maps = [flatten.generate_undist_maps(mei(src_w, src_h), VW, FOV, cam_id) for cam_id in (0, 1)]
    assert all(len(m) == 5 and all(v.shape == (VH, VW, 2) for v in m[1:]) for m in maps)
    r = {"fl": [c.Flatten(ctx, src_w, src_h, m) for m in maps], "files": [], "raw": []}
    for cam in range(2):
        a = ctx.host_alloc((N_KF, src_h, src_w), np.uint8)
        files = []
        for k in range(N_KF):
            data, pix = coded(c, synth.image_u8(seed + 10 * cam + k, src_h, src_w, n_shapes=400))
            assert len(data) <= src_w * src_h // 2                            # within the unit decoder's capacity: the kernels decode it
            files.append(data)
            a[k] = pix
        r["files"].append(files)
        r["raw"].append(a)
    return r


def free_side(ctx, r):
    for fl in r["fl"]:
        fl.close()
    for a in r["raw"]:
        ctx.host_free(a)


@pytest.fixture(scope="module")
def rig(omni, ctx):
    r = make_side(omni.capi, ctx, SRC_W, SRC_H, 7300)
    r["weights"] = (S.synth_weights(0), synth.pca(), V.synth_weights())
    yield r
    free_side(ctx, r)


@contextlib.contextmanager
def make_cam(omni, ctx, rig, prec):
    """a unit created for 4 key frames with 3 active; closed whatever the test does"""
    from omni_swarm_amd import frontend
    sp_w, (comp, mean), vw = rig["weights"]
    lc = frontend.LoopCam(ctx, sp_w, comp, mean, vw, V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), VW, VH, 0.015, MAX_NUM, prec, n_dirs=N_KF_CAP * DIRS)
    try:
        lc.cam.set_active(N_KF * DIRS)
        yield lc
    finally:
        lc.close()


def wait(lc):
    return {k: v.copy() for k, v in lc.cam.wait().items()}


def moved(a, b):
    return [k for k in KEYS if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT"])
def test_unit_of_files_equals_the_unit_fed_the_host_decoded_frames(omni, ctx, rig, prec):
    c = omni.capi
    fu, fd = rig["fl"]
    with make_cam(omni, ctx, rig, getattr(c, prec)) as lc:
        lc.cam.enqueue_fisheye_host(fu, fd, rig["raw"][0], rig["raw"][1], 1, True)
        ref, ref_in = wait(lc), lc.cam.get_input()
        lc.cam.enqueue_fisheye_jpeg_host(fu, fd, rig["files"][0], rig["files"][1], 1, True)
        with pytest.raises(c.OmniError, match="in flight"):
            lc.cam.jpegdec_status()
        got, got_in, status = wait(lc), lc.cam.get_input(), lc.cam.jpegdec_status()
        # a unit that did not come as files has no statuses to show
        lc.cam.enqueue_fisheye_host(fu, fd, rig["raw"][0], rig["raw"][1], 1, True)
        lc.cam.wait()
        with pytest.raises(c.OmniError, match="did not come as JPEG files"):
            lc.cam.jpegdec_status()
    diff = int((got_in != ref_in).sum())
    print(f"{prec}: input block {diff} of {ref_in.size} bytes differ; fields with other bits: {moved(got, ref)}; key points per up view {ref['n_kps'][:N_KF * DIRS].tolist()}, "
          f"matches {ref['n_matches'].tolist()}")
    assert status == [c.JPEGDEC_OK] * (2 * N_KF)
    assert got_in.shape == ref_in.shape == (2 * N_KF * DIRS, VH, VW) and diff == 0
    assert ref_in[:, :VH * 3 // 4].std() > 5 and not ref_in[:, VH * 3 // 4:].any()               # views with content, the masked rows zero
    assert (ref["n_kps"][:N_KF * DIRS] >= 50).all() and ref["n_matches"].sum() > 0              # not vacuous
    assert moved(got, ref) == []


def test_a_frame_for_the_host_and_a_truncated_frame(omni, ctx, rig):
    """up frame 1 is above the decoder's capacity (src_w x src_h / 2 bytes): HOST, decoded on the calling thread, same bytes.  Down frame 2 ends inside its scan:
    CORRUPT, an all-zero fisheye frame and so four all-zero views; every other view is untouched"""
    c = omni.capi
    fu, fd = rig["fl"]
    noise = np.random.default_rng(5).integers(0, 256, (SRC_H, SRC_W)).astype(np.uint8)
    st, big = c.jpeg_encode_host(noise, 100)
    assert st == c.JPEG_OK and len(big) > SRC_W * SRC_H // 2
    up = [rig["files"][0][0], big, rig["files"][0][2]]
    down = rig["files"][1][:2] + [rig["files"][1][2][:len(rig["files"][1][2]) // 2]]
    raw = [ctx.host_alloc((N_KF, SRC_H, SRC_W), np.uint8) for _ in range(2)]
    want = []
    try:
        for a, files in zip(raw, (up, down)):
            for k, f in enumerate(files):
                st, pix = c.jpeg_decode_host(f)
                want.append(c.JPEGDEC_HOST if f is big else st)
                a[k] = pix
        assert not raw[1][2].any()
        with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
            lc.cam.enqueue_fisheye_host(fu, fd, raw[0], raw[1], 1, True)
            ref, ref_in = wait(lc), lc.cam.get_input()
            lc.cam.enqueue_fisheye_jpeg_host(fu, fd, up, down, 1, True)
            got, got_in, status = wait(lc), lc.cam.get_input(), lc.cam.jpegdec_status()
            # the unit of intact files, for the views that must not have moved
            lc.cam.enqueue_fisheye_jpeg_host(fu, fd, rig["files"][0], rig["files"][1], 1, True)
            lc.cam.wait()
            clean_in = lc.cam.get_input()
    finally:
        for a in raw:
            ctx.host_free(a)
    assert want == [c.JPEGDEC_OK, c.JPEGDEC_HOST, c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_CORRUPT] == status
    assert np.array_equal(got_in, ref_in) and moved(got, ref) == []
    views = got_in.reshape(2, N_KF, DIRS, VH, VW)
    clean = clean_in.reshape(2, N_KF, DIRS, VH, VW)
    assert not views[1, 2].any() and got["n_kps"][N_KF * DIRS + 2 * DIRS:].sum() == 0 and got["n_matches"][2 * DIRS:].sum() == 0
    assert views[0, 1].any() and not np.array_equal(views[0, 1], clean[0, 1])                    # the noise frame's own views
    for cam, k in ((0, 0), (0, 2), (1, 0), (1, 1)):
        assert np.array_equal(views[cam, k], clean[cam, k]) and views[cam, k].any()


def test_source_size_that_is_no_multiple_of_16(omni, ctx, rig):
    """427 x 341 frames: the decoder's last MCU column and row are cropped at the store, and the flatten's border taps read right up to that edge"""
    c = omni.capi
    odd = make_side(c, ctx, ODD_W, ODD_H, 7400)
    try:
        with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
            lc.cam.enqueue_fisheye_host(odd["fl"][0], odd["fl"][1], odd["raw"][0], odd["raw"][1], 1, True)
            lc.cam.wait()
            ref_in = lc.cam.get_input()
            lc.cam.enqueue_fisheye_jpeg_host(odd["fl"][0], odd["fl"][1], odd["files"][0], odd["files"][1], 1, True)
            lc.cam.wait()
            got_in, status = lc.cam.get_input(), lc.cam.jpegdec_status()
            # ... and back to the other size on the same handle: the decoder is made again
            lc.cam.enqueue_fisheye_jpeg_host(rig["fl"][0], rig["fl"][1], rig["files"][0], rig["files"][1], 1, True)
            lc.cam.wait()
            assert lc.cam.jpegdec_status() == [c.JPEGDEC_OK] * (2 * N_KF)
    finally:
        free_side(ctx, odd)
    diff = int((got_in != ref_in).sum())
    print(f"{ODD_W} x {ODD_H}: input block {diff} of {ref_in.size} bytes differ")
    assert status == [c.JPEGDEC_OK] * (2 * N_KF) and got_in.shape == ref_in.shape and diff == 0
    # the views do read the frame's last column and row (a map coordinate beyond width - 2 / height - 2 inside the remapped rows)
    from omni_swarm_amd import flatten
    m = flatten.generate_undist_maps(mei(ODD_W, ODD_H), VW, FOV, 0)
    xs = np.concatenate([v[:VH * 3 // 4, :, 0].ravel() for v in m[1:]])
    ys = np.concatenate([v[:VH * 3 // 4, :, 1].ravel() for v in m[1:]])
    inside = (xs > -1) & (xs < ODD_W) & (ys > -1) & (ys < ODD_H)
    print(f"map coordinates inside the frame: x up to {xs[inside].max():.1f} of {ODD_W}, y up to {ys[inside].max():.1f} of {ODD_H}")
    assert ref_in.any()


def test_refusals_enqueue_nothing(omni, ctx, rig):
    c = omni.capi
    fu, fd = rig["fl"]
    uf, df = rig["files"]
    prog = bytearray(uf[0])
    prog[prog.index(b"\xff\xc0") + 1] = 0xC2                                                     # a progressive frame header: UNSUPPORTED
    small = coded(c, synth.image_u8(7500, 96, 128, n_shapes=40))[0]                              # a picture of another size
    from omni_swarm_amd import flatten
    other = c.Flatten(ctx, ODD_W, ODD_H, flatten.generate_undist_maps(mei(ODD_W, ODD_H), VW, FOV, 1))
    with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
        mono = c.Cam(lc.sp, lc.vlad, N_KF * DIRS, V.OUT_DIM, mono=True)
        try:
            with pytest.raises(c.OmniError, match="up frames of 432x352, down frames of 427x341"):
                lc.cam.enqueue_fisheye_jpeg_host(fu, other, uf, df, 1, True)                      # different source sizes
            with pytest.raises(c.OmniError, match="mono"):
                mono.enqueue_fisheye_jpeg_host(fu, fd, uf, df, 1, True)
            with pytest.raises(c.OmniError, match="key frames x 4 directions for a unit of 12"):
                lc.cam.enqueue_fisheye_jpeg_host(fu, fd, uf[:2], df[:2], 1, True)                 # a wrong active size
            with pytest.raises(c.OmniError, match="key frames x 5 directions"):
                lc.cam.enqueue_fisheye_jpeg_host(fu, fd, uf, df, 0, True)
            with pytest.raises(c.OmniError, match="UNSUPPORTED"):
                lc.cam.enqueue_fisheye_jpeg_host(fu, fd, [bytes(prog)] + uf[1:], df, 1, True)
            with pytest.raises(c.OmniError, match="128x96"):
                lc.cam.enqueue_fisheye_jpeg_host(fu, fd, uf, df[:2] + [small], 1, True)
            with pytest.raises(c.OmniError, match="without a pending"):                          # nothing was enqueued by any of them
                lc.cam.wait()
            lc.cam.enqueue_fisheye_jpeg_host(fu, fd, uf, df, 1, True)
            with pytest.raises(c.OmniError, match="in flight"):                                  # a unit in flight
                lc.cam.enqueue_fisheye_jpeg_host(fu, fd, uf, df, 1, True)
            r = wait(lc)                                                                         # and the handle still works
            assert lc.cam.jpegdec_status() == [c.JPEGDEC_OK] * (2 * N_KF) and (r["n_kps"][:N_KF * DIRS] >= 50).all()
        finally:
            mono.close(); other.close()
