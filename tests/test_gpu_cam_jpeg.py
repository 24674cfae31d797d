"""send_img inside the key-frame unit (omni_cam_set_jpeg / omni_cam_jpeg: csrc/jpeg.hip on the unit's MobileNetVLAD stream) against the g++ build of the same
arithmetic (csrc/jpeg_plan.h inside the library, held to Pillow's whole files by tests/test_jpeg_plan_cpu.py) run on the unit's OWN input block
(omni_cam_get_input) with the mask row applied: every main image byte for byte, and every other output of omni_cam_wait with the bits of the same unit with the
stage off.  Networks at 128 x 96 (omni_fisheye_mask_rows: rows 72..95), max_num 100: a stereo handle of four directions (main images = the up images) and a mono
handle of four images (main images = all), fed through omni_cam_enqueue_host with and without fisheye_mask; two units in flight; a partly filled unit."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth

pytestmark = pytest.mark.gpu

W, H, DIRS, MAX_NUM, QUALITY, ROW0 = 128, 96, 4, 100, 75, 72
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")


@pytest.fixture(scope="module")
def rig(omni, ctx):
    from omni_swarm_amd import frontend
    c = omni.capi
    ctx_b = c.Context(0)
    comp, mean = synth.pca()
    sw, vw = S.synth_weights(0), V.synth_weights()
    cams = [frontend.LoopCam(x, sw, comp, mean, vw, V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, c.PREC_F16, n_dirs=DIRS) for x in (ctx, ctx_b)]
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, sw, comp, mean, W, H, 0.015, MAX_NUM, c.PREC_F16, DIRS)
    vlad = c.MobileNetVLAD(vctx, vw, V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, W, H, DIRS)
    mono = c.Cam(sp, vlad, DIRS, V.OUT_DIM, mono=True)
    units = []
    for u in range(2):
        a = ctx.host_alloc((2 * DIRS, H, W), np.uint8)
        up = np.stack([synth.image_u8(9300 + 16 * u + k, H, W, n_shapes=60) for k in range(DIRS)])
        a[:] = np.concatenate([up, np.roll(up, -3, axis=1)])
        units.append(a)
    yield {"cams": cams, "mono": mono, "units": units}
    mono.close()
    sp.close()
    vlad.close()
    for lc in cams:
        lc.close()
    for x in (vctx, ctx_b):
        x.close()
    for a in units:
        ctx.host_free(a)


def run(cam, images, mask, quality):
    cam.set_jpeg(quality)
    cam.enqueue_host(images, mask)
    res = {k: v.copy() for k, v in cam.wait().items()}
    return res, (cam.jpeg() if quality else None), cam.get_input()


def check_unit(c, cam, images, mask, n_main):
    off, _, _ = run(cam, images, mask, 0)
    on, files, inp = run(cam, images, mask, QUALITY)
    assert np.array_equal(inp, images) and len(files) == n_main                 # the input block keeps the unblanked pixels on the _host path
    differing = 0
    for i, (st, data) in enumerate(files):
        st_h, ref = c.jpeg_encode_host(inp[i], QUALITY, zero_from_row=ROW0 if mask else -1)
        differing += abs(len(data) - len(ref)) + sum(a != b for a, b in zip(data, ref))
        assert st == st_h == c.JPEG_OK and data == ref, (i, st, len(data), len(ref))
        if mask:
            blank = inp[i].copy()
            blank[ROW0:] = 0
            assert data == c.jpeg_encode_host(blank, QUALITY)[1] != c.jpeg_encode_host(inp[i], QUALITY)[1]        # the mask reaches the picture
    moved = [k for k in KEYS if not np.array_equal(on[k].view(np.uint8), off[k].view(np.uint8))]
    print(f"{n_main} main images, mask {mask}: differing JPEG bytes {differing}; other outputs with other bits: {moved}")
    assert moved == []
    return files


@pytest.mark.parametrize("mask", [True, False])
def test_stereo_unit_main_images_equal_the_cpu_build_and_nothing_else_changes(omni, rig, mask):
    cam = rig["cams"][0].cam
    cam.set_active(DIRS)
    check_unit(omni.capi, cam, rig["units"][0], mask, DIRS)
    cam.set_jpeg(0)


@pytest.mark.parametrize("mask", [False, True])
def test_mono_unit_encodes_every_image(omni, rig, mask):
    cam = rig["mono"]
    images = np.ascontiguousarray(rig["units"][1][:DIRS])
    files = check_unit(omni.capi, cam, images, mask, DIRS)
    assert len({f for _, f in files}) == DIRS
    cam.set_jpeg(0)


def test_two_units_in_flight(omni, rig):
    c = omni.capi
    a, b = (lc.cam for lc in rig["cams"])
    for cam in (a, b):
        cam.set_active(DIRS)
        cam.set_jpeg(QUALITY)
    a.enqueue_host(rig["units"][0], True)
    b.enqueue_host(rig["units"][1], True)
    for cam, unit in ((b, rig["units"][1]), (a, rig["units"][0])):
        cam.wait()
        files = cam.jpeg()
        assert [f for _, f in files] == [c.jpeg_encode_host(unit[i], QUALITY, zero_from_row=ROW0)[1] for i in range(DIRS)]
        cam.set_jpeg(0)


def test_a_partly_filled_unit(omni, rig):
    c = omni.capi
    cam, unit = rig["cams"][1].cam, rig["units"][1]
    n = 2
    images = np.ascontiguousarray(np.concatenate([unit[:n], unit[DIRS:DIRS + n]]))
    cam.set_active(n)
    files = check_unit(c, cam, images, True, n)
    assert [f for _, f in files] == [c.jpeg_encode_host(unit[i], QUALITY, zero_from_row=ROW0)[1] for i in range(n)]
    cam.set_jpeg(0)
    cam.set_active(DIRS)


def test_truncated_image_and_refusals(omni, rig):
    c = omni.capi
    L = c.lib()
    cam, unit = rig["cams"][0].cam, rig["units"][0]
    cam.set_active(DIRS)
    sizes = [len(c.jpeg_encode_host(unit[i], QUALITY, zero_from_row=ROW0)[1]) for i in range(DIRS)]
    big = int(np.argmax(sizes))
    assert sizes.count(sizes[big]) == 1
    cam.set_jpeg(QUALITY, sizes[big] - 1)
    cam.enqueue_host(unit, True)
    assert L.omni_cam_set_jpeg(cam.h, 50, 4096) == c.ERR_INVALID and b"in flight" in L.omni_last_error()
    r = c._CamJpeg()
    assert L.omni_cam_jpeg(cam.h, r) == c.ERR_INVALID and b"in flight" in L.omni_last_error()
    cam.wait()
    files = cam.jpeg()
    assert [st for st, _ in files] == [c.JPEG_TRUNCATED if i == big else c.JPEG_OK for i in range(DIRS)] and files[big][1] == b""
    assert L.omni_cam_set_jpeg(cam.h, 50, c.JPEG_HEADER_BYTES + 1) == c.ERR_INVALID and b"capacity" in L.omni_last_error()
    assert L.omni_cam_set_jpeg(cam.h, 101, 4096) == c.ERR_INVALID and b"quality" in L.omni_last_error()
    cam.set_jpeg(0)
    cam.enqueue_host(unit, True)
    cam.wait()
    assert L.omni_cam_jpeg(cam.h, r) == c.ERR_INVALID and b"stage off" in L.omni_last_error()
