"""CPU checks of the image-independent band of the fisheye mask (csrc/superpoint.hip sp_mask_skip_rects, omni_sp_mask_band_plan; the GPU side is
tests/test_gpu_mask_band.py).  LoopCam blanks the lower quarter of every image: an output pixel of a layer holds the same bits whatever the image
when every tap of its receptive field lies in the blanked rows or in the zero padding, and the whole tile rows made of such pixels are left out
of the persistent kernels' walks.  The library's plan is compared with a brute-force propagation of "does not depend on the image" through the
layers, pixel by pixel, written here independently; with the 600 x 480 values worked out by hand; and with the rectangles of
omni_sp_mask_skip_plan (the part of the band where the output is one vector), which must lie inside the band and stay what they were."""
import numpy as np
import pytest

SIZES = [(480, 600), (480, 640), (360, 488), (240, 320), (104, 136), (64, 96)]
# (heights that are no multiple of 4: the blanked rows [3H/4, 3H/4 + H/4) stop one to three rows short of the bottom edge -- nothing reaches down to it)
SIZES_SHORT = [(122, 136), (486, 600), (243, 320)]
# conv1b, conv2a, conv2b, conv3a, conv3b: rows of the kernels' output tiles (fp16: CONV_TH = 8, the register-stationary cin = 128 kernel's 6; OMNI_PREC_SPLIT: 4, and 2
# for cin = 128), and whether a 2 x 2 max-pool follows
TILE_ROWS = {"F16": (8, 8, 8, 8, 6), "SPLIT": (4, 4, 4, 4, 2)}
POOL = (True, False, True, False, True)


@pytest.fixture(scope="module")
def capi():
    import omni_loader
    return omni_loader.load().capi


def _conv3x3(ind):
    """a 3x3 padding-1 output pixel is independent when every tap INSIDE the map is (taps outside are padding: zeros whatever the image)"""
    p = np.pad(ind, 1, constant_values=True)
    h, w = ind.shape
    out = np.ones_like(ind)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + h, dx:dx + w]
    return out


def _pool2x2(ind):
    h, w = ind.shape[0] // 2, ind.shape[1] // 2
    v = ind[:2 * h, :2 * w]
    return v[0::2, 0::2] & v[0::2, 1::2] & v[1::2, 0::2] & v[1::2, 1::2]


def _brute_force(h, w, tile_rows):
    """per layer conv1b .. conv3b: (first tile row of the band, tile rows) of the conv-output tile grid"""
    ind = np.zeros((h, w), bool)
    ind[h * 3 // 4:h * 3 // 4 + h // 4] = True                    # omni_fisheye_mask_rows
    ind = _conv3x3(ind)                                           # conv1a
    out = []
    for th, pool in zip(tile_rows, POOL):
        ind = _conv3x3(ind)
        tiles_y = -(-ind.shape[0] // th)
        ok = [bool(ind[t * th:(t + 1) * th].all()) for t in range(tiles_y)]       # (rows past the map's last are outside it: nothing to depend on)
        ty0 = tiles_y
        while ty0 > 0 and ok[ty0 - 1]:
            ty0 -= 1
        out.append((ty0, tiles_y))
        if pool:
            ind = _pool2x2(ind)
    return out


@pytest.mark.parametrize("prec", ["F16", "SPLIT"])
@pytest.mark.parametrize("shape", SIZES + SIZES_SHORT)
def test_band_plan_is_the_brute_force_propagation(capi, shape, prec):
    h, w = shape
    want = _brute_force(h, w, TILE_ROWS[prec])
    for layer, (ty0, tiles_y) in enumerate(want, start=1):
        got = capi.sp_mask_band_plan(w, h, getattr(capi, "PREC_" + prec), layer)
        assert got == (ty0, tiles_y, (tiles_y - ty0) / tiles_y), (shape, prec, layer, got, (ty0, tiles_y))
        assert 0 < got[0]                                          # never a whole image
    if shape in SIZES_SHORT:
        assert all(ty0 == tiles_y for ty0, tiles_y in want)        # (the brute force agrees: no band at all)
    for layer in range(6):
        assert capi.sp_mask_band_plan(w, h, capi.PREC_F32, layer)[2] == 0.0
    assert capi.sp_mask_band_plan(w, h, getattr(capi, "PREC_" + prec), 0)[2] == 0.0      # conv1a: its own rectangle is a full-width band already


def test_band_plan_for_600x480_is_the_one_worked_out_by_hand(capi):
    """rows 360-479 are blanked; conv1a is independent of the image from row 361 down, conv1b from 362, its pooled map from 181, conv2a 182, conv2b 183,
    its pooled map 92, conv3a 93, conv3b 94: the first whole tile row at or below that row, of the layer's tile rows"""
    band = lambda prec, layer: capi.sp_mask_band_plan(600, 480, prec, layer)
    F16, SPLIT = capi.PREC_F16, capi.PREC_SPLIT
    assert band(F16, 1) == (46, 60, 14 / 60)
    assert band(F16, 2) == (23, 30, 7 / 30) and band(F16, 3) == (23, 30, 7 / 30)
    assert band(F16, 4) == (12, 15, 3 / 15)
    assert band(F16, 5) == (16, 20, 4 / 20)
    assert band(SPLIT, 1) == (91, 120, 29 / 120)
    assert band(SPLIT, 2) == (46, 60, 14 / 60) and band(SPLIT, 3) == (46, 60, 14 / 60)
    assert band(SPLIT, 4) == (24, 30, 6 / 30)
    assert band(SPLIT, 5) == (47, 60, 13 / 60)
    # 64 x 96: one tile row of conv1b on the fp16 path (row 50 down of 64: tile row 7 of 8), nothing behind it
    assert band(F16, 1)[2] > 0 and capi.sp_mask_band_plan(96, 64, F16, 1) == (7, 8, 1 / 8)
    assert all(capi.sp_mask_band_plan(96, 64, F16, layer)[2] == 0.0 for layer in (2, 3, 4, 5))


@pytest.mark.parametrize("prec", ["F16", "SPLIT"])
def test_the_constant_rectangle_lies_inside_the_band(capi, prec):
    some = 0
    for h, w in SIZES:
        for layer in range(1, 6):
            (ty0, ty1, tx0, tx1), frac = capi.sp_mask_skip_plan(w, h, getattr(capi, "PREC_" + prec), layer)
            b0, tiles_y, bfrac = capi.sp_mask_band_plan(w, h, getattr(capi, "PREC_" + prec), layer)
            tiles_x = -(-(w // {1: 1, 2: 2, 3: 2, 4: 4, 5: 4}[layer]) // 32)         # the layer's conv-output map is W, W / 2 or W / 4 wide; 32-column tiles
            if ty1 > ty0:
                some += 1
                assert b0 <= ty0 and ty1 <= tiles_y and 0 <= tx0 < tx1 <= tiles_x, (h, w, layer)
                assert frac < bfrac
    assert some >= 15


def test_the_rectangle_plan_is_what_it_was(capi):
    """the values tests/test_mask_skip_cpu.py lists for omni_sp_mask_skip_plan"""
    plan = lambda h, w, prec, layer: capi.sp_mask_skip_plan(w, h, prec, layer)
    F16, SPLIT, F32 = capi.PREC_F16, capi.PREC_SPLIT, capi.PREC_F32
    assert plan(480, 600, F16, 1) == ((46, 59, 1, 18), 13 * 17 / (60 * 19))
    assert plan(480, 600, F16, 2) == ((23, 29, 1, 9), 6 * 8 / (30 * 10))
    assert plan(480, 600, F16, 3) == ((23, 29, 1, 9), 6 * 8 / (30 * 10))
    assert plan(480, 600, F16, 4) == ((12, 14, 1, 4), 2 * 3 / (15 * 5))
    assert plan(480, 600, F16, 0)[1] == 0.0
    assert plan(480, 600, SPLIT, 0) == ((46, 60, 0, 19), 14 / 60)
    assert plan(480, 600, SPLIT, 1) == ((91, 119, 1, 18), 28 * 17 / (120 * 19))
    assert plan(480, 600, SPLIT, 2) == ((46, 59, 1, 9), 13 * 8 / (60 * 10))
    assert plan(480, 600, SPLIT, 5) == ((47, 58, 1, 4), 11 * 3 / (60 * 5))
    assert plan(480, 600, F16, 5) == ((16, 19, 1, 4), 3 * 3 / (20 * 5))
    for layer in range(6):
        assert plan(64, 96, F16, layer)[1] == 0.0
        assert plan(480, 600, F32, layer)[1] == 0.0
