"""The image-independent band of the fisheye mask on the GPU (omni_sp::MaskSkip in csrc/superpoint.hip; the plan's arithmetic: tests/test_mask_band_cpu.py).
A masked pass leaves whole tile rows, at full width down to the last one, out of the walks of conv1b .. conv3b; those rows were computed once over an
all-zero image into image slot 0 and copied into every other slot.  Every layer and every output must be BIT-IDENTICAL to the dense pass
(OMNI_SP_MASK_SKIP[_SPLIT]=0) and to the pass that leaves out only the constant rectangles (OMNI_SP_MASK_RECT=1, what was skipped before the band) --
whatever stands in the blanked rows of the input, after a pass without the mask, with a larger and with a partial batch.  The shapes are the smallest
at which it can go wrong: (64, 96) has a single band tile row, in conv1b only (fp16); at (104, 136) conv2a's band is a partial bottom tile row and the
right tile column is partial (the copy must clamp to the map); (240, 320) has a band in every layer."""
import numpy as np
import pytest

from oracle import superpoint_ref as S
from omni_swarm_amd import synth

pytestmark = pytest.mark.gpu
LAYERS = ["conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "heads"]
# conv1b .. conv3b: the kernels' tile rows (conv-output rows) and the factor of the pool behind the layer
TILE_ROWS = {"PREC_F16": (8, 8, 8, 8, 6), "PREC_SPLIT": (4, 4, 4, 4, 2)}
POOL = (2, 1, 2, 1, 2)


def _same(a, b):
    assert len(a) == len(b)
    for (k0, d0, s0), (k1, d1, s1) in zip(a, b):
        assert np.array_equal(k0, k1) and np.array_equal(s0, s1) and np.array_equal(d0, d1)


def _images(seed, n, h, w):
    imgs = np.stack([synth.image_u8(seed + i, h, w, n_shapes=60 if h < 200 else 200) for i in range(n)])
    imgs[:, h * 3 // 4:] = 200                                    # the blanked rows: whatever stands there must not matter
    return imgs


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT"])
@pytest.mark.parametrize("shape,batch", [((64, 96), 2), ((104, 136), 2), ((240, 320), 3)])
def test_band_is_bit_identical_to_the_dense_pass_and_to_the_rectangles(omni, ctx, shape, batch, prec, monkeypatch):
    h, w = shape
    capi = omni.capi
    env = "OMNI_SP_MASK_SKIP" if prec == "PREC_F16" else "OMNI_SP_MASK_SKIP_SPLIT"
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    imgs, imgs2 = _images(700, batch, h, w), _images(750, batch + 1, h, w)
    sps = {}
    for name, skip, rect in (("dense", "0", "0"), ("rect", "1", "1"), ("band", "1", "0")):
        monkeypatch.setenv(env, skip)
        monkeypatch.setenv("OMNI_SP_MASK_RECT", rect)
        sps[name] = capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, getattr(capi, prec), batch + 1)
    band = sps["band"]

    def check(images, n):
        got = band.inference(images, True)
        layers = {name: band.debug_layer(name, n) for name in LAYERS}
        dense = band.get_dense(n)
        for other in ("dense", "rect"):
            sp = sps[other]
            _same(sp.inference(images, True), got)
            for name in LAYERS:
                a = sp.debug_layer(name, n)
                assert np.array_equal(a, layers[name]), (other, name, int((a != layers[name]).sum()), np.argwhere(a != layers[name])[:4].tolist())
            s0, d0 = sp.get_dense(n)
            assert np.array_equal(s0, dense[0]) and np.array_equal(d0, dense[1]), other
        return layers

    # 1. a masked pass: every layer, every output
    layers = check(imgs, batch)
    # 2. the band rows are the same in two different images, and they are NOT one vector: near the side edges they vary with the column and near the bottom edge
    #    with the row (zero padding is not the constant), which only a copy of the computed rows reproduces
    plan = [capi.sp_mask_band_plan(w, h, getattr(capi, prec), layer) for layer in range(1, 6)]
    assert plan[0][2] > 0                                         # conv1b has a band at every shape here
    if shape == (64, 96) and prec == "PREC_F16":
        assert [p[2] > 0 for p in plan] == [True, False, False, False, False]
    for name, (ty0, tiles_y, frac), th, f in zip(LAYERS, plan, TILE_ROWS[prec], POOL):
        if frac == 0.0:
            continue
        rows = layers[name][:, :, ty0 * th // f:]                 # [image][channel][band row][column]
        assert rows.shape[2] > 0
        assert np.array_equal(rows[0], rows[1]), name
        mid = rows[0, :, 0, rows.shape[3] // 2]
        varies = (rows[0, :, 0, 0] != mid).any() or (rows[0, :, 0, -1] != mid).any() or (rows[0, :, -1, rows.shape[3] // 2] != mid).any()
        assert varies, name
    # 3. a pass WITHOUT the mask overwrites the band; a larger masked batch afterwards (the spare slot was filled too); then a partial batch
    plain = [sp.inference(imgs[:1], False) for sp in sps.values()]
    _same(plain[0], plain[1])
    _same(plain[0], plain[2])
    check(imgs2, batch + 1)
    check(imgs2[1:2], 1)
    for sp in sps.values():
        sp.close()
