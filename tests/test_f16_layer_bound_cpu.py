"""The per-layer fp16 gate of tests/f16_layer_ref.py has teeth (no GPU).

A correct fp16 layer is emulated on the CPU the way the kernels compute it: fp16-valued inputs, weights rounded to nearest fp16, a
float32 convolution, the bias added in float32, ReLU (and the 2x2 max-pool), one round-to-nearest conversion to fp16.  It must pass
``check_layer``.  Then one defect at a time, each of a kind a tiled kernel can have, must fail it:
  1. one (tap, cin) product dropped for the pixels in column 31 of every 32-wide tile;
  2. the halo row between two tile rows read as zero (by the last row of each tile);
  3. one output channel using its neighbour's bias;
  4. one 64-channel K chunk (every tap of input channels [64 j, 64 j + 64)) accumulated in fp16 instead of fp32;
  5. the pool window shifted up by one pixel on the last pooled row;
  6. round-toward-zero instead of round-to-nearest on the output conversion.
The layers: one cin = 64 pooled layer (the shape of conv1b / conv2b; 8-row tiles) and one cin = 128 unpooled layer (conv4a / conv4b;
3-row tiles), at two shapes whose 32-wide tiles overhang the image.  Defect 5 applies to the pooled layer only.  The conv1a bound
helpers are checked against the library's own packer.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f16_layer_ref as R

SHAPES = [(20, 40), (12, 72)]          # 2.5 x 1.25 and 1.5 x 2.25 tiles of 8 x 32
LAYERS = {"c64_pool": (64, 64, True, 8), "c128": (128, 128, False, 3)}     # cin, cout, pool, tile rows
DEFECTS = ["drop_tap_col31", "halo_row_zero", "neighbour_bias", "chunk_in_fp16", "pool_shift_last_row", "round_toward_zero"]


def _layer(cin, cout, h, w, seed):
    rng = np.random.default_rng(seed)
    x16 = R.f16(np.maximum(rng.standard_normal((1, cin, h, w)), 0.0) * 1.5).astype(np.float32)
    wt = ((rng.random((cout, cin, 3, 3)) * 2 - 1) * np.sqrt(6.0 / (9 * cin))).astype(np.float32)
    b = ((rng.random(cout) * 2 - 1) * 0.05).astype(np.float32)
    return x16, wt, b


def _to_f16_rtz(a: np.ndarray) -> np.ndarray:
    r = a.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(a.astype(np.float64))
    r[over] = np.nextafter(r[over], np.float16(0))
    return r


def _emulate(x16, wt, b, pool, th, defect=None):
    """The fp16 layer as the kernels compute it, with at most one defect; returns the stored fp16 values as float32 [1, cout, H', W']."""
    x = torch.from_numpy(x16)
    w16 = torch.from_numpy(R.f16(wt).astype(np.float32))
    h, w = x16.shape[-2:]
    acc = F.conv2d(x, w16, padding=1)
    if defect == "drop_tap_col31":
        ci, (ky, kx) = 5, (1, 1)
        acc[:, :, :, 31::32] -= w16[None, :, ci, ky, kx, None, None] * x[:, ci, None, :, 31::32]
    elif defect == "halo_row_zero":
        for y in range(th - 1, h - 1, th):                    # the last row of a tile reads the next tile's first row as zero
            xz = x.clone()
            xz[:, :, y + 1] = 0
            acc[:, :, y] = F.conv2d(xz, w16, padding=1)[:, :, y]
    elif defect == "chunk_in_fp16":
        j = x16.shape[1] // 64 - 1
        keep = torch.ones(x16.shape[1], dtype=torch.bool)
        keep[64 * j: 64 * j + 64] = False
        acc = F.conv2d(x[:, keep], w16[:, keep], padding=1) if keep.any() else torch.zeros_like(acc)
        xp = F.pad(x, (1, 1, 1, 1))
        s = torch.zeros_like(acc, dtype=torch.float16)
        for ci in range(64 * j, 64 * j + 64):
            for ky in range(3):
                for kx in range(3):
                    s = (s.float() + w16[None, :, ci, ky, kx, None, None] * xp[:, ci, None, ky: ky + h, kx: kx + w]).half()
        acc = acc + s.float()
    bias = torch.from_numpy(b.copy())
    if defect == "neighbour_bias":
        bias[3] = bias[4]
    v = F.relu(acc + bias[None, :, None, None])
    if pool:
        pv = F.max_pool2d(v, 2, 2)
        if defect == "pool_shift_last_row":
            pv[:, :, -1] = F.max_pool2d(v[:, :, h - 3: h - 1], 2, 2)[:, :, 0]
        v = pv
    a = v.numpy()
    out = _to_f16_rtz(a) if defect == "round_toward_zero" else a.astype(np.float16)
    return out.astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_correct_emulation_passes_and_every_defect_fails(layer, shape):
    cin, cout, pool, th = LAYERS[layer]
    h, w = shape
    x16, wt, b = _layer(cin, cout, h, w, seed=cin + h)
    y, E, _ = R.conv_ref(x16, wt, b, relu=True, pool=pool)
    clean = R.check_layer(_emulate(x16, wt, b, pool, th), y, E)
    assert clean["ok"] and clean["violations"] == 0, clean
    assert 0.0 < clean["frac_ne"] < 0.05, clean                 # rounding ties aside, the emulation IS fp16(y)
    for defect in DEFECTS:
        if defect == "pool_shift_last_row" and not pool:
            continue
        r = R.check_layer(_emulate(x16, wt, b, pool, th, defect), y, E)
        assert not r["ok"] and r["violations"] > 0, (defect, r)


def test_ulp16_and_directed_rounding():
    v = np.array([0.0, 2.0 ** -24, 2.0 ** -14, 1.0, 1.5, -3.0, 65504.0])
    assert np.array_equal(R.ulp16(v), [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 32.0])
    x = np.array([1.0 + 2.0 ** -12, 1.0, 0.1, 2.0 ** -30])
    lo, hi = R.f16_down(x), R.f16_up(x)
    assert (lo <= x).all() and (hi >= x).all() and ((hi - lo) <= R.ulp16(x)).all()
    assert lo[1] == hi[1] == 1.0 and lo[3] == 0.0 and hi[3] == 2.0 ** -24


def test_check_layer_rejects_values_that_are_not_fp16():
    y = np.full((1, 1, 2, 2), 1.0)
    got = y.copy()
    got[0, 0, 1, 0] += 2.0 ** -13                                # inside the allowance, but not a half
    r = R.check_layer(got, y, np.zeros_like(y))
    assert not r["ok"] and not r["representable"]


def test_conv1a_u8_split_matches_the_library_packer(omni):
    """The conv1a bound of the fused conv1b (OMNI_PP_U8=1) restates conv1a_pack_u8_weights; the library's own fragments hold the same
    halfs, and the bound covers the packed algebra evaluated exactly over every byte value."""
    from oracle import superpoint_ref as S
    wts = S.synth_weights(0)
    w, b = wts["conv1a.weight"].reshape(64, 9), wts["conv1a.bias"]
    frag, _ = omni.capi.sp_pack_constants(0, w, b)
    f = frag.view(np.float16).astype(np.float64).reshape(2, 2, 64, 8)        # [k step j][m][lane][slot]
    Wh, Wl, bh, bl = R.conv1a_u8_split(w, b)
    for m in range(2):
        co = m * 32 + np.arange(32)
        assert np.array_equal(f[0, m, :32, 0::2], Wh[co, 0:4]) and np.array_equal(f[0, m, :32, 1::2], Wl[co, 0:4])
        assert np.array_equal(f[0, m, 32:, 0::2], Wh[co, 5:9]) and np.array_equal(f[0, m, 32:, 1::2], Wl[co, 5:9])
        assert np.array_equal(f[1, m, :32, 0], Wh[co, 4]) and np.array_equal(f[1, m, :32, 1], Wl[co, 4])
        assert np.array_equal(f[1, m, 32:, 0], bh[co]) and np.array_equal(f[1, m, 32:, 1], bl[co])
    delta = R.conv1a_u8_delta(w, b)
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.integers(0, 256, (4000, 9)), np.zeros((1, 9), np.int64), np.full((1, 9), 255)])
    ideal = ((Wh + Wl)[None] * (4.0 + p[:, None, :] / 256.0)).sum(2) + (bh + bl)[None]
    exact = (w.astype(np.float64)[None] * R.x_oracle(p)[:, None, :].astype(np.float64)).sum(2) + b.astype(np.float64)[None]
    assert (np.abs(ideal - exact) <= delta[None]).all()
    assert delta.max() < 1e-4 * max(1.0, np.abs(w).sum(1).max())               # far below half an fp16 step of a typical activation
    assert (R.conv1a_table_delta(w, b) < 1e-4 * max(1.0, np.abs(w).sum(1).max())).all()
