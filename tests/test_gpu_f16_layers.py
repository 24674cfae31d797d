"""GPU: every layer of the fp16 SuperPoint path (OMNI_PREC_F16, the benchmarked one) against an fp64 recomputation from the kernel's own
input, element by element, with a bound derived from the arithmetic (tests/f16_layer_ref.py).

Production defaults throughout: OMNI_CONV_V1=0, sparse descriptors (the dense heads layer and descriptor map are made on demand from conv4b by
omni_sp_get_dense), mask skip on, conv1a fused into conv1b with its operands straight from the bytes (OMNI_PP_U8=1).  ``inference()`` runs the
production pass, then the layers are read back:
  conv1b   from the image: the fp64 conv1a, rounded to fp16, with the interval the fused conv1a may land in (conv1a_u8_delta) carried through;
  conv2a .. conv4b, each from the stored output of the layer before it (debug_layer);
  heads    (cPa | cDa, 512 channels, ReLU) from conv4b;
  semi     the fp32 heat map, from the heads' first half (the pass's detector head read cPa of the sparse pass; the sparse and dense passes
           give the same heat map bit for bit, tests/test_gpu_superpoint.py);
  desc     the dense descriptors, from the heads' second half.
Gate per element: |got - ref| <= E + extra + ulp16(got) / 2 (fp16 layers; got must be a half) or <= the fp32 tails' bound (semi, desc).

Measured on one MI355X: the worst ratio of error to allowance over all images of a test, and the fraction of elements not equal to
fp16(ref) (fp32(ref) for semi and desc).  Every ratio must be <= 1; the tests print these lines (MEASURED ...) when run with -s.
  production, 12 images over the 7 shapes:  conv1b 0.156 / 2.2e-2   conv2a 0.797 / 2.6e-4   conv2b 0.790 / 2.9e-4   conv3a 0.812 / 4.4e-4
                                            conv3b 0.567 / 5.2e-4   conv4a 0.633 / 5.8e-4   conv4b 0.586 / 5.8e-4   heads 0.642 / 4.8e-4
                                            semi 0.004 / 0.95       desc 0.004 / 0.76
  table form (OMNI_PP_U8=0):                conv1b 0.146 / 3.8e-3
  mask-skip sequence:                       conv1b 0.152, conv2a .. heads 0.565 - 0.806, semi 0.004, desc 0.005
  unaligned image (separate conv1a):        conv1a 0.999 / 1.1e-4   conv1b 0.780 / 3.1e-4   conv2a .. heads 0.538 - 0.798   semi, desc 0.004
The fp16 layers sit at 0.5 - 1.0 of their allowance: half an fp16 step dominates it, and ties of the rounding reach it.  conv1b's ratio is
lower because its allowance also carries the conv1a interval (conv1a_u8_delta: a worst-case gamma_20 over operands offset by 4, about
2.5e-5 absolute against an fp16 step of 5e-4 at 0.5): 2.2 % of its outputs differ from fp16(ref), all inside it.  The two fp32 tails sit
at 0.004 of theirs: those bounds are worst-case gamma_K sums (see tests/f16_layer_ref.py) with no final fp16 step to dominate them,
about 250 times the errors measured -- still per element and from the kernel's own input.
"""
import numpy as np
import pytest

from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import f16_layer_ref as R

pytestmark = pytest.mark.gpu

CHAIN = [("conv2a", "conv1b", False), ("conv2b", "conv2a", True), ("conv3a", "conv2b", False), ("conv3b", "conv3a", True),
         ("conv4a", "conv3b", False), ("conv4b", "conv4a", False)]
# (H, W, batch, fisheye mask)
SHAPES = [(480, 600, 2, True), (480, 640, 1, False), (208, 400, 3, True), (128, 264, 2, True), (104, 136, 1, False), (72, 104, 1, False),
          (64, 96, 2, True)]
DEFAULTS = ("OMNI_CONV_V1", "OMNI_SP_SPARSE_DESC", "OMNI_SP_SPARSE_DA", "OMNI_SP_MASK_SKIP", "OMNI_PP_U8", "OMNI_RS_TRN", "OMNI_DET16")


def rs2_transposed(hc, wc):
    """csrc/conv.hip rs2_transposed: the unpooled cin = 128 layers run on transposed 3-row tiles when that needs fewer tiles."""
    cdiv = lambda a, b: -(-a // b)
    return cdiv(wc, 3) * cdiv(hc, 32) < cdiv(wc, 32) * cdiv(hc, 3)


@pytest.fixture
def production(monkeypatch):
    for k in DEFAULTS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _images(h, w, nb, seed):
    return np.stack([synth.image_u8(seed + i, h, w, n_shapes=60 if h < 100 else 200) for i in range(nb)])


class Gate:
    """Collects every layer's verdict of a test, so that one run reports all failing layers (with the worst element) at once."""

    def __init__(self):
        self.stats, self.failures = {}, []

    def add(self, tag, layer, r):
        s = self.stats.setdefault(layer, {"ratio": 0.0, "frac_ne": [], "n": 0})
        s["ratio"] = max(s["ratio"], r["ratio"])
        s["frac_ne"].append(r["frac_ne"])
        s["n"] += 1
        if not r["ok"]:
            self.failures.append(f"{tag} {layer}: {r}")

    def finish(self, name):
        for layer, s in self.stats.items():
            print(f"MEASURED {name} {layer}: worst ratio {s['ratio']:.3f}, not fp16(ref) {np.mean(s['frac_ne']):.2e} ({s['n']} images)")
        assert not self.failures, "\n".join(self.failures)


def gate_pass(sp, weights, imgs, mask, gate, tag, conv1a="u8", layers=None):
    """Gate every layer of the LAST pass of ``sp`` (over ``imgs``).  conv1a: "u8" / "table" (fused into conv1b: the interval of
    conv1a_u8_delta / conv1a_table_delta) or "direct" (the separate conv1a_kernel<_Float16>, read back and gated itself).
    layers: a subset of names to gate (default: all)."""
    nb = len(imgs)
    want = layers or (["conv1a"] if conv1a == "direct" else []) + ["conv1b"] + [c[0] for c in CHAIN] + ["heads", "semi", "desc"]
    got = {n: sp.debug_layer(n, nb) for n in (["conv1a"] if conv1a == "direct" else []) + ["conv1b"] + [c[0] for c in CHAIN]}
    if {"heads", "semi", "desc"} & set(want):
        got["semi"], got["desc"] = sp.get_dense(nb)
        got["heads"] = sp.debug_layer("heads", nb)
    w = lambda n: weights[n + ".weight"]
    bias = lambda n: weights[n + ".bias"]
    delta = {"u8": R.conv1a_u8_delta, "table": R.conv1a_table_delta}.get(conv1a)
    for b in range(nb):
        t = f"{tag}[{b}]"
        g = R.masked_u8(imgs[b:b + 1], mask)
        if conv1a == "direct":
            # conv1a_kernel<_Float16>: acc = bias, then nine fmaf over fp32 weights and the table's fl32(p) fl32(1/255): 10 terms; ReLU; (_Float16)
            y, E, _ = R.conv_ref(R.x_oracle(g)[:, None], w("conv1a"), bias("conv1a"), relu=True, round_w=False)
            gate.add(t, "conv1a", R.check_layer(got["conv1a"][b:b + 1], y, E))
            y, E, ex = R.conv_ref(got["conv1a"][b:b + 1], w("conv1b"), bias("conv1b"), pool=True)
        else:
            x16, u_in = R.conv1a_interval(R.conv1a_ref(g, w("conv1a"), bias("conv1a")), delta(w("conv1a"), bias("conv1a")))
            y, E, ex = R.conv_ref(x16, w("conv1b"), bias("conv1b"), pool=True, u_in=u_in)
        if "conv1b" in want:
            gate.add(t, "conv1b", R.check_layer(got["conv1b"][b:b + 1], y, E, ex))
        for n, prev, pool in CHAIN:
            if n in want:
                y, E, _ = R.conv_ref(got[prev][b:b + 1], w(n), bias(n), pool=pool)
                gate.add(t, n, R.check_layer(got[n][b:b + 1], y, E))
        if "heads" in want:
            wh = np.concatenate([w("convPa"), w("convDa")])
            bh = np.concatenate([bias("convPa"), bias("convDa")])
            y, E, _ = R.conv_ref(got["conv4b"][b:b + 1], wh, bh)
            gate.add(t, "heads", R.check_layer(got["heads"][b:b + 1], y, E))
        if "semi" in want:
            y, E = R.semi_ref(got["heads"][b:b + 1, :256], w("convPb"), bias("convPb"))
            gate.add(t, "semi", R.check_layer(got["semi"][b:b + 1], y, E, f16_out=False))
        if "desc" in want:
            y, E = R.desc_ref(got["heads"][b:b + 1, 256:], w("convDb"), bias("convDb"))
            gate.add(t, "desc", R.check_layer(got["desc"][b:b + 1], y, E, f16_out=False))
    return got


def test_shapes_cover_both_tile_orientations():
    """The shape list reaches the register-stationary kernel's transposed tiles (480 x 600 .. 128 x 264) and its plain ones (104 x 136 and below)."""
    assert {rs2_transposed(h // 8, w // 8) for h, w, _, _ in SHAPES} == {True, False}
    assert rs2_transposed(60, 75) and rs2_transposed(16, 33) and not rs2_transposed(13, 17) and not rs2_transposed(9, 13)


def test_f16_every_layer_meets_its_fp64_bound(omni, ctx, production):
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    gate = Gate()
    for (h, w, nb, mask) in SHAPES:
        imgs = _images(h, w, nb, 500 + h)
        sp = omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, omni.capi.PREC_F16, nb)
        sp.inference(imgs, fisheye_mask=mask)
        gate_pass(sp, weights, imgs, mask, gate, f"{h}x{w}{' mask' if mask else ''}")
        sp.close()
    gate.finish("production")


def test_f16_table_form_conv1b_meets_its_fp64_bound(omni, ctx, production):
    """OMNI_PP_U8=0: conv1a inside conv1b through the u8 -> (hi, lo) table (conv1a_table_delta)."""
    production.setenv("OMNI_PP_U8", "0")
    weights = S.synth_weights(0)
    gate = Gate()
    for (h, w, nb, mask) in ((480, 600, 2, True), (72, 104, 1, False)):
        imgs = _images(h, w, nb, 600 + h)
        sp = omni.capi.SuperPoint(ctx, weights, None, None, w, h, 0.015, 200, omni.capi.PREC_F16, nb)
        sp.inference(imgs, fisheye_mask=mask)
        gate_pass(sp, weights, imgs, mask, gate, f"{h}x{w}", conv1a="table", layers=["conv1b"])
        sp.close()
    gate.finish("table")


def test_f16_mask_skip_sequence_on_one_handle_meets_the_bound(omni, ctx, production):
    """A masked pass, an unmasked pass (it overwrites the mask-skip rectangles), then a masked pass of a larger batch (calibrates again):
    every layer of every pass meets the gate, so stale or wrongly filled rectangles fail."""
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    h, w = 480, 600
    sp = omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, omni.capi.PREC_F16, 2)
    gate = Gate()
    for i, (nb, mask) in enumerate(((1, True), (1, False), (2, True))):
        imgs = _images(h, w, nb, 700 + 10 * i)
        sp.inference(imgs, fisheye_mask=mask)
        gate_pass(sp, weights, imgs, mask, gate, f"pass{i}")
    sp.close()
    gate.finish("sequence")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the run-time fallback to a separate conv1a: sp_forward fuses conv1a only when the device image has stride % 4 == 0 and a 4-byte aligned pointer
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _upload(ctx, imgs, how):
    """Device copy of [B, H, W] u8 images -> (pointer to pass, stride, pointer to free).  how: "aligned" (stride W), "stride" (rows W + 2 bytes
    apart: stride % 4 == 2) or "offset" (stride W, the pointer one byte past a 4-byte boundary)."""
    nb, h, w = imgs.shape
    if how == "stride":
        buf = np.zeros((nb, h, w + 2), np.uint8)
        buf[..., :w] = imgs
        p = ctx.to_device(buf)
        return p, w + 2, p
    if how == "offset":
        buf = np.zeros(imgs.size + 8, np.uint8)
        buf[1:1 + imgs.size] = imgs.ravel()
        p = ctx.to_device(buf)
        return p + 1, w, p
    p = ctx.to_device(np.ascontiguousarray(imgs))
    return p, w, p


def _dev_pass(ctx, sp, imgs, how, mask):
    p, stride, base = _upload(ctx, imgs, how)
    try:
        sp.enqueue_dev(p, stride, len(imgs), mask)
        return sp.fetch(len(imgs))
    finally:
        ctx.sync()
        ctx.free(base)


def test_f16_unaligned_image_runs_conv1a_separately_and_meets_the_bound(omni, ctx, production):
    """An image the fused kernel cannot read 4 bytes at a time: conv1a runs as conv1a_kernel<_Float16> and is materialised; it and every
    layer after it meet the fp64 gate (conv1b then reads the stored conv1a, no interval)."""
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    gate = Gate()
    for (h, w, nb, mask, how) in ((208, 400, 2, True, "stride"), (72, 104, 1, False, "offset")):
        imgs = _images(h, w, nb, 800 + h)
        sp = omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, omni.capi.PREC_F16, nb)
        _dev_pass(ctx, sp, imgs, how, mask)
        gate_pass(sp, weights, imgs, mask, gate, f"{h}x{w} {how}", conv1a="direct")
        sp.close()
    gate.finish("unaligned")


@pytest.mark.parametrize("how", ["stride", "offset"])
def test_split_unaligned_image_meets_the_fp32_class_gates(omni, ctx, production, how):
    """OMNI_PREC_SPLIT with an unaligned image: conv1a_split runs on its own (the Winograd conv1b needs the fused conv1a and is off for the
    pass); every layer within 2e-5 of its magnitude of the torch oracle, the dense outputs and the key points as test_f32_layers_and_dense_outputs
    requires of the aligned pass.
    Found here: with the pointer one byte off (stride % 4 == 0) and the mask on, conv1a at 480 x 600 was off by 0.049 at (b 0, c 3, y 368, x 0),
    inside conv1a's mask-skip rectangle (8-row tiles from row 368).  The calibration pass over the context's aligned zero image had run the fused
    conv1a, which never fills that rectangle, while the pass itself skipped it; sp_calibrate_mask_skip now calibrates with the pass's conv1a form."""
    from oracle import postproc_ref as P
    from tests.test_gpu_superpoint import CONF_TOL, LAYERS, _oracle_layers, assert_same_keypoints
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    for (h, w, mask) in ((480, 600, True), (72, 104, False)):
        imgs = _images(h, w, 2, 900 + h)
        sp = omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, omni.capi.PREC_SPLIT, 2)
        res = _dev_pass(ctx, sp, imgs, how, mask)
        semi_r, desc_r, layers_r = _oracle_layers(weights, S.preprocess_u8(imgs, fisheye_mask=mask))
        for n in LAYERS + ["heads"]:
            got, ref = sp.debug_layer(n, 2), layers_r[n]
            err = np.abs(got - ref).max()
            assert err < 2e-5 * max(1.0, np.abs(ref).max()), (h, w, n, err, np.unravel_index(np.argmax(np.abs(got - ref)), got.shape))
        semi, desc = sp.get_dense(2)
        assert np.abs(semi - semi_r).max() < CONF_TOL and np.abs(desc - desc_r).max() < 2e-5
        for b in range(2):
            xy, conf, _, _ = P.get_keypoints(semi_r[b], 0.015, 200)
            assert_same_keypoints(res[b][0], res[b][2], xy, conf)
        sp.close()


def _pass_outputs(sp, res, nb, unfused):
    names = (["conv1a"] if unfused else []) + ["conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"]
    return [a for r in res for a in r] + [sp.debug_layer(n, nb) for n in names] + list(sp.get_dense(nb))


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT"])
def test_alternating_aligned_and_unaligned_masked_passes_match_fresh_handles(omni, ctx, production, prec):
    """Aligned (fused conv1a) and unaligned (separate conv1a) masked passes alternate on one handle: the mask skip calibrates again for each
    form (mask_skip_cal_fused).  Every pass is bit-identical to a fresh handle fed the same pass -- key points, descriptors, scores, every
    stored layer, the dense outputs."""
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    h, w, nb = 480, 600, 2
    mk = lambda: omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, getattr(omni.capi, prec), nb)
    sp = mk()
    for i, how in enumerate(("aligned", "offset", "aligned", "stride", "offset")):
        imgs = _images(h, w, nb, 1000 + 10 * i)
        got = _pass_outputs(sp, _dev_pass(ctx, sp, imgs, how, True), nb, how != "aligned")
        fresh = mk()
        ref = _pass_outputs(fresh, _dev_pass(ctx, fresh, imgs, how, True), nb, how != "aligned")
        fresh.close()
        assert len(got) == len(ref)
        for j, (a, b) in enumerate(zip(got, ref)):
            assert a.shape == b.shape and np.array_equal(a, b), (prec, i, how, j, a.shape, b.shape if a.shape == b.shape else None,
                                                                 np.abs(a - b).max() if a.shape == b.shape and a.size else None)
    sp.close()
