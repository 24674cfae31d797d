"""GPU: every inverted-residual block of MobileNetVLAD and the NetVLAD head against an fp64 recomputation from the kernel's own input, element by
element, with an allowance derived from the kernel's arithmetic and summation order (tests/vlad_block_ref.py).

A pass runs with the taps on (omni_vlad_debug_taps), then every layer is read back (omni_vlad_debug_layer) and recomputed from the layer before it:
  stem     from the image, where the plan runs the stem on its own;
  b0       from the image (stem + block 0 in one kernel: the stem's interval carried through) or from the stored stem;
  b1..b16  each from the stored output of the block before it, with the allowance of the kernel that ran it (omni_vlad_block_paths);
  assign   from b16; vlad from b16 and the stored assignment; out from the stored vlad.
Gate per element: |got - ref| <= allowance (check_layer, fp32 outputs).  A mask-skip layer is read whole, rectangle included.

MEASURED on one MI355X: per path, the worst ratio of error to allowance over the images of the path's cases / the share of elements that differ from
fp32(ref).  Every ratio must be <= 1; the tests print these lines (MEASURED ...) when run with -s.
  not measured
"""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from omni_swarm_amd import synth
from tests import vlad_block_ref as R

pytestmark = pytest.mark.gpu

N_BLOCKS = len(V.BLOCKS)
# (H, W, batch, fisheye mask): whole tiles everywhere / too small for a mask rectangle / odd maps at every stride (75 x 105 -> 38 x 53 -> 19 x 27 -> 10 x 14
# -> 5 x 7), partial tiles on every edge / the smallest shape with mask-skip rectangles / more planned layers, overhanging tiles
SHAPES = [(96, 128, 2, False), (104, 136, 1, True), (150, 210, 3, False), (240, 320, 2, True), (360, 488, 1, True)]
SWITCHES = ("OMNI_VLAD_UNFUSED", "OMNI_VLAD_SBLOCK", "OMNI_VLAD_STEM_FUSE", "OMNI_VLAD_MFMA", "OMNI_VLAD_MBLOCK_PX", "OMNI_VLAD_MFMA_PX", "OMNI_VLAD_FC_MFMA",
            "OMNI_VLAD_MASK_SKIP", "OMNI_VLAD_SB_PERSIST", "OMNI_VLAD_MBLOCK_CPW")
# path -> (environment, fp16 mode, head only)
PATHS = {
    "production": ({}, False, False),
    "split_one_tile_per_workgroup": ({"OMNI_VLAD_SB_PERSIST": "0"}, False, False),
    "exact_f32": ({"OMNI_VLAD_SBLOCK": "0"}, False, False),
    "three_launch": ({"OMNI_VLAD_SBLOCK": "0", "OMNI_VLAD_MBLOCK_PX": "0"}, False, False),
    "hidden_split": ({"OMNI_VLAD_SBLOCK": "0", "OMNI_VLAD_MBLOCK_CPW": "2"}, False, False),
    "separate_stem": ({"OMNI_VLAD_STEM_FUSE": "0"}, False, False),
    "unfused": ({"OMNI_VLAD_UNFUSED": "1"}, False, False),
    "fp16": ({}, True, False),
    "valu_fc": ({"OMNI_VLAD_FC_MFMA": "0"}, False, True),
}
CASES = [("production", s) for s in SHAPES] + [(p, s) for p in PATHS if p != "production" for s in SHAPES[2:4]]
FLAVOUR = {"hblock": "f16", "sblock": "split", "mblock": "mblock", "pw_mfma3": "pw_mfma3", "valu": "valu"}


@pytest.fixture
def switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _images(h, w, nb, seed=900):
    imgs = np.stack([synth.image_u8(seed + i, h, w, n_shapes=80) for i in range(nb)])
    imgs[:, h * 3 // 4:] = 200                                       # the band's content must not matter under the mask
    return imgs


def _net(omni, ctx, switches, path, h, w, nb):
    env, fp16, _ = PATHS[path]
    for k, v in env.items():
        switches.setenv(k, v)
    net = omni.capi.MobileNetVLAD(ctx, V.synth_weights(), V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, w, h, nb)
    if fp16:
        net.set_precision(omni.capi.PREC_F16)
    return net, int(env.get("OMNI_VLAD_MBLOCK_CPW", "0"))


class Gate:
    """Collects every layer's verdict of a test, so that one run reports all failing layers (block, path, worst element) at once."""

    def __init__(self):
        self.stats, self.failures = {}, []

    def add(self, tag, layer, r):
        s = self.stats.setdefault(layer, {"ratio": 0.0, "frac_ne": [], "where": None})
        if r["ratio"] >= s["ratio"]:
            s["ratio"], s["where"] = r["ratio"], (tag, r["where"])
        s["frac_ne"].append(r["frac_ne"])
        if not r["ok"]:
            self.failures.append(f"{tag} {layer}: worst element (b, c, y, x) = {r['where']}: {r}")

    def finish(self, name):
        for layer, s in self.stats.items():
            print(f"MEASURED {name} {layer}: worst ratio {s['ratio']:.3f} at {s['where']}, not fp32(ref) {np.mean(s['frac_ne']):.2e}")
        assert not self.failures, "\n".join(self.failures)


def gate_pass(net, imgs, mask, gate, tag, cpw=0, head_only=False):
    """Gate every layer of the LAST pass of ``net`` (over ``imgs``, taps on).  Returns the layers read."""
    vw = V.synth_weights()
    nb = len(imgs)
    plan = net.block_paths()
    names = ([] if plan["stem"] == "stem_b0" else ["stem"]) + [f"b{i}" for i in range(N_BLOCKS)] + ["assign", "vlad", "out"]
    got = {n: net.debug_layer(n, nb) for n in names}
    flav = ["layers"] * N_BLOCKS if plan["stem"] == "layers" else [FLAVOUR[p] if p else "valu" for p in plan["blocks"]]
    chk = lambda n, label, ref: gate.add(tag, label, R.check_layer(got[n], *ref, f16_out=False))
    if not head_only:
        if plan["stem"] == "stem_b0":
            chk("b0", "b0/stem_b0", R.stem_b0_ref(imgs, mask, vw))
        else:
            chk("stem", "stem/" + plan["stem"], R.stem_ref(imgs, mask, vw))
            chk("b0", "b0/" + flav[0], R.block_ref(got["stem"], vw, 0, flav[0]))
        for i in range(1, N_BLOCKS):
            chk(f"b{i}", f"b{i}/{flav[i]}", R.block_ref(got[f"b{i - 1}"], vw, i, flav[i], cpw))
    chk("assign", "assign", R.assign_ref(got[f"b{N_BLOCKS - 1}"], vw))
    chk("vlad", "vlad", R.vlad_ref(got[f"b{N_BLOCKS - 1}"], got["assign"], vw))
    chk("out", "out", R.fc_ref(got["vlad"], vw))
    return got


@pytest.mark.parametrize("path,shape", CASES, ids=[f"{p}-{s[0]}x{s[1]}" for p, s in CASES])
def test_every_block_and_the_head_meet_their_fp64_bound(omni, ctx, switches, path, shape):
    h, w, nb, mask = shape
    net, cpw = _net(omni, ctx, switches, path, h, w, nb)
    imgs = _images(h, w, nb)
    net.debug_taps(True)
    y = net.inference(imgs, fisheye_mask=mask)
    gate = Gate()
    got = gate_pass(net, imgs, mask, gate, f"{h}x{w}{' mask' if mask else ''}", cpw, PATHS[path][2])
    assert np.array_equal(got["out"][:, :, 0, 0], y)
    if path == "production" and h >= 240:
        assert len(net.mask_skip_layers()) >= 2
    net.close()
    gate.finish(path)


def test_the_matrix_reaches_every_block_kernel_and_both_stem_forms(omni, ctx, switches):
    blocks, stems = set(), set()
    for path, (h, w, nb, _) in CASES:
        for k in SWITCHES:
            switches.delenv(k, raising=False)
        net, _ = _net(omni, ctx, switches, path, h, w, 1)
        plan = net.block_paths()
        net.close()
        stems.add(plan["stem"])
        blocks |= {p for p in plan["blocks"] if p}
        assert len(plan["blocks"]) == (0 if plan["stem"] == "layers" else N_BLOCKS) and (plan["blocks"][:1] == [None]) == (plan["stem"] == "stem_b0")
        if path == "production":
            assert set(plan["blocks"][1:]) == {"sblock"} and plan["stem"] == "stem_b0"
        if path == "fp16":
            assert set(plan["blocks"][1:]) == {"hblock"}
    assert blocks == set(omni.capi.VB_NAMES) and stems == set(omni.capi.VLAD_STEM_NAMES), (blocks, stems)


def test_mask_skip_sequence_on_one_handle_meets_the_bound(omni, ctx, switches):
    """A masked pass (it calibrates the rectangles), an unmasked pass (the rotating buffers: the rectangles stay), then a masked pass of a larger batch:
    every block of every pass meets its gate, so a stale or wrongly filled rectangle fails."""
    h, w = 240, 320
    net, _ = _net(omni, ctx, switches, "production", h, w, 2)
    assert len(net.mask_skip_layers()) >= 2
    net.debug_taps(True)
    gate = Gate()
    for i, (nb, mask) in enumerate(((1, True), (1, False), (2, True))):
        imgs = _images(h, w, nb, 700 + 10 * i)
        net.inference(imgs, fisheye_mask=mask)
        gate_pass(net, imgs, mask, gate, f"pass{i}")
    net.close()
    gate.finish("sequence")


@pytest.mark.parametrize("path", ["production", "fp16"])
def test_taps_change_nothing(omni, ctx, switches, path):
    h, w, nb, mask = SHAPES[3]
    imgs = _images(h, w, nb)
    net, _ = _net(omni, ctx, switches, path, h, w, nb)
    off = net.inference(imgs, fisheye_mask=mask)
    net.debug_taps(True)
    on = net.inference(imgs, fisheye_mask=mask)
    net.debug_taps(False)
    off2 = net.inference(imgs, fisheye_mask=mask)
    net.close()
    assert np.array_equal(on, off) and np.array_equal(off2, off)


def test_debug_layer_error_returns(omni, ctx, switches):
    c = omni.capi
    h, w, _, mask = SHAPES[1]
    net, _ = _net(omni, ctx, switches, "production", h, w, 2)
    imgs = _images(h, w, 1)
    net.inference(imgs, fisheye_mask=mask)
    with pytest.raises(c.OmniError):                                  # taps off
        net.debug_layer("b3", 1)
    net.debug_taps(True)
    with pytest.raises(c.OmniError):                                  # no pass with the taps on yet
        net.debug_layer("b3", 1)
    net.inference(imgs, fisheye_mask=mask)
    assert net.debug_layer("b3", 1).shape == (1, 16, 13, 17) and net.debug_layer("assign", 1).shape == (1, V.N_CLUSTERS, 4, 5)
    for bad in ("b17", "b-1", "b", "b3x", "conv1a", ""):
        with pytest.raises(c.OmniError):
            net.debug_layer(bad, 1)
    with pytest.raises(c.OmniError):                                  # the last pass had one image
        net.debug_layer("b3", 2)
    with pytest.raises(c.OmniError):                                  # the stem is inside vlad_stem_b0_kernel on this plan
        net.debug_layer("stem", 1)
    net.debug_taps(False)
    with pytest.raises(c.OmniError):
        net.debug_layer("out", 1)
    net.close()
