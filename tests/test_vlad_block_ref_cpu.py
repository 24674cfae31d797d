"""The per-block gates of tests/vlad_block_ref.py accept honest arithmetic and have teeth (no GPU).

A stand-in for each arithmetic of the MobileNetVLAD kernels is run on the CPU, block by block, each block from the stand-in's own previous output (as the GPU
test chains the taps):
  any                       float32 torch evaluation of every stage, order unknown;
  valu, layers, mblock (with and without the hidden-layer split), pw_mfma3
                            the exact-f32 kernels: float32 fmaf chains in each kernel's own order (vlad_block_ref.expand_order / project_order);
  split                     the pointwise convolutions as float32-accumulated groups of 16 exact products of halfs, x_hi W_hi + x_lo W_hi + x_hi W_lo, bias as
                            be_hi + be_lo, depthwise in float32 (vlad_sblock_kernel);
  f16                       input, We, Wp, h and d rounded to nearest fp16, float32 accumulation, unrounded residual (vlad_hblock_kernel).
Each must pass every block's gate and the head's; so must the oracle's own float32 layers (oracle/mobilenetvlad_ref.py) run on the stand-in's inputs, against
the order-free gate.  Then one block's output is mutated the way the descriptor gates cannot see (4e-6 .. 5e-4 on the descriptor) and that block's gate must
reject it: one pixel x 1.01, the corner pixel taking its neighbour's value, the last column x (1 + 1e-4), the last channel x (1 + 1e-4), in blocks 0, 1, 6, 13
and 16.  All four for the fp32-class gates; for the fp16-mode gate the first two, the other two are reported (``-s`` shows the line).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mobilenetvlad_ref as V
from omni_swarm_amd import synth
from tests import vlad_block_ref as R

SHAPES = [(150, 210), (104, 136)]
N_BLOCKS = len(V.BLOCKS)
MUTATED_BLOCKS = (0, 1, 6, 13, 16)
MUTATIONS = ("pixel", "corner", "column", "channel")
# (path, OMNI_VLAD_MBLOCK_CPW): every arithmetic the gates of tests/vlad_block_ref.py know
CASES = [("any", 0), ("valu", 0), ("layers", 0), ("mblock", 0), ("mblock", 2), ("pw_mfma3", 0), ("split", 0), ("f16", 0)]
case_id = lambda c: c[0] + (f"_cpw{c[1]}" if c[1] else "")

f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
h16 = lambda t: t.to(torch.float16).to(torch.float32)
relu6 = lambda t: t.clamp(0.0, 6.0)


@functools.lru_cache(maxsize=None)
def weights():
    return V.synth_weights()


def fma32(a, Ag, Wg):
    """One instruction of an exact-f32 kernel: an fmaf chain over the group's slots (the products of fp32 operands are not rounded on their own)."""
    for j in range(Ag.shape[1]):
        t = Ag[:, j, None] * Wg[None, :, j, None, None]
        a = (t if a is None else a.double() + t).float()
    return a


def dot32(a, Ag, Wg):
    """One matrix-core instruction on halfs: exact products, summed in float32 and added to the accumulator."""
    S = torch.einsum("nkhw,ck->nchw", Ag.float(), Wg.float())
    return S if a is None else a + S


def standin_block(x, block, path, cpw=0):
    """float32 [N, cout, H', W'] from float32 x, in the arithmetic and the summation order of ``path``."""
    B = R.block_weights(weights(), block)
    x = f32(x)
    x64 = x.double()
    wd, bd, wp, bp = f32(B["wd"])[:, None], f32(B["bd"]), f32(B["wp"]), f32(B["bp"])
    bc = lambda v, like: v[None, :, None, None].expand(like.shape[0], -1, like.shape[2], like.shape[3])
    if B["we"] is None:
        path, h = ("any" if path == "any" else "valu"), x
    elif path == "any":
        h = relu6(torch.einsum("nkhw,ck->nchw", x, f32(B["we"])) + f32(B["be"])[None, :, None, None])
    elif path == "split":
        h = relu6(R.run_sum(*R.split_expand_ops(x64, B), eval32=dot32))
    elif path == "f16":
        h = h16(relu6(R.run_sum(*R.f16_expand_ops(x64, B), eval32=dot32)))
    else:
        first, chains = R.expand_order(path, x.shape[1])
        bias = bc(f32(B["be"]).double(), x)
        h = relu6(R.run_sum(x64, f32(B["we"]).double(), chains, init=bias if first else None, tail=() if first else (bias,), eval32=fma32))
    d = relu6(F.conv2d(h, wd, bd, stride=B["stride"], padding=1, groups=h.shape[1]))
    tail = [bc(bp.double(), d)] + ([x64] if B["res"] else [])
    if path == "any":
        y = torch.einsum("nkhw,ck->nchw", d, wp) + bp[None, :, None, None]
        y = y + x if B["res"] else y
    elif path == "split":
        y = R.run_sum(*R.split_project_ops(d, B), tail=tail, eval32=dot32)
    elif path == "f16":
        y = R.run_sum(h16(d).double(), h16(wp).double(), [R._chunks(np.arange(d.shape[1]), 16)], tail=tail, eval32=dot32)
    else:
        y = R.run_sum(d.double(), wp.double(), R.project_order(path, d.shape[1], cpw), tail=tail, eval32=fma32)
    return y.numpy()


def standin_stem_b0(img, mask):
    wf, b = R.stem_weights(weights())
    g = R.masked_u8(img, mask)
    x = (f32(g.astype(np.float32)) - 128.0) / 128.0
    s = relu6(F.conv2d(x[:, None], f32(wf)[:, None], f32(b), stride=2, padding=1))
    return s.numpy(), standin_block(s.numpy(), 0, "valu")


def oracle_block(x, block):
    """Block ``block`` as oracle/mobilenetvlad_ref.forward evaluates its layers (float32 F.conv2d on OIHW weights)."""
    x = f32(x)
    t = lambda n: torch.from_numpy(weights()[n])
    for name, kind, cin, cout, stride in V.layer_specs():
        if not name.startswith(f"b{block}."):
            continue
        wt, bs = t(name + ".weight"), t(name + ".bias")
        if kind == "pw_relu6":
            block_in = x
            x = F.relu6(F.conv2d(x, wt, bs))
        elif kind == "dw3x3_relu6":
            x = F.relu6(F.conv2d(x, wt, bs, stride=stride, padding=1, groups=cin))
        elif kind == "pw_linear":
            x = F.conv2d(x, wt, bs)
        else:
            x = F.conv2d(x, wt, bs) + block_in
    return x.numpy()


def image(h, w, nb=1):
    return np.stack([synth.image_u8(900 + i, h, w, n_shapes=80) for i in range(nb)])


@functools.lru_cache(maxsize=None)
def chain(h, w, path, cpw=0):
    """The stand-in's outputs b0 .. b16 at (h, w) on ``path`` and, per block, the gate's (y, E) from the stand-in's input to that block."""
    img = image(h, w)
    outs, refs = [standin_stem_b0(img, False)[1]], [R.stem_b0_ref(img, False, weights())]
    for b in range(1, N_BLOCKS):
        refs.append(R.block_ref(outs[-1], weights(), b, path, cpw))
        outs.append(standin_block(outs[-1], b, path, cpw))
    return outs, refs


@pytest.mark.parametrize("mode", CASES, ids=case_id)
@pytest.mark.parametrize("h,w", SHAPES)
def test_honest_standins_pass_every_block_gate(h, w, mode):
    outs, refs = chain(h, w, *mode)
    bad = []
    for b, (got, (y, E)) in enumerate(zip(outs, refs)):
        r = R.check_layer(got, y, E, f16_out=False)
        print(f"{h}x{w} {mode} b{b}: worst ratio {r['ratio']:.3f}, not fp32(ref) {r['frac_ne']:.2e}, median allowance / |ref| {np.median(E / np.maximum(np.abs(y), 1e-30)):.1e}")
        if not r["ok"]:
            bad.append((b, r))
    assert not bad, bad


@pytest.mark.parametrize("h,w", SHAPES)
def test_the_oracles_float32_layers_pass_the_exact_path_gate(h, w):
    outs, refs = chain(h, w, "any")
    bad = []
    for b in range(1, N_BLOCKS):
        r = R.check_layer(oracle_block(outs[b - 1], b), *refs[b], f16_out=False)
        if not r["ok"]:
            bad.append((b, r))
    assert not bad, bad


def mutate(y, kind):
    m = np.array(y, np.float32, copy=True)
    if kind == "pixel":
        m[:, :, -1, -1] *= np.float32(1.01)
    elif kind == "corner":
        m[:, :, 0, 0] = m[:, :, 0, 1]
    elif kind == "column":
        m[..., -1] *= np.float32(1.0 + 1e-4)
    else:
        m[:, -1] *= np.float32(1.0 + 1e-4)
    assert not np.array_equal(m, y)
    return m


@pytest.mark.parametrize("block", MUTATED_BLOCKS)
@pytest.mark.parametrize("mode", [c for c in CASES if c[0] != "any"], ids=case_id)
@pytest.mark.parametrize("h,w", SHAPES)
def test_every_listed_mutation_of_a_block_output_is_rejected(h, w, mode, block):
    """The narrowest margins are the split gate's in block 16: last channel x (1 + 1e-4) is 1.22 times the allowance at 150 x 210, 1.76 times at 104 x 136, the
    last column 3.7 times; an honest stand-in sits at 0.02."""
    outs, refs = chain(h, w, *mode)
    must = MUTATIONS if mode[0] != "f16" else MUTATIONS[:2]
    missed, record = [], []
    for kind in MUTATIONS:
        r = R.check_layer(mutate(outs[block], kind), *refs[block], f16_out=False)
        if kind in must:
            if r["ok"]:
                missed.append((kind, round(r["ratio"], 3)))
        else:
            record.append(f"{kind}: {'accepted' if r['ok'] else 'rejected'} (ratio {r['ratio']:.2f})")
    if record:
        print(f"{h}x{w} fp16-mode gate b{block}, mutations of 1e-4: " + "; ".join(record))
    assert not missed, missed


@pytest.mark.parametrize("h,w", SHAPES)
def test_head_standin_passes_and_mutations_fail(h, w):
    """float32 evaluation of soft assignment, aggregation + the two normalisations and FC + normalisation, each from the previous stand-in's output."""
    vw = weights()
    feat = chain(h, w, "any")[0][-1]
    f = f32(feat)
    aw, ab = f32(vw["vlad.assign.weight"]).reshape(V.N_CLUSTERS, -1), f32(vw["vlad.assign.bias"])
    a = torch.softmax(torch.einsum("ndhw,kd->nkhw", f, aw) + ab[None, :, None, None], 1)
    c = f32(vw["vlad.clusters"])
    v = (a.flatten(2)[:, :, None, :] * (c[None, :, :, None] - f.flatten(2)[:, None])).sum(-1)
    v = v / v.norm(dim=2, keepdim=True)
    v = v.reshape(1, -1)
    v = (v / v.norm(dim=1, keepdim=True))[:, :, None, None]
    y = v.flatten(1) @ f32(vw["fc.weight"]).T + f32(vw["fc.bias"])
    y = (y / y.norm(dim=1, keepdim=True))[:, :, None, None]
    gates = {"assign": (a.numpy(), R.assign_ref(feat, vw)), "vlad": (v.numpy(), R.vlad_ref(feat, a.numpy(), vw)), "out": (y.numpy(), R.fc_ref(v.numpy(), vw))}
    for name, (got, (ref, E)) in gates.items():
        r = R.check_layer(got, ref, E, f16_out=False)
        print(f"{h}x{w} {name}: worst ratio {r['ratio']:.3f}, median allowance / |ref| {np.median(E / np.maximum(np.abs(ref), 1e-30)):.1e}")
        assert r["ok"], (name, r)
        m = got.copy()
        j = int(np.abs(ref[0, :, 0, 0]).argmax())
        m[:, j] *= np.float32(1.01)                                   # one cluster / entry off by 1 %
        assert not R.check_layer(m, ref, E, f16_out=False)["ok"], name
    # the oracle's own head on the same features: its assignment, its normalised NetVLAD vector and its descriptor
    o = V.forward(vw, image(h, w))
    assert np.abs(o[:, :, None, None] - gates["out"][1][0]).max() < 2e-3       # (the oracle's own backbone: a whole-network float32 difference)


@pytest.mark.parametrize("h,w", SHAPES)
def test_stem_b0_ref_equals_the_oracle(h, w):
    """Unmasked: the oracle's layers up to block 0's projection, to fp32 noise.  Masked: the oracle on the blanked frame."""
    vw = weights()
    img = image(h, w, 2)
    img[:, h * 3 // 4:] = 200

    def oracle_b0(g):
        x = (torch.from_numpy(g).float() - 128.0) / 128.0
        x = F.relu6(F.conv2d(x[:, None].repeat(1, 3, 1, 1), torch.from_numpy(vw["stem.weight"]), torch.from_numpy(vw["stem.bias"]), stride=2, padding=1))
        return x.numpy(), oracle_block(x.numpy(), 0)

    for mask in (False, True):
        blank = img.copy()
        if mask:
            blank[:, h * 3 // 4: h * 3 // 4 + h // 4] = 0
        s_o, y_o = oracle_b0(blank)
        (s, Es), (y, E) = R.stem_ref(img, mask, vw), R.stem_b0_ref(img, mask, vw)
        assert s.shape == s_o.shape and y.shape == y_o.shape == (2, 8, (h + 1) // 2, (w + 1) // 2)
        assert np.abs(s - s_o).max() < 2e-6 * max(1.0, np.abs(s).max()) and np.abs(y - y_o).max() < 2e-6 * max(1.0, np.abs(y).max())
        assert R.check_layer(standin_stem_b0(img, mask)[0], s, Es, f16_out=False)["ok"]
        assert R.check_layer(standin_stem_b0(img, mask)[1], y, E, f16_out=False)["ok"]
    masked_differs = np.abs(R.stem_b0_ref(img, True, vw)[0] - R.stem_b0_ref(img, False, vw)[0]).max()
    assert masked_differs > 1e-3
