"""GPU: every convolution layer of the fp32-class SuperPoint paths (OMNI_PREC_SPLIT in its configurations, OMNI_PREC_F32) against the ideal value of
the kernel's own algebra in float64, recomputed from the layer's own stored input, element by element (tests/split_layer_ref.py).

``inference()`` runs the production pass; the layers are read back with ``debug_layer`` and gated in two tiers:
  tier 1  |got - y| <= gamma_K T + storage (+ the fused conv1a's interval): derived, per element, never to be exceeded;
  tier 2  per slice (every output channel, every row class and column class of the kernel's tile grid) RMS(got - y) <= c RMS(emulation - y), the
          emulation being the same algebra in float32 on the CPU; split-64 outputs also meet the lo-half bias gate (``lo_bias``).
c (split_layer_ref.TIER2_C, one per kernel form) is twice the largest clean ratio measured on the MI355X over every configuration below (an MFMA's internal
order of its 16 products is not documented), and stays far below the smallest ratio any defect of tests/test_split_layer_bound_cpu.py produces (175).

The fp32 tails are gated in both tiers too, with the per-element bounds of f16_layer_ref.semi_ref / desc_ref extended with the fp32-input algebra and the float32
emulations ``semi_emul`` / ``desc_emul`` / ``convdb_split_emul``:
  semi       the heat map from the stored fp32 ``heads``: detector_head_mfma16_kernel<float>, or the exact-f32 head (OMNI_DET16=0, PREC_F32); sliced by logit
             channel (64) and by the cell's lane in its 32-cell fragment;
  desc       the dense descriptors ``get_dense`` makes of the stored cDa: the exact-f32 1 x 1 convolution + l2norm_kernel;
  desc_rows  the sparse tail the production pass itself ran: the compact cDa rows around the key points (debug_layer "desc_rows_in") against the rows made
             of them ("desc_rows_out"): convdb_l2norm_split_kernel under PREC_SPLIT (the three-term hi / lo algebra from the stored fp32 rows), the exact-f32
             convolution + l2norm_kernel under PREC_F32; every row of every key point, sliced by output channel and by the row's place in its 32-row tile.

Configurations: PREC_SPLIT at its defaults (Winograd conv1b / conv2a / conv2b with the fused conv1a, sparse heads), OMNI_SPLIT_WINO = 0, 8, 10 and 15 (the
direct cin = 64 kernels, the Winograd conv3a, the raw-32 <-> split-64 hand-overs in both directions), OMNI_SPLIT_FUSE1A=0 (conv1a a tensor, gated
itself), OMNI_DET16=0, PREC_F32; a mask-skip sequence on one handle and an unaligned image; 480 x 600 masked once for PREC_SPLIT and once for PREC_F32.  At
480 x 600 PREC_F32 meets tier 1 on every element and tier 2 on a band of eight output rows per layer that holds every channel and every row and column class
(``_f32_layer``): the float32 emulation of its product-by-product chain over the whole frame would take minutes on the CPU.

MEASURED on one MI355X, worst tier-1 ratio / worst tier-2 ratio per layer and configuration (every tier-1 ratio must be <= 1, every tier-2 ratio <= its c; printed with -s):
  split defaults        conv1b 0.0016/1.95  conv2a 0.0026/2.19  conv2b 0.0028/1.92  conv3a 0.0024/3.13  conv3b 0.0006/2.17  conv4a 0.0011/2.35
                        conv4b 0.0007/2.74  heads 0.0011/2.86  semi 0.0034/1.98  desc 0.0079/1.25  desc_rows 0.0021/1.98
  OMNI_SPLIT_WINO=0     conv1b 0.0020/1.93  conv2a 0.0027/2.75  conv2b 0.0030/1.95  conv3a 0.0024/2.52  conv3b 0.0006/1.95  conv4a 0.0010/2.15
                        conv4b 0.0008/2.17  heads 0.0008/2.59  semi 0.0034/1.83  desc 0.0069/1.19  desc_rows 0.0019/2.31
  OMNI_SPLIT_WINO=8     conv1b 0.0020/1.93  conv2a 0.0027/2.75  conv2b 0.0030/1.95  conv3a 0.0033/2.41  conv3b 0.0005/2.26  conv4a 0.0008/2.50
                        conv4b 0.0007/2.35  heads 0.0009/2.38  semi 0.0032/2.12  desc 0.0067/1.24  desc_rows 0.0018/1.79
  OMNI_SPLIT_WINO=10    conv1b 0.0020/1.93  conv2a 0.0028/2.51  conv2b 0.0024/1.59  conv3a 0.0033/1.73  conv3b 0.0006/1.99  conv4a 0.0008/2.42
                        conv4b 0.0007/2.22  heads 0.0008/2.65  semi 0.0034/1.51  desc 0.0088/1.23  desc_rows 0.0022/2.00
  OMNI_SPLIT_WINO=15    conv1b 0.0015/1.95  conv2a 0.0025/2.14  conv2b 0.0021/1.70  conv3a 0.0031/2.10  conv3b 0.0005/1.96  conv4a 0.0008/2.23
                        conv4b 0.0007/2.23  heads 0.0008/2.66  semi 0.0033/1.86  desc 0.0074/1.21  desc_rows 0.0020/1.90
  OMNI_SPLIT_FUSE1A=0   conv1a 0.3280/1.00  conv1b 0.0022/2.05  conv2a 0.0026/1.80  conv2b 0.0026/1.48  conv3a 0.0021/1.77  conv3b 0.0005/2.04
                        conv4a 0.0006/1.92  conv4b 0.0007/2.00  heads 0.0007/2.18  semi 0.0029/1.44  desc 0.0056/1.21  desc_rows 0.0018/2.02
  OMNI_DET16=0          conv1b 0.0016/1.95  conv2a 0.0026/1.81  conv2b 0.0025/1.54  conv3a 0.0021/2.57  conv3b 0.0005/1.92  conv4a 0.0006/1.87
                        conv4b 0.0007/1.94  heads 0.0007/2.49  semi 0.0067/1.01  desc 0.0066/1.20  desc_rows 0.0019/1.98
  split 480x600         conv1b 0.0015/1.96  conv2a 0.0021/2.41  conv2b 0.0024/2.13  conv3a 0.0024/3.58  conv3b 0.0007/2.43  conv4a 0.0010/2.02
                        conv4b 0.0007/2.17  heads 0.0009/2.85  semi 0.0035/1.40  desc 0.0088/1.22  desc_rows 0.0018/1.59
  f32                   conv1a 0.3479/1.17  conv1b 0.0076/1.49  conv2a 0.0089/1.11  conv2b 0.0108/1.21  conv3a 0.0101/1.24  conv3b 0.0029/1.14
                        conv4a 0.0036/1.27  conv4b 0.0033/1.14  heads 0.0037/1.24  semi 0.0065/1.02  desc 0.0070/1.23  desc_rows 0.0070/1.33
  f32 480x600           conv1a 0.4174/1.17  conv1b 0.0082/1.07  conv2a 0.0083/1.03  conv2b 0.0084/1.15  conv3a 0.0092/1.06  conv3b 0.0033/1.11
                        conv4a 0.0048/1.13  conv4b 0.0039/1.05  heads 0.0045/1.06  semi 0.0061/1.07  desc 0.0066/1.22  desc_rows 0.0061/1.13
  split sequence        conv1b 0.0016/2.00  conv2a 0.0024/2.20  conv2b 0.0030/1.73  conv3a 0.0025/3.20  conv3b 0.0006/2.25  conv4a 0.0010/2.30
                        conv4b 0.0007/2.78  heads 0.0010/2.75  semi 0.0036/1.42  desc 0.0086/1.11  desc_rows 0.0021/1.68
  split unaligned       conv1a 0.3197/1.00  conv1b 0.0021/1.52  conv2a 0.0016/1.45  conv2b 0.0025/1.23  conv3a 0.0019/1.57  conv3b 0.0005/1.72
                        conv4a 0.0005/1.74  conv4b 0.0005/2.01  heads 0.0006/2.28  semi 0.0027/1.77  desc 0.0072/1.19  desc_rows 0.0020/1.85
Largest clean tier-2 ratio per kernel form (c is twice it): direct 3.585 (conv3a, 480 x 600), direct behind the fused conv1a 1.928, Winograd 2.508 (conv2a,
OMNI_SPLIT_WINO=10), Winograd behind the fused conv1a 2.002 (sequence), the separate conv1a 1.000, exact-f32 1.487, semi 2.120 (split head) / 1.070 (exact-f32 head),
desc and the exact-f32 desc_rows 1.327, the split convDb's desc_rows 2.306.
Tier 1 sits at 0.0005 - 0.01 of its allowance for the convolutions and the tails (a worst-case gamma_K over K = 769 .. 3458 terms against errors that grow like
sqrt(K)) and at 0.33 - 0.42 for the separate conv1a (K = 10); tier 2 is what sees a subtle defect.  The clean tier-2 ratios of the fp16 matrix-core kernels are
1.4 - 3.6 in the worst slice and 1.13 - 1.48 over a whole layer: their accumulation is a little noisier than one rounding per 16-term dot, with a mean error of
-0.05 of its RMS; the exact-f32 kernels follow the emulation (1.0 - 1.5 in the worst slice).  The lo-half bias of the clean kernels: |B| <= 0.0153 (at most 0.49
of its limit).
"""
import numpy as np
import pytest

from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import f16_layer_ref as R16
from tests import split_layer_ref as R
from tests.test_gpu_f16_layers import _dev_pass, _images

pytestmark = pytest.mark.gpu

DEFAULTS = ("OMNI_CONV_V1", "OMNI_SP_SPARSE_DESC", "OMNI_SP_SPARSE_DA", "OMNI_SP_MASK_SKIP", "OMNI_SP_MASK_SKIP_SPLIT", "OMNI_SP_SPLIT_DB", "OMNI_DET16",
            "OMNI_SPLIT_FUSE1A", "OMNI_SPLIT_WINO", "OMNI_SPLIT_TRN", "OMNI_SP_MASK_RECT")
# (H, W, batch, fisheye mask)
SMALL = [(64, 96, 1, False), (72, 104, 1, False), (104, 136, 1, False), (128, 264, 1, True), (208, 400, 3, True)]


@pytest.fixture
def production(monkeypatch):
    for k in DEFAULTS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def cdiv(a, b):
    return -(-a // b)


def split_c128_transposed(hc, wc):
    """csrc/conv_split.hip split_c128_transposed: the unpooled cin = 128 layers run on transposed 2 x 32 tiles when that needs fewer tiles."""
    return cdiv(hc, 32) * cdiv(wc, 2) < cdiv(wc, 32) * cdiv(hc, 2)


def wino_layers(requested, h, w, fuse1a):
    """csrc/sp_plan.h sp_wino_layers."""
    m = requested
    if h % 8 or w % 8:
        m &= 7
    if h % 4 or w % 4:
        m &= 1
    if h % 2 or w % 2 or not fuse1a:
        m &= ~1
    return m


def split_plan(h, w, wino_req=7, fuse1a=True):
    """The layers of a PREC_SPLIT pass as csrc/sp_plan.h plans them: (name, input layer, kind, pool, output form, (tile rows, tile columns, transposed))."""
    m = wino_layers(wino_req, h, w, fuse1a)
    wn = [bool(m & 1), bool(m & 2), bool(m & 4), bool(m & 8)]
    names, pools = ["conv1b", "conv2a", "conv2b", "conv3a"], [True, False, True, False]
    plan = []
    for i, n in enumerate(names):
        nxt_wino = i < 3 and wn[i + 1]
        out = ("raw32" if nxt_wino else "split") if wn[i] else "split"
        plan.append((n, "conv1a" if i == 0 else names[i - 1], "wino" if wn[i] else "direct", pools[i], out, (4, 32, False)))
    trn = split_c128_transposed(h // 8, w // 8)
    plan.append(("conv3b", "conv3a", "direct", True, "split", (2, 32, False)))
    plan.append(("conv4a", "conv3b", "direct", False, "split", (2, 32, trn)))
    plan.append(("conv4b", "conv4a", "direct", False, "split", (2, 32, trn)))
    plan.append(("heads", "conv4b", "direct", False, "f32", (2, 32, trn)))
    return plan


class Gate:
    """Collects every layer's verdicts of a test, so that one run reports all failing layers (with the worst element and slice) at once."""

    def __init__(self):
        self.stats, self.kinds, self.failures = {}, {}, []

    def add(self, tag, layer, kind, t1, t2, lb=None):
        self.kinds[kind] = max(self.kinds.get(kind, 0.0), t2["ratio"])
        s = self.stats.setdefault(layer, {"t1": 0.0, "t2": 0.0, "B": 0.0, "n": 0})
        s["t1"], s["t2"], s["n"] = max(s["t1"], t1["ratio"]), max(s["t2"], t2["ratio"]), s["n"] + 1
        if lb is not None:
            s["B"] = max(s["B"], abs(lb["B"]) / lb["limit"])
        if not t1["ok"]:
            self.failures.append(f"{tag} {layer} tier 1: {t1}")
        if not t2["ratio"] <= R.TIER2_C[kind]:
            self.failures.append(f"{tag} {layer} tier 2 (c = {R.TIER2_C[kind]}): {t2}")
        if lb is not None and not lb["ok"]:
            self.failures.append(f"{tag} {layer} lo bias: {lb}")

    def finish(self, name):
        for layer, s in self.stats.items():
            print(f"MEASURED {name} {layer}: worst tier-1 ratio {s['t1']:.4f}, worst tier-2 ratio {s['t2']:.3f}, lo bias / limit {s['B']:.2f} ({s['n']} images)")
        print(f"MEASURED {name} worst tier-2 ratio per kernel form: " + ", ".join(f"{k} {v:.3f} (c = {R.TIER2_C[k]})" for k, v in self.kinds.items()))
        assert not self.failures, "\n".join(self.failures)


def _gate_layer(gate, tag, name, kind, got, ref, emul, tiles, pool, out):
    th, tw, trn = tiles
    t1 = R.tier1(got, ref)
    t2 = R.tier2(got, emul, ref, th, tw, pool, trn)
    gate.add(tag, name, kind, t1, t2, R.lo_bias(got, emul, ref) if out == "split" else None)


def _cells4(a, r):
    """[R, 256, 1, 1] rows -> [1, 256, R, 1]: channel and row slices for ``tier2`` (32 rows are one tile of convdb_l2norm_split_kernel)."""
    return np.asarray(a).reshape(r, 256).T.reshape(1, 256, r, 1)


def gate_tails(sp, weights, heads, gate, tag, det16, n_kps, split_db):
    """From the stored fp32 ``heads``: the heat map (detector_head_mfma16_kernel<float>, or the exact-f32 head) and the dense descriptors (exact-f32 convDb +
    l2norm_kernel); from the pass's own compact cDa rows (``desc_rows_in``): the rows the sparse descriptor tail made of them (``desc_rows_out``:
    convdb_l2norm_split_kernel under PREC_SPLIT, the exact-f32 convolution + l2norm_kernel under PREC_F32).  Both tiers each."""
    nb = len(heads)
    rows_in, rows_out = sp.debug_layer("desc_rows_in", nb), sp.debug_layer("desc_rows_out", nb)      # before get_dense: the pass's own rows
    assert rows_in.shape[1] % 32 == 0                                                                  # every image's rows start a 32-row tile
    semi, desc = sp.get_dense(nb)
    wP, bP, wD, bD = weights["convPb.weight"], weights["convPb.bias"], weights["convDb.weight"], weights["convDb.bias"]
    for b in range(nb):
        t = f"{tag}[{b}]"
        cpa, cda = heads[b:b + 1, :256], heads[b:b + 1, 256:]
        y, E = R16.semi_ref(cpa, wP, bP, x_f32=det16, exact_f32=not det16)
        ref = R.Ref(R.semi_cells(y), R.semi_cells(E))
        got, emul = R.semi_cells(semi[b:b + 1]), R.semi_cells(R.semi_emul(cpa, wP, bP, exact_f32=not det16))
        gate.add(t, "semi", "semi" if det16 else "semi_f32", R.tier1(got, ref), R.tier2(got, emul, ref, 1, 32, False))
        y, E = R16.desc_ref(cda, wD, bD, round_w=False)
        ref = R.Ref(y, E)
        gate.add(t, "desc", "desc", R.tier1(desc[b:b + 1], ref), R.tier2(desc[b:b + 1], R.desc_emul(cda, wD, bD), ref, 8, 32, False))
        r = 4 * n_kps[b]
        if r == 0:
            continue
        x = rows_in[b, :r].reshape(r, 256, 1, 1)
        y, E = R16.desc_ref(x, wD, bD, round_w=False, split=split_db)
        ref = R.Ref(_cells4(y, r), _cells4(E, r))
        emul = R.convdb_split_emul(x, wD, bD) if split_db else R.desc_emul(x, wD, bD)
        got = _cells4(rows_out[b, :r], r)
        gate.add(t, "desc_rows", "desc_rows_split" if split_db else "desc", R.tier1(got, ref), R.tier2(got, _cells4(emul, r), ref, 32, 1, False))


def gate_split_pass(sp, weights, imgs, mask, gate, tag, res, wino_req=7, fuse1a=True, aligned=True, det16=True):
    """Gate every convolution layer of the LAST pass of ``sp`` (PREC_SPLIT over ``imgs``)."""
    nb, h, w = imgs.shape
    fused = fuse1a and aligned
    plan = split_plan(h, w, wino_req, fused)
    # the restated plan is the library's own: Winograd layers (bits 1, 2, 4, 8), the fused conv1a (16), the split detector head (32), the split convDb over compact rows (64, 128)
    want = sum(1 << i for i, p in enumerate(plan[:4]) if p[2] == "wino") | (16 if fused else 0) | (32 if det16 else 0) | 64 | 128
    assert sp.last_plan() == want, (tag, sp.last_plan(), want)
    got = {n: sp.debug_layer(n, nb) for n in ([] if fused else ["conv1a"]) + [p[0] for p in plan]}
    wt = lambda n: weights[n + ".weight"]
    bs = lambda n: weights[n + ".bias"]
    for b in range(nb):
        t = f"{tag}[{b}]"
        g = R.masked_u8(imgs[b:b + 1], mask)
        if not fused:
            _gate_layer(gate, t, "conv1a", "conv1a", got["conv1a"][b:b + 1], R.conv1a_split_ref(g, wt("conv1a"), bs("conv1a")),
                        R.conv1a_split_emul(g, wt("conv1a"), bs("conv1a")), (8, 32, False), False, "split")
        for (n, prev, kind, pool, out, tiles) in plan:
            if n == "heads":
                wn, bn = np.concatenate([wt("convPa"), wt("convDa")]), np.concatenate([bs("convPa"), bs("convDa")])
            else:
                wn, bn = wt(n), bs(n)
            u_in = None
            if n == "conv1b" and fused:
                x, u_in = R.conv1a_fused_input(g, wt("conv1a"), bs("conv1a"), split_store=kind == "direct")
                xe = R.conv1a_fused_emul(g, wt("conv1a"), bs("conv1a"), split_store=kind == "direct")
            else:
                x = xe = got[prev][b:b + 1]
            if kind == "wino":
                ref = R.wino_ref(x, wn, bn, pool=pool, out_split=out == "split", u_in=u_in)
                emul = R.wino_emul(xe, wn, bn, pool=pool, out_split=out == "split")
            else:
                ref = R.direct_ref(x, wn, bn, pool=pool, out_f32=out == "f32", u_in=u_in)
                emul = R.direct_emul(xe, wn, bn, pool=pool, out_f32=out == "f32")
            _gate_layer(gate, t, n, kind + ("_fused1a" if u_in is not None else ""), got[n][b:b + 1], ref, emul, tiles, pool, out)
    gate_tails(sp, weights, got["heads"], gate, tag, det16, [len(r[0]) for r in res], split_db=True)
    return got


F32_CHAIN = [("conv1b", "conv1a", True), ("conv2a", "conv1b", False), ("conv2b", "conv2a", True), ("conv3a", "conv2b", False), ("conv3b", "conv3a", True),
             ("conv4a", "conv3b", False), ("conv4b", "conv4a", False), ("heads", "conv4b", False)]


def _f32_layer(gate, t, name, got, x, wn, bn, pool, band):
    """One exact-f32 layer: tier 1 over the whole map; tier 2 over the whole map, or (``band``) over a band of eight output rows from a multiple of eight in the
    middle of the map -- every channel, every row class and every column class of the 8 x 32 tiles, the float32 chain emulated for those rows alone (a row's
    chain does not depend on the others: the band is emulated from its own input rows plus one output row's worth on either side, which is then dropped)."""
    ref = R.f32_ref(x, wn, bn, pool=pool)
    t1 = R.tier1(got, ref)
    ho = got.shape[2]
    if not band or ho <= 8:
        t2 = R.tier2(got, R.f32_emul(x, wn, bn, pool=pool), ref, 8, 32, pool)
    else:
        f = 2 if pool else 1
        o0 = ho // 2 // 8 * 8
        o1 = min(o0 + 8, ho)
        a, b = max(o0 - 1, 0), min(o1 + 1, ho)
        emul = R.f32_emul(x[:, :, f * a: f * b], wn, bn, pool=pool)[:, :, o0 - a: o1 - a]
        t2 = R.tier2(got[:, :, o0:o1], emul, R.Ref(ref.y[:, :, o0:o1], ref.E[:, :, o0:o1]), 8, 32, pool)
    gate.add(t, name, "f32", t1, t2)


def gate_f32_pass(sp, weights, imgs, mask, gate, tag, res, band=False):
    """PREC_F32: conv1a_kernel<float> and conv_mfma_kernel<float> (8 x 32 tiles)."""
    nb = len(imgs)
    assert sp.last_plan() == 128, sp.last_plan()            # no Winograd, no fusion, the exact-f32 head, compact rows through the exact-f32 convDb
    got = {n: sp.debug_layer(n, nb) for n in ["conv1a"] + [c[0] for c in F32_CHAIN]}
    wt = lambda n: weights[n + ".weight"]
    bs = lambda n: weights[n + ".bias"]
    for b in range(nb):
        t = f"{tag}[{b}]"
        x0 = R.x_oracle(R.masked_u8(imgs[b:b + 1], mask))[:, None]
        _f32_layer(gate, t, "conv1a", got["conv1a"][b:b + 1], x0, wt("conv1a"), bs("conv1a"), False, band)
        for (n, prev, pool) in F32_CHAIN:
            if n == "heads":
                wn, bn = np.concatenate([wt("convPa"), wt("convDa")]), np.concatenate([bs("convPa"), bs("convDa")])
            else:
                wn, bn = wt(n), bs(n)
            _f32_layer(gate, t, n, got[n][b:b + 1], got[prev][b:b + 1], wn, bn, pool, band)
    gate_tails(sp, weights, got["heads"], gate, tag, False, [len(r[0]) for r in res], split_db=False)
    return got


def test_shapes_cover_both_tile_orientations_and_every_kernel_form():
    """The small shapes reach the cin = 128 kernel's plain tiles (64 x 96 .. 128 x 264) and its transposed ones (208 x 400); the full frame is transposed.
    The OMNI_SPLIT_WINO values of the tests reach both kernels of every cin = 64 layer and both output forms of the Winograd kernel."""
    assert {split_c128_transposed(h // 8, w // 8) for h, w, _, _ in SMALL} == {True, False}
    assert split_c128_transposed(60, 75) and split_c128_transposed(26, 50) and not split_c128_transposed(16, 33) and not split_c128_transposed(13, 17)
    forms = set()
    for req in (7, 0, 8, 10, 15):
        forms |= {(n, kind, out) for (n, _, kind, _, out, _) in split_plan(208, 400, req) if n in ("conv1b", "conv2a", "conv2b", "conv3a")}
    for n in ("conv2a", "conv2b", "conv3a"):
        assert (n, "direct", "split") in forms and (n, "wino", "split") in forms, n
    assert ("conv1b", "direct", "split") in forms and ("conv1b", "wino", "raw32") in forms and ("conv2a", "wino", "raw32") in forms and ("conv2b", "wino", "raw32") in forms
    assert wino_layers(15, 72, 100, True) == 7 and wino_layers(15, 72, 104, True) == 15 and wino_layers(7, 72, 104, False) == 6


def _split_handle(omni, ctx, weights, h, w, nb):
    comp, mean = synth.pca()
    return omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, omni.capi.PREC_SPLIT, nb)


def _run_split(omni, ctx, production, shapes, name, wino_req=7, fuse1a=True, env=(), det16=True):
    for k, v in env:
        production.setenv(k, v)
    weights = S.synth_weights(0)
    gate = Gate()
    for (h, w, nb, mask) in shapes:
        imgs = _images(h, w, nb, 1500 + h)
        sp = _split_handle(omni, ctx, weights, h, w, nb)
        res = sp.inference(imgs, fisheye_mask=mask)
        gate_split_pass(sp, weights, imgs, mask, gate, f"{h}x{w}{' mask' if mask else ''}", res, wino_req, fuse1a, det16=det16)
        sp.close()
    gate.finish(name)


def test_split_defaults_every_layer_meets_both_tiers(omni, ctx, production):
    _run_split(omni, ctx, production, SMALL, "split defaults")


@pytest.mark.parametrize("wino", [0, 8, 10, 15])
def test_split_winograd_subsets_every_layer_meets_both_tiers(omni, ctx, production, wino):
    _run_split(omni, ctx, production, [(72, 104, 1, False), (104, 136, 1, False), (208, 400, 1, True)], f"OMNI_SPLIT_WINO={wino}", wino_req=wino,
               env=(("OMNI_SPLIT_WINO", str(wino)),))


def test_split_unfused_conv1a_every_layer_meets_both_tiers(omni, ctx, production):
    _run_split(omni, ctx, production, [(72, 104, 1, False), (128, 264, 1, True)], "OMNI_SPLIT_FUSE1A=0", fuse1a=False, env=(("OMNI_SPLIT_FUSE1A", "0"),))


def test_split_exact_f32_detector_head_meets_its_bound(omni, ctx, production):
    _run_split(omni, ctx, production, [(72, 104, 1, False), (128, 264, 1, True)], "OMNI_DET16=0", env=(("OMNI_DET16", "0"),), det16=False)


def test_split_full_frame_every_layer_meets_both_tiers(omni, ctx, production):
    _run_split(omni, ctx, production, [(480, 600, 1, True)], "split 480x600")


def _run_f32(omni, ctx, shapes, name, band=False):
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    gate = Gate()
    for (h, w, nb, mask) in shapes:
        imgs = _images(h, w, nb, 1600 + h)
        sp = omni.capi.SuperPoint(ctx, weights, comp, mean, w, h, 0.015, 200, omni.capi.PREC_F32, nb)
        res = sp.inference(imgs, fisheye_mask=mask)
        gate_f32_pass(sp, weights, imgs, mask, gate, f"{h}x{w}", res, band)
        sp.close()
    gate.finish(name)


def test_f32_every_layer_meets_both_tiers(omni, ctx, production):
    _run_f32(omni, ctx, [(72, 104, 1, False), (104, 136, 1, True)], "f32")


def test_f32_full_frame_every_layer_meets_both_tiers(omni, ctx, production):
    """480 x 600 masked: tier 1 on every element, tier 2 on a band of rows per layer (``_f32_layer``)."""
    _run_f32(omni, ctx, [(480, 600, 1, True)], "f32 480x600", band=True)


def test_split_mask_skip_sequence_on_one_handle_meets_both_tiers(omni, ctx, production):
    """A masked pass, an unmasked pass (it overwrites the mask-skip rectangles), then a masked pass of a larger batch (calibrates again)."""
    weights = S.synth_weights(0)
    h, w = 208, 400
    sp = _split_handle(omni, ctx, weights, h, w, 2)
    gate = Gate()
    for i, (nb, mask) in enumerate(((1, True), (1, False), (2, True))):
        imgs = _images(h, w, nb, 1700 + 10 * i)
        res = sp.inference(imgs, fisheye_mask=mask)
        gate_split_pass(sp, weights, imgs, mask, gate, f"pass{i}", res)
    sp.close()
    gate.finish("split sequence")


def test_split_unaligned_image_meets_both_tiers(omni, ctx, production):
    """An image the fused conv1a cannot read 4 bytes at a time: conv1a_split runs on its own and the Winograd conv1b is off for the pass."""
    weights = S.synth_weights(0)
    h, w, nb = 72, 104, 1
    imgs = _images(h, w, nb, 1800)
    sp = _split_handle(omni, ctx, weights, h, w, nb)
    res = _dev_pass(ctx, sp, imgs, "offset", False)
    gate = Gate()
    gate_split_pass(sp, weights, imgs, False, gate, "72x104 offset", res, aligned=False)
    sp.close()
    gate.finish("split unaligned")
