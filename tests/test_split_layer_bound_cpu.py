"""The per-layer gates of tests/split_layer_ref.py for the fp32-class SuperPoint layers have teeth, and their restated constants are the
library's (no GPU).

The clean float32 emulation of a layer passes both tiers (and the lo-half bias gate of split-64 outputs).  Then one defect at a time, each of a kind
these kernels can have, must fail:
  direct split kernels      drop_xl_wh            xl wh dropped in one (tap, 16-channel k-group)
                            drop_xh_wl_wave       xh wl dropped for one wave's 32 output channels
                            lo_rtz                lo halves rounded toward zero (split-64 outputs: caught by the lo-half bias gate; see below)
                            partner_col31         cin = 128: the partner wave's partial sum taken from the neighbouring pixel in column 31 of each tile
                            inv_x2_group          the weight scale's inverse off by a factor 2 for one 64-channel group
                            pool_shift_last_row   the pool window shifted up by one pixel on the last pooled row
                            neighbour_bias        one channel using its neighbour's bias
  Winograd kernels          ul_missing_pos        Ul missing at one position (i, j)
                            v_split_before_hadd   V split before the horizontal add (the halves combined in fp16)
                            at_sign_flip_odd_col  one row of A^T with its sign flipped for odd tile columns
                            lo_rtz, pool_shift_last_row, neighbour_bias
  exact-f32 path            kstep_fp16            one k-step accumulated in fp16;  pool_shift_last_row, neighbour_bias
  split detector head,      drop_xl_wh            xl wh dropped in one k-step of 16 channels (tier 1 passes it: 0.4 - 0.6 of the bound; tier 2: 348 and 853)
  split convDb              wl_wrong_kstep        one k-step multiplied with the wl fragment of the next one (tier 2: 605 and 1680)
  exact-f32 detector head   kstep_fp16
  a nearly dead channel     drop_xh_wl_channel40  xh wl dropped for one output channel that the ReLU leaves live at 3 % of its elements: tier 2's floor on a slice's
                                                  denominator (a quarter of the average slice) holds that channel to the layer's noise, and the defect still shows 436
Sizes: (20, 40) and (12, 72) for the direct and exact-f32 layers, (16, 40) and (12, 68) for Winograd (even maps, overhanging tiles).

For each defect the verdict of the EXISTING max-norm gate, |got - ref| < 2e-5 max(1, max |ref|) against the float64 convolution with the weights as given,
is recorded too (printed with -s).  At activations of magnitude 0.01 -- the "small activations" where that gate's absolute floor leaves the most room --
drop_xl_wh, drop_xh_wl_wave, lo_rtz and ul_missing_pos pass it: the gap the new gates close.  At magnitude 1.5 the first two and ul_missing_pos reach its
floor (errors of 1e-4 .. 4e-4 against 6e-5 .. 9e-5); lo_rtz passes it at every magnitude.

lo_rtz and the RMS ratio.  Rounding the lo half of a stored output toward zero doubles a 2^-23-relative error that sits below the 3e-7-relative
accumulation noise: the tier-2 ratio moves from 1.0 to 1.2 - 1.5, inside any c >= 2 x 1.0.  No c separates it, so the lo-half bias gate
(split_layer_ref.lo_bias: the error's covariance with the sign of the ideal lo half; clean |B| <= 0.02, rounded toward zero B = -0.10 .. -0.17 against a
limit of 0.03 .. 0.06: six sigma, and at least twice the clean kernels' 0.0153 on the MI355X) catches it for split-64 outputs.  A raw-32 or fp32 output has no lo half of its own: there lo_rtz only touches the
packed weights (pinned index by index below) and the Winograd kernel's Vl, whose ratio of 1.5 against c stays unseparated -- reported, not gated.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import split_layer_ref as R

# name: (kind, cin, cout, pool, output form, tile rows, shapes)
DIRECT_SHAPES, WINO_SHAPES = [(20, 40), (12, 72)], [(16, 40), (12, 68)]
LAYERS = {
    "direct_c64_pool": ("direct", 64, 64, True, "split", 4, DIRECT_SHAPES),          # conv1b / conv2b
    "direct_c64_n128": ("direct", 64, 128, False, "split", 4, DIRECT_SHAPES),        # conv3a: two 64-channel groups
    "direct_c128": ("direct", 128, 128, False, "split", 2, DIRECT_SHAPES),           # conv4a / conv4b
    "direct_c128_pool": ("direct", 128, 128, True, "split", 2, DIRECT_SHAPES),       # conv3b
    "direct_c128_f32": ("direct", 128, 128, False, "f32", 2, DIRECT_SHAPES),         # the heads layer
    "wino_pool_raw32": ("wino", 64, 64, True, "raw32", 4, WINO_SHAPES),              # conv1b / conv2b in front of a Winograd layer
    "wino_split": ("wino", 64, 64, False, "split", 4, WINO_SHAPES),                  # conv2a / conv3a in front of a direct layer
    "f32_c64_pool": ("f32", 64, 64, True, "f32", 8, DIRECT_SHAPES),
    "f32_c128": ("f32", 128, 128, False, "f32", 8, DIRECT_SHAPES),
}
DEFECTS = {"direct": ["drop_xl_wh", "drop_xh_wl_wave", "lo_rtz", "partner_col31", "inv_x2_group", "pool_shift_last_row", "neighbour_bias"],
           "wino": ["ul_missing_pos", "v_split_before_hadd", "at_sign_flip_odd_col", "lo_rtz", "pool_shift_last_row", "neighbour_bias"],
           "f32": ["kstep_fp16", "pool_shift_last_row", "neighbour_bias"]}
PASS_THE_OLD_GATE = ("drop_xl_wh", "drop_xh_wl_wave", "lo_rtz", "ul_missing_pos")
SCALES = (1.5, 0.01)


def _layer(cin, cout, h, w, seed, scale):
    rng = np.random.default_rng(seed)
    x = R.store_split((np.maximum(rng.standard_normal((1, cin, h, w)), 0.0) * scale * R.ACT).astype(np.float32))      # a stored split-64 activation
    wt = ((rng.random((cout, cin, 3, 3)) * 2 - 1) * np.sqrt(6.0 / (9 * cin))).astype(np.float32)
    b = ((rng.random(cout) * 2 - 1) * 0.05 * scale).astype(np.float32)
    return x, wt, b


def _true(x, wt, b, pool):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    y = F.relu(F.conv2d(t(x), t(wt), t(b), padding=1))
    return (F.max_pool2d(y, 2, 2) if pool else y).numpy()


def _run(kind, x, wt, b, pool, out, defect=None):
    if kind == "direct":
        return R.direct_emul(x, wt, b, pool=pool, out_f32=out == "f32", defect=defect)
    if kind == "wino":
        return R.wino_emul(x, wt, b, pool=pool, out_split=out == "split", defect=defect)
    return R.f32_emul(x, wt, b, pool=pool, defect=defect)


def _ref(kind, x, wt, b, pool, out):
    if kind == "direct":
        return R.direct_ref(x, wt, b, pool=pool, out_f32=out == "f32")
    if kind == "wino":
        return R.wino_ref(x, wt, b, pool=pool, out_split=out == "split")
    return R.f32_ref(x, wt, b, pool=pool)


def _verdict(kind, got, clean, ref, th, pool, out):
    t1, t2 = R.tier1(got, ref), R.tier2(got, clean, ref, th, 32, pool)
    lb = R.lo_bias(got, clean, ref) if out == "split" else None
    ok = t1["ok"] and t2["ratio"] <= R.TIER2_C[kind] and (lb is None or lb["ok"])
    return ok, t1, t2, lb


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_clean_emulation_passes_and_every_defect_fails(name, scale):
    kind, cin, cout, pool, out, th, shapes = LAYERS[name]
    for (h, w) in shapes:
        x, wt, b = _layer(cin, cout, h, w, cin + h, scale)
        ref, yt = _ref(kind, x, wt, b, pool, out), _true(x, wt, b, pool)
        assert ref.exact_in                                                         # hi is recovered from hi + lo: xl is a half again
        clean = _run(kind, x, wt, b, pool, out)
        ok, t1, t2, lb = _verdict(kind, clean, clean, ref, th, pool, out)
        assert ok and t1["violations"] == 0 and t1["ratio"] < 0.05, (name, h, w, t1, t2, lb)      # worst-case K against sqrt(K) errors
        assert R.old_gate(clean, yt)
        for d in DEFECTS[kind]:
            if (d == "partner_col31" and cin != 128) or (d == "pool_shift_last_row" and not pool):
                continue
            if d == "lo_rtz" and out != "split":                                   # no lo half of its own: see the module docstring
                continue
            got = _run(kind, x, wt, b, pool, out, d)
            ok, t1, t2, lb = _verdict(kind, got, clean, ref, th, pool, out)
            old = R.old_gate(got, yt)
            print(f"DEFECT {name} {h}x{w} scale {scale} {d}: tier 1 {t1['ratio']:.3g} ({t1['violations']} violations), tier 2 {t2['ratio']:.3g} at {t2['where']}, "
                  f"lo bias {lb['B'] / lb['limit'] if lb else 0:.2f} of its limit; the old max-norm gate {'passes' if old else 'fails'} it")
            assert not ok, (name, h, w, d, t1, t2, lb)
            if d != "lo_rtz":
                assert t2["ratio"] > 10 * max(R.TIER2_C.values()), (name, d, t2)   # every c in use stays far below what a defect shows
            if scale == min(SCALES) and d in PASS_THE_OLD_GATE:
                assert old, (name, h, w, d)


def test_a_defect_confined_to_a_nearly_dead_channel_fails_tier2():
    """tier2 floors a slice's denominator at a quarter of the average slice (channels dead behind the ReLU): a channel live at a few per cent of its
    elements is then held to the layer's noise, and a defect that touches only that channel -- xh wl dropped for it -- still fails by a wide margin."""
    x, wt, b = _layer(64, 64, 20, 72, 5, 1.5)
    b[40] = -1.0
    for _ in range(6):
        clean = R.direct_emul(x, wt, b, pool=True)
        live = float((clean[0, 40] > 0).mean())
        if 0.0 < live < 0.05:
            break
        b[40] *= 1.3 if live >= 0.05 else 0.85
    assert 0.0 < live < 0.05, live
    ref = R.direct_ref(x, wt, b, pool=True)
    ok, t1, t2, lb = _verdict("direct", clean, clean, ref, 4, True, "split")
    assert ok, (t1, t2, lb)
    got = R.direct_emul(x, wt, b, pool=True, defect="drop_xh_wl_channel40")
    ok, t1, t2, lb = _verdict("direct", got, clean, ref, 4, True, "split")
    print(f"DEFECT quiet channel (live at {live:.3f} of its elements): tier 2 {t2['ratio']:.3g} at {t2['where']}")
    assert not ok and t2["where"] == ("channel", 40) and t2["ratio"] > 10 * max(R.TIER2_C.values()), (t1, t2)


def _tail_inputs(cells_h, cells_w, seed):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((1, 256, cells_h, cells_w)), 0.0).astype(np.float32)
    wP = ((rng.random((65, 256, 1, 1)) * 2 - 1) * np.sqrt(6.0 / 256)).astype(np.float32)
    wD = ((rng.random((256, 256, 1, 1)) * 2 - 1) * np.sqrt(6.0 / 256)).astype(np.float32)
    return x, wP, ((rng.random(65) * 2 - 1) * 0.05).astype(np.float32), wD, ((rng.random(256) * 2 - 1) * 0.05).astype(np.float32)


def _tail_verdict(kind, got, clean, ref, th, tw):
    t1, t2 = R.tier1(got, ref), R.tier2(got, clean, ref, th, tw, False)
    return t1["ok"] and t2["ratio"] <= R.TIER2_C[kind], t1, t2


@pytest.mark.parametrize("exact_f32", [False, True])
def test_detector_head_emulation_passes_and_its_defects_fail(exact_f32):
    """The heat map of 7 x 11 cells (three fragments of 32 cells, the last ragged): the split head with xl wh dropped in one k-step or the wl fragment of the
    neighbouring k-step; the exact-f32 head with one step accumulated in fp16.  The old gate is the max-norm against the float64 softmax."""
    from tests import f16_layer_ref as R16
    x, wP, bP, _, _ = _tail_inputs(7, 11, 21)
    y, E = R16.semi_ref(x, wP, bP, x_f32=not exact_f32, exact_f32=exact_f32)
    ref = R.Ref(R.semi_cells(y), R.semi_cells(E))
    kind = "semi_f32" if exact_f32 else "semi"
    clean = R.semi_cells(R.semi_emul(x, wP, bP, exact_f32=exact_f32))
    ok, t1, t2 = _tail_verdict(kind, clean, clean, ref, 1, 32)
    assert ok and t1["ratio"] < 0.05, (t1, t2)
    for d in (["kstep_fp16"] if exact_f32 else ["drop_xl_wh", "wl_wrong_kstep"]):
        got = R.semi_cells(R.semi_emul(x, wP, bP, exact_f32=exact_f32, defect=d))
        ok, t1, t2 = _tail_verdict(kind, got, clean, ref, 1, 32)
        old = R.old_gate(got, ref.y)
        print(f"DEFECT {kind} {d}: tier 1 {t1['ratio']:.3g}, tier 2 {t2['ratio']:.3g} at {t2['where']}; the old max-norm gate {'passes' if old else 'fails'} it")
        assert not ok and t2["ratio"] > 10 * max(R.TIER2_C.values()), (d, t1, t2)
        if not exact_f32:
            assert t1["ok"], (d, t1)                        # far inside the derived bound: only tier 2 sees it


def test_split_convdb_emulation_passes_and_its_defects_fail():
    """convdb_l2norm_split over 72 compact rows (three tiles of 32, the last ragged)."""
    from tests import f16_layer_ref as R16
    x, _, _, wD, bD = _tail_inputs(72, 1, 22)
    rows = x.transpose(2, 1, 0, 3).copy()                   # [72, 256, 1, 1]
    to4 = lambda a: np.asarray(a).reshape(72, 256).T.reshape(1, 256, 72, 1)
    y, E = R16.desc_ref(rows, wD, bD, round_w=False, split=True)
    ref = R.Ref(to4(y), to4(E))
    clean = to4(R.convdb_split_emul(rows, wD, bD))
    ok, t1, t2 = _tail_verdict("desc_rows_split", clean, clean, ref, 32, 1)
    assert ok and t1["ratio"] < 0.05, (t1, t2)
    yt, _ = R16.desc_ref(rows, wD, bD, round_w=False)
    for d in ("drop_xl_wh", "wl_wrong_kstep"):
        got = to4(R.convdb_split_emul(rows, wD, bD, defect=d))
        ok, t1, t2 = _tail_verdict("desc_rows_split", got, clean, ref, 32, 1)
        old = R.old_gate(got, to4(yt))
        print(f"DEFECT desc_rows_split {d}: tier 1 {t1['ratio']:.3g}, tier 2 {t2['ratio']:.3g} at {t2['where']}; the old max-norm gate {'passes' if old else 'fails'} it")
        assert not ok and t2["ratio"] > 10 * max(R.TIER2_C.values()), (d, t1, t2)
    ok, t1, t2 = _tail_verdict("desc", to4(R.desc_emul(rows, wD, bD)), to4(R.desc_emul(rows, wD, bD)), R.Ref(to4(yt), to4(R16.desc_ref(rows, wD, bD, round_w=False)[1])), 32, 1)
    assert ok, (t1, t2)


def test_tier1_compares_elements_without_terms_exactly():
    """T = 0 (an all-zero neighbourhood): the kernel's value is its bias, stored as the kernel stores it; nothing else passes."""
    x, wt, b = _layer(64, 64, 12, 40, 3, 1.0)
    x[:, :, :6] = 0.0
    ref = R.direct_ref(x, wt, b)
    clean = R.direct_emul(x, wt, b)
    assert (ref.E[:, :, :5] == 0).all() and (ref.E[:, :, 6:] > 0).all()
    assert R.tier1(clean, ref)["ok"]
    bad = clean.copy()
    c = int(np.argmax(b))
    assert clean[0, c, 2, 7] > 0
    bad[0, c, 2, 7] = np.nextafter(bad[0, c, 2, 7], np.float32(9))
    r = R.tier1(bad, ref)
    assert not r["ok"] and r["violations"] == 1 and r["where"] == (0, c, 2, 7)
    bad = clean.copy()
    bad[0, 5, 9, 9] = np.nan
    assert not R.tier1(bad, ref)["ok"]


def test_fused_conv1a_interval_covers_its_emulation():
    """The interval carried through the fused conv1b holds the float32 emulation of the two MFMAs, for both consumers' storage forms."""
    from oracle import superpoint_ref as S
    wts = S.synth_weights(0)
    w, b = wts["conv1a.weight"], wts["conv1a.bias"]
    img = np.random.default_rng(1).integers(0, 256, (1, 24, 40)).astype(np.uint8)
    img[:, 18:] = 0
    for split_store in (True, False):
        x, u = R.conv1a_fused_input(img, w, b, split_store)
        e = R.conv1a_fused_emul(img, w, b, split_store).astype(np.float64)
        assert (np.abs(e - x) <= u).all()
        assert u.max() < 1e-5 * max(1.0, x.max())


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the restated packers are the library's, index by index
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _halfs(u16):
    return u16.view(np.float16).astype(np.float64)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128), (128, 512)])
def test_direct_split_fragments_are_the_restated_halfs(omni, cin, cout):
    """conv_pack_weights_split: [g32][cb][wh | wl][tap][kg4][lane][8], cout = 32 g32 + (lane & 31), cin = 64 cb + 16 kg4 + 8 (lane >> 5) + e."""
    rng = np.random.default_rng(cin + cout)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.07).astype(np.float32)
    w[3, 5] = 0.0
    w[1, 2, 1, 1] = np.float32(2.0 ** -20)                                         # a lo half deep in fp16's subnormals
    frag, inv = omni.capi.sp_pack_constants(2, w, None, cout)
    wh, wl, inv_r = R.pack_split(w)
    assert inv == inv_r and 256 <= np.abs(w).max() / inv < 512
    f = _halfs(frag).reshape(cout // 32, cin // 64, 2, 9, 4, 64, 8)
    lane, e = np.arange(64), np.arange(8)
    for g32 in range(cout // 32):
        co = g32 * 32 + (lane & 31)
        for cb in range(cin // 64):
            for kg4 in range(4):
                ci = cb * 64 + kg4 * 16 + (lane[:, None] >> 5) * 8 + e[None, :]
                for hl, ref in ((0, wh), (1, wl)):
                    want = ref.reshape(cout, cin, 9)[co[:, None], ci]              # [lane, e, tap]
                    assert np.array_equal(f[g32, cb, hl, :, kg4], want.transpose(2, 0, 1)), (g32, cb, kg4, hl)


def test_convdb_split_fragments_are_the_restated_halfs(omni):
    """convdb_pack_weights_split: hi and lo fragments [8 waves][16 k-steps][64 lanes][8], cout = 32 wave + (lane & 31), k = 16 ks + 8 (lane >> 5) + j."""
    rng = np.random.default_rng(9)
    w = (rng.standard_normal((256, 256)) * 0.05).astype(np.float32)
    frag, scale = omni.capi.sp_pack_constants(3, w)
    assert scale == 1.0 and frag.shape == (131072,)
    f = _halfs(frag).reshape(2, 8, 16, 64, 8)
    hi, lo = R.convdb_split(w)
    lane, j = np.arange(64), np.arange(8)
    for wv in range(8):
        co = 32 * wv + (lane & 31)
        for ks in range(16):
            k = 16 * ks + 8 * (lane[:, None] >> 5) + j[None, :]
            assert np.array_equal(f[0, wv, ks], hi[co[:, None], k]) and np.array_equal(f[1, wv, ks], lo[co[:, None], k]), (wv, ks)
    assert np.abs(w - hi - lo).max() <= 2.0 ** -22 * np.abs(w).max()


def test_winograd_restatement_is_the_library_packer_bit_for_bit(omni):
    """conv_pack_weights_wino against split_layer_ref.pack_wino: the same halfs at every (position, cout, cin), the same scale."""
    rng = np.random.default_rng(11)
    for cout in (64, 128):
        g = (rng.standard_normal((cout, 64, 3, 3)) * 0.05).astype(np.float32)
        frag, inv = omni.capi.sp_pack_constants(1, g, None, cout)
        Uh, Ul, inv_r = R.pack_wino(g)
        assert inv == inv_r
        f = _halfs(frag).reshape(cout // 64, 4, 2, 4, 4, 2, 64, 8)                   # [cg][i][hl][j][kg][m][lane][e]
        lane, e = np.arange(64), np.arange(8)
        for cg in range(cout // 64):
            for i in range(4):
                for m in range(2):
                    co = cg * 64 + ((m * 32 + (lane & 31) + 16 * i) & 63)
                    for kg in range(4):
                        ci = kg * 16 + (lane[:, None] >> 5) * 8 + e[None, :]
                        for j in range(4):
                            assert np.array_equal(f[cg, i, 0, j, kg, m], Uh[i, j][co[:, None], ci]) and np.array_equal(f[cg, i, 1, j, kg, m], Ul[i, j][co[:, None], ci])
