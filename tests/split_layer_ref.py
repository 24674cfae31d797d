"""fp64 references, arithmetic error bounds and float32 emulations for the fp32-class SuperPoint layers (OMNI_PREC_SPLIT and OMNI_PREC_F32),
beside tests/f16_layer_ref.py (whose helpers are used here, not copied).

A layer's reference is the IDEAL VALUE OF THE KERNEL'S OWN ALGEBRA in float64, from the layer's stored input (``debug_layer``: split-64 frames
return hi + lo, raw-32 frames and ``heads`` are fp32 -- both exact) and the packed constants restated from the packers:

  direct split kernels (csrc/conv_split.hip conv3x3_split_kernel).  xs = 32 x (the stored activation), xh = half(xs), xl = xs - xh (a half
      again: ``Ref.exact_in``); W = w 2^k (conv_pack_weights_split: max |W| in [256, 512)), wh = half(W), wl = half(W - wh).  The kernel adds
      xh wh + xh wl + xl wh per product, which is  xs (wh + wl) - xl wl  exactly: the dropped xl wl and the weight residue W - wh - wl are IN the
      reference.  v = fmaf(sum, inv, bias'), ReLU, (the 2x2 maximum: taken before the fmaf, which is monotone), then
        split-64 output: inv = 2^-k, bias' = 32 b, hi = half(v), lo = half(v - hi): |v - hi - lo| <= max(2^-22 |v|, 2^-25)  (half an fp16 step of lo,
                         |lo| <= ulp16(v) / 2; the floor where lo is subnormal); the stored value is (hi + lo) / 32;
        fp32 output (the heads layer): inv = 2^-k / 32, bias' = b, the fmaf's result as it is.
      K.  9 taps x cin / 16 k-groups x 3 MFMAs, each adding 16 exact products to the fp32 accumulator in an order the hardware does not document:
      27 cin terms; cin = 128 adds the wave pair's two partial sums (+ 1); the fmaf (+ 1):  K = 27 cin + 2.
  Winograd kernels (csrc/conv_wino.hip).  d = 32 x as fp32; W_i = fmaf(+-1, d[rb], d[ra]) down the patch (row i of B^T), V_ij = W_a +- W_b across (one
      rounding each: bit for bit restated in ``wino_V``), Vh = half(V), Vl = half(V - Vh); U = G g G^T in double, rounded to float, x 2^k, split
      (conv_pack_weights_wino).  M_ij = sum_ci Uh Vh + Ul Vh + Uh Vl = (Uh + Ul) V - Ul Vl; the reference takes V = B^T d B exactly in float64 and Vl
      from the restated fp32 V.  T'(0) = (M0 + M1) + M2, T'(1) = (M1 - M2) - M3 along j, the same along i through LDS, fmaf(raw, inv, 32 b), ReLU,
      clamp, (2x2 maximum = one tile).  raw-32 output: the fp32 value; split-64 output: as above.
      K.  64 x 3 products per M_ij (192), two roundings inside V (+ 2, relative to |B^T| |d| |B|), one more for the second-order difference of Vl,
      three additions per direction of the output transform (+ 6), the fmaf (+ 1):  K = 202.  T = |A^T| [sum_ci (|Uh| + |Ul|) (|B^T| |d| |B|)] |A|.
  conv1a.  Unfused (conv1a_split_kernel): bias + nine fmaf over fp32 weights and the table's fl32(p) fl32(1/255), K = 10, x 32, split-64.  Fused into
      conv1b (OMNI_SPLIT_FUSE1A=1): conv1a is no tensor; the interval it may land in, a +- gamma_29 sum |products| around the exact value of the
      split-table algebra (``conv1a_fused``), and its storage step are carried through conv1b as ``extra``; there the kernel's xh cannot be
      recovered, so xl wl leaves the reference and |xl| <= ulp16(32 x) / 2 bounds it inside ``extra``.
  exact-f32 path (conv_mfma_kernel<float>, v_mfma_f32_32x32x2_f32): fp32 weights as given, K = 9 cin + 1: f16_layer_ref.conv_ref(round_w=False).

Two tiers per element, both from the kernel's own input.
  Tier 1 (derived, never to be exceeded): |got - y| <= gamma_K T + storage (+ extra), T = the sum of the magnitudes of the terms the kernel adds.
      Where T = 0 the kernel's value is fmaf(0, inv, bias') = bias' exactly: compared exactly (allowance 0 around the stored form of relu(bias')).
  Tier 2 (sensitivity): the same algebra emulated in float32 (``direct_emul`` / ``wino_emul`` / ``f32_emul``: one MFMA = an exact 16-term dot added to
      the accumulator with one rounding, in the kernels' order: tap column outer, tap row inner, hi k-groups against wh then wl, lo k-groups against wh),
      and per slice -- every output channel, every tile-position class -- RMS(got - y) / RMS(emulation - y) <= c (``tier2``).
  The fp32 tails (heat map, dense descriptors, the sparse tail's compact rows) take their references and tier-1 bounds from f16_layer_ref.semi_ref / desc_ref
      (extended with the fp32-input and the split convDb algebra) and their tier-2 emulations from ``semi_emul`` / ``desc_emul`` / ``convdb_split_emul`` here.
The emulators take a ``defect`` name: tests/test_split_layer_bound_cpu.py shows that each of them fails the gate.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.f16_layer_ref import U, _h2f, _t, f16, gamma, masked_u8, ulp16, x_oracle  # noqa: F401  (re-exported for the tests)

ACT = 32.0              # SPL_ACT_SCALE / WN_ACT_SCALE
# tier 2: the largest slice ratio a layer may show (``tier2``), per kernel form: twice the largest clean ratio measured on the MI355X over every configuration
# and shape of tests/test_gpu_split_layers.py (its docstring lists them per layer and configuration: direct 3.585, direct behind the fused conv1a 1.928,
# Winograd 2.508, Winograd behind the fused conv1a 2.002, the separate conv1a 1.000, exact-f32 1.487, the split detector head 2.120, the exact-f32 head 1.070,
# the exact-f32 convDb + norm 1.327, the split convDb + norm 2.306), far below the smallest ratio of any defect in tests/test_split_layer_bound_cpu.py (175)
TIER2_C = {"direct": 7.17, "direct_fused1a": 3.86, "wino": 5.02, "wino_fused1a": 4.0, "conv1a": 2.0, "f32": 2.97,
           "semi": 4.24, "semi_f32": 2.14, "desc": 2.65, "desc_rows_split": 4.61}
# lo-half bias gate: twice the largest clean |B| measured on the MI355X (0.0153), below the smallest |B| of lo halves rounded toward zero (0.10)
LO_BIAS_C = 0.031
CLAMP_SPLIT = 65000.0
CLAMP_WINO = 16000.0
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def f32(a) -> np.ndarray:
    return np.asarray(a, np.float64).astype(np.float32)


def _rtz16(v32: np.ndarray) -> np.ndarray:
    r = v32.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(v32.astype(np.float64))
    r[over] = np.nextafter(r[over], np.float16(0))
    return r


def split(v, lo_rtz: bool = False):
    """hi = half(v), lo = half(v - hi) of fp32 values (v - float(hi) is exact in fp32), as float64."""
    v32 = np.asarray(v, np.float32)
    hi = v32.astype(np.float16)
    r = v32 - hi.astype(np.float32)
    lo = _rtz16(r) if lo_rtz else r.astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def pow2_scale(mx: float) -> int:
    """k of the packers: mx = m 2^ex, m in [0.5, 1); k = 9 - ex."""
    return 9 - (int(np.frexp(np.float32(mx))[1]) if mx > 0 else 0)


def pack_split(w, lo_rtz: bool = False):
    """conv_pack_weights_split: (wh, wl [cout, cin, 3, 3] float64 of w 2^k, inv = 2^-k)."""
    w = np.asarray(w, np.float32)
    k = pow2_scale(float(np.abs(w).max()))
    wh, wl = split(np.ldexp(w, k), lo_rtz)
    return wh, wl, 2.0 ** -k


def wino_U(w) -> np.ndarray:
    """U = G g G^T in double, in the packer's order of summation, rounded to float: [4, 4, cout, cin] float32."""
    g = np.asarray(w, np.float32).astype(np.float64)
    out = np.zeros((4, 4) + g.shape[:2], np.float64)
    for i in range(4):
        for j in range(4):
            s = np.zeros(g.shape[:2], np.float64)
            for k in range(3):
                for l in range(3):
                    s = s + (G[i, k] * g[:, :, k, l]) * G[j, l]
            out[i, j] = s
    return out.astype(np.float32)


def pack_wino(w, lo_rtz: bool = False):
    """conv_pack_weights_wino: (Uh, Ul [4, 4, cout, cin] float64 of U 2^k, inv = 2^-k); k from max |G g G^T| in double."""
    g = np.asarray(w, np.float32).astype(np.float64)
    mx = float(np.abs(np.einsum("ik,ockl,jl->ijoc", G, g, G)).max())
    k = 9 - (int(np.frexp(mx)[1]) if mx > 0 else 0)
    Uh, Ul = split(np.ldexp(wino_U(w), k), lo_rtz)
    return Uh, Ul, 2.0 ** -k


def convdb_split(w):
    """convdb_pack_weights_split: hi = half(w), lo = half(w - hi), [256, 256] float64 each."""
    return split(np.asarray(w, np.float32).reshape(256, 256))


def store_split(v32: np.ndarray, lo_rtz: bool = False) -> np.ndarray:
    """What debug_layer returns for a split-64 value v (scaled by 32): fp32((hi + lo) / 32)."""
    hi, lo = split(v32, lo_rtz)
    return ((hi + lo) / ACT).astype(np.float32)


def storage_term(v_scaled) -> np.ndarray:
    """|v - hi - lo| of a split-64 store, in scaled units."""
    return np.maximum(2.0 ** -22 * np.abs(v_scaled), 2.0 ** -25)


class Ref:
    """y: the ideal value (true units); E: tier-1 allowance without ``extra``; extra: what an uncertain input may add; exact_in: the input's xl were halfs."""

    def __init__(self, y, E, extra=0.0, exact_in=True):
        self.y, self.E, self.extra, self.exact_in = y, E, extra, exact_in


def _conv(x, w):
    return F.conv2d(x, w, padding=1)


def _pool(t):
    return F.max_pool2d(t, 2, 2)


def _finish(S, T, X, c, bb, K, relu, pool, out, clamp):
    """Common tail of the references: v = S c + bias' (scaled units when out_split), allowance gamma_K (T c + |bias'|) + X c, ReLU / clamp, pool, the
    storage term, the T = 0 elements made exact.  out: "split" (split-64 frame), "raw32" (fp32 of the scaled value) or "f32" (true values).  Returns Ref in
    true units."""
    bt = _t(bb)[None, :, None, None]
    v = S * c + bt
    E = gamma(K) * (T * c + bt.abs())
    X = X * c if X is not None else None
    zero = (T == 0) & (X == 0 if X is not None else True)
    if relu:
        v = F.relu(v)
    v = v.clamp(-clamp, clamp)
    if pool:
        v, E, zero = _pool(v), _pool(E), -_pool(-zero.double()) > 0
        X = _pool(X) if X is not None else None
    v, E, zero = v.numpy(), E.numpy(), zero.numpy()
    Xn = X.numpy() if X is not None else 0.0
    if out == "split":
        E = E + storage_term(np.abs(v) + E + Xn)
        v[zero] = store_split(v[zero].astype(np.float32)).astype(np.float64) * ACT       # fmaf(0, inv, bias') = bias': exact, and stored as the kernel stores it
    else:
        v[zero] = v[zero].astype(np.float32).astype(np.float64)
    E[zero] = 0.0
    s = 1.0 if out == "f32" else 1.0 / ACT
    return Ref(v * s, E * s * (1 + 1e-9), Xn * s)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# direct split kernels
# ------------------------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def direct_ref(x, w, b, pool=False, out_f32=False, relu=True, u_in=None) -> Ref:
    """x [N, cin, H, W]: the stored input, true values (float64 of the fp32 debug_layer output; with ``u_in`` the ideal input of the fused conv1a and
    how far the kernel's own may be from it, both in true units)."""
    wh, wl, inv = pack_split(w)
    cin = wh.shape[1]
    xs = np.asarray(x, np.float64) * ACT
    xh = f16(xs).astype(np.float64)
    xl = xs - xh
    exact = u_in is not None or bool(np.array_equal(xl.astype(np.float16).astype(np.float64), xl))
    wht, wlt = _t(wh), _t(wl)
    S = _conv(_t(xs), wht + wlt)
    T = _conv(_t(np.abs(xh)), wht.abs() + wlt.abs())
    X = None
    if u_in is None:
        S = S - _conv(_t(xl), wlt)
        T = T + _conv(_t(np.abs(xl)), wht.abs())
    else:
        us = np.asarray(u_in, np.float64) * ACT
        half_step = 0.5 * ulp16(np.abs(xs) + us)
        T = T + _conv(_t(half_step), wht.abs())
        X = _conv(_t(us), wht.abs() + wlt.abs()) + _conv(_t(half_step), wlt.abs())       # the input's interval, and the xl wl that cannot be restated
    c = inv / ACT if out_f32 else inv
    bb = np.asarray(b, np.float64) * (1.0 if out_f32 else ACT)
    r = _finish(S, T, X, c, bb, 27 * cin + 2, relu, pool, "f32" if out_f32 else "split", CLAMP_SPLIT)
    r.exact_in = exact
    return r


@torch.no_grad()
def direct_emul(x, w, b, pool=False, out_f32=False, relu=True, defect=None) -> np.ndarray:
    """The direct split kernel in float32: the stored output [N, cout, H', W'] (true units, fp32).  x: the stored input (fp32, true units)."""
    rtz = defect == "lo_rtz"
    wh, wl, inv = pack_split(w, rtz)
    cout, cin = wh.shape[:2]
    xh, xl = split(np.asarray(x, np.float32) * np.float32(ACT))
    n, _, h, wd = xh.shape
    xhp, xlp = F.pad(_t(xh), (1, 1, 1, 1)), F.pad(_t(xl), (1, 1, 1, 1))
    wht, wlt = _t(wh), _t(wl)
    parts = []
    for cb in range(cin // 64):
        acc = torch.zeros((n, cout, h, wd), dtype=torch.float32)
        add = lambda a, ww, xx: (a.double() + torch.einsum("ok,nkhw->nohw", ww, xx)).float()
        for kx in range(3):
            for ky in range(3):
                for kq in range(4):
                    ch = slice(cb * 64 + kq * 16, cb * 64 + kq * 16 + 16)
                    xw = xhp[:, ch, ky:ky + h, kx:kx + wd]
                    acc = add(acc, wht[:, ch, ky, kx], xw)
                    wlo = wlt[:, ch, ky, kx]
                    if defect == "drop_xh_wl_wave":
                        wlo = wlo.clone()
                        wlo[32:64] = 0
                    if defect == "drop_xh_wl_channel40":
                        wlo = wlo.clone()
                        wlo[40] = 0
                    acc = add(acc, wlo, xw)
                for kq in range(4):
                    if defect == "drop_xl_wh" and (kx, ky, kq, cb) == (1, 2, 2, 0):
                        continue
                    ch = slice(cb * 64 + kq * 16, cb * 64 + kq * 16 + 16)
                    acc = add(acc, wht[:, ch, ky, kx], xlp[:, ch, ky:ky + h, kx:kx + wd])
        parts.append(acc)
    if len(parts) == 2:
        other = parts[1]
        if defect == "partner_col31":                     # the partner's partial sum of the pixel to the left, in column 31 of every tile
            other = other.clone()
            other[..., 31::32] = parts[1][..., 30::32][..., : other[..., 31::32].shape[-1]]
        acc = parts[0] + other
    else:
        acc = parts[0]
    return _emul_tail(acc, b, inv, pool, out_f32, relu, CLAMP_SPLIT, defect)


def _emul_tail(acc, b, inv, pool, out_f32, relu, clamp, defect, raw32=False):
    """fmaf(raw, inv', bias'), ReLU and clamp, (the pool on the raw sums: monotone), the store."""
    h = acc.shape[-2]
    if pool:
        p = _pool(acc)
        if defect == "pool_shift_last_row":
            p[:, :, -1] = _pool(acc[:, :, h - 3: h - 1])[:, :, 0]
        acc = p
    c = np.full(acc.shape[1], inv / ACT if out_f32 else inv)
    if defect == "inv_x2_group":
        c[:64] *= 2.0
    bb = f32(np.asarray(b, np.float64) * (1.0 if out_f32 else ACT)).astype(np.float64)
    if defect == "neighbour_bias":
        bb[3] = bb[4]
    v = (acc.double() * _t(c)[None, :, None, None] + _t(bb)[None, :, None, None]).float()          # one rounding: fmaf
    v = v.clamp(0.0 if relu else -clamp, clamp).numpy()
    if out_f32:
        return v
    if raw32:
        return (v.astype(np.float64) / ACT).astype(np.float32)
    return store_split(v, defect == "lo_rtz")


# ------------------------------------------------------------------------------------------------------------------------------------------------
# Winograd F(2x2, 3x3) kernels
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _patches(d: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] (H, W even) -> the 4 x 4 input patches of the 2 x 2 output tiles, [N, C, H / 2, W / 2, 4, 4]."""
    p = F.pad(d, (1, 1, 1, 1))
    return p.unfold(2, 4, 2).unfold(3, 4, 2)


def wino_V(d32: np.ndarray, defect=None):
    """The kernel's V = B^T d B in fp32: W_i = fmaf(beta_i, d[rb_i], d[ra_i]), then V_i0 = W0 - W2, V_i1 = W1 + W2, V_i2 = W2 - W1, V_i3 = W1 - W3.
    Returns (Vh, Vl) [N, C, ty, tx, 4, 4] float64 tensors."""
    P = _patches(_t(d32))
    r32 = lambda t: t.float().double()
    Wv = [r32(P[..., 0, :] - P[..., 2, :]), r32(P[..., 1, :] + P[..., 2, :]), r32(P[..., 2, :] - P[..., 1, :]), r32(P[..., 1, :] - P[..., 3, :])]
    Wv = torch.stack(Wv, -2)                                                  # [..., i, column]
    pairs = ((0, 2, -1.0), (1, 2, 1.0), (2, 1, -1.0), (1, 3, -1.0))
    if defect == "v_split_before_hadd":                                       # the column sums split first, the halves combined in fp16
        wh, wl = split(Wv.numpy().astype(np.float32))
        h16 = lambda a: _t(np.asarray(a, np.float64).astype(np.float16).astype(np.float64))
        Vh = torch.stack([h16(wh[..., a] + s * wh[..., b]) for a, b, s in pairs], -1)
        Vl = torch.stack([h16(wl[..., a] + s * wl[..., b]) for a, b, s in pairs], -1)
        return Vh, Vl
    V = torch.stack([r32(Wv[..., a] + s * Wv[..., b]) for a, b, s in pairs], -1)
    vh, vl = split(V.numpy().astype(np.float32), defect == "lo_rtz")
    return _t(vh), _t(vl)


def _pos_major(Vm):
    """[n, c, y, x, i, j] -> [16, c, n y x] (position-major, contiguous): the layout the sixteen matrix products want."""
    n, c, y, x = Vm.shape[:4]
    return Vm.permute(4, 5, 1, 0, 2, 3).reshape(16, c, n * y * x)


def _mm16(Um, V16):
    """sum_c U[i, j, o, c] V16[4 i + j, c, t] -> [16, o, t] (float64)."""
    return torch.bmm(Um.reshape(16, Um.shape[2], Um.shape[3]).contiguous(), V16)


def _tiles(M16, n, y, x):
    """[16, o, n y x] -> [n, o, y, x, i, j] (a view)."""
    return M16.reshape(4, 4, M16.shape[1], n, y, x).permute(3, 2, 4, 5, 0, 1)


def _out_transform64(M):
    """A^T M A of [N, O, ty, tx, 4, 4] -> [N, O, 2 ty, 2 tx] in float64."""
    A = _t(AT)
    Y = torch.einsum("ai,noyxij,bj->noyaxb", A, M, A)
    n, o, ty, _, tx, _ = Y.shape
    return Y.reshape(n, o, 2 * ty, 2 * tx)


@torch.no_grad()
def wino_ref(x, w, b, pool=False, out_split=False, relu=True, u_in=None) -> Ref:
    Uh, Ul, inv = pack_wino(w)
    d = np.asarray(x, np.float64) * ACT
    Ut, Ult = _t(Uh + Ul), _t(Ul)
    Uabs = _t(np.abs(Uh) + np.abs(Ul))
    B = _t(BT)
    P = _patches(_t(d))
    V = torch.einsum("ik,nchwkl,jl->nchwij", B, P, B)
    Vabs = torch.einsum("ik,nchwkl,jl->nchwij", B.abs(), P.abs(), B.abs()) * (1 + 2.0 ** -10)
    n, _, ty, tx = V.shape[:4]
    V16 = _pos_major(V)
    mm = lambda Um, Vm: _mm16(Um, _pos_major(Vm))
    M = _mm16(Ut, V16)
    Tm = _tiles(mm(Uabs, Vabs), n, ty, tx)
    Xm = None
    if u_in is None:
        _, Vl = wino_V(d.astype(np.float32))
        M = M - mm(Ult, Vl)
    else:
        us = _t(np.asarray(u_in, np.float64) * ACT)
        Uin = torch.einsum("ik,nchwkl,jl->nchwij", B.abs(), _patches(us), B.abs())
        half_step = _t(0.5 * ulp16((Vabs + Uin).numpy()))
        Xm = _tiles(mm(Uabs, Uin) + mm(Ult.abs(), half_step), n, ty, tx)
    M = _tiles(M, n, ty, tx)
    A = _t(np.abs(AT))
    absT = lambda Mm: (lambda Y: Y.reshape(Y.shape[0], Y.shape[1], 2 * Y.shape[2], 2 * Y.shape[4]))(torch.einsum("ai,noyxij,bj->noyaxb", A, Mm, A))
    S, T = _out_transform64(M), absT(Tm)
    X = absT(Xm) if Xm is not None else None
    return _finish(S, T, X, inv, np.asarray(b, np.float64) * ACT, 202, relu, pool, "split" if out_split else "raw32", CLAMP_WINO)


@torch.no_grad()
def wino_emul(x, w, b, pool=False, out_split=False, relu=True, defect=None) -> np.ndarray:
    """The Winograd kernel in float32: stored output (true units, fp32).  x: the stored input (fp32, true units; the frame holds 32 x as fp32)."""
    Uh, Ul, inv = pack_wino(w, defect == "lo_rtz")
    if defect == "ul_missing_pos":
        Ul = Ul.copy()
        Ul[1, 2] = 0.0
    Uht, Ult = _t(Uh), _t(Ul)
    d32 = (np.asarray(x, np.float32) * np.float32(ACT)).astype(np.float32)
    Vh, Vl = wino_V(d32, defect)
    n, _, ty, tx = Vh.shape[:4]
    cout = Uh.shape[2]
    Vh16, Vl16 = _pos_major(Vh), _pos_major(Vl)
    acc = torch.zeros((16, cout, n * ty * tx), dtype=torch.float32)
    add = lambda a, Um, Vm: (a.double() + _mm16(Um, Vm)).float()
    for kg in range(4):
        ch = slice(16 * kg, 16 * kg + 16)
        acc = add(acc, Uht[:, :, :, ch], Vh16[:, ch])
        acc = add(acc, Ult[:, :, :, ch], Vh16[:, ch])
        acc = add(acc, Uht[:, :, :, ch], Vl16[:, ch])
    acc = _tiles(acc, n, ty, tx)
    # along j (lane-local): T'(0) = (M0 + M1) + M2, T'(1) = (M1 - M2) - M3
    M = acc
    T0 = (M[..., 0] + M[..., 1]) + M[..., 2]
    T1 = (M[..., 1] - M[..., 2]) - M[..., 3]
    Tp = torch.stack([T0, T1], -1)                                            # [n, o, ty, tx, i, b]
    # along i: the wave that finishes a channel quarter adds the other three waves' terms first (its own slot reads zero), its own last
    ya = torch.zeros((n, cout, ty, tx, 2, 2), dtype=torch.float32)
    for q in range(cout // 16):
        wv = q % 4
        sl = slice(16 * q, 16 * q + 16)
        t = [Tp[:, sl, :, :, s, :] if s != wv else torch.zeros_like(Tp[:, sl, :, :, 0, :]) for s in range(4)]
        own = Tp[:, sl, :, :, wv, :]
        c0 = 0.0 if wv == 3 else 1.0
        c1 = 0.0 if wv == 0 else (1.0 if wv == 1 else -1.0)
        ya[:, sl, :, :, 0, :] = ((t[0] + t[1]) + t[2]) + own * c0
        ya[:, sl, :, :, 1, :] = ((t[1] - t[2]) - t[3]) + own * c1
    if defect == "at_sign_flip_odd_col":
        ya[:, :, :, 1::2, 1, :] = -ya[:, :, :, 1::2, 1, :]
    raw = ya.permute(0, 1, 2, 4, 3, 5).reshape(n, cout, 2 * ty, 2 * tx)
    return _emul_tail(raw, b, inv, pool, False, relu, CLAMP_WINO, defect, raw32=not out_split)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# conv1a
# ------------------------------------------------------------------------------------------------------------------------------------------------
def conv1a_fused_parts(w1a, b1a):
    """The constants of the fused conv1a (conv1a_split_pack_fused + conv1a_make_split_lut), float64: per byte value xh, xl [256]; wh, wl [64, 9] of 32 w;
    bh, bl [64] of 32 b."""
    xo = x_oracle(np.arange(256))
    xh, xl = split(xo)
    w32 = np.asarray(w1a, np.float32).reshape(64, 9) * np.float32(ACT)
    b32 = np.asarray(b1a, np.float32) * np.float32(ACT)
    wh, wl = split(w32)
    bh, bl = split(b32)
    return xh, xl, wh, wl, bh, bl


def _taps(img_u8: np.ndarray) -> np.ndarray:
    """[N, H, W] u8 (already masked) -> the byte under each of the nine taps, [N, 9, H, W] (0 outside the image)."""
    p = np.pad(np.asarray(img_u8, np.int64), ((0, 0), (1, 1), (1, 1)))
    h, w = img_u8.shape[-2:]
    return np.stack([p[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 1)


def conv1a_fused(img_u8, w1a, b1a):
    """(a, delta) [N, 64, H, W] float64, scaled by 32: the exact value of the fused conv1a's 29 products, sum_t (xh wh + xl wh + xh wl) + bh + bl (before
    the ReLU), and gamma_29 times the sum of their magnitudes -- what two MFMAs that add them in fp32 may be off by."""
    xh, xl, wh, wl, bh, bl = conv1a_fused_parts(w1a, b1a)
    t = _taps(img_u8)
    XH, XL = xh[t], xl[t]
    a = np.einsum("nthw,ct->nchw", XH + XL, wh) + np.einsum("nthw,ct->nchw", XH, wl) + (bh + bl)[None, :, None, None]
    mag = np.einsum("nthw,ct->nchw", np.abs(XH) + np.abs(XL), np.abs(wh)) + np.einsum("nthw,ct->nchw", np.abs(XH), np.abs(wl)) + (np.abs(bh) + np.abs(bl))[None, :, None, None]
    return a, gamma(29) * mag


def conv1a_fused_input(img_u8, w1a, b1a, split_store: bool):
    """(x, u_in) in true units for the layer behind the fused conv1a: x = relu(a) / 32, u_in = delta (+ the split-64 storage step of the direct kernel's halo)."""
    a, d = conv1a_fused(img_u8, w1a, b1a)
    v = np.maximum(a, 0.0)
    u = d + (storage_term(v + d) if split_store else 2.0 ** -24 * (v + d))      # (Winograd: the fp32 value itself, rounded once by the MFMA's last add: inside delta; kept as margin)
    return v / ACT, u / ACT


def conv1a_fused_emul(img_u8, w1a, b1a, split_store: bool) -> np.ndarray:
    """The fused conv1a in float32 (two MFMAs: taps 0-3 and 5-8 against wh from zero; then tap 4, the wl terms and the bias halves), ReLU, stored as the
    consumer reads it: (hi + lo) / 32 for the direct kernel, the fp32 value / 32 for the Winograd kernel."""
    xh, xl, wh, wl, bh, bl = conv1a_fused_parts(w1a, b1a)
    t = _taps(img_u8)
    XH, XL = xh[t], xl[t]
    o = [0, 1, 2, 3, 5, 6, 7, 8]
    d0 = np.einsum("nthw,ct->nchw", (XH + XL)[:, o], wh[:, o]).astype(np.float32)
    d1 = np.einsum("nhw,c->nchw", (XH + XL)[:, 4], wh[:, 4]) + np.einsum("nthw,ct->nchw", XH, wl) + (bh + bl)[None, :, None, None]
    a = (d0.astype(np.float64) + d1).astype(np.float32)
    v = np.clip(a, 0.0, CLAMP_SPLIT if split_store else CLAMP_WINO)
    return store_split(v) if split_store else (v.astype(np.float64) / ACT).astype(np.float32)


@torch.no_grad()
def conv1a_split_ref(img_u8, w1a, b1a) -> Ref:
    """conv1a_split_kernel: acc = bias, nine fmaf(x_t, w_t, acc) in fp32 (K = 10), x 32 (exact), ReLU, split-64."""
    x = _t(x_oracle(img_u8).astype(np.float64)[:, None])
    wt = _t(np.asarray(w1a, np.float64).reshape(64, 1, 3, 3))
    S = _conv(x, wt) * ACT
    T = _conv(x.abs(), wt.abs()) * ACT
    return _finish(S, T, None, 1.0, np.asarray(b1a, np.float64) * ACT, 10, True, False, "split", CLAMP_SPLIT)


def conv1a_split_emul(img_u8, w1a, b1a) -> np.ndarray:
    x = x_oracle(img_u8).astype(np.float64)
    t = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    h, w = x.shape[-2:]
    w64 = np.asarray(w1a, np.float32).reshape(64, 9).astype(np.float64)
    acc = np.broadcast_to(np.asarray(b1a, np.float32)[None, :, None, None], (x.shape[0], 64, h, w)).astype(np.float32)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        acc = (acc.astype(np.float64) + t[:, None, ky:ky + h, kx:kx + w] * w64[None, :, tap, None, None]).astype(np.float32)
    return store_split(np.clip(acc * np.float32(ACT), 0.0, CLAMP_SPLIT))


# ------------------------------------------------------------------------------------------------------------------------------------------------
# exact-f32 path
# ------------------------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def f32_ref(x, w, b, pool=False, relu=True) -> Ref:
    """conv_mfma_kernel<float> (v_mfma_f32_32x32x2_f32: every product rounded into the fp32 accumulator) / conv1a_kernel<float>: K = k k cin + 1."""
    from tests.f16_layer_ref import conv_ref
    y, E, _ = conv_ref(np.asarray(x, np.float64), w, b, relu=relu, pool=pool, round_w=False)
    return Ref(y, E * (1 + 1e-9))


@torch.no_grad()
def f32_emul(x, w, b, pool=False, relu=True, defect=None) -> np.ndarray:
    """A float32 accumulation chain in conv_mfma_kernel's order: 64-channel chunks outer, taps in raster order, the chunk's channels inner (k-steps of two:
    one v_mfma_f32_32x32x2_f32, each product added with its own rounding); the pool on the raw sums, then the bias, then the ReLU."""
    w64 = _t(np.asarray(w, np.float32).astype(np.float64))
    cout, cin, k, _ = w64.shape
    xp = F.pad(_t(np.asarray(x, np.float32).astype(np.float64)), (k // 2,) * 4)
    n, _, h, wd = x.shape
    acc = torch.zeros((n, cout, h, wd), dtype=torch.float32)
    for c0 in range(0, cin, 64):
        for ky in range(k):
            for kx in range(k):
                xs = xp[:, :, ky:ky + h, kx:kx + wd]
                for ci in range(c0, min(c0 + 64, cin)):
                    term = w64[None, :, ci, ky, kx, None, None] * xs[:, ci, None]
                    if defect == "kstep_fp16" and (ky, kx) == (1, 1) and ci // 2 == 3:
                        acc = (acc.double() + term).half().float()
                    else:
                        acc = (acc.double() + term).float()
    bb = np.asarray(b, np.float32).astype(np.float64).copy()
    if defect == "neighbour_bias":
        bb[3] = bb[4]
    v = (acc.double() + _t(bb)[None, :, None, None]).float()
    if relu:
        v = F.relu(v)
    if pool:
        p = _pool(v)
        if defect == "pool_shift_last_row":
            p[:, :, -1] = _pool(v[:, :, h - 3: h - 1])[:, :, 0]
        v = p
    return v.numpy()


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the fp32 tails: float32 emulations for tier 2 (their references and tier-1 bounds: f16_layer_ref.semi_ref / desc_ref)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _chain32(acc, x64, w64, ks):
    """acc (float32 [N, C, H, W]) += w[:, k] x[:, k] for k in ks, one product at a time, each sum rounded to float32."""
    for k in ks:
        acc = (acc.double() + w64[None, :, k, None, None] * x64[:, k, None]).float()
    return acc


@torch.no_grad()
def semi_emul(heads_cpa, wPb, bPb, exact_f32=False, defect=None) -> np.ndarray:
    """The detector head in float32: [N, 8 Hc, 8 Wc].  detector_head_mfma16_kernel<float>: per k-step of 16 channels wl xh, wh xh, wh xl (one exact 16-term dot
    and one rounding each), then the bias; the dustbin two fmaf chains (channels 16 s + 8 hh ..+ 8, s ascending) added, then its bias.  exact_f32
    (detector_head_mfma_kernel<float>): step j adds the products of channels j and 128 + j, each rounded into the accumulator; the dustbin's chains are channels
    [0, 128) and [128, 256).  Softmax as the kernel: z - max, expf, the sum (here in double, rounded once: its order moves the result by 1e-7 relative, below the
    logits' share), one division."""
    x32 = np.asarray(heads_cpa, np.float32)
    w32 = np.asarray(wPb, np.float32).reshape(65, 256)
    b64 = _t(np.asarray(bPb, np.float32).astype(np.float64))
    x64, w64 = _t(x32.astype(np.float64)), _t(w32.astype(np.float64))
    n, _, h, wd = x32.shape
    acc = torch.zeros((n, 64, h, wd), dtype=torch.float32)
    if exact_f32:
        order = [k for j in range(128) for k in (j, 128 + j)]
        if defect == "kstep_fp16":
            acc = _chain32(acc, x64, w64[:64], order[:40])
            acc = _chain32(acc, x64, w64[:64], order[40:42]).half().float()
            acc = _chain32(acc, x64, w64[:64], order[42:])
        else:
            acc = _chain32(acc, x64, w64[:64], order)
        halves = [range(0, 128), range(128, 256)]
    else:
        xh, xl = (_t(a) for a in split(x32))
        wh, wl = (_t(a) for a in split(w32[:64]))
        add = lambda a, ww, xx: (a.double() + torch.einsum("ok,nkhw->nohw", ww, xx)).float()
        for s in range(16):
            ch = slice(16 * s, 16 * s + 16)
            wlo = wl[:, ch]
            if defect == "wl_wrong_kstep" and s == 9:
                wlo = wl[:, 16 * 10: 16 * 11]
            acc = add(acc, wlo, xh[:, ch])
            acc = add(acc, wh[:, ch], xh[:, ch])
            if not (defect == "drop_xl_wh" and s == 5):
                acc = add(acc, wh[:, ch], xl[:, ch])
        halves = [[16 * s + 8 * hh + e for s in range(16) for e in range(8)] for hh in range(2)]
    z = (acc.double() + b64[None, :64, None, None]).float()
    d = [_chain32(torch.zeros((n, 1, h, wd), dtype=torch.float32), x64, w64[64:], ks) for ks in halves]
    dust = ((d[0] + d[1]).double() + b64[64]).float()
    z = torch.cat([z, dust], 1)
    e = torch.exp(z - z.max(1, keepdim=True).values)
    p = (e / e.double().sum(1, keepdim=True).float())[:, :64]
    return p.permute(0, 2, 3, 1).reshape(n, h, wd, 8, 8).permute(0, 1, 3, 2, 4).reshape(n, h * 8, wd * 8).numpy()


def semi_cells(semi) -> np.ndarray:
    """[N, 8 Hc, 8 Wc] -> [1, 64, 1, N Hc Wc]: the 64 logit channels of every cell, the cells in the kernels' linear order (32 consecutive cells are one MFMA
    fragment: ``tier2`` with 1 x 32 tiles slices by channel and by the cell's lane)."""
    s = np.asarray(semi)
    n, H, W = s.shape
    return s.reshape(n, H // 8, 8, W // 8, 8).transpose(2, 4, 0, 1, 3).reshape(1, 64, 1, -1)


def _l2norm32(v: torch.Tensor) -> np.ndarray:
    nrm = v.double().pow(2).sum(1, keepdim=True).float().sqrt()
    return (v / nrm).numpy()


@torch.no_grad()
def desc_emul(cda, wDb, bDb) -> np.ndarray:
    """The fp32-class dense descriptors in float32: the exact-f32 1 x 1 convolution (``f32_emul``), then l2norm_kernel (the sum of squares in double, rounded once)."""
    return _l2norm32(_t(f32_emul(cda, np.asarray(wDb, np.float32).reshape(256, 256, 1, 1), bDb, relu=False)))


@torch.no_grad()
def convdb_split_emul(rows, wDb, bDb, defect=None) -> np.ndarray:
    """convdb_l2norm_split_kernel in float32 over rows [R, 256, 1, 1]: per k-step of 16 channels wl xh, wh xh, wh xl (an exact 16-term dot and one rounding each),
    the bias, the row's norm, the division."""
    xh, xl = (_t(a) for a in split(np.asarray(rows, np.float32)))
    wh, wl = (_t(a) for a in convdb_split(wDb))
    acc = torch.zeros(xh.shape, dtype=torch.float32)
    add = lambda a, ww, xx: (a.double() + torch.einsum("ok,nkhw->nohw", ww, xx)).float()
    for s in range(16):
        ch = slice(16 * s, 16 * s + 16)
        wlo = wl[:, ch]
        if defect == "wl_wrong_kstep" and s == 9:
            wlo = wl[:, 16 * 10: 16 * 11]
        acc = add(acc, wlo, xh[:, ch])
        acc = add(acc, wh[:, ch], xh[:, ch])
        if not (defect == "drop_xl_wh" and s == 5):
            acc = add(acc, wh[:, ch], xl[:, ch])
    v = (acc.double() + _t(np.asarray(bDb, np.float32).astype(np.float64))[None, :, None, None]).float()
    return _l2norm32(v)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the gates
# ------------------------------------------------------------------------------------------------------------------------------------------------
def tier1(got, ref: Ref) -> dict:
    """Per element |got - y| <= E + extra.  Nothing is left out: an element without allowance (T = 0) must be exact, a non-finite one fails."""
    g = np.asarray(got, np.float64)
    assert g.shape == ref.y.shape, (g.shape, ref.y.shape)
    allow = np.broadcast_to(ref.E + ref.extra, g.shape)
    err = np.abs(g - ref.y)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allow > 0, err / allow, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(g), ratio, np.inf)
    i = int(np.argmax(ratio))
    return {"ok": bool(ref.exact_in) and bool((ratio <= 1.0).all()), "exact_in": bool(ref.exact_in), "ratio": float(ratio.flat[i]),
            "where": tuple(int(v) for v in np.unravel_index(i, g.shape)), "violations": int((ratio > 1.0).sum()), "n": int(g.size),
            "got": float(g.flat[i]), "ref": float(ref.y.flat[i])}


def tile_classes(h: int, w: int, tile_h: int, tile_w: int, pooled: bool, transposed: bool = False):
    """Labels [h, w] of an OUTPUT map: (y mod the tile's rows, x mod the tile's columns) in the kernel's tile grid (tile_h x tile_w of the layer's
    pre-pool map; transposed tiles swap the roles); a pooled output pixel takes the class of its window."""
    f = 2 if pooled else 1
    th, tw = (tile_w, tile_h) if transposed else (tile_h, tile_w)
    th, tw = max(th // f, 1), max(tw // f, 1)
    yy, xx = np.meshgrid(np.arange(h) % th, np.arange(w) % tw, indexing="ij")
    return yy, xx, th, tw


SLICE_FLOOR = 0.25     # tier 2: a slice's emulated sum of squares counts as at least this share of the average slice of its kind


def tier2(got, emul, ref: Ref, tile_h: int, tile_w: int, pooled: bool, transposed: bool = False) -> dict:
    """The worst ratio RMS(z_got) / RMS(z_emul) over the slices -- every output channel, every row class, every column class of the tile grid --, z = the
    error divided by the element's tier-1 allowance (errors scale with the magnitude of the terms: without it a few large outputs are the whole RMS).
    Every element is in one slice of each kind.  Behind a ReLU a channel may be zero (and exact) nearly everywhere; an RMS over its few live elements says
    nothing, so the denominator is at least SLICE_FLOOR of the average slice of the kind: such a slice is held to the layer's noise instead of its own, and
    tier 1 still holds each of its elements.  A layer whose emulation is exact everywhere must be exact in ``got`` too (ratio inf otherwise)."""
    allow = np.broadcast_to(ref.E + ref.extra, ref.y.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        zg = np.where(allow > 0, (np.asarray(got, np.float64) - ref.y) / allow, np.where(np.asarray(got, np.float64) == ref.y, 0.0, np.inf))
        ze = np.where(allow > 0, (np.asarray(emul, np.float64) - ref.y) / allow, 0.0)
    eg, ee = np.where(np.isfinite(zg), zg, np.inf) ** 2, ze ** 2
    n, c, h, w = eg.shape
    yy, xx, th, tw = tile_classes(h, w, tile_h, tile_w, pooled, transposed)
    worst, where = 0.0, None

    def upd(kind, sg, se):
        nonlocal worst, where
        den = np.maximum(se, SLICE_FLOOR * se.mean())
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(den > 0, np.sqrt(sg / np.where(den > 0, den, 1.0)), np.where(sg > 0, np.inf, 0.0))
        i = int(np.argmax(r))
        if r.flat[i] > worst or where is None:
            worst, where = float(r.flat[i]), (kind, i)

    upd("channel", eg.sum((0, 2, 3)), ee.sum((0, 2, 3)))
    rows_g, rows_e = eg.sum((0, 1, 3)), ee.sum((0, 1, 3))
    upd("row class", np.array([rows_g[yy[:, 0] == k].sum() for k in range(th)]), np.array([rows_e[yy[:, 0] == k].sum() for k in range(th)]))
    cols_g, cols_e = eg.sum((0, 1, 2)), ee.sum((0, 1, 2))
    upd("column class", np.array([cols_g[xx[0] == k].sum() for k in range(tw)]), np.array([cols_e[xx[0] == k].sum() for k in range(tw)]))
    return {"ratio": worst, "where": where, "rms_got": float(np.sqrt(eg.mean())), "rms_emul": float(np.sqrt(ee.mean()))}


def lo_bias(got, emul, ref: Ref) -> dict:
    """Split-64 outputs only: B = cov(got - y, s) / RMS(emul - y), s = the sign of the ideal lo half, y - half(y) (scaled values).  Rounding lo to nearest
    leaves the error uncorrelated with s: B is the mean of n zero-mean variates of about unit RMS, |B| <= 6 r / sqrt(n) at six sigma (r = the ratio
    RMS(got - y) / RMS(emul - y) of the whole layer).  The covariance, not the plain mean of e s: the matrix cores' accumulation leaves the error a small mean
    of its own (measured: -0.1 of its RMS), which times the imbalance of s would pass for a correlation.  A lo half rounded toward zero is short by up to an
    fp16 step of lo on the side of s: B goes to -0.1 .. -0.17, far outside.  On the MI355X the clean kernels show a small correlation of their own (|B| up to
    0.0153 over 7e5 elements, beyond six sigma of pure noise): the limit is at least LO_BIAS_C, twice that."""
    ys = ref.y * ACT
    s = np.sign(ys - ys.astype(np.float16).astype(np.float64))
    e = np.asarray(got, np.float64) - ref.y
    rms_e = float(np.sqrt(((np.asarray(emul, np.float64) - ref.y) ** 2).mean()))
    rms_g = float(np.sqrt((e ** 2).mean()))
    n = int(np.count_nonzero(s))
    cov = float((e * s).mean() - e.mean() * s.mean())
    B = cov / rms_e if rms_e > 0 else (0.0 if rms_g == 0 else np.inf)
    limit = max(6.0 * (rms_g / rms_e if rms_e > 0 else 1.0) / np.sqrt(max(n, 1)), LO_BIAS_C)
    return {"B": B, "limit": float(limit), "ok": bool(abs(B) <= limit), "n": n}


def old_gate(got, ref_true) -> bool:
    """The max-norm gate of tests/test_gpu_superpoint.py: |got - ref| < 2e-5 max(1, max |ref|)."""
    return bool(np.abs(np.asarray(got, np.float64) - ref_true).max() < 2e-5 * max(1.0, np.abs(ref_true).max()))
