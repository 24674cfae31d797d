"""fp64 references and arithmetic error bounds for the layers of the fp16 SuperPoint path (OMNI_PREC_F16).

Each fp16 layer is almost fully determined by its own input: ``omni_sp_debug_layer`` returns the stored fp16 activations exactly, the
packers round the weights to nearest fp16 (``pack_weights<__half>`` -> ``__float2half_rn``, ``convdb_pack_weights`` -> ``f2h_bits``), the
biases stay fp32, ``v_mfma_f32_32x32x16_f16`` forms exact products and sums them in fp32, and the epilogue adds the bias, applies ReLU
(and the 2x2 max-pool) and rounds once to nearest fp16.  So a layer is recomputed here in float64 from the kernel's own input, and the
difference may only be what that arithmetic allows.  The errors of earlier layers do not enter.

Accumulation bound.  A sum of K terms evaluated in fp32 with round-to-nearest, in any order, is within gamma_K * sum |term| of the exact
sum, gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).  A 3x3
layer with cin input channels sums K = 9 cin + 1 terms: the products and the bias (added in fp32 in the epilogue).  ReLU and max are
1-Lipschitz, so the bound of a pooled output is the largest bound in its 2x2 window.  The final conversion to fp16 adds at most half the
fp16 spacing of the stored value (``ulp16``; subnormals included: omni-swarm_amd/Makefile builds with plain ``-O3`` and no
denormal-flushing or fast-math flag, and fp16 denormals are always kept by the hardware).

The fp32 outputs (the heat map and the dense descriptors) carry their own evaluation terms, derived in ``semi_ref`` and ``desc_ref``.
These two bounds come out looser than 1e-5 absolute: they are worst-case sums of |terms| over K = 513 and K = 257 products, about
3e-5 and 1.5e-5 of the sum of the absolute products, and the heat map adds the softmax's amplification of the logits' bound.  Typical
errors are square-root-of-K smaller; the measured ratios in tests/test_gpu_f16_layers.py show how much.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def f16(a) -> np.ndarray:
    """Round to nearest fp16 (ties to even), from the fp32 value, as ``__float2half_rn`` does."""
    return np.asarray(a, np.float32).astype(np.float16)


def f16_down(v: np.ndarray) -> np.ndarray:
    """The largest fp16 <= v (float64 in, float64 out)."""
    r = v.astype(np.float16)
    bad = r.astype(np.float64) > v
    r[bad] = np.nextafter(r[bad], np.float16(-np.inf))
    return r.astype(np.float64)


def f16_up(v: np.ndarray) -> np.ndarray:
    """The smallest fp16 >= v (float64 in, float64 out)."""
    r = v.astype(np.float16)
    bad = r.astype(np.float64) < v
    r[bad] = np.nextafter(r[bad], np.float16(np.inf))
    return r.astype(np.float64)


def ulp16(v: np.ndarray) -> np.ndarray:
    """The fp16 spacing at |v|: 2^(e - 10) for |v| in [2^e, 2^(e+1)), 2^-24 below 2^-14 (subnormals) and at zero."""
    a = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(a)                       # a = m 2^e, m in [0.5, 1)
    e = np.maximum(e - 1, -14)
    return np.where(a == 0, 2.0 ** -24, np.ldexp(1.0, e - 10))


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


@torch.no_grad()
def conv_ref(x16, w, b, relu: bool = True, pool: bool = False, round_w: bool = True, u_in=None, k_terms: int | None = None):
    """fp64 reference of one convolution layer and its accumulation bound.

    x16 [N, cin, H, W]: the layer's input as the kernel read it; w [cout, cin, k, k] fp32 (rounded to nearest fp16 here when
    ``round_w``, as the packers do); b [cout] fp32.  Returns (y, E, extra), all [N, cout, H', W'] float64:
      y     = relu(conv(x, w16, pad k // 2) + b), then the 2x2 max-pool when ``pool``;
      E     = gamma_K (conv(|x| + u_in, |w16|) + |b|), K = k k cin + 1 (or ``k_terms``), the window maximum when pooled;
      extra = conv(u_in, |w16|) (window maximum when pooled): how far the layer may move when every input may be off by up to
              u_in [N, cin, H, W] from x16 (the conv1a interval of the fused conv1b); 0 when u_in is None.
    """
    x = _t(x16)
    w64 = f16(w).astype(np.float64) if round_w else np.asarray(w, np.float64)
    wt, bt = _t(w64), _t(b)
    k = w64.shape[-1]
    K = k_terms if k_terms is not None else k * k * w64.shape[1] + 1
    y = F.conv2d(x, wt, bt, padding=k // 2)
    ax = x.abs()
    if u_in is not None:
        ut = _t(u_in)
        both = F.conv2d(torch.cat([ax + ut, ut]), wt.abs(), padding=k // 2)
        A, extra = both[: x.shape[0]], both[x.shape[0]:]
    else:
        A, extra = F.conv2d(ax, wt.abs(), padding=k // 2), None
    E = gamma(K) * (A + bt.abs()[None, :, None, None])
    if relu:
        y = F.relu(y)
    if pool:
        y, E = F.max_pool2d(y, 2, 2), F.max_pool2d(E, 2, 2)
        extra = F.max_pool2d(extra, 2, 2) if extra is not None else None
    return y.numpy(), E.numpy(), (extra.numpy() if extra is not None else 0.0)


def check_layer(got, y, E, extra=0.0, f16_out: bool = True) -> dict:
    """Element-wise gate: |got - y| <= E + extra + ulp16(got) / 2 (the last term only for fp16 outputs, which must also be exactly
    representable in fp16).  Returns what an assertion message needs: ``ok``, the worst ratio of error to allowance and its
    (b, c, y, x), the number of violations, and the fraction of elements that differ from fp16(y) (fp32(y) for fp32 outputs)."""
    g = np.asarray(got, np.float64)
    y = np.asarray(y, np.float64)
    assert g.shape == y.shape, (g.shape, y.shape)
    allow = np.broadcast_to(np.asarray(E, np.float64) + extra, g.shape)
    representable = True
    if f16_out:
        representable = bool(np.array_equal(g.astype(np.float16).astype(np.float64), g, equal_nan=False))
        allow = allow + 0.5 * ulp16(g)
        rounded = y.astype(np.float16).astype(np.float64)
    else:
        rounded = y.astype(np.float32).astype(np.float64)
    err = np.abs(g - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allow > 0, err / allow, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(g), ratio, np.inf)
    i = int(np.argmax(ratio))
    return {"ok": representable and bool((ratio <= 1.0).all()), "representable": representable, "ratio": float(ratio.flat[i]),
            "where": tuple(int(v) for v in np.unravel_index(i, g.shape)), "violations": int((ratio > 1.0).sum()),
            "frac_ne": float((g != rounded).mean()), "got": float(g.flat[i]), "ref": float(y.flat[i])}


# ------------------------------------------------------------------------------------------------------------------------------
# conv1a (1 -> 64 channels, 3x3): the oracle's input, an fp64 reference, and what each of the kernel's three forms of it may add
# ------------------------------------------------------------------------------------------------------------------------------
def x_oracle(p: np.ndarray) -> np.ndarray:
    """float32(p) * float32(1/255), rounded once (cv::Mat::convertTo as oracle/superpoint_ref.py:preprocess_u8 restates it)."""
    return (np.asarray(p, np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)


def _h2f(h) -> np.ndarray:
    return np.asarray(h, np.float16).astype(np.float64)


def conv1a_u8_delta(w1a: np.ndarray, b1a: np.ndarray) -> np.ndarray:
    """[64] bound on |a_kernel - a| of the fused conv1a with operands straight from the bytes (OMNI_PP_U8=1, conv1a_pack_u8_weights),
    a = sum_t w_t x_t + b in exact arithmetic over the oracle's input x_t = fl32(p_t * fl32(1/255)).

    The kernel's operands: P_t = half(4 + p_t / 256) (= 0x4400 | p_t, exact) in both halves of a dword, against Wh_t and Wl_t, the split
    of W_t = fl32(w_t 256 / 255); the bias slot holds (1, 1) against the split (bh, bl) of fl32(b - 4 sum_t (Wh_t + Wl_t)).  With
    Weff_t = Wh_t + Wl_t and Beff = bh + bl the exact value of the kernel's 20 products is
        sum_t Weff_t (4 + p_t / 256) + Beff = sum_t Weff_t p_t / 256 + b + (Beff + 4 sum_t Weff_t - b),
    so  a_ideal - a = sum_t (Weff_t p_t / 256 - w_t x_t) + (Beff + 4 sum Weff - b).  Per tap the first term is at most its maximum over
    the 256 byte values (this also carries the difference between x_t = fl32(p) fl32(1/255) and p / 255, and the 2^-22-relative split of
    W_t); the second is one number per channel.  The products of two halfs are exact in fp32; the MFMAs add 20 terms (18 products and the
    two bias halves; zero operands add nothing) in fp32: gamma_20 (sum_t (|Wh_t| + |Wl_t|) (4 + 255 / 256) + |bh| + |bl|).
    Out-of-image and masked pixels read p = 0, the same value the oracle's zero padding / mask gives."""
    p = np.arange(256, dtype=np.float64)
    xo = x_oracle(np.arange(256)).astype(np.float64)
    w = np.asarray(w1a, np.float64).reshape(64, 9)
    b = np.asarray(b1a, np.float64)
    Wh, Wl, bh, bl = conv1a_u8_split(w1a, b1a)
    Weff, Beff = Wh + Wl, bh + bl
    dev_tap = np.abs(Weff[:, :, None] * p / 256.0 - w[:, :, None] * xo).max(2).sum(1)
    dev_bias = np.abs(Beff + 4.0 * Weff.sum(1) - b)
    rnd = gamma(20) * ((np.abs(Wh) + np.abs(Wl)).sum(1) * (4.0 + 255.0 / 256.0) + np.abs(bh) + np.abs(bl))
    return (dev_tap + dev_bias + rnd) * (1.0 + 1e-9)


def conv1a_u8_split(w1a: np.ndarray, b1a: np.ndarray):
    """conv1a_pack_u8_weights' halfs as float64: Wh, Wl [64, 9] = the split of fl32(w 256 / 255); bh, bl [64] = the split of
    fl32(b - 4 sum_t (Wh_t + Wl_t)) (the sum in double)."""
    w = np.asarray(w1a, np.float32).reshape(64, 9)
    b = np.asarray(b1a, np.float32)
    W = (w.astype(np.float64) * 256.0 / 255.0).astype(np.float32)
    Wh = f16(W)
    Wl = f16(W - Wh.astype(np.float32))
    S = (_h2f(Wh) + _h2f(Wl)).sum(1)
    bb = (b.astype(np.float64) - 4.0 * S).astype(np.float32)
    bh = f16(bb)
    bl = f16(bb - bh.astype(np.float32))
    return _h2f(Wh), _h2f(Wl), _h2f(bh), _h2f(bl)


def conv1a_table_delta(w1a: np.ndarray, b1a: np.ndarray) -> np.ndarray:
    """[64] the same bound for the table form (OMNI_PP_U8=0: conv1a_pack_split_weights + conv1a_make_split_lut).

    The table splits the oracle's own input, x_t = xh_t + xl_t + r_t (xh = half(x), xl = half(x - xh)), the weights w_t = wh_t + wl_t + s_t,
    the bias b = bh + bl + s_b.  The K slots pair up as wh xh + wh xl + wl xh per tap (wl xl is left out) and (bh, bl) against (1, 1), so
        a_ideal - a = sum_t (wh_t xh_t + wh_t xl_t + wl_t xh_t - w_t x_t) + (bh + bl - b),
    bounded per tap by its maximum over the 256 byte values.  The MFMAs add 29 exact products in fp32: gamma_29 times the largest sum of
    their magnitudes."""
    xo = x_oracle(np.arange(256))
    xh = f16(xo)
    xl = f16(xo - xh.astype(np.float32))
    xh64, xl64 = _h2f(xh), _h2f(xl)
    w = np.asarray(w1a, np.float32).reshape(64, 9)
    b = np.asarray(b1a, np.float32)
    wh = f16(w)
    wl = f16(w - wh.astype(np.float32))
    wh64, wl64 = _h2f(wh)[:, :, None], _h2f(wl)[:, :, None]
    ideal = wh64 * xh64 + wh64 * xl64 + wl64 * xh64
    dev_tap = np.abs(ideal - w.astype(np.float64)[:, :, None] * xo.astype(np.float64)).max(2).sum(1)
    bh = f16(b)
    bl = f16(b - bh.astype(np.float32))
    dev_bias = np.abs(_h2f(bh) + _h2f(bl) - b.astype(np.float64))
    mag = (np.abs(wh64 * xh64) + np.abs(wh64 * xl64) + np.abs(wl64 * xh64)).max(2).sum(1)
    rnd = gamma(29) * (mag + np.abs(_h2f(bh)) + np.abs(_h2f(bl)))
    return (dev_tap + dev_bias + rnd) * (1.0 + 1e-9)


def masked_u8(imgs: np.ndarray, fisheye_mask: bool) -> np.ndarray:
    g = np.array(imgs, np.uint8, copy=True)
    if fisheye_mask:
        h = g.shape[-2]
        g[..., h * 3 // 4: h * 3 // 4 + h // 4, :] = 0
    return g


@torch.no_grad()
def conv1a_ref(img_u8: np.ndarray, w1a, b1a) -> np.ndarray:
    """[N, 64, H, W] fp64 conv1a before the ReLU, over the oracle's input x = fl32(p) fl32(1/255) of the (already masked) image."""
    x = _t(x_oracle(img_u8).astype(np.float64)[:, None])
    return F.conv2d(x, _t(w1a), _t(b1a), padding=1).numpy()


def conv1a_interval(a: np.ndarray, delta: np.ndarray):
    """The fused kernel's conv1a activation lies in [fp16_down(relu(a - delta)), fp16_up(relu(a + delta))] whatever its rounding.
    Returns (x16, u_in): x16 = fp16(relu(a)) to nearest, the input conv1b's reference uses, and u_in = the interval's largest
    distance from x16, which conv_ref carries through conv1b as ``extra``."""
    d = np.asarray(delta, np.float64)[None, :, None, None]
    x16 = np.maximum(a, 0.0).astype(np.float16).astype(np.float64)
    lo = f16_down(np.maximum(a - d, 0.0))
    hi = f16_up(np.maximum(a + d, 0.0))
    return x16, np.maximum(hi - x16, x16 - lo)


# ------------------------------------------------------------------------------------------------------------------------------
# the two fp32 tails: detector head (semi) and dense descriptors
# ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def semi_ref(cpa16: np.ndarray, wPb: np.ndarray, bPb: np.ndarray, x_f32: bool = False, exact_f32: bool = False):
    """Heat map: (ref, bound), each [N, 8 Hc, 8 Wc] float64.  ref = the fp64 softmax over 65 of convPb(cPa16) + b without the dustbin,
    arranged depth-to-space, with the fp32 weights as given.

    Logits (detector_head_mfma16_kernel, weights from detector_pack_weights16): channel c < 64 sums the exact products of x_k with
    wh = half(w) and wl = half(w - wh), 2 x 256 terms, in fp32 MFMA accumulators, then adds the bias in fp32: K = 513 terms,
        E_c = sum_k |x_k| |w_ck - wh_ck - wl_ck| + gamma_513 (sum_k |x_k| (|wh_ck| + |wl_ck|) + |b_c|).
    The dustbin is an fmaf chain over the fp32 weights, two partial sums and the bias: E_64 = gamma_258 (sum_k |x_k w_k| + |b_64|).
    Softmax: logits off by d_j (|d_j| <= E_j) move p_c by the factor exp(d_c) / sum_j p_j exp(d_j), so |dp_c| <= p_c (exp(E_c + Emax) - 1).
    The fp32 evaluation (l - mx, expf, a sum of 65 positive terms, one division) adds a relative error of at most
        u |z_c - m| + 4 u  (the subtraction and expf, taken as 2 ulp)  +  u max_j |z_j - m| + 4 u + gamma_65  (the sum)  +  u  (the division),
    where |z - m| grows by 2 Emax in the computed logits.  Near the ends of fp32's range an absolute 1e-37 covers underflow.

    x_f32 (detector_head_mfma16_kernel<float>, OMNI_PREC_SPLIT: the input is the heads layer's fp32 output): the kernel splits the activation as well,
    xh = half(x), xl = half(x - xh), and adds wl xh + wh xh + wh xl, 3 x 256 exact products and the bias, K = 769.  Against z = sum_k w_k x_k + b this
    leaves out exactly (w - wh - wl) x + wh (x - xh - xl) + wl (x - xh), each bounded by its magnitude:
        E_c = sum_k |x_k| |w - wh - wl| + |wh| |x_k - xh_k - xl_k| + |wl| |x_k - xh_k|  +  gamma_769 (sum_k |xh_k| (|wh| + |wl|) + |xl_k| |wh| + |b_c|).
    exact_f32 (detector_head_mfma: v_mfma_f32_32x32x2_f32 over the fp32 weights; OMNI_PREC_F32 and OMNI_DET16=0): every product rounded into the fp32
    accumulator, then the bias: E_c = gamma_258 (sum_k |x_k w_ck| + |b_c|) for all 65 channels."""
    x = _t(cpa16)
    w = np.asarray(wPb, np.float32).reshape(65, 256)
    wh = f16(w)
    wl = f16(w - wh.astype(np.float32))
    wh64, wl64 = _h2f(wh), _h2f(wl)
    rep = np.abs(w.astype(np.float64) - wh64 - wl64)
    rep[64] = 0.0
    mag = np.abs(wh64) + np.abs(wl64)
    mag[64] = np.abs(w[64].astype(np.float64))
    conv1 = lambda inp, ww: torch.einsum("nkhw,ck->nchw", inp, _t(ww))
    z = conv1(x, w.astype(np.float64)) + _t(bPb)[None, :, None, None]
    ax = x.abs()
    g = np.full(65, gamma(513))
    g[64] = gamma(258)
    Ez = conv1(ax, rep) + _t(g)[None, :, None, None] * (conv1(ax, mag) + _t(np.abs(bPb))[None, :, None, None])
    if exact_f32:
        Ez = gamma(258) * (conv1(ax, np.abs(w.astype(np.float64))) + _t(np.abs(bPb))[None, :, None, None])
    elif x_f32:
        x32 = np.asarray(cpa16, np.float32)
        xh = x32.astype(np.float16).astype(np.float32)
        xl = (x32 - xh).astype(np.float16).astype(np.float32)
        axh, axl = _t(np.abs(xh)), _t(np.abs(xl))
        r1, r2 = _t(np.abs(x32.astype(np.float64) - xh - xl)), _t(np.abs(x32.astype(np.float64) - xh))
        awh, awl = np.abs(wh64), np.abs(wl64)                 # (row 64, the dustbin, is overwritten below)
        Ez = (conv1(ax, rep) + conv1(r1, awh) + conv1(r2, awl)
              + gamma(769) * (conv1(axh, mag) + conv1(axl, awh) + _t(np.abs(bPb))[None, :, None, None]))
        Ez[:, 64] = gamma(258) * (conv1(ax, mag)[:, 64] + abs(float(np.asarray(bPb)[64])))
    p = torch.softmax(z, 1)
    Emax = Ez.max(1, keepdim=True).values
    prop = p * torch.expm1(Ez + Emax)
    m = z.max(1, keepdim=True).values
    dz = (z - m).abs() + 2 * Emax
    rel = U * dz + 4 * U + U * dz.max(1, keepdim=True).values + 4 * U + gamma(65) + U
    bound = prop + (p + prop) * rel * 1.001 + 1e-37
    def d2s(t):
        t = t[:, :64]
        n, _, hc, wc = t.shape
        return t.permute(0, 2, 3, 1).reshape(n, hc, wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(n, hc * 8, wc * 8).numpy()
    return d2s(p), d2s(bound)


@torch.no_grad()
def desc_ref(cda16: np.ndarray, wDb: np.ndarray, bDb: np.ndarray, round_w: bool = True, split: bool = False):
    """Dense descriptors: (ref, bound), each [N, 256, Hc, Wc] float64.  ref = the fp64 normalize(convDb(cDa16; fp16(wDb)) + b).

    convdb_l2norm_kernel (weights from convdb_pack_weights, rounded to nearest fp16): v_c = 256 exact products summed in fp32 MFMA
    accumulators, then + b_c in fp32: |v_c - d_c| <= E_c = gamma_257 (sum_k |x_k w16_ck| + |b_c|).  With e = v - d, ||e|| <= ||E||:
        |v_c / ||v|| - d_c / ||d||| <= (E_c + |ref_c| ||E||) / (||d|| - ||E||)
    (v_c/||v|| - d_c/||d|| = e_c / ||v|| + d_c (||d|| - ||v||) / (||v|| ||d||)).  The norm is evaluated in fp32: 256 non-negative squares
    (fmaf) summed: relative gamma_256, halved by the square root; sqrtf and the division round once each (correctly rounded: the build
    keeps HIP's default correctly rounded fp32 division and square root).  A cell whose ||d|| <= ||E|| has no bound (inf).

    round_w=False (the fp32-class paths' dense map: the exact-f32 1x1 convolution over the fp32 cDa with the weights as given, then l2norm_kernel):
    256 products rounded into the fp32 accumulator and the bias, the same gamma_257; the norm's 256 squares are summed in a tree: within gamma_256.

    split=True (convdb_l2norm_split_kernel, the sparse tail of OMNI_PREC_SPLIT over the compact fp32 cDa rows, given as [rows, 256, 1, 1]): xh = half(x),
    xl = half(x - xh), wh = half(w), wl = half(w - wh) (convdb_pack_weights_split); the kernel adds wl xh + wh xh + wh xl, 3 x 256 exact products in fp32 MFMA
    accumulators, then the bias: d is the exact value of THAT sum (the dropped wl xl, the residues w - wh - wl and x - xh - xl are in the reference) and
    E_c = gamma_769 (sum_k |xh_k| (|wh_ck| + |wl_ck|) + |xl_k| |wh_ck| + |b_c|); the norm as above (fmaf chains of 16, then a tree: within gamma_256)."""
    x = _t(cda16)
    w16 = np.asarray(wDb, np.float32).reshape(256, 256).astype(np.float64)
    if round_w:
        w16 = f16(w16).astype(np.float64)
    conv1 = lambda inp, ww: torch.einsum("nkhw,ck->nchw", inp, _t(ww))
    bt = _t(bDb)[None, :, None, None]
    if split:
        x32, w32 = np.asarray(cda16, np.float32), np.asarray(wDb, np.float32).reshape(256, 256)
        xh = x32.astype(np.float16).astype(np.float32)
        xl = (x32 - xh).astype(np.float16).astype(np.float64)
        wh = w32.astype(np.float16).astype(np.float32)
        wl = (w32 - wh).astype(np.float16).astype(np.float64)
        xh, wh = xh.astype(np.float64), wh.astype(np.float64)
        d = conv1(_t(xh), wh + wl) + conv1(_t(xl), wh) + bt
        E = gamma(769) * (conv1(_t(np.abs(xh)), np.abs(wh) + np.abs(wl)) + conv1(_t(np.abs(xl)), np.abs(wh)) + bt.abs())
    else:
        d = conv1(x, w16) + bt
        E = gamma(257) * (conv1(x.abs(), np.abs(w16)) + bt.abs())
    n = d.norm(dim=1, keepdim=True)
    En = E.norm(dim=1, keepdim=True)
    ref = d / n
    den = n - En
    prop = torch.where(den > 0, (E + ref.abs() * En) / den.clamp_min(1e-300), torch.full_like(E, np.inf))
    bound = prop + (ref.abs() + prop) * (gamma(256) / 2 + 3 * U) * 1.001 + 1e-37
    return ref.numpy(), bound.numpy()
