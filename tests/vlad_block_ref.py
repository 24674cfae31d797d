"""fp64 references and arithmetic error bounds for MobileNetVLAD, block by block (csrc/vlad.hip, vlad_s.hip, vlad_h.hip), in the style of
tests/f16_layer_ref.py (whose ``gamma``, ``ulp16`` and ``check_layer`` are used here).

Every stage is recomputed in float64 from the kernel's own stored input -- the previous tap of ``omni_vlad_debug_layer``, or the u8 image for the
stem and block 0 -- so the errors of earlier blocks do not enter, and the difference may only be what the kernel's arithmetic allows.  Each function
returns (y, E): the fp64 value over the fp32 operands (weights as given, input as stored) and a per-element allowance, gated with
``check_layer(got, y, E, f16_out=False)``: |got - y| <= E.  Also in OMNI_PREC_F16 the blocks' outputs are fp32 tensors; there y is the fp64 value over
the operands rounded as vlad_h.hip states, see below.

Sums, order unknown.  A sum of K terms evaluated in fp32 with round-to-nearest, in any order, with or without fused multiply-adds, is within
gamma_K sum |term| of the exact sum, gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1);
where every term passes through at most h additions, gamma_h (section 4.2).  This is path "any" for the three stages of a block (what an fp32 evaluation in an
unknown order, such as the oracle's torch layers, must meet), and what the stem, the depthwise stage and the head use.  At the deep blocks it is too loose
to be a gate: gamma_338 over block 16's projection, carried through the stages, allows 1.4e-4 of an output or more, and a column or channel that is off by
1e-4 passes (tests/test_vlad_block_ref_cpu.py).

Sums, order known (``run_sum``).  The two pointwise stages of a block are therefore bounded along the order in which the kernel adds: an instruction that adds
the products of a group G to an accumulator a rounds at most |G| times, and every partial result lies within |a| + sum_G |product| (+ how far the kernel's
accumulator may lie from the reference's), so it adds at most gamma_|G| (|a| + sum_G |product|); a, the exact partial sum at that point, is computed here.
Every later single addition (partial tiles of a K split, the bias, the residual) adds u |its result|.  The orders, read from the kernels:
  "valu"      vlad_block_kernel: expand = the bias, then one fmaf per input channel, ascending; projection = one fmaf per hidden channel, ascending, over the
              chunks (padded channels carry zero weights: exact), then + bias, + residual.  The stem kernels and block 0 are short sums (K = 10, 10, 17): gamma_K.
  "layers"    vlad_pw_kernel (OMNI_VLAD_UNFUSED): as "valu" with the bias added last in the expand stage too.
  "mblock"    vlad_mblock_kernel: v_mfma_f32_32x32x2_f32 adds the products of channels (2 j, 2 j + 1) per instruction (an fmaf chain: two roundings), ascending;
              with OMNI_VLAD_MBLOCK_CPW = c one such chain per group of 32 c hidden channels, the groups added in order (vlad_mblock_reduce_kernel), then bias, residual.
  "pw_mfma3"  vlad_pw_mfma_kernel<SPLITK> (SPLITK = 4 from 128 input channels on): wave w takes its K range [ks, ke), an instruction adds the products of
              channels ks + t and ks + nk + t (the two half-waves, nk = (ke - ks) / 2); the waves' tiles are added in order, then bias (ReLU6 | residual).
  "split"     vlad_sblock_kernel, below: v_mfma_f32_32x32x16_f16, taken as its definition D = A B + C reads: the dot product of 16 exact products is summed in
              fp32, in any order (15 roundings, every partial sum within [-sum of the negative products, sum of the positive ones]), and that sum is added
              to the accumulator once (one rounding of |a + S|).  Sixteen roundings of the accumulator per instruction -- each product added to it in turn --
              would be the other extreme; with it the expand stage's twelve instructions alone allow 3e-4 of block 16's outputs and a channel that is
              off by 1e-4 passes, so the gate states the narrower reading and the MI355X run of tests/test_gpu_vlad_blocks.py is what confirms it.
  "f16"       vlad_hblock_kernel, below: the same instruction over [half(x) | 1 1] and over the hidden channels in steps of 16, ascending.

One block = three stages, each a sum:
  expand     h = ReLU6(sum_k x_k We_k + be)                  (absent in block 0: h = x)
  depthwise  d = ReLU6(sum_t h_t Wd_t + bd)                  ten terms in fp32 on every path (gamma_10), 3x3, padding 1 (zeros outside the EXPANDED map), stride 1 or 2
  project    y = sum_k d_k Wp_k + bp (+ x, the residual)
Across stages an error is carried as an interval per element: a stage whose inputs are each within e_i of the reference's moves by at most
sum_i |w_i| e_i (zero for the padding, which is exact; the stride-2 taps pick the e_i they read), and ReLU6 maps the interval [v - e, v + e] onto
[ReLU6(v - e), ReLU6(v + e)], never wider (1-Lipschitz), and to a point where the whole interval lies below 0 or above 6.

The stem reads p as (p - 128) / 128 (exact in fp32; the rows of omni_fisheye_mask_rows read p = 0) against weights folded over the three identical input
channels at create time, fl(fl(w_0 + w_1) + w_2) in fp32: that folded weight is the operand.

VB_SBLOCK (vlad_sblock_kernel, vlad_s.hip:5-16), path "split".  The block's input x is known exactly, so its halves x_hi = half(x), x_lo = half(x - x_hi)
are too, and so are those of We, be and Wp.  The expand stage forms the exact products x_hi We_hi, x_lo We_hi, be_hi, be_lo (slots [x_hi | x_lo | 1 1] in
S1 = ceil((2 cin + 2) / 16) instructions) and x_hi We_lo (S2 = ceil(cin / 16) more); lo.lo is left out.  Its exact value h_s is computed here in fp64 and
|h_s - h| is part of the allowance -- a number, not a bound: it carries the representation error of every operand, the dropped term and fp16's subnormal
floor of x_lo as they are for this input.  The depthwise stage is plain fp32.  The projection splits the kernel's own fp32 d, which is only known to
within its interval e: d_hi = half(d), |d - d_hi| <= 2^-11 |d| + 2^-25 (the second term where d_hi is subnormal), d_lo = half(d - d_hi),
|d - d_hi - d_lo| <= 2^-22 |d| + 2^-25, so with r_w = Wp - Wp_hi - Wp_lo
    |sum_k d Wp - (d_hi Wp_hi + d_lo Wp_hi + d_hi Wp_lo)| <= sum_k (2^-22 |d| + 2^-25) |Wp_hi| + |d| |r_w| + (2^-11 |d| + 2^-25) |Wp_lo|,  |d| <= d_ref + e,
and per 16 hidden channels three instructions (Wp_hi d_hi, Wp_hi d_lo, Wp_lo d_hi) whose accumulators are taken from the reference's split of d, off by at
most sum |Wp| e + 2^-9 sum |d Wp| + 2^-23 sum |Wp| from the kernel's (a d that differs moves d_hi by up to one fp16 step).  The gate stays against the
fp64 value over the fp32 operands: "fp32-class" is what it certifies.

VB_HBLOCK (vlad_hblock_kernel, vlad_h.hip:8-12), path "f16".  Rounded to nearest fp16: the block's input, We and Wp (at pack time), and h and d as
stored in LDS; be rides as be_hi + be_lo; accumulations, Wd, bd, bp and the residual (the unrounded fp32 x) are fp32.  y is the fp64 value with exactly these
roundings.  The kernel's fp32 value before a rounding is known to within its interval; rounding to nearest is monotonic, so the stored half lies in
[half(v - e), half(v + e)] -- one point for most elements, two neighbouring halves where the interval straddles a rounding boundary (the technique of
f16_layer_ref.conv1a_interval, with rounding to nearest at the ends because __builtin_convertvector rounds to nearest even).

Head.  Logits z_k = sum_d f_d A_kd + a_k: K = D + 1.  Softmax as in f16_layer_ref.semi_ref: logits off by at most E move p_k by at most
p_k (exp(E_k + E_max) - 1); the evaluation (the subtraction of the maximum, expf taken as 2 ulp as there, K positive terms summed, one correctly rounded
division: the build has no fast-math flag) adds the relative u |z_k - m| + 4 u + u max |z - m| + 4 u + gamma_K + u.  Aggregation
V_kd = sum_p a_pk (c_kd - f_pd): each difference is rounded once, then P terms: gamma_(P + 2) sum |a| |c - f|.  A normalisation v / ||v|| of a vector known to
within E (f16_layer_ref.desc_ref): (E_c + |ref_c| ||E||) / (||v|| - ||E||), plus its evaluation: n squares summed (relative gamma_(n + 1), halved by the
root), a correctly rounded sqrtf and division.  "vlad" is the aggregation followed by the intra-normalisation over D and the L2 normalisation over K D;
"out" is the FC (gamma of the most additions a product passes through, FC_DEPTH below) followed by the L2 normalisation over its outputs.  No term of the
head is measured.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mobilenetvlad_ref as V
from tests.f16_layer_ref import U, check_layer, gamma, masked_u8, ulp16  # noqa: F401  (check_layer, ulp16: for the tests that import this module)



def _t(a) -> torch.Tensor:
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _h(a) -> torch.Tensor:
    """Round to nearest fp16 (one rounding, from float64), as float64."""
    return _t(a).to(torch.float16).to(torch.float64)


def split16(a):
    """(hi, lo) of fp32 values as the packers and kernels split them: hi = half(v), lo = half(v - hi) (v - hi is exact in fp32)."""
    v = _t(np.asarray(a, np.float32).astype(np.float64))
    hi = _h(v)
    return hi, _h(v - hi)


def _pw(x, w):
    return torch.einsum("nkhw,ck->nchw", x, w)


def _dw(x, w, stride):
    return F.conv2d(x, w[:, None], stride=stride, padding=1, groups=x.shape[1])


def _c(v):
    return v[None, :, None, None]


def _relu6_iv(v, e):
    """ReLU6 of a value known to within e: (ReLU6(v), the interval's largest distance from it)."""
    r = v.clamp(0.0, 6.0)
    return r, torch.maximum((v + e).clamp(0.0, 6.0) - r, r - (v - e).clamp(0.0, 6.0))


def _half_iv(v, e):
    """The half a value known to within e is stored as: (half(v), the largest distance of [half(v - e), half(v + e)] from it)."""
    r = _h(v)
    return r, torch.maximum(_h(v + e) - r, r - _h(v - e))


def block_weights(weights, block: int) -> dict:
    """Block ``block`` of the oracle's layer table as float64 tensors: we [hid, cin] / be (None for block 0), wd [hid, 3, 3] / bd, wp [cout, hid] / bp,
    stride, res."""
    specs = {n: (kind, cin, cout, s) for n, kind, cin, cout, s in V.layer_specs()}
    g = lambda n: np.asarray(weights[n], np.float32)
    p = f"b{block}."
    out = {"stride": specs[p + "dw"][3], "res": specs[p + "project"][0] == "pw_linear_res", "we": None, "be": None}
    if p + "expand" in specs:
        out["we"], out["be"] = g(p + "expand.weight").reshape(specs[p + "expand"][2], -1), g(p + "expand.bias")
    out["wd"], out["bd"] = g(p + "dw.weight").reshape(-1, 3, 3), g(p + "dw.bias")
    out["wp"], out["bp"] = g(p + "project.weight").reshape(specs[p + "project"][2], -1), g(p + "project.bias")
    return out


def _chunks(idx, g):
    idx = np.asarray(idx)
    return [idx[i:i + g] for i in range(0, len(idx), g)]


def _zeros(like, n):
    """n zero slots along dimension 1"""
    shape = list(like.shape)
    shape[1] = n
    return torch.zeros(shape, dtype=like.dtype)


def mfma3_chains(K: int):
    """vlad_pw_mfma_kernel<SPLITK>: wave w takes K range [ks, ke), its two half-waves the two contiguous halves; one MFMA adds products ks + t and ks + nk + t."""
    sk = 4 if K >= 128 else 1
    kq = (K + sk * 8 - 1) // (sk * 8) * 8
    chains = []
    for w in range(sk):
        ks = min(w * kq, K)
        ke = min(ks + kq, K)
        nk = (ke - ks) // 2
        if nk:
            chains.append([np.array([ks + t, ks + nk + t]) for t in range(nk)])
    return chains


def expand_order(path: str, cin: int):
    """(bias first?, chains) of the expand stage's cin products on an exact-f32 path; the bias is the accumulator's first value or the one term of the tail."""
    k = np.arange(cin)
    if path == "valu":
        return True, [_chunks(k, 1)]
    if path == "layers":
        return False, [_chunks(k, 1)]
    if path == "mblock":
        return False, [_chunks(k, 2)]
    return False, mfma3_chains(cin)


def project_order(path: str, hid: int, cpw: int = 0):
    """Chains of the projection's hid products on an exact-f32 path (tail: bias, then the residual)."""
    k = np.arange(hid)
    if path in ("valu", "layers"):
        return [_chunks(k, 1)]
    if path == "mblock":
        per = 32 * cpw if cpw > 0 else hid
        return [_chunks(k[i:i + per], 2) for i in range(0, hid, per)]
    return mfma3_chains(hid)


def run_sum(A, W, chains, init=None, tail=(), unc=0.0, eval32=None, dot=False):
    """The ordered sum out[n, c] = init + sum_k A[n, k] W[c, k] + tail as a kernel evaluates it: per chain an accumulator that starts at ``init`` (first
    chain; exact) or 0 and takes one group of slots G per instruction, the chains' totals added in order, then the tail's terms one by one.
    Returns (exact value, bound): with ``dot`` an instruction is a dot product in fp32 plus one addition to the accumulator (the module's docstring, "split");
    otherwise an instruction that adds g products to an accumulator a rounds at most g times, each partial result at most
    |a| + sum_G |A W| (+ unc, how far any partial result of the kernel may lie from the reference's) in magnitude: gamma_g of that; every later
    single addition u |result|.  A [N, K, H, W], W [C, K] float64; eval32: a callable (a, A_G, W_G) -> a' that evaluates one instruction in float32 (the CPU
    stand-ins: then the float32 result is returned in place of the bound)."""
    E = 0.0
    totals = []
    for ci, chain in enumerate(chains):
        a = init if ci == 0 else None
        a32 = None if a is None or eval32 is None else a.to(torch.float32)
        for G in chain:
            Ag, Wg = A[:, G], W[:, G]
            if eval32 is not None:
                a32 = eval32(a32, Ag, Wg)
                continue
            S = _pw(Ag, Wg)
            if dot:                                              # D = A B + C: the dot product in fp32 (any order), then one addition to the accumulator
                Ap, An, Wp_, Wn = Ag.clamp_min(0.0), (-Ag).clamp_min(0.0), Wg.clamp_min(0.0), (-Wg).clamp_min(0.0)
                pos, neg = _pw(Ap, Wp_) + _pw(An, Wn), _pw(Ap, Wn) + _pw(An, Wp_)       # every partial sum of the products lies in [-neg, pos]
                E = E + gamma(len(G) - 1) * (torch.maximum(pos, neg) + unc)
                a = S if a is None else a + S
                E = E + U * (a.abs() + unc)
                continue
            E = E + gamma(len(G)) * ((a.abs() if a is not None else 0.0) + _pw(Ag.abs(), Wg.abs()) + unc)
            a = S if a is None else a + S
        totals.append(a32 if eval32 is not None else a)
    run = totals[0]
    for t in list(totals[1:]) + list(tail):
        if eval32 is not None:
            run = run + t.to(torch.float32)
        else:
            run = run + t
            E = E + U * (run.abs() + unc)
    return run if eval32 is not None else (run, E * 1.001)


def split_expand_ops(x, B):
    """vlad_sblock_kernel's expand as slots: [x_hi | x_lo | 1 1 | 0 ..] against [We_hi | We_hi | be_hi be_lo | 0 ..] in S1 steps of 16, then x_hi against We_lo in
    S2 steps of 16 (vlad_s.hip SBlockCfg)."""
    (xh, xl), (wh, wl), (bh, bl) = split16(x), split16(B["we"]), split16(B["be"])
    cin = xh.shape[1]
    s1, s2 = (2 * cin + 2 + 15) // 16, (cin + 15) // 16
    A = torch.cat([xh, xl, torch.ones_like(xh[:, :2]), _zeros(xh, s1 * 16 - 2 * cin - 2), xh, _zeros(xh, s2 * 16 - cin)], 1)
    Wt = torch.cat([wh, wh, bh[:, None], bl[:, None], _zeros(wh, s1 * 16 - 2 * cin - 2), wl, _zeros(wh, s2 * 16 - cin)], 1)
    return A, Wt, [_chunks(np.arange((s1 + s2) * 16), 16)]


def f16_expand_ops(x, B):
    """vlad_hblock_kernel's expand as slots: [half(x) | 1 1 | 0 ..] against [half(We) | be_hi be_lo | 0 ..] in KS steps of 16."""
    x16, w16 = _h(x), _h(_t(B["we"]))
    bh, bl = split16(B["be"])
    cin = x16.shape[1]
    ks = (cin + 2 + 15) // 16
    pad = ks * 16 - cin - 2
    A = torch.cat([x16, torch.ones_like(x16[:, :2]), _zeros(x16, pad)], 1)
    Wt = torch.cat([w16, bh[:, None], bl[:, None], _zeros(w16, pad)], 1)
    return A, Wt, [_chunks(np.arange(ks * 16), 16)]


def split_project_ops(d, B):
    """vlad_sblock_kernel's projection as slots: per 16 hidden channels three instructions, Wp_hi d_hi, Wp_hi d_lo, Wp_lo d_hi."""
    dh, dl = split16(d.to(torch.float32).numpy())
    wh, wl = split16(B["wp"])
    hid = dh.shape[1]
    A, Wt = torch.cat([dh, dl, dh], 1), torch.cat([wh, wh, wl], 1)
    chain = []
    for j in range(0, hid, 16):
        k = np.arange(j, min(j + 16, hid))
        chain += [k, hid + k, 2 * hid + k]
    return A, Wt, [chain]


PATHS = ("any", "valu", "layers", "mblock", "pw_mfma3", "split", "f16")


@torch.no_grad()
def block_ref(x, weights, block: int, path: str = "any", cpw: int = 0):
    """One inverted-residual block from its stored input x [N, cin, H, W] (fp32 values): (y, E), each [N, cout, H', W'] float64.
    path: the kernel whose arithmetic the allowance is for -- "valu" (vlad_block_kernel), "layers" (the layer-by-layer kernels), "mblock"
    (vlad_mblock_kernel; cpw = OMNI_VLAD_MBLOCK_CPW), "pw_mfma3", "split" (vlad_sblock_kernel), "f16" (vlad_hblock_kernel), or "any": an fp32
    evaluation in an unknown order (gamma_K over every stage)."""
    assert path in PATHS
    B = block_weights(weights, block)
    s = B["stride"]
    x = _t(np.asarray(x, np.float32).astype(np.float64))
    wd, bd, bp, wp = _t(B["wd"]), _t(B["bd"]), _t(B["bp"]), _t(B["wp"])
    hid, cin = wd.shape[0], x.shape[1]
    if B["we"] is None:
        if path in ("split", "f16", "mblock", "pw_mfma3"):
            path = "valu"                                        # block 0 has no matrix-core form (VB_VALU at every precision)
        h, e1 = x, torch.zeros_like(x)
    elif path == "any":
        we, be = _t(B["we"]), _t(B["be"])
        pre = _pw(x, we) + _c(be)
        h, e1 = _relu6_iv(pre, gamma(cin + 1) * (_pw(x.abs(), we.abs()) + _c(be.abs())))
    elif path == "split":
        A, Wt, chains = split_expand_ops(x, B)
        pre_s, e = run_sum(A, Wt, chains, dot=True)
        pre = _pw(x, _t(B["we"])) + _c(_t(B["be"]))
        h, e1 = _relu6_iv(pre, (pre_s - pre).abs() + e)
    elif path == "f16":
        A, Wt, chains = f16_expand_ops(x, B)
        pre, e = run_sum(A, Wt, chains, dot=True)
        h, e1 = _half_iv(*_relu6_iv(pre, e))
    else:
        we, be = _t(B["we"]), _t(B["be"])
        first, chains = expand_order(path, cin)
        bias = _c(be).expand(x.shape[0], -1, x.shape[2], x.shape[3])
        pre, e = run_sum(x, we, chains, init=bias if first else None, tail=() if first else (bias,))
        h, e1 = _relu6_iv(pre, e)
    # depthwise: fp32 on every path, ten terms
    pre = _dw(h, wd, s) + _c(bd)
    d, e2 = _relu6_iv(pre, _dw(e1, wd.abs(), s) + gamma(10) * (_dw(h.abs() + e1, wd.abs(), s) + _c(bd.abs())))
    y = _pw(d, wp) + _c(bp) + (x if B["res"] else 0.0)
    tail = [_c(bp).expand_as(y)] + ([x] if B["res"] else [])
    prop = _pw(e2, wp.abs())
    if path == "any":
        E = prop + gamma(hid + 2) * (_pw(d.abs() + e2, wp.abs()) + _c(bp.abs()) + (x.abs() if B["res"] else 0.0))
    elif path == "split":
        wh, wl = split16(B["wp"])
        dm = d.abs() + e2
        dev = _pw(2.0 ** -22 * dm + 2.0 ** -25, wh.abs()) + _pw(dm, (wp - wh - wl).abs()) + _pw(2.0 ** -11 * dm + 2.0 ** -25, wl.abs())
        A, Wt, chains = split_project_ops(d, B)
        unc = prop * (1 + 2.0 ** -9) + 2.0 ** -9 * _pw(d.abs(), wp.abs()) + 2.0 ** -23 * wp.abs().sum(1)[None, :, None, None]
        _, e = run_sum(A, Wt, chains, tail=tail, unc=unc, dot=True)
        E = prop + dev + e
    elif path == "f16":
        d16, ed = _half_iv(d, e2)
        w16 = _h(wp)
        prop = _pw(ed, w16.abs())
        y, e = run_sum(d16, w16, [_chunks(np.arange(hid), 16)], tail=tail, unc=prop, dot=True)
        E = prop + e
    else:
        _, e = run_sum(d, wp, project_order(path, hid, cpw), tail=tail, unc=prop)
        E = prop + e
    return y.numpy(), (E * (1.0 + 1e-9)).numpy()


def stem_weights(weights):
    """The stem's weights folded over the three identical input channels as omni_vlad_create folds them (fp32: 0 + w_0, + w_1, + w_2): [16, 3, 3], and the bias."""
    w = np.asarray(weights["stem.weight"], np.float32)
    f = np.zeros((w.shape[0], 3, 3), np.float32)
    for ci in range(w.shape[1]):
        f = (f + w[:, ci]).astype(np.float32)
    return f, np.asarray(weights["stem.bias"], np.float32)


@torch.no_grad()
def stem_ref(img_u8, mask: bool, weights):
    """The stem from the image [N, H, W] u8 (the fisheye rows blanked here when ``mask``): (y, E), [N, 16, ceil(H / 2), ceil(W / 2)]."""
    wf, b = stem_weights(weights)
    g = masked_u8(np.asarray(img_u8), mask)
    x = _t((g.astype(np.float64) - 128.0) / 128.0)[:, None]
    w, bt = _t(wf)[:, None], _t(b)
    pre = F.conv2d(x, w, bt, stride=2, padding=1)
    y, e = _relu6_iv(pre, gamma(10) * (F.conv2d(x.abs(), w.abs(), bt.abs(), stride=2, padding=1)))
    return y.numpy(), (e * (1.0 + 1e-9)).numpy()


@torch.no_grad()
def stem_b0_ref(img_u8, mask: bool, weights):
    """Stem + block 0 in one kernel (vlad_stem_b0_kernel), from the image: (y, E), [N, 8, ceil(H / 2), ceil(W / 2)].  The stem map is not stored: its interval
    is carried through block 0's two stages."""
    st, e0 = stem_ref(img_u8, mask, weights)
    B = block_weights(weights, 0)
    wd, bd, wp, bp = _t(B["wd"]), _t(B["bd"]), _t(B["wp"]), _t(B["bp"])
    h, e1 = _t(st), _t(e0)
    pre = _dw(h, wd, 1) + _c(bd)
    d, e2 = _relu6_iv(pre, _dw(e1, wd.abs(), 1) + gamma(10) * (_dw(h + e1, wd.abs(), 1) + _c(bd.abs())))
    y = _pw(d, wp) + _c(bp)
    E = _pw(e2, wp.abs()) + gamma(wd.shape[0] + 1) * (_pw(d + e2, wp.abs()) + _c(bp.abs()))
    return y.numpy(), (E * (1.0 + 1e-9)).numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# the NetVLAD head
# ------------------------------------------------------------------------------------------------------------------------------
def _normalise(v, E, dim, n_terms):
    """v / ||v|| over ``dim`` for v known to within E, evaluated in fp32 with n_terms squares: (ref, bound)."""
    n = v.norm(dim=dim, keepdim=True)
    En = E.norm(dim=dim, keepdim=True)
    ref = v / n
    den = n - En
    prop = torch.where(den > 0, (E + ref.abs() * En) / den.clamp_min(1e-300), torch.full_like(E, np.inf))
    return ref, prop + (ref.abs() + prop) * (gamma(n_terms + 1) / 2 + 3 * U) * 1.001 + 1e-37


@torch.no_grad()
def assign_ref(feat, weights):
    """Soft assignment from the backbone's stored output feat [N, D, hf, wf]: (a, E), [N, K, hf, wf]."""
    f = _t(np.asarray(feat, np.float32).astype(np.float64))
    aw = _t(np.asarray(weights["vlad.assign.weight"], np.float32).reshape(V.N_CLUSTERS, -1))
    ab = _t(np.asarray(weights["vlad.assign.bias"], np.float32))
    K, D = aw.shape
    z = _pw(f, aw) + _c(ab)
    Ez = gamma(D + 1) * (_pw(f.abs(), aw.abs()) + _c(ab.abs()))
    p = torch.softmax(z, 1)
    Emax = Ez.max(1, keepdim=True).values
    prop = p * torch.expm1(Ez + Emax)
    dz = (z - z.max(1, keepdim=True).values).abs() + 2 * Emax
    rel = U * dz + 4 * U + U * dz.max(1, keepdim=True).values + 4 * U + gamma(K) + U
    return p.numpy(), (prop + (p + prop) * rel * 1.001 + 1e-37).numpy()


@torch.no_grad()
def vlad_ref(feat, assign, weights):
    """The normalised NetVLAD vector from the stored feat [N, D, hf, wf] and the stored assignment [N, K, hf, wf]: (v, E), [N, K D, 1, 1], k-major."""
    f = _t(np.asarray(feat, np.float32).astype(np.float64)).flatten(2)             # [N, D, P]
    a = _t(np.asarray(assign, np.float32).astype(np.float64)).flatten(2)           # [N, K, P]
    c = _t(np.asarray(weights["vlad.clusters"], np.float32))                       # [K, D]
    N, D, P = f.shape
    K = a.shape[1]
    v = a.sum(-1, keepdim=True) * c[None] - torch.einsum("nkp,ndp->nkd", a, f)
    mag = torch.zeros_like(v)
    for k in range(K):                                                             # sum_p |a_pk| |c_kd - f_pd|
        mag[:, k] = ((c[k][None, :, None] - f).abs() * a[:, k][:, None, :].abs()).sum(-1)
    u1, B1 = _normalise(v, gamma(P + 2) * mag, 2, D)
    u2, B2 = _normalise(u1.reshape(N, K * D), B1.reshape(N, K * D), 1, K * D)
    return u2.reshape(N, K * D, 1, 1).numpy(), B2.reshape(N, K * D, 1, 1).numpy()


# The most additions any product of the FC passes through (a sum evaluated as a tree of that height is within gamma_height sum |term|, Higham section 4.2).
# vlad_fc_mfma_kernel, K D = 3584: a wave's chain is 14 groups x 4 instructions of two products each (2 + 55), then 3 additions over the waves of a workgroup,
# 7 over the K split's workgroups (vlad_fc_finish_kernel) and the bias: 68.  vlad_fc4_kernel / vlad_fc_kernel: a lane's chain of 3584 / 64 = 56 fmaf, six
# shuffle additions and the bias: 63.
FC_DEPTH = 68


@torch.no_grad()
def fc_ref(vlad, weights):
    """The descriptor from the stored NetVLAD vector [N, K D, 1, 1]: (y, E), [N, out_dim, 1, 1]."""
    v = _t(np.asarray(vlad, np.float32).astype(np.float64)).flatten(1)
    w = _t(np.asarray(weights["fc.weight"], np.float32))
    b = _t(np.asarray(weights["fc.bias"], np.float32))
    y = v @ w.T + b
    E = gamma(FC_DEPTH) * (v.abs() @ w.abs().T + b.abs())
    r, Bn = _normalise(y, E, 1, y.shape[1])
    return r[:, :, None, None].numpy(), Bn[:, :, None, None].numpy()
