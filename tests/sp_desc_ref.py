"""fp64 references, derived error bounds and float32 emulations for the SuperPoint descriptor tail (csrc/sp_post.hip, computeDescriptors,
superpoint_tensorrt.cpp:192-230), beside tests/f16_layer_ref.py and tests/index_scan_ref.py (whose gamma, Ref, tier1 and tier2 are used here).  numpy and
torch in float64 on the CPU; the library is not imported.

Every stage is recomputed FROM THE KERNEL'S OWN INPUT TO THAT STAGE (omni_sp_debug_layer "desc_raw" / "desc_norm_partial"), so an earlier stage's error never
enters a later stage's gate.  u = 2^-24, gamma(k) = k u / (1 - k u).  All bounds assume no fp32 under- or overflow (the cases keep every product normal).

Stage 1, sp_sample_kernel (and its restatements sample_corner + sp_gather_cells_kernel / sp_sample_compact_kernel, convdb_sparse_sample).
  Coordinates.  The kernel's chain  gx = 2 kx / W - 1,  ix = ((gx + 1) Wc - 1) / 2  (csrc/conv.h sp_sample_coord: contraction switched off, a correctly
  rounded division),  x0 = floor(ix),  wx1 = ix - x0,  wx0 = (x0 + 1) - ix  is IEEE single, operation by operation, which numpy float32 reproduces exactly
  (``corners32``): cells and the four products wx wy are the kernel's bits, not approximations of them.
  y = the float64 sum of the m <= 4 in-map terms w_j t_j (w_j the emulated fp32 weight product, t_j the stored tap), T = sum |w_j t_j|.
  K.  ``v += tap * w`` from v = 0, in the order y0x0, y0x1, y1x0, y1x1.  Contracted (hipcc's default): m fmaf, the first term is rounded m times.  Not contracted: the
  product is rounded once, 0 + p is exact, then m - 1 additions: m roundings on the first two terms.  K = m covers both:  E = gamma_m T.  (m = 1: one rounding.)
  The IDEAL weights (``ideal_corners``).  For an integer key point and W a multiple of 8, in exact arithmetic ix = kx / 8 - 1 / 2: the weights are multiples of
  1 / 8, and kx = 4 (mod 8) lies EXACTLY on a cell boundary (ix an integer, wx1 = 0; the issue's "kx / 8 - 7 / 16, never on a boundary" was a slip: kx = 4 gives
  ix = 0).  Error of the fp32 chain, absolute:  2 kx exact;  b = fl(2 kx / W) in [0, 2): <= 2 u;  gx = fl(b - 1): exact for b >= 1 / 2, else <= u / 2;
  c = fl(gx + 1): exact below 1 / 2, else <= u: together 3.5 u;  d = fl(c Wc): 3.5 u Wc + 2 u Wc;  e = fl(d - 1): + 2 u Wc = 7.5 u Wc;  ix = e / 2 exact: 3.75 u Wc.
  wx1 and wx0 add at most u / 2 each:  |w - w_ideal| <= WEIGHT_ERR(Wc) = 4 u Wc per axis (Wc >= 2).  Off a boundary the ideal ix is >= 1 / 8 from an integer,
  so the fp32 cell IS the ideal's (asserted for every kx of W in 64, 104, 600, 640, 1280); on a boundary the chain may land on either side -- the cell to the
  left with weight 1 - eps, or the ideal's with weight 1 -- which is the same sample to within the bound: ``axis_weights`` compares the weight each CELL receives.
  The ideal is also checked against float64 F.grid_sample (align_corners=false, zeros padding), an independent restatement.

Stage 2, sp_chan_sumsq_kernel.  per = ceil(n / 8), segment seg = rows [seg per, min(seg per + per, n)), one fmaf per row from ss = 0:  y = sum v^2 in float64,
  E = gamma_m sum v^2 for a segment of m rows (the first square is rounded m times).  An empty segment is exactly 0 (E = 0).
  chan_norm_of: ss = ((0 + p_0) + p_1) + .. + p_7 in fp32 (7 roundings), dn = sqrtf(ss) (correctly rounded: the build has no fast-math option):
  dn = dn_ideal (1 + t),  |t| <= 3.5 u + u + O(u^2) < gamma_5,  dn_ideal = sqrt(sum_s p_s) of the STORED partial sums.

Stage 3, sp_pca_kernel.  From the stored raw and partial sums, q_c = raw_c / dn_ideal_c,  x_c = q_c - mean_c,  y_j = sum_c x_c comp_jc in float64.
  fl(raw / dn) = q (1 + t'),  |t'| <= gamma_5 + u + O(u^2) < gamma_6 (one correctly rounded division);  the subtraction rounds once:
      |x^ - x| <= gamma_6 |q| + u (|q| (1 + gamma_6) + |mean|) <= ex_c = gamma_7 |q_c| + u |mean_c|.
  The dot product: 4 partial sums (channels 64 p .. 64 p + 63) of 64 fmaf each from 0, combined as (s0 + s1) + (s2 + s3): every term is rounded at most 66 times:
      |y^_j - y_j| <= E_j = gamma_66 sum_c (|x_c| + ex_c) |comp_jc| + sum_c ex_c |comp_jc|.
  Without PCA (copy_raw_desc_kernel): y = q, E = gamma_6 |q|.
  NaN rule.  A channel whose stored partial sums are all zero is 0 / 0 = NaN exactly as in the reference: without PCA that channel alone, with PCA every output
  of the image (NaN times anything is NaN, a zero component included).  The refs return that exact pattern; ``gate`` compares patterns with np.isnan equality
  and leaves those positions out of the ratios.  Squares that overflow fp32 are out of scope (the float32 reference gives inf there too).

Tiers (as index_scan_ref).  tier 1: max |got - y| / E <= 1, nothing left out but NaN positions.  tier 2: per class of >= 1 000 values,
RMS(z_got) / RMS(z_emulation) <= c, z = error / allowance; the emulations (``sample_emul``, ``sumsq_emul``, ``project_emul``) run each stage in float32 in the
kernel's summation order (contracted form for stage 1).  Classes: key-point slot mod 8 (sampling workgroup) and mod 4 (PCA workgroup), segment, image slot,
number of in-map taps (4 / 2 / 1), output block of 64.  TIER2_C: twice the largest clean ratio measured on the MI355X per stage (tests/test_gpu_sp_desc.py lists them).

``chain_ref`` is the whole tail from the map in float64 with ideal weights and an allowance for ANY float32 implementation (any summation order, either cell at
a boundary): tests/test_sp_desc_ref_cpu.py holds oracle.postproc_ref.compute_descriptors -- the restatement pinned to the reference's text -- to it.
  raw:  A1 = (dx + dy + 2 u) S + gamma_4 T,  dx = WEIGHT_ERR(Wc), dy = WEIGHT_ERR(Hc) (a product of two weights in [0, 1] moves by at most dx + dy + dx dy, one rounding),
        S = sum |tap| over the ideal's four cells and, on a boundary, the column / row before them;
  dn:   the norm is 1-Lipschitz:  Adn = |A1|_2 + gamma_(n+2) dn  (n squares in any order, a square root);
  q:    Aq = (A1 + |q| Adn) / (dn - Adn) + u |q|;
  out:  Aout_j = sum_c (Aq_c + u (|q_c| + |mean_c|)) |comp_jc| (1 + gamma_256) + gamma_256 sum_c |x_c comp_jc|.
"""
from __future__ import annotations

import numpy as np

from tests.index_scan_ref import MIN_CLASS, U, Ref, gamma
from tests.index_scan_ref import tier1 as _tier1
from tests.index_scan_ref import tier2 as _tier2

NORM_SEGS = 8
# tier 2 gates: twice the largest clean ratio measured on the MI355X per stage over every case of tests/test_gpu_sp_desc.py (listed there)
TIER2_C = {"sample": 2.0, "sumsq": 2.0, "project": 2.0}
F1, F2 = np.float32(1), np.float32(2)


def weight_err(cells: int) -> float:
    return 4.0 * U * cells


# ---- stage 1: coordinates -------------------------------------------------------------------------------------------------------------
def coord32(k, size: int) -> np.ndarray:
    """The kernel's ix (iy) of key-point coordinates k for an image of `size` pixels: float32, operation by operation."""
    k = np.asarray(k, np.float32)
    g = (F2 * k) / np.float32(size) - F1
    return ((g + F1) * np.float32(size >> 3) - F1) / F2


def axis32(k, size: int):
    """(x0 int64, w0 float32, w1 float32) along one axis, as the kernel."""
    ix = coord32(k, size)
    f0 = np.floor(ix)
    return f0.astype(np.int64), (f0 + F1) - ix, ix - f0


def axis_ideal(k, size: int):
    """The same in exact arithmetic (integer k, size a multiple of 8): ix = k / 8 - 1 / 2, float64 without rounding."""
    ix = np.asarray(k, np.float64) / 8.0 - 0.5
    f0 = np.floor(ix)
    return f0.astype(np.int64), (f0 + 1.0) - ix, ix - f0


def axis_weights(x0, w0, w1, cells: int) -> np.ndarray:
    """[n, cells + 2] float64: the weight each cell -1 .. cells receives (index + 1)."""
    x0 = np.asarray(x0)
    out = np.zeros((len(x0), cells + 2))
    r = np.arange(len(x0))
    out[r, x0 + 1] += np.asarray(w0, np.float64)
    out[r, x0 + 2] += np.asarray(w1, np.float64)
    return out


def corners32(kps, W: int, H: int):
    """(cx, cy [n, 4] int64, w [n, 4] float32, inmap [n, 4]) in the kernel's order y0x0, y0x1, y1x0, y1x1."""
    kps = np.asarray(kps, np.float32).reshape(-1, 2)
    x0, wx0, wx1 = axis32(kps[:, 0], W)
    y0, wy0, wy1 = axis32(kps[:, 1], H)
    cx = np.stack([x0, x0 + 1, x0, x0 + 1], axis=1)
    cy = np.stack([y0, y0, y0 + 1, y0 + 1], axis=1)
    w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], axis=1).astype(np.float32)
    inmap = (cx >= 0) & (cx < (W >> 3)) & (cy >= 0) & (cy < (H >> 3))
    return cx, cy, w, inmap


def ideal_corners(kps, W: int, H: int):
    """corners32 in exact arithmetic (w float64)."""
    kps = np.asarray(kps, np.float64).reshape(-1, 2)
    x0, wx0, wx1 = axis_ideal(kps[:, 0], W)
    y0, wy0, wy1 = axis_ideal(kps[:, 1], H)
    cx = np.stack([x0, x0 + 1, x0, x0 + 1], axis=1)
    cy = np.stack([y0, y0, y0 + 1, y0 + 1], axis=1)
    w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], axis=1)
    inmap = (cx >= 0) & (cx < (W >> 3)) & (cy >= 0) & (cy < (H >> 3))
    return cx, cy, w, inmap


def _taps(desc, cx, cy, inmap) -> np.ndarray:
    """[n, 4, 256] in desc's dtype: the stored tap, 0 outside the map."""
    Hc, Wc = desc.shape[1], desc.shape[2]
    t = desc[:, np.clip(cy, 0, Hc - 1), np.clip(cx, 0, Wc - 1)]             # [256, n, 4]
    return np.where(inmap[None], t, 0).transpose(1, 2, 0)


def n_taps(kps, W: int, H: int) -> np.ndarray:
    return corners32(kps, W, H)[3].sum(axis=1)


def sample_ref(desc, kps, W: int, H: int) -> Ref:
    """Stage 1 from the dense map desc [256, H / 8, W / 8] float32 and the key points [n, 2]: y, E, T [n, 256]."""
    desc = np.asarray(desc, np.float32)
    cx, cy, w, inmap = corners32(kps, W, H)
    terms = _taps(desc, cx, cy, inmap).astype(np.float64) * w.astype(np.float64)[:, :, None]
    T = np.abs(terms).sum(axis=1)
    return Ref(terms.sum(axis=1), gamma(inmap.sum(axis=1).astype(np.float64))[:, None] * T, T)


def _fma32(a, b, acc32):
    """fmaf of fp32 operands: the product is exact in float64, one rounding of the sum to fp32 (a second one only on a 2^-29 tie pattern)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + acc32).astype(np.float32)


SAMPLE_DEFECTS = ("clamp_border", "swap_wx", "map_f16")


def sample_emul(desc, kps, W: int, H: int, defect: str | None = None) -> np.ndarray:
    """sp_sample_kernel in float32 [n, 256].  Defects: clamp_border -- at the first key point with a tap outside the map, those taps read the nearest border cell;
    swap_wx -- wx0 and wx1 swapped where x0 = -1; map_f16 -- the map rounded to fp16."""
    desc = np.asarray(desc, np.float32)
    if defect == "map_f16":
        desc = desc.astype(np.float16).astype(np.float32)
    cx, cy, w, inmap = corners32(kps, W, H)
    if defect == "swap_wx":
        sw = cx[:, 0] == -1
        w = np.where(sw[:, None], w[:, [1, 0, 3, 2]], w)
    t = _taps(desc, cx, cy, inmap)
    if defect == "clamp_border":
        i = int(np.nonzero(~inmap.all(axis=1))[0][0])
        inmap = inmap.copy()
        inmap[i] = True
        t = _taps(desc, cx, cy, inmap)
    acc = np.zeros((len(w), 256), np.float32)
    for j in range(4):
        acc = np.where(inmap[:, j, None], _fma32(t[:, j], w[:, j, None], acc), acc)
    return acc


# ---- stage 2: channel sums of squares -------------------------------------------------------------------------------------------------
def segments(n: int, floor_per: bool = False):
    per = n // NORM_SEGS if floor_per else (n + NORM_SEGS - 1) // NORM_SEGS
    return [(min(s * per, n), min(s * per + per, n)) for s in range(NORM_SEGS)]


def sumsq_ref(raw) -> Ref:
    """Stage 2 from the stored raw descriptors [n, 256] float32: y, E, T [8, 256]."""
    r64 = np.asarray(raw, np.float32).astype(np.float64) ** 2
    y = np.stack([r64[a:b].sum(axis=0) for a, b in segments(len(r64))])
    m = np.array([b - a for a, b in segments(len(r64))], np.float64)
    return Ref(y, gamma(m)[:, None] * y, y)


SUMSQ_DEFECTS = ("drop_last", "floor_per")


def sumsq_emul(raw, defect: str | None = None) -> np.ndarray:
    """sp_chan_sumsq_kernel in float32 [8, 256].  Defects: drop_last -- the last non-empty segment omits its last key point; floor_per -- per = floor(n / 8)."""
    raw = np.asarray(raw, np.float32)
    segs = segments(len(raw), defect == "floor_per")
    if defect == "drop_last":
        s = max(i for i, (a, b) in enumerate(segs) if b > a)
        segs[s] = (segs[s][0], segs[s][1] - 1)
    out = np.zeros((NORM_SEGS, 256), np.float32)
    for s, (a, b) in enumerate(segs):
        for i in range(a, b):
            out[s] = _fma32(raw[i], raw[i], out[s])
    return out


def chan_norm32(partial) -> np.ndarray:
    """chan_norm_of: the 8 partial sums added in order in fp32, sqrtf."""
    partial = np.asarray(partial, np.float32)
    ss = np.zeros(256, np.float32)
    for s in range(NORM_SEGS):
        ss = ss + partial[s]
    return np.sqrt(ss)


# ---- stage 3: normalisation + projection ----------------------------------------------------------------------------------------------
def project_ref(raw, partial, comp=None, mean=None) -> Ref:
    """Stage 3 from the stored raw [n, 256] and partial sums [8, 256]; comp [D, 256] + mean [256], or None for the 256-d output.  NaN where the kernel's is."""
    raw64, ss = np.asarray(raw, np.float32).astype(np.float64), np.asarray(partial, np.float32).astype(np.float64).sum(axis=0)
    nan_c = ss == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = raw64 / np.sqrt(ss)[None]
    if comp is None:
        y = np.where(nan_c[None], np.nan, q)
        return Ref(y, gamma(6) * np.abs(y), np.abs(y))
    c64, m64 = np.asarray(comp, np.float32).astype(np.float64), np.asarray(mean, np.float32).astype(np.float64)
    qz = np.where(nan_c[None], 0.0, q)
    x = qz - m64[None]
    ex = gamma(7) * np.abs(qz) + U * np.abs(m64)[None]
    ac = np.abs(c64).T
    T = np.abs(x) @ ac
    y, E = x @ c64.T, gamma(66) * ((np.abs(x) + ex) @ ac) + ex @ ac
    if nan_c.any():
        y, E, T = np.full_like(y, np.nan), np.full_like(E, np.nan), np.full_like(T, np.nan)
    return Ref(y, E, T)


PROJECT_DEFECTS = ("comp_f16", "prev_norm", "mean_first")


def project_emul(raw, partial, comp=None, mean=None, defect: str | None = None, partial_prev=None) -> np.ndarray:
    """sp_pca_kernel / copy_raw_desc_kernel in float32 [n, D].  Defects: comp_f16 -- components rounded to fp16; prev_norm -- the norm of `partial_prev` (the image
    before) divides; mean_first -- the mean is subtracted before the division."""
    raw = np.asarray(raw, np.float32)
    dn = chan_norm32(partial_prev if defect == "prev_norm" else partial)
    with np.errstate(divide="ignore", invalid="ignore"):
        if comp is None:
            return raw / dn[None]
        comp, mean = np.asarray(comp, np.float32), np.asarray(mean, np.float32)
        if defect == "comp_f16":
            comp = comp.astype(np.float16).astype(np.float32)
        x = (raw - mean[None]) / dn[None] if defect == "mean_first" else raw / dn[None] - mean[None]
        D = comp.shape[0]
        xp = x.astype(np.float64).reshape(len(raw), 4, 64)
        cp = comp.astype(np.float64).reshape(D, 4, 64)
        acc = np.zeros((len(raw), 4, D), np.float32)
        for cc in range(64):
            acc = (xp[:, :, cc, None] * cp[None, :, :, cc].transpose(0, 2, 1) + acc).astype(np.float32)
        return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


# ---- tiers ----------------------------------------------------------------------------------------------------------------------------
def nan_equal(got, ref: Ref) -> bool:
    return bool(np.array_equal(np.isnan(np.asarray(got)), np.isnan(ref.y)))


def tier1(got, ref: Ref) -> float:
    """index_scan_ref.tier1 over every position that is not NaN in the reference (check ``nan_equal`` first)."""
    ok = ~np.isnan(ref.y)
    return _tier1(np.asarray(got, np.float64)[ok], Ref(ref.y[ok], ref.E[ok], ref.T[ok]))


def tier2(got, emul, ref: Ref, classes: dict) -> dict:
    """index_scan_ref.tier2 with the reference's NaN positions taking no part."""
    ok = ~np.isnan(ref.y)
    z = lambda a: np.where(ok, a, 0.0)
    return _tier2(z(np.asarray(got, np.float64)), z(np.asarray(emul, np.float64)), Ref(z(ref.y), z(ref.E), z(ref.T)), classes, ok)


def cat_refs(refs) -> Ref:
    return Ref(np.concatenate([r.y for r in refs]), np.concatenate([r.E for r in refs]), np.concatenate([r.T for r in refs]))


def row_classes(counts, width: int, taps=None) -> dict:
    """Labels [sum counts, width] of the rows of a batch's images stacked: key-point slot mod 8 and mod 4, segment, image slot, in-map taps, output block of 64."""
    slot = np.concatenate([np.arange(n) for n in counts]) if len(counts) else np.zeros(0, np.int64)
    seg = np.concatenate([np.arange(n) // max(1, (n + NORM_SEGS - 1) // NORM_SEGS) for n in counts])
    img = np.concatenate([np.full(n, b) for b, n in enumerate(counts)])
    col = lambda a: np.broadcast_to(np.asarray(a, np.int64)[:, None], (len(slot), width))
    cls = {"slot%8": col(slot % 8), "slot%4": col(slot % 4), "segment": col(seg), "image": col(img),
           "block64": np.broadcast_to((np.arange(width) // 64)[None], (len(slot), width))}
    if taps is not None:
        cls["taps"] = col(taps)
    return cls


def seg_classes(n_images: int) -> dict:
    """Labels [8 n_images, 256] of the partial sums of a batch's images stacked."""
    return {"segment": np.broadcast_to(np.tile(np.arange(NORM_SEGS), n_images)[:, None], (NORM_SEGS * n_images, 256)),
            "image": np.broadcast_to(np.repeat(np.arange(n_images), NORM_SEGS)[:, None], (NORM_SEGS * n_images, 256))}


# ---- the whole tail in float64, with an allowance for any float32 implementation ------------------------------------------------------
def chain_ref(desc, kps, W: int, H: int, comp=None, mean=None):
    """{"raw", "q", "out": Ref}: the ideal tail from the map (ideal weights) and what any float32 restatement may differ by (module docstring).  NaN as the reference."""
    desc = np.asarray(desc, np.float32)
    kps = np.asarray(kps, np.float64).reshape(-1, 2)
    n, Wc, Hc = len(kps), W >> 3, H >> 3
    cx, cy, w, inmap = ideal_corners(kps, W, H)
    t = _taps(desc, cx, cy, inmap).astype(np.float64)
    raw = (t * w[:, :, None]).sum(axis=1)
    T = (np.abs(t) * w[:, :, None]).sum(axis=1)
    # S: |tap| over the ideal's cells and, on a boundary, the column / row before them
    pad = np.zeros((256, Hc + 3, Wc + 3))
    pad[:, 2:Hc + 2, 2:Wc + 2] = np.abs(desc)
    S = np.zeros((n, 256))
    bx, by = (kps[:, 0] % 8 == 4), (kps[:, 1] % 8 == 4)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            use = ((dx >= 0) | bx) & ((dy >= 0) | by)
            S += np.where(use[None], pad[:, cy[:, 0] + dy + 2, cx[:, 0] + dx + 2], 0.0).T
    A1 = (weight_err(Wc) + weight_err(Hc) + 2 * U) * S + gamma(4) * T
    dn = np.sqrt((raw ** 2).sum(axis=0))
    Adn = np.sqrt((A1 ** 2).sum(axis=0)) + gamma(n + 2) * dn
    nan_c = dn == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(nan_c[None], np.nan, raw / dn[None])
        Aq = (A1 + np.abs(q) * Adn[None]) / (dn - Adn)[None] + U * np.abs(q)
    res = {"raw": Ref(raw, A1, T), "q": Ref(q, Aq, np.abs(q))}
    if comp is not None:
        c64, m64 = np.asarray(comp, np.float32).astype(np.float64), np.asarray(mean, np.float32).astype(np.float64)
        ac = np.abs(c64).T
        qz, Az = np.where(nan_c[None], 0.0, q), np.where(nan_c[None], 0.0, Aq)
        x = qz - m64[None]
        out = x @ c64.T
        Aout = ((Az + U * (np.abs(qz) + np.abs(m64)[None])) @ ac) * (1 + gamma(256)) + gamma(256) * (np.abs(x) @ ac)
        if nan_c.any():
            out, Aout = np.full_like(out, np.nan), np.full_like(Aout, np.nan)
        res["out"] = Ref(out, Aout, np.abs(x) @ ac)
    return res


# ---- the cases both test modules share ------------------------------------------------------------------------------------------------
THRES = 0.5
SIZES = ((64, 32), (104, 72), (136, 104))


def special_points(W: int, H: int):
    """Corners, edges, kx / ky in {3, 4} (x0 = -1 against 0), {W - 5, W - 4} / {H - 5, H - 4} (x1 = Wc - 1 against Wc), interior."""
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2 + 1, H - 1), (0, H // 2), (W - 1, H // 2 + 1),
            (3, 3), (4, 4), (3, 4), (4, 3), (W - 5, H - 5), (W - 4, H - 4), (W - 5, H - 4), (W - 4, H - 5), (W // 2 + 3, H // 2 - 2), (17, 13)]


def place(W: int, H: int, n: int, seed: int) -> np.ndarray:
    """n distinct pixels [n, 2] (x, y) in row-major order: the special points first (from a start the seed picks), seeded random pixels behind them."""
    sp = special_points(W, H)
    pts = [sp[(5 * seed + i) % len(sp)] for i in range(min(n, len(sp)))]
    if n > len(pts):
        rng = np.random.default_rng(seed)
        taken = {y * W + x for x, y in pts}
        free = np.array([p for p in rng.permutation(W * H) if p not in taken][:n - len(pts)])
        pts += [(int(p % W), int(p // W)) for p in free]
    pts = np.array(pts, np.int64).reshape(-1, 2)
    return pts[np.lexsort((pts[:, 0], pts[:, 1]))]


def plateau_map(W: int, H: int, pts) -> np.ndarray:
    """Equal confidences never suppress each other and come out in row-major order."""
    semi = np.zeros((H, W), np.float32)
    if len(pts):
        semi[pts[:, 1], pts[:, 0]] = 0.875
    return semi


def lattice(W: int, H: int, n: int, seed: int):
    """(semi, pts in the order of their confidences): isolated peaks on a 9-pixel lattice, distinct confidences in seeded order."""
    rng = np.random.default_rng(seed)
    xs, ys = np.arange(0, W, 9), np.arange(0, H, 9)
    sites = np.array([(x, y) for y in ys for x in xs], np.int64)
    order = rng.permutation(len(sites))
    pts = sites[np.concatenate([[0], order[order != 0]])[:n]]              # the corner site (one in-map tap) is always among them
    pts = pts[rng.permutation(len(pts))]
    conf = (0.95 - 0.3 * np.arange(n) / max(n, 1)).astype(np.float32)
    semi = np.zeros((H, W), np.float32)
    semi[pts[:, 1], pts[:, 0]] = conf
    return semi, pts


def pca_of(dim: int, seed: int = 1):
    """Orthonormal components [dim, 256] and a small mean, as synth.pca."""
    rng = np.random.default_rng(1000 * seed + dim)
    qm, _ = np.linalg.qr(rng.normal(size=(256, dim)))
    return np.ascontiguousarray(qm.T.astype(np.float32)), (rng.normal(size=256) * 0.01).astype(np.float32)


def desc_map(kind: str, W: int, H: int, seed: int, pts=None) -> np.ndarray:
    """[256, H / 8, W / 8] float32.  unit: unit-norm columns as production; scales: times per-channel scales 1e-6 .. 1e3; cancel: channel 2 k + 1 =
    -(channel 2 k) (1 + 1e-4 noise), for a projection whose components come in equal pairs; zero_channel: channel 5 zero at every cell; one_nonzero: channel 5
    zero at every cell but those around one key point that shares no cell with another."""
    rng = np.random.default_rng(seed)
    Hc, Wc = H >> 3, W >> 3
    d = rng.standard_normal((256, Hc, Wc))
    d /= np.linalg.norm(d, axis=0, keepdims=True)
    if kind == "scales":
        d *= rng.permutation(np.logspace(-6, 3, 256))[:, None, None]
    elif kind == "cancel":
        d[1::2] = -d[0::2] * (1 + 1e-4 * rng.standard_normal((128, Hc, Wc)))
    elif kind in ("zero_channel", "one_nonzero"):
        keep = d[5].copy()
        d[5] = 0
        if kind == "one_nonzero":
            cx, cy, _, inmap = corners32(np.asarray(pts, np.float32), W, H)
            cells = [set((cy[i][inmap[i]] * Wc + cx[i][inmap[i]]).tolist()) for i in range(len(pts))]
            i = next(i for i in range(len(pts)) if not any(cells[i] & cells[k] for k in range(len(pts)) if k != i))      # a key point no other one shares a cell with
            d[5, cy[i][inmap[i]], cx[i][inmap[i]]] = keep[cy[i][inmap[i]], cx[i][inmap[i]]]
    elif kind != "unit":
        raise ValueError(kind)
    return d.astype(np.float32)


class Image:
    def __init__(self, semi, desc, kps):
        self.semi, self.desc, self.kps = semi, desc, np.asarray(kps, np.int64).reshape(-1, 2)


class Case:
    """One handle configuration and the images of one call; kps: the key points the call must return, in order."""

    def __init__(self, name, W, H, max_num, pca_dim, images, comp=None, mean=None):
        self.name, self.W, self.H, self.max_num, self.pca_dim, self.images = name, W, H, max_num, pca_dim, images
        self.comp, self.mean = (comp, mean) if comp is not None or pca_dim is None else pca_of(pca_dim)

    def __repr__(self):
        return self.name


def image(W, H, n, seed, kind="unit", max_num=None) -> Image:
    pts = place(W, H, n, seed)
    return Image(plateau_map(W, H, pts), desc_map(kind, W, H, seed + 100, pts), pts if max_num is None else pts[:max_num])


def cases() -> list:
    out = []
    counts = [(0, 8), (1, 8), (2, 8), (7, 8), (8, 8), (9, 200), (15, 200), (16, 200), (17, 200), (63, 200), (64, 200), (65, 200), (200, 200), (200, 1000)]
    for i, (n, M) in enumerate(counts):
        W, H = SIZES[i % 3]
        out.append(Case(f"n{n}_max{M}_{W}x{H}", W, H, M, 64, [image(W, H, n, i)]))
    out.append(Case("n1000_max1000_64x32", 64, 32, 1000, 64, [image(64, 32, 1000, 20)]))
    out.append(Case("n12_cut_at_max8_104x72", 104, 72, 8, 64, [image(104, 72, 12, 21, max_num=8)]))
    for i, d in enumerate((None, 1, 63, 65, 128, 256)):
        for j, n in enumerate((9, 200)):
            W, H = SIZES[(i + j) % 3]
            out.append(Case(f"pca{d}_n{n}_{W}x{H}", W, H, 200, d, [image(W, H, n, 30 + 2 * i + j, "scales" if (i + j) % 2 else "unit")]))
    semi, pts = lattice(600, 480, 200, 50)
    out.append(Case("lattice_600x480", 600, 480, 200, 64, [Image(semi, desc_map("unit", 600, 480, 51), pts)]))
    out.append(Case("scales_n65_104x72", 104, 72, 200, 64, [image(104, 72, 65, 52, "scales")]))
    comp, mean = pca_of(64, 2)
    comp[:, 1::2], mean[1::2] = comp[:, 0::2], -mean[0::2]
    out.append(Case("cancel_n200_136x104", 136, 104, 200, 64, [image(136, 104, 200, 53, "cancel")], comp, mean))
    for kind in ("zero_channel", "one_nonzero"):
        for d in (None, 64):
            out.append(Case(f"{kind}_pca{d}_n17_104x72", 104, 72, 200, d, [image(104, 72, 17, 54, kind)]))
    for s in (0, 1, 2, 3):                                                  # one key point, no PCA: every output is exactly +-1 (NaN in the zero channel)
        W, H = SIZES[s % 3]
        out.append(Case(f"exact_one_point_{s}_{W}x{H}", W, H, 8, None, [image(W, H, 1, 60 + 7 * s, "zero_channel" if s % 2 else "scales")]))
    W, H = 104, 72
    out.append(Case("batch_0_200_1", W, H, 200, 64, [image(W, H, 0, 70), image(W, H, 200, 71), image(W, H, 1, 72)]))
    out.append(Case("batch_200nan_0_200", W, H, 200, 64, [image(W, H, 200, 73, "zero_channel"), image(W, H, 0, 74), image(W, H, 200, 75, "scales")]))
    return out


def passes_case() -> list:
    """One handle, passes of 200, then 3, then 0, then 200 key points (104 x 72, max_num 200, PCA 64)."""
    return [Case(f"pass{k}_n{n}", 104, 72, 200, 64, [image(104, 72, n, 80 + k)]) for k, n in enumerate((200, 3, 0, 200))]
