"""fp64 references, arithmetic error bounds and float32 emulations for the scan kernels of the loop-closure index (csrc/index.hip), beside
tests/f16_layer_ref.py and tests/split_layer_ref.py.  Pure numpy; the library is not imported.

``IndexFlatIP.debug_scan`` (omni_index_debug_scan) returns EVERY 64-bit key a scan kernel wrote, undecoded.  ``decode_keys`` / ``make_keys`` restate
csrc/common.h omni_make_key: high word = the order-preserving map of the fp32 score (sign bit set -> all bits flipped, else the sign bit set; -0 sorts just
below +0), low word = 0xFFFFFFFF - row, 0 = OMNI_KEY_EMPTY for a row at or beyond its query's limit.

A score's reference is the IDEAL VALUE OF THE KERNEL'S OWN ALGEBRA in float64, from the operands AS STORED:
  ip_scan_kernel<float, QB>, ip_scan_rows_kernel<QB, 4>, cert_refine_kernel.  fp32 rows, fp32 queries:  y = sum_k q_k row_k.
      A lane adds its dim / 64 products with one fmaf each (index.hip:157-168 / 209-224 / 625-629: columns 4 lane + 256 j + e, j outer, e inner), wave_sum adds
      the 64 lanes in a butterfly of 6 additions (index.hip:128-132, offsets 32, 16, .. 1):  K = dim / 64 + 6.
  ip_scan_t16_kernel<QB>.  Rows are fp16(row) (f32_to_t16_kernel, round to nearest even), converted back exactly:  y = sum_k q_k fp16(row_k).  Lane (r, c) of
      a 16-row block adds the 8 halfs of chunk 4 st + c for st = 0 .. dim / 32 - 1 (index.hip:563-580): a chain of dim / 4 fmaf; two shuffles (xor 16, xor 32,
      index.hip:585-586) add the 4 chunk lanes of a row:  K = dim / 4 + 2.
  ip_scan_mq_kernel (on an fp16 shard, or on the fp16 mirror of an fp32 shard).  ``mq_prep`` restates mq_prep_kernel (index.hip:258-292): per query
      m = max |q|, sh = 13 - ilogb(m) clamped to +-100 (0 for m = 0 and for the padding slots nq .. 63, whose operands are zero), v = fl32(q 2^sh),
      hi = half(v), lo = half(v - hi), inv = 2^-sh.  The kernel adds hi_k row_k and lo_k row_k (both exact in fp32) and multiplies by inv once
      (index.hip:461):  y = inv sum_k (hi_k + lo_k) fp16(row_k).  The dropped residue v - hi - lo is no error of the scan: it is an allowance of its own,
      R = inv sum_k max(2^-22 |v_k|, 2^-25) |fp16(row_k)|  (half an fp16 step of lo, |lo| <= ulp16(v) / 2; 2^-25 absolute where lo is an fp16 subnormal),
      which the certificate's budget has to cover as well (``cert_eps``).
      K.  Per k-step one v_mfma_f32_16x16x32_f16 against hi, one against lo, each adding 32 exact products to the fp32 accumulator (index.hip:331-336).
      ASSUMED of one MFMA: nothing but that every addition inside it rounds no worse than an fp32 addition, in any order (the hardware's order and its
      intermediate width are not documented).  Any such summation of the 2 dim products stays within gamma_(2 dim) T:  K = 2 dim, the full-gamma
      convention of split_layer_ref for tier 1.  The final multiplication by a power of two is exact (scores in the normal range).

Two tiers per score.
  Tier 1 (derived, never to be exceeded): |got - y| <= gamma_K T (+ R), T = the sum of the magnitudes of the terms the kernel adds, u = 2^-24.  T = 0 (a zero
      query): the score is exactly 0.
  Tier 2 (sensitivity): the same summation emulated in float32 on the CPU (``valu_emul``, ``t16_emul``, ``mq_emul``: the lane's fmaf chain and the shuffles in
      the kernel's order; for the matrix cores one MFMA = one exact 32-term dot added to the accumulator with one rounding, hi then lo per k-step, the k-slices
      in the order the rotation gives the row's 512-row block (index.hip:364-367: block index mod dim / 256), times inv once).  Per class (``tier2``), with
      z = error / tier-1 allowance:  RMS(z_got) <= c RMS(z_emul).  Classes hold >= 1 000 scores (smaller ones are not judged alone; a case with fewer than
      1 000 scores in all is left to tier 1): for the VALU kernels the query slot and the row mod 4 (fp32: the rows kernel's place in its group) or mod 16
      (fp16: the row of the block); for the matrix cores the query slot (64), the (wave, row tile) place of the row's 16-row tile in its 512-row block (32),
      the pass index of the workgroup that scores the block (block index / grid), and the rows of the last block when it has clamped tiles.
The emulators take a ``defect``: tests/test_index_scan_ref_cpu.py shows that each of them fails the gate in its class.

TIER2_C: twice the largest clean ratio measured on the MI355X per kernel (tests/test_gpu_index_scores.py lists them).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
# tier 2 gates: twice the largest clean ratio measured on the MI355X over every case of tests/test_gpu_index_scores.py (listed there): the VALU kernels follow their
# emulation exactly (1.000); the matrix-core scan reached 4.285 (dim 4096, 1 029 rows, the slot of the 1e30 query) -- an MFMA's accumulation of its 32 products is
# noisier than one rounding, as the fp16 matrix-core convolutions showed (split_layer_ref.TIER2_C).  The smallest defect ratio of tests/test_index_scan_ref_cpu.py is 68.
TIER2_C = {"f32": 2.0, "t16": 2.0, "mq": 8.57}
MIN_CLASS = 1000
KEY_EMPTY = np.uint64(0)
# cert_select_kernel's constants (index.hip:677-682), as the float32 literals they are
CERT_RND = np.float32(4.8829e-4) * np.float32(1.0001)
CERT_SUB = np.float32(6.0e-8)
CERT_ARITH = np.float32(4.0e-6)
CERT_MAX_NORM = 6.0e4
CERT_Q_RANGE = (np.float32(1.0e-15), np.float32(1.0e15))      # max |q| outside: not certifiable (the fp32 norm under eps and mq_prep_kernel's shift both break down)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


# ---- keys -----------------------------------------------------------------------------------------------------------------------------
def make_keys(scores, rows) -> np.ndarray:
    """omni_make_key for float32 scores [..., n] and row numbers [n]."""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(rows, np.uint64))


def decode_keys(keys):
    """(scores float32, rows int64, empty) of raw keys; the score and row of an empty key are not meaningful."""
    keys = np.asarray(keys, np.uint64)
    o = (keys >> np.uint64(32)).astype(np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    rows = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return u.view(np.float32), rows, keys == KEY_EMPTY


def h16(a) -> np.ndarray:
    """fp16(a) as float32 (round to nearest even from the fp32 value, as f32_to_t16_kernel's __floats2half2_rn)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---- the float64 ideals and tier 1 ----------------------------------------------------------------------------------------------------
class Ref:
    """y [nq, n]: the ideal score; E: the tier-1 allowance (R included); T: sum of |terms|."""

    def __init__(self, y, E, T):
        self.y, self.E, self.T = y, E, T


def valu_ref(q, rows_stored, chain: int) -> Ref:
    """fp32 queries against rows as stored (fp32 rows, or h16(rows) for ip_scan_t16_kernel); chain = K."""
    q64, r64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(rows_stored, np.float32).astype(np.float64)
    T = np.abs(q64) @ np.abs(r64).T
    return Ref(q64 @ r64.T, gamma(chain) * T, T)


def f32_ref(q, rows) -> Ref:
    return valu_ref(q, rows, q.shape[1] // 64 + 6)


def t16_ref(q, rows16) -> Ref:
    return valu_ref(q, rows16, q.shape[1] // 4 + 2)


def mq_prep(q):
    """mq_prep_kernel: (hi, lo [nq, dim] float64 -- halfs --, v [nq, dim] float64 -- the scaled fp32 query --, inv [nq] float32)."""
    q = np.asarray(q, np.float32)
    m = np.abs(q).max(axis=1)
    sh = np.zeros(len(q), np.int64)
    ok = (m > 0) & (m < np.float32(3.0e38))
    sh[ok] = np.clip(13 - (np.frexp(m[ok])[1].astype(np.int64) - 1), -100, 100)          # ilogb = frexp's exponent - 1
    with np.errstate(over="ignore", under="ignore"):
        v = np.ldexp(q, sh[:, None].astype(np.int32)).astype(np.float32)                 # fl32(q * 2^sh): rounds only into the subnormals
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)                              # v - hi is exact in fp32
    return hi.astype(np.float64), lo.astype(np.float64), v.astype(np.float64), np.ldexp(np.float32(1), (-sh).astype(np.int32)).astype(np.float32)


def mq_ref(q, rows16) -> Ref:
    """ip_scan_mq_kernel against rows16 = h16(rows)."""
    hi, lo, v, inv = mq_prep(q)
    r64 = np.asarray(rows16, np.float32).astype(np.float64)
    ar = np.abs(r64).T
    inv64 = inv.astype(np.float64)[:, None]
    T = ((np.abs(hi) + np.abs(lo)) @ ar) * inv64
    R = (np.maximum(2.0 ** -22 * np.abs(v), np.where(v != 0, 2.0 ** -25, 0.0)) @ ar) * inv64
    return Ref(((hi + lo) @ r64.T) * inv64, gamma(2 * q.shape[1]) * T + R, T)


def tier1(got, ref: Ref) -> float:
    """The worst |got - y| / E (<= 1 passes); a score whose allowance is 0 must equal y: inf otherwise."""
    err = np.abs(np.asarray(got, np.float64) - ref.y)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ref.E > 0, err / np.where(ref.E > 0, ref.E, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- float32 emulations ---------------------------------------------------------------------------------------------------------------
def _fma32(a64, b64, acc32):
    """fmaf of fp32 operands held as float64: the product is exact in float64, one rounding of the sum to fp32 (a second one only on a 2^-29 tie pattern)."""
    return (a64 * b64 + acc32).astype(np.float32)


def valu_emul(q, rows, defect: str | None = None, chunk: int = 1 << 22) -> np.ndarray:
    """ip_scan_kernel / ip_scan_rows_kernel / cert_refine_kernel: [nq, n] float32.  defect "last_fmaf": lane 37 of every row loses its last fmaf."""
    q, rows = np.asarray(q, np.float32), np.asarray(rows, np.float32)
    nq, dim = q.shape
    n, J = rows.shape[0], dim // 256
    qr = q.astype(np.float64).reshape(nq, 1, J, 64, 4)
    out = np.empty((nq, n), np.float32)
    step = max(1, chunk // (nq * 64))
    x = np.arange(64)
    for s in range(0, n, step):
        rr = rows[s:s + step].astype(np.float64).reshape(1, -1, J, 64, 4)
        acc = np.zeros((nq, rr.shape[1], 64), np.float32)
        for j in range(J):
            for e in range(4):
                new = _fma32(rr[:, :, j, :, e], qr[:, :, j, :, e], acc)
                if defect == "last_fmaf" and j == J - 1 and e == 3:
                    new[:, :, 37] = acc[:, :, 37]
                acc = new
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, x ^ off]
        out[:, s:s + step] = acc[:, :, 0]
    return out


def t16_emul(q, rows16, chunk: int = 1 << 22) -> np.ndarray:
    """ip_scan_t16_kernel on rows16 = h16(rows): [nq, n] float32."""
    q, rows16 = np.asarray(q, np.float32), np.asarray(rows16, np.float32)
    nq, dim = q.shape
    n, steps = rows16.shape[0], dim // 32
    qr = q.astype(np.float64).reshape(nq, 1, steps, 4, 8)
    out = np.empty((nq, n), np.float32)
    step = max(1, chunk // (nq * 4))
    for s in range(0, n, step):
        rr = rows16[s:s + step].astype(np.float64).reshape(1, -1, steps, 4, 8)
        acc = np.zeros((nq, rr.shape[1], 4), np.float32)
        for st in range(steps):
            for e in range(8):
                acc = _fma32(rr[:, :, st, :, e], qr[:, :, st, :, e], acc)
        acc = acc + acc[:, :, [1, 0, 3, 2]]
        acc = acc + acc[:, :, [2, 3, 0, 1]]
        out[:, s:s + step] = acc[:, :, 0]
    return out


MQ_DEFECTS = ("lo_step", "lo_fragment", "stale_slice", "clamped_tile", "no_rotation", "inv_twice")


def mq_emul(q, rows16, rotate: bool = True, defect: str | None = None) -> np.ndarray:
    """ip_scan_mq_kernel on rows16 = h16(rows): [nq, n] float32.  Defects (each what a plausible slip in the kernel would compute):
      lo_step       the lo operand of the 3rd k-step of the 2nd slice unit is not added;
      lo_fragment   the same, for the query fragment 16 .. 31 only (the others keep it);
      stale_slice   the query operands of that k-step are read from the previous unit's LDS buffer;
      clamped_tile  the 16-row tile at place 5 of the first 512-row block is scored with the rows of the shard's last tile;
      no_rotation   the row pointers of block 1 ignore the rotation their query slices follow;
      inv_twice     the last query slot (the one next to the padding) is multiplied by inv twice."""
    hi, lo, _, inv = mq_prep(q)
    nq, dim = hi.shape
    r64 = np.asarray(rows16, np.float32).astype(np.float64)
    n, S = r64.shape[0], dim // 256
    if defect == "clamped_tile":
        last = ((n + 15) // 16 - 1) * 16
        src = np.minimum(last + np.arange(16), n - 1)          # (rows of the last tile beyond n hold whatever the block holds: the last row stands in)
        r64 = r64.copy()
        r64[80:96] = r64[src][:len(r64[80:96])]
    blk = np.arange(n) // 512
    out = np.empty((nq, n), np.float32)
    for r in (range(S) if rotate else (0,)):
        groups = [np.nonzero(blk % S == r)[0]] if rotate else [np.arange(n)]
        if defect == "no_rotation" and rotate:                 # block 1 on its own
            groups = [g for g in (groups[0][blk[groups[0]] != 1], groups[0][blk[groups[0]] == 1]) if len(g)]
        for sel in groups:
            if len(sel) == 0:
                continue
            unrot = defect == "no_rotation" and rotate and blk[sel[0]] == 1
            R = r64[sel]
            acc = np.zeros((nq, len(sel)), np.float32)
            for j in range(S):
                sl = (j + r) % S
                rsl = j if unrot else sl
                for s in range(8):
                    kq, kr = sl * 256 + s * 32, rsl * 256 + s * 32
                    here = j == min(1, S - 1) and s == 2
                    if defect == "stale_slice" and here:
                        kq = ((j - 1 + r) % S) * 256 + s * 32
                    Rt = R[:, kr:kr + 32].T
                    acc = (acc + hi[:, kq:kq + 32] @ Rt).astype(np.float32)
                    lo_k = lo[:, kq:kq + 32]
                    if here and defect == "lo_step":
                        continue
                    if here and defect == "lo_fragment":
                        lo_k = lo_k.copy()
                        lo_k[16:32] = 0
                    acc = (acc + lo_k @ Rt).astype(np.float32)
            res = acc * inv[:, None]
            if defect == "inv_twice":
                res[nq - 1] = res[nq - 1] * inv[nq - 1]
            out[:, sel] = res
    return out


# ---- tier 2 ---------------------------------------------------------------------------------------------------------------------------
def valu_classes(nq: int, n: int, mod: int) -> dict:
    rows = np.arange(n)
    return {"slot": np.broadcast_to(np.arange(nq)[:, None], (nq, n)), f"row%{mod}": np.broadcast_to((rows % mod)[None], (nq, n))}


def mq_classes(nq: int, n: int, grid: int) -> dict:
    """grid = the launch's workgroups: min(blocks, CUs)."""
    rows = np.arange(n)
    blocks = (n + 511) // 512
    cls = {"slot": np.broadcast_to(np.arange(nq)[:, None], (nq, n)), "tile": np.broadcast_to(((rows // 16) % 32)[None], (nq, n)),
           "pass": np.broadcast_to(((rows // 512) // grid)[None], (nq, n))}
    if (n + 15) // 16 < blocks * 32:                           # the last block has clamped tiles
        cls["last_block"] = np.broadcast_to(np.where(rows // 512 == blocks - 1, 0, -1)[None], (nq, n))
    return cls


def tier2(got, emul, ref: Ref, classes: dict, valid=None) -> dict:
    """The worst RMS(z_got) / RMS(z_emul) over the classes (label arrays shaped like got; label < 0 = in no class of that kind) of >= MIN_CLASS scores, z = error /
    tier-1 allowance (scores of zero allowance: z = 0 when exact, inf otherwise).  ``valid``: the scores that take part (not the empty keys).  When no class
    of a kind is large enough the kind is judged as one class; with fewer than MIN_CLASS scores in all nothing is judged (ratio 0, judged 0)."""
    got, emul = np.asarray(got, np.float64), np.asarray(emul, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = ref.E > 0
        den = np.where(pos, ref.E, 1.0)
        zg = np.where(pos, (got - ref.y) / den, np.where(got == ref.y, 0.0, np.inf)) ** 2
        ze = np.where(pos, (emul - ref.y) / den, 0.0) ** 2
    take = np.ones(got.shape, bool) if valid is None else np.asarray(valid, bool)
    worst, where, judged = 0.0, None, 0
    for kind, lab in classes.items():
        lab = np.where(take, lab, -1).ravel()
        keep = lab >= 0
        if keep.sum() < MIN_CLASS:
            continue
        cnt = np.bincount(lab[keep])
        if cnt.max() < MIN_CLASS:
            lab, cnt = np.where(keep, 0, -1), np.array([keep.sum()])
            keep = lab >= 0
        sg = np.bincount(lab[keep], zg.ravel()[keep], minlength=len(cnt))
        se = np.bincount(lab[keep], ze.ravel()[keep], minlength=len(cnt))
        for c in np.nonzero(cnt >= MIN_CLASS)[0]:
            judged += 1
            r = np.sqrt(sg[c] / se[c]) if se[c] > 0 else (0.0 if sg[c] == 0 else np.inf)
            if where is None or r > worst:
                worst, where = float(r), (kind, int(c))
    return {"ratio": worst, "where": where, "judged": judged}


# ---- the mirror's certificate ---------------------------------------------------------------------------------------------------------
def cert_eps(q, rows) -> np.ndarray:
    """cert_select_kernel's eps per query (index.hip: the certificate block at the end of the kernel): rows = every fp32 row the shard has held (norm_max is
    never lowered).  inf where the kernel refuses to certify whatever the scores: a row norm of 6e4 or more (or NaN), max |q| outside CERT_Q_RANGE."""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    rn = np.sqrt((np.asarray(rows, np.float32).astype(np.float64) ** 2).sum(axis=1).max())
    qn = np.sqrt((q64 ** 2).sum(axis=1))
    eps = float(CERT_RND) * qn * rn + float(CERT_SUB) * np.abs(q64).sum(axis=1) + float(CERT_ARITH) * qn * rn
    qm = np.abs(q64).max(axis=1)
    sound = (qm > float(CERT_Q_RANGE[0])) & (qm < float(CERT_Q_RANGE[1])) & bool(rn < CERT_MAX_NORM)
    return np.where(sound, eps, np.inf)


def worst_case_row(dim: int, seed: int) -> np.ndarray:
    """The row the fp16 mirror loses most of: every element 2^e (1 + 2^-11 (1 - 2^-6)), e in [-9, -6], random signs -- just below the midpoint of two halfs,
    rounded down by a relative 2^-11 (1 - 2^-6) / (1 + 2^-11): 4.80e-4.  float32."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-9, -5, dim)
    s = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
    return (s * np.ldexp(1.0 + 2.0 ** -11 * (1.0 - 2.0 ** -6), e)).astype(np.float32)


def victim_scene(dim: int, k: int, seed: int, n_background: int = 150):
    """The shard of the end-to-end certificate test: (rows float32 [n, dim], q float32 [dim], victim row number, filler row numbers).
    q is parallel to the victim v = worst_case_row, scaled so that q . v = 1.  k - 1 rows v (1 + 0.002 j) score above it, the victim is the true k-th
    neighbour, and kp - k + 1 fillers (kp = max(k + 24, 2 k), the candidates of search_dev) -- elements exactly representable in fp16, norm <= |v|, made as
    fp16(a (v + 0.005 w)), w orthogonal to v with |w| = |v| -- have float64 scores spread over the middle 80 % of (q . fp16(v), q . v): the mirror ranks all
    of them above the victim, so the victim is no candidate, and only a certificate with a sound eps sends the query to the exact scan."""
    rng = np.random.default_rng(seed)
    v = worst_case_row(dim, seed + 1)
    v64 = v.astype(np.float64)
    q = (v64 / (v64 @ v64)).astype(np.float32)
    q64 = q.astype(np.float64)
    s32, s16 = float(q64 @ v64), float(q64 @ h16(v).astype(np.float64))
    kp = max(k + 24, 2 * k)
    nf = kp - k + 1
    targets = s16 + (s32 - s16) * (0.1 + 0.8 * (np.arange(nf) + 0.5) / nf)
    fillers = []
    for t in targets:
        w = rng.standard_normal(dim)
        w -= (w @ v64) / (v64 @ v64) * v64
        w *= np.linalg.norm(v64) / np.linalg.norm(w)
        a = t / s32
        for _ in range(8):                                     # re-aim after the fp16 rounding of the elements
            f = h16(a * (v64 + 0.005 * w)).astype(np.float64)
            a *= t / float(q64 @ f)
        fillers.append(f.astype(np.float32))
    better = [(v64 * (1.0 + 0.002 * (j + 1))).astype(np.float32) for j in range(k - 1)]
    bg = rng.standard_normal((n_background, dim)).astype(np.float32)
    bg *= (0.9 * np.linalg.norm(v64) / np.linalg.norm(bg, axis=1, keepdims=True)).astype(np.float32)
    rows = np.concatenate([bg, np.stack(better + [v] + fillers) if better else np.stack([v] + fillers)])
    perm = rng.permutation(len(rows))
    rows = rows[perm]
    where = np.argsort(perm)                                   # old position -> new row number
    base = n_background + len(better)
    return rows, q, int(where[base]), where[base + 1:base + 1 + nf]


def oracle_topk(q, rows, k):
    """float64 scores, k best descending, ties -> lower row: (ids [nq, k], scores [nq, k])."""
    s = np.asarray(q, np.float32).astype(np.float64) @ np.asarray(rows, np.float32).astype(np.float64).T
    ids = np.stack([np.lexsort((np.arange(s.shape[1]), -s[i]))[:k] for i in range(s.shape[0])])
    return ids, np.take_along_axis(s, ids, axis=1)


# ---- the cases both test modules share ------------------------------------------------------------------------------------------------
def unit_rows(n: int, dim: int, seed: int) -> np.ndarray:
    """n unit rows, cheap at any size: a seeded base of <= 4096 rows; block j = the base with its columns rolled by 37 j under a per-block sign pattern."""
    rng = np.random.default_rng(seed)
    m = min(n, 4096)
    base = rng.standard_normal((m, dim), dtype=np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    if n <= m:
        return base
    out = np.empty((n, dim), np.float32)
    for j, s in enumerate(range(0, n, m)):
        sign = np.where(np.random.default_rng(seed + 1 + j).random(dim) < 0.5, np.float32(-1), np.float32(1))
        out[s:s + m] = (np.roll(base, 37 * j, axis=1) * sign)[:n - s]
    return out


def queries(rows: np.ndarray, nq: int, seed: int, special: bool) -> np.ndarray:
    """row + 0.02 noise, the rows spread over the shard (the first and the last among them).  special (the matrix-core cases): slot 0 x 37.5, slot 1 x 1e-3,
    slot 2 x 1e30, slot 3 all zero, slot 4 one element 2^20 times the largest other one (the others' lo halves are fp16 subnormals), slot 5 x 1e-32 (the shift
    of mq_prep_kernel clamped to 100) -- as far as nq reaches."""
    rng = np.random.default_rng(seed)
    n, dim = rows.shape
    pick = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, nq)]))[:nq] if nq > 1 else np.array([n - 1])
    pick = np.resize(pick, nq)
    q = rows[pick] + np.float32(0.02) * rng.standard_normal((nq, dim), dtype=np.float32)
    if special and nq >= 4:
        q[0] *= np.float32(37.5)
        q[1] *= np.float32(1e-3)
        q[2] *= np.float32(1e30)
        q[3] = 0
    if special and nq >= 6:
        q[4, 7] = np.abs(q[4]).max() * np.float32(2.0 ** 20)
        q[5] *= np.float32(1e-32)
    return np.ascontiguousarray(q, np.float32)
