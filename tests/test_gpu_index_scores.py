"""GPU: EVERY score of every scan kernel of the loop-closure index (csrc/index.hip) against the float64 ideal of the kernel's own algebra, and the fp16
mirror's exactness certificate against the error it has to cover (tests/index_scan_ref.py; tests/test_gpu_index.py sees a scan only through its best k scores).

``IndexFlatIP.debug_scan`` (omni_index_debug_scan) launches one named kernel through the search's own launch functions and returns every raw 64-bit key:
  keys    the low word is 0xFFFFFFFF - row, the empty key marks exactly the rows at or beyond the query's limit, the high word decodes to the score gated below
          (positive and negative ones); a production search's top k are the k largest of these keys, bit for bit;
  tier 1  |score - y| <= gamma_K T (+ the split residue): derived, per score, never to be exceeded;
  tier 2  per class (query slot, row place, pass of a persistent workgroup, the clamped last block) RMS(z_gpu) <= c RMS(z_emulation), z = error / allowance,
          the emulation being the same summation in float32 on the CPU; c = index_scan_ref.TIER2_C;
  bits    ip_scan_kernel<float, QB>, ip_scan_rows_kernel<QB, 4> and cert_refine_kernel give ip_scan_kernel<float, 1>'s bits on every row;
  mirror  |mirror score - float64(q . fp32 row)| <= cert_select_kernel's eps for every row and query, the worst-case row included; end to end a victim row that
          only a sound eps saves comes back, through the fallback, as the float64 oracle's k-th neighbour (half the eps would certify and lose it).

MEASURED on one MI355X (256 CUs; printed with -s): worst tier-1 ratio / worst tier-2 ratio over the query blocks of each case (every tier-1 ratio must be <= 1, every
tier-2 ratio <= its c; 0.000 = fewer than 1 000 scores, tier 1 only).  Two runs gave the same figures to the last digit; the fp16 shard and the fp32 shard's mirror
gave the same keys.
  ip_scan_kernel / ip_scan_rows_kernel   dim 512:  n 1 0.0956/0.000  3 0.1219/0.000  4 0.0719/0.000  5 0.1316/0.000  1027 0.1474/1.000  32771 0.1261/1.000
                                         dim 4096: n 1 0.0165/0.000  3 0.0161/0.000  4 0.0135/0.000  5 0.0138/0.000  1027 0.0115/1.000
  ip_scan_t16_kernel                     dim 512:  n 1 0.0294/0.000  15 0.0192/0.000  16 0.0228/0.000  17 0.0264/0.000  1000 0.0200/1.000  131125 0.0259/1.000
                                         dim 4096: n 17 0.0033/0.000  1000 0.0066/1.000
  ip_scan_mq_kernel (fp16 = mirror)      dim 4096: n 1 0.0023/0.000  15 0.0025/0.000  16 0.0024/2.055  17 0.0035/2.527  511 0.0042/2.895  512 0.0043/3.260
                                                   513 0.0041/3.204  1029 0.0049/4.285  8275 0.0048/2.305
                                         dim 512 n 265875: 0.0283/2.120      dim 1024 n 265875: 0.0045/2.084
Largest clean tier-2 ratio per kernel, and c = twice it (index_scan_ref.TIER2_C): the fp32 wave kernels 1.000 -> 2.0, ip_scan_t16_kernel 1.000 -> 2.0 (both follow
their float32 emulation rounding for rounding), ip_scan_mq_kernel 4.285 -> 8.57 (dim 4096, 1 029 rows, 4 queries, the slot of the x 1e30 query; the worst slots of the
other cases sit at 2.0 - 3.7: one MFMA's accumulation of its 32 products is noisier than the emulation's single rounding).  The smallest defect ratio of
tests/test_index_scan_ref_cpu.py is 68 (>= 5 c).
The mirror against its certificate: the worst |mirror score - exact score| / eps is 0.965 (the victim row: 4.80e-4 |q||row| lost of an eps of 4.98e-4); the mirror scan's
own error uses at most 0.29 of its 4e-6 |q| max|row| share of eps over every certifiable query of this module.  FOUND with this module and fixed in cert_select_kernel: a
query of magnitude 1e-32 reached 1.50 of that share (mq_prep_kernel's shift is clamped at 2^100, the lo halves are lost) while the kernel's fp32 |q| had vanished (the
squares go subnormal), leaving eps 400 times too small: a query whose largest element lies outside [1e-15, 1e15] is no longer certified (index_scan_ref.CERT_Q_RANGE;
``test_uncertifiable_rows_fall_back_and_subnormal_rows_stay_exact``).
"""
import numpy as np
import pytest

from tests import index_scan_ref as R

pytestmark = pytest.mark.gpu


def _cus(ctx):
    return int(ctx.device_info()["n_cu"])


def _shard(omni, ctx, rows, f16):
    idx = omni.capi.IndexFlatIP(ctx, rows.shape[1], omni.capi.STORE_F16 if f16 else omni.capi.STORE_F32, capacity=len(rows))
    idx.add(rows)
    assert idx.ntotal == len(rows)
    return idx


def _check_keys(keys, n, limits=None):
    """Low words, empties; returns (scores, valid)."""
    sc, rr, empty = R.decode_keys(keys)
    lim = np.full(keys.shape[0], n, np.int64) if limits is None else np.minimum(np.asarray(limits, np.int64), n)
    want_empty = np.arange(n)[None, :] >= lim[:, None]
    assert np.array_equal(empty, want_empty), "OMNI_KEY_EMPTY marks exactly the rows at or beyond the limit"
    assert np.array_equal(rr[~empty], np.broadcast_to(np.arange(n), keys.shape)[~empty]), "low word = 0xFFFFFFFF - row"
    assert np.array_equal(R.make_keys(sc, np.arange(n))[~empty], keys[~empty])
    return sc, ~empty


def _gate(tag, kernel, keys, ref, emul, classes, limits=None):
    n = keys.shape[1]
    sc, valid = _check_keys(keys, n, limits)
    got = np.where(valid, sc.astype(np.float64), ref.y)                       # rows beyond a limit take no part
    assert np.isfinite(sc[valid]).all()
    t1 = R.tier1(got, ref)
    t2 = R.tier2(got, emul, ref, classes, valid)
    print(f"[{kernel}] {tag}: tier1 {t1:.4f}  tier2 {t2['ratio']:.3f} at {t2['where']} ({t2['judged']} classes)")
    assert t1 <= 1.0, (tag, t1)
    assert t2["ratio"] <= R.TIER2_C[kernel], (tag, t2)
    return got


def _top(keys_row, k):
    """What topk_keys + decode_topk_kernel make of one query's keys: (D, I)."""
    order = np.sort(keys_row)[::-1][:k]
    sc, rows, empty = R.decode_keys(order)
    D = np.where(empty, np.float32(-3.402823466e+38), sc)
    I = np.where(empty, -1, rows)
    if len(order) < k:
        D = np.concatenate([D, np.full(k - len(order), -3.402823466e+38, np.float32)])
        I = np.concatenate([I, np.full(k - len(order), -1, np.int64)])
    return D.astype(np.float32), I.astype(np.int64)


def _batch(ctx, idx, q, k, limits):
    rows_dev = ctx.to_device(q)
    buf = ctx.alloc(len(q) * k * 12)
    idx.search_batch_prefix_dev(rows_dev, None, k, limits, buf + len(q) * k * 8, buf)
    raw = ctx.from_device(buf, (len(q) * k * 12,), np.uint8)
    ctx.free(rows_dev)
    ctx.free(buf)
    return raw[len(q) * k * 8:].view(np.float32).reshape(len(q), k), raw[:len(q) * k * 8].view(np.int64).reshape(len(q), k)


# ---- fp32 shard: ip_scan_kernel<float, QB>, ip_scan_rows_kernel<QB, 4>, cert_refine_kernel -------------------------------------------------
@pytest.mark.parametrize("dim,n", [(d, n) for d in (512, 4096) for n in (1, 3, 4, 5, 1027)] + [(512, 0)])
def test_fp32_kernels_every_row(omni, ctx, dim, n):
    """n = 0 stands for 8 CUs 4 4 + 3 rows: both kernels take a second grid-stride iteration, and the rows kernel's last group is ragged (it re-reads its clamped
    last row)."""
    c = omni.capi
    big = n == 0
    if big:
        n = 8 * _cus(ctx) * 4 * 4 + 3
    rows = R.unit_rows(n, dim, seed=100 + dim + n % 97)
    q = R.queries(rows, 8, seed=7, special=False)
    q[6] *= np.float32(-1.0)                                                   # the own-row score negative: the other half of the key's order map
    idx = _shard(omni, ctx, rows, False)
    ref, emul = R.f32_ref(q, rows), R.valu_emul(q, rows)
    classes = R.valu_classes(8, n, 4)
    sub = lambda d, qb: {k: v[:qb] for k, v in d.items()}
    one = np.concatenate([idx.debug_scan(c.SCAN_F32, q[i:i + 1]) for i in range(8)])           # ip_scan_kernel<float, 1>, query by query
    _gate(f"dim {dim} n {n} QB 1 x 8", "f32", one, ref, emul, classes)
    for qb in ((4, 8) if big else range(2, 9)):
        r = R.Ref(ref.y[:qb], ref.E[:qb], ref.T[:qb])
        keys = idx.debug_scan(c.SCAN_F32, q[:qb])
        _gate(f"dim {dim} n {n} QB {qb}", "f32", keys, r, emul[:qb], sub(classes, qb))
        assert np.array_equal(keys, one[:qb]), ("ip_scan_kernel<float, QB> != <float, 1>", qb)
        if qb >= 4:
            keys = idx.debug_scan(c.SCAN_F32_ROWS, q[:qb])
            _gate(f"dim {dim} n {n} rows QB {qb}", "f32", keys, r, emul[:qb], sub(classes, qb))
            assert np.array_equal(keys, one[:qb]), ("ip_scan_rows_kernel<QB, 4> != ip_scan_kernel<float, 1>", qb)
    # per-query limits inside a block: 0, inside a group of 4 rows, beyond n
    lim = [0, max(n - 2, 0), n + 50, n, max(n // 2, 1), 1, n, max(n - 1, 0)]
    for which in (c.SCAN_F32, c.SCAN_F32_ROWS):
        keys = idx.debug_scan(which, q, limits=lim)
        _check_keys(keys, n, lim)
        assert np.array_equal(keys[keys != R.KEY_EMPTY], one[keys != R.KEY_EMPTY])
    # a production search's results are the largest keys (one query: ip_scan_kernel<float, 1>; eight: the mirror pass + cert_refine_kernel + the certificate)
    k = 32
    D1, I1 = idx.search(q[:1], k)
    Dt, It = _top(one[0], k)
    assert np.array_equal(D1[0], Dt) and np.array_equal(I1[0], It)
    served0, fall0 = idx.cert_stats()
    D, I = _batch(ctx, idx, q, k, [n] * 8)                                     # kp = 64 candidates: with n <= 32 EVERY row is re-scored by cert_refine_kernel
    served, fall = idx.cert_stats()
    assert served - served0 == 8, "the batch went through the mirror pass and cert_refine_kernel"
    if n <= k:
        assert fall == fall0                                                   # every row a candidate: exact by construction, cert_refine_kernel's bits
    for j in range(8):
        Dt, It = _top(one[j], k)
        assert np.array_equal(D[j], Dt) and np.array_equal(I[j], It), ("cert_refine_kernel != ip_scan_kernel<float, 1>", j)
    idx.close()


@pytest.mark.parametrize("dim", [512, 4096])
def test_cert_refine_kernel_every_row_of_32(omni, ctx, dim):
    """32 rows, k = 32, 64 candidates: every score of the batched search is cert_refine_kernel's; all of them equal ip_scan_kernel<float, 1>'s bits and meet tier 1."""
    c = omni.capi
    rows = R.unit_rows(32, dim, seed=dim + 5)
    q = R.queries(rows, 8, seed=8, special=False)
    idx = _shard(omni, ctx, rows, False)
    one = np.concatenate([idx.debug_scan(c.SCAN_F32, q[i:i + 1]) for i in range(8)])
    D, I = _batch(ctx, idx, q, 32, [32] * 8)
    assert idx.cert_stats() == (8, 0)
    ref = R.f32_ref(q, rows)
    for j in range(8):
        Dt, It = _top(one[j], 32)
        assert np.array_equal(D[j], Dt) and np.array_equal(I[j], It)
        got = np.empty(32)
        got[I[j]] = D[j]
        assert R.tier1(got[None], R.Ref(ref.y[j:j + 1], ref.E[j:j + 1], ref.T[j:j + 1])) <= 1.0
    idx.close()


# ---- fp16 shard: ip_scan_t16_kernel<QB> ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(512, n) for n in (1, 15, 16, 17, 1000)] + [(4096, 17), (4096, 1000), (512, 0)])
def test_fp16_valu_kernel_every_row(omni, ctx, monkeypatch, dim, n):
    """n = 0 stands for 8 CUs 4 16 + 16 3 + 5 rows: a second grid-stride iteration over 16-row blocks, the last block ragged."""
    c = omni.capi
    monkeypatch.setenv("OMNI_MQ_MIN", "0")                                     # searches of this handle stay on the VALU kernel
    big = n == 0
    if big:
        n = 8 * _cus(ctx) * 4 * 16 + 16 * 3 + 5
    nq = 2 if big else 8
    rows = R.unit_rows(n, dim, seed=200 + dim + n % 97)
    rows16 = R.h16(rows)
    q = R.queries(rows16, nq, seed=9, special=False)
    q[nq - 1] *= np.float32(-1.0)
    idx = _shard(omni, ctx, rows, True)
    ref, emul = R.t16_ref(q, rows16), R.t16_emul(q, rows16)
    classes = R.valu_classes(nq, n, 16)
    sub = lambda d, qb: {k: v[:qb] for k, v in d.items()}
    full = idx.debug_scan(c.SCAN_T16, q)
    _gate(f"dim {dim} n {n} QB {nq}", "t16", full, ref, emul, classes)
    for qb in (() if big else range(1, 8)):
        keys = idx.debug_scan(c.SCAN_T16, q[:qb])
        _gate(f"dim {dim} n {n} QB {qb}", "t16", keys, R.Ref(ref.y[:qb], ref.E[:qb], ref.T[:qb]), emul[:qb], sub(classes, qb))
        assert np.array_equal(keys, full[:qb]), ("a query's score does not depend on its block", qb)
    lim = ([0, n + 9] if big else [0, max(n - 5, 0), n + 50, n, max(n // 2, 1), 1, n, max(n - 1, 0)])
    keys = idx.debug_scan(c.SCAN_T16, q, limits=lim)
    _check_keys(keys, n, lim)
    assert np.array_equal(keys[keys != R.KEY_EMPTY], full[keys != R.KEY_EMPTY])
    k = min(10, n)
    D, I = idx.search(q, k)                                                    # production: the same kernel, the largest keys
    for j in range(nq):
        Dt, It = _top(full[j], k)
        assert np.array_equal(D[j], Dt) and np.array_equal(I[j], It)
    idx.close()


# ---- ip_scan_mq_kernel on fp16 rows and on an fp32 shard's mirror ------------------------------------------------------------------------------
MARGIN = {"budget": 0.0}                        # largest (mirror scan's own error) / (4e-6 |q| max |row|) seen: the certificate's arithmetic budget


def _mirror_checks(tag, got, q, rows, rows16, valid):
    """Every mirror score against the exact fp32-row score and the certificate's eps (inf for a query the kernel never certifies); the share of the arithmetic
    budget the scan itself uses, over the certifiable queries."""
    q64 = q.astype(np.float64)
    exact = q64 @ rows.astype(np.float64).T
    eps = R.cert_eps(q, rows)[:, None]
    d = np.abs(got - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(valid & (eps > 0), d / np.where(eps > 0, eps, 1.0), np.where(valid & (d > 0), np.inf, 0.0))
    assert (rel <= 1.0).all(), (tag, float(rel.max()))
    own = np.abs(got - q64 @ rows16.astype(np.float64).T)
    budget = float(R.CERT_ARITH) * np.sqrt((q64 ** 2).sum(axis=1)) * np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max())
    live = (budget > 0) & np.isfinite(eps[:, 0])
    share = np.where(valid[live], own[live] / budget[live, None], 0.0).max(axis=1) if live.any() else np.zeros(1)
    MARGIN["budget"] = max(MARGIN["budget"], float(share.max()))
    print(f"[mirror] {tag}: worst |mirror - exact| / eps {float(rel.max()):.4f}; scan error / arithmetic budget {float(share.max()):.4f} (so far {MARGIN['budget']:.4f})")


def _mq_case(omni, ctx, dim, n, nqs, rotates, seed, with_limits=False, search_k=0):
    """One shard of each kind -- fp16 rows, and fp32 rows whose mirror holds the same halfs -- against one reference and one emulation."""
    c = omni.capi
    rows = R.unit_rows(n, dim, seed=seed)
    rows16 = R.h16(rows)
    shards = [(False, _shard(omni, ctx, rows, True)), (True, _shard(omni, ctx, rows, False))]
    grid = min((n + 511) // 512, _cus(ctx))
    for nq in nqs:
        q = R.queries(rows16, nq, seed=seed + nq, special=True)
        ref = R.mq_ref(q, rows16)
        classes = R.mq_classes(nq, n, grid)
        for rot in rotates:
            emul = R.mq_emul(q, rows16, rot)
            for mirror, idx in shards:
                which = c.SCAN_MQ_MIRROR if mirror else c.SCAN_MQ
                tag = f"{'mirror' if mirror else 'fp16'} dim {dim} n {n} nq {nq} rot {int(rot)}"
                keys = idx.debug_scan(which, q, rotate=rot)
                got = _gate(tag, "mq", keys, ref, emul, classes)
                if mirror:
                    _mirror_checks(tag, got, q, rows, rows16, np.ones(got.shape, bool))
                if with_limits:
                    lim = np.random.default_rng(nq).integers(1, n + 1, nq)
                    lim[0] = 0
                    lim[-1] = n + 50
                    if nq > 2:
                        lim[1] = max(n - 7, 0)                                 # inside a 16-row tile
                    kl = idx.debug_scan(which, q, limits=lim, rotate=rot)
                    _check_keys(kl, n, lim)
                    assert np.array_equal(kl[kl != R.KEY_EMPTY], keys[kl != R.KEY_EMPTY])
                if search_k and rot and not mirror and nq >= 4:                # production (OMNI_MQ_ROT at its default): the same kernel, the largest keys
                    D, I = idx.search(q, min(search_k, n))
                    for j in range(nq):
                        Dt, It = _top(keys[j], min(search_k, n))
                        assert np.array_equal(D[j], Dt) and np.array_equal(I[j], It)
    for _, idx in shards:
        idx.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 511, 512, 513, 1029])
def test_matrix_core_scan_every_row(omni, ctx, n):
    """dim 4096, fp16 rows and an fp32 shard's mirror; 1, 4, 63 and 64 queries (slot 0 x 37.5, 1 x 1e-3, 2 x 1e30, 3 all zero, 4 one element 2^20 times the rest,
    5 x 1e-32); from 513 rows on a second block, whose rotation differs: rotation on and off; limits of 0, inside a 16-row tile and beyond n."""
    _mq_case(omni, ctx, 4096, n, (1, 4, 63, 64), (True, False) if n > 512 else (True,), seed=300 + n, with_limits=True, search_k=10)


def test_matrix_core_scan_all_rotations(omni, ctx):
    """dim 4096, 16 512 + 83 rows: seventeen 512-row blocks, all 16 rotations and one wrap, rotation on and off."""
    _mq_case(omni, ctx, 4096, 16 * 512 + 83, (64,), (True, False), seed=400)


@pytest.mark.parametrize("dim,nq", [(512, 16), (1024, 4)])
def test_matrix_core_scan_three_passes(omni, ctx, dim, nq):
    """n = 2 CUs 512 + 512 7 + 16 9 + 3: the first workgroups walk three passes, the others two; the last block is ragged and has clamped tiles."""
    n = 2 * _cus(ctx) * 512 + 512 * 7 + 16 * 9 + 3
    _mq_case(omni, ctx, dim, n, (nq,), (True,), seed=500 + dim)


# ---- the mirror pass against its certificate, end to end -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
def test_victim_row_is_saved_by_a_sound_certificate(omni, ctx, k):
    """The scene of index_scan_ref.victim_scene (its margins are asserted in float64 first): the mirror ranks kp - k + 1 fillers above the worst-case victim row,
    the true k-th neighbour, so the victim is no candidate.  A sound certificate refuses (the best filler's exact score is not above the kp-th mirror score by
    eps), and the exact scan returns the victim.  With eps halved the kernel would certify and lose it; with other constants than cert_eps restates, this
    test's certificate check of every row or its fallback count fails."""
    c = omni.capi
    rows, qv, victim, fillers = R.victim_scene(4096, k, seed=40 + k)
    kp = max(k + 24, 2 * k)
    assert kp == (25 if k == 1 else 34)
    r64, q64 = rows.astype(np.float64), qv.astype(np.float64)
    exact, mirror = r64 @ q64, R.h16(rows).astype(np.float64) @ q64
    assert (mirror[fillers] - mirror[victim] >= 1e-5).all() and (exact[victim] - exact[fillers] >= 1e-5).all()
    rng = np.random.default_rng(k)
    others = np.setdiff1d(np.arange(len(rows)), np.concatenate([fillers, [victim]]))
    bg = [o for o in others if abs(exact[o]) < 0.5][:2]                        # two background rows: queries near them certify
    q = np.stack([qv, rows[bg[0]] + 0.002 * rng.standard_normal(4096), qv * 2.0, rows[bg[1]] + 0.002 * rng.standard_normal(4096)]).astype(np.float32)
    idx = _shard(omni, ctx, rows, False)
    # every row of the scene, the worst-case row among them, within the certificate's eps
    keys = idx.debug_scan(c.SCAN_MQ_MIRROR, q)
    sc, valid = _check_keys(keys, len(rows))
    _mirror_checks(f"victim scene k {k}", sc.astype(np.float64), q, rows, R.h16(rows), valid)
    gap = exact[victim] - float(sc[0, victim])
    eps = float(R.cert_eps(q[:1], rows)[0])
    print(f"[victim k {k}] exact - mirror score of the victim {gap:.4e}, eps {eps:.4e}")
    assert 0.5 * eps < gap <= eps
    served0, fall0 = idx.cert_stats()
    D, I = _batch(ctx, idx, q, k, [len(rows)] * 4)
    served, fall = idx.cert_stats()
    ids, sco = R.oracle_topk(q, rows, k)
    assert np.array_equal(I, ids), (I.tolist(), ids.tolist())
    assert I[0, k - 1] == victim and I[2, k - 1] == victim
    assert np.allclose(D, sco, rtol=1e-5, atol=1e-6)
    assert served - served0 == 4 and fall - fall0 == 2, (served, fall)         # the two victim queries, and only they
    idx.close()


def test_uncertifiable_rows_fall_back_and_subnormal_rows_stay_exact(omni, ctx):
    """A row with an element of 7e4 is inf in the mirror: no query of that shard may be certified.  Rows whose elements are fp16 subnormals (< 6e-5) lose
    absolute, not relative, accuracy in the mirror -- the 6e-8 |q|_1 term -- probed by a query of large |q|_1 (all elements of equal magnitude)."""
    c = omni.capi
    dim, k = 512, 5
    rng = np.random.default_rng(77)
    rows = R.unit_rows(300, dim, seed=78)
    rows[100:200] *= np.float32(2e-4)                                          # elements ~ 1e-5: fp16 subnormals
    q = np.stack([rows[3], rows[150] * 5000, np.where(rng.random(dim) < 0.5, -1.0, 1.0), rows[250] + 0.01 * rng.standard_normal(dim)]).astype(np.float32)
    q[2] = np.abs(q[2]) * np.sign(rows[120] + 1e-30)                            # |q|_1 = sqrt(dim) |q|, aligned with a subnormal row
    idx = _shard(omni, ctx, rows, False)
    keys = idx.debug_scan(c.SCAN_MQ_MIRROR, q)
    sc, valid = _check_keys(keys, len(rows))
    _mirror_checks("subnormal rows", sc.astype(np.float64), q, rows, R.h16(rows), valid)
    D, I = _batch(ctx, idx, q, k, [len(rows)] * 4)
    ids, sco = R.oracle_topk(q, rows, k)
    assert np.array_equal(I, ids) and np.allclose(D, sco, rtol=1e-5, atol=1e-7)
    assert idx.cert_stats()[0] == 4
    # queries of magnitude 1e-32 and 1e30: the fp32 norm under eps vanishes / overflows and mq_prep_kernel's shift is clamped: never certified, still exact
    served0, fall0 = idx.cert_stats()
    qt = np.stack([q[0] * np.float32(1e-32), q[3] * np.float32(1e-30), q[0] * np.float32(1e30), q[3] * np.float32(1e-20)])
    assert np.isinf(R.cert_eps(qt, rows)).all()
    D, I = _batch(ctx, idx, qt, k, [len(rows)] * 4)
    ids, sco = R.oracle_topk(qt, rows, k)
    assert np.array_equal(I, ids) and np.allclose(D, sco, rtol=1e-5, atol=0)
    assert idx.cert_stats() == (served0 + 4, fall0 + 4)
    idx.close()
    rows[200, 17] = np.float32(7e4)
    idx = _shard(omni, ctx, rows, False)
    D, I = _batch(ctx, idx, q, k, [len(rows)] * 4)
    ids, sco = R.oracle_topk(q, rows, k)
    assert np.array_equal(I, ids) and np.allclose(D, sco, rtol=1e-5, atol=1e-7)
    assert idx.cert_stats() == (4, 4)                                          # nothing certified over a row fp16 cannot hold
    idx.close()


# ---- the hook itself -----------------------------------------------------------------------------------------------------------------------
def test_debug_scan_leaves_the_handle_as_it_was_and_refuses_what_does_not_fit(omni, ctx):
    c = omni.capi
    rows = R.unit_rows(700, 512, seed=1)
    q = R.queries(rows, 8, seed=2, special=False)
    f32, f16 = _shard(omni, ctx, rows, False), _shard(omni, ctx, rows, True)
    before = [(x.search(q, 10), _batch(ctx, x, q, 10, [700] * 8), x.cert_stats()) for x in (f32, f16)]
    ms = [x.last_scan_ms() for x in (f32, f16)]
    for which in (c.SCAN_F32, c.SCAN_F32_ROWS, c.SCAN_MQ_MIRROR):
        f32.debug_scan(which, q)
    for which in (c.SCAN_T16, c.SCAN_MQ):
        f16.debug_scan(which, q)
    assert [x.last_scan_ms() for x in (f32, f16)] == ms
    for x, (s, b, st) in zip((f32, f16), before):
        assert x.cert_stats() == st
        s2, b2 = x.search(q, 10), _batch(ctx, x, q, 10, [700] * 8)
        assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(s + b, s2 + b2))
    for x, which, qq in ((f32, c.SCAN_T16, q), (f32, c.SCAN_MQ, q), (f16, c.SCAN_F32, q), (f16, c.SCAN_F32_ROWS, q), (f16, c.SCAN_MQ_MIRROR, q),
                         (f32, c.SCAN_F32_ROWS, q[:3]), (f32, 9, q), (f32, c.SCAN_F32, np.concatenate([q, q[:1]]))):
        with pytest.raises(c.OmniError):
            x.debug_scan(which, qq)
    with pytest.raises(c.OmniError):
        f32.debug_scan(c.SCAN_F32, q, n=701)
    sharded = _shard(omni, ctx, rows, False)
    sharded.set_shard(0, 2)                                                    # gives up its mirror
    with pytest.raises(c.OmniError):
        sharded.debug_scan(c.SCAN_MQ_MIRROR, q)
    for x in (f32, f16, sharded):
        x.close()
