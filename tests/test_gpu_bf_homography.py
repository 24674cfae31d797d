"""The fused entry (omni_bf_match_homography_multi: matcher, flag filter and homography RANSAC in one GPU round trip) against omni_bf_match_multi followed by the
CPU build of csrc/ransac_plan.h (tests/cpp/ransac_plan_pin.cpp) on the matcher's own lists: the match lists, the kept list, status, mask, info and the bits of H
identical.  Descriptor sets of 0, 1, 7, 100 and 200 key points, flags that drop none, some or all matches or end in front of the last key points, and pairs of
different sizes in one call."""
import ctypes

import numpy as np
import pytest

from tests import homography_cases as Hc

pytestmark = pytest.mark.gpu


def make_pair(omni, seed, nq, nt, flags="some", share=0.7):
    """descriptors of a noisy permutation (most key points have their partner), the old image's pixels random, `share` of the new image's key points at the
    homography of their partner's pixel"""
    from omni_swarm_amd import synth
    rng = np.random.default_rng(seed)
    n = max(nq, nt)
    a, b, perm = synth.local_descriptors(n, 64, seed, pair_noise=0.15) if n else (np.zeros((0, 64), np.float32), np.zeros((0, 64), np.float32), np.zeros(0, np.int64))
    q, t = a[:nq], b[:nt]                                                       # b[j] is the partner of a[perm[j]]
    t_xy = np.stack([rng.uniform(20, 580, nt), rng.uniform(20, 460, nt)], 1)
    q_xy = np.stack([rng.uniform(20, 580, nq), rng.uniform(20, 460, nq)], 1)
    for j in range(nt):
        i = perm[j]
        if i < nq and rng.uniform() < share:
            q_xy[i] = 1.02 * t_xy[j] + np.array([7.0, -4.0]) + rng.uniform(-0.5, 0.5, 2)
    f = {"none": np.ones(nq, np.uint8), "all": np.zeros(nq, np.uint8), "some": (rng.uniform(size=nq) < 0.7).astype(np.uint8), "short": np.ones(nq, np.uint8)[:nq * 2 // 3]}[flags]
    return (np.ascontiguousarray(q), np.ascontiguousarray(t), q_xy.astype(np.float32), t_xy.astype(np.float32), f)


CALLS = {
    "one pair of 200": [(1, 200, 200, "some")],
    "two sizes": [(2, 200, 100, "none"), (3, 7, 100, "some")],
    "small and empty sets": [(4, 0, 0, "none"), (5, 1, 1, "none"), (6, 7, 7, "none"), (7, 0, 100, "none"), (8, 100, 0, "some"), (9, 1, 200, "none"), (10, 7, 1, "none")],
    "flags": [(11, 100, 100, "all"), (12, 100, 100, "short"), (13, 200, 200, "none"), (14, 100, 200, "some"), (15, 200, 7, "short")],
    "no common structure": [(16, 200, 200, "none", 0.0), (17, 100, 100, "some", 0.0)],
}


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return Hc.build_pin(tmp_path_factory.mktemp("ransac_plan"))


@pytest.mark.parametrize("name", list(CALLS))
def test_fused_entry_equals_matcher_then_cpu_build(omni, ctx, pin, name):
    c = omni.capi
    pairs = [make_pair(omni, *spec) for spec in CALLS[name]]
    got = c.bf_match_homography_multi(ctx, pairs)
    matched = c.bf_match_multi(ctx, [(p[0], p[1]) for p in pairs])
    cases = [{"q_idx": qi, "t_idx": ti, "q_xy": p[2], "t_xy": p[3], "flags": p[4]} for p, (qi, ti, _) in zip(pairs, matched)]
    ref = Hc.run_pin(pin, ("plan", 64), cases)
    bad = []
    for k, (g, m, r, p) in enumerate(zip(got, matched, ref, pairs)):
        same_matches = all(np.array_equal(x, y) for x, y in zip((g["q_idx"], g["t_idx"], g["dist"].view(np.uint32)), (m[0], m[1], m[2].view(np.uint32))))
        same_kept = np.array_equal(g["kept"], r["kept"][:r["n_kept"]])
        same_mask = len(g["mask"]) == r["n_kept"] and np.array_equal(g["mask"], r["mask"][:r["n_kept"]])
        same_info = g["info"].tolist() == [r["count"], r["iters_run"], r["best_iter"], r["max_good"]]
        hb = int((g["H"].view(np.uint64) != np.ascontiguousarray(r["H"]).view(np.uint64)).sum())
        print(f"{name} pair {k}: nq {len(p[0])} nt {len(p[1])} flags {len(p[4])} ({int(p[4].sum())} set): {len(m[0])} matches, kept {len(g['kept'])} / {r['n_kept']}, status {g['status']} / {r['status']}, "
              f"info {g['info'].tolist()}, inliers {int(g['mask'].sum())}; differing: matches {not same_matches}, kept {not same_kept}, mask {not same_mask}, info {not same_info}, H entries {hb}; "
              f"tied eigenvalues on the CPU {r['ties']}")
        assert r["ties"] == 0 and r["status"] != Hc.HOST
        if not (same_matches and same_kept and same_mask and same_info and hb == 0 and g["status"] == r["status"]):
            bad.append(k)
    assert bad == []


def test_the_calls_reach_every_path(omni, ctx):
    """not vacuous: pairs with a model, pairs below four flagged matches, a pair that runs all 2 000 iterations"""
    c = omni.capi
    got = c.bf_match_homography_multi(ctx, [make_pair(omni, *s) for s in CALLS["one pair of 200"] + CALLS["no common structure"] + CALLS["flags"][:1]])
    assert got[0]["status"] == c.HG_OK and got[0]["mask"].sum() >= 30 and 0 < got[0]["info"][1] <= 64
    assert got[1]["info"][1] == 2000 and len(got[1]["kept"]) == len(got[1]["q_idx"]) >= 100
    assert got[3]["status"] == c.HG_UNFILTERED and len(got[3]["kept"]) == 0 and len(got[3]["q_idx"]) > 50


def test_refusals(omni, ctx):
    c = omni.capi
    lib = c.lib()
    q, t, qx, tx, f = make_pair(omni, 1, 8, 8, "none")
    P = 65
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    arr = lambda a: (fp * P)(*[a.ctypes.data_as(fp)] * P)
    fl = (ctypes.c_void_p * P)(*[f.ctypes.data] * P)
    n8 = np.full(P, 8, np.int32)
    outs_i = [np.zeros((P, 16), np.int32) for _ in range(6)]
    dd, mask, H = np.zeros((P, 16), np.float32), np.zeros((P, 16), np.uint8), np.zeros((P, 9))
    def call(pairs, max_n, nf=n8, flp=fl, dim=64):
        i = [a.ctypes.data_as(ip) for a in outs_i]
        return lib.omni_bf_match_homography_multi(ctx.h, pairs, arr(q), n8.ctypes.data_as(ip), arr(t), n8.ctypes.data_as(ip), dim, c.BF_OPENCV, max_n, arr(qx), arr(tx), flp,
                                                  nf.ctypes.data_as(ip), i[0], i[1], dd.ctypes.data_as(fp), i[2], i[3], i[4], mask.ctypes.data, H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  i[5], outs_i[2].ctypes.data_as(ip))
    for pairs, max_n, what in ((0, 8, "n_pairs=0"), (65, 8, "n_pairs=65"), (2, 0, "max_n=0"), (2, 1025, "max_n=1025"), (2, 7, "nq=8")):
        assert call(pairs, max_n) == c.ERR_CAPACITY and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
    assert call(2, 8, nf=np.full(P, 9, np.int32)) == c.ERR_CAPACITY and b"n_flags=9" in lib.omni_last_error()
    assert call(2, 8, flp=(ctypes.c_void_p * P)()) == c.ERR_INVALID and b"null" in lib.omni_last_error()
    assert call(2, 8, flp=None) == c.ERR_INVALID and b"null argument" in lib.omni_last_error()
    assert call(2, 8) == c.OK
