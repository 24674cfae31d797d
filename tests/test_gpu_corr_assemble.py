"""The correspondence kernel (csrc/corr_assemble.hip) against omni_corr_assemble_host, the g++ build of the same header (csrc/corr_plan.h), bit for bit: the cases of
tests/test_corr_plan_cpu.py -- which that file holds against LoopGeometry::compute_correspond_features -- the pairs of 63, 64, 65, 255, 256 and 257 matches among
them (the wave and workgroup boundaries of the compaction), three candidates with 0, 1 and 4 pairs in one call, and a pair the homography stage hands back, which
must come back marked for the host.  Then the fused entry (omni_bf_match_homography_corr_multi) on real descriptor sets: its matcher and homography outputs are
omni_bf_match_homography_multi's, and its correspondences are the host stage's on those very lists and masks."""
import numpy as np
import pytest

from tests import test_corr_plan_cpu as CP
from tests import test_gpu_bf_homography as BH

pytestmark = pytest.mark.gpu


def same(a, b):
    (ca, pa), (cb, pb) = a, b
    assert len(ca) == len(cb) and len(pa) == len(pb)
    for x, y in zip(ca, cb):
        assert (x["n_corr"], x["matched_dir_count"], x["gate"]) == (y["n_corr"], y["matched_dir_count"], y["gate"])
        assert x["X"].tobytes() == y["X"].tobytes() and x["u"].tobytes() == y["u"].tobytes()
    for x, y in zip(pa, pb):
        assert np.array_equal(x["new_idx"], y["new_idx"]) and np.array_equal(x["old_idx"], y["old_idx"])


@pytest.fixture(scope="module")
def cases(omni):
    out = CP.cases()
    for cs in out:
        CP.reference(cs)                                       # (writes the host function's dq_old into the pairs)
    return out


def test_kernel_equals_the_cpu_build_case_by_case(omni, ctx, cases):
    c = omni.capi
    for cs in cases:
        cand, pairs = CP.to_call(cs)
        host, dev = c.corr_assemble([cand], pairs), c.corr_assemble([cand], pairs, ctx)
        print(f"{cs['name']}: n_corr {dev[0][0]['n_corr']}, matched_dir_count {dev[0][0]['matched_dir_count']}, gate {dev[0][0]['gate']}, per pair {[len(p['new_idx']) for p in dev[1]]}")
        same(dev, host)
        CP.assert_equals_reference(cs, CP.reference(cs), dev[0][0], dev[1])      # ... and, through it, the host function itself


def test_every_case_in_calls_of_several_candidates(omni, ctx, cases):
    """all cases packed into calls of up to 64 pairs, an empty candidate in front: 0, 1, 2 and 4 pairs side by side"""
    c = omni.capi
    cands, pairs, calls = [(0, 0, 15, 3, 30, 10, 0)], [], 0
    for cs in cases + [None]:
        if cs is None or len(pairs) + len(cs["pairs"]) > 64:
            host, dev = c.corr_assemble(cands, pairs), c.corr_assemble(cands, pairs, ctx)
            same(dev, host)
            assert dev[0][0]["gate"] == c.CORR_REJECT and {cd[1] for cd in cands} >= {0, 1, 2}
            cands, pairs, calls = [(0, 0, 15, 3, 30, 10, 0)], [], calls + 1
        if cs is not None:
            cands.append(CP.to_call(cs, len(pairs))[0])
            pairs = pairs + cs["pairs"]
    assert calls >= 1


def test_a_pair_handed_back_marks_its_candidate_for_the_host(omni, ctx, cases):
    c = omni.capi
    four = next(cs for cs in cases if cs["name"].startswith("four pairs"))
    one = next(cs for cs in cases if cs["name"].startswith("one pair"))
    handed = [dict(p) for p in four["pairs"]]
    handed[1]["hg_status"] = c.HG_HOST
    cands = [CP.to_call(four, 0)[0], CP.to_call(one, 4)[0]]
    host, dev = c.corr_assemble(cands, handed + one["pairs"]), c.corr_assemble(cands, handed + one["pairs"], ctx)
    same(dev, host)
    assert dev[0][0]["gate"] == c.CORR_HOST and dev[0][1]["gate"] == c.CORR_OK      # ... and its neighbour is served


def test_refusals_on_the_device_entry(omni, ctx, cases):
    c = omni.capi
    cand, pairs = CP.to_call(cases[0])
    for cands, kw in (([(0, 5, 1, 1, 1, 1, 0)], {}), ([(1, 1, 1, 1, 1, 1, 0)], {}), ([cand], {"cap": 3}), ([cand], {"max_n": 2000})):
        with pytest.raises(c.OmniError):
            c.corr_assemble(cands, pairs, ctx, **kw)
    same(c.corr_assemble([cand], pairs, ctx), c.corr_assemble([cand], pairs))      # the context stays usable


def test_fused_entry_equals_its_parts(omni, ctx):
    """matcher + flag filter + homography RANSAC + correspondences in one round trip: candidates of 1, 4 and 2 pairs of 200 / 100 / 7 key points"""
    c = omni.capi
    rng = np.random.default_rng(5)
    specs = [(1, 200, 200, "some"), (2, 200, 100, "none"), (3, 7, 100, "some"), (12, 100, 100, "short"), (14, 100, 200, "some"), (16, 200, 200, "none", 0.0), (13, 200, 200, "none")]
    base = [BH.make_pair(omni, *s) for s in specs]
    pairs = []
    for q, t, q_xy, t_xy, f in base:
        dq = rng.normal(size=4)
        pairs.append((q, t, q_xy, t_xy, f, rng.normal(size=(len(q), 3)).astype(np.float32) * 4, rng.normal(size=(len(t), 2)).astype(np.float32) * 0.5, dq / np.linalg.norm(dq)))
    cands = [(0, 1, 15, 1, 30, 10, 0), (1, 4, 15, 3, 30, 10, 0), (5, 2, 15, 1, 30, 10, 1)]
    hg, got_c, got_p = c.bf_match_homography_corr_multi(ctx, pairs, cands)
    plain = c.bf_match_homography_multi(ctx, base)
    for g, r in zip(hg, plain):
        assert g["status"] == r["status"] and all(np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8), np.ascontiguousarray(r[k]).view(np.uint8))
                                                  for k in ("q_idx", "t_idx", "dist", "kept", "mask", "H", "info"))
    as_dicts = [dict(q_idx=g["q_idx"], t_idx=g["t_idx"], q_flags=p[4], nq=len(p[0]), nt=len(p[1]), mask=g["mask"], hg_status=g["status"], q_3d=p[5], t_norm=p[6], dq_old=p[7])
                for g, p in zip(hg, pairs)]
    host = c.corr_assemble(cands, as_dicts, max_n=200)
    print([(x["n_corr"], x["matched_dir_count"], x["gate"]) for x in got_c], [g["status"] for g in hg])
    same((got_c, got_p), host)
    assert got_c[0]["gate"] == c.CORR_OK and got_c[0]["n_corr"] > 30 and c.HG_HOST not in [g["status"] for g in hg]      # conditions on the inputs: not vacuous
