"""CPU gate of the correspondence stage (csrc/corr_plan.h through omni_corr_assemble_host of libomni_hip.so, no GPU): what the kernel of csrc/corr_assemble.hip must
equal, against LoopGeometry::compute_correspond_features itself -- the frame-pair function of host/loop_geometry.hpp run by omni_verify_correspond_host on two frames
built from the case, with a stub matcher that returns the case's match lists and a homography hook that returns its masks.  No tolerance: n_corr, every pair's
new_idx / old_idx, the bits of X (the new frame's landmarks_3d) and of u (the old frame's landmarks_2d_norm rotated by dq_old and cast to float), the function's
return value and compute_loop_core's size gate as the stage's gate, matched_dir_count as the per-pair counts give it.  The quaternions dq_old are the host
function's own (it hands them back): the quaternion algebra stays on the host.  tests/test_gpu_corr_assemble.py runs the same cases through the kernel."""
import numpy as np
import pytest

SELF_THRESHOLDS = dict(min_match_pre_dir=15, min_direction_loop=3, min_loop_num=30, init_min=10)


def quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def make_pair(rng, n_matches, n_flagged=None, status=None, nq=None, nt=None, keep_share=0.7):
    """a pair with n_matches matches in the matcher's order (ascending query index), n_flagged of them on flagged key points; the mask keeps about keep_share"""
    from omni_swarm_amd import capi as c
    nq = nq if nq is not None else n_matches + int(rng.integers(1, 9))
    nt = nt if nt is not None else n_matches + int(rng.integers(1, 9))
    q_idx = np.sort(rng.choice(nq, n_matches, replace=False)).astype(np.int32)
    t_idx = rng.choice(nt, n_matches, replace=False).astype(np.int32)
    n_flagged = n_matches if n_flagged is None else n_flagged
    flags = (rng.random(nq) < 0.5).astype(np.uint8)
    flags[q_idx] = 0
    flags[rng.choice(q_idx, n_flagged, replace=False)] = 1 if n_flagged else 0
    if status is None:
        status = c.HG_UNFILTERED if n_flagged < 4 else c.HG_OK
    mask = (rng.random(n_flagged) < keep_share).astype(np.uint8) if status != c.HG_NO_MODEL else np.zeros(n_flagged, np.uint8)
    if n_matches >= 30 and rng.random() < 0.3:
        flags = flags[:max(1, int(q_idx.max(initial=0)) + (0 if rng.random() < 0.5 else 1))]      # landmarks_flag shorter than the key points: the tail counts as unflagged
    return dict(q_idx=q_idx, t_idx=t_idx, q_flags=flags, nq=nq, nt=nt, mask=mask, hg_status=status, q_3d=rng.normal(size=(nq, 3)) * 3, t_norm=rng.normal(size=(nt, 2)) * 0.6,
                dq_old=[1, 0, 0, 0])


def case(name, rng, max_dirs, main_new, main_old, steps, pairs, init_mode=0, **thr):
    t = dict(SELF_THRESHOLDS, **thr)
    return dict(name=name, max_dirs=max_dirs, main_new=main_new, main_old=main_old, steps=steps, pairs=pairs, init_mode=init_mode, thr=t,
                old_quat=np.array([quat(rng) for _ in range(max_dirs)]))


def cases():
    from omni_swarm_amd import capi as c
    rng = np.random.default_rng(2024)
    P = lambda *a, **k: make_pair(rng, *a, **k)
    out = [
        case("one pair, five matches", rng, 1, 0, 0, [1], [P(5)], min_match_pre_dir=3, min_direction_loop=1, min_loop_num=2),
        case("four pairs, main directions 1 and 3 (wrap-around)", rng, 4, 1, 3, [1, 1, 1, 1], [P(40), P(37), P(52), P(33)]),
        case("a pair with three flagged matches keeps them unfiltered", rng, 4, 0, 0, [1, 1, 1, 1], [P(40), P(20, 3), P(45), P(39)]),
        case("a pair with no matches", rng, 4, 2, 1, [1, 1, 1, 1], [P(40), P(0), P(45), P(39)]),
        case("a missing direction", rng, 4, 3, 0, [1, 0, 1, 1], [P(40), P(45), P(39)]),
        case("fails MIN_DIRECTION_LOOP", rng, 4, 0, 2, [1, 1, 1, 1], [P(40), P(9), P(12), P(39)]),
        case("the size gate, out of init_mode: 25 correspondences are not more than 30", rng, 1, 0, 0, [1], [P(25, keep_share=1.1)], min_direction_loop=1),
        case("the size gate, in init_mode: 25 are more than 10", rng, 1, 0, 0, [1], [P(25, keep_share=1.1)], init_mode=1, min_direction_loop=1),
        case("the size gate, in init_mode: 10 are not", rng, 1, 0, 0, [1], [P(10, keep_share=1.1)], init_mode=1, min_direction_loop=1, min_match_pre_dir=5),
        case("no model: every mask entry 0", rng, 4, 0, 0, [1, 1, 1, 1], [P(40), P(30, status=c.HG_NO_MODEL), P(45), P(39)]),
        case("nothing at all", rng, 2, 0, 1, [1, 1], [P(0), P(6, 0)], min_direction_loop=0, min_match_pre_dir=0),
        case("exactly four flagged matches: filtered", rng, 1, 0, 0, [1], [P(9, 4)], min_match_pre_dir=1, min_direction_loop=1, min_loop_num=0),
    ]
    for n in (63, 64, 65, 255, 256, 257):                      # the wave and workgroup boundaries of the kernel's compaction
        out.append(case(f"{n} matches", rng, 2, 1, 0, [1, 1], [P(n), P(n, n - 1)]))
    return out


def to_call(cs, first=0):
    """-> (cand tuple, pairs) of one case whose pairs start at `first`"""
    t = cs["thr"]
    return (first, len(cs["pairs"]), t["min_match_pre_dir"], t["min_direction_loop"], t["min_loop_num"], t["init_min"], cs["init_mode"]), cs["pairs"]


def reference(cs):
    """compute_correspond_features on the case -> its result, with dq_old written into the case's pairs"""
    from omni_swarm_amd import pipeline
    cand, pairs = to_call(cs)
    ref = pipeline.verify_correspond_host([cand], pairs, 0, cs["max_dirs"], cs["main_new"], cs["main_old"], cs["steps"], cs["old_quat"])
    for j, p in enumerate(pairs):
        p["dq_old"] = ref["dq_old"][j]
    return ref


def assert_equals_reference(cs, ref, got_cand, got_pairs):
    from omni_swarm_amd import capi as c
    t = cs["thr"]
    assert got_cand["n_corr"] == ref["n_corr"], cs["name"]
    assert got_cand["X"].tobytes() == ref["X"].tobytes() and got_cand["u"].tobytes() == ref["u"].tobytes(), cs["name"]
    for j in range(len(cs["pairs"])):
        assert np.array_equal(got_pairs[j]["new_idx"], ref["new_idx"][j]) and np.array_equal(got_pairs[j]["old_idx"], ref["old_idx"][j]), (cs["name"], j)
    matched = sum(len(x) >= t["min_match_pre_dir"] for x in ref["new_idx"])
    assert got_cand["matched_dir_count"] == matched, cs["name"]
    assert ref["result"] == (ref["n_corr"] > 0 and matched >= t["min_direction_loop"]), cs["name"]      # (the test's own reading of the host function agrees with it)
    assert got_cand["gate"] == (c.CORR_OK if ref["result"] and ref["size_gate"] else c.CORR_REJECT), cs["name"]


def test_the_stage_equals_compute_correspond_features(omni):
    c = omni.capi
    seen = {"ok": 0, "reject": 0, "unfiltered": 0}
    for cs in cases():
        ref = reference(cs)
        cand, pairs = to_call(cs)
        (got,), got_pairs = c.corr_assemble([cand], pairs)
        assert_equals_reference(cs, ref, got, got_pairs)
        seen["ok" if got["gate"] == c.CORR_OK else "reject"] += 1
        seen["unfiltered"] += any(p["hg_status"] == c.HG_UNFILTERED and len(p["q_idx"]) for p in pairs)
    assert seen["ok"] >= 5 and seen["reject"] >= 4 and seen["unfiltered"] >= 2, seen      # conditions on the cases
    # the cases by name: what each is there for
    by = {cs["name"]: cs for cs in cases()}
    for name, gate in (("fails MIN_DIRECTION_LOOP", c.CORR_REJECT), ("the size gate, out of init_mode: 25 correspondences are not more than 30", c.CORR_REJECT),
                       ("the size gate, in init_mode: 25 are more than 10", c.CORR_OK), ("the size gate, in init_mode: 10 are not", c.CORR_REJECT),
                       ("a missing direction", c.CORR_OK), ("nothing at all", c.CORR_REJECT)):
        cs = by[name]
        reference(cs)
        (got,), _ = c.corr_assemble(*[[to_call(cs)[0]], to_call(cs)[1]])
        assert got["gate"] == gate, name
    cs = by["a pair with three flagged matches keeps them unfiltered"]
    reference(cs)
    _, gp = c.corr_assemble([to_call(cs)[0]], to_call(cs)[1])
    assert len(gp[1]["new_idx"]) == 3


def test_several_candidates_in_one_call_and_a_pair_handed_back(omni):
    """three candidates with 0, 1 and 4 pairs in one call equal the same candidates alone; a pair with status HOST marks its candidate for the host"""
    c = omni.capi
    by = {cs["name"]: cs for cs in cases()}
    one, four = by["one pair, five matches"], by["four pairs, main directions 1 and 3 (wrap-around)"]
    reference(one); reference(four)
    alone = [c.corr_assemble([to_call(cs)[0]], to_call(cs)[1]) for cs in (one, four)]
    empty = (0, 0, 15, 3, 30, 10, 0)
    got, got_pairs = c.corr_assemble([empty, to_call(one, 0)[0], to_call(four, 1)[0]], one["pairs"] + four["pairs"])
    assert (got[0]["n_corr"], got[0]["matched_dir_count"], got[0]["gate"]) == (0, 0, c.CORR_REJECT)
    for k, (cand_alone, pairs_alone) in enumerate(alone):
        g = got[k + 1]
        assert (g["n_corr"], g["matched_dir_count"], g["gate"]) == (cand_alone[0]["n_corr"], cand_alone[0]["matched_dir_count"], cand_alone[0]["gate"])
        assert g["X"].tobytes() == cand_alone[0]["X"].tobytes() and g["u"].tobytes() == cand_alone[0]["u"].tobytes()
    assert all(np.array_equal(a["new_idx"], b["new_idx"]) for a, b in zip(got_pairs, alone[0][1] + alone[1][1]))
    handed = [dict(p) for p in four["pairs"]]
    handed[2]["hg_status"] = c.HG_HOST
    (g,), _ = c.corr_assemble([to_call(four)[0]], handed)
    assert g["gate"] == c.CORR_HOST


def test_every_refusal(omni):
    c = omni.capi
    from omni_swarm_amd import pipeline
    cs = cases()[0]
    reference(cs)
    cand, pairs = to_call(cs)
    for cands, kw, word in (([], {}, "n_cands"), ([(0, 5, 1, 1, 1, 1, 0)], {}, "more than 4 pairs"), ([(1, 1, 1, 1, 1, 1, 0)], {}, "outside the call"),
                            ([(-1, 1, 1, 1, 1, 1, 0)], {}, "outside the call"), ([cand], {"max_n": 2000}, "max_n"), ([cand], {"cap": 3}, "cap below"),
                            ([cand], {"cap": 5000}, "cap outside"), ([cand] * 65, {}, "n_cands")):
        with pytest.raises(c.OmniError, match=word):
            c.corr_assemble(cands, pairs, **kw)
    with pytest.raises(c.OmniError, match="n_pairs"):
        c.corr_assemble([cand], pairs * 65)
    assert c.lib().omni_corr_assemble_host(None) == c.ERR_INVALID and b"null argument" in c.lib().omni_last_error()
    handed = [dict(pairs[0], hg_status=c.HG_HOST)]
    with pytest.raises(c.OmniError, match="OMNI_HG_HOST"):
        pipeline.verify_correspond_host([cand], handed, 0, 1, 0, 0, [1], cs["old_quat"])
    with pytest.raises(c.OmniError, match="pair_count steps"):
        pipeline.verify_correspond_host([cand], pairs, 0, 1, 0, 0, [0], cs["old_quat"])
    with pytest.raises(c.OmniError, match="out of range"):
        pipeline.verify_correspond_host([cand], pairs, 0, 1, 1, 0, [1], cs["old_quat"])
