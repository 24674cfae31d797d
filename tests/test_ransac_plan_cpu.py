"""CPU gate of the loop-verification RANSAC's arithmetic (csrc/ransac_plan.h, what csrc/homography.hip spreads over lanes): built with g++ into
tests/cpp/ransac_plan_pin.cpp and compared with the host functions it restates -- geom::find_homography_ransac and the image-pair
LoopGeometry::compute_correspond_features -- on the seeded inputs of tests/homography_cases.py: ok, the mask, the BITS of the best H, iterations run, the best
iteration, max_good, the kept list and the reduced index lists.  The header takes the arg-min of the diagonal where the host sorts the eigenvalues: equal where the
smallest one is unique, so both programs count tied smallest eigenvalues and the count must be 0.  The LoopGeometry hook: tests/cpp/homography_hook_check.cpp."""
import os
import subprocess

import numpy as np
import pytest

from tests import homography_cases as Hc
from tests.test_geometry_cpu import frame_text, make_frame, scene      # noqa: F401  (the frame pairs of the geometry tests; `scene` is their fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return Hc.build_pin(tmp_path_factory.mktemp("ransac_plan"))


@pytest.fixture(scope="module")
def runs(pin):
    cases = Hc.gate_cases()
    return cases, {R: Hc.run_pin(pin, ("plan", R), cases) for R in (1, 64, 2000)}, Hc.run_pin(pin, ("host",), cases)


def test_header_equals_the_host_functions_bit_for_bit(runs):
    cases, plan, host = runs
    seen = {s: 0 for s in (Hc.UNFILTERED, Hc.OK, Hc.NO_MODEL, Hc.HOST)}
    full_runs = early_stops = 0
    for i, (c, a, b) in enumerate(zip(cases, plan[64], host)):
        print(f"case {i}: seed {c['seed']} count {c['count']} share {c['share']} {c['kind']}: kept {a['n_kept']} of {len(c['q_idx'])}, status header {a['status']} host {b['status']}, "
              f"iterations {a['iters_run']} / {b['iters_run']}, best {a['best_iter']} / {b['best_iter']}, inliers {a['max_good']} / {b['max_good']}, ties {a['ties']} / {b['ties']}")
        seen[a["status"]] += 1
        if i >= len(cases) - Hc.DEGENERATE:
            assert a["status"] == Hc.HOST, i                               # duplicated / collinear points: handed back
            assert a["n_kept"] == b["n_kept"] and np.array_equal(a["kept"], b["kept"])
            continue
        assert a["status"] != Hc.HOST, i                                      # a case cannot pass by falling back
        assert Hc.differing(a, b) == [], (i, Hc.differing(a, b))
        assert b["ties"] == 0 and a["ties"] == 0, i                           # the host code alone first: the inputs are inside what the arg-min form covers
        full_runs += a["iters_run"] == 2000
        early_stops += 0 < a["iters_run"] <= 64
    assert min(seen.values()) >= 1 and seen[Hc.OK] >= 30 and seen[Hc.UNFILTERED] >= 10, seen      # not vacuous
    assert full_runs >= 3 and early_stops >= 10, (full_runs, early_stops)     # rejected candidates run all 2 000 iterations, true loops stop inside the first round


def test_round_size_changes_nothing(runs):
    cases, plan, _ = runs
    for i in range(len(cases)):
        for R in (1, 2000):
            d = Hc.differing(plan[R][i], plan[64][i])
            assert d == [], (i, R, d)
    assert max(r["ties"] for r in plan[2000]) == 0                           # also among the hypotheses a larger round evaluates and throws away


def test_special_cases(runs, pin):
    cases, plan, host = runs
    by = {(c["count"], c["share"], len(c["q_idx"]) - c["count"]): r for c, r in zip(cases[:50], plan[64][:50])}
    assert by[(0, 0.0, 0)]["status"] == by[(3, 1.0, 0)]["status"] == Hc.UNFILTERED and by[(3, 1.0, 0)]["n_reduced"] == 3 and by[(3, 1.0, 0)]["ret"] == 0
    r = by[(4, 1.0, 0)]
    assert r["status"] == Hc.OK and r["mask"].tolist() == [1, 1, 1, 1] and (r["iters_run"], r["best_iter"], r["max_good"]) == (1, 0, 4)
    # the count-5 pair without a valid subset: NO_MODEL with no iteration run -- the host spends its 10 000 attempts and returns false
    i = len(cases) - Hc.DEGENERATE - 1
    assert cases[i]["seed"] == Hc.NO_SUBSET_SEED == Hc.find_no_subset_seed(pin, Hc.NO_SUBSET_SEED, 1)
    for r in (plan[64][i], host[i]):
        assert (r["status"], r["n_kept"], r["iters_run"], r["best_iter"], r["max_good"], r["ret"], r["n_reduced"]) == (Hc.NO_MODEL, 5, 0, -1, 0, 1, 0) and not r["mask"].any()
    # all matches dropped by the flags: nothing kept, nothing estimated
    for c, r in zip(cases, plan[64]):
        if c["count"] == 0 and len(c["q_idx"]):
            assert r["status"] == Hc.UNFILTERED and r["n_kept"] == 0 and r["n_reduced"] == 0
    # flags that drop some: the kept list is the flagged matches in match order
    some = 0
    for c, r in zip(cases, plan[64]):
        keep = [j for j, q in enumerate(c["q_idx"]) if q < len(c["flags"]) and c["flags"][q]]
        assert r["kept"][:r["n_kept"]].tolist() == keep
        some += 0 < len(keep) < len(c["q_idx"])
    assert some >= 8


def test_planted_inliers_are_found(runs):
    """sanity against the generator: the best model holds most of the planted correspondences.  Not all of them: it is a minimal-sample model from points with
    +- 0.5 pixel of noise, unrefined, and it may leave the 3-pixel band far from its four points -- half is what the check asks for; the gate is the bit
    comparison above"""
    cases, plan, _ = runs
    checked = 0
    for c, r in zip(cases[:50], plan[64][:50]):
        if c["count"] >= 30 and c["share"] >= 0.3:
            assert r["status"] == Hc.OK and 2 * r["max_good"] >= c["n_inliers_planted"], (c["seed"], r["max_good"], c["n_inliers_planted"])
            checked += 1
    assert checked == 20


def test_stop_rule_is_a_table_lookup(pin):
    """niters = RANSACUpdateNumIters(0.995, (count - good) / count, 4, niters) == min(T[good], niters): counts 5..200, good 4..count, niters 0..2000"""
    combos, bad = (int(v) for v in subprocess.run([pin, "scan"], capture_output=True, text=True, check=True).stdout.split())
    print(f"{combos} combinations, {bad} mismatches")
    assert combos == 39023502 and bad == 0


def test_loop_geometry_hook_changes_nothing(scene, tmp_path):
    """compute_loop with LoopGeometry::homography_mask fed by the host function, and by the header the GPU runs, returns the Correspondence and the LoopEdge of the
    run without a hook, field for field"""
    exe = str(tmp_path / "homography_hook_check")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "homography_hook_check.cpp"),
                           "-L", os.path.join(ROOT, "oracle"), "-loracle", f"-Wl,-rpath,{os.path.join(ROOT, 'oracle')}"])
    new, old = scene["new"], scene["old"]
    rng = np.random.default_rng(9)
    pts2 = rng.standard_normal((800, 3)) * 3 + np.array([0, 0, 1.0])
    d2 = rng.standard_normal((800, 64))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    other = make_frame(pts2, d2, scene["pose_new"], 11, 1, rng)              # a frame from another place: no loop
    text = "\n".join(f"{dn} {dold} {im} {is4}\n{frame_text(a)}\n{frame_text(old)}" for a, (dn, dold, im, is4) in
                     ((new, (1, 1, 0, 1)), (new, (1, 1, 1, 0)), (new, (0, 0, 0, 1)), (other, (1, 1, 0, 1))))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.strip().split("\n")]
    print(rows)
    assert len(rows) == 4 and all(x[0] == "HOOK" and x[2] == "1" and x[3] == "1" and x[5] == "0" for x in rows)
    assert [x[1] for x in rows] == ["1", "1", "1", "0"] and sum(int(x[4]) for x in rows) >= 12 and all(int(x[7]) > 100 for x in rows[:3])
