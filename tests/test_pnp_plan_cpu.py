"""CPU gate of the loop-verification PnP RANSAC's arithmetic (csrc/pnp_plan.h, what csrc/pnp.hip gives to its lanes): built with g++ into
tests/cpp/pnp_plan_pin.cpp and compared with the host functions it restates -- geom::ransac_run<PnPModel> and geom::solve_pnp_ransac -- on the seeded inputs of
tests/pnp_cases.py: status, the mask, the BITS of the best EPnP model, iterations run, the best iteration, max_good; and, with geom::pnp_refit behind the header,
solve_pnp_ransac's return value, the bits of its pose and its inlier list.  No case is left out: a difference is a bug in the header.  The LoopGeometry hook:
tests/cpp/pnp_hook_check.cpp.  The sanitizer pass runs the same stand-alone program built with -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

from tests import pnp_cases as Pc
from tests.test_geometry_cpu import frame_text, make_frame, scene      # noqa: F401  (the frame pairs of the geometry tests; `scene` is their fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return Pc.build_pin(tmp_path_factory.mktemp("pnp_plan"))


@pytest.fixture(scope="module")
def runs(pin):
    cases = Pc.gate_cases()
    return cases, {R: Pc.run_pin(pin, ("plan", R), cases) for R in (1, 64, 1000)}, Pc.run_pin(pin, ("host",), cases)


def test_header_equals_the_host_functions_bit_for_bit(runs):
    cases, plan, host = runs
    seen = {s: 0 for s in (Pc.SKIPPED, Pc.OK, Pc.NO_MODEL, Pc.HOST)}
    full_runs = early_stops = five = 0
    for i, (c, a, b) in enumerate(zip(cases, plan[64], host)):
        print(f"case {i}: seed {c['seed']} count {c['count']} share {c['share']} limit {c['max_iters']} {c['kind']}: status header {a['status']} host {b['status']}, "
              f"iterations {a['iters_run']} / {b['iters_run']}, best {a['best_iter']} / {b['best_iter']}, inliers {a['max_good']} / {b['max_good']}, "
              f"solve_pnp_ransac {a['ret']} / {b['ret']} with {a['n_inliers']} / {b['n_inliers']} inliers")
        seen[a["status"]] += 1
        assert a["status"] != Pc.HOST, i                                      # a case cannot pass by falling back
        assert Pc.differing(a, b) == [], (i, Pc.differing(a, b))
        assert a["ret"] == (a["status"] == Pc.OK), i                          # six inliers or more always refit (the DLT's failure falls back to the model)
        full_runs += a["iters_run"] == c["max_iters"] == 1000
        early_stops += 0 < a["iters_run"] <= 64 and c["max_iters"] >= 100
        five += a["status"] == Pc.NO_MODEL and a["max_good"] == 5
    assert seen[Pc.SKIPPED] == 10 and seen[Pc.OK] >= 60 and seen[Pc.NO_MODEL] >= 5, seen      # not vacuous; HOST is not reached by any gate case
    assert full_runs >= 5 and early_stops >= 25 and five >= 1, (full_runs, early_stops, five)  # 1 000 iterations to the end; stops inside the first round; the `< 6` rule


def test_round_size_changes_nothing(runs):
    cases, plan, _ = runs
    for i in range(len(cases)):
        for R in (1, 1000):
            d = Pc.differing(plan[R][i], plan[64][i])
            assert d == [], (i, R, d)


def test_degenerate_sets_terminate_with_the_host_result(runs):
    cases, plan, host = runs
    for i in range(len(cases) - Pc.DEGENERATE, len(cases)):
        assert cases[i]["kind"] in ("coplanar", "duplicated")
        assert plan[64][i]["status"] in (Pc.OK, Pc.NO_MODEL) and Pc.differing(plan[64][i], host[i]) == []


def test_planted_inliers_are_found(runs):
    """sanity against the generator: with a planted share of 0.6 or more the best model holds at least the planted correspondences' half (the threshold is 3
    NORMALISED units, so unrelated points within it count too: at least, not exactly)"""
    cases, plan, _ = runs
    checked = 0
    for c, r in zip(cases, plan[64]):
        if c["kind"] == "random" and c["count"] >= 16 and c["share"] >= 0.6 and c["max_iters"] >= 100:
            assert r["status"] == Pc.OK and 2 * r["max_good"] >= c["n_inliers_planted"], (c["seed"], r["max_good"], c["n_inliers_planted"])
            checked += 1
    assert checked >= 25


def test_stop_rule_is_a_table_lookup(pin):
    """niters = RANSACUpdateNumIters(0.99, (count - good) / count, 5, niters) == min(T[good], niters), T at the 1 000-iteration limit: every count 6..300, then
    300..2048 in steps of 97, good 5..count, niters 1..1000 (both of compute_relative_pose's limits start inside that range)"""
    combos, bad = (int(v) for v in subprocess.run([pin, "scan"], capture_output=True, text=True, check=True).stdout.split())
    print(f"{combos} combinations, {bad} mismatches")
    assert combos == 65870000 and bad == 0


def test_sanitized_build_runs_the_gate_cases_clean(tmp_path):
    """the pin program as a stand-alone executable built with -fsanitize=address,undefined: the header (and pnp_refit behind it), once over the gate cases"""
    exe = Pc.build_pin(tmp_path, sanitize=True)
    r = subprocess.run([exe, "plan", "64"], input=b"".join(Pc.pack(c) for c in Pc.gate_cases()), capture_output=True)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-2000:]


def test_loop_geometry_hook_changes_nothing(scene, tmp_path):
    """compute_loop with LoopGeometry::pnp_ransac fed by the host function, and by the header the GPU runs, returns the Correspondence and the LoopEdge of the run
    without a hook, field for field"""
    exe = str(tmp_path / "pnp_hook_check")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pnp_hook_check.cpp"),
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
    assert [x[1] for x in rows] == ["1", "1", "1", "0"] and sum(int(x[4]) for x in rows) >= 6 and all(int(x[7]) > 100 for x in rows[:3])
