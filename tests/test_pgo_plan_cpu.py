"""CPU gate of the 4-DoF pose graph (csrc/pgo_plan.h, through omni_pgo_solve_host / omni_pgo_residuals_host / omni_pgo_plan_graph_host / omni_pgo_sincos /
omni_pgo_sum_host of libomni_hip.so and through tests/cpp/pgo_plan_pin.cpp; no GPU): what the kernel of csrc/pgo.hip must equal bit for bit (tests/test_gpu_pgo.py).

Parity with the reference (swarm_localization's loop + ego-motion problem under Ceres) is unpinned -- Ceres, Eigen and swarm_msgs are not vendored -- so the header is
the specification and these tests hold it against independent restatements and against SciPy:
  pin program     the header alone under g++, once plain and once under -fsanitize=address,undefined: the pose algebra against geom::Pose, the sum's shape, the plan,
                  a ground-truth solve, the statuses, the refusals
  sine, cosine    against np.sin / np.cos over [-pi, pi] (200001 points), +-10, +-1e5, 401 neighbours of every multiple of pi/4 up to 2 pi, signed zeros and
                  subnormals.  Largest distance measured: 1 ulp each; the gate is SINCOS_GATE_ULP = 2 (the next power of two above it)
  restatement     tests/pgo_cases.py (4 x 4 matrices, np.arctan2, Ceres' definition of the loss): residuals to RES_ATOL = 1e-9 absolute on residuals of size up to
                  ~1e3 (sqrt_inf up to 100 times pose differences of some metres, each rounded at 1e-16 relative, and the two sides' trigonometry differ in the last
                  bits: 1e-11 is expected, measured 1.7e-13), costs to RES_ATOL x (|r| + 1), what that error of a residual can move them by; the analytic Jacobians against
                  central differences of the restatement
                  (step 1e-6: truncation ~1e-12 x the third derivative, rounding ~1e-16 x |r| / 1e-6 ~ 1e-7 for |r| ~ 1e3; gate JAC_RTOL = 1e-6 of the Jacobian's largest
                  entry, measured 1.0e-9)
  the solver      (a) ground truth: final cost below 1e-20 and poses within 1e-9 (measured over five seeds: 3.0e-25 and 3.8e-13 m / 2.8e-14 rad at most)
                  (b) against scipy.optimize.least_squares without the loss, (c) with outliers and the loss: see SCIPY_* below and DESIGN.md 0.2r
                  (d) the statuses"""
import os
import subprocess

import numpy as np
import pytest

from tests import pgo_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINCOS_GATE_ULP = 2
RES_ATOL = 1e-9
JAC_RTOL = 1e-6
SEEDS = [0, 1, 2, 3, 4]
TIGHT = dict(function_tolerance=1e-10, parameter_tolerance=1e-10, cg_tolerance=1e-8, max_iterations=100)
# (b), measured on the five seeds: |cost - scipy's| / scipy's 1.3e-14 at most, positions 9.8e-8 m, yaws 4.6e-9 rad; each gate is the next power of ten
SCIPY_B_COST_RTOL, SCIPY_B_POS_ATOL, SCIPY_B_YAW_ATOL = 1e-13, 1e-7, 1e-8
# (c), measured on the five seeds: (cost - scipy's) / scipy's 3.9e-11 at most; the gate is the next power of ten
SCIPY_C_COST_MARGIN = 1e-10


@pytest.mark.parametrize("flags", [["-O2", "-ffp-contract=off"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_header_alone(tmp_path, flags):
    exe = str(tmp_path / "pgo_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pgo_plan_pin.cpp")])
    for seed in ("1", "7"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


def ulp_distance(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.signbit(a), np.signbit(b))
    return np.abs(np.abs(a).view(np.int64) - np.abs(b).view(np.int64))


def test_sine_and_cosine_against_numpy(omni):
    c = omni.capi
    rng = np.random.default_rng(0)
    xs = [np.linspace(-np.pi, np.pi, 200001), rng.uniform(-10, 10, 50000), rng.uniform(-1e5, 1e5, 50000)]
    for q in range(-8, 9):
        b = q * np.pi / 4
        xs += [b + np.arange(-200, 201) * np.spacing(max(abs(b), 1e-300)), b + rng.normal(size=300) * 1e-8]
    xs = np.concatenate(xs)
    sc = np.array([c.pgo_sincos(float(x)) for x in xs])
    ds, dc = ulp_distance(sc[:, 0], np.sin(xs)), ulp_distance(sc[:, 1], np.cos(xs))
    print("sincos_plan: largest distance from np.sin", int(ds.max()), "ulp, from np.cos", int(dc.max()), "ulp")
    assert ds.max() <= SINCOS_GATE_ULP and dc.max() <= SINCOS_GATE_ULP
    for x in (0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1e-310):
        s, co = c.pgo_sincos(x)
        assert s == x and np.signbit(s) == np.signbit(x) and co == 1.0
    assert all(np.isnan(v) for x in (np.nan, np.inf, -np.inf) for v in c.pgo_sincos(x))
    # NormalizeAngle as the reference writes it: into [-pi, pi), the identity inside
    for a in np.concatenate([rng.uniform(-20, 20, 2000), [np.pi, -np.pi, 3 * np.pi, 0.0]]):
        n = c.lib().omni_pgo_normalize_angle(float(a))
        assert -np.pi <= n < np.pi + 1e-15 and abs(PC.wrap(n - a)) < 1e-14
        if -np.pi <= a < np.pi:
            assert n == a


def random_edges(c, rng, n, m):
    """poses and edges with yaw differences on both sides of +-pi and robust edges on both sides of s = 1"""
    x = np.concatenate([rng.normal(size=(n, 3)) * 3, rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)
    edges = []
    for k in range(m):
        i, j = rng.choice(n, 2, replace=False)
        z = PC.delta_restated(x[i], x[j])
        kind = k % 4
        if kind == 0:                         # near the truth, heavy weights: s below and above 1
            z = z + rng.normal(size=4) * 10.0 ** rng.uniform(-4, -1)
        elif kind == 1:                       # the yaw residual next to +-pi, on either side
            z[3] = PC.wrap(z[3] + np.pi + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-9, -1))
        elif kind == 2:                       # an unnormalised measurement
            z = z + np.array([0, 0, 0, 2 * np.pi * rng.integers(-2, 3)]) + rng.normal(size=4) * 0.05
        else:
            z = z + rng.normal(size=4)
        edges.append(PC.make_edge(i, j, z, 10.0 ** rng.uniform(-1, 2, 4), k % 3 != 0))
    return x, np.array(edges, c.PGO_EDGE_DTYPE)


def test_residuals_and_costs_equal_the_restatement(omni):
    c = omni.capi
    x, edges = random_edges(c, np.random.default_rng(3), 40, 600)
    x[::5, 3] += 2 * np.pi                    # poses need not be normalised either
    r, _, _, cost = c.pgo_residuals_host(x, edges)
    worst_r = worst_c = 0.0
    sides = [0, 0, 0]
    for k, e in enumerate(edges):
        rr, cc = PC.edge_restated(x, e)
        raw = PC.raw_residual(x, e)
        s = float(raw @ raw)
        sides[0 if not e["robust"] else (1 if s <= 1 else 2)] += 1
        # a cost is |r|^2 / 2 or sqrt(|r|^2) - 1 / 2: an error dr of the residual moves it by at most (|r| + dr) dr
        worst_r, worst_c = max(worst_r, np.abs(r[k] - rr).max()), max(worst_c, abs(cost[k] - cc) / (np.sqrt(s) + 1.0))
    print(f"residuals: largest difference from the restatement {worst_r:.2e}, costs {worst_c:.2e} x (|r| + 1); plain / robust below 1 / robust above 1: {sides}")
    assert worst_r < RES_ATOL and worst_c < RES_ATOL and min(sides) >= 20


def test_the_jacobians_against_central_differences(omni):
    c = omni.capi
    x, edges = random_edges(c, np.random.default_rng(4), 12, 120)
    _, ji, jj, _ = c.pgo_residuals_host(x, edges)
    worst, h = 0.0, 1e-6
    for k, e in enumerate(edges):
        r0 = PC.raw_residual(x, e)
        if abs(abs(r0[3] / e["sqrt_inf"][3]) - np.pi) < 1e-3:
            continue                          # the wrap's jump sits inside the difference quotient's step
        for side, J in (("i", ji[k]), ("j", jj[k])):
            num = np.zeros((4, 4))
            for col in range(4):
                xp, xm = x.copy(), x.copy()
                xp[e[side], col] += h
                xm[e[side], col] -= h
                d = PC.edge_restated(xp, e)[0] - PC.edge_restated(xm, e)[0]
                num[:, col] = d / (2 * h)
            if e["robust"] and float(r0 @ r0) > 1:
                # Ceres scales the Jacobian by sqrt(rho') and does NOT differentiate the scale (alpha = 0): compare with the scaled raw Jacobian
                for col in range(4):
                    xp, xm = x.copy(), x.copy()
                    xp[e[side], col] += h
                    xm[e[side], col] -= h
                    num[:, col] = (PC.raw_residual(xp, e) - PC.raw_residual(xm, e)) / (2 * h) * np.sqrt(PC.rho_prime(float(r0 @ r0)))
            worst = max(worst, np.abs(J - num).max() / max(np.abs(num).max(), 1e-300))
    print(f"Jacobians: largest difference from central differences {worst:.2e} of the largest entry")
    assert worst < JAC_RTOL


def test_plan_graph_against_brute_force(omni):
    c = omni.capi
    rng = np.random.default_rng(5)
    for n, m in ((2, 1), (5, 0), (30, 200), (80, 79)):
        edges = np.zeros(m, c.PGO_EDGE_DTYPE)
        for k in range(m):
            edges["i"][k], edges["j"][k] = rng.choice(n, 2, replace=False)
        if m == 200:
            edges["i"][:70], edges["j"][:70] = 7, 8 + np.arange(70) % 20        # a hub
        fixed = (rng.random(n) < 0.2).astype(np.uint8)
        off, inc, act, na = c.pgo_plan_graph_host(fixed, edges)
        for p in range(n):
            want = sorted([2 * e for e in range(m) if edges["i"][e] == p] + [2 * e + 1 for e in range(m) if edges["j"][e] == p])
            assert list(inc[off[p]:off[p + 1]]) == want
            assert act[p] == (not fixed[p] and len(want) > 0)
        assert off[n] == 2 * m and na == act.sum()


def test_the_fixed_shape_sum(omni):
    c = omni.capi
    rng = np.random.default_rng(6)
    for count in (0, 1, 255, 256, 257, 2048, 2049, 5000):
        v = rng.normal(size=count) * 10.0 ** rng.integers(-6, 6, count)
        want = 0.0
        for base in range(0, count, 256):
            w = np.zeros(256)
            w[:len(v[base:base + 256])] = v[base:base + 256]
            stride = 128
            while stride >= 1:
                w[:stride] = w[:stride] + w[stride:2 * stride]
                stride //= 2
            want = want + w[0]
        assert c.pgo_sum_host(v) == want


def test_a_solves_ground_truth_to_rounding_level(omni):
    c = omni.capi
    worst = [0.0, 0.0, 0.0]
    for seed in SEEDS:
        g = PC.Graph(seed, odo_sigma=(0, 0), loop_sigma=(0, 0), start_sigma=(0.2, 0.05))
        out, st, best = c.pgo_solve_host(g.init, g.fixed, g.edges, c.pgo_params(function_tolerance=0.0, parameter_tolerance=1e-13, cg_tolerance=1e-10, max_iterations=100))
        assert st[0]["status"] == c.PGO_CONVERGED and best == 0 and st[0]["initial_cost"] > 100
        worst = [max(worst[0], st[0]["final_cost"]), max(worst[1], np.abs(out[0][:, :3] - g.truth[:, :3]).max()), max(worst[2], np.abs(PC.wrap(out[0][:, 3] - g.truth[:, 3])).max())]
    print(f"ground truth: largest final cost {worst[0]:.2e}, position error {worst[1]:.2e} m, yaw error {worst[2]:.2e} rad")
    assert worst[0] < 1e-20 and worst[1] < 1e-9 and worst[2] < 1e-9


@pytest.fixture(scope="module")
def scipy_runs():
    """SciPy's solutions of the (b) and (c) graphs, computed once"""
    runs = {}
    for kind, kw in (("b", dict(loops=12, outliers=0, robust=False)), ("c", dict(loops=12, outliers=3, robust=True))):
        for seed in SEEDS:
            g = PC.Graph(seed, **kw)
            runs[kind, seed] = (g, *PC.scipy_solve(g))
    return runs


def test_b_equals_scipy_without_the_loss(omni, scipy_runs):
    c = omni.capi
    worst = [0.0, 0.0, 0.0]
    for seed in SEEDS:
        g, xs, cost_s, status_s = scipy_runs["b", seed]
        assert status_s > 0, ("SciPy did not converge on this seed", seed, status_s)
        assert len(g.truth) == 150 and not g.edges["robust"].any()
        out, st, _ = c.pgo_solve_host(g.init, g.fixed, g.edges, c.pgo_params(**TIGHT))
        assert st[0]["status"] == c.PGO_CONVERGED
        assert abs(PC.cost_restated(out[0], g.edges) - st[0]["final_cost"]) <= 1e-12 * st[0]["final_cost"]
        worst = [max(worst[0], abs(st[0]["final_cost"] - cost_s) / cost_s), max(worst[1], np.abs(out[0][:, :3] - xs[:, :3]).max()), max(worst[2], np.abs(PC.wrap(out[0][:, 3] - xs[:, 3])).max())]
    print(f"(b) against SciPy: cost {worst[0]:.2e} relative, positions {worst[1]:.2e} m, yaws {worst[2]:.2e} rad")
    assert worst[0] <= SCIPY_B_COST_RTOL and worst[1] <= SCIPY_B_POS_ATOL and worst[2] <= SCIPY_B_YAW_ATOL


def test_c_is_no_worse_than_scipy_with_outliers_and_the_loss(omni, scipy_runs):
    c = omni.capi
    worst = -1.0
    for seed in SEEDS:
        g, xs, cost_s, status_s = scipy_runs["c", seed]
        assert status_s > 0, ("SciPy did not converge on this seed", seed, status_s)
        assert len(g.outlier_edges) == 3 and g.edges["robust"][g.outlier_edges].all()
        out, st, _ = c.pgo_solve_host(g.init, g.fixed, g.edges, c.pgo_params(**TIGHT))
        assert st[0]["status"] == c.PGO_CONVERGED
        assert abs(PC.cost_restated(out[0], g.edges) - st[0]["final_cost"]) <= 1e-12 * st[0]["final_cost"]
        worst = max(worst, (st[0]["final_cost"] - cost_s) / cost_s)
        assert st[0]["final_cost"] <= cost_s * (1 + SCIPY_C_COST_MARGIN)
    print(f"(c) against SciPy: (cost - SciPy's) / SciPy's {worst:.2e} at most")


def test_d_the_statuses(omni):
    c = omni.capi
    g = PC.Graph(9, drones=2, length=20, loops=4)
    out, st, best = c.pgo_solve_host(g.init, np.ones(len(g.fixed), np.uint8), g.edges)
    assert st[0]["status"] == c.PGO_EMPTY and best == -1 and np.array_equal(out[0], g.init) and st[0]["final_cost"] == 0 and st[0]["iterations"] == 0
    out, st, best = c.pgo_solve_host(g.init, g.fixed, g.edges[:0])
    assert st[0]["status"] == c.PGO_EMPTY and best == -1 and np.array_equal(out[0], g.init)
    e = g.edges.copy()
    e["sqrt_inf"][7] = c.pgo_sqrt_inf([0.01, 0.0, 0.01], 0.003)
    assert np.isinf(e["sqrt_inf"][7][1])
    out, st, best = c.pgo_solve_host(g.init, g.fixed, e)
    assert st[0]["status"] == c.PGO_NONFINITE and best == -1 and np.array_equal(out[0], g.init) and not np.isfinite(st[0]["final_cost"])
    out, st, best = c.pgo_solve_host(g.init, g.fixed, g.edges, c.pgo_params(max_iterations=2, function_tolerance=0.0, parameter_tolerance=0.0))
    assert st[0]["status"] == c.PGO_MAX_ITERATIONS and st[0]["iterations"] == 2 and best == 0 and st[0]["final_cost"] < st[0]["initial_cost"]
    out, st, best = c.pgo_solve_host(g.init, g.fixed, g.edges, c.pgo_params(max_cg_iterations=3))
    assert st[0]["cg_iterations"] <= 3 * st[0]["iterations"] * 17
    # a free pose without an edge stays; the rest is solved as without it
    x2 = np.concatenate([g.init, [[5.0, 6.0, 7.0, 0.5]]])
    out2, st2, _ = c.pgo_solve_host(x2, np.concatenate([g.fixed, [0]]), g.edges)
    out1, st1, _ = c.pgo_solve_host(g.init, g.fixed, g.edges)
    assert np.array_equal(out2[0][:-1], out1[0]) and np.array_equal(out2[0][-1], x2[-1]) and st2[0] == st1[0]
