"""The pose-graph solver on the GPU (csrc/pgo.hip through omni_pgo_solve_multi) against the g++ build of the same header (omni_pgo_solve_host;
tests/test_pgo_plan_cpu.py holds that against its restatements and against SciPy): no tolerance -- every pose bit, both costs, both iteration counts, the status of
every start, and `best`.

The shapes are the smallest at which the kernel can go wrong: 2 poses / 1 edge; chains of 63, 64, 65 poses with one loop (a wave's width); 255 / 256 / 257 edges (the
chunk of the fixed-shape sum); 3 drones x 50 poses with 12 loops, 3 of them outliers (the window the pipeline solves); a hub pose with 70 incident edges (a chain
longer than a wave); a component no edge ties to the fixed pose, held by `fixed`; yaws crossing +-pi during the solve; 1, 2 and 64 starts (every start equals its
own single solve, `best` is the cheapest with ties to the lower index); the iteration cap; a zero covariance, whose NONFINITE comes from arithmetic; the refusals;
two calls on one handle."""
import numpy as np
import pytest

from tests import pgo_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pgo(omni, ctx):
    p = omni.capi.Pgo(ctx)
    yield p
    p.close()


def same(got, want):
    (xg, sg, bg), (xw, sw, bw) = got, want
    assert bg == bw
    assert sg.tobytes() == sw.tobytes(), (sg, sw)
    assert xg.tobytes() == xw.tobytes(), np.abs(xg - xw).max()


def both(c, pgo, poses, fixed, edges, params=None):
    want = c.pgo_solve_host(poses, fixed, edges, params)
    got = pgo.solve(poses, fixed, edges, params)
    same(got, want)
    return want


def test_two_poses_one_edge(omni, pgo):
    c = omni.capi
    e = np.array([PC.make_edge(0, 1, [1.0, 0.5, -0.2, 0.3], [10, 10, 10, 20], True)], c.PGO_EDGE_DTYPE)
    x = np.array([[0.3, -0.2, 0.1, 2.9], [2.0, 2.0, 1.0, -2.5]])
    _, st, best = both(c, pgo, x, [1, 0], e)
    assert st[0]["status"] == c.PGO_CONVERGED and best == 0 and st[0]["final_cost"] < 1e-12 < st[0]["initial_cost"]


@pytest.mark.parametrize("length", [63, 64, 65])
def test_a_chain_with_one_loop(omni, pgo, length):
    c = omni.capi
    g = PC.chain_with_loop(length, seed=length)
    _, st, _ = both(c, pgo, g.init, g.fixed, g.edges)
    assert len(g.edges) == length and st[0]["status"] == c.PGO_CONVERGED and st[0]["final_cost"] < st[0]["initial_cost"]


@pytest.mark.parametrize("n_edges", [255, 256, 257])
def test_the_sums_chunk_boundary(omni, pgo, n_edges):
    c = omni.capi
    g = PC.chain_with_loop(100, seed=n_edges, extra_edges=n_edges - 100)
    _, st, _ = both(c, pgo, g.init, g.fixed, g.edges)
    assert len(g.edges) == n_edges and st[0]["status"] == c.PGO_CONVERGED


@pytest.fixture(scope="module")
def window():
    return PC.Graph(2, drones=3, length=50, loops=12, outliers=3)


def test_the_window_with_outliers(omni, pgo, window):
    c = omni.capi
    g = window
    _, st, _ = both(c, pgo, g.init, g.fixed, g.edges)
    assert len(g.truth) == 150 and len(g.outlier_edges) == 3 and st[0]["status"] == c.PGO_CONVERGED and st[0]["iterations"] >= 3 and st[0]["cg_iterations"] > 150


def test_a_hub_with_seventy_edges(omni, pgo):
    c = omni.capi
    g = PC.Graph(5, drones=1, length=90, loops=0)
    rng = np.random.default_rng(5)
    hub = [PC.make_edge(3, 10 + k, PC.delta_restated(g.truth[3], g.truth[10 + k]) + 0.02 * rng.normal(size=4), np.full(4, 30.0), True) for k in range(68)]
    edges = np.concatenate([g.edges, np.array(hub, c.PGO_EDGE_DTYPE)])
    off, _, _, _ = c.pgo_plan_graph_host(g.fixed, edges)
    assert off[4] - off[3] == 70
    _, st, _ = both(c, pgo, g.init, g.fixed, edges)
    assert st[0]["status"] == c.PGO_CONVERGED


def test_an_unreachable_component_is_held_by_fixed(omni, pgo):
    c = omni.capi
    g = PC.Graph(6, drones=3, length=20, loops=6)
    keep = [k for k, e in enumerate(g.edges) if (e["i"] // 20 == 2) == (e["j"] // 20 == 2)]      # no loop reaches drone 2
    edges = g.edges[keep]
    fixed = g.fixed.copy()
    fixed[40:] = 1
    (out, st, _) = both(c, pgo, g.init, fixed, edges)
    assert st[0]["status"] == c.PGO_CONVERGED and np.array_equal(out[0][40:], g.init[40:]) and not np.array_equal(out[0][1:40], g.init[1:40])


def test_yaws_cross_pi_during_the_solve(omni, pgo):
    c = omni.capi
    g = PC.Graph(7, drones=2, length=30, loops=6, yaw0=np.pi - 0.05, start_sigma=(0.1, 0.15))
    out, st, _ = both(c, pgo, g.init, g.fixed, g.edges)
    before, after = g.init[:, 3], out[0][:, 3]
    crossed = (np.abs(before) < np.pi) != (np.abs(after) < np.pi)
    wrapped = np.abs(PC.wrap(before) - PC.wrap(after)) > np.pi
    assert st[0]["status"] == c.PGO_CONVERGED and (crossed | wrapped).any()


@pytest.mark.parametrize("n_starts", [1, 2, 64])
def test_every_start_equals_its_own_solve(omni, pgo, window, n_starts):
    c = omni.capi
    g = window
    rng = np.random.default_rng(n_starts)
    starts = np.stack([g.init + (0.0 if k == 0 else 0.05 * k) * rng.normal(size=g.init.shape) for k in range(n_starts)])
    if n_starts == 64:
        starts[5] = starts[9] = starts[0]            # a three-way tie
    starts[:, 0] = g.truth[0]
    pr = c.pgo_params(max_iterations=6)
    out, st, best = both(c, pgo, starts, g.fixed, g.edges, pr)
    for k in sorted({0, 1 % n_starts, n_starts - 1, 5 % n_starts}):
        o1, s1, _ = c.pgo_solve_host(starts[k], g.fixed, g.edges, pr)
        assert o1[0].tobytes() == out[k].tobytes() and s1[0] == st[k]
    cheapest = min(st["final_cost"])
    assert best == int(np.flatnonzero(st["final_cost"] == cheapest)[0])
    if n_starts == 64:
        assert st[5] == st[0] and st[9] == st[0] and len(set(st["final_cost"].tolist())) > 30


def test_the_cap_is_reached(omni, pgo, window):
    c = omni.capi
    g = window
    _, st, best = both(c, pgo, g.init, g.fixed, g.edges, c.pgo_params(max_iterations=2, function_tolerance=0.0, parameter_tolerance=0.0))
    assert st[0]["status"] == c.PGO_MAX_ITERATIONS and st[0]["iterations"] == 2 and best == 0
    _, st, _ = both(c, pgo, g.init, g.fixed, g.edges, c.pgo_params(max_cg_iterations=5, max_iterations=4))
    assert st[0]["cg_iterations"] <= 5 * 4 * 17


def test_a_zero_covariance_is_nonfinite_by_arithmetic(omni, pgo, window):
    c = omni.capi
    g = window
    e = g.edges.copy()
    e["sqrt_inf"][60] = c.pgo_sqrt_inf([0.0, 0.01, 0.01], 0.003)
    starts = np.stack([g.init, g.init + 0.01])
    out, st, best = both(c, pgo, starts, g.fixed, e)
    assert (st["status"] == c.PGO_NONFINITE).all() and best == -1 and np.array_equal(out, starts)
    # all poses fixed, and no edge at all: EMPTY
    _, st, best = both(c, pgo, g.init, np.ones(150, np.uint8), g.edges)
    assert st[0]["status"] == c.PGO_EMPTY and best == -1
    _, st, best = both(c, pgo, g.init, g.fixed, g.edges[:0])
    assert st[0]["status"] == c.PGO_EMPTY and best == -1


def test_the_refusals(omni, pgo, window):
    c = omni.capi
    g = window
    bad = g.edges.copy()
    bad["j"][3] = 150
    loop = g.edges.copy()
    loop["j"][3] = loop["i"][3]
    for args, word in (((g.init, g.fixed, bad), "outside the graph"), ((g.init, g.fixed, loop), "with itself"),
                       ((np.zeros((65, 150, 4)), g.fixed, g.edges), "n_starts"), ((np.zeros((4097, 4)), np.zeros(4097, np.uint8), g.edges), "n_poses"),
                       ((g.init, g.fixed, np.zeros(16385, c.PGO_EDGE_DTYPE)), "n_edges")):
        with pytest.raises(c.OmniError, match=word):
            pgo.solve(*args)
    for kw, word in ((dict(initial_lambda=0.0), "initial_lambda"), (dict(max_iterations=-1), "negative cap"), (dict(cg_tolerance=float("nan")), "cg_tolerance")):
        with pytest.raises(c.OmniError, match=word):
            pgo.solve(g.init, g.fixed, g.edges, c.pgo_params(**kw))
    L = c.lib()
    assert L.omni_pgo_solve_multi(None, None, None, None, None, 1, 0, 1, None, None, None, None) != 0 and b"null argument" in L.omni_last_error()


def test_two_calls_on_one_handle(omni, ctx, window):
    c = omni.capi
    p = c.Pgo(ctx)
    try:
        small = PC.chain_with_loop(10, seed=1)
        for g in (window, small, window):             # the buffers grow, are reused for a smaller graph, and hold nothing over
            same(p.solve(g.init, g.fixed, g.edges, time_kernel=True), c.pgo_solve_host(g.init, g.fixed, g.edges))
            assert p.last_kernel_us > 0
    finally:
        p.close()
