"""Pose graphs for the 4-DoF pose-graph tests (tests/test_pgo_plan_cpu.py, tests/test_gpu_pgo.py) and an INDEPENDENT restatement of csrc/pgo_plan.h's edge
arithmetic: a pose as a 4 x 4 matrix (a rotation about z and a translation), the relative pose as inverse(A) B, yaws read back with numpy's arctan2, angles wrapped
through arctan2(sin, cos), and Huber's loss written from Ceres' definition (rho(s) = s for s <= 1, 2 sqrt(s) - 1 above; a block's residual and Jacobian are scaled
by sqrt(rho'(s)) because rho'' < 0 leaves Corrector's alpha at 0) -- none of the header's expressions.

A graph: every drone flies a planar-ish random walk; ego-motion edges join consecutive poses with noise proportional to the step; loop edges join random pairs with
the true relative pose plus a little noise, some of them replaced by gross outliers.  The initial values are the integrated noisy odometry."""
import numpy as np

from omni_swarm_amd.capi import PGO_EDGE_DTYPE


def mat(p):
    c, s = np.cos(p[3]), np.sin(p[3])
    return np.array([[c, -s, 0, p[0]], [s, c, 0, p[1]], [0, 0, 1, p[2]], [0, 0, 0, 1.0]])


def unmat(M):
    return np.array([M[0, 3], M[1, 3], M[2, 3], np.arctan2(M[1, 0], M[0, 0])])


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def delta_restated(a, b):
    return unmat(np.linalg.solve(mat(a), mat(b)))


def mul_restated(a, b):
    return unmat(mat(a) @ mat(b))


def rho(s):
    return s if s <= 1.0 else 2.0 * np.sqrt(s) - 1.0


def rho_prime(s):
    return 1.0 if s <= 1.0 else 1.0 / np.sqrt(s)


def raw_residual(x, e):
    """sqrt_inf o (z - DeltaPose(x_i, x_j)), yaw wrapped, before any loss"""
    d = e["z"] - delta_restated(x[e["i"]], x[e["j"]])
    d[3] = wrap(d[3])
    return e["sqrt_inf"] * d


def edge_restated(x, e):
    """(corrected residual, cost) of one edge"""
    r = raw_residual(x, e)
    s = float(r @ r)
    if e["robust"]:
        return np.sqrt(rho_prime(s)) * r, 0.5 * rho(s)
    return r, 0.5 * s


def cost_restated(x, edges):
    return sum(edge_restated(x, e)[1] for e in edges)


def mats(p):
    """mat() for poses [k][4] at once"""
    M = np.zeros((len(p), 4, 4))
    c, s = np.cos(p[:, 3]), np.sin(p[:, 3])
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1], M[:, 2, 2], M[:, 3, 3] = c, -s, s, c, 1.0, 1.0
    M[:, :3, 3] = p[:, :3]
    return M


def raw_residuals(x, edges):
    """raw_residual() for all edges at once (batched solves), for the optimiser's many evaluations"""
    D = np.linalg.solve(mats(x[edges["i"]]), mats(x[edges["j"]]))
    d = edges["z"] - np.stack([D[:, 0, 3], D[:, 1, 3], D[:, 2, 3], np.arctan2(D[:, 1, 0], D[:, 0, 0])], axis=1)
    d[:, 3] = wrap(d[:, 3])
    return edges["sqrt_inf"] * d


def scipy_residuals(x, edges):
    """what scipy.optimize.least_squares minimises half the squared norm of: per edge r sqrt(rho(s) / s), so that the sum is the robust cost"""
    r = raw_residuals(x, edges)
    s = np.einsum("ij,ij->i", r, r)
    big = (edges["robust"] != 0) & (s > 1.0)
    k = np.ones(len(edges))
    k[big] = np.sqrt((2.0 * np.sqrt(s[big]) - 1.0) / s[big])
    return (r * k[:, None]).ravel()


def scipy_solve(g, tol=1e-12):
    """scipy.optimize.least_squares on scipy_residuals from g.init over the free poses: (poses, cost, status)"""
    from scipy.optimize import least_squares
    free = g.fixed == 0

    def f(v):
        x = g.init.copy()
        x[free] = v.reshape(-1, 4)
        return scipy_residuals(x, g.edges)

    r = least_squares(f, g.init[free].ravel(), method="trf", xtol=tol, ftol=tol, gtol=tol, max_nfev=200)
    x = g.init.copy()
    x[free] = r.x.reshape(-1, 4)
    return x, float(r.cost), int(r.status)


def make_edge(i, j, z, sqrt_inf, robust):
    e = np.zeros((), PGO_EDGE_DTYPE)
    e["i"], e["j"], e["z"], e["sqrt_inf"], e["robust"] = i, j, z, sqrt_inf, int(robust)
    return e


def walk(rng, length, origin):
    """a drone's true poses: steps of about half a metre, yaw drifting"""
    p = np.zeros((length, 4))
    p[0] = origin
    for k in range(1, length):
        step = np.array([0.3 + 0.4 * rng.random(), 0.1 * rng.normal(), 0.05 * rng.normal(), 0.25 * rng.normal()])
        p[k] = mul_restated(p[k - 1], step)
    return p


class Graph:
    """drones x length poses (pose d * length + k is frame k of drone d), ego-motion edges first, then the loops.
    odo_sigma: noise of an ego-motion edge per sqrt(metre) (position, yaw); 0 gives edges made from the truth.
    loops / outliers: how many loop edges, and how many of them are gross outliers (the LAST ones drawn are NOT the outliers: positions are drawn at random).
    robust: the loop edges carry the loss."""

    def __init__(self, seed, drones=3, length=50, loops=12, outliers=0, odo_sigma=(0.03, 0.01), loop_sigma=(0.02, 0.01), robust=True, start_sigma=(0.0, 0.0), yaw0=None):
        rng = np.random.default_rng(seed)
        self.drones, self.length = drones, length
        n = drones * length
        origins = [np.array([4.0 * d * rng.normal(), 4.0 * d * rng.normal(), 0.3 * d, rng.uniform(-np.pi, np.pi) if yaw0 is None else yaw0]) for d in range(drones)]
        self.truth = np.concatenate([walk(rng, length, o) for o in origins])
        edges, init = [], np.zeros((n, 4))
        for d in range(drones):
            base = d * length
            init[base] = self.truth[base]
            if d:
                init[base] = mul_restated(self.truth[base], np.array([0.3 * rng.normal(), 0.3 * rng.normal(), 0.05 * rng.normal(), 0.05 * rng.normal()]))
            for k in range(1, length):
                z = delta_restated(self.truth[base + k - 1], self.truth[base + k])
                step = max(float(np.linalg.norm(z[:3])), 1e-3)
                sig = np.array([odo_sigma[0]] * 3 + [odo_sigma[1]]) * np.sqrt(step)
                z = z + sig * rng.normal(size=4)
                cov = np.where(sig > 0, sig * sig, np.array([0.01, 0.01, 0.01, 0.003]) * step)
                edges.append(make_edge(base + k - 1, base + k, z, 1.0 / np.sqrt(cov), False))
                init[base + k] = mul_restated(init[base + k - 1], z)
        bad = set(rng.choice(loops, outliers, replace=False).tolist()) if outliers else set()
        lsig = np.array([loop_sigma[0]] * 3 + [loop_sigma[1]])
        for k in range(loops):
            while True:
                i, j = (int(v) for v in rng.integers(0, n, 2))
                if i != j and (i // length != j // length or abs(i - j) > length // 3):
                    break
            z = delta_restated(self.truth[i], self.truth[j]) + lsig * rng.normal(size=4)
            if k in bad:
                z = z + np.array([3.0, -2.5, 0.5, 1.2]) * rng.choice([-1.0, 1.0], 4)
            cov = np.where(lsig > 0, lsig * lsig, 4e-4)
            edges.append(make_edge(i, j, z, 1.0 / np.sqrt(cov), robust))
        self.outlier_edges = sorted(n - drones + k for k in bad)      # indices into self.edges
        self.edges = np.array(edges, PGO_EDGE_DTYPE)
        self.init = init + np.array([start_sigma[0]] * 3 + [start_sigma[1]]) * rng.normal(size=(n, 4))
        self.init[0] = self.truth[0]
        self.fixed = np.zeros(n, np.uint8)
        self.fixed[0] = 1


def chain_with_loop(length, seed=0, extra_edges=0):
    """one drone, `length` poses, length - 1 ego-motion edges + one loop from the last pose to the first (+ extra_edges further loops): length + extra_edges edges"""
    g = Graph(seed, drones=1, length=length, loops=0)
    rng = np.random.default_rng(seed + 1000)
    pairs = [(length - 1, 0)]
    while len(pairs) < 1 + extra_edges:
        i, j = (int(v) for v in rng.integers(0, length, 2))
        if abs(i - j) > 1:
            pairs.append((i, j))
    loops = [make_edge(i, j, delta_restated(g.truth[i], g.truth[j]) + 0.01 * rng.normal(size=4), np.full(4, 50.0), True) for i, j in pairs]
    g.edges = np.concatenate([g.edges, np.array(loops, PGO_EDGE_DTYPE)])
    return g
