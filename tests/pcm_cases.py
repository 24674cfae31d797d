"""Loop edges for the pairwise-consistency tests (tests/test_pcm_plan_cpu.py, tests/test_gpu_pcm.py) and an INDEPENDENT restatement of csrc/pcm_plan.h's pair
arithmetic: poses as 4 x 4 matrices for the translation, Hamilton products for the rotation, numpy's arctan2 for the angle -- none of the header's expressions.

A scene: every drone k flies a random path P_k(t) in its own odometry frame, which sits at G_k in the world.  The true relative pose of an edge between frame ta of
drone a and frame tb of drone b is inverse(G_a P_a(ta)) * G_b P_b(tb); for two such edges of the same drone pair the header's error pose is the identity."""
import numpy as np

from omni_swarm_amd.capi import PCM_EDGE_DTYPE


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def qrot(q, v):
    """q v q* through the cross-product form"""
    w, u = q[0], np.asarray(q[1:])
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def pmul(a, b):
    q = qmul(a[3:], b[3:])
    return np.concatenate([a[:3] + qrot(a[3:], b[:3]), q / np.linalg.norm(q)])


def pinv(a):
    qi = a[3:] * np.array([1.0, -1, -1, -1])
    return np.concatenate([-qrot(qi, a[:3]), qi])


def rand_quat(rng, scale=None):
    if scale is None:
        q = rng.normal(size=4)
    else:
        q = np.concatenate([[1.0], rng.normal(size=3) * scale])
    return q / np.linalg.norm(q)


class Scene:
    def __init__(self, seed, drones=(1, 2, 3), steps=120):
        self.rng = rng = np.random.default_rng(seed)
        self.drones, self.steps = tuple(drones), steps
        self.G, self.P, self.arc = {}, {}, {}
        for d in self.drones:
            self.G[d] = np.concatenate([rng.normal(size=3) * 4, rand_quat(rng)])
            pos, P = rng.normal(size=3), []
            att = rand_quat(rng)
            for _ in range(steps):
                pos = pos + rng.normal(size=3) * 0.4
                att = qmul(att, rand_quat(rng, 0.08))
                att = att / np.linalg.norm(att)
                P.append(np.concatenate([pos, att]))
            self.P[d] = np.array(P)
            self.arc[d] = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(self.P[d][:, :3], axis=0), axis=1))])
        self.next_id = 1000

    def world(self, d, t):
        return pmul(self.G[d], self.P[d][t])

    def edge(self, a, b, noise=0.0, displaced=False, cov=(0.05, 0.05), ta=None, tb=None):
        rng = self.rng
        ta = int(rng.integers(self.steps)) if ta is None else ta
        tb = int(rng.integers(self.steps)) if tb is None else tb
        rel = pmul(pinv(self.world(a, ta)), self.world(b, tb))
        if noise:
            rel = pmul(rel, np.concatenate([rng.normal(size=3) * noise, rand_quat(rng, noise * 0.5)]))
        if displaced:
            rel = pmul(rel, np.concatenate([rng.normal(size=3) * 3, rand_quat(rng)]))
        e = np.zeros((), PCM_EDGE_DTYPE)
        e["id"], e["drone_a"], e["drone_b"] = self.next_id, a, b
        self.next_id += 1
        e["relative_pose"], e["self_pose_a"], e["self_pose_b"] = rel, self.P[a][ta], self.P[b][tb]
        e["arc_a"], e["arc_b"] = self.arc[a][ta], self.arc[b][tb]
        e["pos_cov"], e["ang_cov"] = cov[0], cov[1]
        return e

    def edges(self, n, pair=(1, 2), noise=0.05, outliers=0.25, others=0.1, selfs=0.1):
        """n edges in arrival order: mostly between pair[0] and pair[1] in either order (orientations 1 and 2), some of one drone with itself and some with the third
        drone (orientation 0 against the pair's); `outliers` of them displaced; the noise puts pairs of inliers on both sides of the default threshold"""
        rng, out = self.rng, []
        third = [d for d in self.drones if d not in pair][0]
        for _ in range(n):
            r = rng.random()
            if r < others:
                a, b = (pair[0], third) if rng.random() < 0.5 else (third, pair[1])
            elif r < others + selfs:
                a = b = pair[int(rng.integers(2))]
            else:
                a, b = pair if rng.random() < 0.5 else pair[::-1]
            out.append(self.edge(a, b, noise=noise, displaced=rng.random() < outliers))
        return np.array(out, PCM_EDGE_DTYPE)


def same_robot_pair(e1, e2):
    if e1["drone_a"] == e2["drone_a"] and e1["drone_b"] == e2["drone_b"]:
        return 1
    if e1["drone_a"] == e2["drone_b"] and e1["drone_b"] == e2["drone_a"]:
        return 2
    return 0


def mat(p):
    w, x, y, z = p[3:]
    M = np.eye(4)
    M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    M[:3, 3] = p[:3]
    return M


def smd_restated(e1, e2, pos_per_m=0.01, yaw_per_m=0.003):
    """(orientation, smd) of the NEW edge e1 against the earlier edge e2"""
    o = same_robot_pair(e1, e2)
    if o == 0:
        return 0, 0.0
    sw = o == 2
    p1, p2 = np.array(e1["relative_pose"]), np.array(e2["relative_pose"])
    a2, b2 = (e2["self_pose_b"], e2["self_pose_a"]) if sw else (e2["self_pose_a"], e2["self_pose_b"])
    arc_a2, arc_b2 = (e2["arc_b"], e2["arc_a"]) if sw else (e2["arc_a"], e2["arc_b"])
    inv = np.linalg.inv
    M2 = inv(mat(p2)) if sw else mat(p2)
    oa, ob = inv(mat(e1["self_pose_a"])) @ mat(a2), inv(mat(e1["self_pose_b"])) @ mat(b2)
    t = (oa @ M2 @ inv(ob) @ inv(mat(p1)))[:3, 3]
    conj = np.array([1.0, -1, -1, -1])
    q2 = p2[3:] * conj if sw else p2[3:]
    qa, qb = qmul(e1["self_pose_a"][3:] * conj, a2[3:]), qmul(e1["self_pose_b"][3:] * conj, b2[3:])
    q = qmul(qmul(qmul(qa, q2), qb * conj), p1[3:] * conj)
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    vn = np.linalg.norm(q[1:])
    k = 2 * np.arctan2(vn, q[0]) / vn if vn > 1e-12 else 2.0
    v = np.concatenate([t, k * q[1:]])
    la, lb = abs(arc_a2 - e1["arc_a"]), abs(arc_b2 - e1["arc_b"])
    per = np.array([pos_per_m] * 3 + [yaw_per_m] * 3)
    c = np.concatenate([e1["pos_cov"] + e2["pos_cov"], e1["ang_cov"] + e2["ang_cov"]]) + (la + lb) * per
    with np.errstate(divide="ignore", invalid="ignore"):
        return o, float(np.sum(v * v / c))


def bits_to_dense(rows, n):
    """bitset rows [m][words] u64 -> bool [m][n]"""
    r = np.ascontiguousarray(rows, np.uint64)
    b = np.unpackbits(r.view(np.uint8).reshape(r.shape[0], -1), axis=1, bitorder="little")
    return b[:, :n].astype(bool)


def dense_to_bits(A, words=None):
    A = np.asarray(A, bool)
    n = A.shape[1]
    words = words or max(1, (n + 63) // 64)
    pad = np.zeros((A.shape[0], words * 64), np.uint8)
    pad[:, :n] = A
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(A.shape[0], words)


def clique_restated(A):
    """the clique rule of csrc/pcm_plan.h on adjacency LISTS: -> the vertices, the start vertex first"""
    n = len(A)
    nbr = [[u for u in range(n) if A[v][u]] for v in range(n)]
    deg = [len(x) for x in nbr]
    best = []
    for v in range(n):
        if deg[v] < len(best):
            continue
        S = [u for u in nbr[v] if deg[u] >= len(best)]
        cur = [v]
        while S:
            u = max(S)
            cur.append(u)
            S = [x for x in S if x in nbr[u] and deg[x] >= len(best)]
        if len(cur) > len(best):
            best = cur
    return best
