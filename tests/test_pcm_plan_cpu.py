"""CPU gate of the pairwise consistency of loop edges (csrc/pcm_plan.h, through omni_pcm_rows_host / omni_pcm_max_clique_host / omni_pcm_atan2 of libomni_hip.so and
through tests/cpp/pcm_plan_pin.cpp; no GPU): what the kernels of csrc/pcm.hip must equal bit for bit (tests/test_gpu_pcm.py).

Parity with the reference (swarm_localization's OutlierRejectionLoopEdgesPCM) is unpinned -- swarm_msgs is not vendored -- so the header is the specification and
these tests hold it against independent restatements:
  pin program     the header alone under g++, once plain and once under -fsanitize=address,undefined: pair_smd against geom::Pose + std::atan2, symmetry, degrees,
                  chunked calls, zero covariance, the clique, the arctangent's edge values
  restatement     tests/pcm_cases.py (4 x 4 matrices, Hamilton products, numpy's arctan2): verdicts identical; smd to SMD_RTOL = 1e-9 relative.  Measured on this
                  scene: 2.9e-13 at most (the error pose of two noisy edges is a difference of poses of size ~10, so ~1e3 ulp of cancellation is expected; 1e-9 is the
                  pin program's bound too and far below the distance of any smd of the scene from the threshold)
  ground truth    edges made from true poses: smd < 1e-20 (rounding level: |translation error| ~ 1e-14, squared, over a covariance of 0.1) in both orientations and
                  for edges of one drone with itself
  arctangent      against np.arctan2 over a dense sweep of directions at four magnitudes, of ratios in [0, 1] both ways, over random operands of 60 decades, and the
                  edge values.  Largest distance measured: 2 ulp; the gate is ATAN_GATE_ULP = 4 (the next power of two above it)
  clique          against a list-based restatement on 200 random graphs of 1..80 vertices: the same vertices in the same order, always a clique; a planted clique is
                  found on the seeds where the restatement finds it (checked below: it does on every one of them)"""
import os
import subprocess

import numpy as np
import pytest

from tests import pcm_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMD_RTOL = 1e-9
ATAN_GATE_ULP = 4
ATAN_MEASURED_ULP = 2


@pytest.mark.parametrize("flags", [["-O2", "-ffp-contract=off"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_the_header_alone(tmp_path, flags):
    exe = str(tmp_path / "pcm_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pcm_plan_pin.cpp")])
    for seed in ("1", "7"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.fixture(scope="module")
def scene_edges(omni):
    return PC.Scene(11).edges(130)


def test_verdicts_equal_the_restatement_and_smd_is_close(omni, scene_edges):
    c = omni.capi
    e, n = scene_edges, len(scene_edges)
    rows, deg, smd = c.pcm_rows_host(e, with_smd=True)
    A = PC.bits_to_dense(rows, n)
    assert np.array_equal(A, A.T) and not A.diagonal().any() and np.array_equal(A.sum(1), deg)
    worst, seen, below, above = 0.0, [0, 0, 0], 0, 0
    for i in range(n):
        for j in range(i):
            o, s = PC.smd_restated(e[i], e[j])
            seen[o] += 1
            if o == 0:
                assert not A[i, j] and smd[i, j] == 0
                continue
            assert A[i, j] == (s < 0.6), (i, j, s, smd[i, j])
            worst = max(worst, abs(smd[i, j] - s) / max(abs(s), 1e-12))
            below, above = below + (s < 0.6), above + (s >= 0.6)
    print(f"smd: largest relative difference from the restatement {worst:.3e}; orientations {seen}; {below} pairs below the threshold, {above} not")
    assert worst < SMD_RTOL
    assert min(seen) > 200 and below > 200 and above > 200


def test_a_second_call_continues_the_first(omni, scene_edges):
    c = omni.capi
    n = len(scene_edges)
    rows, deg = c.pcm_rows_host(scene_edges, stride_words=4)
    for first in (1, 63, 64, 65, n - 1):
        r1, d1 = c.pcm_rows_host(scene_edges, first=first, stride_words=4)
        _, d0 = c.pcm_rows_host(scene_edges[:first], stride_words=4)
        assert np.array_equal(r1, rows[first:]) and np.array_equal(np.concatenate([d0, np.zeros(n - first, np.int32)]) + d1, deg)


def test_ground_truth_edges_are_consistent_at_rounding_level(omni):
    c = omni.capi
    sc = PC.Scene(5, drones=(4, 9))
    e = np.array([sc.edge(4, 9), sc.edge(9, 4), sc.edge(4, 9), sc.edge(9, 4)] + [sc.edge(4, 4) for _ in range(3)] + [sc.edge(9, 9) for _ in range(3)], c.PCM_EDGE_DTYPE)
    rows, deg, smd = c.pcm_rows_host(e, with_smd=True)
    A = PC.bits_to_dense(rows, len(e))
    groups = [range(0, 4), range(4, 7), range(7, 10)]
    for g in groups:
        for i in g:
            for j in g:
                if j < i:
                    assert A[i, j] and 0 <= smd[i, j] < 1e-20, (i, j, smd[i, j])
    assert A.sum() == 2 * (6 + 3 + 3)                         # ... and no verdict across groups (same_robot_pair 0)
    print("ground truth: largest smd", smd.max())


def ulp_distance(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.signbit(a), np.signbit(b))
    return np.abs(np.abs(a).view(np.int64) - np.abs(b).view(np.int64))


def test_the_arctangent_against_numpy(omni):
    L = omni.capi.lib()
    f = np.vectorize(lambda y, x: L.omni_pcm_atan2(float(y), float(x)), otypes=[np.float64])
    rng = np.random.default_rng(1)
    th = np.linspace(-np.pi, np.pi, 20001)
    worst = 0
    for r in (1.0, 1e-300, 1e300, 3.7):
        y, x = np.sin(th) * r, np.cos(th) * r
        worst = max(worst, int(ulp_distance(f(y, x), np.arctan2(y, x)).max()))
    t = np.linspace(0, 1, 40001)
    worst = max(worst, int(ulp_distance(f(t, np.ones_like(t)), np.arctan2(t, 1.0)).max()), int(ulp_distance(f(np.ones_like(t), t), np.arctan2(1.0, t)).max()))
    y, x = (rng.normal(size=30000) * 10.0 ** rng.integers(-30, 30, 30000) for _ in range(2))
    worst = max(worst, int(ulp_distance(f(y, x), np.arctan2(y, x)).max()))
    # the log map's own operands: (|v|, w) of unit quaternions, small angles included
    vn = np.concatenate([10.0 ** rng.uniform(-16, 0, 20000), rng.random(20000)])
    w = np.sqrt(np.maximum(0.0, 1 - vn * vn))
    worst = max(worst, int(ulp_distance(f(vn, w), np.arctan2(vn, w)).max()))
    print("arctangent: largest distance from np.arctan2", worst, "ulp")
    assert worst <= ATAN_GATE_ULP
    inf, tiny, sub = np.inf, 2.2250738585072014e-308, 5e-324
    edge = [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (inf, inf), (inf, -inf),
            (-inf, inf), (-inf, -inf), (1.0, inf), (1.0, -inf), (-1.0, -inf), (inf, 1.0), (-inf, -1.0), (tiny, tiny), (sub, sub), (sub, 1.0), (1.0, sub), (sub, -1.0), (tiny, 1e308),
            (1e308, 1e308), (1e308, tiny), (1.0, 1.0), (0.25, 1.0), (0.125, 1.0), (0.375, 1.0), (0.625, 1.0), (0.875, 1.0), (1.0, 0.875)]
    for y, x in edge:
        assert ulp_distance(L.omni_pcm_atan2(y, x), np.arctan2(y, x)) <= ATAN_GATE_ULP, (y, x, L.omni_pcm_atan2(y, x), np.arctan2(y, x))
    for y, x in [(0.0, 1.0), (-0.0, 1.0), (0.0, 0.0), (-0.0, 0.0), (sub, 1.0)]:
        assert L.omni_pcm_atan2(y, x) == np.arctan2(y, x)
    assert np.isnan(L.omni_pcm_atan2(np.nan, 1.0)) and np.isnan(L.omni_pcm_atan2(1.0, np.nan))


def random_graph(rng, n, p):
    A = rng.random((n, n)) < p
    A = np.triu(A, 1)
    return A | A.T


def is_clique(A, vs):
    return len(set(vs)) == len(vs) and all(A[a, b] for a in vs for b in vs if a != b)


def test_the_clique_heuristic_against_the_list_restatement(omni):
    c = omni.capi
    rng = np.random.default_rng(2025)
    sizes = []
    for g in range(200):
        n = int(rng.integers(1, 81))
        A = random_graph(rng, n, rng.choice([0.1, 0.3, 0.5, 0.8, 0.95]))
        got = c.pcm_max_clique_host(PC.dense_to_bits(A, words=2), n)
        ref = PC.clique_restated(A)
        assert list(got) == ref and is_clique(A, got) and len(got) >= 1, (g, n, list(got), ref)
        sizes.append(len(got))
    assert max(sizes) > 10 and min(sizes) == 1


PLANTED_SEEDS = list(range(40, 60))


def test_a_planted_clique_is_found(omni):
    c = omni.capi
    for seed in PLANTED_SEEDS:
        rng = np.random.default_rng(seed)
        n, k = int(rng.integers(30, 81)), int(rng.integers(10, 21))
        A = random_graph(rng, n, 0.15)
        members = np.sort(rng.choice(n, k, replace=False))
        A[np.ix_(members, members)] = True
        np.fill_diagonal(A, False)
        ref = PC.clique_restated(A)
        assert sorted(ref) == list(members), ("the restatement misses the planted clique on this seed: choose another", seed)
        got = c.pcm_max_clique_host(PC.dense_to_bits(A), n)
        assert sorted(got) == list(members) and is_clique(A, got)
    assert len(c.pcm_max_clique_host(np.zeros((1, 1), np.uint64), 0)) == 0
