"""The consistency rows on the GPU (csrc/pcm.hip through omni_pcm_*) against the g++ build of the same header (omni_pcm_rows_host; tests/test_pcm_plan_cpu.py holds
that against its restatements): no tolerance -- every adjacency word of the handle's bit matrix, both triangles, every degree, and what omni_pcm_add hands back.

One scene of 321 edges (tests/pcm_cases.py: orientations 0 / 1 / 2 mixed, noisy inliers on both sides of the threshold, displaced outliers, and two edges of the same
frames with ZERO covariance, whose pair divides by zero) and ONE host reference for it: a pair's verdict does not depend on what else the graph holds, so the graph of
the first m edges is the reference's top-left m x m block.  Handles holding 0, 1, 63, 64, 65 and 257 edges (filled in calls of at most 64) take calls of 1, 2, 8 and 64
new edges; a handle of capacity 64 is filled to the brim; the refusals."""
import numpy as np
import pytest

from tests import pcm_cases as PC

pytestmark = pytest.mark.gpu
CAP = 384
ZERO_AT = (3, 70)


@pytest.fixture(scope="module")
def graph(omni):
    c = omni.capi
    sc = PC.Scene(21)
    e = sc.edges(257 + 64)
    for k in ZERO_AT:                      # the same two frames, true relative pose, no covariance at all: smd = 0 / 0 or x / 0
        z = sc.edge(1, 2, ta=5, tb=9, cov=(0.0, 0.0))
        z["id"] = e[k]["id"]
        e[k] = z
    rows, deg, smd = c.pcm_rows_host(e, stride_words=CAP // 64, with_smd=True)
    A = PC.bits_to_dense(rows, len(e))
    s = smd[ZERO_AT[1], ZERO_AT[0]]
    assert (np.isnan(s) or np.isinf(s)) and not A[ZERO_AT[1], ZERO_AT[0]]
    fin = smd[np.isfinite(smd) & (smd > 0)]
    assert (fin < 0.6).sum() > 500 and (fin >= 0.6).sum() > 500
    return e, A


def expect(A, m, words):
    """the handle's matrix after the first m edges: rows [m][words] and degrees"""
    B = np.zeros((m, words * 64), bool)
    B[:, :m] = A[:m, :m]
    return PC.dense_to_bits(B, words), A[:m, :m].sum(1).astype(np.int32)


@pytest.mark.parametrize("held", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_new", [1, 2, 8, 64])
def test_rows_and_degrees_equal_the_host_build(omni, ctx, graph, held, n_new):
    c = omni.capi
    e, A = graph
    words = CAP // 64
    p = c.Pcm(ctx, CAP)
    try:
        at = 0
        while at < held:
            step = min(64, held - at)
            deg, rows = p.add(e[at:at + step])
            at += step
            er, ed = expect(A, at, words)
            assert np.array_equal(deg, ed) and np.array_equal(rows, er[at - step:])
        assert p.size == held
        deg, rows = p.add(e[held:held + n_new], time_kernel=True)
        m = held + n_new
        er, ed = expect(A, m, words)
        assert p.size == m and np.array_equal(deg, ed) and np.array_equal(rows, er[held:])
        all_rows, all_deg = p.adjacency(0, CAP)
        assert np.array_equal(all_rows[:m], er) and not all_rows[m:].any() and np.array_equal(all_deg, ed)
        assert np.array_equal(PC.bits_to_dense(all_rows[:m], m), PC.bits_to_dense(all_rows[:m], m).T)
        assert p.last_kernel_us > 0
    finally:
        p.close()


def test_a_full_handle_changes_nothing(omni, ctx, graph):
    c = omni.capi
    e, A = graph
    p = c.Pcm(ctx, 64)
    try:
        assert p.add(e[:60]) is not None
        before = p.adjacency(0, 64)
        assert p.add(e[60:68]) is None and p.size == 60
        after = p.adjacency(0, 64)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        deg, rows = p.add(e[60:64])
        er, ed = expect(A, 64, 1)
        assert p.size == 64 and np.array_equal(deg, ed) and np.array_equal(rows, er[60:]) and np.array_equal(p.adjacency(0, 64)[0], er)
        assert p.add(e[64:65]) is None and p.size == 64 and np.array_equal(p.adjacency(0, 64)[0], er)
    finally:
        p.close()


def test_refusals(omni, ctx, graph):
    c = omni.capi
    e, _ = graph
    for cap in (0, 32, 100, 65536, -64):
        with pytest.raises(c.OmniError):
            c.Pcm(ctx, cap)
    p = c.Pcm(ctx, 128)
    try:
        for n in (0, 65):
            with pytest.raises(c.OmniError):
                p.add(e[:n])
        assert p.size == 0
        with pytest.raises(c.OmniError):
            p.adjacency(100, 64)
        assert c.lib().omni_pcm_add(p.h, None, 1, None, None, None) == c.ERR_INVALID
    finally:
        p.close()
