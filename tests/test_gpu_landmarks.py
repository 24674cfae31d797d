"""The stereo-landmark kernel alone (csrc/landmarks.hip through omni_landmarks_enqueue_dev) against the CPU build of the arithmetic it runs
(csrc/landmark_plan.h in tests/cpp/landmark_plan_pin.cpp, itself held to the host geometry's bits by tests/test_landmarks_cpu.py) on the same arrays:
EVERY output bit-identical -- lifted floats, 3-D points, flags, count_3d.  That is the design: the same f64 operations in the same order, IEEE add / mul /
div / sqrt, contraction off.  Shapes: tests/landmark_cases.py gate_cases (1, 5 and 8 pairs; max_num 7, 100, 200; images with 0, accept_min, accept_min + 1,
max_num key points; 0, 1, 63, 64, 65, n_kps matches; 1 and 4 directions per key frame with poses per key frame; accept_min_3d_pts 3 and 50)."""
import numpy as np
import pytest

from tests import landmark_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(omni, tmp_path_factory):
    cases = L.gate_cases(omni)
    return cases, L.run_pin(L.build_pin(tmp_path_factory.mktemp("landmark_plan")), "plan", cases)


def run_gpu(omni, ctx, c):
    return omni.capi.landmarks(ctx, c["model"], c["poses"], c["kps_xy"], c["n_kps"], c["match_up"], c["match_down"], c["n_matches"])


@pytest.mark.parametrize("i", range(7))
def test_kernel_equals_the_cpu_build_bit_for_bit(omni, ctx, reference, i):
    cases, ref = reference
    assert len(cases) == 7
    c, r = cases[i], ref[i]
    got = run_gpu(omni, ctx, c)
    a, b = got["landmarks_3d"].view(np.uint32), r["landmarks_3d"].view(np.uint32)
    moved = (a != b).any(-1)
    worst = float(np.abs(got["landmarks_3d"].astype(np.float64) - r["landmarks_3d"].astype(np.float64))[moved].max()) if moved.any() else 0.0
    print(f"case {i}: {c['n_pairs']} pairs x {c['max_num']}: count_3d GPU {got['count_3d'].tolist()} CPU {r['count_3d'].tolist()}; 3-D points with other bits: "
          f"{int(moved.sum())} of {int(r['landmarks_flag'].sum())} (largest difference {worst:.3g}); flags differing: {int((got['landmarks_flag'] != r['landmarks_flag']).sum())}; "
          f"lifted floats differing: {int((got['norm2d'].view(np.uint32) != r['norm2d'].view(np.uint32)).sum())}; tied eigenvalues on the CPU: {int(r['ties'][0])}")
    assert int(r["ties"][0]) == 0
    assert L.same_bits(got, r) == []


def test_refusals(omni, ctx, reference):
    """each before anything is launched: a model whose directions do not divide the pairs, a direction count other than the model's, sizes out of range"""
    c = omni.capi
    case = reference[0][6]                                                    # 8 pairs of 4 directions
    m4, m1 = case["model"], L.model(omni, 1, 3)
    lib = c.lib()
    args = [16] * 9                                                           # (refused before a pointer is used)
    for model, pairs, dirs, max_num, what in ((m4, 6, 4, 100, "6 pairs of 4"), (m4, 8, 1, 100, "the model has 4"), (m1, 0, 1, 100, "0 pairs"), (m1, 5, 1, 2000, "max_num")):
        import ctypes
        rc = lib.omni_landmarks_enqueue_dev(ctx.h, ctypes.byref(model), 16, pairs, dirs, max_num, *args)
        assert rc == c.ERR_INVALID and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
    bad = L.model(omni, 1, 3)
    bad.fx = 0.0
    with pytest.raises(c.OmniError, match="focal"):
        run_gpu(omni, ctx, dict(reference[0][0], model=bad))
