"""The stereo-landmark kernel with a lens model (csrc/landmarks.hip through omni_landmarks_enqueue_dev_camera; the lens: csrc/camera_plan.h, camodocal's PINHOLE
with distortion and MEI) against the CPU build of the arithmetic it runs (tests/cpp/camera_plan_pin.cpp `plan`, itself held to the host functions' bits and to
a Python restatement of the formulas by tests/test_camera_plan_cpu.py) on the same arrays: lifted floats, 3-D points, flags and count_3d BIT FOR BIT, on the seven
gate shapes of tests/landmark_cases.py seen through the cameras of tests/camera_cases.py.  A camera whose undistortion rounds diverge: flags, counts, the isnan /
isinf masks and the bits of every finite value.  A model whose coefficients are zero, and no model at all, are omni_landmarks_enqueue_dev."""
import ctypes

import numpy as np
import pytest

from tests import camera_cases as K
from tests import landmark_cases as L

pytestmark = pytest.mark.gpu

CAMERAS = ("mild", "euroc", "mei")


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return K.build_pin(tmp_path_factory.mktemp("camera_plan"))


@pytest.fixture(scope="module")
def reference(omni, pin):
    """per camera: the seven cases and the g++ build's outputs, computed once"""
    out = {}
    for name in CAMERAS:
        cases = K.gate_cases(omni, name)
        out[name] = (cases, K.run_pin(pin, "plan", cases))
    return out


def run_gpu(omni, ctx, c, camera="case", camera_entry=False):
    cam = c["camera"] if camera == "case" else camera
    return omni.capi.landmarks(ctx, c["model"], c["poses"], c["kps_xy"], c["n_kps"], c["match_up"], c["match_down"], c["n_matches"], camera=cam, camera_entry=camera_entry)


@pytest.mark.parametrize("i", range(7))
@pytest.mark.parametrize("name", CAMERAS)
def test_kernel_with_a_camera_equals_the_cpu_build_bit_for_bit(omni, ctx, reference, name, i):
    cases, ref = reference[name]
    assert len(cases) == 7
    c, r = cases[i], ref[i]
    got = run_gpu(omni, ctx, c)
    print(f"{name} case {i}: {c['n_pairs']} pairs x {c['max_num']}: count_3d GPU {got['count_3d'].tolist()} CPU {r['count_3d'].tolist()}; 3-D points with other bits: "
          f"{int((got['landmarks_3d'].view(np.uint32) != r['landmarks_3d'].view(np.uint32)).any(-1).sum())} of {int(r['landmarks_flag'].sum())}; flags differing: "
          f"{int((got['landmarks_flag'] != r['landmarks_flag']).sum())}; lifted floats differing: {int((got['norm2d'].view(np.uint32) != r['norm2d'].view(np.uint32)).sum())}; "
          f"tied eigenvalues on the CPU: {int(r['ties'][0])}")
    assert int(r["ties"][0]) == 0 and np.isfinite(r["norm2d"]).all() and not np.isnan(r["landmarks_3d"]).any()      # conditions, on the CPU build
    assert L.same_bits(got, r) == []


def test_a_camera_that_diverges(omni, ctx, pin):
    cases = K.diverging_cases(omni, pin)
    ref = K.run_pin(pin, "plan", cases)
    for i, (c, r) in enumerate(zip(cases, ref)):
        got = run_gpu(omni, ctx, c)
        print(f"diverging case {i}: non-finite lifted floats CPU {int((~np.isfinite(r['norm2d'])).sum())} GPU {int((~np.isfinite(got['norm2d'])).sum())}; "
              f"count_3d GPU {got['count_3d'].tolist()} CPU {r['count_3d'].tolist()}")
        assert int((~np.isfinite(r["norm2d"])).sum()) > 20                       # not vacuous, by the CPU build
        assert K.same_where_finite(got, r) == [], i


def test_zero_coefficients_and_no_camera_are_the_earlier_entry(omni, ctx):
    for i in (3, 6):
        c = L.gate_cases(omni)[i]
        old = omni.capi.landmarks(ctx, c["model"], c["poses"], c["kps_xy"], c["n_kps"], c["match_up"], c["match_down"], c["n_matches"])      # omni_landmarks_enqueue_dev
        assert old["count_3d"].sum() > 0
        null = run_gpu(omni, ctx, c, camera=None, camera_entry=True)                                                                    # _camera with NULL
        zero = run_gpu(omni, ctx, c, camera=K.camera(omni, "zero"))
        assert L.same_bits(null, old) == [] and L.same_bits(zero, old) == []
        # (and a camera does change the result: the lens is in the path)
        assert L.same_bits(run_gpu(omni, ctx, c, camera=K.camera(omni, "mild")), old) != []


def test_refusals(omni, ctx):
    """each returned before anything is launched (the pointers are not device memory)"""
    c = omni.capi
    lib = c.lib()
    model = L.model(omni, 1, 3)
    args = [16] * 9
    for cam, what in ((c.camera_model(2, 0.1), "unknown type"), (c.camera_model("MEI", xi=0.0), "xi > 0"), (c.camera_model("MEI", xi=-0.5), "xi > 0"),
                      (c.camera_model("PINHOLE", k2=float("nan")), "not finite"), (c.camera_model("MEI", p1=float("inf"), xi=1.0), "not finite")):
        rc = lib.omni_landmarks_enqueue_dev_camera(ctx.h, ctypes.byref(model), ctypes.byref(cam), 16, 5, 1, 100, *args)
        assert rc == c.ERR_INVALID and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
    good = c.camera_model("MEI", xi=1.2)
    for pairs, dirs, max_num, what in ((0, 1, 100, "0 pairs"), (5, 2, 100, "the model has 1"), (5, 1, 2000, "max_num")):      # the earlier entry's refusals hold here too
        rc = lib.omni_landmarks_enqueue_dev_camera(ctx.h, ctypes.byref(model), ctypes.byref(good), 16, pairs, dirs, max_num, *args)
        assert rc == c.ERR_INVALID and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
    assert lib.omni_landmarks_enqueue_dev_camera(ctx.h, ctypes.byref(model), ctypes.byref(good), None, 5, 1, 100, *args) == c.ERR_INVALID
