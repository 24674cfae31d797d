"""The gfx950 build of the depth-landmark stage (omni_depth_landmarks_enqueue_dev: csrc/depth_landmarks.hip running csrc/depth_plan.h one key-point slot per
lane) against the g++ build of the same header (omni_depth_landmarks_host), which tests/test_depth_capi_cpu.py holds to the host functions: flags, counts and the
BITS of every float.  3 images, max_num 300 (the lane loop wraps at 256), the ideal pinhole, PINHOLE with k1 k2 p1 p2 and MEI; the inputs are
tests/depth_cases.py's -- the gate and rounding points, the depth values around the window, a depth image smaller than the gate, a stride above the width,
key-point counts 0 / accept_min / accept_min + 1 / 257 / 300 / above max_num, un-normalised quaternions, one image without a depth frame."""
import ctypes

import numpy as np
import pytest

from tests import depth_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(omni):
    cs = D.gate_cases(omni)
    refs = [omni.capi.depth_landmarks_host(c["model"], c["poses"], c["kps_xy"], c["n_kps"], c["depth"], have=c["have"], camera=c["camera"], depth_stride=c["stride"]) for c in cs]
    return cs, refs


@pytest.mark.parametrize("i", range(5))
def test_kernel_equals_the_cpu_build_bit_for_bit(omni, ctx, cases, i):
    c, ref = cases[0][i], cases[1][i]
    got = omni.capi.depth_landmarks(ctx, c["model"], c["poses"], c["kps_xy"], c["n_kps"], c["depth"], have=c["have"], camera=c["camera"], depth_stride=c["stride"])
    print(f"case {i} ({c['lens']}, {c['n_images']} images x {c['max_num']}): count_3d GPU {got['count_3d'].tolist()} CPU {ref['count_3d'].tolist()}")
    assert D.same_bits(got, ref) == []
    assert i in (0, 3) or got["count_3d"].sum() > 50                          # not vacuous


def test_null_camera_and_null_have(omni, ctx, cases):
    c, ref = cases[0][0], cases[1][0]                                         # the ideal pinhole, every image with a frame
    got = omni.capi.depth_landmarks(ctx, c["model"], c["poses"], c["kps_xy"], c["n_kps"], c["depth"], have=None, camera=None, depth_stride=c["stride"])
    assert D.same_bits(got, ref) == []


def test_refusals(omni, ctx):
    """each before anything is launched: the arguments are small integers that would fault if they were read"""
    c = omni.capi
    L = c.lib()
    case = D.make_case(omni, "ideal", 9, 8, 64, 48, 64, [8, 8, 8], [1, 1, 1])
    m = case["model"]

    def call(model=m, camera=None, n=3, M=8, stride=64, args=(16,) * 8, have=16):
        a = list(args)
        return L.omni_depth_landmarks_enqueue_dev(ctx.h, ctypes.byref(model), ctypes.byref(camera) if camera is not None else None, a[0], n, M, a[1], a[2], a[3], stride, have,
                                                  a[4], a[5], a[6], a[7])

    def model(**kw):
        x = type(m).from_buffer_copy(m)
        for k, v in kw.items():
            setattr(x, k, v)
        return x
    for word, kw in ((b"null", dict(args=(None,) + (16,) * 7)), (b"null", dict(args=(16,) * 7 + (None,))), (b"max_num", dict(M=0)), (b"max_num", dict(M=1025)),
                     (b"focal", dict(model=model(fx=0.0))), (b"focal", dict(model=model(fy=float("nan")))), (b"depth_width", dict(model=model(depth_width=0))),
                     (b"depth_width", dict(model=model(depth_height=-1))), (b"stride", dict(stride=63)), (b"NaN", dict(model=model(depth_near=float("nan")))),
                     (b"NaN", dict(model=model(depth_far=float("nan")))), (b"unknown type", dict(camera=c.CameraModel(type=5))),
                     (b"MEI needs xi", dict(camera=c.CameraModel(type=c.CAMERA_MEI, xi=-1.0))), (b"n_images", dict(n=0))):
        assert call(**kw) == c.ERR_INVALID and word in L.omni_last_error(), (word, kw, L.omni_last_error())
    ctx.sync()                                                                # nothing was launched: the context is as it was
