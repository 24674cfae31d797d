"""CPU-side checks of the lens model's host entries in libomni_hip.so (no GPU, no context): omni_camera_lift_host and omni_camera_project_host equal the g++ build
of csrc/camera_plan.h (tests/cpp/camera_plan_pin.cpp) bit for bit for every camera of tests/camera_cases.py, a NULL camera is the ideal pinhole, and what
cam::check refuses is refused with a code and a message -- here and at omni_landmarks_enqueue_dev_camera / omni_cam_set_camera_model before a handle is touched.
The C++ adapters and the Python frontend's argument exist."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import camera_cases as K
from tests import landmark_cases as L

PKG = os.path.join(L.ROOT, "omni-swarm_amd")
LIBDIR = os.path.join(PKG, "lib")


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return K.build_pin(tmp_path_factory.mktemp("camera_capi"))


def pixels():
    x0, x1, y0, y1 = K.PIXEL_RANGE
    rng = np.random.default_rng(7)
    return np.stack([rng.uniform(x0, x1, 4000), rng.uniform(y0, y1, 4000)], 1).astype(np.float32)


@pytest.mark.parametrize("name", ("ideal", "zero", "mild", "barrel", "euroc", "mei", "diverging"))
def test_lift_and_project_host_equal_the_pin_program(omni, pin, name):
    c = omni.capi
    pts = pixels()
    cam = None if name == "ideal" else K.camera(omni, name)
    got = c.camera_lift_host(cam, K.intrinsics(name), pts)
    ref = K.run_points(pin, "lift", name, pts, omni)
    assert got.dtype == np.float64 and got.shape == ref.shape
    if name == "diverging":                                                   # NaN payloads are not part of the contract: masks, and the bits of what is finite
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got.view(np.uint64)[fin], ref.view(np.uint64)[fin])
        assert (~fin).any()
    else:
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    rng = np.random.default_rng(8)
    X = np.stack([rng.uniform(-2, 2, 500), rng.uniform(-1.5, 1.5, 500), rng.uniform(1, 8, 500)], 1)
    assert np.array_equal(c.camera_project_host(cam, K.intrinsics(name), X).view(np.uint64), K.run_points(pin, "project", name, X, omni).view(np.uint64))
    assert c.camera_lift_host(cam, K.intrinsics(name), np.zeros((0, 2), np.float32)).shape == (0, 2)


def test_refusals_come_back_as_a_code_and_a_message(omni):
    c = omni.capi
    lib = c.lib()
    k = np.array([300.0, 299.5, 300.25, 239.75])
    xy, out = np.zeros((2, 2), np.float32), np.zeros((2, 2))
    for cam, what in ((c.camera_model(2), "unknown type"), (c.camera_model(-1), "unknown type"), (c.camera_model("MEI", xi=0.0), "xi > 0"), (c.camera_model("MEI", xi=-1.0), "xi > 0"),
                      (c.camera_model("MEI", xi=float("nan")), "not finite"), (c.camera_model("PINHOLE", k1=float("inf")), "not finite"), (c.camera_model("PINHOLE", p2=float("nan")), "not finite")):
        for fn in (lib.omni_camera_lift_host, lib.omni_camera_project_host):
            assert fn(ctypes.byref(cam), k.ctypes.data, xy.ctypes.data, 2, out.ctypes.data) == c.ERR_INVALID and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
        with pytest.raises(c.OmniError, match=what):
            c.camera_lift_host(cam, k, xy)
    good = c.camera_model("MEI", xi=1.2)
    assert lib.omni_camera_lift_host(ctypes.byref(good), None, xy.ctypes.data, 2, out.ctypes.data) == c.ERR_INVALID
    assert lib.omni_camera_lift_host(ctypes.byref(good), k.ctypes.data, None, 2, out.ctypes.data) == c.ERR_INVALID
    assert lib.omni_camera_lift_host(ctypes.byref(good), k.ctypes.data, xy.ctypes.data, -1, out.ctypes.data) == c.ERR_INVALID
    bad_k = np.array([0.0, 299.5, 300.25, 239.75])
    assert lib.omni_camera_lift_host(ctypes.byref(good), bad_k.ctypes.data, xy.ctypes.data, 2, out.ctypes.data) == c.ERR_INVALID and b"focal" in lib.omni_last_error()
    # the GPU entries refuse a null handle before anything else
    m = L.model(omni, 1, 3)
    assert lib.omni_landmarks_enqueue_dev_camera(None, ctypes.byref(m), ctypes.byref(good), None, 1, 1, 100, *([None] * 9)) == c.ERR_INVALID and b"null" in lib.omni_last_error()
    assert lib.omni_cam_set_camera_model(None, ctypes.byref(good)) == c.ERR_INVALID
    with pytest.raises(ValueError, match="KANNALA"):
        c.camera_model("KANNALA_BRANDT")


def test_cpp_adapters_and_the_python_argument_exist(tmp_path):
    """LoopCamHIP::set_camera_model, KeyframePipeline::set_camera_model / Config::camera_model and omni::CameraModel are plain C++17 over the C ABI"""
    src = tmp_path / "adapters.cpp"
    src.write_text('#include "keyframe_pipeline.hpp"\n'
                   '#include "omni_host_camera.h"\n'
                   'int main() {\n'
                   '    omni::KeyframePipeline::Config c;\n'
                   '    if (!omni::cam::is_ideal(c.camera_model)) return 1;\n'
                   '    void (omni::LoopCamHIP::*a)(const omni_camera_model*) = &omni::LoopCamHIP::set_camera_model;\n'
                   '    void (omni::KeyframePipeline::*s)(const omni_camera_model&, const double*) = &omni::KeyframePipeline::set_camera_model;\n'
                   '    omni::CameraModel k;\n'
                   '    k.fx = 300; k.fy = 299.5; k.cx = 300.25; k.cy = 239.75;\n'
                   '    const omni::Point2f p{420.f, 130.f};\n'
                   '    const omni::geom::Vec2 ideal = k.lift(p);\n'
                   '    if (ideal.x != ((double)p.x - k.cx) / k.fx || ideal.y != ((double)p.y - k.cy) / k.fy) return 2;\n'
                   '    k.model.k1 = -0.05;\n'
                   '    const omni::geom::Vec2 q = k.lift(p), back = k.project({q.x, q.y, 1.0});\n'
                   '    if (q.x == ideal.x || back.x < 419.999 || back.x > 420.001 || back.y < 129.999 || back.y > 130.001) return 3;\n'
                   '    const omni::CameraModel half = k.scaled(300, 240);\n'
                   '    if (half.fx != k.fx) return 4;                       /* no size stated: nothing to scale from */\n'
                   '    return a && s ? 0 : 5;\n}\n')
    exe = tmp_path / "adapters"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(L.ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lomni_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    from omni_swarm_amd import capi, frontend, pipeline
    assert "camera_model" in inspect.signature(frontend.LoopCam.__init__).parameters
    assert "camera_model" in inspect.signature(pipeline.KeyframePipeline.__init__).parameters
    assert "camera" in inspect.signature(capi.landmarks).parameters and hasattr(capi.Cam, "set_camera_model")
