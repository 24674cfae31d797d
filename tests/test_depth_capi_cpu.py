"""CPU-side checks of what the depth-landmark stage adds to the C boundaries (no GPU): omni_depth_landmarks_host (csrc/depth_plan.h compiled by g++ into
libomni_hip.so) equals the expectations of tests/cpp/depth_plan_pin.cpp's host mode -- fill_image_descriptor + fill_depth_landmarks -- bit for bit; every entry
refuses bad arguments with a code and a message; the new symbols are declared, exported and listed in capi.SYMBOLS; include/omni_host_depth.h is valid C99 and
libomni_host_depth.so exports exactly what it declares; the C++ adapters compile from a plain C++ program; the arithmetic lives in one header.

The switch's round trip on a live pipeline and its refusal for configurations 0 and 1 need a pipeline, and a pipeline needs a GPU: tests/test_gpu_e2e_depth_device.py
holds them.  Here the entry points are called with a null pipeline."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import depth_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
LIBDIR = os.path.join(PKG, "lib")
NEW = {"omni_depth_landmarks_enqueue_dev", "omni_depth_landmarks_host", "omni_cam_set_depth_model", "omni_cam_set_depth_host", "omni_cam_set_depth_dev"}


@pytest.fixture(scope="module")
def expected(omni, tmp_path_factory):
    pin = D.build_pin(tmp_path_factory.mktemp("depth_capi"))
    cases = D.gate_cases(omni)
    return cases, D.run_pin(pin, "host", cases)


def _host(omni, c, **over):
    a = dict(model=c["model"], poses7=c["poses"], kps_xy=c["kps_xy"], n_kps=c["n_kps"], depth=c["depth"], have=c["have"], camera=c["camera"], depth_stride=c["stride"])
    a.update(over)
    return omni.capi.depth_landmarks_host(a.pop("model"), a.pop("poses7"), a.pop("kps_xy"), a.pop("n_kps"), a.pop("depth"), **a)


def test_host_entry_equals_the_host_functions_bit_for_bit(omni, expected):
    cases, want = expected
    for i, (c, w) in enumerate(zip(cases, want)):
        got = _host(omni, c)
        print(f"case {i} ({c['lens']}): count_3d {got['count_3d'].tolist()}")
        assert D.same_bits(got, w) == [], i
    # camera NULL is the ideal pinhole, have NULL is "every image has a frame"
    c, w = cases[0], want[0]
    assert D.same_bits(_host(omni, c, camera=None, have=None), w) == []


def test_every_refusal(omni):
    c = omni.capi
    L = c.lib()
    case = D.make_case(omni, "ideal", 9, 8, 64, 48, 64, [8, 8, 8], [1, 1, 1])

    def refused(word, **over):
        with pytest.raises(c.OmniError) as e:
            _host(omni, case, **over)
        assert word in str(e.value), (word, str(e.value))

    def model(**kw):
        m = type(case["model"]).from_buffer_copy(case["model"])
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    refused("focal", model=model(fx=0.0))
    refused("focal", model=model(fy=float("nan")))
    refused("depth_width", model=model(depth_width=0))
    refused("depth_width", model=model(depth_height=0))
    refused("NaN", model=model(depth_near=float("nan")))
    refused("NaN", model=model(depth_far=float("nan")))
    refused("stride", depth_stride=63)
    refused("unknown type", camera=c.CameraModel(type=7))
    refused("MEI needs xi", camera=c.CameraModel(type=c.CAMERA_MEI, xi=0.0))
    for M in (0, 1025):
        with pytest.raises(c.OmniError) as e:
            c.depth_landmarks_host(case["model"], case["poses"], np.zeros((3, M, 2), np.float32), case["n_kps"], case["depth"])
        assert "max_num" in str(e.value)
    m = case["model"]
    nul = [None] * 4
    assert L.omni_depth_landmarks_host(None, None, None, 3, 8, None, None, None, 64, None, *nul) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_depth_landmarks_host(ctypes.byref(m), None, case["poses"].ctypes.data, 3, 8, None, None, None, 64, None, *nul) == c.ERR_INVALID
    # the device entry and the unit's entries: a code and a message, not an abort (their other refusals need a context: tests/test_gpu_depth_landmarks.py, test_gpu_cam_depth.py)
    assert L.omni_depth_landmarks_enqueue_dev(None, ctypes.byref(m), None, None, 3, 8, None, None, None, 64, None, *nul) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_cam_set_depth_model(None, ctypes.byref(m), None) == c.ERR_INVALID
    assert L.omni_cam_set_depth_host(None, None, 64, 1) == c.ERR_INVALID
    assert L.omni_cam_set_depth_dev(None, None, 64, None, 1) == c.ERR_INVALID


def test_new_entries_are_declared_exported_and_bound(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libomni_hip.so")], capture_output=True, text=True).stdout
    assert NEW <= {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    assert ctypes.sizeof(c.DepthModel) == 6 * 8 + 3 * 4 + 4 + 7 * 8                            # (three ints, padded to the doubles behind them)
    m = c.depth_model(300, 301, 302, 303, 0.3, 10.0, 50, 640, 480, [0, 0, 0.1, 1, 0, 0, 0])
    assert (m.fy, m.depth_far, m.accept_min_3d_pts, m.depth_height, list(m.extrinsic)) == (301, 10.0, 50, 480, [0, 0, 0.1, 1, 0, 0, 0])


def test_depth_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_depth.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_depth.so")
    assert os.path.exists(lib), "libomni_host_depth.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.DEPTH_SYMBOLS) == declared == {"omni_depth_last_error", "omni_pipeline_set_device_depth_landmarks", "omni_pipeline_get_device_depth_landmarks"}
    L = pipeline.depth_lib()
    assert all(hasattr(L, s) for s in declared)
    on = ctypes.c_int(7)
    assert L.omni_pipeline_set_device_depth_landmarks(None, 1) == 1 and b"null pipeline" in L.omni_depth_last_error()      # a code and a message, not an abort
    assert L.omni_pipeline_get_device_depth_landmarks(None, ctypes.byref(on)) == 1 and on.value == 7
    # omni_host.h and its library are untouched by this stage
    assert "depth_landmarks" not in open(os.path.join(ROOT, "include", "omni_host.h")).read()


def test_the_arithmetic_is_stated_once():
    """depth_plan.h is plain C++ for both compilers and restates nothing of landmark_plan.h / camera_plan.h; the kernel, the host entry and the unit only call it"""
    plan = open(os.path.join(PKG, "csrc", "depth_plan.h")).read()
    code = re.sub(r"//.*", "", plan)
    for word in ("hip/", "common.h", "std::vector", "std::function", "<vector>", "<functional>", "sqrt", "pose_from7(const", "quat_R(const", "clamp_count(int"):
        assert word not in code, word
    assert '#include "landmark_plan.h"' in plan and "#pragma clang fp contract(off)" in open(os.path.join(PKG, "csrc", "landmark_plan.h")).read()
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "build/depth_landmarks.o: HIPFLAGS += -ffp-contract=off" in mk and "lib/libomni_host_depth.so" in mk
    for f in ("depth_landmarks.hip", "depth_host.cpp", "cam.hip", "cam_input.h"):
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", f)).read())
        assert not re.search(r"\brint\(", text) and "/ 1000" not in text and "> 640" not in text, f
    kernel = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "depth_landmarks.hip")).read())
    assert "atomic" not in kernel and kernel.count("__shared__") == 1 and "__ballot" in kernel and "__popcll" in kernel


def test_cpp_adapters_compile_from_a_plain_cpp_program(tmp_path):
    """LoopCamHIP::set_depth_model / set_depth_host / set_depth_dev (host/omni_swarm.hpp) and KeyframePipeline::Config::device_depth_landmarks (default off)"""
    src = tmp_path / "adapters.cpp"
    src.write_text('#include "keyframe_pipeline.hpp"\n'
                   'int main() {\n'
                   '    omni::KeyframePipeline::Config c;\n'
                   '    if (c.device_depth_landmarks) return 1;                      // the default stays off\n'
                   '    void (omni::LoopCamHIP::*a)(const omni_depth_model*, const omni_camera_model*) = &omni::LoopCamHIP::set_depth_model;\n'
                   '    void (omni::LoopCamHIP::*b)(const uint16_t* const*, int, int) = &omni::LoopCamHIP::set_depth_host;\n'
                   '    void (omni::LoopCamHIP::*d)(const uint16_t*, int, const uint8_t*, int) = &omni::LoopCamHIP::set_depth_dev;\n'
                   '    void (omni::KeyframePipeline::*s)(bool) = &omni::KeyframePipeline::set_device_depth_landmarks;\n'
                   '    bool (omni::KeyframePipeline::*g)() const = &omni::KeyframePipeline::device_depth_landmarks;\n'
                   '    return a && b && d && s && g ? 0 : 2;\n}\n')
    exe = tmp_path / "adapters"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lomni_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
