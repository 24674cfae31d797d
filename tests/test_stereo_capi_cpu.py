"""CPU-side checks of what the STEREO_PINHOLE camera configuration adds to the two C boundaries (no GPU): include/omni_host_stereo.h is valid C99 and
libomni_host_stereo.so exports exactly what it declares and pipeline.py binds exactly that; libomni_hip.so exports the resize object and the raw-frame entries of
the key-frame unit, which refuse bad arguments with a code and a message; the host layer asks the camera configuration one question at a time (stereo / dirs /
masked), and the resize's coefficients are computed in one place."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")


def test_stereo_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_stereo.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(PKG, "lib", "libomni_host_stereo.so")
    assert os.path.exists(lib), "libomni_host_stereo.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.STEREO_SYMBOLS) == declared == {"omni_stereo_last_error", "omni_pipeline_create_stereo_pinhole", "omni_pipeline_set_stereo_extrinsics"}
    L = pipeline.stereo_lib()
    assert all(hasattr(L, s) for s in declared)
    # argument errors are codes and messages, not aborts
    assert L.omni_pipeline_set_stereo_extrinsics(None, None, None) == 1 and b"null pipeline" in L.omni_stereo_last_error()


def test_resize_and_raw_unit_entries_are_exported_and_refuse_bad_arguments(omni):
    c = omni.capi
    L = c.lib()
    new = {"omni_resize_create", "omni_resize_destroy", "omni_resize_mode", "omni_resize_enqueue_dev", "omni_cam_enqueue_raw_dev", "omni_cam_enqueue_raw_host",
           "omni_cam_enqueue_raw_host_parts"}
    assert new <= set(c.SYMBOLS) and all(hasattr(L, s) for s in new)
    assert L.omni_resize_create(None, 64, 48, 64, 48) is None and b"null context" in L.omni_last_error()
    assert L.omni_resize_mode(None) == -1
    assert L.omni_resize_enqueue_dev(None, None, 0, 0, None) == c.ERR_INVALID
    assert L.omni_cam_enqueue_raw_host(None, None, None, None, 0, 0) == c.ERR_INVALID
    assert L.omni_cam_enqueue_raw_dev(None, None, None, None, 0, 0) == c.ERR_INVALID
    assert L.omni_cam_enqueue_raw_host_parts(None, None, None, None, 0, None, None, 0, 0) == c.ERR_INVALID
    L.omni_resize_destroy(None)
    assert (c.RESIZE_COPY, c.RESIZE_AREA2, c.RESIZE_LINEAR) == (0, 1, 2)


def test_the_camera_configuration_is_asked_one_question_at_a_time():
    """Config::mono() meant one camera, one direction and no mask at once: STEREO_PINHOLE has two cameras, one direction and no mask"""
    src = open(os.path.join(PKG, "host", "keyframe_pipeline.hpp")).read()
    assert "mono()" not in src and "mono()" not in open(os.path.join(PKG, "host", "host_capi.cpp")).read()
    for q in ("bool stereo() const { return camera_configuration != 2; }", "int dirs() const { return camera_configuration == 1 ? 4 : 1; }",
              "bool masked() const { return camera_configuration == 1; }"):
        assert q in src, q
    assert "det_.stereo_fisheye = c.masked();" in src                       # the query direction: 1 for STEREO_FISHEYE only (loop_detector.cpp:252-258)
    assert "cfg_.masked() ? 1 : 0, k)" in src                               # ... and in the sharded step
    # no HIP in the plan's header, and no second place that makes a coefficient
    plan = open(os.path.join(PKG, "csrc", "resize_plan.h")).read()
    assert "hip/" not in plan and "__device__" not in plan and "common.h" not in plan
    for f in ("resize.hip", "cam.hip", "cam_input.h"):
        text = open(os.path.join(PKG, "csrc", f)).read()
        assert "nearbyint" not in text and "rint(" not in text and "floor" not in text, f
    assert "resize_plan(src_width, src_height, dst_width, dst_height)" in open(os.path.join(PKG, "csrc", "resize.hip")).read()


def test_cpp_adapters_compile_from_a_plain_cpp_program(tmp_path):
    """ResizeHIP and LoopCamHIP::enqueue_raw_* (host/omni_swarm.hpp) and the STEREO_PINHOLE configuration of KeyframePipeline are plain C++17 over the C ABI"""
    src = tmp_path / "adapters.cpp"
    src.write_text('#include "keyframe_pipeline.hpp"\n'
                   'int main() {\n'
                   '    omni::KeyframePipeline::Config c;\n'
                   '    c.camera_configuration = 0; c.src_width = 752; c.src_height = 480;\n'
                   '    if (!(c.stereo() && c.dirs() == 1 && !c.masked() && c.raw() && c.in_width() == 752 && c.in_height() == 480)) return 1;\n'
                   '    c.camera_configuration = 1; c.src_width = c.src_height = 0;\n'
                   '    if (!(c.stereo() && c.dirs() == 4 && c.masked() && !c.raw() && c.in_width() == c.width)) return 2;\n'
                   '    c.camera_configuration = 2;\n'
                   '    if (!(!c.stereo() && c.dirs() == 1 && !c.masked() && !c.raw())) return 3;\n'
                   '    c.camera_configuration = 3;\n'
                   '    try { omni::KeyframePipeline::resolved(c); return 4; } catch (const std::runtime_error&) {}\n'
                   '    c.camera_configuration = 2; c.src_width = 640; c.src_height = 480;\n'
                   '    try { omni::KeyframePipeline::resolved(c); return 5; } catch (const std::runtime_error&) {}\n'
                   '    void (omni::LoopCamHIP::*f)(omni_resize*, const uint8_t*, const uint8_t*, int, int) = &omni::LoopCamHIP::enqueue_raw_host;\n'
                   '    return f && sizeof(omni::ResizeHIP) > 0 ? 0 : 6;\n}\n')
    libdir = os.path.join(PKG, "lib")
    exe = tmp_path / "adapters"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", libdir, "-lomni_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
