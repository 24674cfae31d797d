"""The raw-fisheye surface without a GPU: include/omni_host_fisheye.h declares what libomni_host_fisheye.so exports and pipeline.FISHEYE_SYMBOLS binds, the unit
entry omni_cam_enqueue_fisheye_jpeg_host is declared, listed and bound, and calls without a handle return the error and leave the message."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "omni_host_fisheye.h")
LIB = os.path.join(ROOT, "omni-swarm_amd", "lib", "libomni_host_fisheye.so")


def test_header_declares_what_the_library_exports_and_python_binds(omni):
    from omni_swarm_amd import pipeline
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HDR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)                            # declarations only
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    assert os.path.exists(LIB), "libomni_host_fisheye.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    assert declared == set(pipeline.FISHEYE_SYMBOLS) and len(pipeline.FISHEYE_SYMBOLS) == 3
    L = pipeline.fisheye_lib()
    assert all(hasattr(L, s) for s in pipeline.FISHEYE_SYMBOLS)
    assert pipeline.FISHEYE_LIB_PATH == LIB


def test_unit_entry_is_declared_listed_and_bound(omni):
    c = omni.capi
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    m = re.search(r"int\s+omni_cam_enqueue_fisheye_jpeg_host\(([^;]*)\);", hdr)
    assert m, "omni_cam_enqueue_fisheye_jpeg_host is not declared in include/omni_hip.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1] for a in args] == ["cam", "up", "down", "up_files", "up_sizes", "down_files", "down_sizes", "n_keyframes", "first_view", "fisheye_mask"]
    assert "omni_cam_enqueue_fisheye_jpeg_host" in c.SYMBOLS
    f = c.lib().omni_cam_enqueue_fisheye_jpeg_host
    assert f.restype is C.c_int and len(f.argtypes) == 10
    assert hasattr(c.Cam, "enqueue_fisheye_jpeg_host")
    from omni_swarm_amd import frontend
    assert hasattr(frontend.LoopCam, "on_fisheye_jpeg")


def test_null_handles_return_the_error_and_the_message(omni):
    from omni_swarm_amd import pipeline
    c = omni.capi
    rc = c.lib().omni_cam_enqueue_fisheye_jpeg_host(None, None, None, None, None, None, None, 1, 1, 1)
    assert rc == c.ERR_INVALID and "null argument" in c.lib().omni_last_error().decode()
    L = pipeline.fisheye_lib()
    w, h = C.c_int(7), C.c_int(7)
    assert L.omni_pipeline_get_fisheye_raw(None, C.byref(w), C.byref(h)) == 1
    assert "null pipeline" in L.omni_fisheye_last_error().decode() and (w.value, h.value) == (7, 7)
    mei = (C.c_double * 9)(1.8, 0, 0, 0, 0, 1100, 1100, 640, 512)
    common = (0, None, None, None, None, 600, 312, 0.015, 200, c.PREC_F16, 2, 2, c.STORE_F32, 1, 0.3, 0.2, 5, 10, 3, 0)
    assert L.omni_pipeline_create_stereo_fisheye_raw(*common, 1280, 1024, 235.0, mei, mei, 1) is None
    assert "null argument" in L.omni_fisheye_last_error().decode()
    common = (0, b"sp", None, None, b"vlad") + common[5:]
    assert L.omni_pipeline_create_stereo_fisheye_raw(*common, 0, 0, 235.0, mei, mei, 1) is None
    assert "src_width x src_height" in L.omni_fisheye_last_error().decode()
    # the Config checks come before any GPU object: side views of another size, half a frame size
    assert L.omni_pipeline_create_stereo_fisheye_raw(*(common[:6] + (320,) + common[7:]), 1280, 1024, 235.0, mei, mei, 1) is None
    assert "600 x 312 but the networks take 600 x 320" in L.omni_fisheye_last_error().decode()
    assert L.omni_pipeline_create_stereo_fisheye_raw(*common, 1280, 1024, 235.0, mei, mei, 0) is None
    assert "fisheye_first_view + 4" in L.omni_fisheye_last_error().decode()
    with pytest.raises(ValueError, match="raw_fisheye belongs to STEREO_FISHEYE"):
        pipeline.KeyframePipeline(0, "sp", "c", "m", "v", raw_fisheye=dict(src_width=1, src_height=1, fov_deg=235.0, mei_up=[0] * 9, mei_down=[0] * 9),
                                  stereo_pinhole=dict(fx=1, fy=1, cx=1, cy=1))
