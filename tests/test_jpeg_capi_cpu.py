"""CPU-side checks of what send_img adds to the C boundaries (no GPU): include/omni_host_jpeg.h is valid C99, libomni_host_jpeg.so exports exactly what it
declares and pipeline.py binds exactly that; libomni_hip.so exports the new entries of include/omni_hip.h, which refuse bad arguments with a code and a message;
the arithmetic lives in one header that both compilers take."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
LIBDIR = os.path.join(PKG, "lib")
NEW = {"omni_jpeg_create", "omni_jpeg_destroy", "omni_jpeg_enqueue_dev", "omni_jpeg_header", "omni_jpeg_encode_host", "omni_cam_set_jpeg", "omni_cam_jpeg"}


def test_jpeg_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_jpeg.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_jpeg.so")
    assert os.path.exists(lib), "libomni_host_jpeg.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.JPEG_SYMBOLS) == declared == {"omni_jpeg_host_last_error", "omni_pipeline_set_send_img", "omni_pipeline_get_send_img", "omni_pipeline_jpeg_truncated",
                                                      "omni_pipeline_frame_image"}
    L = pipeline.jpeg_lib()
    assert all(hasattr(L, s) for s in declared)
    assert L.omni_pipeline_set_send_img(None, 1, 75) == 1 and b"null pipeline" in L.omni_jpeg_host_last_error()      # a code and a message, not an abort


def test_new_entries_of_the_hip_library_are_declared_exported_bound_and_refuse_bad_arguments(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "omni_hip.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert c.JPEG_HEADER_BYTES == int(re.search(r"#define OMNI_JPEG_HEADER_BYTES (\d+)", hdr).group(1)) == len(c.jpeg_header(600, 480, 75))
    assert (c.JPEG_OK, c.JPEG_TRUNCATED) == tuple(int(re.search(rf"#define OMNI_JPEG_{n} (\d+)", hdr).group(1)) for n in ("OK", "TRUNCATED"))
    assert ctypes.sizeof(c._CamJpeg) == 8 + 8 + 3 * 8
    assert not L.omni_jpeg_create(None, 8, 8, 1, 75, 4096) and b"null" in L.omni_last_error()
    assert L.omni_jpeg_enqueue_dev(None, None, 8, 1, 8, None, None, None) == c.ERR_INVALID
    assert L.omni_cam_set_jpeg(None, 75, 4096) == c.ERR_INVALID and L.omni_cam_jpeg(None, None) == c.ERR_INVALID
    L.omni_jpeg_destroy(None)


def test_the_arithmetic_is_stated_once():
    """jpeg_plan.h is plain C++ for both compilers (no HIP header, no containers); the kernels, the library's host entry and the pin program only call it"""
    plan = open(os.path.join(PKG, "csrc", "jpeg_plan.h")).read()
    code = re.sub(r"//.*", "", plan)
    for word in ("hip/", "common.h", "std::vector", "<vector>", "<algorithm>", "float", "double"):
        assert word not in code, word
    for f in ("jpeg.hip", "cam.hip", "cam_input.h", "jpeg_host.cpp"):
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", f)).read())
        for word in ("4433", "15137", "0x7d", "5000 /"):                     # the DCT's constants, the Huffman table, the quality rule
            assert word not in text, (f, word)
    assert "9633" in code and "0x7d" in code and "5000 / q" in code
