"""CPU-side checks of what the loop-verification RANSAC adds to the C boundaries (no GPU): include/omni_host_homography.h is valid C99, libomni_host_homography.so
exports exactly what it declares and pipeline.py binds exactly that, a C program built with gcc alone links against it; libomni_hip.so exports the two new entries
of include/omni_hip.h, capi.py binds them, and they refuse bad arguments with a code and a message; the C++ adapters compile from a plain C++ program; the
arithmetic lives in one header."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
LIBDIR = os.path.join(PKG, "lib")
NEW = {"omni_homography_ransac_multi", "omni_bf_match_homography_multi"}
HOST = {"omni_homography_last_error", "omni_pipeline_set_device_homography", "omni_pipeline_get_device_homography"}


def test_homography_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_homography.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_homography.so")
    assert os.path.exists(lib), "libomni_host_homography.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.HOMOGRAPHY_SYMBOLS) == declared == HOST
    L = pipeline.homography_lib()
    assert all(hasattr(L, s) for s in declared)
    assert L.omni_pipeline_set_device_homography(None, 1) == 1 and b"null pipeline" in L.omni_homography_last_error()      # a code and a message, not an abort
    assert L.omni_pipeline_get_device_homography(None, None, None, None) == 1 and b"null pipeline" in L.omni_homography_last_error()


def test_a_c_program_links_and_calls_the_library(tmp_path):
    src = tmp_path / "hg.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "omni_host_homography.h"\n'
                   'int main(void) {\n'
                   '    int on = 7;\n'
                   '    if (strlen(omni_homography_last_error()) != 0) return 1;              /* no failure yet on this thread */\n'
                   '    if (omni_pipeline_set_device_homography(NULL, 1) != 1) return 2;\n'
                   '    if (omni_pipeline_get_device_homography(NULL, &on, NULL, NULL) != 1 || on != 7) return 3;\n'
                   '    printf("%s\\n", omni_homography_last_error());\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "hg"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", LIBDIR,
                        "-lomni_host_homography", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "null pipeline" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_new_entries_of_the_hip_library_are_declared_exported_bound_and_refuse_bad_arguments(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    for name, value in (("UNFILTERED", 0), ("OK", 1), ("NO_MODEL", 2), ("HOST", 3)):
        assert getattr(c, "HG_" + name) == value == int(re.search(rf"#define OMNI_HG_{name} (\d+)", hdr).group(1))
    assert L.omni_homography_ransac_multi(None, 1, 8, None, None, None, None, None, None, None) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_bf_match_homography_multi(None, 1, None, None, None, None, 64, 0, 8, *([None] * 14)) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert callable(c.homography_ransac_multi) and callable(c.bf_match_homography_multi)


def test_the_arithmetic_is_stated_once():
    """ransac_plan.h is plain C++ for both compilers (no HIP header, no containers), carries both budgets, and the kernel file only calls it"""
    plan = open(os.path.join(PKG, "csrc", "ransac_plan.h")).read()
    code = re.sub(r"//.*", "", plan)
    for word in ("hip/", "common.h", "std::vector", "std::function", "std::sort", "<vector>", "<functional>", "<algorithm>"):
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in plan
    assert re.search(r"kAttemptBudget = 256;", code) and re.search(r"kDrawBudget = 262144;", code)
    assert "build/homography.o: HIPFLAGS += -ffp-contract=off" in open(os.path.join(PKG, "Makefile")).read()
    text = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "homography.hip")).read())
    for word in ("sqrt", "fabs", "4164903690", "pow(", "log("):
        assert word not in text, word
    assert '"ransac_plan.h"' in text


def test_cpp_adapters_compile_from_a_plain_cpp_program(tmp_path):
    """BFMatcherL2X::match_homography_multi, LoopGeometry::homography_mask and KeyframePipeline::Config::device_homography are plain C++17 over the C ABI; the hook
    replaces the host call only when it returns true with a mask of the right length"""
    src = tmp_path / "adapters.cpp"
    src.write_text('#include "keyframe_pipeline.hpp"\n'
                   'int main() {\n'
                   '    omni::KeyframePipeline::Config c;\n'
                   '    const bool dflt = c.device_homography;\n'
                   '    c.device_homography = !dflt;\n'
                   '    void (omni::BFMatcherL2X::*m)(const std::vector<omni::BFMatcherL2X::PairH>&, int, std::vector<std::vector<omni::DMatch>>&, std::vector<omni::BFMatcherL2X::Homography>&) =\n'
                   '        &omni::BFMatcherL2X::match_homography_multi;\n'
                   '    void (omni::KeyframePipeline::*s)(bool) = &omni::KeyframePipeline::set_device_homography;\n'
                   '    int (omni::KeyframePipeline::*n)() const = &omni::KeyframePipeline::homography_pairs_host;\n'
                   '    omni::BFMatcherL2X::Homography h;\n'
                   '    if (h.status != OMNI_HG_UNFILTERED || h.info[2] != -1) return 2;\n'
                   '    omni::LoopGeometry g;\n'
                   '    if (g.homography_mask) return 3;\n'
                   '    return m && s && n ? 0 : 4;\n}\n')
    exe = tmp_path / "adapters"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lomni_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
