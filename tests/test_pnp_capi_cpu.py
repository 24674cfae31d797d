"""CPU-side checks of what the PnP RANSAC adds to the C boundaries (no GPU): include/omni_host_pnp.h is valid C99, libomni_host_pnp.so exports exactly what it
declares and pipeline.py binds exactly that, a C program built with gcc alone links against it; libomni_hip.so exports the new entry of include/omni_hip.h,
capi.py binds it, and it refuses bad arguments with a code and a message; the C++ adapters compile from a plain C++ program; the arithmetic lives in one header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
LIBDIR = os.path.join(PKG, "lib")
HOST = {"omni_pnp_last_error", "omni_pipeline_set_device_pnp", "omni_pipeline_get_device_pnp", "omni_pipeline_recv_copy_as_remote"}


def test_pnp_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_pnp.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_pnp.so")
    assert os.path.exists(lib), "libomni_host_pnp.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.PNP_SYMBOLS) == declared == HOST
    L = pipeline.pnp_lib()
    assert all(hasattr(L, s) for s in declared)
    assert L.omni_pipeline_set_device_pnp(None, 1) == 1 and b"null pipeline" in L.omni_pnp_last_error()      # a code and a message, not an abort
    assert L.omni_pipeline_get_device_pnp(None, None, None, None) == 1 and b"null pipeline" in L.omni_pnp_last_error()
    assert L.omni_pipeline_recv_copy_as_remote(None, 0, 2, 1, None, None) == 1 and b"null pipeline" in L.omni_pnp_last_error()


def test_a_c_program_links_and_calls_the_library(tmp_path):
    src = tmp_path / "pnp.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "omni_host_pnp.h"\n'
                   'int main(void) {\n'
                   '    int on = 7;\n'
                   '    if (strlen(omni_pnp_last_error()) != 0) return 1;              /* no failure yet on this thread */\n'
                   '    if (omni_pipeline_set_device_pnp(NULL, 1) != 1) return 2;\n'
                   '    if (omni_pipeline_get_device_pnp(NULL, &on, NULL, NULL) != 1 || on != 7) return 3;\n'
                   '    printf("%s\\n", omni_pnp_last_error());\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "pnp"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", LIBDIR,
                        "-lomni_host_pnp", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "null pipeline" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_new_entry_of_the_hip_library_is_declared_exported_bound_and_refuses_bad_arguments(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert "omni_pnp_ransac_multi" in set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and "omni_pnp_ransac_multi" in c.SYMBOLS and hasattr(L, "omni_pnp_ransac_multi")
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    for name, value in (("SKIPPED", 0), ("OK", 1), ("NO_MODEL", 2), ("HOST", 3)):
        assert getattr(c, "PNP_" + name) == value == int(re.search(rf"#define OMNI_PNP_{name} (\d+)", hdr).group(1))
    plan = open(os.path.join(PKG, "csrc", "pnp_plan.h")).read()
    assert c.PNP_MAX_POINTS == int(re.search(r"kMaxN = (\d+);", plan).group(1)) and c.PNP_MAX_ITERS == int(re.search(r"kMaxIters = (\d+);", plan).group(1))
    assert L.omni_pnp_ransac_multi(None, 1, 8, None, None, None, None, None, None, None, None) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert callable(c.pnp_ransac_multi)


def test_the_arithmetic_is_stated_once():
    """pnp_plan.h is plain C++ for both compilers (no HIP header, no containers, no std::sort / fmax / fmin), carries the draw budget, and the kernel file only
    calls it"""
    plan = open(os.path.join(PKG, "csrc", "pnp_plan.h")).read()
    code = re.sub(r"//.*", "", plan)
    for word in ("hip/", "common.h", "std::vector", "std::function", "std::sort", "<vector>", "<functional>", "<algorithm>", "fmax", "fmin", "cbrt", "cos(", "sin("):
        assert word not in code, word
    assert re.search(r"kSubsetDrawBudget = 256;", code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(PKG, "csrc", "ransac_plan.h")).read() and '"ransac_plan.h"' in code
    assert "build/pnp.o: HIPFLAGS += -ffp-contract=off" in open(os.path.join(PKG, "Makefile")).read()
    text = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "pnp.hip")).read())
    for word in ("sqrt", "fabs", "4164903690", "pow(", "log("):
        assert word not in text, word
    assert '"pnp_plan.h"' in text


def test_cpp_adapters_compile_from_a_plain_cpp_program(tmp_path):
    """PnPRansacX::run_multi, LoopGeometry::pnp_ransac and KeyframePipeline::Config::device_pnp are plain C++17 over the C ABI; the switch is off by default;
    solve_pnp_ransac is the composition of its two halves"""
    src = tmp_path / "adapters.cpp"
    src.write_text('#include "keyframe_pipeline.hpp"\n'
                   'int main() {\n'
                   '    omni::KeyframePipeline::Config c;\n'
                   '    if (c.device_pnp) return 1;\n'
                   '    void (omni::PnPRansacX::*m)(const std::vector<omni::PnPRansacX::Candidate>&, std::vector<omni::PnPRansacX::Result>&) = &omni::PnPRansacX::run_multi;\n'
                   '    void (omni::KeyframePipeline::*s)(bool) = &omni::KeyframePipeline::set_device_pnp;\n'
                   '    int (omni::KeyframePipeline::*n)() const = &omni::KeyframePipeline::pnp_candidates_host;\n'
                   '    omni::PnPRansacX::Result r;\n'
                   '    if (r.status != OMNI_PNP_SKIPPED || r.info[2] != -1) return 2;\n'
                   '    omni::LoopGeometry g;\n'
                   '    if (g.pnp_ransac) return 3;\n'
                   '    std::vector<omni::geom::Vec3> X; std::vector<omni::geom::Vec2> u; std::vector<uint8_t> mask; std::vector<int> inl; omni::geom::Rt best, pose;\n'
                   '    if (omni::geom::pnp_ransac(X, u, 100, 3.0, 0.99, mask, best) || omni::geom::pnp_refit(X, u, mask, best, pose, inl)) return 5;\n'
                   '    return m && s && n ? 0 : 4;\n}\n')
    exe = tmp_path / "adapters"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lomni_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
