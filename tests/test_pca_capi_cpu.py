"""CPU-side checks of what the PCA fit adds to the C boundaries (no GPU): the new symbols of include/omni_hip.h are declared, exported and listed in capi.SYMBOLS, the
ABI version stays 2; include/omni_host_pca.h is valid C99 and libomni_host_pca.so exports exactly what it declares and pipeline.PCA_SYMBOLS binds; every entry
refuses bad arguments with a code and a message; the files omni_pca_write_csv writes are read back by load_csv_floats (the reader behind every SuperPoint handle,
host/omni_swarm.hpp) to the same f32 values and [64 x 256] / [256] shapes; the C++ adapters compile from a plain C++ program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
LIBDIR = os.path.join(PKG, "lib")
NEW = {"omni_pcafit_create", "omni_pcafit_destroy", "omni_pcafit_reset", "omni_pcafit_enqueue_rows_dev", "omni_sp_set_pcafit", "omni_pcafit_stats", "omni_pcafit_moments",
       "omni_pcafit_merge_host", "omni_pca_solve_host", "omni_pcafit_solve", "omni_pca_moments_host", "omni_pca_write_csv"}
HOST = {"omni_pca_host_last_error", "omni_pipeline_set_fit_pca", "omni_pipeline_get_fit_pca", "omni_pipeline_pca_fit_stats", "omni_pipeline_pca_fit_moments",
        "omni_pipeline_pca_fit_solve", "omni_pipeline_pca_fit_write", "omni_pipeline_pca_fit_reset"}


def _exported(lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}


def test_new_entries_are_declared_exported_and_bound(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NEW <= declared and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    assert NEW <= _exported(os.path.join(LIBDIR, "libomni_hip.so"))
    assert {s for s in declared if "pca" in s} == NEW                                          # nothing else of this stage is declared
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2 and c.ABI_VERSION == 2      # additions only
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "omni_hip.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pca_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_pca.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_pca.so")
    assert os.path.exists(lib), "libomni_host_pca.so missing: run __graft_entry__.build()"
    exported = _exported(lib)
    assert declared == exported == HOST, (sorted(declared ^ exported), sorted(declared ^ HOST))
    from omni_swarm_amd import pipeline
    assert set(pipeline.PCA_SYMBOLS) == HOST
    L = pipeline.pca_lib()
    assert all(hasattr(L, s) for s in HOST)
    # a code and a message, not an abort
    on, n = ctypes.c_int(7), ctypes.c_int64(7)
    calls = {"omni_pipeline_set_fit_pca": lambda: L.omni_pipeline_set_fit_pca(None, 1), "omni_pipeline_get_fit_pca": lambda: L.omni_pipeline_get_fit_pca(None, ctypes.byref(on)),
             "omni_pipeline_pca_fit_stats": lambda: L.omni_pipeline_pca_fit_stats(None, ctypes.byref(n), None),
             "omni_pipeline_pca_fit_moments": lambda: L.omni_pipeline_pca_fit_moments(None, None, None, None, None),
             "omni_pipeline_pca_fit_solve": lambda: L.omni_pipeline_pca_fit_solve(None, 64, None, None, None, None, None, None),
             "omni_pipeline_pca_fit_write": lambda: L.omni_pipeline_pca_fit_write(None, b"a", b"b", 64), "omni_pipeline_pca_fit_reset": lambda: L.omni_pipeline_pca_fit_reset(None)}
    assert set(calls) == HOST - {"omni_pca_host_last_error"}
    for name, call in calls.items():
        assert call() == 1 and name.encode() + b": null pipeline" in L.omni_pca_host_last_error(), (name, L.omni_pca_host_last_error())
    assert on.value == 7 and n.value == 7
    # omni_host.h and its library are untouched by this stage
    assert "pca_fit" not in open(os.path.join(ROOT, "include", "omni_host.h")).read() and "fit_pca" not in open(os.path.join(ROOT, "include", "omni_host.h")).read()
    assert not (_exported(os.path.join(LIBDIR, "libomni_host.so")) & HOST)


def test_bad_arguments_return_a_code_and_a_message(omni, tmp_path):
    c = omni.capi
    L = c.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    s, S = np.zeros(256), np.eye(256)
    n, sk = ctypes.c_int64(0), ctypes.c_int64(0)
    raw, part, kps = np.zeros((1, 8, 256), np.float32), np.ones((1, 8, 256), np.float32), np.array([8], np.int32)

    def moments(raw_p, batch, max_num):
        return L.omni_pca_moments_host(raw_p, part.ctypes.data, kps.ctypes.data, batch, max_num, ctypes.byref(n), ctypes.byref(sk), s.ctypes.data_as(dp), S.ctypes.data_as(dp))
    assert moments(None, 1, 8) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert moments(raw.ctypes.data, 0, 8) == c.ERR_INVALID and b"batch" in L.omni_last_error()
    assert moments(raw.ctypes.data, 1, 0) == c.ERR_INVALID and b"max_num" in L.omni_last_error()
    assert moments(raw.ctypes.data, 1, 1025) == c.ERR_INVALID and b"max_num" in L.omni_last_error()
    n.value = -1
    assert moments(raw.ctypes.data, 1, 8) == c.ERR_INVALID and b"negative" in L.omni_last_error()
    assert L.omni_pca_solve_host(300, None, None, 64, *[None] * 6) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_pcafit_merge_host(None, None, None, 0, None, None) == c.ERR_INVALID and b"null" in L.omni_last_error()
    # the device entries without a handle (their other refusals need a context: tests/test_gpu_pcafit.py, tests/test_gpu_sp_pcafit.py)
    assert L.omni_pcafit_create(None) is None and b"null" in L.omni_last_error()
    L.omni_pcafit_destroy(None)
    assert L.omni_pcafit_reset(None) == c.ERR_INVALID and L.omni_pcafit_enqueue_rows_dev(None, None, None, None, 1, 8) == c.ERR_INVALID
    assert L.omni_pcafit_stats(None, None, None) == c.ERR_INVALID and L.omni_pcafit_moments(None, None, None) == c.ERR_INVALID
    assert L.omni_pcafit_solve(None, 64, *[None] * 6) == c.ERR_INVALID and L.omni_sp_set_pcafit(None, None) == c.ERR_INVALID and b"null" in L.omni_last_error()
    comp, mean = np.zeros((64, 256), np.float32), np.zeros(256, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    assert L.omni_pca_write_csv(None, b"m", comp.ctypes.data_as(fp), mean.ctypes.data_as(fp), 64) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_pca_write_csv(b"c", b"m", comp.ctypes.data_as(fp), mean.ctypes.data_as(fp), 0) == c.ERR_INVALID and b"pca_dim" in L.omni_last_error()
    missing = os.fsencode(str(tmp_path / "no" / "such" / "dir" / "c.csv"))
    assert L.omni_pca_write_csv(missing, b"m", comp.ctypes.data_as(fp), mean.ctypes.data_as(fp), 64) == c.ERR_INVALID and b"cannot write" in L.omni_last_error()
    with pytest.raises(ValueError):
        c.PcaMoments().add_rows(raw, part[:, :4], kps)


READER = r'''
#include <cstdio>
#include <cstring>
#include "omni_swarm.hpp"
int main(int argc, char** argv) {
    int rows = 0, cols = 0, r1 = 0, c1 = 0;
    const std::vector<float> comp = omni::load_csv_floats(argv[1], &rows, &cols), mean = omni::load_csv_floats(argv[2], &r1, &c1);
    std::printf("%d %d %d %d\n", rows, cols, r1, c1);
    std::FILE* f = std::fopen(argv[3], "wb");
    std::fwrite(comp.data(), 4, comp.size(), f); std::fwrite(mean.data(), 4, mean.size(), f);
    std::fclose(f);
    // the adapters of this stage exist with these signatures
    void (Swarm::SuperPointHIP::*a)(omni::PcaFitX*) = &Swarm::SuperPointHIP::set_pcafit;
    omni::PcaMoments (omni::PcaFitX::*b)() = &omni::PcaFitX::moments;
    omni::PcaSolution (*s)(const omni::PcaMoments&, int) = &omni::pca_solve;
    return a && b && s ? 0 : 2;
}
'''


def test_csv_round_trip_through_the_handles_own_reader(omni, tmp_path):
    c = omni.capi
    rng = np.random.default_rng(3)
    comp = (rng.normal(size=(64, 256)) * 10.0 ** rng.integers(-12, 3, size=(64, 256))).astype(np.float32)
    mean = rng.normal(size=256).astype(np.float32)
    comp[0, :4] = [0.0, -0.0, np.float32(1.17549435e-38), np.float32(3.4028235e38)]          # zeros, the smallest normal, the largest finite
    mean[:3] = [np.float32(1e-45), np.float32(-1e-39), np.float32(-1) / np.float32(3)]         # denormals: written as 0 (std::stof refuses them)
    cp, mp, out = str(tmp_path / "components_.csv"), str(tmp_path / "mean_.csv"), str(tmp_path / "read.bin")
    c.pca_write_csv(cp, mp, comp, mean)
    mean[:2] = 0.0
    comp[0, 1] = 0.0                                                                            # (and -0 as 0)
    lines = open(cp).read().splitlines()
    assert len(lines) == 64 and all(l.count(",") == 255 for l in lines) and len(open(mp).read().splitlines()) == 256
    assert np.array_equal(np.loadtxt(cp, delimiter=",", dtype=np.float64).astype(np.float32), comp)         # ... and np.loadtxt reads them as the notebook's files
    src, exe = tmp_path / "reader.cpp", tmp_path / "reader"
    src.write_text(READER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lomni_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), cp, mp, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["64", "256", "256", "1"], (r.returncode, r.stdout, r.stderr)
    back = np.fromfile(out, np.float32)
    assert back[:64 * 256].tobytes() == comp.tobytes() and back[64 * 256:].tobytes() == mean.tobytes()


def test_pipeline_config_switch_defaults_off_and_follows_the_launch_parameter(tmp_path):
    """KeyframePipeline::Config::fit_pca (default off) and SwarmLoopParams::to_pipeline_config's output_raw_superpoint_desc -> fit_pca"""
    src = tmp_path / "config.cpp"
    src.write_text('#include "keyframe_pipeline.hpp"\n#include "swarm_loop_params.hpp"\n'
                   'int main() {\n'
                   '    omni::KeyframePipeline::Config c;\n'
                   '    if (c.fit_pca) return 1;\n'
                   '    omni::SwarmLoopParams p;\n'
                   '    p.to_pipeline_config(c);\n'
                   '    if (c.fit_pca) return 2;\n'
                   '    p.output_raw_superpoint_desc = true;\n'
                   '    p.to_pipeline_config(c);\n'
                   '    if (!c.fit_pca) return 3;\n'
                   '    void (omni::KeyframePipeline::*s)(bool) = &omni::KeyframePipeline::set_fit_pca;\n'
                   '    omni::PcaMoments (omni::KeyframePipeline::*m)() = &omni::KeyframePipeline::pca_fit_moments;\n'
                   '    void (omni::KeyframePipeline::*w)(const std::string&, const std::string&, int) = &omni::KeyframePipeline::pca_fit_write;\n'
                   '    return s && m && w ? 0 : 4;\n}\n')
    exe = tmp_path / "config"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe),
                        "-L", LIBDIR, "-lomni_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
