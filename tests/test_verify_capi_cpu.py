"""CPU-side checks of what batch_verify adds to the C boundary (no GPU): include/omni_host_verify.h is valid C99, libomni_host_verify.so exports exactly what it
declares and pipeline.VERIFY_SYMBOLS binds exactly that; a null pipeline and a null argument are a code and a message; the Makefile builds the library and tracks
its headers."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")
HOST = {"omni_verify_last_error", "omni_pipeline_set_batch_verify", "omni_pipeline_get_batch_verify", "omni_pipeline_verify_stats", "omni_pipeline_edge_ids", "omni_pipeline_corr_stats", "omni_verify_correspond_host", "omni_verify_plan"}


def declared_in(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))


def exported_by(lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}


def test_verify_library_exports_what_its_c_header_declares():
    hdr = os.path.join(ROOT, "include", "omni_host_verify.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", hdr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = os.path.join(LIBDIR, "libomni_host_verify.so")
    assert os.path.exists(lib), "libomni_host_verify.so missing: run __graft_entry__.build()"
    declared, exported = declared_in(hdr), exported_by(lib)
    assert declared == exported == HOST, (sorted(declared ^ exported), sorted(declared ^ HOST))
    from omni_swarm_amd import pipeline
    assert set(pipeline.VERIFY_SYMBOLS) == declared
    L = pipeline.verify_lib()
    assert all(hasattr(L, s) for s in declared)
    on, out = ctypes.c_int(7), (ctypes.c_int64 * 4)(5, 5, 5, 5)
    assert L.omni_pipeline_set_batch_verify(None, 1) == 1 and b"null pipeline" in L.omni_verify_last_error()
    assert L.omni_pipeline_get_batch_verify(None, ctypes.byref(on)) == 1 and on.value == 7
    assert L.omni_pipeline_verify_stats(None, out) == 1 and list(out) == [5, 5, 5, 5]
    assert L.omni_pipeline_edge_ids(None, None, 0) == -1
    assert L.omni_pipeline_corr_stats(None, None) == 1 and b"null" in L.omni_verify_last_error()
    assert L.omni_verify_correspond_host(None, 0, 1, 0, 0, *([None] * 11)) == 1 and b"null argument" in L.omni_verify_last_error()
    assert L.omni_verify_plan(1, 3, 1, None, None, None, None, None, 0, None, None, None, None, 4) == 1 and b"null" in L.omni_verify_last_error()
    assert L.omni_verify_plan(1, 3, 0, None, None, None, None, None, 0, None, None, None, None, 0) == 0


def test_the_makefile_builds_the_library_and_tracks_the_headers():
    mk = open(os.path.join(ROOT, "omni-swarm_amd", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    hdrs = next(l for l in mk.splitlines() if l.startswith("HOST_HDRS :="))
    assert "lib/libomni_host_verify.so" in all_line and "../include/omni_host_verify.h" in hdrs and "$(wildcard host/*.hpp)" in hdrs
