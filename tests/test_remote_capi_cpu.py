"""CPU-side checks of what remote_in_stream adds to the C boundaries (no GPU): include/omni_host_remote.h is valid C99, libomni_host_remote.so exports exactly
what it declares and pipeline.REMOTE_SYMBOLS binds exactly that; a null pipeline is a code and a message; capi.SYMBOLS still matches what include/omni_hip.h
declares and libomni_hip.so exports, the three new entries among them, at ABI version 2 (additions only)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")
NEW = {"omni_rows_assemble_enqueue_dev", "omni_rows_assemble_host", "omni_memcpy_h2d_async"}
HOST = {"omni_remote_last_error", "omni_pipeline_set_remote_in_stream", "omni_pipeline_get_remote_in_stream", "omni_pipeline_remote_pending",
        "omni_pipeline_remote_stats", "omni_pipeline_queue_copy_as_remote", "omni_remote_merge_plan"}


def declared_in(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))


def exported_by(lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}


def test_remote_library_exports_what_its_c_header_declares():
    hdr = os.path.join(ROOT, "include", "omni_host_remote.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = os.path.join(LIBDIR, "libomni_host_remote.so")
    assert os.path.exists(lib), "libomni_host_remote.so missing: run __graft_entry__.build()"
    declared, exported = declared_in(hdr), exported_by(lib)
    assert declared == exported == HOST, (sorted(declared ^ exported), sorted(declared ^ HOST))
    from omni_swarm_amd import pipeline
    assert set(pipeline.REMOTE_SYMBOLS) == declared
    L = pipeline.remote_lib()
    assert all(hasattr(L, s) for s in declared)
    on, out = ctypes.c_int(7), (ctypes.c_int64 * 4)(5, 5, 5, 5)
    assert L.omni_pipeline_set_remote_in_stream(None, 1) == 1 and b"null pipeline" in L.omni_remote_last_error()
    assert L.omni_pipeline_get_remote_in_stream(None, ctypes.byref(on)) == 1 and on.value == 7
    assert L.omni_pipeline_remote_pending(None) == -1
    assert L.omni_pipeline_remote_stats(None, out) == 1 and list(out) == [5, 5, 5, 5]
    assert L.omni_pipeline_queue_copy_as_remote(None, 1, 2, 3) == 1 and b"null pipeline" in L.omni_remote_last_error()
    n, taken = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert L.omni_remote_merge_plan(0, 4, None, 0, None, None, 2, ctypes.byref(n), ctypes.byref(taken)) == 1 and n.value == 4 and b"do not fit" in L.omni_remote_last_error()
    assert L.omni_remote_merge_plan(0, 4, None, 0, None, None, 8, None, None) == 1 and b"null" in L.omni_remote_last_error()


def test_capi_symbols_still_match_libomni_hip(omni):
    c = omni.capi
    L = c.lib()
    hdr = os.path.join(ROOT, "include", "omni_hip.h")
    inline = set(re.findall(r"static inline \w+ (omni_[a-z0-9_]+)\s*\(", open(hdr).read()))      # helpers defined in the header itself: nothing to export
    declared, exported = declared_in(hdr) - inline, exported_by(os.path.join(LIBDIR, "libomni_hip.so"))
    assert len(c.SYMBOLS) == len(set(c.SYMBOLS)) and set(c.SYMBOLS) == declared, sorted(set(c.SYMBOLS) ^ declared)
    assert declared <= exported, sorted(declared - exported)
    assert NEW <= declared and all(hasattr(L, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in open(hdr).read() and L.omni_abi_version() == 2 == c.ABI_VERSION      # additions only
    text = open(hdr).read()
    assert (c.ROW_UNIT, c.ROW_STAGED, c.ROW_ZERO) == tuple(int(re.search(rf"#define OMNI_ROW_{n} (\d+)", text).group(1)) for n in ("UNIT", "STAGED", "ZERO"))


def test_the_makefile_builds_the_library_and_tracks_the_headers():
    mk = open(os.path.join(ROOT, "omni-swarm_amd", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    hdrs = next(l for l in mk.splitlines() if l.startswith("HOST_HDRS :="))
    assert "lib/libomni_host_remote.so" in all_line and "../include/omni_host_remote.h" in hdrs and "csrc/rows_plan.h" in hdrs
    assert "build/rows_assemble_host.o" in next(l for l in mk.splitlines() if l.startswith("OBJS :="))
