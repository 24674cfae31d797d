"""What the pairwise-consistency stage adds to the C boundaries, without a GPU: include/omni_host_pcm.h is valid C99, libomni_host_pcm.so exports exactly what it
declares and pipeline.PCM_SYMBOLS binds exactly that; a null pipeline and a null argument are a code and a message; the new entries of include/omni_hip.h are
declared, exported, listed in capi.SYMBOLS and refuse null arguments; the Makefile builds the library and compiles pcm.o with contraction off; omni_pcm_rows_host and
omni_pcm_max_clique_host through ctypes on a hand-made graph; LoopOutlierRejection on the host's rows (omni_pcm_filter_host): ids seen twice, both orders of a pair,
`redundant`, the batches, a full handle."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import pcm_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")
NEW = {"omni_pcm_create", "omni_pcm_destroy", "omni_pcm_size", "omni_pcm_capacity", "omni_pcm_add", "omni_pcm_adjacency", "omni_pcm_rows_host", "omni_pcm_max_clique_host",
       "omni_pcm_atan2"}
HOST = {"omni_pcm_host_last_error", "omni_pipeline_set_pcm", "omni_pipeline_get_pcm", "omni_pipeline_good_edges", "omni_pipeline_pcm_stats", "omni_pipeline_pcm_records",
        "omni_pcm_filter_host"}

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "omni_host_pcm.h"
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main(void) {
    int on = 7, red = 7, cap = 7, n = 7;
    double thres = 7;
    int64_t st[6] = {7, 7, 7, 7, 7, 7};
    omni_remote_edge e[1];
    omni_pcm_edge r[1];
    omni_pcm_params pr = {0.6, 0.01, 0.003};
    uint8_t good[1];
    CHECK(sizeof(omni_pcm_edge) == 248 && sizeof(omni_pcm_params) == 24);
    CHECK(OMNI_PCM_FULL == 100 && OMNI_PCM_MAX_ADD == 64 && OMNI_PCM_MIN_CAPACITY == 64 && OMNI_PCM_MAX_CAPACITY == 32768 && OMNI_PCM_DEFAULT_CAPACITY == 4096);
    CHECK(omni_pipeline_set_pcm(NULL, 1, 0.6, 0, 4096) == 1 && strstr(omni_pcm_host_last_error(), "omni_pipeline_set_pcm: null pipeline"));
    CHECK(omni_pipeline_get_pcm(NULL, &on, &thres, &red, &cap) == 1 && on == 7 && thres == 7 && red == 7 && cap == 7 && strstr(omni_pcm_host_last_error(), "omni_pipeline_get_pcm"));
    CHECK(omni_pipeline_good_edges(NULL, e, 1, &n) == 1 && n == 7 && strstr(omni_pcm_host_last_error(), "omni_pipeline_good_edges: null pipeline"));
    CHECK(omni_pipeline_pcm_stats(NULL, st) == 1 && st[0] == 7 && strstr(omni_pcm_host_last_error(), "omni_pipeline_pcm_stats: null pipeline"));
    CHECK(omni_pipeline_pcm_records(NULL, r, 1, &n) == 1 && n == 7 && strstr(omni_pcm_host_last_error(), "omni_pipeline_pcm_records: null pipeline"));
    CHECK(omni_pcm_filter_host(NULL, 1, NULL, 0, 1, 0, 4096, &pr, good, st) == 1 && strstr(omni_pcm_host_last_error(), "omni_pcm_filter_host: null argument"));
    CHECK(omni_pcm_filter_host(r, 0, NULL, 0, 1, 0, 100, &pr, good, st) == 1 && strstr(omni_pcm_host_last_error(), "capacity"));
    CHECK(omni_pcm_filter_host(r, 0, NULL, 0, 1, 0, 64, &pr, good, st) == 0 && st[0] == 0 && st[3] == 0);
    CHECK(omni_pcm_create(NULL, 4096, &pr, NULL) == OMNI_ERR_INVALID && strstr(omni_last_error(), "omni_pcm_create: null argument"));
    CHECK(omni_pcm_add(NULL, r, 1, NULL, NULL, NULL) == OMNI_ERR_INVALID && omni_pcm_adjacency(NULL, 0, 0, NULL, NULL) == OMNI_ERR_INVALID);
    CHECK(omni_pcm_size(NULL) == 0 && omni_pcm_capacity(NULL) == 0);
    omni_pcm_destroy(NULL);
    printf("OK\n");
    return 0;
}
"""


def test_c_program_links_the_library_and_meets_every_null_refusal(tmp_path):
    src, exe = tmp_path / "pcm_capi.c", tmp_path / "pcm_capi"
    src.write_text(PROGRAM)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", LIBDIR,
                        "-lomni_host_pcm", "-lomni_hip", f"-Wl,-rpath,{LIBDIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr[-2000:]


def test_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_pcm.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_pcm.so")
    assert os.path.exists(lib), "libomni_host_pcm.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported == HOST, (sorted(declared ^ exported), sorted(declared ^ HOST))
    from omni_swarm_amd import pipeline
    assert set(pipeline.PCM_SYMBOLS) == declared
    L = pipeline.pcm_lib()
    assert all(hasattr(L, s) for s in declared)
    assert L.omni_pipeline_set_pcm(None, 1, 0.6, 0, 4096) == 1 and b"null pipeline" in L.omni_pcm_host_last_error()
    mk = open(os.path.join(ROOT, "omni-swarm_amd", "Makefile")).read()
    assert "lib/libomni_host_pcm.so: host/host_pcm_capi.cpp $(HOST_HDRS)" in mk and "../include/omni_host_pcm.h" in mk
    assert "build/pcm.o: HIPFLAGS += -ffp-contract=off" in mk and "build/pcm_host.o: csrc/pcm_host.cpp csrc/pcm_plan.h" in mk


def test_new_entries_of_the_kernel_library_are_declared_exported_and_bound(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libomni_hip.so")], capture_output=True, text=True).stdout
    assert NEW <= {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert c.PCM_EDGE_DTYPE.itemsize == 248 and ctypes.sizeof(c.PcmParams) == 24 and (c.PCM_FULL, c.PCM_MAX_ADD, c.PCM_DEFAULT_CAPACITY) == (100, 64, 4096)
    assert L.omni_pcm_rows_host(None, 1, 0, None, 1, None, None, None) == c.ERR_INVALID and b"null" in L.omni_last_error()
    e = np.zeros(2, c.PCM_EDGE_DTYPE)
    rows, deg, pr = np.zeros(1, np.uint64), np.zeros(2, np.int32), c.pcm_params()
    for n_total, first, stride in ((0, 0, 1), (2, 2, 1), (2, -1, 1), (2, 0, 0)):
        assert L.omni_pcm_rows_host(e.ctypes.data, n_total, first, ctypes.byref(pr), stride, rows.ctypes.data, deg.ctypes.data, None) == c.ERR_INVALID
    assert L.omni_pcm_max_clique_host(None, 1, 1, None, None) == c.ERR_INVALID


def test_rows_and_clique_through_ctypes(omni):
    c = omni.capi
    sc = PC.Scene(9, drones=(1, 2))
    e = np.array([sc.edge(1, 2), sc.edge(2, 1), sc.edge(1, 2, displaced=True), sc.edge(1, 2), sc.edge(1, 1), sc.edge(2, 1, displaced=True)], c.PCM_EDGE_DTYPE)
    rows, deg = c.pcm_rows_host(e)
    A = PC.bits_to_dense(rows, 6)
    want = np.zeros((6, 6), bool)
    for i in (0, 1, 3):
        for j in (0, 1, 3):
            want[i, j] = i != j
    assert np.array_equal(A, want) and list(deg) == [2, 2, 0, 2, 0, 0]
    assert sorted(c.pcm_max_clique_host(rows, 6)) == [0, 1, 3] and list(c.pcm_max_clique_host(rows, 6)) == [0, 3, 1]      # the start vertex, then the highest index first
    rows2, deg2 = c.pcm_rows_host(e, first=3, stride_words=2)
    assert rows2.shape == (3, 2) and np.array_equal(PC.bits_to_dense(rows2, 6), want[3:]) and list(deg2) == [1, 1, 0, 2, 0, 0]
    assert c.pcm_atan2(1.0, 1.0) == np.pi / 4


def test_loop_outlier_rejection_on_the_host_rows(omni):
    from omni_swarm_amd import pipeline
    c = omni.capi
    sc = PC.Scene(31)
    e = sc.edges(150, noise=0.0, outliers=0.3)                       # true edges agree exactly: every pair's clique is its undisplaced edges
    good, st = pipeline.pcm_filter_host(e, self_id=1)
    pair = lambda r: (int(r["drone_a"]), int(r["drone_b"]))
    with_self = np.array([1 in pair(r) for r in e])
    assert good[~with_self].all()                                    # pairs without this drone: never evaluated, everything passes
    assert st["edges_entered"] == int(with_self.sum()) and st["clique_runs"] == len({tuple(sorted(pair(r))) for r in e[with_self]}) and st["full_handles"] == 0
    # a displaced edge is consistent with nothing of its pair; an undisplaced one with every other undisplaced one
    A = PC.bits_to_dense(c.pcm_rows_host(e)[0], len(e))
    displaced = A.sum(1) == 0
    groups = {}
    for k, r in enumerate(e):
        groups.setdefault(tuple(sorted(pair(r))), []).append(k)
    for key, ks in groups.items():
        if 1 not in key:
            continue
        inl = [k for k in ks if not displaced[k]]
        if len(inl) >= 2:
            assert good[inl].all() and not good[[k for k in ks if displaced[k]]].any(), key
    # the same edges in batches, and offered twice: the same verdicts, the same pairs
    good_b, st_b = pipeline.pcm_filter_host(np.concatenate([e, e]), self_id=1, batches=[1, 7, 64, 78, 150])
    assert np.array_equal(good_b[:150], good) and np.array_equal(good_b[150:], good)
    assert [st_b[k] for k in ("edges_entered", "pairs_evaluated", "consistent_pairs")] == [st[k] for k in ("edges_entered", "pairs_evaluated", "consistent_pairs")]
    assert st_b["clique_runs"] > st["clique_runs"]
    # redundant: every pair is evaluated, under a >= b
    good_r, st_r = pipeline.pcm_filter_host(e, self_id=1, redundant=True)
    assert st_r["edges_entered"] == len(e) and st_r["clique_runs"] == len(groups) and np.array_equal(good_r[with_self], good[with_self])
    # a full handle: what does not fit stays outside and passes
    good_f, st_f = pipeline.pcm_filter_host(e, self_id=1, capacity=64)
    big = max((ks for key, ks in groups.items() if 1 in key), key=len)
    assert len(big) > 64 and st_f["full_handles"] == sum(max(0, len(ks) - 64) for key, ks in groups.items() if 1 in key) and good_f[big[64:]].all()
