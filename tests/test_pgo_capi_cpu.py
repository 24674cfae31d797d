"""What the pose graph adds to the C boundary of libomni_hip.so, without a GPU: the new entries of include/omni_hip.h are valid C99, exported and listed in
capi.SYMBOLS; the structs have the sizes capi.py's records and ctypes mirror assume; the defaults; every refusal of the _host entries is a code and a message; the
Makefile compiles pgo.o and pgo_host.o with contraction off."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pgo_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")
NEW = {"omni_pgo_default_params", "omni_pgo_create", "omni_pgo_destroy", "omni_pgo_solve_multi", "omni_pgo_solve_host", "omni_pgo_residuals_host",
       "omni_pgo_plan_graph_host", "omni_pgo_sincos", "omni_pgo_normalize_angle", "omni_pgo_sum_host"}

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include "omni_hip.h"
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main(void) {
    omni_pgo_params pr;
    omni_pgo_edge e[2];
    omni_pgo_stats st[1];
    double x[8] = {0, 0, 0, 0, 1, 0, 0, 0}, out[8];
    uint8_t fixed[2] = {1, 0};
    int best = 7;
    CHECK(sizeof(omni_pgo_edge) == 80 && sizeof(omni_pgo_params) == 48 && sizeof(omni_pgo_stats) == 32);
    CHECK(offsetof(omni_pgo_edge, z) == 8 && offsetof(omni_pgo_edge, sqrt_inf) == 40 && offsetof(omni_pgo_edge, robust) == 72 && offsetof(omni_pgo_params, initial_lambda) == 16);
    CHECK(offsetof(omni_pgo_stats, iterations) == 16 && offsetof(omni_pgo_stats, status) == 24);
    CHECK(OMNI_PGO_CONVERGED == 0 && OMNI_PGO_MAX_ITERATIONS == 1 && OMNI_PGO_NONFINITE == 2 && OMNI_PGO_EMPTY == 3);
    CHECK(OMNI_PGO_MAX_POSES == 4096 && OMNI_PGO_MAX_EDGES == 16384 && OMNI_PGO_MAX_STARTS == 64);
    CHECK(omni_pgo_default_params(NULL) == OMNI_ERR_INVALID && omni_pgo_default_params(&pr) == OMNI_OK);
    CHECK(pr.max_iterations == 50 && pr.max_cg_iterations == 0 && pr.max_lambda_retries == 16 && pr.initial_lambda == 1e-4 && pr.function_tolerance == 1e-6);
    CHECK(pr.parameter_tolerance == 1e-8 && pr.cg_tolerance == 1e-6);
    memset(e, 0, sizeof e);
    e[0].i = 0; e[0].j = 1; e[0].sqrt_inf[0] = e[0].sqrt_inf[1] = e[0].sqrt_inf[2] = e[0].sqrt_inf[3] = 1;
    CHECK(omni_pgo_solve_host(NULL, x, fixed, e, 2, 1, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "omni_pgo_solve_host: null argument"));
    CHECK(omni_pgo_solve_host(&pr, NULL, fixed, e, 2, 1, 1, out, st, &best) == OMNI_ERR_INVALID && omni_pgo_solve_host(&pr, x, NULL, e, 2, 1, 1, out, st, &best) == OMNI_ERR_INVALID);
    CHECK(omni_pgo_solve_host(&pr, x, fixed, NULL, 2, 1, 1, out, st, &best) == OMNI_ERR_INVALID && omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 1, NULL, st, &best) == OMNI_ERR_INVALID);
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 1, out, NULL, &best) == OMNI_ERR_INVALID && omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 1, out, st, NULL) == OMNI_ERR_INVALID);
    CHECK(best == 7);
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 0, 1, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_poses outside 1..4096"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 4097, 0, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_poses"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, -1, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_edges outside 0..16384"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 16385, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_edges"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 0, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_starts outside 1..64"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 65, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_starts"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 1, 1, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "outside the graph"));
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 2, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "with itself"));
    pr.max_lambda_retries = -1;
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "negative cap"));
    omni_pgo_default_params(&pr); pr.parameter_tolerance = -1;
    CHECK(omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 1, out, st, &best) == OMNI_ERR_INVALID && strstr(omni_last_error(), "parameter_tolerance"));
    omni_pgo_default_params(&pr);
    CHECK(best == 7 && omni_pgo_solve_host(&pr, x, fixed, e, 2, 1, 1, out, st, &best) == OMNI_OK && best == 0 && st[0].status == OMNI_PGO_CONVERGED);
    CHECK(out[4] < 1e-6 && out[4] > -1e-6 && out[0] == 0 && st[0].initial_cost == 0.5 && st[0].final_cost < 1e-12);
    CHECK(omni_pgo_residuals_host(NULL, e, 2, 1, out, NULL, NULL, NULL) == OMNI_ERR_INVALID && strstr(omni_last_error(), "omni_pgo_residuals_host: null argument"));
    CHECK(omni_pgo_residuals_host(x, e, 1, 1, out, NULL, NULL, NULL) == OMNI_ERR_INVALID && omni_pgo_residuals_host(x, e, 2, 1, NULL, NULL, NULL, NULL) == OMNI_OK);
    CHECK(omni_pgo_plan_graph_host(NULL, e, 2, 1, NULL, NULL, NULL, NULL) == OMNI_ERR_INVALID && strstr(omni_last_error(), "omni_pgo_plan_graph_host: null argument"));
    CHECK(omni_pgo_create(NULL, NULL) == OMNI_ERR_INVALID && strstr(omni_last_error(), "omni_pgo_create: null argument"));
    CHECK(omni_pgo_solve_multi(NULL, &pr, x, fixed, e, 2, 1, 1, out, st, &best, NULL) == OMNI_ERR_INVALID && strstr(omni_last_error(), "omni_pgo_solve_multi: null argument"));
    omni_pgo_destroy(NULL);
    printf("OK\n");
    return 0;
}
"""


def test_c_program_links_the_library_and_meets_every_refusal(tmp_path):
    src, exe = tmp_path / "pgo_capi.c", tmp_path / "pgo_capi"
    src.write_text(PROGRAM)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", LIBDIR,
                        "-lomni_hip", f"-Wl,-rpath,{LIBDIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr[-2000:]


def test_symbols_are_declared_exported_and_listed(omni):
    c = omni.capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omni_hip.h")).read(), flags=re.S)
    declared = {s for s in re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text) if s.startswith("omni_pgo_")}
    assert declared == NEW
    assert NEW <= set(c.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libomni_hip.so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("omni_pgo_")}
    assert exported == NEW


def test_the_mirror_has_the_headers_sizes_and_defaults(omni):
    c = omni.capi
    assert c.PGO_EDGE_DTYPE.itemsize == 80 and c.PGO_STATS_DTYPE.itemsize == 32 and ctypes.sizeof(c.PgoParams) == 48
    assert c.PGO_EDGE_DTYPE.fields["z"][1] == 8 and c.PGO_EDGE_DTYPE.fields["sqrt_inf"][1] == 40 and c.PGO_EDGE_DTYPE.fields["robust"][1] == 72
    assert c.PGO_STATS_DTYPE.fields["iterations"][1] == 16 and c.PGO_STATS_DTYPE.fields["status"][1] == 24 and c.PgoParams.initial_lambda.offset == 16
    assert (c.PGO_CONVERGED, c.PGO_MAX_ITERATIONS, c.PGO_NONFINITE, c.PGO_EMPTY) == (0, 1, 2, 3)
    assert (c.PGO_MAX_POSES, c.PGO_MAX_EDGES, c.PGO_MAX_STARTS) == (4096, 16384, 64)
    pr = c.pgo_params()
    assert (pr.max_iterations, pr.max_cg_iterations, pr.max_lambda_retries, pr.initial_lambda, pr.function_tolerance, pr.parameter_tolerance, pr.cg_tolerance) == \
        (50, 0, 16, 1e-4, 1e-6, 1e-8, 1e-6)
    assert np.array_equal(c.pgo_sqrt_inf([0.01, 0.04, 0.25], 0.0), [10.0, 5.0, 2.0, np.inf])


def test_the_python_wrappers_refuse(omni):
    c = omni.capi
    g = PC.chain_with_loop(10, seed=3)
    with pytest.raises(c.OmniError, match="one byte per pose"):
        c.pgo_solve_host(g.init, g.fixed[:5], g.edges)
    with pytest.raises(c.OmniError, match=r"\[n\]\[4\]"):
        c.pgo_solve_host(g.init[:, :3], g.fixed, g.edges)
    bad = g.edges.copy()
    bad["i"][0] = -1
    with pytest.raises(c.OmniError, match="outside the graph"):
        c.pgo_solve_host(g.init, g.fixed, bad)
    with pytest.raises(c.OmniError, match="outside the graph"):
        c.pgo_residuals_host(g.init, bad)
    with pytest.raises(c.OmniError, match="outside the graph"):
        c.pgo_plan_graph_host(g.fixed, bad)
    with pytest.raises(c.OmniError, match="n_starts"):
        c.pgo_solve_host(np.zeros((65, 10, 4)), g.fixed, g.edges)


def test_the_makefile_builds_both_objects_with_contraction_off():
    mk = open(os.path.join(ROOT, "omni-swarm_amd", "Makefile")).read()
    assert "build/pgo.o: HIPFLAGS += -ffp-contract=off" in mk and "build/pgo_host.o" in mk.split("OBJS :=")[1].splitlines()[0]
    rule = mk.split("build/pgo_host.o: csrc/pgo_host.cpp")[1].split("\n\n")[0]
    assert "-ffp-contract=off" in rule and "g++" in rule
