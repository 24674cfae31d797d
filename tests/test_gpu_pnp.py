"""The PnP-RANSAC kernel (csrc/pnp.hip through omni_pnp_ransac_multi) against the CPU build of the arithmetic it runs (csrc/pnp_plan.h in
tests/cpp/pnp_plan_pin.cpp, itself held to geom::ransac_run<PnPModel>'s bits by tests/test_pnp_plan_cpu.py) on the same correspondences: status, info, mask and
the BITS of the 12 doubles of the best model identical.  That is the design: the same f64 operations in the same order, IEEE add / mul / div / sqrt, contraction
off, the stop rule an integer scan.  Cases: tests/pnp_cases.py gate_cases (counts 0 .. 2 048, planted shares 0 .. 1, limits of 7, 100 and 1 000 iterations, a
coplanar and a duplicated set), in calls of 1, 5 and 64 candidates."""
import ctypes

import numpy as np
import pytest

from tests import pnp_cases as Pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    cases = Pc.gate_cases()
    return cases, Pc.run_pin(Pc.build_pin(tmp_path_factory.mktemp("pnp_plan")), ("plan", 64), cases)


def compare(got, ref, label):
    """counts of differing items, printed; -> True when every candidate of the call is identical"""
    st = sum(g["status"] != r["status"] for g, r in zip(got, ref))
    info = sum(g["info"].tolist() != [r["count"], r["iters_run"], r["best_iter"], r["max_good"]] for g, r in zip(got, ref))
    mask = sum(int((g["mask"] != r["mask"]).sum()) if len(g["mask"]) == len(r["mask"]) else len(r["mask"]) for g, r in zip(got, ref))
    rb = sum(int((Pc.bits(g["Rt"]) != Pc.bits(r["Rt"])).sum()) for g, r in zip(got, ref))
    worst = max(float(np.abs(g["Rt"] - r["Rt"]).max()) for g, r in zip(got, ref))
    print(f"{label}: {len(got)} candidates, statuses GPU {[g['status'] for g in got]}; differing: statuses {st}, info rows {info}, mask entries {mask} of {sum(r['count'] for r in ref)}, "
          f"Rt entries by bits {rb} (largest difference {worst:.3g}); iterations run {[int(g['info'][1]) for g in got]}")
    return st == 0 and info == 0 and mask == 0 and rb == 0


# single candidates as (count, share, limit): count 6; 64 / 65; 300 (above the workgroup's 256 lanes); the largest count at share 0 and 1 000 iterations (every
# round runs: 64 + 3 x 256 + a last round of 168) and at share 0.9 (the stop falls in the first round); 7 iterations; counts 0 and 5 (skipped)
SINGLES = [(6, 0.6, 100), (6, 0.0, 1000), (64, 0.9, 100), (65, 0.0, 100), (300, 0.3, 100), (Pc.MAX_N, 0.0, 1000), (Pc.MAX_N, 0.9, 1000), (200, 0.0, 1000), (200, 0.9, 1000),
           (200, 0.0, 7), (0, 0.0, 100), (5, 1.0, 100)]


@pytest.mark.parametrize("count,share,limit", SINGLES)
def test_one_candidate_equals_the_cpu_build_bit_for_bit(omni, ctx, reference, count, share, limit):
    cases, ref = reference
    i = Pc.index_of(cases, count, share, limit)
    got = omni.capi.pnp_ransac_multi(ctx, [(cases[i]["X"], cases[i]["u"], limit)])
    assert compare(got, ref[i:i + 1], f"case {i}")


# five candidates: the five shares of count 63 and of count 1 500; the last five cases (7 iterations, the coplanar and the duplicated set).  64 candidates: the
# first 64 cases (every count, 100 and 1 000 iterations) and the last 64 (limits of 100, 1 000 and 7 in one call, the degenerate sets)
@pytest.mark.parametrize("first,n", [(25, 5), (50, 5), (87, 5), (0, 64), (28, 64)])
def test_calls_of_several_candidates_equal_the_cpu_build_bit_for_bit(omni, ctx, reference, first, n):
    cases, ref = reference
    assert len(cases) == 92
    sub = cases[first:first + n]
    if n == 64:
        assert len({c["max_iters"] for c in sub}) >= 2                       # mixed limits in one call
    got = omni.capi.pnp_ransac_multi(ctx, [(c["X"], c["u"], c["max_iters"]) for c in sub])
    assert compare(got, ref[first:first + n], f"cases {first}..{first + n - 1}")


def test_statuses_and_rounds_cover_every_kind(reference):
    cases, ref = reference
    assert {r["status"] for r in ref} == {Pc.SKIPPED, Pc.OK, Pc.NO_MODEL}      # HOST: no gate case reaches the draw budget on the CPU build either
    full = ref[Pc.index_of(cases, Pc.MAX_N, 0.0, 1000)]
    assert full["iters_run"] == 1000 and (1000 - 64) % 256 != 0                # every round, the last one partial
    assert 0 < ref[Pc.index_of(cases, 200, 0.9, 1000)]["iters_run"] <= 64      # the stop falls in the first round
    assert any(r["status"] == Pc.NO_MODEL and r["max_good"] == 5 for r in ref)


def test_refusals(omni, ctx):
    """each before anything is launched: n_cands outside 1..64, max_n outside 1..2048, a count beyond max_n, a limit outside 1..1000, null arrays"""
    c = omni.capi
    lib = c.lib()
    X, u, cnt, it = np.zeros((65, 8, 3), np.float32), np.zeros((65, 8, 2), np.float32), np.full(65, 8, np.int32), np.full(65, 100, np.int32)
    st, mask, Rt, info = np.zeros(65, np.int32), np.zeros((65, 8), np.uint8), np.zeros((65, 12)), np.zeros((65, 4), np.int32)
    fp, ip, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    args = lambda: (X.ctypes.data_as(fp), u.ctypes.data_as(fp), cnt.ctypes.data_as(ip), it.ctypes.data_as(ip), st.ctypes.data_as(ip), mask.ctypes.data, Rt.ctypes.data_as(dp),
                    info.ctypes.data_as(ip))
    for cands, max_n, code, what in ((0, 8, c.ERR_CAPACITY, "n_cands=0"), (65, 8, c.ERR_CAPACITY, "n_cands=65"), (2, 0, c.ERR_CAPACITY, "max_n=0"),
                                     (2, c.PNP_MAX_POINTS + 1, c.ERR_CAPACITY, f"max_n={c.PNP_MAX_POINTS + 1}"), (2, 7, c.ERR_CAPACITY, "count=8")):
        assert lib.omni_pnp_ransac_multi(ctx.h, cands, max_n, *args()) == code and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
    for bad in (0, c.PNP_MAX_ITERS + 1):
        it[1] = bad
        assert lib.omni_pnp_ransac_multi(ctx.h, 2, 8, *args()) == c.ERR_CAPACITY and f"max_iters={bad}" in lib.omni_last_error().decode()
    it[1] = 100
    a = list(args())
    for k in range(8):
        b = list(a)
        b[k] = None
        assert lib.omni_pnp_ransac_multi(ctx.h, 2, 8, *b) == c.ERR_INVALID and b"null" in lib.omni_last_error()
    assert lib.omni_pnp_ransac_multi(None, 2, 8, *a) == c.ERR_INVALID
    assert not st.any() and not mask.any() and not Rt.any() and not info.any()      # nothing was written
