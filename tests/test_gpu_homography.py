"""The homography-RANSAC kernel alone (csrc/homography.hip through omni_homography_ransac_multi) against the CPU build of the arithmetic it runs
(csrc/ransac_plan.h in tests/cpp/ransac_plan_pin.cpp, itself held to geom::find_homography_ransac's bits by tests/test_ransac_plan_cpu.py) on the same point
lists: status, mask, info and the BITS of H identical.  That is the design: the same f64 operations in the same order, IEEE add / mul / div / sqrt, contraction
off, the stop rule an integer scan.  Cases: tests/homography_cases.py gate_cases (counts 0 .. 200, planted shares 0 .. 1, matches dropped by the flags, the count-5
pair without a valid subset, duplicated and collinear points), grouped into calls of 1, 5 and 64 pairs."""
import ctypes

import numpy as np
import pytest

from tests import homography_cases as Hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    cases = Hc.gate_cases()
    ref = Hc.run_pin(Hc.build_pin(tmp_path_factory.mktemp("ransac_plan")), ("plan", 64), cases)
    return cases, ref, [Hc.point_lists(c, r) for c, r in zip(cases, ref)]


def compare(got, ref, label):
    """counts of differing items, printed; -> True when every pair of the call is identical"""
    st = sum(g["status"] != r["status"] for g, r in zip(got, ref))
    info = sum(g["info"].tolist() != [r["count"], r["iters_run"], r["best_iter"], r["max_good"]] for g, r in zip(got, ref))
    mask = sum(int((g["mask"] != r["mask"][:len(g["mask"])]).sum()) if len(g["mask"]) == r["n_kept"] else r["n_kept"] for g, r in zip(got, ref))
    hb = sum(int((g["H"].view(np.uint64) != np.ascontiguousarray(r["H"]).view(np.uint64)).sum()) for g, r in zip(got, ref))
    worst = max(float(np.abs(g["H"] - r["H"]).max()) for g, r in zip(got, ref))
    print(f"{label}: {len(got)} pairs, statuses GPU {[g['status'] for g in got]}; differing: statuses {st}, info rows {info}, mask entries {mask} of {sum(r['n_kept'] for r in ref)}, "
          f"H entries by bits {hb} (largest difference {worst:.3g}); iterations run {[int(g['info'][1]) for g in got]}; tied eigenvalues on the CPU: {sum(r['ties'] for r in ref)}")
    return st == 0 and info == 0 and mask == 0 and hb == 0


# single pairs: count 200 at share 0 (all 2 000 iterations) and 0.9 (one round), count 4, 5, 65, flags dropping some, the pair without a valid subset, the two
# degenerate ones; five pairs: the five shares of count 63 and of count 200; 64 pairs: every case in one call
CALLS = [(i, 1) for i in (45, 48, 10, 15, 42, 55, 61, 62, 63)] + [(30, 5), (45, 5), (0, 64)]


@pytest.mark.parametrize("first,n", CALLS)
def test_kernel_equals_the_cpu_build_bit_for_bit(omni, ctx, reference, first, n):
    cases, ref, pts = reference
    assert len(cases) == 64
    got = omni.capi.homography_ransac_multi(ctx, pts[first:first + n])
    r = ref[first:first + n]
    assert sum(x["ties"] for x in r) == 0
    assert compare(got, r, f"cases {first}..{first + n - 1}")


def test_statuses_cover_every_kind(reference):
    cases, ref, _ = reference
    assert {r["status"] for r in ref} == {Hc.UNFILTERED, Hc.OK, Hc.NO_MODEL, Hc.HOST}
    assert [r["status"] for r in ref[-Hc.DEGENERATE:]] == [Hc.HOST] * Hc.DEGENERATE and all(r["status"] != Hc.HOST for r in ref[:-Hc.DEGENERATE])
    assert ref[45]["iters_run"] == 2000 and 0 < ref[48]["iters_run"] <= 64


def test_refusals(omni, ctx):
    """each before anything is launched: n_pairs outside 1..64, max_n outside 1..1024, a count beyond max_n, null arrays"""
    c = omni.capi
    lib = c.lib()
    src, cnt = np.zeros((65, 8, 2), np.float32), np.full(65, 8, np.int32)
    st, mask, H, info = np.zeros(65, np.int32), np.zeros((65, 8), np.uint8), np.zeros((65, 9)), np.zeros((65, 4), np.int32)
    fp, ip, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    args = lambda: (src.ctypes.data_as(fp), src.ctypes.data_as(fp), cnt.ctypes.data_as(ip), st.ctypes.data_as(ip), mask.ctypes.data, H.ctypes.data_as(dp), info.ctypes.data_as(ip))
    for pairs, max_n, code, what in ((0, 8, c.ERR_CAPACITY, "n_pairs=0"), (65, 8, c.ERR_CAPACITY, "n_pairs=65"), (2, 0, c.ERR_CAPACITY, "max_n=0"), (2, 1025, c.ERR_CAPACITY, "max_n=1025"),
                                    (2, 7, c.ERR_CAPACITY, "count=8")):
        assert lib.omni_homography_ransac_multi(ctx.h, pairs, max_n, *args()) == code and what in lib.omni_last_error().decode(), (what, lib.omni_last_error())
    a = list(args())
    for k in range(7):
        b = list(a)
        b[k] = None
        assert lib.omni_homography_ransac_multi(ctx.h, 2, 8, *b) == c.ERR_INVALID and b"null" in lib.omni_last_error()
    assert lib.omni_homography_ransac_multi(None, 2, 8, *a) == c.ERR_INVALID
