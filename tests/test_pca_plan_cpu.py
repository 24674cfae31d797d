"""csrc/pca_plan.h on the host (no GPU): the g++ build in libomni_hip.so (omni_pca_moments_host, the stand-in the kernels of csrc/pca_fit.hip equal bit for bit;
omni_pcafit_merge_host; omni_pca_solve_host) against numpy in f64 and against scikit-learn's PCA(64, svd_solver='full') on the fixture
tests/golden/pca_fit_cases.npz (tools/gen_pca_fit_golden.py), and the header as a stand-alone program under ASan + UBSan (tests/cpp/pcafit_pin.cpp).

Gates.  Moments: |S - X^T X| <= n 2^-53 sum_k |x_ki x_kj| per entry, the bound of a chain of n fused multiply-adds (products of two f32 values are exact in f64, so
every step rounds once); s likewise with sum_k |x_kc|.  Solve against the fixture: components (f64) 1e-9 -- three orders above what two independent f64 solvers
differ by on this matrix (5e-13) and four below what an f32 fit gives (9.5e-6) --, mean 1e-12, explained variance 1e-10 relative, the f32 outputs 1e-7."""
import os
import subprocess

import numpy as np
import pytest

from tests import pcafit_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("pca_fit_cases.npz")


@pytest.fixture(scope="module")
def solved(omni, fixture):
    m = omni.capi.PcaMoments().add_descriptors([fixture["X"]])
    return m, m.solve(64)


def test_moments_against_numpy_f64(omni):
    p = P.make_pass(11, [200, 65, 7, 0, 1], 200)
    m = omni.capi.PcaMoments().add_rows(p["raw"], p["part"], p["n_kps"])
    X = P.rows_of(p).astype(np.float64)
    n = len(X)
    assert (m.n, m.skipped) == (n, 0) and n == 273
    err_S, bound_S = np.abs(m.S - X.T @ X), n * U * (np.abs(X).T @ np.abs(X))
    err_s, bound_s = np.abs(m.s - X.sum(0)), n * U * np.abs(X).sum(0)
    print(f"{n} rows: max |S - X^T X| {err_S.max():.3e} (bound there {bound_S.flat[err_S.argmax()]:.3e}), max |s - sum| {err_s.max():.3e} (bound {bound_s[err_s.argmax()]:.3e})")
    assert (err_S <= bound_S).all() and (err_s <= bound_s).all()
    assert np.array_equal(m.S, m.S.T)
    # ... and exactly, against the chain restated with Python's own fma-free arithmetic on a few entries: a product of two f32 values is exact in f64
    for (i, j) in ((0, 0), (3, 200), (255, 255)):
        acc = 0.0
        for k in range(n):
            acc = _fma(float(X[k, i]), float(X[k, j]), acc)
        assert acc == m.S[i, j], (i, j)


def _fma(a, b, c):
    """fma(a, b, c) for a, b that are f32 values: a * b is exact in f64, so fma == the correctly rounded sum of the exact product and c"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_cutting_the_stream_changes_no_bit(omni):
    c = omni.capi
    M = 40
    counts = [0, 1, 7, M, 7, 1, M]
    whole = P.make_pass(5, counts, M)
    one = c.PcaMoments().add_rows(whole["raw"], whole["part"], whole["n_kps"])
    assert one.n == sum(counts)

    def cut(bounds):
        m = c.PcaMoments()
        for a, b in zip(bounds[:-1], bounds[1:]):
            m.add_rows(whole["raw"][a:b], whole["part"][a:b], whole["n_kps"][a:b])
        return m
    assert P.same_moments(one, cut([0, 3, 7])) == []              # two calls
    assert P.same_moments(one, cut(list(range(8)))) == []         # seven calls
    # the same rows in a larger max_num (the slots behind them do not exist) and as descriptors with a norm of one
    wide = {"raw": np.full((7, 64, 256), np.nan, np.float32), "part": whole["part"], "n_kps": whole["n_kps"]}
    wide["raw"][:, :M] = whole["raw"]
    assert P.same_moments(one, c.PcaMoments().add_rows(wide["raw"], wide["part"], wide["n_kps"])) == []
    rows = P.rows_of(whole)
    assert P.same_moments(one, c.PcaMoments().add_descriptors([rows[:9], rows[9:]])) == []


def test_an_image_with_a_zero_channel_is_skipped_whole_and_counted(omni):
    c = omni.capi
    p = P.make_pass(6, [7, 40, 3], 40, zero_channel_images=(1,))
    m = c.PcaMoments().add_rows(p["raw"], p["part"], p["n_kps"])
    assert (m.n, m.skipped) == (10, 40) and np.isfinite(m.S).all() and np.isfinite(m.s).all()
    keep = {k: v[[0, 2]] for k, v in p.items() if k != "max_num"}
    assert P.same_moments(c.PcaMoments(skipped=40).add_rows(keep["raw"], keep["part"], keep["n_kps"]), m) == []
    # one non-finite element leaves out that row alone
    q = P.make_pass(7, [8], 8)
    q["raw"][0, 3, 100] = np.inf
    m = c.PcaMoments().add_rows(q["raw"], q["part"], q["n_kps"])
    assert (m.n, m.skipped) == (7, 1)


def test_merge_of_two_halves(omni):
    c = omni.capi
    p = P.make_pass(8, [40, 40, 40, 40], 40)
    left = c.PcaMoments().add_rows(p["raw"][:2], p["part"][:2], p["n_kps"][:2])
    right = c.PcaMoments().add_rows(p["raw"][2:], p["part"][2:], p["n_kps"][2:])
    want_n, want_s, want_S = left.n + right.n, left.s + right.s, left.S + right.S
    left.merge(right)
    assert left.n == want_n == 160 and np.array_equal(left.s, want_s) and np.array_equal(left.S, want_S)      # the rule: element-wise, left += right
    whole = c.PcaMoments().add_rows(p["raw"], p["part"], p["n_kps"])
    X = P.rows_of(p).astype(np.float64)
    assert (np.abs(left.S - whole.S) <= 2 * 160 * U * (np.abs(X).T @ np.abs(X))).all()


def test_solve_against_scikit_learn(fixture, solved):
    m, o = solved
    d = {"components": np.abs(o["components"] - fixture["components_"]).max(), "mean": np.abs(o["mean"] - fixture["mean_"]).max(),
         "explained variance (relative)": np.abs(o["explained_variance"] / fixture["explained_variance_"] - 1).max(),
         "components f32": np.abs(o["components_f32"].astype(np.float64) - fixture["components_"]).max(),
         "mean f32": np.abs(o["mean_f32"].astype(np.float64) - fixture["mean_"]).max()}
    print(", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert m.n == 300 and m.skipped == 0
    assert d["components"] < 1e-9
    assert d["mean"] < 1e-12
    assert d["explained variance (relative)"] < 1e-10
    assert d["components f32"] < 1e-7 and d["mean f32"] < 1e-7
    Xd = fixture["X"].astype(np.float64)
    assert abs(o["total_variance"] - Xd.var(0, ddof=1).sum()) < 1e-12 * o["total_variance"] * 256


def test_signs_order_and_shapes(solved):
    _, o = solved
    v = o["components"]
    arg = np.argmax(np.abs(v), axis=1)
    assert (v[np.arange(64), arg] > 0).all()                                   # the entry of largest magnitude of each row is positive
    assert (np.diff(o["explained_variance"]) <= 0).all()                      # descending
    assert np.abs(v @ v.T - np.eye(64)).max() < 1e-12
    assert np.array_equal(o["components_f32"], v.astype(np.float32)) and np.array_equal(o["mean_f32"], o["mean"].astype(np.float32))


def test_solve_of_a_smaller_pca_dim_is_a_prefix(omni, solved):
    m, o = solved
    o8 = m.solve(8)
    assert np.array_equal(o8["components"], o["components"][:8]) and np.array_equal(o8["explained_variance"], o["explained_variance"][:8])
    assert o8["total_variance"] == o["total_variance"]


def _refused(omni, n, pca_dim, word):
    c = omni.capi
    with pytest.raises(c.OmniError) as e:
        c.pca_solve_host(n, np.zeros(256), np.eye(256), pca_dim)
    assert word in str(e.value), str(e.value)


def test_refused_fewer_than_two_rows(omni):
    _refused(omni, 1, 1, "n < 2")
    _refused(omni, 0, 1, "n < 2")


def test_refused_pca_dim_below_one(omni):
    _refused(omni, 300, 0, "pca_dim outside")


def test_refused_pca_dim_above_256(omni):
    _refused(omni, 300, 257, "pca_dim outside")


def test_refused_no_more_rows_than_components(omni):
    _refused(omni, 64, 64, "n <= pca_dim")
    _refused(omni, 40, 64, "n <= pca_dim")


def test_header_as_a_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pcafit_pin_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pcafit_pin.cpp")])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    comp = np.loadtxt(str(tmp_path / "components_.csv"), delimiter=",")
    assert comp.shape == (64, 256) and np.loadtxt(str(tmp_path / "mean_.csv")).shape == (256,)


def test_the_arithmetic_is_stated_once():
    """pca_plan.h is plain C++ for both compilers; the kernels, the host entries and the pin program only call it"""
    import re
    pkg = os.path.join(ROOT, "omni-swarm_amd")
    plan = open(os.path.join(pkg, "csrc", "pca_plan.h")).read()
    code = re.sub(r"//.*", "", plan)
    for word in ("hip/", "common.h", "std::", "<vector>", "<algorithm>"):
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in plan and code.count("fma(") == 1
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "build/pca_fit.o: HIPFLAGS += -ffp-contract=off" in mk and "build/pca_fit_host.o" in mk and "lib/libomni_host_pca.so" in mk
    kernel = re.sub(r"//.*", "", open(os.path.join(pkg, "csrc", "pca_fit.hip")).read())
    assert "atomic" not in kernel and "fma(" not in kernel and "sqrt" not in kernel and "pca::step(" in kernel and "pca::chan_norm(" in kernel
    assert "/ norm" not in kernel and "(double)" not in kernel and kernel.count("pca::widened(") == 2 and "pca::row_value(" in kernel
    host = re.sub(r"//.*", "", open(os.path.join(pkg, "csrc", "pca_fit_host.cpp")).read())
    assert "fma(" not in host and "sqrt" not in host
