#!/usr/bin/env python3
"""tests/golden/pca_fit_cases.npz: rows with a known spectrum and what scikit-learn's PCA(64, svd_solver='full') -- the fit of the reference's pca.ipynb -- makes of
them, so that csrc/pca_plan.h's solve is gated against the library the reference's workflow uses (tests/test_pca_plan_cpu.py).  CPU only; needs scikit-learn.

    rng = default_rng(20261020);  Q = qr(normal(256, 256));  sigma_k = 0.07 * 0.96**k
    X = (normal(300, 256) * sigma) @ Q + 0.05 * normal(256), stored as float32;  PCA fitted on X.astype(float64)

The tool asserts that the fixture is well conditioned for the gates that rest on it: the smallest relative gap between neighbouring eigenvalues among the first
64 is >= 5e-3, and numpy's eigh on the f64 moment covariance agrees with scikit-learn's components within 1e-11.
"""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, DIM, PCA_DIM, SEED = 300, 256, 64, 20261020


def make_rows():
    rng = np.random.default_rng(SEED)
    Q, _ = np.linalg.qr(rng.normal(size=(DIM, DIM)))
    sigma = 0.07 * 0.96 ** np.arange(DIM)
    X = (rng.normal(size=(N_ROWS, DIM)) * sigma) @ Q + 0.05 * rng.normal(size=DIM)
    return X.astype(np.float32)


def flip_rows(v):
    """the entry of largest magnitude of each row positive, ties to the lowest column"""
    arg = np.argmax(np.abs(v), axis=1)
    return v * np.sign(v[np.arange(len(v)), arg])[:, None]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pca_fit_cases.npz"))
    args = ap.parse_args()
    import sklearn
    from sklearn.decomposition import PCA
    X = make_rows()
    Xd = X.astype(np.float64)
    pca = PCA(PCA_DIM, svd_solver="full").fit(Xd)
    ev = pca.explained_variance_
    # the whole spectrum for the gap: the 64th eigenvalue's neighbour is the 65th
    n = len(Xd)
    s, S = Xd.sum(0), Xd.T @ Xd
    cov = (S - np.outer(s, s) / n) / (n - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1], v[:, ::-1].T
    gap = np.min((w[:PCA_DIM] - w[1:PCA_DIM + 1]) / w[:PCA_DIM])
    d_comp = np.abs(flip_rows(v[:PCA_DIM]) - flip_rows(pca.components_)).max()
    d_ev = np.abs(w[:PCA_DIM] / ev - 1).max()
    signs_as_sklearn = np.array_equal(flip_rows(pca.components_), pca.components_)
    print(f"scikit-learn {sklearn.__version__}: rows {X.shape}, smallest relative eigenvalue gap among the first {PCA_DIM}: {gap:.3e}")
    print(f"numpy eigh on the f64 moment covariance vs scikit-learn: components {d_comp:.3e}, explained variance (relative) {d_ev:.3e}")
    print(f"scikit-learn's own signs follow the largest-magnitude rule: {signs_as_sklearn}")
    assert gap >= 5e-3, gap
    assert d_comp < 1e-11, d_comp
    assert signs_as_sklearn
    np.savez_compressed(args.out, X=X, components_=pca.components_, mean_=pca.mean_, explained_variance_=ev)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
