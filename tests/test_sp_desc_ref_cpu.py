"""CPU: the references, bounds and emulations of tests/sp_desc_ref.py are held themselves -- to exact arithmetic, to float64 F.grid_sample, to the oracle that
restates the reference's text (oracle.postproc_ref.compute_descriptors), and by seeded defects that every gate of tests/test_gpu_sp_desc.py must catch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import postproc_ref as P
from tests import sp_desc_ref as R

CASES = R.cases()


def test_fp32_cells_are_the_ideal_ones_and_weights_stay_within_the_derived_bound():
    """Every kx of five widths: off a cell boundary (kx != 4 mod 8) the fp32 chain's cell is the ideal's; everywhere the weight each cell receives is within
    WEIGHT_ERR = 4 u Wc of the ideal's multiple of 1 / 8; on a boundary the chain lands on the ideal's cell or the one before it."""
    for W in (64, 104, 600, 640, 1280):
        k = np.arange(W)
        x0, w0, w1 = R.axis32(k, W)
        i0, v0, v1 = R.axis_ideal(k, W)
        assert np.array_equal(v0 * 8, np.round(v0 * 8)) and np.array_equal(i0[[3, 4, W - 5, W - 4]], [-1, 0, (W >> 3) - 2, (W >> 3) - 1])
        off = k % 8 != 4
        assert np.array_equal(x0[off], i0[off]), W
        assert np.isin(x0[~off] - i0[~off], (-1, 0)).all(), W
        err = np.abs(R.axis_weights(x0, w0, w1, W >> 3) - R.axis_weights(i0, v0, v1, W >> 3)).max()
        print(f"W {W}: worst weight error {err / (R.U * (W >> 3)):.3f} u Wc (bound 4), {int((x0[~off] != i0[~off]).sum())} of {int((~off).sum())} boundary points land one cell early")
        assert err <= R.weight_err(W >> 3), (W, err)


def _grid_sample64(desc, kps, W, H):
    g = torch.zeros(1, 1, len(kps), 2, dtype=torch.float64)
    g[0, 0, :, 0] = 2.0 * torch.from_numpy(kps[:, 0].astype(np.float64)) / W - 1
    g[0, 0, :, 1] = 2.0 * torch.from_numpy(kps[:, 1].astype(np.float64)) / H - 1
    d = F.grid_sample(torch.from_numpy(desc.astype(np.float64))[None], g, mode="bilinear", padding_mode="zeros", align_corners=False)
    return d[0, :, 0, :].T.numpy()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_reference_against_grid_sample_and_the_oracle(case):
    """The float64 ideal against float64 grid_sample (an independent restatement of align_corners=false); the oracle's float32 results within the allowance
    derived for any float32 restatement, NaN pattern included; the float32 emulation chain within the same allowance and within every stage's tier-1 bound."""
    for b, im in enumerate(case.images):
        n = len(im.kps)
        if n == 0:
            continue
        ch = R.chain_ref(im.desc, im.kps, case.W, case.H, case.comp, case.mean)
        g64 = _grid_sample64(im.desc, im.kps, case.W, case.H)
        # float64 grid_sample rounds its coordinates (2^-53 Wc on a weight): the same bound with float64's unit roundoff
        assert (np.abs(g64 - ch["raw"].y) <= ch["raw"].E * 2.0 ** -29 + 1e-300).all()
        out32, q32 = P.compute_descriptors(im.desc, im.kps, case.W, case.H, case.comp, case.mean)
        assert R.nan_equal(q32, ch["q"])
        rq = R.tier1(q32, ch["q"])
        # the stage references, fed stage by stage with the float32 emulation, as the GPU gates feed them with the kernels' outputs
        raw = R.sample_emul(im.desc, im.kps, case.W, case.H)
        part = R.sumsq_emul(raw)
        out = R.project_emul(raw, part, case.comp, case.mean)
        s1, s2, s3 = R.sample_ref(im.desc, im.kps, case.W, case.H), R.sumsq_ref(raw), R.project_ref(raw, part, case.comp, case.mean)
        assert R.nan_equal(out, s3)
        t = (R.tier1(raw, s1), R.tier1(part, s2), R.tier1(out, s3))
        final = ch["out"] if case.comp is not None else ch["q"]
        assert R.nan_equal(out32, final) and R.nan_equal(out, final)
        ro, re = R.tier1(out32, final), R.tier1(out, final)
        print(f"{case.name}[{b}] n {n}: oracle / chain allowance: normalised {rq:.4f} output {ro:.4f}; emulation / chain {re:.4f}; emulation tier 1 per stage {t[0]:.4f} {t[1]:.4f} {t[2]:.4f}")
        assert rq <= 1 and ro <= 1 and re <= 1 and max(t) <= 1
        empty = np.array([a == e for a, e in R.segments(n)])
        assert (part[empty] == 0).all() and (s2.E[empty] == 0).all()


def test_cases_cover_every_position_count_and_dimension():
    taps, seen = set(), set()
    for case in CASES:
        for im in case.images:
            taps |= set(R.n_taps(im.kps, case.W, case.H).tolist())
            sp = R.special_points(case.W, case.H)
            seen |= {i for i, p in enumerate(sp) if (im.kps == np.array(p)).all(axis=1).any()}
    assert taps == {1, 2, 4} and seen == set(range(18))
    singles = {(len(c.images[0].kps), c.max_num) for c in CASES if len(c.images) == 1 and c.pca_dim == 64}
    assert {n for n, _ in singles} >= {0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 1000} and {(8, 8), (200, 200), (1000, 1000)} <= singles
    assert {(c.pca_dim, len(c.images[0].kps)) for c in CASES} >= {(d, n) for d in (None, 1, 63, 64, 65, 128, 256) for n in (9, 200)}
    assert {tuple(len(im.kps) for im in c.images) for c in CASES if len(c.images) == 3} == {(0, 200, 1), (200, 0, 200)}
    cancel = next(c for c in CASES if c.name.startswith("cancel"))
    raw = R.sample_emul(cancel.images[0].desc, cancel.images[0].kps, cancel.W, cancel.H)
    ref = R.project_ref(raw, R.sumsq_emul(raw), cancel.comp, cancel.mean)
    assert (np.abs(ref.y) < 1e-3 * ref.T).all()                           # the projection cancels to below 1e-3 of the sum of its terms' magnitudes


def test_every_seeded_defect_is_caught():
    """Each defect (what a plausible slip in a kernel would compute) must give a tier-1 ratio > 1 or a tier-2 ratio >= 5 c in its stage; the clean emulation passes."""
    W, H = 104, 72
    comp, mean = R.pca_of(64)
    ims = [R.image(W, H, 65, 90), R.image(W, H, 200, 91)]
    counts = [len(im.kps) for im in ims]
    raws = [R.sample_emul(im.desc, im.kps, W, H) for im in ims]
    parts = [R.sumsq_emul(r) for r in raws]
    taps = np.concatenate([R.n_taps(im.kps, W, H) for im in ims])
    refs = {"sample": R.cat_refs([R.sample_ref(im.desc, im.kps, W, H) for im in ims]), "sumsq": R.cat_refs([R.sumsq_ref(r) for r in raws]),
            "project": R.cat_refs([R.project_ref(r, p, comp, mean) for r, p in zip(raws, parts)])}
    cls = {"sample": R.row_classes(counts, 256, taps), "sumsq": R.seg_classes(2), "project": R.row_classes(counts, 64)}

    def run(stage, defect):
        if stage == "sample":
            return np.concatenate([R.sample_emul(im.desc, im.kps, W, H, defect) for im in ims])
        if stage == "sumsq":
            return np.concatenate([R.sumsq_emul(r, defect) for r in raws])
        return np.concatenate([R.project_emul(r, p, comp, mean, defect, parts[b - 1]) for b, (r, p) in enumerate(zip(raws, parts))])

    for stage, defects in (("sample", R.SAMPLE_DEFECTS), ("sumsq", R.SUMSQ_DEFECTS), ("project", R.PROJECT_DEFECTS)):
        clean = run(stage, None)
        t2 = R.tier2(clean, clean, refs[stage], cls[stage])
        assert R.tier1(clean, refs[stage]) <= 1 and t2["ratio"] == 1.0 and t2["judged"] > 0
        for d in defects:
            bad = run(stage, d)
            t1, t2 = R.tier1(bad, refs[stage]), R.tier2(bad, clean, refs[stage], cls[stage])
            print(f"{stage} defect {d}: tier1 {t1:.3g}  tier2 {t2['ratio']:.3g} at {t2['where']}  (5 c = {5 * R.TIER2_C[stage]:.1f})")
            assert t1 > 1 or t2["ratio"] >= 5 * R.TIER2_C[stage], (stage, d, t1, t2)
