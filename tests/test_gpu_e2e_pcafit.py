"""The key-frame pipeline with fit_pca (KeyframePipeline(..., fit_pca=True): every lane's SuperPoint handle feeds a PCA-fit accumulator of its own, csrc/pca_fit.hip)
on the rendered fisheye scene of tests/test_gpu_e2e_scene.py: hits, candidates, every field of every edge, the geometry counters and the database are those of the
run with the switch off; n + skipped is the number of key points of all SuperPoint images (a replay of the same frames on one handle without PCA); the merged
moments agree with the stand-in on the replay's descriptors within 2 n 2^-53 sum |x_i x_j| per entry (lanes change the order of additions: a bound, not bits);
the files pca_fit_write writes create a pipeline that runs, and a handle that projects the replay's rows with them."""
import os

import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import test_gpu_e2e_scene as FE

pytestmark = pytest.mark.gpu
MB, DIRS = 4, 4


@pytest.fixture(scope="module")
def files(omni, tmp_path_factory):
    from omni_swarm_amd import weights
    comp, mean = synth.pca()
    return weights.write_pipeline_files(str(tmp_path_factory.mktemp("e2e_pcafit")), S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), omni.capi.VLAD_KINDS)


@pytest.fixture(scope="module")
def scene():
    plan = FE.schedule()
    first = [q for q in plan[:FE.N_PLACES] if q[0] < 8]
    again = [q for q in plan[FE.N_PLACES:] if q[0] < 8]
    return [(synth.room_keyframe(p, FE.H, FE.W, rv, sg), np.concatenate([pose[0], pose[1]])) for (p, rv, sg, pose) in first + again]


@pytest.fixture(scope="module")
def replay(omni, ctx, scene):
    """every SuperPoint image of the stream (the up and the down views of every key frame, the fisheye mask on) through ONE handle without PCA: per key frame, the
    256-d descriptors of its eight images; computed once"""
    c = omni.capi
    plain = c.SuperPoint(ctx, S.synth_weights(0), None, None, FE.W, FE.H, FE.THR, FE.MAXN, c.PREC_F16, 2 * DIRS)
    try:
        return [[d for (_, d, _) in plain.inference(np.stack(list(views)), fisheye_mask=True)] for views, _ in scene]
    finally:
        plain.close()


def block_of(ctx, kf):
    """the pinned input block of a unit: the up views of its key frames, then the down views"""
    p = ctx.host_alloc((2 * DIRS * len(kf),) + kf[0].shape[1:], np.uint8)
    p[:] = np.stack([v[i] for v in kf for i in range(DIRS)] + [v[DIRS + i] for v in kf for i in range(DIRS)])
    return p


def through(omni, ctx, files, scene, fit_pca, after=None):
    """-> (hits, candidates, edges, geometry stats, database rows), what after(pipeline) returns"""
    from omni_swarm_amd import pipeline
    c, P, n = omni.capi, FE.PARAMS, len(scene)
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], FE.W, FE.H, FE.THR, FE.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, fit_pca=fit_pca)
    pins = []
    try:
        assert pl.fit_pca() == fit_pca
        full = n - n % MB
        for s in range(0, n, MB):
            pins.append(block_of(ctx, [scene[s + m][0] for m in range(min(MB, n - s))]))
        pl.set_poses(0, np.array([pose for _, pose in scene]))
        hits = pl.run(n, 0, [p.ctypes.data for p in pins[:full // MB]], 0, pins[-1].ctypes.data if n % MB else None, True)      # (a trailing partial unit runs on a tail lane)
        pl.sync()
        with pytest.raises(c.OmniError, match="after the first key frame"):
            pl.set_fit_pca(not fit_pca)
        if not fit_pca:
            with pytest.raises(c.OmniError, match="without fit_pca"):
                pl.pca_fit_moments()
        return (hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows), (after(pl) if after else None)
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


def close_to_stand_in(c, m, descs):
    """n + skipped = the replay's key points; the merged moments within 2 n 2^-53 sum |x_i x_j| (s: sum |x_c|) of the stand-in on the replay's descriptors.
    -> (key points, max |S - stand-in|, the bound there)"""
    want = c.PcaMoments().add_descriptors(descs)
    X = np.concatenate(descs).astype(np.float64)
    X = X[np.isfinite(X).all(1)]
    bound = 2 * max(want.n, 1) * 2.0 ** -53 * (np.abs(X).T @ np.abs(X))
    err_S, err_s = np.abs(m.S - want.S), np.abs(m.s - want.s)
    n_points = sum(len(d) for d in descs)
    assert m.n + m.skipped == n_points and (m.n, m.skipped) == (want.n, want.skipped) and m.n > 64
    assert (err_S <= bound).all()
    assert (err_s <= 2 * want.n * 2.0 ** -53 * np.abs(X).sum(0)).all()
    return n_points, err_S.max(), bound.flat[err_S.argmax()]


def test_a_trailing_partial_unit_runs_on_a_tail_lane_that_fits_too(omni, ctx, files, scene, replay):
    """6 key frames at micro-batch 4: one full unit on a lane, two key frames on a tail lane made by the run -- its accumulator is created with it, merged behind
    the lanes' and reset with them"""
    c = omni.capi
    n = MB + 2

    def after(pl):
        m = pl.pca_fit_moments()
        pl.pca_fit_reset()
        z = pl.pca_fit_moments()
        assert (z.n, z.skipped) == (0, 0) and not z.s.any() and not z.S.any()
        return m

    _, m = through(omni, ctx, files, scene[:n], True, after)
    descs = [d for kf in replay[:n] for d in kf]
    lane_only = sum(len(d) for kf in replay[:MB] for d in kf)
    n_points, err, bound = close_to_stand_in(c, m, descs)
    print(f"{n} key frames = one unit of {MB} + a tail unit of {n - MB}: {n_points} key points ({lane_only} on the lane), n {m.n} skipped {m.skipped}; "
          f"max |S - stand-in| {err:.3e} (bound there {bound:.3e})")
    assert m.n + m.skipped > lane_only                                          # the tail lane's rows are in the merge


def test_fit_pca_changes_nothing_and_fits_the_streams_descriptors(omni, ctx, files, scene, replay, tmp_path):
    c = omni.capi
    assert len(scene) % MB == 0
    comp_path, mean_path = str(tmp_path / "components_.csv"), str(tmp_path / "mean_.csv")

    def after(pl):
        m = pl.pca_fit_moments()
        o = pl.pca_fit(64)
        pl.pca_fit_write(comp_path, mean_path, 64)
        pl.pca_fit_reset()
        z = pl.pca_fit_moments()
        assert (z.n, z.skipped) == (0, 0) and not z.s.any() and not z.S.any()
        return m, o

    off, _ = through(omni, ctx, files, scene, False)
    on, (m, o) = through(omni, ctx, files, scene, True, after)
    assert len(off[1]) >= 4 and len(off[2]) >= 2                                # loop candidates and accepted edges: not vacuous
    assert on[0] == off[0] and on[3] == off[3] and on[4] == off[4]
    assert np.array_equal(on[1], off[1])
    assert on[2].shape == off[2].shape and np.array_equal(on[2], off[2])        # every field of every edge, bit for bit

    # against the replay of the same frames on one handle without PCA
    descs = [d for kf in replay for d in kf]
    n_points, err, bound = close_to_stand_in(c, m, descs)
    print(f"{len(scene)} key frames, {len(descs)} SuperPoint images, {n_points} key points: n {m.n} skipped {m.skipped}; max |S - stand-in| {err:.3e} "
          f"(bound there {bound:.3e}); explained variance of 64 components {o['explained_variance'].sum() / o['total_variance']:.4f}")

    # the written files: what the solve returned, and a pipeline created on them runs
    comp32, mean32 = np.loadtxt(comp_path, delimiter=",", dtype=np.float32), np.loadtxt(mean_path, dtype=np.float32)
    assert comp32.shape == (64, 256) and mean32.shape == (256,)
    assert np.array_equal(comp32, o["components_f32"]) and np.array_equal(mean32, o["mean_f32"])
    fitted = dict(files, comp=comp_path, mean=mean_path)
    again, _ = through(omni, ctx, fitted, scene, False)
    assert again[4] == off[4] and len(again[1]) >= 1                             # the same database rows; the revisits still find candidates
    # ... and a handle created with them returns (x - mean) . comp^T of the replay's rows (the projection gate of tests/test_gpu_superpoint.py: 1e-4)
    sp = c.SuperPoint(ctx, S.synth_weights(0), comp32, mean32, FE.W, FE.H, FE.THR, FE.MAXN, c.PREC_F16, 2 * DIRS)
    try:
        views = np.stack(list(scene[0][0]))
        got = [d for (_, d, _) in sp.inference(views, fisheye_mask=True)]
    finally:
        sp.close()
    worst = 0.0
    for g, x in zip(got, descs[:2 * DIRS]):
        assert g.shape == (len(x), 64)
        ok = np.isfinite(x).all(1)
        if ok.any():
            worst = max(worst, float(np.abs(g[ok] - (x[ok] - mean32) @ comp32.T).max()))
    print(f"64-d descriptors of key frame 0 with the fitted files vs (x - mean) . comp^T: {worst:.3e}")
    assert worst < 1e-4
    assert os.path.getsize(comp_path) > 64 * 256 * 2
