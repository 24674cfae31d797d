"""A PCA fit attached to a SuperPoint handle (omni_sp_set_pcafit: csrc/pca_fit.hip behind sp_chan_sumsq_kernel on the pass's own stream), on the smallest image of
tests/test_gpu_superpoint.py, for every precision: the pass returns the same bytes with and without a fit, and the fit's moments after two passes equal, bit for
bit, the stand-in (omni_pca_moments_host) fed the 256-d descriptors that a handle WITHOUT PCA of the same weights and precision returns for the same images."""
import numpy as np
import pytest

from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import pcafit_cases as P

pytestmark = pytest.mark.gpu
W, H = 96, 64


def _bytes(res):
    return [tuple(a.tobytes() for a in r) for r in res]


@pytest.fixture(scope="module")
def images():
    return [np.stack([synth.image_u8(400 + 2 * p + i, H, W, n_shapes=60) for i in range(2)]) for p in range(2)]


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_F16", "PREC_SPLIT"])
def test_fit_changes_no_byte_and_equals_the_stand_in(omni, ctx, images, prec):
    c = omni.capi
    weights = S.synth_weights(0)
    comp, mean = synth.pca()
    sp = c.SuperPoint(ctx, weights, comp, mean, W, H, 0.015, 200, getattr(c, prec), 2)
    plain = c.SuperPoint(ctx, weights, None, None, W, H, 0.015, 200, getattr(c, prec), 2)
    fit = c.PcaFit(ctx)
    try:
        without = [_bytes(sp.inference(im)) for im in images]
        sp.set_pcafit(fit)
        with_fit = [_bytes(sp.inference(im)) for im in images]
        assert with_fit == without
        got = fit.moments()
        descs = [d for im in images for (_, d, _) in plain.inference(im)]
        assert all(d.shape[1] == 256 for d in descs)
        want = c.PcaMoments().add_descriptors(descs)
        n_points = sum(len(d) for d in descs)
        print(f"{prec}: {n_points} key points in {len(descs)} images, n {got.n} skipped {got.skipped}")
        assert got.n + got.skipped == n_points and got.n > 64
        assert P.same_moments(got, want) == []
        # detached: a pass adds nothing; attached again: it does
        sp.set_pcafit(None)
        assert _bytes(sp.inference(images[0])) == without[0]
        assert fit.stats() == (got.n, got.skipped)
        sp.set_pcafit(fit)
        sp.inference(images[0])
        want.add_descriptors(descs[:2])
        assert P.same_moments(fit.moments(), want) == []
        # a fisheye-masked pass over an all-black image: whatever key points it returns (none) are what the fit counts
        before = fit.stats()
        black = sp.inference(np.zeros((2, H, W), np.uint8), fisheye_mask=True)
        n_black = sum(len(k) for k, _, _ in black)
        print(f"{prec}: all-black masked pass: {n_black} key points")
        after = fit.stats()
        assert n_black == 0 and after == before
        assert P.same_moments(fit.moments(), want) == []
        # and the fit of what was accumulated is a projection the handle's own kind takes: [64][256] with orthonormal rows
        o = fit.solve(64)
        assert o["components_f32"].shape == (64, 256) and np.abs(o["components"] @ o["components"].T - np.eye(64)).max() < 1e-12
    finally:
        sp.set_pcafit(None)
        fit.close(); sp.close(); plain.close()


def test_one_fit_one_handle_one_context_and_either_may_go_first(omni, ctx, images):
    """a fit of another context of the same device is refused (its stream is not the pass's); so is a fit another handle holds; a fit closed while attached is
    let go of by the handle, and a handle closed while attached lets go of the fit"""
    c = omni.capi
    weights = S.synth_weights(0)
    a = c.SuperPoint(ctx, weights, None, None, W, H, 0.015, 200, c.PREC_F16, 2)
    b = c.SuperPoint(ctx, weights, None, None, W, H, 0.015, 200, c.PREC_F16, 2)
    other = c.Context(0)
    foreign, fit = c.PcaFit(other), c.PcaFit(ctx)
    try:
        with pytest.raises(c.OmniError) as e:
            a.set_pcafit(foreign)
        assert "another context" in str(e.value)
        without = _bytes(a.inference(images[0]))
        a.set_pcafit(fit)
        a.set_pcafit(fit)                                     # again: nothing changes
        with pytest.raises(c.OmniError) as e:
            b.set_pcafit(fit)
        assert "another SuperPoint handle" in str(e.value)
        a.inference(images[0])
        one = fit.stats()
        assert one[0] + one[1] > 0
        a.close()                                             # the handle goes first: the fit is free again and keeps what it has
        b.set_pcafit(fit)
        b.inference(images[0])
        assert fit.stats() == (2 * one[0], 2 * one[1])
        fit.close()                                           # the fit goes first: the handle lets go of it, the next pass is an ordinary one
        assert _bytes(b.inference(images[0])) == without
    finally:
        fit.close(); foreign.close(); a.close(); b.close(); other.close()


def test_a_fit_on_another_device_is_refused(omni, ctx):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    c = omni.capi
    other = c.Context(1)
    weights = S.synth_weights(0)
    sp = c.SuperPoint(ctx, weights, None, None, W, H, 0.015, 200, c.PREC_F16, 1)
    fit = c.PcaFit(other)
    try:
        with pytest.raises(c.OmniError) as e:
            sp.set_pcafit(fit)
        assert "device" in str(e.value)
    finally:
        fit.close(); sp.close(); other.close()
