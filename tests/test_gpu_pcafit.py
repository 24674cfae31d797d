"""The gfx950 build of the PCA fit's moments (omni_pcafit_enqueue_rows_dev: csrc/pca_fit.hip walking csrc/pca_plan.h's chain, one v_fma_f64 per entry per kept row)
against the g++ build of the same header (omni_pca_moments_host, which tests/test_pca_plan_cpu.py holds to numpy in f64): n, skipped, every entry of s and every
entry of S bit for bit, whatever the batch, max_num, the images' key-point counts and the number of consecutive enqueues."""
import numpy as np
import pytest

from tests import pcafit_cases as P

pytestmark = pytest.mark.gpu


def _device(omni, ctx, fit, passes):
    for p in passes:
        ptrs = [ctx.to_device(p[k]) for k in ("raw", "part", "n_kps")]
        try:
            fit.enqueue_rows_dev(*ptrs, len(p["n_kps"]), p["max_num"])
            ctx.sync()                                    # (the operands are freed below)
        finally:
            for q in ptrs:
                ctx.free(q)
    return fit.moments()


def _host(omni, passes):
    m = omni.capi.PcaMoments()
    for p in passes:
        m.add_rows(p["raw"], p["part"], p["n_kps"])
    return m


CASES = {
    "batch1_m8_full": [dict(n_kps=[8], max_num=8)],
    "batch1_m8_one": [dict(n_kps=[1], max_num=8)],
    "batch1_m8_none": [dict(n_kps=[0], max_num=8)],
    "batch1_m200_seven": [dict(n_kps=[7], max_num=200)],
    "batch1_m200_full": [dict(n_kps=[200], max_num=200)],
    "batch3_m8_mixed": [dict(n_kps=[0, 8, 7], max_num=8)],
    "batch3_m200_mixed": [dict(n_kps=[1, 200, 7], max_num=200)],
    "batch3_m200_mixed_b": [dict(n_kps=[200, 0, 200], max_num=200)],
    "zero_channel_image": [dict(n_kps=[7, 200, 8], max_num=200, zero_channel_images=(1,))],
    "counts_beyond_range": [dict(n_kps=[-3, 9, 8], max_num=8, garbage=False)],              # clamped to 0 .. max_num
    "two_enqueues": [dict(n_kps=[200, 7, 1], max_num=200), dict(n_kps=[8], max_num=8)],
    "three_enqueues": [dict(n_kps=[7], max_num=8), dict(n_kps=[0, 200, 65], max_num=200, zero_channel_images=(2,)), dict(n_kps=[64, 128, 1], max_num=200)],
}


def _passes(name):
    out = []
    for i, kw in enumerate(CASES[name]):
        kw = dict(kw)
        n_kps = kw.pop("n_kps")
        clamped = np.clip(n_kps, 0, kw["max_num"])
        p = P.make_pass(1000 + 17 * i + len(name), clamped, **kw)
        p["n_kps"] = np.asarray(n_kps, np.int32)
        out.append(p)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_device_moments_equal_the_host_build_bit_for_bit(omni, ctx, name):
    passes = _passes(name)
    want = _host(omni, passes)
    fit = omni.capi.PcaFit(ctx)
    try:
        got = _device(omni, ctx, fit, passes)
        kept = sum(int(np.isfinite(P.rows_of(dict(p, n_kps=np.clip(p["n_kps"], 0, p["max_num"])))).all(1).sum()) for p in passes)
        total = sum(int(np.clip(p["n_kps"], 0, p["max_num"]).sum()) for p in passes)
        print(f"{name}: n {got.n} skipped {got.skipped} (host {want.n} / {want.skipped}; numpy {kept} / {total - kept})")
        assert (want.n, want.skipped) == (kept, total - kept)
        assert P.same_moments(got, want) == []
        assert np.array_equal(got.S, got.S.T)
    finally:
        fit.close()


def test_cut_into_calls_changes_no_bit_and_reset_gives_zeros(omni, ctx):
    """the same rows as ONE pass of three images and as three passes of one image each; then reset"""
    whole = P.make_pass(77, [65, 200, 7], 200)
    parts = [{"raw": whole["raw"][b:b + 1], "part": whole["part"][b:b + 1], "n_kps": whole["n_kps"][b:b + 1], "max_num": 200} for b in range(3)]
    fit = omni.capi.PcaFit(ctx)
    try:
        a = _device(omni, ctx, fit, [whole])
        assert a.n == 272
        fit.reset()
        z = fit.moments()
        assert (z.n, z.skipped) == (0, 0) and not z.s.any() and not z.S.any()
        b = _device(omni, ctx, fit, parts)
        assert P.same_moments(a, b) == []
        assert P.same_moments(a, _host(omni, [whole])) == []
        # the handle's own solve = moments + the host solve
        o, w = fit.solve(64), a.solve(64)
        assert all(np.array_equal(o[k], w[k]) for k in ("components", "components_f32", "mean", "mean_f32", "explained_variance")) and o["total_variance"] == w["total_variance"]
    finally:
        fit.close()


def test_refusals(omni, ctx):
    c = omni.capi
    fit = c.PcaFit(ctx)
    try:
        p = ctx.alloc(4096)
        for batch, max_num, word in ((0, 8, "batch"), (1, 0, "max_num"), (1, 1025, "max_num")):
            with pytest.raises(c.OmniError) as e:
                fit.enqueue_rows_dev(p, p, p, batch, max_num)
            assert word in str(e.value)
        with pytest.raises(c.OmniError) as e:
            fit.enqueue_rows_dev(None, p, p, 1, 8)
        assert "null" in str(e.value)
        ctx.free(p)
        with pytest.raises(c.OmniError) as e:
            fit.solve(64)                                 # nothing accumulated
        assert "n < 2" in str(e.value)
    finally:
        fit.close()
