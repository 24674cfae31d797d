"""GPU: every number of the SuperPoint descriptor tail (csrc/sp_post.hip: sp_sample_kernel, sp_chan_sumsq_kernel + chan_norm_of, sp_pca_kernel /
copy_raw_desc_kernel) against the float64 ideal of the kernel's own algebra, stage by stage (tests/sp_desc_ref.py; tests/test_gpu_sp_post.py sees the tail only
through one absolute tolerance on its final output against a float32 oracle).

omni_sp_debug_layer "desc_raw" / "desc_norm_partial" return what stage 1 and stage 2 left in HBM, so every stage is gated from ITS OWN input:
  stage 1  desc_raw against the dense map handed to postprocess_dense and the key points it returned;
  stage 2  desc_norm_partial against desc_raw (empty segments exactly 0);
  stage 3  the returned descriptors against desc_raw and desc_norm_partial; the NaN pattern of the reference (a channel that is zero at every key point)
           must be the kernel's, position for position.
  tier 1   |got - y| <= E, derived in tests/sp_desc_ref.py, nothing left out but the NaN positions;
  tier 2   per class of >= 1 000 values (key-point slot mod 8 / mod 4, segment, image slot, in-map taps 4 / 2 / 1, output block of 64):
           RMS(z_gpu) <= c RMS(z_emulation), c = sp_desc_ref.TIER2_C.
Key points are placed exactly through the heat map (plateaus of equal confidence come out in row-major order; isolated peaks in the order of their confidences)
and must come back as placed.  Production passes (inference in all three precisions, batch 3, with and without the fisheye mask) are gated in stages 2 and 3
from their own desc_raw; their stage 1 is bit-identical to the dense path by tests/test_gpu_superpoint.py, re-asserted here once for PREC_F32.

MEASURED on one MI355X (printed with -s): worst tier-1 ratio per stage (sample / sumsq / project; every one must be <= 1) over the cases of each group; every tier-2
ratio of every judged class of every case was 1.000 in all three stages: the kernels follow their float32 emulations rounding for rounding, so c = 2.0 per stage
(sp_desc_ref.TIER2_C), and the tier-1 ratios below are the emulation's own (tests/test_sp_desc_ref_cpu.py prints the same figures).
  counts, PCA 64       n 1 0.7262/0.9539/0.0056  2 0.9138/0.9250/0.0070  7 0.9852/0.9941/0.0169  8 0.9939/0.9560/0.0133  9 0.9598/0.9891/0.0151  15 0.9932/0.9482/0.0147
                       16 0.9914/0.8219/0.0123  17 0.9992/0.6750/0.0130  63 0.9996/0.4616/0.0154  64 0.9962/0.3987/0.0160  65 0.9981/0.7756/0.0153
                       200 0.9997/0.2112/0.0217  200 of max 1000 0.9900/0.1915/0.0165  1000 0.9995/0.0892/0.0234  12 placed, cut at max_num 8 0.9745/0.9722/0.0124
  PCA dimension        none: n 9 0.9216/0.9123/0.4503  200 0.9977/0.1944/0.4491;  1, 63, 65, 128, 256: sample <= 0.9972, sumsq <= 0.9540, project <= 0.0289
  600 x 480 lattice    0.7174/0.2172/0.0172     scales 1e-6 .. 1e3  0.9895/0.7084/0.0180      cancelling projection  0.9877/0.2087/0.0042
  zero / one-nonzero channel  0.9983/0.8727/0.4052 (no PCA), 0.0161 (PCA, one_nonzero; zero_channel: every output NaN, as the reference)
  batches              (0, 200, 1) 0.9975/0.2134/0.0182      (200 NaN, 0, 200) 0.9986/0.2155/0.0234      passes 200, 3, 0, 200 on one handle: <= 0.9975
  production passes    PREC_F16, PREC_SPLIT, PREC_F32, batch 3 (40 + 40 + 61 key points; 26 + 30 + 44 under the mask): sumsq <= 0.7754, project <= 0.0201
(A sample / sumsq ratio near 1 is one rounding of one term, |fl(x) - x| <= u |x| against gamma_1 |x|: the bound is tight there, not loose elsewhere.)

FOUND with this module and fixed (csrc/conv.h sp_sample_coord): the sampler's coordinate chain, written with __fmul_rn / __fsub_rn to be IEEE single operation by
operation, was not: the intrinsics are plain operators in the HIP headers, and hipcc's default contraction made (g + 1) Wc - 1 one v_fma_f32 in sp_sample_kernel and in
each of its four restatements.  With a power-of-two cell count the product is exact and nothing shows (every width tests/test_gpu_sp_post.py uses but 600 hid it below
its 2e-5); at W = 104, 136 and 600 the weights moved by a few ulps and stage 1 exceeded its tier-1 bound 4 to 23 times (13 cases).  Nothing tied the five copies to the
same contraction decision, while the cell each of them picks by floor() has to be the same one: they now call one function with contraction switched off.
"""
import numpy as np
import pytest

from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import sp_desc_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
_WEIGHTS = []


def _weights():
    if not _WEIGHTS:
        _WEIGHTS.append(S.synth_weights(0))
    return _WEIGHTS[0]


def _make(omni, ctx, case, max_batch=None):
    return omni.capi.SuperPoint(ctx, _weights(), case.comp, case.mean, case.W, case.H, R.THRES, case.max_num, omni.capi.PREC_F32,
                                max_batch or len(case.images))


@pytest.fixture(scope="module")
def handles(omni, ctx):
    """One handle per configuration, shared by the cases that use it (so most cases also run behind an earlier pass of another size)."""
    cache = {}

    def get(case):
        key = (case.W, case.H, case.max_num, case.pca_dim, len(case.images), None if case.comp is None else hash(case.comp.tobytes()))
        if key not in cache:
            cache[key] = _make(omni, ctx, case)
        return cache[key]

    yield get
    for sp in cache.values():
        sp.close()


def _taps(sp, batch):
    raw, part = sp.debug_layer("desc_raw", batch), sp.debug_layer("desc_norm_partial", batch)
    assert raw.shape == (batch, sp.max_num, 256, 1) and part.shape == (batch, 8, 256, 1)
    return raw[..., 0], part[..., 0]


def _gate(tag, stage, got, emul, ref, classes):
    assert R.nan_equal(got, ref), (tag, stage, "NaN pattern")
    t1 = R.tier1(got, ref)
    t2 = R.tier2(got, emul, ref, classes)
    print(f"[{stage}] {tag}: tier1 {t1:.4f}  tier2 {t2['ratio']:.3f} at {t2['where']} ({t2['judged']} classes)")
    assert t1 <= 1.0, (tag, stage, t1)
    assert t2["ratio"] <= R.TIER2_C[stage], (tag, stage, t2)


def _gate_tail(tag, counts, raw_t, part_t, descs, comp, mean):
    """Stages 2 and 3 of a pass from its own taps: counts [B], raw_t [B, max_num, 256], part_t [B, 8, 256], descs: the returned descriptors per image."""
    raws = [raw_t[b, :n] for b, n in enumerate(counts)]
    assert np.isfinite(np.concatenate(raws)).all()
    for b, n in enumerate(counts):
        empty = np.array([a == e for a, e in R.segments(n)])
        assert (part_t[b][empty] == 0).all(), (tag, b, "an empty segment is exactly 0")
    _gate(tag, "sumsq", np.concatenate(list(part_t)), np.concatenate([R.sumsq_emul(r) for r in raws]), R.cat_refs([R.sumsq_ref(r) for r in raws]),
          R.seg_classes(len(counts)))
    if sum(counts):
        _gate(tag, "project", np.concatenate(descs), np.concatenate([R.project_emul(r, part_t[b], comp, mean) for b, r in enumerate(raws)]),
              R.cat_refs([R.project_ref(r, part_t[b], comp, mean) for b, r in enumerate(raws)]), R.row_classes(counts, descs[0].shape[1]))


def _run(sp, case, tag=None):
    """One postprocess_dense call of the case's images, every check of the module; returns (results, raw tap, partial tap)."""
    tag = tag or case.name
    B = len(case.images)
    res = sp.postprocess_dense(np.stack([im.semi for im in case.images]), np.stack([im.desc for im in case.images]))
    raw_t, part_t = _taps(sp, B)
    counts = [len(im.kps) for im in case.images]
    for b, im in enumerate(case.images):
        assert np.array_equal(res[b][0].astype(np.int64), im.kps), (tag, b, "the key points are the placed ones, in order")
    again = sp.fetch(B)                                                      # what the caller got is what stage 3 left in HBM
    assert all(a[1].tobytes() == r[1].tobytes() and np.array_equal(a[0], r[0]) for a, r in zip(again, res))
    if sum(counts):
        taps = np.concatenate([R.n_taps(im.kps, case.W, case.H) for im in case.images])
        _gate(tag, "sample", np.concatenate([raw_t[b, :n] for b, n in enumerate(counts)]),
              np.concatenate([R.sample_emul(im.desc, im.kps, case.W, case.H) for im in case.images]),
              R.cat_refs([R.sample_ref(im.desc, im.kps, case.W, case.H) for im in case.images]), R.row_classes(counts, 256, taps))
    _gate_tail(tag, counts, raw_t, part_t, [r[1] for r in res], case.comp, case.mean)
    return res, raw_t, part_t


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_stage_of_the_descriptor_tail(handles, case):
    sp = handles(case)
    res, raw_t, part_t = _run(sp, case)
    counts = [len(im.kps) for im in case.images]
    if max(counts) >= 18:
        assert set(np.concatenate([R.n_taps(im.kps, case.W, case.H) for im in case.images]).tolist()) == {1, 2, 4}
    if case.name.startswith("exact_one_point"):
        # raw / sqrt(fl(raw^2)): sqrt(fl(v^2)) = |v| exactly, so every output is +-1, or 0 / 0 = NaN where the sample is 0
        raw, d = raw_t[0, 0], res[0][1][0]
        assert np.array_equal(np.isnan(d), raw == 0) and np.array_equal(d[raw != 0], np.sign(raw[raw != 0]))
        assert (np.abs(raw[raw != 0]) > 1e-15).all() and (np.abs(raw) < 1e15).all()
    if "zero_channel" in case.name or "200nan" in case.name:
        d = res[0][1]
        assert np.isnan(d).all() if case.comp is not None else (np.isnan(d[:, 5]).all() and np.isfinite(np.delete(d, 5, axis=1)).all())
    if "one_nonzero" in case.name and case.comp is None:
        assert np.isfinite(res[0][1]).all() and np.count_nonzero(res[0][1][:, 5]) == 1 and np.abs(res[0][1][:, 5]).max() == 1.0
    if len(case.images) > 1:
        # every image equals its own single-image call, bit for bit: stage outputs and results (a NaN-channel image leaves its neighbours untouched)
        for b, im in enumerate(case.images):
            (k1, d1, s1), = sp.postprocess_dense(im.semi, im.desc)
            r1, p1 = _taps(sp, 1)
            n = counts[b]
            assert np.array_equal(k1, res[b][0]) and d1.tobytes() == res[b][1].tobytes() and np.array_equal(s1, res[b][2]), (case.name, b)
            assert r1[0, :n].tobytes() == raw_t[b, :n].tobytes() and p1[0].tobytes() == part_t[b].tobytes(), (case.name, b)


def test_passes_of_200_3_0_200_on_one_handle_equal_a_fresh_handle(omni, ctx):
    passes = R.passes_case()
    one = _make(omni, ctx, passes[0])
    for case in passes:
        res, raw_t, part_t = _run(one, case)
        fresh = _make(omni, ctx, case)
        (kf, df, sf), = fresh.postprocess_dense(case.images[0].semi, case.images[0].desc)
        rf, pf = _taps(fresh, 1)
        fresh.close()
        n = len(case.images[0].kps)
        assert np.array_equal(kf, res[0][0]) and df.tobytes() == res[0][1].tobytes() and np.array_equal(sf, res[0][2]), case.name
        assert rf[0, :n].tobytes() == raw_t[0, :n].tobytes() and pf.tobytes() == part_t.tobytes(), case.name
    one.close()


def test_the_taps_refuse_without_a_pass_and_change_nothing(omni, ctx):
    case = next(c for c in CASES if c.name == "batch_0_200_1")
    sp = _make(omni, ctx, case)
    for name in ("desc_raw", "desc_norm_partial"):
        with pytest.raises(omni.capi.OmniError):
            sp.debug_layer(name, 1)                                          # before any pass
    im = case.images[1]
    (k0, d0, s0), = sp.postprocess_dense(im.semi, im.desc)
    for name in ("desc_raw", "desc_norm_partial"):
        with pytest.raises(omni.capi.OmniError):
            sp.debug_layer(name, 2)                                          # batch > the last pass's
    r0, p0 = _taps(sp, 1)
    r1, p1 = _taps(sp, 1)
    assert r0.tobytes() == r1.tobytes() and p0.tobytes() == p1.tobytes()
    (k1, d1, s1), = sp.fetch(1)
    assert np.array_equal(k0, k1) and d0.tobytes() == d1.tobytes() and np.array_equal(s0, s1)
    (k2, d2, s2), = sp.postprocess_dense(im.semi, im.desc)                   # and the next pass is what it was
    assert np.array_equal(k0, k2) and d0.tobytes() == d2.tobytes() and np.array_equal(s0, s2)
    sp.close()


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT", "PREC_F32"])
def test_production_passes_from_their_own_desc_raw(omni, ctx, monkeypatch, prec):
    """inference on 104 x 72, batch 3, without and with the fisheye mask: stages 2 and 3 of the pass from its own taps (the sparse paths' stage 1 is held bit for
    bit to the dense map + sp_sample_kernel by tests/test_gpu_superpoint.py; PREC_F32: re-asserted here on desc_raw itself)."""
    c = omni.capi
    w, h, batch = 104, 72, 3
    comp, mean = synth.pca()
    imgs = np.stack([synth.image_u8(60 + i, h, w, n_shapes=40) for i in range(batch)])
    sp = c.SuperPoint(ctx, _weights(), comp, mean, w, h, 0.015, 200, getattr(c, prec), batch)
    dense = None
    if prec == "PREC_F32":
        monkeypatch.setenv("OMNI_SP_SPARSE_DESC", "0")
        dense = c.SuperPoint(ctx, _weights(), comp, mean, w, h, 0.015, 200, c.PREC_F32, batch)
        monkeypatch.delenv("OMNI_SP_SPARSE_DESC")
    for mask in (False, True):
        res = sp.inference(imgs, fisheye_mask=mask)
        raw_t, part_t = _taps(sp, batch)
        counts = [len(r[0]) for r in res]
        assert sum(counts) > 0
        _gate_tail(f"{prec} mask {int(mask)} n {counts}", counts, raw_t, part_t, [r[1] for r in res], comp, mean)
        if dense is not None:
            rd = dense.inference(imgs, fisheye_mask=mask)
            raw_d, part_d = _taps(dense, batch)
            assert (sp.last_plan() & 128) and not (dense.last_plan() & 128)
            for b, n in enumerate(counts):
                assert np.array_equal(rd[b][0], res[b][0]) and raw_d[b, :n].tobytes() == raw_t[b, :n].tobytes() and part_d[b].tobytes() == part_t[b].tobytes()
    sp.close()
    if dense is not None:
        dense.close()
