#!/usr/bin/env python3
"""Times the PCA fit of the key-frame stream (csrc/pca_fit.hip, KeyframePipeline::Config::fit_pca) on one commit:

  kernels   the three accumulation kernels alone (omni_pcafit_enqueue_rows_dev on HBM-resident operands): HIP events around one enqueue, for a pass of
            64 images x 200 key points and one of 8 x 200, the two shapes ALTERNATING; median of 20 enqueues each after 5 warm-up enqueues;
  unit      a STEREO_FISHEYE pipeline (fp16, 600 x 480, max_num 200, micro-batch 8: 64 SuperPoint images per unit, geometry off) fed units of 8 key frames by
            run(), fit_pca off and on in two pipelines of the same process, ALTERNATING: per unit the wall time of run(), which returns with the unit collected;
  solve     pca_fit(64) of the pipeline with the switch on: the lanes' moments merged and the 256 x 256 Jacobi on the host, wall time.

    python tools/pcafit_timing.py [--out profiles/pcafit_timing.md] [--units 30]

Records figures; gates nothing."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omni_loader  # noqa: E402

W, H, MAX_NUM, KF, DIRS, REPS, WARMUP = 600, 480, 200, 8, 4, 20, 5
SHAPES = ((64, MAX_NUM), (8, MAX_NUM))


def med(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def time_kernels(c, ctx):
    rng = np.random.default_rng(0)
    fit = c.PcaFit(ctx)
    ops = {}
    for (B, M) in SHAPES:
        raw = rng.normal(size=(B, M, 256)).astype(np.float32)
        part = np.zeros((B, 8, 256), np.float32)
        part[:, 0] = (raw.astype(np.float64) ** 2).sum(1).astype(np.float32)
        ops[(B, M)] = [ctx.to_device(a) for a in (raw, part, np.full(B, M, np.int32))]
    ms = {s: [] for s in SHAPES}
    try:
        for r in range(WARMUP + REPS):
            for s in SHAPES:                                                # alternating: the two shapes see the same machine
                ctx.sync()
                ctx.timer_start()
                fit.enqueue_rows_dev(*ops[s], *s)
                dt = ctx.timer_stop()
                if r >= WARMUP:
                    ms[s].append(dt)
        n, skipped = fit.stats()
    finally:
        fit.close()
        for v in ops.values():
            for p in v:
                ctx.free(p)
    return {s: med(v) for s, v in ms.items()}, n, skipped


def time_units(omni, ctx, n_units):
    from oracle import mobilenetvlad_ref as V
    from oracle import superpoint_ref as S
    from omni_swarm_amd import pipeline, synth, weights
    c = omni.capi
    comp, mean = synth.pca()
    block = ctx.host_alloc((2 * DIRS * KF, H, W), np.uint8)
    block[:] = np.stack([synth.image_u8(700 + i, H, W, n_shapes=200) for i in range(2 * DIRS * KF)])
    res = {}
    with tempfile.TemporaryDirectory() as td:
        files = weights.write_pipeline_files(td, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), c.VLAD_KINDS)
        pls = {on: pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, MAX_NUM, c.PREC_F16, KF, 2, c.STORE_F32, 1, 0.3, 0.2, 5, 30, 3,
                                             fit_pca=on) for on in (False, True)}
        wall = {False: [], True: []}
        try:
            for u in range(WARMUP + n_units):
                for on in (False, True):                                    # alternating
                    t0 = time.perf_counter()
                    pls[on].run(KF, u * KF, [block.ctypes.data], 0, None, True)
                    dt = (time.perf_counter() - t0) * 1e3
                    if u >= WARMUP:
                        wall[on].append(dt)
            m = pls[True].pca_fit_moments()
            solve = []
            for _ in range(3):
                t0 = time.perf_counter()
                o = pls[True].pca_fit(64)
                solve.append((time.perf_counter() - t0) * 1e3)
            res = {"wall": {on: med(v) for on, v in wall.items()}, "n": m.n, "skipped": m.skipped, "solve": med(solve),
                   "explained": float(o["explained_variance"].sum() / o["total_variance"])}
        finally:
            for pl in pls.values():
                pl.close()
    ctx.host_free(block)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcafit_timing.md"))
    ap.add_argument("--units", type=int, default=30)
    args = ap.parse_args()
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    kern, n, skipped = time_kernels(c, ctx)
    units = time_units(omni, ctx, args.units)
    ctx.close()
    lines = ["# PCA fit of the key-frame stream: the accumulation kernels, the unit, the solve", "",
             f"`tools/pcafit_timing.py` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs).  Figures are recorded, not gated.", "",
             "## The accumulation kernels alone", "",
             f"`pca_keep_kernel` + `pca_list_kernel` + `pca_moments_kernel`, HIP events around one `omni_pcafit_enqueue_rows_dev` on HBM-resident operands, every row kept; the two "
             f"shapes alternating, median of {REPS} enqueues each after {WARMUP} warm-up enqueues ({n} rows accumulated, {skipped} skipped).  One chain per entry: a pass of "
             f"B x {MAX_NUM} rows is B x {MAX_NUM} sequential f64 FMAs per entry of S.", "",
             "| pass | median ms | min ms | max ms | us per row |", "|---|---|---|---|---|"]
    lines += [f"| {B} images x {M} key points | {m:.3f} | {lo:.3f} | {hi:.3f} | {m * 1e3 / (B * M):.3f} |" for (B, M), (m, lo, hi) in kern.items()]
    off, on = units["wall"][False], units["wall"][True]
    lines += ["", "## The key-frame unit", "",
              f"A STEREO_FISHEYE pipeline (fp16, {W} x {H}, max_num {MAX_NUM}, micro-batch {KF}: {2 * DIRS * KF} SuperPoint images per unit, 2 lanes, geometry off), `run()` of one unit "
              f"of {KF} key frames, `fit_pca` off and on in two pipelines of one process, alternating; {args.units} timed units each after {WARMUP} warm-up units.  `run()` returns "
              f"with the unit collected, so its wall time is the unit's whole latency on an otherwise idle GPU.  Milliseconds: median (min .. max).", "",
              "| fit_pca | run() wall |", "|---|---|",
              f"| off | {off[0]:.3f} ({off[1]:.3f} .. {off[2]:.3f}) |", f"| on | {on[0]:.3f} ({on[1]:.3f} .. {on[2]:.3f}) |", "",
              f"Medians, on minus off: {on[0] - off[0]:+.3f} ms per unit.  The stream with the switch on accumulated {units['n']} rows ({units['skipped']} skipped).", "",
              "## The solve", "",
              f"`pca_fit(64)`: waits for the lanes, merges their moments and runs the cyclic Jacobi on the 256 x 256 covariance on the host, f64: "
              f"{units['solve'][0]:.0f} ms (min {units['solve'][1]:.0f}, max {units['solve'][2]:.0f}; 3 calls).  The 64 components hold {units['explained']:.4f} of the total variance "
              "of this synthetic stream.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
