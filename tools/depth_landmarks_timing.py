#!/usr/bin/env python3
"""Times PINHOLE_DEPTH's depth landmarks inside the key-frame unit (KeyframePipeline::Config::device_depth_landmarks) against the host path, on one commit:

  kernel    `depth_landmarks_kernel` alone (omni_depth_landmarks_enqueue_dev on HBM-resident arrays): HIP events around one launch, 8 images x 200 key points,
            640 x 480 depth images, the ideal pinhole and a EuRoC-class PINHOLE lens; median of 20 launches after 5 warm-up launches;
  upload    the u16 depth frames of a unit against its gray frames: bytes (the copy's time is inside the unit's figures, not measured apart);
  unit      a PINHOLE_DEPTH pipeline (fp16, 640 x 480, max_num 200, micro-batch 8, the EuRoC-class lens, geometry on) fed units of 8 key frames by run(), the
            switch off and on in two pipelines of the same process, ALTERNATING: per unit the wall time of run() (upload, unit, messages, detector step,
            geometry) and host_times() -- `messages` is what finish() spends building the frame messages, which on the host path holds fill_image_descriptor
            and fill_depth_landmarks.  Median and spread over the timed units.

    python tools/depth_landmarks_timing.py [--out profiles/depth_landmarks_timing.md] [--units 40]

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

W, H, MAX_NUM, KF, REPS, WARMUP = 640, 480, 200, 8, 20, 5
FX = FY = 320.0
CX, CY = 320.0, 240.0
EUROC = dict(type="PINHOLE", k1=-0.2917, k2=0.08228, p1=5.333e-5, p2=-1.578e-4)
EXT = [0.0, 0.0, 0.0, 0.5, -0.5, 0.5, -0.5]


def med(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def time_kernel(c, ctx):
    rng = np.random.default_rng(0)
    kps = np.stack([rng.integers(0, W, (KF, MAX_NUM)), rng.integers(0, H, (KF, MAX_NUM))], 2).astype(np.float32)
    ins = [np.tile(np.array([1.0, 2.0, 0.5, 1, 0, 0, 0]), (KF, 1)), kps, np.full(KF, MAX_NUM, np.int32), rng.integers(300, 9000, (KF, H, W)).astype(np.uint16)]
    outs = [((KF, MAX_NUM, 2), np.float32), ((KF, MAX_NUM, 3), np.float32), ((KF, MAX_NUM), np.uint8), ((KF,), np.int32)]
    dev = [ctx.to_device(a) for a in ins] + [ctx.alloc(int(np.prod(s)) * np.dtype(d).itemsize) for s, d in outs]
    model = c.depth_model(FX, FY, CX, CY, 0.3, 10.0, 30, W, H, EXT)
    rows = []
    try:
        for name, cam in (("ideal", None), ("euroc", c.camera_model(EUROC["type"], EUROC["k1"], EUROC["k2"], EUROC["p1"], EUROC["p2"]))):
            def launch():
                c.depth_landmarks_dev(ctx, model, dev[0], KF, MAX_NUM, dev[1], dev[2], dev[3], W, None, *dev[4:], camera=cam)
            for _ in range(WARMUP):
                launch()
            ctx.sync()
            ms = []
            for _ in range(REPS):
                ctx.timer_start()
                launch()
                ms.append(ctx.timer_stop())
            rows.append((name,) + tuple(x * 1e3 for x in med(ms)) + (int(ctx.from_device(dev[7], (KF,), np.int32).sum()),))
    finally:
        for d in dev:
            ctx.free(d)
    return rows


def time_units(omni, ctx, n_units):
    from oracle import mobilenetvlad_ref as V
    from oracle import superpoint_ref as S
    from omni_swarm_amd import pipeline, synth, weights
    c = omni.capi
    comp, mean = synth.pca()
    frames = [synth.depth_keyframe(p, H, W, 0, 0.0) for p in range(KF)]
    block = ctx.host_alloc((KF, H, W), np.uint8)
    block[:] = np.stack([f[0] for f in frames])
    depth = np.stack([f[1] for f in frames])
    poses = np.tile(np.array([0.0, 0.0, 1.0, 1, 0, 0, 0]), (KF, 1))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        files = weights.write_pipeline_files(td, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), c.VLAD_KINDS)
        pls = {}
        for on in (False, True):
            pls[on] = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, MAX_NUM, c.PREC_F16, KF, 2, c.STORE_F32, 1, 0.3, 0.2, 3, 30, 1,
                                                geometry=True, pinhole_depth=dict(fx=FX, fy=FY, cx=CX, cy=CY, depth_near=0.3, depth_far=7.0, accept_min_3d_pts=30),
                                                camera_model=EUROC, device_depth_landmarks=on)
        wall = {False: [], True: []}
        host = {False: {k: [] for k in ("enqueue", "wait_gpu", "messages", "detector", "geometry")}, True: None}
        host[True] = {k: [] for k in host[False]}
        n3 = {}
        for u in range(WARMUP + n_units):
            for on in (False, True):                                        # alternating: the two paths see the same machine
                pl = pls[on]
                first = u * KF
                pl.set_poses(first, poses)
                pl.set_depth(first, depth)
                pl.host_times(True)
                t0 = time.perf_counter()
                pl.run(KF, first, [block.ctypes.data], 0, None, True)        # returns with the unit's detector step and geometry collected
                dt = (time.perf_counter() - t0) * 1e3
                ht = pl.host_times(True)
                if u >= WARMUP:
                    wall[on].append(dt)
                    for k in host[on]:
                        host[on][k].append(ht[k])
                if u == 0:
                    n3[on] = [int(pl.frame_landmarks(i, 0)["landmarks_flag"].sum()) for i in range(KF)]
        for on in (False, True):
            pls[on].close()
            res[on] = {"wall": med(wall[on]), "host": {k: med(v) for k, v in host[on].items()}, "landmarks": n3[on]}
    ctx.host_free(block)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_landmarks_timing.md"))
    ap.add_argument("--units", type=int, default=40)
    args = ap.parse_args()
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    kern = time_kernel(c, ctx)
    units = time_units(omni, ctx, args.units)
    ctx.close()
    gray, dep = KF * W * H, KF * W * H * 2
    lines = ["# PINHOLE_DEPTH: depth landmarks inside the key-frame unit against the host path", "",
             f"`tools/depth_landmarks_timing.py` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs).  Figures are recorded, not gated.", "",
             "## The kernel alone", "",
             f"`depth_landmarks_kernel`, HIP events around one launch on HBM-resident arrays: {KF} images x {MAX_NUM} key points, {W} x {H} depth images, median of {REPS} launches "
             f"after {WARMUP} warm-up launches outside the timed region.", "",
             "| lens | median us | min us | max us | landmarks set |", "|---|---|---|---|---|"]
    lines += [f"| {n} | {m:.1f} | {lo:.1f} | {hi:.1f} | {k} |" for n, m, lo, hi, k in kern]
    lines += ["", "## The upload", "",
              f"A unit of {KF} key frames uploads {gray} bytes of gray frames; with the switch on it uploads {dep} bytes of u16 depth frames more ({dep / gray:.0f} x the gray "
              f"frames' bytes: {(gray + dep) / gray:.0f} x the upload in all), plus {KF * 56} bytes of poses and {KF} have flags.  The copy's own time was not measured apart from "
              "the unit; the unit's wall time below contains it.", "",
              "## The unit", "",
              f"A PINHOLE_DEPTH pipeline (fp16, {W} x {H}, max_num {MAX_NUM}, micro-batch {KF}, 2 lanes, EuRoC-class PINHOLE lens, geometry on), `run()` of one unit of {KF} key frames "
              f"(`synth.depth_keyframe` places 0..{KF - 1}; landmarks per key frame: {units[True]['landmarks']}), the switch off and on in two pipelines of one process, alternating; "
              f"{args.units} timed units each after {WARMUP} warm-up units.  `run()` returns with the unit's detector step and geometry collected, so its wall time is the unit's "
              "whole latency on an otherwise idle GPU.  `host_times()` is the calling thread's time per unit; `messages` is finish()'s message building, which on the host path "
              "holds `fill_image_descriptor` (one f64 lift per key point) and `fill_depth_landmarks` (a second lift per accepted point).  Milliseconds: median (min .. max).", "",
              "| switch | run() wall | enqueue | wait_gpu | messages | detector | geometry |", "|---|---|---|---|---|---|---|"]
    for on in (False, True):
        r = units[on]
        f = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
        lines.append(f"| {'on' if on else 'off'} | {f(r['wall'])} | " + " | ".join(f(r["host"][k]) for k in ("enqueue", "wait_gpu", "messages", "detector", "geometry")) + " |")
    d_msg = units[False]["host"]["messages"][0] - units[True]["host"]["messages"][0]
    d_wall = units[False]["wall"][0] - units[True]["wall"][0]
    d_enq = units[True]["host"]["enqueue"][0] - units[False]["host"]["enqueue"][0]
    lines += ["", f"Medians, off minus on: `messages` {d_msg:+.3f} ms per unit ({d_msg / KF * 1e3:+.1f} us per key frame), `run()` wall {d_wall:+.3f} ms; on minus off: `enqueue` "
              f"{d_enq:+.3f} ms (the depth frames' copy into the handle's pinned block and the larger upload's launch).  The landmark counts per key frame are equal on both paths: "
              f"{units[False]['landmarks'] == units[True]['landmarks']}."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
