#!/usr/bin/env python3
"""Times the stereo-landmark kernel alone (csrc/landmarks.hip through omni_landmarks_enqueue_dev_camera) with and without a lens model: HIP events around one
launch on HBM-resident arrays, 32 image pairs x 200 key points x 200 matches, medians of 20 with the warm-up outside the timed region.  Cameras: the ideal
pinhole, a PINHOLE with EuRoC-class distortion (eight undistortion rounds per lift) and an MEI model (six rounds, one square root, one division more).

    python tools/landmarks_camera_timing.py [--out profiles/landmarks_camera_timing.md]

Records figures; gates nothing."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omni_loader  # noqa: E402

PAIRS, MAX_NUM, REPS, WARMUP = 32, 200, 20, 5
CAMERAS = {                                             # name -> (type, k1, k2, p1, p2, xi, focal)
    "ideal": ("PINHOLE", 0.0, 0.0, 0.0, 0.0, 0.0, 300.0),
    "euroc": ("PINHOLE", -0.2917, 0.08228, 5.333e-5, -1.578e-4, 0.0, 300.0),
    "mei": ("MEI", -0.05, 0.01, 1e-3, -1e-3, 1.2, 620.0),
}


def inputs(seed=0):
    """a forward stereo pair 10 cm apart, scene points 1..8 m away seen at whole pixels: every key point matched (the stage's largest unit of work)"""
    rng = np.random.default_rng(seed)
    kps = np.zeros((2 * PAIRS, MAX_NUM, 2), np.float32)
    for p in range(PAIRS):
        x, y, z = rng.integers(80, 560, MAX_NUM), rng.integers(40, 440, MAX_NUM), rng.uniform(1.0, 8.0, MAX_NUM)
        kps[p] = np.stack([x, y], 1)
        kps[PAIRS + p] = np.stack([np.rint(x - 300.0 * 0.10 / z), y + rng.integers(-1, 2, MAX_NUM)], 1)
    idx = np.stack([rng.permutation(MAX_NUM) for _ in range(PAIRS)]).astype(np.int32)
    poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (PAIRS, 1))
    return poses, kps, np.full(2 * PAIRS, MAX_NUM, np.int32), idx, idx.copy(), np.full(PAIRS, MAX_NUM, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmarks_camera_timing.md"))
    args = ap.parse_args()
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    ins = inputs()
    outs = [((2 * PAIRS, MAX_NUM, 2), np.float32), ((2 * PAIRS, MAX_NUM, 3), np.float32), ((2 * PAIRS, MAX_NUM), np.uint8), ((PAIRS,), np.int32)]
    dev = [ctx.to_device(a) for a in ins] + [ctx.alloc(int(np.prod(s)) * np.dtype(d).itemsize) for s, d in outs]
    rows = []
    try:
        for name, (typ, k1, k2, p1, p2, xi, f) in CAMERAS.items():
            model = c.stereo_model(f, f, 300.0, 240.0, 0.006, 50, [[0, 0, 0, 1, 0, 0, 0]], [[0.10, 0, 0, 1, 0, 0, 0]])
            cam = None if name == "ideal" else c.camera_model(typ, k1, k2, p1, p2, xi)
            for _ in range(WARMUP):
                c.landmarks_dev(ctx, model, dev[0], PAIRS, MAX_NUM, *dev[1:], camera=cam, camera_entry=True)
            ctx.sync()
            ms = []
            for _ in range(REPS):
                ctx.timer_start()
                c.landmarks_dev(ctx, model, dev[0], PAIRS, MAX_NUM, *dev[1:], camera=cam, camera_entry=True)
                ms.append(ctx.timer_stop())
            count = ctx.from_device(dev[9], (PAIRS,), np.int32)
            rows.append((name, typ, float(np.median(ms)) * 1e3, float(np.min(ms)) * 1e3, float(np.max(ms)) * 1e3, int(count.sum())))
    finally:
        for d in dev:
            ctx.free(d)
    info = ctx.device_info()
    ctx.close()
    lines = ["# Stereo-landmark kernel with a lens model: time of one launch", "",
             f"`tools/landmarks_camera_timing.py` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs): `landmarks_kernel` alone, HIP events around one launch, {PAIRS} pairs x {MAX_NUM} key points x {MAX_NUM} matches "
             f"(every key point matched), median of {REPS} launches after {WARMUP} warm-up launches outside the timed region.  Figures are recorded, not gated.", "",
             "| camera | type | median us | min us | max us | landmarks kept |", "|---|---|---|---|---|---|"]
    lines += [f"| {n} | {t} | {med:.1f} | {lo:.1f} | {hi:.1f} | {k} |" for n, t, med, lo, hi, k in rows]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
