"""The two fisheye remap kernels on the same 8 raw key-frame pairs (1280 x 1024, fov 235, views 600 wide), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o flatten -- python tools/flatten_trace.py run
    python tools/flatten_trace.py report OUT

run:    (a) flatten_remap_kernel, one launch per camera: all five views of the 8 frames (omni_flatten_enqueue_dev);
        (b) flatten_unit_kernel, one launch per camera: views 1..4, masked, inside a key-frame unit (omni_cam_enqueue_fisheye_dev).
report: the median launch time of each kernel from the trace's per-dispatch rows, and bytes/s against the algorithmic 13 B per computed output pixel
        (8 map + 4 gathered source + 1 output; the zero rows of (b) are counted as 1 B each)."""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEI = (1.8, -0.2, 0.05, 0.001, -0.002, 1100.0, 1098.0, 640.0, 512.0)
N_KF, SRC_W, SRC_H, VW, VH, REPS = 8, 1280, 1024, 600, 312, 30
PX_A = N_KF * (VW * VW + 4 * VW * VH)                         # computed pixels per launch (one camera)
PX_B, ZERO_B = N_KF * 4 * VW * (VH * 3 // 4), N_KF * 4 * VW * (VH - VH * 3 // 4)


def run():
    import omni_loader
    omni = omni_loader.load()
    from omni_swarm_amd import flatten, frontend, synth
    from oracle import mobilenetvlad_ref as V          # (weights only: the networks run behind (b), their kernels are not what is measured)
    from oracle import superpoint_ref as S
    c = omni.capi
    ctx = c.Context(0)
    fl = [c.Flatten(ctx, SRC_W, SRC_H, flatten.generate_undist_maps(MEI, VW, 235.0, cam_id)) for cam_id in (0, 1)]
    raw = [ctx.to_device(np.stack([synth.image_u8(7000 + 10 * cam + k, SRC_H, SRC_W, n_shapes=400) for k in range(N_KF)])) for cam in range(2)]
    out = ctx.alloc(fl[0].out_bytes * N_KF)
    comp, mean = synth.pca()
    lc = frontend.LoopCam(ctx, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), VW, VH, 0.015, 200,
                          c.PREC_F16, n_dirs=4 * N_KF)
    for _ in range(REPS):                                  # alternating, so that both see the same machine
        for cam in range(2):
            fl[cam].enqueue_dev(raw[cam], SRC_W, N_KF, out)
        ctx.sync()
        lc.cam.enqueue_fisheye_dev(fl[0], fl[1], raw[0], raw[1], SRC_W, N_KF, 1, True)
        lc.cam.wait()
    lc.close()
    print("flatten_trace: done")


def report(d):
    files = [f for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)]
    assert files, f"no *kernel_trace.csv under {d}"
    t = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            for k in ("flatten_remap_kernel", "flatten_unit_kernel"):
                if k in r["Kernel_Name"]:
                    t.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for k, px, extra in (("flatten_remap_kernel", PX_A, 0), ("flatten_unit_kernel", PX_B, ZERO_B)):
        us = np.sort(np.array(t[k][4:]))                   # (the first two rounds: code-object load, cold maps)
        med = float(np.median(us))
        print(f"{k}: {len(us)} launches, median {med:.1f} us (min {us[0]:.1f}, p90 {us[int(0.9 * len(us))]:.1f}); {px} computed pixels -> "
              f"{(13 * px + extra) / med * 1e-6:.3f} TB/s of algorithmic bytes, {med * 1e3 / px:.4f} ns per computed pixel")
    a, b = (float(np.median(t[k][4:])) for k in ("flatten_remap_kernel", "flatten_unit_kernel"))
    print(f"unit / remap per launch: {b / a:.3f} (computed pixels: {PX_B / PX_A:.3f})")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else report(sys.argv[2])
