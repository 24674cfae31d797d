"""The resize kernel on the raw frames of a unit of 8 stereo-pinhole key frames (16 frames of 752 x 480 -> 600 x 480), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o resize -- python tools/resize_trace.py run
    python tools/resize_trace.py report OUT

run:    omni_resize_enqueue_dev on the 16 frames, REPS launches; then, for scale, the upload of the same 16 frames from pinned host memory (one blocking
        copy, timed on the host) -- printed, and written to OUT_H2D (an environment variable naming a file) when that is set.
report: the median launch time of resize_kernel from the trace's per-dispatch rows, and bytes/s against the algorithmic bytes per destination pixel
        (1 output + 4 gathered source bytes; the tables, 10 KB, stay in cache)."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, SRC_W, SRC_H, W, H, REPS = 16, 752, 480, 600, 480, 40


def run():
    import omni_loader
    omni = omni_loader.load()
    from omni_swarm_amd import synth
    c = omni.capi
    ctx = c.Context(0)
    pinned = ctx.host_alloc((N, SRC_H, SRC_W), np.uint8)
    pinned[:] = np.stack([synth.image_u8(7300 + k, SRC_H, SRC_W, n_shapes=200) for k in range(N)])
    rs = c.Resize(ctx, SRC_W, SRC_H, W, H)
    src, out = ctx.to_device(pinned), ctx.alloc(N * W * H)
    for _ in range(REPS):
        rs.enqueue_dev(src, SRC_W, N, out)
        ctx.sync()
    h2d = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c._check(c.lib().omni_memcpy_h2d(ctx.h, src, pinned.ctypes.data_as(c._vp), pinned.nbytes))
        h2d.append((time.perf_counter() - t0) * 1e6)
    h2d = np.sort(np.array(h2d[4:]))
    line = (f"h2d of {N} frames {SRC_W}x{SRC_H} ({pinned.nbytes / 1e6:.2f} MB) from pinned memory: median {np.median(h2d):.1f} us (min {h2d[0]:.1f}) = "
            f"{pinned.nbytes / np.median(h2d) * 1e-3:.1f} GB/s")
    print(line)
    if os.environ.get("OUT_H2D"):
        open(os.environ["OUT_H2D"], "w").write(line + "\n")
    rs.close()
    ctx.free(src); ctx.free(out); ctx.host_free(pinned)
    ctx.close()
    print("resize_trace: done")


def report(d):
    files = [f for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)]
    assert files, f"no *kernel_trace.csv under {d}"
    us = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "resize_kernel" in r["Kernel_Name"]:
                us.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    us = np.sort(np.array(us[4:]))                         # (the first launches: code-object load, cold tables)
    med, px = float(np.median(us)), N * W * H
    print(f"resize_kernel: {len(us)} launches, median {med:.1f} us (min {us[0]:.1f}, p90 {us[int(0.9 * len(us))]:.1f}); {px} destination pixels -> "
          f"{5 * px / med * 1e-6:.3f} TB/s of algorithmic bytes, {med * 1e3 / px:.4f} ns per pixel")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else report(sys.argv[2])
