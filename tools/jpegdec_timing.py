"""Times the JPEG decode stage (csrc/jpeg_dec.hip) for one key-frame unit's worth of camera frames -- 16 frames of 640 x 480 -- and writes profiles/r10_jpegdec.md:
  (a) the stage on the GPU: upload and memsets + kernels, from the handle's own events (omni_jpegdec_last_ms), per subsequence length S of a sweep;
  (b) omni_jpeg_decode_host on ONE host thread for the same frames;
  (c) the bytes the stage uploads against the raw unit's 16 x 640 x 480;
  (d) relaxation rounds to the fixed point and subsequences per frame at every S.
Also: the calling thread's share (parse + unstuff + pack) per unit.  The frames are synthetic camera-like pictures (omni_swarm_amd.synth), encoded with the
project's own encoder at quality 75 and 95.
    python tools/jpegdec_timing.py [--out profiles/r10_jpegdec.md] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omni_loader  # noqa: E402

S_SWEEP = [256, 512, 1024, 2048, 4096, 8192, 16384]
S_ENV = "OMNI_JPEGDEC_SUBSEQ_BITS"
W, H, N = 640, 480, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_jpegdec.md"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    omni = omni_loader.load()
    c = omni.capi
    from omni_swarm_amd import synth
    ctx = c.Context(0)
    frames = [synth.image_u8(4100 + i, H, W, n_shapes=120) for i in range(N)]
    default = c.config_value(S_ENV)
    info = ctx.device_info()
    name = info["name"].strip()
    if not name or name.startswith("("):                       # the runtime gives some boards no marketing name, only " (gfx950:...)": say so, keep what it gave
        name = f"no marketing name from the runtime [{info['name'].strip()}]"
    lines = ["# JPEG decode stage: one unit of 16 frames of 640 x 480", "", f"device: {name} ({info['n_cu']} CUs, {info['clock_mhz']} MHz); {a.reps} repetitions, medians; "
             f"default {S_ENV} = {default}; sweep {S_SWEEP}", ""]
    out = ctx.alloc(N * W * H)
    stat = ctx.alloc(4 * N)
    for q in (75, 95):
        files = []
        for g in frames:
            st, data = c.jpeg_encode_host(g, q)
            assert st == c.JPEG_OK
            files.append(data)
        ref = [c.jpeg_decode_host(f)[1] for f in files]
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            for f in files:
                c.jpeg_decode_host(f)
            t.append((time.perf_counter() - t0) * 1e3)
        host_ms = float(np.median(t))
        total = sum(len(f) for f in files)
        lines += [f"## quality {q}", "", f"files: {total} bytes for the unit ({total // N} per frame); raw unit: {N * W * H} bytes", "",
                  f"(b) omni_jpeg_decode_host, one thread, 16 frames (through ctypes, allocation included): {host_ms:.2f} ms", "",
                  "| S (bits) | subsequences / frame | rounds (max over frames) | upload ms | memsets + kernels ms | calling thread ms | uploaded bytes | vs raw |",
                  "|---|---|---|---|---|---|---|---|"]
        for S in S_SWEEP:
            os.environ[S_ENV] = str(S)
            dec = c.JpegDec(ctx, W, H, N, 256 * 1024)
            up, ker, call = [], [], []
            for r in range(a.reps + 2):
                t0 = time.perf_counter()
                dec.enqueue_host(files, out, W, stat)
                t1 = time.perf_counter()
                u, k, nbytes = dec.last_ms()
                if r >= 2:
                    up.append(u), ker.append(k), call.append((t1 - t0) * 1e3)
            stats = dec.last_stats(N)
            got = ctx.from_device(out, (N, H, W), np.uint8)
            status = ctx.from_device(stat, (N,), np.int32)
            assert (status == c.JPEGDEC_OK).all() and all(np.array_equal(got[i], ref[i]) for i in range(N)), (q, S)
            dec.close()
            lines.append(f"| {S} | {int(np.mean([s[1] for s in stats]))} | {max(s[0] for s in stats)} | {np.median(up):.3f} | {np.median(ker):.3f} | {np.median(call):.3f} | "
                         f"{nbytes} | {nbytes / (N * W * H):.3f} |")
        os.environ.pop(S_ENV, None)
        lines.append("")
    ctx.free(out)
    ctx.free(stat)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
