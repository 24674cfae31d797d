"""Times the JPEG decode stage (csrc/jpeg_dec.hip) on restart-interval files and writes profiles/jpegdec_restart_timing.md: 16 frames of 1280 x 1024 at quality
75 and 95, every picture
  (a) as a file without restart markers: today's kernel path, one workgroup of the entropy kernel per picture -- the baseline;
  (b) as a restart_marker_rows=1 file with OMNI_JPEGDEC_RESTART_WGS = 0: decoded on the calling thread, its pixels uploaded;
  (c) as the same restart file with the switch at W in {1, 2, 4, 8, 16}: its intervals spread over at most W workgroups.
Reported: memsets + kernels from the handle's own events (omni_jpegdec_last_ms), the upload, and beside them the calling thread's time in the enqueue (parse,
unstuff, plan, pack -- and for (b) the host decode).  Every run's pixels are compared with the host decoder's.  The frames are synthetic camera-like pictures
(omni_swarm_amd.synth) written by Pillow, which is only needed to make the files:
    python tools/jpegdec_restart_timing.py --make-frames frames.npz          (needs Pillow, no GPU)
    python tools/jpegdec_restart_timing.py --frames frames.npz [--out profiles/jpegdec_restart_timing.md] [--reps 20]
Without --frames the files are made on the spot."""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omni_loader  # noqa: E402

W_SWEEP = [1, 2, 4, 8, 16]
W_ENV = "OMNI_JPEGDEC_RESTART_WGS"
W, H, N = 1280, 1024, 16
QUALITIES = (75, 95)


def make_frames() -> dict:
    """{"plain_q<q>_<i>" / "rows_q<q>_<i>": the file's bytes}"""
    from PIL import Image
    omni_loader.load()
    from omni_swarm_amd import synth
    out = {}
    for i in range(N):
        im = Image.fromarray(synth.image_u8(4100 + i, H, W, n_shapes=120), "L")
        for q in QUALITIES:
            for kind, save in (("plain", {}), ("rows", dict(restart_marker_rows=1))):
                b = io.BytesIO()
                im.save(b, "JPEG", quality=q, **save)
                out[f"{kind}_q{q}_{i}"] = np.frombuffer(b.getvalue(), np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegdec_restart_timing.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--make-frames", default=None)
    a = ap.parse_args()
    if a.make_frames:
        np.savez(a.make_frames, **make_frames())
        print(f"{a.make_frames}: {os.path.getsize(a.make_frames)} bytes")
        return
    if a.frames:
        with np.load(a.frames) as z:
            frames = {k: z[k] for k in z.files}
    else:
        frames = make_frames()
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    name = info["name"].strip()
    if not name or name.startswith("("):
        name = f"no marketing name from the runtime [{info['name'].strip()}]"
    lines = [f"# JPEG decode stage on restart-interval files: {N} frames of {W} x {H}", "",
             f"device: {name} ({info['n_cu']} CUs, {info['clock_mhz']} MHz); {a.reps} repetitions, medians; OMNI_JPEGDEC_SUBSEQ_BITS = "
             f"{c.config_value('OMNI_JPEGDEC_SUBSEQ_BITS')}; restart files: one interval per MCU row ({H // 8} intervals)", ""]
    out = ctx.alloc(N * W * H)
    stat = ctx.alloc(4 * N)
    for q in QUALITIES:
        plain = [frames[f"plain_q{q}_{i}"].tobytes() for i in range(N)]
        rows = [frames[f"rows_q{q}_{i}"].tobytes() for i in range(N)]
        ref = [c.jpeg_decode_host(f)[1] for f in plain]
        assert all(np.array_equal(c.jpeg_decode_host(f)[1], r) for f, r in zip(rows, ref))          # the markers change no pixel
        lines += [f"## quality {q}", "", f"files without markers: {sum(map(len, plain)) // N} bytes per frame; with: {sum(map(len, rows)) // N}", "",
                  "| files | switch | status | chunks / frame | subsequences / frame | rounds (max) | upload ms | memsets + kernels ms | calling thread ms |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for label, files, Wv, want in [("no restart markers (baseline)", plain, 0, c.JPEGDEC_OK), ("restart rows=1", rows, 0, c.JPEGDEC_HOST)] + \
                                      [("restart rows=1", rows, v, c.JPEGDEC_OK) for v in W_SWEEP]:
            os.environ[W_ENV] = str(Wv)
            dec = c.JpegDec(ctx, W, H, N)
            up, ker, call = [], [], []
            for r in range(a.reps + 2):
                t0 = time.perf_counter()
                dec.enqueue_host(files, out, W, stat)
                t1 = time.perf_counter()
                u, k, _ = dec.last_ms()
                if r >= 2:
                    up.append(u), ker.append(k), call.append((t1 - t0) * 1e3)
            stats, chunks = dec.last_stats(N), dec.last_chunks(N)
            got = ctx.from_device(out, (N, H, W), np.uint8)
            status = ctx.from_device(stat, (N,), np.int32)
            assert (status == want).all() and all(np.array_equal(got[i], ref[i]) for i in range(N)), (q, label, Wv, status)
            dec.close()
            lines.append(f"| {label} | {Wv} | {'OK' if want == c.JPEGDEC_OK else 'HOST'} | {np.mean(chunks):.1f} | {int(np.mean([s[1] for s in stats]))} | {max(s[0] for s in stats)} | "
                         f"{np.median(up):.3f} | {np.median(ker):.3f} | {np.median(call):.3f} |")
        os.environ.pop(W_ENV, None)
        lines.append("")
    ctx.free(out)
    ctx.free(stat)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
