"""Times the JPEG decode stage (csrc/jpeg_dec.hip) with OMNI_JPEGDEC_UNSTUFF_DEV off and on and writes profiles/jpegdec_unstuff_timing.md: 16 frames of 1280 x 1024
at quality 75 and 95 (the frames of tools/jpegdec_restart_timing.py), as files without restart markers (W = OMNI_JPEGDEC_PLAIN_WGS) and with one restart interval
per MCU row (W = OMNI_JPEGDEC_RESTART_WGS), W in {0, 16}.
  switch 0   the calling thread unstuffs every scan byte by byte into the pinned block; the clean scans are uploaded;
  switch 1   it surveys the 0xFF bytes (memchr) and copies the raw scans; they are uploaded as they are and jpegdec_unstuff_kernel compacts them.
The four handles of one kind of file are made once and take turns, repetition by repetition, in this one process; medians of --reps.  Per row: the calling
thread's time inside the enqueue call (perf_counter), the upload and memsets + kernels from the handle's own events (omni_jpegdec_last_ms; the unstuff kernel
counts among the kernels), the bytes uploaded.  Every configuration's pixels are compared with the host decoder's.
--unit runs tools/fisheye_intake_timing.py (the key-frame unit fed fisheye files of quality 75 / 95) in processes of their own with OMNI_JPEGDEC_PLAIN_WGS=16,
the switch off and on, alternated --unit-rounds times, and adds the unit's time on the SuperPoint stream.
    python tools/jpegdec_restart_timing.py --make-frames frames.npz          (needs Pillow, no GPU)
    python tools/jpegdec_unstuff_timing.py --frames frames.npz [--unit] [--out profiles/jpegdec_unstuff_timing.md] [--reps 20]
Without --frames the files are made on the spot (Pillow)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omni_loader  # noqa: E402

U_ENV, P_ENV, R_ENV = "OMNI_JPEGDEC_UNSTUFF_DEV", "OMNI_JPEGDEC_PLAIN_WGS", "OMNI_JPEGDEC_RESTART_WGS"
W, H, N = 1280, 1024, 16
QUALITIES = (75, 95)
CONFIGS = [(0, 0), (0, 1), (16, 0), (16, 1)]                   # (W, switch)


def load_frames(path):
    if path:
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jpegdec_restart_timing
    return jpegdec_restart_timing.make_frames()


def time_kind(c, ctx, out, stat, files, ref, w_env, reps):
    """the four handles of CONFIGS on one list of files, taking turns -> [dict of medians] in CONFIGS' order"""
    decs = []
    for Wv, sw in CONFIGS:
        os.environ[w_env], os.environ[U_ENV] = str(Wv), str(sw)
        decs.append(c.JpegDec(ctx, W, H, N))
    os.environ.pop(w_env, None)
    os.environ.pop(U_ENV, None)
    t = [dict(up=[], ker=[], call=[]) for _ in CONFIGS]
    for r in range(reps + 2):
        for k, dec in enumerate(decs):
            t0 = time.perf_counter()
            dec.enqueue_host(files, out, W, stat)
            t1 = time.perf_counter()
            u, ker, nbytes = dec.last_ms()
            if r >= 2:
                t[k]["up"].append(u), t[k]["ker"].append(ker), t[k]["call"].append((t1 - t0) * 1e3)
            t[k]["bytes"] = nbytes
    rows = []
    for k, dec in enumerate(decs):
        dec.enqueue_host(files, out, W, stat)
        got, status = ctx.from_device(out, (N, H, W), np.uint8), ctx.from_device(stat, (N,), np.int32)
        assert all(np.array_equal(got[i], ref[i]) for i in range(N)) and len(set(status.tolist())) == 1, (CONFIGS[k], status)
        pictures, raw, clean = dec.last_unstuff()
        rows.append(dict(status={c.JPEGDEC_OK: "OK", c.JPEGDEC_HOST: "HOST"}[int(status[0])], call=float(np.median(t[k]["call"])), up=float(np.median(t[k]["up"])),
                         ker=float(np.median(t[k]["ker"])), bytes=t[k]["bytes"], pictures=pictures, raw=raw, clean=clean))
        dec.close()
    return rows


def unit_rows(rounds, reps):
    """tools/fisheye_intake_timing.py with OMNI_JPEGDEC_PLAIN_WGS=16, the switch off and on, processes of their own -> [(switch, round, {quality: unit ms})]"""
    out = []
    for r in range(rounds):
        for sw in (0, 1)[::1 if r % 2 == 0 else -1]:
            env = dict(os.environ)
            env[P_ENV], env[U_ENV] = "16", str(sw)
            with tempfile.TemporaryDirectory() as td:
                path = os.path.join(td, "unit.md")
                p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fisheye_intake_timing.py"), "--out", path, "--reps", str(reps)], env=env, capture_output=True,
                                   text=True, timeout=900)
                assert p.returncode == 0, (sw, p.returncode, p.stderr[-2000:])
                text = open(path).read()
            ms = {q: float(re.search(rf"^\| jpeg q{q} \| \d+ \| ([0-9.]+) \|", text, re.M).group(1)) for q in QUALITIES}
            out.append((sw, r, ms))
            print(f"unit, switch {sw}, run {r + 1}: {ms}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegdec_unstuff_timing.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--unit", action="store_true")
    ap.add_argument("--unit-rounds", type=int, default=2)
    a = ap.parse_args()
    unit = unit_rows(a.unit_rounds, a.reps) if a.unit else []                                  # processes of their own, before this one opens the GPU
    frames = load_frames(a.frames)
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    name = info["name"].strip()
    if not name or name.startswith("("):
        name = f"no marketing name from the runtime [{info['name'].strip()}]"
    lines = [f"# JPEG decode stage, OMNI_JPEGDEC_UNSTUFF_DEV off and on: {N} frames of {W} x {H}", "",
             f"device: {name} ({info['n_cu']} CUs, {info['clock_mhz']} MHz); {a.reps} repetitions, medians, the four handles of a table taking turns; "
             f"OMNI_JPEGDEC_SUBSEQ_BITS = {c.config_value('OMNI_JPEGDEC_SUBSEQ_BITS')}", ""]
    out = ctx.alloc(N * W * H)
    stat = ctx.alloc(4 * N)
    for q in QUALITIES:
        for kind, w_env, label in (("plain", P_ENV, "files without restart markers, W = OMNI_JPEGDEC_PLAIN_WGS"),
                                   ("rows", R_ENV, f"files with one restart interval per MCU row ({H // 8 - 1} markers), W = OMNI_JPEGDEC_RESTART_WGS")):
            files = [frames[f"{kind}_q{q}_{i}"].tobytes() for i in range(N)]
            ref = [c.jpeg_decode_host(f)[1] for f in files]
            rows = time_kind(c, ctx, out, stat, files, ref, w_env, a.reps)
            lines += [f"## quality {q}, {label}", "", f"{sum(map(len, files)) // N} bytes per frame", "",
                      "| W | switch | status | calling thread ms | upload ms | memsets + kernels ms | bytes uploaded | scans unstuffed on the device | their raw bytes | their clean bytes |",
                      "|---|---|---|---|---|---|---|---|---|---|"]
            for (Wv, sw), m in zip(CONFIGS, rows):
                lines.append(f"| {Wv} | {sw} | {m['status']} | {m['call']:.3f} | {m['up']:.3f} | {m['ker']:.3f} | {m['bytes']} | {m['pictures']} | {m['raw']} | {m['clean']} |")
            lines.append("")
    ctx.free(out)
    ctx.free(stat)
    if unit:
        lines += ["## the key-frame unit fed fisheye files (tools/fisheye_intake_timing.py), OMNI_JPEGDEC_PLAIN_WGS = 16", "",
                  f"the unit on the SuperPoint stream, ms, medians of {a.reps} units; processes of their own, alternated", "",
                  "| switch | run | files of quality 75 | files of quality 95 |", "|---|---|---|---|"]
        for sw, r, ms in unit:
            lines.append(f"| {sw} | {r + 1} | {ms[75]:.3f} | {ms[95]:.3f} |")
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
