"""Times the JPEG decode stage (csrc/jpeg_dec.hip) on files WITHOUT restart markers with OMNI_JPEGDEC_PLAIN_WGS = W in {0, 1, 2, 4, 8, 16, 32} and writes
profiles/jpegdec_plain_timing.md: 16 frames of 1280 x 1024 at quality 75 and 95 (the frames of tools/jpegdec_restart_timing.py, its "plain" files).
  W = 0, 1   one workgroup of the entropy kernel per picture;
  W >= 2     a picture's subsequences over min(W, n_sub) workgroups of the chunk kernel, the seam kernel, the write kernel.
Reported per W, medians of --reps runs: chunks per frame, subsequences, rounds, seam rounds, the upload and memsets + kernels from the handle's own events
(omni_jpegdec_last_ms), and the calling thread's time in the enqueue (parse, unstuff, pack).  Every run's pixels are compared with the host decoder's.
A second table per quality: OMNI_JPEGDEC_SUBSEQ_BITS below its default at W in {16, 32} -- a spread picture keeps short subsequences (jpeg_dec_plan.h,
plain_subseq_bits), and every kernel of the path takes about as long as ONE lane needs for its subsequences.
--parent-tree names a built checkout of the PARENT commit (omni_loader.py, omni-swarm_amd/ and its lib/ are all it needs): the switch-off path of both trees is
then timed on the same files in processes of their own, alternated --ab-rounds times on this one box (which of the two goes first alternates too), and both
ranges are written down (the parent knows no switch: the variable is unset in both).
    python tools/jpegdec_restart_timing.py --make-frames frames.npz          (needs Pillow, no GPU)
    python tools/jpegdec_plain_timing.py --frames frames.npz [--parent-tree DIR] [--out profiles/jpegdec_plain_timing.md] [--reps 20]
Without --frames the files are made on the spot (Pillow)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else ROOT      # (the A/B's child: the tree whose package and library are timed)
sys.path.insert(0, TREE)
import omni_loader  # noqa: E402

W_SWEEP = [0, 1, 2, 4, 8, 16, 32]
S_SWEEP = [(256, 16), (256, 32), (512, 16), (512, 32)]          # (OMNI_JPEGDEC_SUBSEQ_BITS, W) of the second table
W_ENV, S_ENV = "OMNI_JPEGDEC_PLAIN_WGS", "OMNI_JPEGDEC_SUBSEQ_BITS"
W, H, N = 1280, 1024, 16
QUALITIES = (75, 95)


def load_frames(path):
    if path:
        with np.load(path) as z:
            return {k: z[k] for k in z.files if k.startswith("plain_")}
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jpegdec_restart_timing
    return {k: v for k, v in jpegdec_restart_timing.make_frames().items() if k.startswith("plain_")}


def time_one(c, ctx, out, stat, files, ref, Wv, reps, S=None):
    """one handle created with the switch at Wv (None: the variable unset) and S bits per subsequence (None: the default) -> dict of medians and statistics"""
    if Wv is None:
        os.environ.pop(W_ENV, None)
    else:
        os.environ[W_ENV] = str(Wv)
    if S:
        os.environ[S_ENV] = str(S)
    dec = c.JpegDec(ctx, W, H, N)
    up, ker, call = [], [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        dec.enqueue_host(files, out, W, stat)
        t1 = time.perf_counter()
        u, k, _ = dec.last_ms()
        if r >= 2:
            up.append(u), ker.append(k), call.append((t1 - t0) * 1e3)
    stats, chunks = dec.last_stats(N), dec.last_chunks(N)
    seam = dec.last_seam(N) if hasattr(dec, "last_seam") else [(0, 0)] * N
    got = ctx.from_device(out, (N, H, W), np.uint8)
    status = ctx.from_device(stat, (N,), np.int32)
    assert (status == c.JPEGDEC_OK).all() and all(np.array_equal(got[i], ref[i]) for i in range(N)), (Wv, status)
    dec.close()
    os.environ.pop(W_ENV, None)
    os.environ.pop(S_ENV, None)
    return dict(chunks=float(np.mean(chunks)), n_sub=int(np.mean([s[1] for s in stats])), bits=max(s[2] for s in stats), rounds=max(s[0] for s in stats),
                seam_rounds=max(s[0] for s in seam), upload=float(np.median(up)), kernels=float(np.median(ker)), call=float(np.median(call)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegdec_plain_timing.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=None, help="(the A/B's child) the tree to time instead of this one")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--switch-off-json", action="store_true", help="(the A/B's child) time the switch-off path alone and print one JSON line")
    a = ap.parse_args()
    ab = []
    if a.parent_tree and not a.switch_off_json:                                                # processes of their own, before this one opens the GPU
        for r in range(a.ab_rounds):
            for which, tree in [("parent", os.path.abspath(a.parent_tree)), ("this tree", ROOT)][::1 if r % 2 == 0 else -1]:
                env = dict(os.environ)
                env.pop("OMNI_LIB", None)
                env.pop(W_ENV, None)
                env.pop(S_ENV, None)
                cmd = [sys.executable, os.path.abspath(__file__), "--switch-off-json", "--tree", tree, "--reps", str(a.reps)] + (["--frames", a.frames] if a.frames else [])
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, (which, p.returncode, p.stderr[-2000:])
                ab.append((which, r, json.loads(p.stdout.strip().splitlines()[-1])))
    frames = load_frames(a.frames)
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    out = ctx.alloc(N * W * H)
    stat = ctx.alloc(4 * N)
    per_q = {}
    for q in QUALITIES:
        files = [frames[f"plain_q{q}_{i}"].tobytes() for i in range(N)]
        ref = [c.jpeg_decode_host(f)[1] for f in files]
        sweep = [None] if a.switch_off_json else W_SWEEP
        per_q[q] = (sum(map(len, files)) // N, [(Wv, time_one(c, ctx, out, stat, files, ref, Wv, a.reps)) for Wv in sweep],
                    [] if a.switch_off_json else [(S, Wv, time_one(c, ctx, out, stat, files, ref, Wv, a.reps, S)) for S, Wv in S_SWEEP])
    info = ctx.device_info()
    ctx.free(out)
    ctx.free(stat)
    if a.switch_off_json:
        print(json.dumps({str(q): per_q[q][1][0][1]["kernels"] for q in QUALITIES}))
        return
    name = info["name"].strip()
    if not name or name.startswith("("):
        name = f"no marketing name from the runtime [{info['name'].strip()}]"
    lines = [f"# JPEG decode stage on files without restart markers, OMNI_JPEGDEC_PLAIN_WGS = W: {N} frames of {W} x {H}", "",
             f"device: {name} ({info['n_cu']} CUs, {info['clock_mhz']} MHz); {a.reps} repetitions, medians; OMNI_JPEGDEC_SUBSEQ_BITS = "
             f"{c.config_value('OMNI_JPEGDEC_SUBSEQ_BITS')}", ""]
    for q in QUALITIES:
        size, rows, short = per_q[q]
        base = rows[0][1]["kernels"]
        lines += [f"## quality {q}", "", f"{size} bytes per frame", "",
                  "| W | chunks / frame | subsequences / frame | bits / subsequence | rounds (max) | seam rounds (max) | upload ms | memsets + kernels ms | against W = 0 | calling thread ms |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for Wv, m in rows:
            note = "" if Wv == 0 else f"{m['kernels'] / base:.2f}x" + (" (SLOWER)" if m["kernels"] > base * 1.02 else "")
            lines.append(f"| {Wv} | {m['chunks']:.1f} | {m['n_sub']} | {m['bits']} | {m['rounds']} | {m['seam_rounds']} | {m['upload']:.3f} | {m['kernels']:.3f} | {note} | {m['call']:.3f} |")
        lines += ["", "shorter subsequences (OMNI_JPEGDEC_SUBSEQ_BITS as asked for; the row's own `bits / subsequence` is what the picture was decoded with):", "",
                  "| OMNI_JPEGDEC_SUBSEQ_BITS | W | chunks / frame | subsequences / frame | bits / subsequence | rounds (max) | seam rounds (max) | memsets + kernels ms | against W = 0 | calling thread ms |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for S, Wv, m in short:
            lines.append(f"| {S} | {Wv} | {m['chunks']:.1f} | {m['n_sub']} | {m['bits']} | {m['rounds']} | {m['seam_rounds']} | {m['kernels']:.3f} | {m['kernels'] / base:.2f}x | {m['call']:.3f} |")
        lines.append("")
    if ab:
        lines += ["## the switch-off path against the parent commit's library", "",
                  f"memsets + kernels ms, the variable unset, medians of {a.reps}; processes of their own, alternated {a.ab_rounds} times on this one box", "",
                  "| library | run | quality 75 | quality 95 |", "|---|---|---|---|"]
        for which, r, m in ab:
            lines.append(f"| {which} | {r + 1} | {m['75']:.3f} | {m['95']:.3f} |")
        lines.append("")
        for q in QUALITIES:
            rng = {w: [m[str(q)] for ww, _, m in ab if ww == w] for w in ("parent", "this tree")}
            lines.append(f"quality {q}: parent {min(rng['parent']):.3f} .. {max(rng['parent']):.3f} ms, this tree {min(rng['this tree']):.3f} .. {max(rng['this tree']):.3f} ms")
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
