#!/usr/bin/env python3
"""Times the pairwise-consistency stage of the loop edges (csrc/pcm.hip, csrc/pcm_plan.h, host/loop_outlier_rejection.hpp; KeyframePipeline(..., pcm=True)) on one
commit:

  rows      omni_pcm_add with 8 new edges against 256 / 1 024 / 4 096 held ones: the device time between two events around the four launches and the wall time of
            the call (upload, launches, download), median of 10 calls after 3 warm-up calls (the handle grows by 8 edges per call), the returned rows compared bit
            for bit with omni_pcm_rows_host; next to it omni_pcm_rows_host for the same 8 edges on one thread of the same machine;
  clique    omni_pcm_max_clique_host at those sizes on an all-consistent graph and on a half-consistent one (every pair consistent with probability 1/2), median
            of 5 calls;
  bench     `bench.py --gpus 1 --steps 200 --warmup 20` of this tree (the switch is off: bench.py does not know it) alternated with the same command in a build
            of the parent commit (--parent DIR), --bench-reps times each; a difference of the medians below three times the parent's own spread (half of max - min)
            is reported as not resolved;
  stream    the bench-shaped STEREO_FISHEYE pipeline with the geometry stage (fp16, 600 x 480, max_num 200, micro-batch 8, 1 000 key frames pre-loaded, 32 rendered
            rooms again and again: bench.py's with_geometry leg) with the switch off and on, two pipelines of one process, regions of --steps key frames
            interleaved, --reps regions each after one warm-up region: key frames/s, edges, and the stage's counters.

    python tools/pcm_timing.py [--out profiles/pcm_timing.md] [--parent DIR] [--bench-reps 3] [--steps 192] [--reps 4]

Records figures; gates nothing."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD = (256, 1024, 4096)
NEW = 8


def med(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def random_edges(c, n, seed):
    """n edges of drones 1 and 2, either order, with unrelated poses: no pair is consistent -- every lane runs the same arithmetic whatever the verdict"""
    rng = np.random.default_rng(seed)
    e = np.zeros(n, c.PCM_EDGE_DTYPE)
    q = rng.normal(size=(3, n, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    e["id"] = np.arange(n) + 1000
    swap = rng.random(n) < 0.5
    e["drone_a"], e["drone_b"] = np.where(swap, 2, 1), np.where(swap, 1, 2)
    for k, name in enumerate(("relative_pose", "self_pose_a", "self_pose_b")):
        e[name][:, :3] = rng.normal(size=(n, 3)) * 5
        e[name][:, 3:] = q[k]
    e["arc_a"], e["arc_b"] = rng.random(n) * 200, rng.random(n) * 200
    e["pos_cov"], e["ang_cov"] = 0.05, 0.05
    return e


def time_rows(c, ctx):
    out = {}
    for held in HELD:
        e = random_edges(c, held + NEW * 13, held)
        p = c.Pcm(ctx, held + 128)
        for at in range(0, held, 64):
            p.add(e[at:at + 64])
        dev, wall, host = [], [], []
        for k in range(13):
            lo = held + NEW * k
            t0 = time.perf_counter()
            deg, rows = p.add(e[lo:lo + NEW], time_kernel=True)
            t1 = time.perf_counter()
            t2 = time.perf_counter()
            hrows, _ = c.pcm_rows_host(e[:lo + NEW], first=lo, stride_words=p.capacity // 64)
            t3 = time.perf_counter()
            assert np.array_equal(rows, hrows)
            if k >= 3:
                dev.append(p.last_kernel_us); wall.append((t1 - t0) * 1e6); host.append((t3 - t2) * 1e6)
        p.close()
        out[held] = (med(dev), med(wall), med(host))
    return out


def time_clique(c):
    from tests import pcm_cases as PC      # the bitset packing only
    out = {}
    rng = np.random.default_rng(5)
    for n in HELD:
        full = ~np.eye(n, dtype=bool)
        half = np.triu(rng.random((n, n)) < 0.5, 1)
        half = half | half.T
        row = []
        for A in (full, half):
            bits = PC.dense_to_bits(A)
            us, size = [], 0
            for _ in range(5):
                t0 = time.perf_counter()
                size = len(c.pcm_max_clique_host(bits, n))
                us.append((time.perf_counter() - t0) * 1e6)
            row.append((med(us), size))
        out[n] = row
    return out


def bench_once(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed: {r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["value"])


def time_bench(parent, reps):
    here, there = [], []
    for _ in range(reps):
        there.append(bench_once(parent))
        print("bench: parent", there[-1], flush=True)
        here.append(bench_once(ROOT))
        print("bench: this tree", here[-1], flush=True)
    return here, there


def time_stream(omni, steps, reps):
    from omni_swarm_amd import capi as c, pipeline, synth, weights
    W, H, MB, ROOMS = 600, 480, 8, 32
    sp_w = weights.superpoint_synth_weights(0)
    comp, mean = synth.pca()
    td = tempfile.TemporaryDirectory(prefix="omni_pcm_timing_")
    files = weights.write_pipeline_files(td.name, sp_w, comp, mean, weights.mobilenetvlad_synth_weights(), weights.mobilenetvlad_layer_specs(), c.VLAD_KINDS)
    ictx = c.Context(0)
    blocks = []
    for p in range(ROOMS // MB):
        a = ictx.host_alloc((8 * MB, H, W), np.uint8)
        kf = [synth.room_keyframe(MB * p + m, H, W) for m in range(MB)]
        a[:] = np.stack([kf[m][i] for m in range(MB) for i in range(4)] + [kf[m][4 + i] for m in range(MB) for i in range(4)])
        blocks.append(a)
    ptrs = [a.ctypes.data for a in blocks]
    rng = np.random.default_rng(7)
    db = rng.normal(size=(4000, 4096)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    pls, state = {}, {}
    for on in (False, True):
        pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, 200, c.PREC_F16, MB, 0, c.STORE_F32, 1, 0.3, 0.2, 5, 30, 3,
                                       geometry=True, pcm=on)
        pl.preload(db)
        pl.prepare(steps)
        pls[on], state[on] = pl, dict(id=0, slot=0, rate=[])
    for rep in range(reps + 1):
        for on in (False, True):
            pl, s = pls[on], state[on]
            pl.sync()
            t0 = time.perf_counter()
            pl.run(steps, s["id"], ptrs, s["slot"], None, True)
            pl.sync()
            if on:
                pl.pcm_stats()                                   # (whatever the last batch left enters the stage inside the timed region)
            dt = time.perf_counter() - t0
            s["id"] += steps; s["slot"] += steps // MB
            if rep:
                s["rate"].append(steps / dt)
            print("stream: region", rep, "pcm", on, round(steps / dt, 1), flush=True)
    out = {}
    for on in (False, True):
        pl = pls[on]
        out[on] = dict(rate=med(state[on]["rate"]), edges=pl.geometry_stats()[1], good=len(pl.good_edges()), stats=pl.pcm_stats())
        pl.close()
    for a in blocks:
        ictx.host_free(a)
    ictx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_timing.md"))
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: bench.py there alternates with bench.py here")
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--skip-stream", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import omni_loader
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    name = f"{info['name'].strip()}, {info['n_cu']} CUs" if isinstance(info, dict) else str(info)
    L = ["# Pairwise consistency of loop edges: timings", "", f"Device: {name}.  `tools/pcm_timing.py`; figures are medians (min .. max).", ""]
    rows = time_rows(c, ctx)
    print("rows: done", flush=True)
    L += ["## omni_pcm_add, 8 new edges", "", "| held edges | pairs | device, 4 launches (us) | wall, whole call (us) | omni_pcm_rows_host, one thread (us) |", "|---|---|---|---|---|"]
    f = lambda m: f"{m[0]:.1f} ({m[1]:.1f} .. {m[2]:.1f})"
    for held, (dev, wall, host) in rows.items():
        L.append(f"| {held} | {NEW * held + NEW * (NEW - 1) // 2} | {f(dev)} | {f(wall)} | {f(host)} |")
    cl = time_clique(c)
    L += ["", "## omni_pcm_max_clique_host", "", "| vertices | all consistent (us) | clique | half consistent (us) | clique |", "|---|---|---|---|---|"]
    for n, ((a, sa), (h, sh)) in cl.items():
        L.append(f"| {n} | {f(a)} | {sa} | {f(h)} | {sh} |")
    ctx.close()
    if args.parent:
        here, there = time_bench(args.parent, args.bench_reps)
        mh, mt = med(here), med(there)
        spread = (mt[2] - mt[1]) / 2
        verdict = "not resolved" if abs(mh[0] - mt[0]) <= 3 * spread else "RESOLVED"
        L += ["", "## bench.py --gpus 1 --steps 200 --warmup 20, the switch off, alternated with the parent commit", "",
              f"- parent: {f(mt)} key frames/s over {there}", f"- this tree: {f(mh)} key frames/s over {here}",
              f"- difference of the medians {mh[0] - mt[0]:+.1f}, three times the parent's spread {3 * spread:.1f}: {verdict}"]
    if not args.skip_stream:
        st = time_stream(omni, args.steps, args.reps)
        L += ["", f"## with the geometry stage, regions of {args.steps} key frames, the switch off / on", ""]
        for on in (False, True):
            r = st[on]
            L.append(f"- pcm {'on' if on else 'off'}: {f(r['rate'])} key frames/s; {r['edges']} edges, {r['good']} in good_edges(); stats {r['stats']}")
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
