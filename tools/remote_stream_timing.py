#!/usr/bin/env python3
"""Times remote key frames joining the unit stream (KeyframePipeline(..., remote_in_stream=True); host/remote_queue.hpp, csrc/rows_assemble.hip) against the serial
flow they replace, on one commit:

  kernel    `rows_assemble_kernel` alone (omni_rows_assemble_enqueue_dev on HBM-resident blocks): HIP events around one launch at the shapes of a unit's batch --
            32 unit rows plus 4 R staged rows of 4096 floats, R = 0, 1, 4, 8 -- median of 20 launches after 5 warm-up launches;
  stream    the bench-shaped STEREO_FISHEYE pipeline (fp16, 600 x 480 flattened views, max_num 200, micro-batch 8, the library's default units in flight, no
            geometry stage, 1 000 key frames pre-loaded) fed through push_keyframe, R remote key frames injected behind every 8 local ones: copies of stored
            frames under other ids, as drone 2's.  Switch off = the parent commit's behaviour and the baseline: what the wire does per frame, flush() and then
            on_remote_frame (omni_pipeline_recv_copy_as_remote).  Switch on: omni_pipeline_queue_copy_as_remote.  Two pipelines of one process; regions of
            --units units each, R and the switch INTERLEAVED, --reps regions per combination after one warm-up region.  Per region: key frames/s (local key
            frames over the wall time, the closing flush() included) and the calling thread's milliseconds per unit inside the pipeline's calls.

A difference below three times the baseline's own spread (half of max - min over its regions) is reported as not resolved.

    python tools/remote_stream_timing.py [--out profiles/remote_in_stream_timing.md] [--units 24] [--reps 7]

Records figures; gates nothing."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MAX_NUM, MB, DIRS, REPS_K, WARMUP_K = 600, 480, 200, 8, 4, 20, 5
RS = (0, 1, 4, 8)


def med(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def time_kernel(c, ctx):
    rng = np.random.default_rng(0)
    out = {}
    for R in RS:
        n_unit, n_staged = DIRS * MB, DIRS * R
        unit, staged = rng.standard_normal((n_unit, 4096)).astype(np.float32), rng.standard_normal((max(n_staged, 1), 4096)).astype(np.float32)
        table = np.array([[c.ROW_STAGED, i] for i in range(n_staged)] + [[c.ROW_UNIT, i] for i in range(n_unit)], np.int32)
        dev = [ctx.to_device(table), ctx.to_device(unit), ctx.to_device(staged), ctx.alloc(4 * 4096 * len(table))]
        try:
            args = (ctx, len(table), 4096, dev[0], dev[1], n_unit, dev[2] if n_staged else None, n_staged, dev[3])
            for _ in range(WARMUP_K):
                c.rows_assemble_dev(*args)
            ctx.sync()
            ms = []
            for _ in range(REPS_K):
                ctx.timer_start()
                c.rows_assemble_dev(*args)
                ms.append(ctx.timer_stop())
            got = ctx.from_device(dev[3], (len(table), 4096), np.float32)
            assert np.array_equal(got.view(np.uint32), c.rows_assemble_host(table, unit, staged[:n_staged], 4096).view(np.uint32))
        finally:
            for d in dev:
                ctx.free(d)
        out[R] = (len(table), tuple(x * 1e3 for x in med(ms)))
    return out


def time_stream(omni, ctx, n_units, reps, geometry):
    from omni_swarm_amd import pipeline, synth, weights
    c = omni.capi
    comp, mean = synth.pca()
    POOL = 2
    # --geometry: rendered rooms (synth.room_keyframe), revisited every POOL * MB key frames, so that the geometry stage has loops to close and every remote copy a
    # candidate to verify on the spot
    frames = [list(synth.room_keyframe(k, H, W)) if geometry else [synth.image_u8(8 * k + i, H, W) for i in range(2 * DIRS)] for k in range(POOL * MB)]
    rng = np.random.default_rng(7)
    db = rng.standard_normal((4000, 4096)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    res = {}
    with tempfile.TemporaryDirectory() as td:
        files = weights.write_pipeline_files(td, weights.superpoint_synth_weights(0), comp, mean, weights.mobilenetvlad_synth_weights(), weights.mobilenetvlad_layer_specs(),
                                             c.VLAD_KINDS)
        pls, state = {}, {}
        for on in (False, True):
            pls[on] = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, MAX_NUM, c.PREC_F16, MB, 0, c.STORE_F32, 1, 0.3, 0.2, 5, 30, 3,
                                                geometry=geometry, remote_in_stream=on)
            pls[on].preload(db)
            state[on] = {"id": 0, "remote": 0}

        def region(on, R):
            """n_units units of MB key frames, R remote frames behind each; -> (seconds, seconds inside the pipeline's calls)"""
            pl, st = pls[on], state[on]
            stored = list(range(MB))                                       # the warm-up region's first key frames: in the database
            inside = 0.0
            pl.sync()
            t_region = time.perf_counter()
            for _ in range(n_units):
                for m in range(MB):
                    t0 = time.perf_counter()
                    pl.push_keyframe(frames[st["id"] % len(frames)], st["id"], float(st["id"]))
                    inside += time.perf_counter() - t0
                    st["id"] += 1
                for r in range(R):
                    src, new = stored[(st["remote"] + r) % len(stored)], 10_000_000 + st["remote"]
                    t0 = time.perf_counter()
                    if on:
                        pl.queue_copy_as_remote(src, 2, new)
                    else:
                        pl.flush()                                         # what drain_inbox does for every frame the wire completes
                        pl.recv_copy_as_remote(src, 2, new)
                    inside += time.perf_counter() - t0
                    st["remote"] += 1
            t0 = time.perf_counter()
            pl.flush()
            inside += time.perf_counter() - t0
            pl.sync()
            return time.perf_counter() - t_region, inside

        for on in (False, True):
            region(on, 0)                                                  # warm-up: every lane used, the first key frames stored
        kfs, host = {(on, R): [] for on in (False, True) for R in RS}, {(on, R): [] for on in (False, True) for R in RS}
        for _ in range(reps):
            for R in RS:                                                   # interleaved: every combination sees the same machine
                for on in (False, True):
                    dt, inside = region(on, R)
                    kfs[(on, R)].append(n_units * MB / dt)
                    host[(on, R)].append(inside * 1e3 / n_units)
        stats = {on: pls[on].remote_stats() for on in pls}
        rows = {on: pls[on].db_rows for on in pls}
        cands = {on: len(pls[on].candidates()) for on in pls}
        edges = {on: len(pls[on].edges()) for on in pls}
        for on in pls:
            pls[on].close()
        res = {"kfs": {k: med(v) for k, v in kfs.items()}, "host": {k: med(v) for k, v in host.items()}, "stats": stats, "rows": rows, "candidates": cands, "edges": edges}
    return res


def verdict(base, new):
    """the project's rule: a difference below three times the baseline's own spread is not resolved"""
    spread = (base[2] - base[1]) / 2
    d = new[0] - base[0]
    return f"{d:+.4g} ({100 * d / base[0]:+.1f} %)" + ("" if abs(d) >= 3 * spread else " -- not resolved")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remote_in_stream_timing.md"))
    ap.add_argument("--units", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--geometry", action="store_true", help="the stream with the geometry stage on, on rendered rooms (remote candidates are verified on the spot)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import omni_loader
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    kern = time_kernel(c, ctx)
    s = time_stream(omni, ctx, args.units, args.reps, args.geometry)
    ctx.close()
    f3 = lambda t: f"{t[0]:.4g} ({t[1]:.4g} .. {t[2]:.4g})"
    lines = ["# Remote key frames in the unit stream against the serial flow (flush + on_remote_frame)", "",
             f"`tools/remote_stream_timing.py --units {args.units} --reps {args.reps}{' --geometry' if args.geometry else ''}` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs).  Figures are recorded, not gated.", "",
             "## The kernel alone", "",
             f"`rows_assemble_kernel`, HIP events around one launch on HBM-resident blocks (the events bracket the launch, so an idle stream's launch latency is inside): {DIRS * MB} unit rows "
             f"plus 4 R staged rows of 4096 floats, the table in device memory.  Median of {REPS_K} launches after {WARMUP_K} warm-up launches; the output is compared bit for bit with "
             "`omni_rows_assemble_host`.", "",
             "| R | rows | bytes moved (read + written) | us, median | min | max |", "|---|---|---|---|---|---|"]
    for R in RS:
        n, us = kern[R]
        lines.append(f"| {R} | {n} | {2 * n * 4096 * 4} | {us[0]:.1f} | {us[1]:.1f} | {us[2]:.1f} |")
    lines += ["", "## The stream", "",
              f"The bench-shaped STEREO_FISHEYE pipeline (fp16, {W} x {H}, max_num {MAX_NUM}, micro-batch {MB}, the library's default units in flight, "
              + ("the geometry stage on, 1 000 key frames pre-loaded), `push_keyframe` of 16 rendered rooms (`synth.room_keyframe`) again and again," if args.geometry else
                 "no geometry stage, 1 000 key frames pre-loaded), `push_keyframe` of synthetic key frames,") +
              f" R remote key frames behind every {MB} local ones (copies of stored frames as drone 2's).  Regions of {args.units} "
              f"units ({args.units * MB} local key frames, closed by `flush()`), R and the switch interleaved, {args.reps} regions per combination after a warm-up region.  Switch off: "
              "`flush()` + `recv_copy_as_remote` per frame -- the parent commit's behaviour, the baseline.  Switch on: `queue_copy_as_remote`.  Median (min .. max).", "",
              "| R | key frames/s, off | key frames/s, on | on - off | calling thread ms/unit, off | ms/unit, on | on - off |", "|---|---|---|---|---|---|---|"]
    for R in RS:
        ko, kn, ho, hn = s["kfs"][(False, R)], s["kfs"][(True, R)], s["host"][(False, R)], s["host"][(True, R)]
        lines.append(f"| {R} | {f3(ko)} | {f3(kn)} | {verdict(ko, kn)} | {f3(ho)} | {f3(hn)} | {verdict(ho, hn)} |")
    lines += ["", f"Counters at the end (frames queued, joined a unit's batch, batches of remote frames alone, flushes forced): on {s['stats'][True]}; the off pipeline queues nothing "
              f"(its frames went through `recv_copy_as_remote`).  Both pipelines end with {s['rows'][True]} / {s['rows'][False]} database rows and {s['candidates'][True]} / "
              f"{s['candidates'][False]} candidates and {s['edges'][True]} / {s['edges'][False]} edges (on / off)."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
