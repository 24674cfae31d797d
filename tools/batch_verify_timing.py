#!/usr/bin/env python3
"""Times inter-drone loop candidates verified with their batch (KeyframePipeline(..., batch_verify=True); host/verify_plan.hpp, csrc/corr_assemble.hip) against
verifying them on the spot, on one commit:

  kernel    `corr_assemble_kernel` alone (omni_corr_assemble_multi): HIP events around one launch at the shapes of a unit's resolve -- 8 + R candidates of 4 direction
            pairs of 200 key points each, R = 0, 1, 4, 8 -- median of 20 launches after 5 warm-up launches, the output compared bit for bit with
            omni_corr_assemble_host; next to it the calling thread's time in omni_corr_assemble_host for the same call: the arithmetic a pool task no longer runs;
  stream    the bench-shaped STEREO_FISHEYE pipeline (fp16, 600 x 480 flattened views, max_num 200, micro-batch 8, the library's default units in flight, the
            geometry stage on, remote_in_stream on, 1 000 key frames pre-loaded) fed through push_keyframe with 16 rendered rooms again and again, R remote key
            frames queued behind every 8 local ones: copies of stored frames under other ids, as drone 2's.  Switch off = the parent commit's behaviour and the
            baseline.  Two pipelines of one process; regions of --units units each, R and the switch INTERLEAVED, --reps regions per combination after one warm-up
            region.  Per region: key frames/s (local key frames over the wall time, the closing flush() included) and the calling thread's milliseconds per unit
            inside the pipeline's calls.

A difference below three times the baseline's own spread (half of max - min over its regions) is reported as not resolved.

    python tools/batch_verify_timing.py [--out profiles/batch_verify_timing.md] [--units 24] [--reps 5]

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


def kernel_call(c, rng, n_cands, n=MAX_NUM):
    """n_cands candidates of DIRS pairs of n key points: about 85 % matched, 70 % of the key points flagged, a mask that keeps 60 %"""
    cands, pairs = [], []
    for k in range(n_cands):
        cands.append((len(pairs), DIRS, 15, 3, 30, 10, 0))
        for _ in range(DIRS):
            m = int(0.85 * n)
            q_idx = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
            flags = (rng.random(n) < 0.7).astype(np.uint8)
            kept = int(flags[q_idx].sum())
            dq = rng.normal(size=4)
            pairs.append(dict(q_idx=q_idx, t_idx=rng.choice(n, m, replace=False).astype(np.int32), q_flags=flags, nq=n, nt=n, mask=(rng.random(kept) < 0.6).astype(np.uint8),
                              hg_status=c.HG_OK, q_3d=rng.normal(size=(n, 3)), t_norm=rng.normal(size=(n, 2)) * 0.5, dq_old=dq / np.linalg.norm(dq)))
    return cands, pairs


def same(a, b):
    return all(x["n_corr"] == y["n_corr"] and x["gate"] == y["gate"] and x["X"].tobytes() == y["X"].tobytes() and x["u"].tobytes() == y["u"].tobytes() for x, y in zip(a[0], b[0])) and \
        all(np.array_equal(x["new_idx"], y["new_idx"]) and np.array_equal(x["old_idx"], y["old_idx"]) for x, y in zip(a[1], b[1]))


def time_kernel(c, ctx):
    rng = np.random.default_rng(0)
    out = {}
    for R in RS:
        cands, pairs = kernel_call(c, rng, MB + R)
        arrays = c.CorrArrays(cands, pairs)
        import ctypes as C
        host_us = []
        for _ in range(REPS_K):
            t0 = time.perf_counter()
            c.lib().omni_corr_assemble_host(C.byref(arrays.io))
            host_us.append((time.perf_counter() - t0) * 1e6)
        host = arrays.result()
        for _ in range(WARMUP_K):
            c.corr_assemble(cands, pairs, ctx)
        us, dev = [], None
        for _ in range(REPS_K):
            cd, pp, t = c.corr_assemble(cands, pairs, ctx, time_kernel=True)
            us.append(t); dev = (cd, pp)
        assert same(dev, host)
        out[R] = (len(cands), len(pairs), sum(x["n_corr"] for x in host[0]), med(us), med(host_us))
    return out


def time_stream(omni, ctx, n_units, reps):
    from omni_swarm_amd import pipeline, synth, weights
    c = omni.capi
    comp, mean = synth.pca()
    POOL = 2
    # rendered rooms (synth.room_keyframe), revisited every POOL * MB key frames: the geometry stage has loops to close and every remote copy a candidate to verify
    frames = [list(synth.room_keyframe(k, H, W)) for k in range(POOL * MB)]
    rng = np.random.default_rng(7)
    db = rng.standard_normal((4000, 4096)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    with tempfile.TemporaryDirectory() as td:
        files = weights.write_pipeline_files(td, weights.superpoint_synth_weights(0), comp, mean, weights.mobilenetvlad_synth_weights(), weights.mobilenetvlad_layer_specs(),
                                             c.VLAD_KINDS)
        pls, state = {}, {}
        for on in (False, True):
            pls[on] = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, MAX_NUM, c.PREC_F16, MB, 0, c.STORE_F32, 1, 0.3, 0.2, 5, 30, 3,
                                                geometry=True, remote_in_stream=True, batch_verify=on)
            pls[on].preload(db)
            state[on] = {"id": 0, "remote": 0}

        def region(on, R):
            """n_units units of MB key frames, R remote frames queued behind each; -> (seconds, seconds inside the pipeline's calls)"""
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
                    pl.queue_copy_as_remote(src, 2, new)
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
        vstats = {R: None for R in RS}
        for _ in range(reps):
            for R in RS:                                                   # interleaved: every combination sees the same machine
                for on in (False, True):
                    before = pls[on].verify_stats() + pls[on].corr_stats()
                    dt, inside = region(on, R)
                    kfs[(on, R)].append(n_units * MB / dt)
                    host[(on, R)].append(inside * 1e3 / n_units)
                    if on:
                        vstats[R] = tuple(a - b for a, b in zip(pls[on].verify_stats() + pls[on].corr_stats(), before))
        same_results = np.array_equal(np.array(pls[True].candidates()), np.array(pls[False].candidates())) and np.array_equal(pls[True].edges(), pls[False].edges()) and \
            np.array_equal(pls[True].edge_ids(), pls[False].edge_ids())
        res = {"kfs": {k: med(v) for k, v in kfs.items()}, "host": {k: med(v) for k, v in host.items()}, "vstats": vstats, "total": pls[True].verify_stats() + pls[True].corr_stats(),
               "rows": {on: pls[on].db_rows for on in pls}, "candidates": {on: len(pls[on].candidates()) for on in pls}, "edges": {on: len(pls[on].edges()) for on in pls},
               "same": bool(same_results)}
        for on in pls:
            pls[on].close()
    return res


def verdict(base, new):
    """the project's rule: a difference below three times the baseline's own spread is not resolved"""
    spread = (base[2] - base[1]) / 2
    d = new[0] - base[0]
    return f"{d:+.4g} ({100 * d / base[0]:+.1f} %)" + ("" if abs(d) >= 3 * spread else " -- not resolved")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_verify_timing.md"))
    ap.add_argument("--units", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import omni_loader
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    kern = time_kernel(c, ctx)
    s = time_stream(omni, ctx, args.units, args.reps)
    ctx.close()
    f3 = lambda t: f"{t[0]:.4g} ({t[1]:.4g} .. {t[2]:.4g})"
    lines = ["# Inter-drone loop candidates verified with their batch against verifying them on the spot", "",
             f"`tools/batch_verify_timing.py --units {args.units} --reps {args.reps}` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs).  Figures are recorded, not gated.", "",
             "## The kernel alone", "",
             f"`corr_assemble_kernel`, HIP events around one launch (the events bracket the launch, so an idle stream's launch latency is inside): {MB} + R candidates of {DIRS} direction "
             f"pairs of {MAX_NUM} key points each, about 85 % of them matched, 70 % flagged, a mask that keeps 60 %.  Median of {REPS_K} launches after {WARMUP_K} warm-up launches; "
             "the output is compared bit for bit with `omni_corr_assemble_host`.  Host: the calling thread's time in `omni_corr_assemble_host` for the same call on this box's CPU "
             "-- the arithmetic the candidates' pool tasks no longer run.", "",
             "| R | candidates | pairs | correspondences | kernel us, median | min | max | host us, median | min | max |", "|---|---|---|---|---|---|---|---|---|---|"]
    for R in RS:
        nc, npairs, ncorr, us, hus = kern[R]
        lines.append(f"| {R} | {nc} | {npairs} | {ncorr} | {us[0]:.1f} | {us[1]:.1f} | {us[2]:.1f} | {hus[0]:.1f} | {hus[1]:.1f} | {hus[2]:.1f} |")
    lines += ["", "## The stream", "",
              f"The bench-shaped STEREO_FISHEYE pipeline (fp16, {W} x {H}, max_num {MAX_NUM}, micro-batch {MB}, the library's default units in flight, the geometry stage on, "
              "`remote_in_stream` on, 1 000 key frames pre-loaded), `push_keyframe` of 16 rendered rooms (`synth.room_keyframe`) again and again, "
              f"R remote key frames queued behind every {MB} local ones (copies of stored frames as drone 2's).  Regions of {args.units} units ({args.units * MB} local key frames, closed "
              f"by `flush()`), R and the switch interleaved, {args.reps} regions per combination after a warm-up region.  Switch off: every inter-drone candidate verified on the spot "
              "-- the parent commit's behaviour, the baseline.  Median (min .. max).", "",
              "| R | key frames/s, off | key frames/s, on | on - off | calling thread ms/unit, off | ms/unit, on | on - off |", "|---|---|---|---|---|---|---|"]
    for R in RS:
        ko, kn, ho, hn = s["kfs"][(False, R)], s["kfs"][(True, R)], s["host"][(False, R)], s["host"][(True, R)]
        lines.append(f"| {R} | {f3(ko)} | {f3(kn)} | {verdict(ko, kn)} | {f3(ho)} | {f3(hn)} | {verdict(ho, hn)} |")
    lines += ["", "`verify_stats()` + `corr_stats()` of the switch-on pipeline over the last region of every R (inter-drone candidates deferred, resolves at the end of a batch, early "
              "resolves, matcher round trips spent on them, candidates whose correspondences came from the GPU, candidates handed back):", ""]
    lines += [f"* R = {R}: {s['vstats'][R]}" for R in RS]
    lines += ["", f"Over the whole run: {s['total']}.  Both pipelines end with {s['rows'][True]} / {s['rows'][False]} database rows, {s['candidates'][True]} / {s['candidates'][False]} "
              f"candidates and {s['edges'][True]} / {s['edges'][False]} edges (on / off); candidates, every field of every edge and the edge ids identical: {s['same']}."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
