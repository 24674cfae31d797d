#!/usr/bin/env python3
"""Times the LoopNet wire of a key-frame unit (KeyframePipeline::Config::wire / device_wire; csrc/wire_pack.hip) for a unit of 8 STEREO_FISHEYE key frames at 200
key points, on one commit:

  kernel    `wire_pack_kernel` alone (omni_wire_pack_enqueue_dev on HBM-resident arrays): HIP events around one launch, 32 images x 200 key points, two thirds of
            them flagged; median of 20 launches after 5 warm-up launches; and omni_wire_pack_host on the same arrays on one thread;
  bytes     what the stage copies down per unit besides the unit's arrays;
  unit      a STEREO_FISHEYE pipeline (fp16, 600 x 480 flattened views, max_num 200, micro-batch 8, geometry and device_landmarks on) fed units of 8 key frames by
            run(), with the wire off, on the host path and with device_wire, in three pipelines of one process, ALTERNATING: per unit the wall time of run(), the
            calling thread's time in the wire inside finish() (wire_host_ms) and host_times().  Median and spread over the timed units.

    python tools/wire_pack_timing.py [--out profiles/wire_pack_timing.md] [--units 40]
    python tools/wire_pack_timing.py --leg off --root <a checkout with built libraries> [--units 40]      one line: the wire-off leg alone, for pairs against another commit

Records figures; gates nothing."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MAX_NUM, KF, DIRS, REPS, WARMUP = 600, 480, 200, 8, 4, 20, 5
LEGS = {"off": (False, False), "host": (True, False), "device": (True, True)}


def med(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def time_kernel(c, ctx):
    rng = np.random.default_rng(0)
    N, M = KF * DIRS, MAX_NUM
    meta = np.zeros(N, c.WIRE_META_DTYPE)
    meta["drone_id"], meta["direction"] = 1, np.arange(N) % 4
    ins = [rng.uniform(0, 600, (N, M, 2)).astype(np.float32), np.full(N, M, np.int32), rng.uniform(-1, 1, (N, M, 64)).astype(np.float32),
           rng.uniform(-1, 1, (N, M, 2)).astype(np.float32), rng.uniform(-5, 5, (N, M, 3)).astype(np.float32), (rng.integers(0, 3, (N, M)) != 0).astype(np.uint8),
           rng.uniform(-1, 1, (N, 4096)).astype(np.float32), meta]
    dev = [ctx.to_device(a.view(np.uint8) if a.dtype == c.WIRE_META_DTYPE else a) for a in ins]
    dev += [ctx.alloc(N * c.wire_packet_capacity(M)), ctx.alloc(4 * N * c.wire_table_ints(M))]
    try:
        for _ in range(WARMUP):
            c.wire_pack_dev(ctx, N, M, *dev)
        ctx.sync()
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            c.wire_pack_dev(ctx, N, M, *dev)
            ms.append(ctx.timer_stop())
        table = ctx.from_device(dev[-1], (N, c.wire_table_ints(M)), np.int32)
    finally:
        for d in dev:
            ctx.free(d)
    host = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.wire_pack_host(*ins)
        host.append((time.perf_counter() - t0) * 1e3)
    return {"gpu_us": tuple(x * 1e3 for x in med(ms)), "host_ms": med(host), "packets": int(table[:, 0].sum()), "bytes": int(table[:, 1].sum() - 3 * N), "images": N}


def time_units(omni, ctx, n_units, legs):
    from oracle import mobilenetvlad_ref as V
    from oracle import superpoint_ref as S
    from omni_swarm_amd import pipeline, synth, weights
    c = omni.capi
    comp, mean = synth.pca()
    kf = [synth.room_keyframe(p, H, W, 0, 0.0) for p in range(KF)]
    block = ctx.host_alloc((2 * DIRS * KF, H, W), np.uint8)
    block[:] = np.stack([kf[m][i] for m in range(KF) for i in range(DIRS)] + [kf[m][DIRS + i] for m in range(KF) for i in range(DIRS)])
    poses = np.tile(np.array([0.0, 0.0, 1.0, 1, 0, 0, 0]), (KF, 1))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        files = weights.write_pipeline_files(td, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), c.VLAD_KINDS)
        pls = {}
        for leg in legs:
            pls[leg] = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, MAX_NUM, c.PREC_F16, KF, 2, c.STORE_F32, 1, 0.3, 0.2, 5, 30, 3,
                                                 geometry=True, device_landmarks=True)
            if LEGS[leg][0]:
                pls[leg].set_wire(*LEGS[leg])
        keys = ("enqueue", "wait_gpu", "messages", "detector", "geometry")
        wall, wire, host, sent = {l: [] for l in legs}, {l: [] for l in legs}, {l: {k: [] for k in keys} for l in legs}, {}
        for u in range(WARMUP + n_units):
            for leg in legs:                                                # alternating: the legs see the same machine
                pl = pls[leg]
                first = u * KF
                pl.set_poses(first, poses)
                pl.host_times(True)
                t0 = time.perf_counter()
                pl.run(KF, first, [block.ctypes.data], 0, None, True)        # returns with the unit's detector step and geometry collected
                dt = (time.perf_counter() - t0) * 1e3
                ht = pl.host_times(True)
                ws = pl.wire_host_ms(True) if LEGS[leg][0] else 0.0
                if LEGS[leg][0]:
                    n_pk = n_b = 0
                    while pl.wire_pending:
                        _, pk = pl.take_packets()
                        n_pk += len(pk)
                        n_b += sum(len(b) for _, b in pk)
                    sent[leg] = (n_pk, n_b)
                if u >= WARMUP:
                    wall[leg].append(dt)
                    wire[leg].append(ws)
                    for k in keys:
                        host[leg][k].append(ht[k])
        for leg in legs:
            pls[leg].close()
            res[leg] = {"wall": med(wall[leg]), "wire": med(wire[leg]), "host": {k: med(v) for k, v in host[leg].items()}, "sent": sent.get(leg)}
    ctx.host_free(block)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_pack_timing.md"))
    ap.add_argument("--units", type=int, default=40)
    ap.add_argument("--leg", default=None, help="off: time the wire-off leg alone and print one JSON line (works on a commit without the wire)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and libraries are loaded")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import omni_loader
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    if args.leg:
        r = time_units(omni, ctx, args.units, [args.leg])[args.leg]
        ctx.close()
        print(json.dumps({"leg": args.leg, "root": os.path.abspath(args.root), "units": args.units, "wall_ms": r["wall"], "messages_ms": r["host"]["messages"]}))
        return
    info = ctx.device_info()
    kern = time_kernel(c, ctx)
    units = time_units(omni, ctx, args.units, list(LEGS))
    ctx.close()
    cap, te, n_img = c.wire_packet_capacity(MAX_NUM), c.wire_table_ints(MAX_NUM), KF * DIRS
    lines = ["# LoopNet wire: a key-frame unit's packets packed on the GPU against the host loop", "",
             f"`tools/wire_pack_timing.py` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs).  Figures are recorded, not gated.", "",
             "## The kernel alone", "",
             f"`wire_pack_kernel`, HIP events around one launch on HBM-resident arrays: {kern['images']} images (a unit of {KF} STEREO_FISHEYE key frames) x {MAX_NUM} key points, two "
             f"thirds flagged: {kern['packets']} packets, {kern['bytes']} bytes.  Median of {REPS} launches after {WARMUP} warm-up launches; `omni_wire_pack_host` (the g++ build of the "
             "same header) on the same arrays on one thread next to it.", "",
             "| | median | min | max |", "|---|---|---|---|",
             f"| kernel, us | {kern['gpu_us'][0]:.1f} | {kern['gpu_us'][1]:.1f} | {kern['gpu_us'][2]:.1f} |",
             f"| omni_wire_pack_host, ms | {kern['host_ms'][0]:.3f} | {kern['host_ms'][1]:.3f} | {kern['host_ms'][2]:.3f} |", "",
             "## The extra copies", "",
             f"With `device_wire` a unit of {KF} key frames copies down {n_img} buffers of {cap} bytes and {n_img} tables of {te} ints more: {n_img * cap + 4 * n_img * te} bytes "
             f"({(n_img * cap + 4 * n_img * te) / 1e6:.2f} MB; the buffers go down at their full capacity, whatever they hold), and uploads {n_img * 144} bytes of records.", "",
             "## The unit", "",
             f"A STEREO_FISHEYE pipeline (fp16, {W} x {H} flattened views, max_num {MAX_NUM}, micro-batch {KF}, 2 lanes, geometry and device_landmarks on), `run()` of one unit of {KF} key "
             f"frames (`synth.room_keyframe` places 0..{KF - 1}), the wire off, on the host path and with `device_wire` in three pipelines of one process, alternating; {args.units} timed "
             f"units each after {WARMUP} warm-up units.  A unit sends {units['host']['sent'][0]} packets, {units['host']['sent'][1]} bytes (host path) / {units['device']['sent'][0]} "
             f"packets, {units['device']['sent'][1]} bytes (`device_wire`).  `wire in finish()` is the calling thread's time in the wire per unit: "
             "`LoopNetWire::broadcast_fisheye_desc` on the host path, the copy out of the pinned block and the id patch with `device_wire`.  Milliseconds: median (min .. max).", "",
             "| wire | run() wall | wire in finish() | enqueue | wait_gpu | messages | detector | geometry |", "|---|---|---|---|---|---|---|---|"]
    for leg in LEGS:
        r = units[leg]
        lines.append(f"| {leg} | {fmt(r['wall'])} | {fmt(r['wire'])} | " + " | ".join(fmt(r["host"][k]) for k in ("enqueue", "wait_gpu", "messages", "detector", "geometry")) + " |")
    d = units["host"]["wire"][0] - units["device"]["wire"][0]
    lines += ["", f"Medians: the host loop costs the calling thread {units['host']['wire'][0]:.3f} ms per unit ({units['host']['wire'][0] / KF * 1e3:.0f} us per key frame), `device_wire` "
              f"{units['device']['wire'][0]:.3f} ms: {d:+.3f} ms per unit.  `run()` wall, against the wire off: host path {units['host']['wall'][0] - units['off']['wall'][0]:+.3f} ms, "
              f"`device_wire` {units['device']['wall'][0] - units['off']['wall'][0]:+.3f} ms."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
