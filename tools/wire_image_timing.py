#!/usr/bin/env python3
"""Times the whole image descriptor on the LoopNet wire (KeyframePipeline::Config::wire_img_desc; wire_pack_image_kernel in csrc/wire_pack.hip) for a unit of 8
STEREO_FISHEYE key frames at 200 key points, send_img at quality 75, in the modes IMAGE (the file, no 64-d descriptors) and WHOLE (both):

  kernel    `wire_pack_image_kernel` alone (omni_wire_pack_image_enqueue_dev on HBM-resident arrays): HIP events around one launch, 32 images x 200 key points, files of
            half the capacity; median of 20 launches after 5 warm-up launches; and omni_wire_pack_image_host on the same arrays on one thread;
  bytes     what the stage copies down per unit besides the unit's arrays and its header + landmark packets;
  unit      a STEREO_FISHEYE pipeline (fp16, 600 x 480 flattened views, max_num 200, micro-batch 8, geometry, device_landmarks and send_img on) fed units of 8 key
            frames by run(), per mode on the host path and with device_wire, next to the wire without the new packets, in pipelines of one process, ALTERNATING: per
            unit the wall time of run() (the unit's latency) and the calling thread's time in the wire inside finish() (wire_host_ms).  Median and spread.

    python tools/wire_image_timing.py [--out profiles/wire_image_timing.md] [--units 30]

Records figures; gates nothing."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MAX_NUM, KF, DIRS, REPS, WARMUP, Q = 600, 480, 200, 8, 4, 20, 5, 75
JCAP = W * H // 2
LEGS = {"wire, host": ("off", False), "wire, device": ("off", True), "IMAGE, host": ("image", False), "IMAGE, device": ("image", True), "WHOLE, host": ("whole", False),
        "WHOLE, device": ("whole", True)}


def med(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def time_kernel(c, ctx, with_features):
    rng = np.random.default_rng(0)
    N, M = KF * DIRS, MAX_NUM
    meta = np.zeros(N, c.WIRE_META_DTYPE)
    meta["drone_id"], meta["direction"] = 1, np.arange(N) % 4
    ins = [rng.uniform(0, 600, (N, M, 2)).astype(np.float32), np.full(N, M, np.int32), rng.uniform(-1, 1, (N, M, 64)).astype(np.float32),
           rng.uniform(-1, 1, (N, M, 2)).astype(np.float32), rng.uniform(-5, 5, (N, M, 3)).astype(np.float32), (rng.integers(0, 3, (N, M)) != 0).astype(np.uint8),
           rng.uniform(-1, 1, (N, 4096)).astype(np.float32), meta]
    jp = [rng.integers(0, 256, (N, JCAP)).astype(np.uint8), np.full(N, JCAP // 2 + 1, np.int32), np.zeros(N, np.int32)]
    dev = [ctx.to_device(a.view(np.uint8) if a.dtype == c.WIRE_META_DTYPE else a) for a in ins + jp]
    dev += [ctx.alloc(N * c.wire_image_capacity(M, JCAP)), ctx.alloc(8 * N)]
    try:
        launch = lambda: c.wire_pack_image_dev(ctx, N, M, *dev[:11], JCAP, W, H, *dev[11:], with_features=with_features, with_image=True)
        for _ in range(WARMUP):
            launch()
        ctx.sync()
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            launch()
            ms.append(ctx.timer_stop())
        sizes = ctx.from_device(dev[-1], (N, 2), np.int32)
    finally:
        for d in dev:
            ctx.free(d)
    host = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.wire_pack_image_host(*ins, *jp, width=W, height=H, with_features=with_features)
        host.append((time.perf_counter() - t0) * 1e3)
    return {"gpu_us": tuple(x * 1e3 for x in med(ms)), "host_ms": med(host), "bytes": int(sizes[:, 1].sum()), "images": N}


def time_units(omni, ctx, n_units):
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
        pls = {leg: pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, 0.02, MAX_NUM, c.PREC_F16, KF, 2, c.STORE_F32, 1, 0.3, 0.2, 5, 30, 3,
                                              geometry=True, device_landmarks=True, send_img=True, jpg_quality=Q, wire=True, device_wire=dev, wire_img_desc=mode)
               for leg, (mode, dev) in LEGS.items()}
        wall, wire, sent = {l: [] for l in LEGS}, {l: [] for l in LEGS}, {}
        for u in range(WARMUP + n_units):
            for leg, pl in pls.items():                                     # alternating: the legs see the same machine
                first = u * KF
                pl.set_poses(first, poses)
                t0 = time.perf_counter()
                pl.run(KF, first, [block.ctypes.data], 0, None, True)        # returns with the unit's detector step and geometry collected
                dt = (time.perf_counter() - t0) * 1e3
                ws = pl.wire_host_ms(True)
                n_pk = n_b = n_w = 0
                while pl.wire_pending:
                    _, pk = pl.take_packets()
                    n_pk += len(pk)
                    n_b += sum(len(b) for _, b in pk)
                    n_w += sum(len(b) for ch, b in pk if ch == "SWARM_LOOP_IMG_DES")
                sent[leg] = (n_pk, n_b, n_w)
                if u >= WARMUP:
                    wall[leg].append(dt)
                    wire[leg].append(ws)
        for leg, pl in pls.items():
            pl.close()
            res[leg] = {"wall": med(wall[leg]), "wire": med(wire[leg]), "sent": sent[leg]}
    ctx.host_free(block)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_image_timing.md"))
    ap.add_argument("--units", type=int, default=30)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import omni_loader
    omni = omni_loader.load()
    c = omni.capi
    ctx = c.Context(0)
    info = ctx.device_info()
    kern = {name: time_kernel(c, ctx, wf) for name, wf in (("IMAGE", False), ("WHOLE", True))}
    units = time_units(omni, ctx, args.units)
    ctx.close()
    cap, n_img = c.wire_image_capacity(MAX_NUM, JCAP), KF * DIRS
    lines = ["# LoopNet wire: the whole image descriptor packed on the GPU against the host loop", "",
             f"`tools/wire_image_timing.py` on {str(info.get('name', '')).strip()} ({info.get('n_cu')} CUs).  Figures are recorded, not gated.", "",
             "## The kernel alone", "",
             f"`wire_pack_image_kernel`, HIP events around one launch on HBM-resident arrays: {n_img} images (a unit of {KF} STEREO_FISHEYE key frames) x {MAX_NUM} key points, files "
             f"of {JCAP // 2 + 1} bytes in rows of {JCAP}.  Median of {REPS} launches after {WARMUP} warm-up launches; `omni_wire_pack_image_host` (the g++ build of the same header) on "
             "the same arrays on one thread next to it.", "",
             "| mode | packet bytes | kernel, us: median (min .. max) | omni_wire_pack_image_host, ms |", "|---|---|---|---|"]
    for name, k in kern.items():
        lines.append(f"| {name} | {k['bytes']} | {k['gpu_us'][0]:.1f} ({k['gpu_us'][1]:.1f} .. {k['gpu_us'][2]:.1f}) | {fmt(k['host_ms'])} |")
    lines += ["", "## The extra copies", "",
              f"With `device_wire` and either mode a unit of {KF} key frames copies down {n_img} buffers of {cap} bytes and {n_img} pairs of ints more: {n_img * cap + 8 * n_img} bytes "
              f"({(n_img * cap + 8 * n_img) / 1e6:.2f} MB; the buffers go down at their full capacity -- {JCAP} bytes of it the JPEG stage's capacity -- whatever they hold).", "",
              "## The unit", "",
              f"A STEREO_FISHEYE pipeline (fp16, {W} x {H} flattened views, max_num {MAX_NUM}, micro-batch {KF}, 2 lanes, geometry, device_landmarks and send_img at quality {Q} on), "
              f"`run()` of one unit of {KF} key frames (`synth.room_keyframe` places 0..{KF - 1}): the wire without the new packets, IMAGE and WHOLE, each on the host path and with "
              f"`device_wire`, in six pipelines of one process, alternating; {args.units} timed units each after {WARMUP} warm-up units.  `wire in finish()` is the calling thread's "
              "time in the wire per unit (`wire_host_ms`): `LoopNetWire::broadcast_fisheye_desc` on the host path, the copies out of the pinned blocks and the id patches with "
              "`device_wire`.  `run()` wall is the unit's latency.  Milliseconds: median (min .. max).", "",
              "| leg | packets | bytes sent | of them whole descriptors | run() wall | wire in finish() |", "|---|---|---|---|---|---|"]
    for leg in LEGS:
        r = units[leg]
        lines.append(f"| {leg} | {r['sent'][0]} | {r['sent'][1]} | {r['sent'][2]} | {fmt(r['wall'])} | {fmt(r['wire'])} |")
    lines.append("")
    for mode in ("IMAGE", "WHOLE"):
        h, d, b = units[f"{mode}, host"], units[f"{mode}, device"], units["wire, device"]
        lines.append(f"{mode}, medians: the calling thread spends {h['wire'][0]:.3f} ms per unit in the wire on the host path and {d['wire'][0]:.3f} ms with `device_wire` "
                     f"({h['wire'][0] - d['wire'][0]:+.3f} ms saved); `run()` wall {h['wall'][0]:.3f} ms against {d['wall'][0]:.3f} ms ({d['wall'][0] - h['wall'][0]:+.3f} ms with "
                     f"`device_wire`); against `device_wire` without the new packets: {d['wall'][0] - b['wall'][0]:+.3f} ms.")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
