"""Times the intake of one STEREO_FISHEYE key-frame unit of 8 key frames -- 16 fisheye frames of 1280 x 1024, 64 side views of 600 x 312 -- three ways and writes
profiles/fisheye_intake_timing.md:
  views      the flattened views uploaded, as a pipeline configured for flattened views does (omni_cam_enqueue_host);
  raw        the fisheye frames uploaded as pixels and flattened inside the unit (omni_cam_enqueue_fisheye_host);
  jpeg q     the fisheye frames as JPEG files of quality 75 and 95, decoded and flattened inside the unit (omni_cam_enqueue_fisheye_jpeg_host).
Per way, medians of --reps units: the bytes that go up, the time of the whole unit on its SuperPoint stream between two HIP events (upload + decode + flatten +
SuperPoint + matcher + downloads), and the calling thread's time inside the enqueue call (for files: parse + unstuff + pack, then the launches).  The stages are
separated by units whose inputs are already in HBM (omni_cam_enqueue_dev: the networks alone; omni_cam_enqueue_fisheye_dev: flatten + networks) and by a decoder
of the unit's geometry on its own (omni_jpegdec_last_ms: its upload and its memsets + kernels from the handle's events; omni_jpegdec_last_stats: subsequences and
relaxation rounds per frame).  The frames are synthetic camera-like pictures (omni_swarm_amd.synth).
    python tools/fisheye_intake_timing.py [--out profiles/fisheye_intake_timing.md] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omni_loader  # noqa: E402

MEI = (1.8, -0.2, 0.05, 0.001, -0.002, 1100.0, 1098.0, 640.0, 512.0)
SRC_W, SRC_H, FOV, VW, VH, DIRS, N_KF = 1280, 1024, 235.0, 600, 312, 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisheye_intake_timing.md"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    omni = omni_loader.load()
    c = omni.capi
    from omni_swarm_amd import flatten, frontend, synth, weights
    ctx = c.Context(0)
    info = ctx.device_info()
    fl = [c.Flatten(ctx, SRC_W, SRC_H, flatten.generate_undist_maps(MEI, VW, FOV, cam_id)) for cam_id in (0, 1)]
    comp, mean = synth.pca()
    lc = frontend.LoopCam(ctx, weights.superpoint_synth_weights(0), comp, mean, weights.mobilenetvlad_synth_weights(), weights.mobilenetvlad_layer_specs(), (32, 112, 4096),
                          VW, VH, 0.015, 200, c.PREC_F16, n_dirs=N_KF * DIRS)
    cam = lc.cam
    frames = [[synth.image_u8(5200 + 100 * cam_id + k, SRC_H, SRC_W, n_shapes=400) for k in range(N_KF)] for cam_id in range(2)]
    raw = [ctx.host_alloc((N_KF, SRC_H, SRC_W), np.uint8) for _ in range(2)]

    def unit(enqueue):
        """-> (SuperPoint-stream ms of the unit, calling-thread ms of the enqueue call), medians"""
        dev, call = [], []
        for r in range(a.reps + 2):
            ctx.sync()
            ctx.timer_start()
            t0 = time.perf_counter()
            enqueue()
            t1 = time.perf_counter()
            ms = ctx.timer_stop()
            cam.wait()
            if r >= 2:
                dev.append(ms), call.append((t1 - t0) * 1e3)
        return float(np.median(dev)), float(np.median(call))

    rows, notes = [], []
    flat = ctx.host_alloc((2 * N_KF * DIRS, VH, VW), np.uint8)
    for quality in (None, 75, 95):
        if quality is None:
            for cam_id in range(2):
                raw[cam_id][:] = np.stack(frames[cam_id])
            files = None
        else:
            files = [[c.jpeg_encode_host(g, quality)[1] for g in frames[cam_id]] for cam_id in range(2)]
            for cam_id in range(2):
                raw[cam_id][:] = np.stack([c.jpeg_decode_host(f)[1] for f in files[cam_id]])
        if quality is None:
            # the unit's own input block, read back once, is what the flattened-view ways upload
            cam.enqueue_fisheye_host(fl[0], fl[1], raw[0], raw[1], 1, False)
            cam.wait()
            flat[:] = cam.get_input()
            flat_dev, raw_dev = ctx.to_device(flat), [ctx.to_device(r) for r in raw]
            nets = unit(lambda: cam.enqueue_dev(flat_dev, VW, True))
            fl_nets = unit(lambda: cam.enqueue_fisheye_dev(fl[0], fl[1], raw_dev[0], raw_dev[1], SRC_W, N_KF, 1, True))
            views = unit(lambda: cam.enqueue_host(flat, True))
            pix = unit(lambda: cam.enqueue_fisheye_host(fl[0], fl[1], raw[0], raw[1], 1, True))
            ctx.free(flat_dev)
            for p in raw_dev:
                ctx.free(p)
            notes += [f"networks alone (views already in HBM, omni_cam_enqueue_dev): {nets[0]:.3f} ms on the SuperPoint stream",
                      f"flatten + networks (frames already in HBM, omni_cam_enqueue_fisheye_dev): {fl_nets[0]:.3f} ms -> the two flatten launches: {fl_nets[0] - nets[0]:.3f} ms"]
            rows.append(("views (as today)", flat.nbytes, views[0], views[0] - nets[0], 0.0, 0.0, views[1], "", ""))
            rows.append(("raw pixels", raw[0].nbytes + raw[1].nbytes, pix[0], pix[0] - fl_nets[0], 0.0, fl_nets[0] - nets[0], pix[1], "", ""))
            continue
        jp = unit(lambda: cam.enqueue_fisheye_jpeg_host(fl[0], fl[1], files[0], files[1], 1, True))
        assert cam.jpegdec_status() == [c.JPEGDEC_OK] * (2 * N_KF)
        # the decode stage on its own: a decoder of the unit's geometry, the same 16 files
        dec = c.JpegDec(ctx, SRC_W, SRC_H, 2 * N_KF, SRC_W * SRC_H // 2)
        out, stat = ctx.alloc(2 * N_KF * SRC_W * SRC_H), ctx.alloc(4 * 2 * N_KF)
        up, ker, call = [], [], []
        both = files[0] + files[1]
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            dec.enqueue_host(both, out, SRC_W, stat)
            t1 = time.perf_counter()
            u, k, nbytes = dec.last_ms()
            if r >= 2:
                up.append(u), ker.append(k), call.append((t1 - t0) * 1e3)
        stats = dec.last_stats(2 * N_KF)
        got = ctx.from_device(out, (2 * N_KF, SRC_H, SRC_W), np.uint8)
        assert np.array_equal(got, np.concatenate(raw))
        dec.close()
        ctx.free(out), ctx.free(stat)
        total = sum(len(f) for f in both)
        notes.append(f"quality {quality}: files {total} bytes ({total // (2 * N_KF)} per frame); decoder alone: upload {np.median(up):.3f} ms, memsets + kernels {np.median(ker):.3f} ms, "
                     f"calling thread (parse + unstuff + pack + launches) {np.median(call):.3f} ms; subsequences per frame {min(s[1] for s in stats)}..{max(s[1] for s in stats)} of "
                     f"{stats[0][2]} bits, rounds per frame {min(s[0] for s in stats)}..{max(s[0] for s in stats)}")
        rows.append((f"jpeg q{quality}", nbytes, jp[0], float(np.median(up)), float(np.median(ker)), None, jp[1], f"{int(np.mean([s[1] for s in stats]))}", f"{max(s[0] for s in stats)}"))
    name = info["name"].strip() or "no marketing name from the runtime"
    lines = ["# STEREO_FISHEYE intake: one unit of 8 key frames (16 fisheye frames of 1280 x 1024 -> 64 views of 600 x 312), fp16", "",
             f"device: {name} ({info['n_cu']} CUs, {info['clock_mhz']} MHz); medians of {a.reps} units", "",
             "| way | bytes uploaded | unit on the SuperPoint stream ms | upload ms | decode kernels ms | flatten ms | calling thread in enqueue ms | subsequences / frame | rounds (max) |",
             "|---|---|---|---|---|---|---|---|---|"]
    flatten_ms = rows[1][5]
    for w, b, unit_ms, up_ms, dec_ms, f_ms, call_ms, nsub, rounds in rows:
        lines.append(f"| {w} | {b} | {unit_ms:.3f} | {up_ms:.3f} | {dec_ms:.3f} | {(flatten_ms if f_ms is None else f_ms):.3f} | {call_ms:.3f} | {nsub} | {rounds} |")
    lines += ["", "upload ms: views / raw pixels = the unit minus the same unit with its input already in HBM; jpeg = the stand-alone decoder's upload.  flatten ms: the unit from frames in HBM "
              "minus the unit from views in HBM (the same two launches in all raw ways).", ""] + [f"- {n}" for n in notes] + [""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    ctx.host_free(flat)
    for r in raw:
        ctx.host_free(r)
    lc.close()
    for f in fl:
        f.close()


if __name__ == "__main__":
    main()
