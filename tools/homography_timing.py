"""Device time of the loop-verification round trip (omni_bf_match_homography_multi: matcher + flag filter + homography RANSAC, csrc/homography.hip) for P pairs of
N key points, beside the matcher alone (omni_bf_match_multi), the RANSAC kernel alone on the same point lists (omni_homography_ransac_multi), and the host's
geom::find_homography_ransac on the same pairs (g++ -O2, one thread: tests/cpp/ransac_plan_pin.cpp `time`).  HIP events on the context's stream around each
blocking call (upload, launches, download), median of --reps after one warm-up; prints one JSON line per inlier share.

    python tools/homography_timing.py [--pairs 16] [--points 200] [--shares 0.0 0.9] [--reps 7]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.0, 0.9])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import omni_loader
    omni = omni_loader.load()
    from tests import homography_cases as Hc
    from tests.test_gpu_bf_homography import make_pair
    c = omni.capi
    ctx = c.Context(0)
    with tempfile.TemporaryDirectory() as td:
        pin = Hc.build_pin(td)

        def timed(f):
            f()
            dev, wall = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.timer_start()
                f()
                dev.append(ctx.timer_stop())
                wall.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(dev)), 3), round(float(np.median(wall)), 3)

        for share in a.shares:
            pairs = [make_pair(omni, 1000 + p, a.points, a.points, "none", share) for p in range(a.pairs)]
            got = c.bf_match_homography_multi(ctx, pairs)
            lists = [(p[3][g["t_idx"][g["kept"]]], p[2][g["q_idx"][g["kept"]]]) for p, g in zip(pairs, got)]
            fused = timed(lambda: c.bf_match_homography_multi(ctx, pairs))
            match = timed(lambda: c.bf_match_multi(ctx, [(p[0], p[1]) for p in pairs]))
            kernel = timed(lambda: c.homography_ransac_multi(ctx, lists))
            cases = [{"q_idx": g["q_idx"], "t_idx": g["t_idx"], "q_xy": p[2], "t_xy": p[3], "flags": p[4]} for p, g in zip(pairs, got)]
            host = [float(l.split()[1]) for l in subprocess.run([pin, "time"], input=b"".join(Hc.pack(x) for x in cases), capture_output=True, check=True).stdout.decode().splitlines()]
            print(json.dumps({"pairs": a.pairs, "points": a.points, "inlier_share": share, "matches_kept": [len(g["kept"]) for g in got],
                              "iterations": [int(g["info"][1]) for g in got], "statuses": [g["status"] for g in got],
                              "fused_ms_device_wall": fused, "matcher_alone_ms_device_wall": match, "ransac_alone_ms_device_wall": kernel,
                              "host_find_homography_ms_sum_one_thread": round(sum(host), 3), "host_ms_per_pair_max": round(max(host), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
