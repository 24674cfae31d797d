"""Device round trip of the loop candidates' PnP RANSAC (omni_pnp_ransac_multi, csrc/pnp.hip) for C candidates of N correspondences, in one call and one call per
candidate (what the key-frame pipeline's geometry tasks do), beside the RANSAC half of geom::solve_pnp_ransac on the same candidates (g++ -O2, one thread:
tests/cpp/pnp_plan_pin.cpp `time`).  HIP events on the context's stream around each blocking call (upload, launch, download), median of --reps after one warm-up;
prints one JSON line per (inlier share, iteration limit).

    python tools/pnp_timing.py [--cands 16] [--points 200] [--shares 0.0 0.9] [--limits 100 1000] [--reps 7]
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
    ap.add_argument("--cands", type=int, default=16)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.0, 0.9])
    ap.add_argument("--limits", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import omni_loader
    omni = omni_loader.load()
    from tests import pnp_cases as Pc
    c = omni.capi
    ctx = c.Context(0)
    with tempfile.TemporaryDirectory() as td:
        pin = Pc.build_pin(td)

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
            for limit in a.limits:
                cases = [Pc.make_case(2000 + k, a.points, share, limit) for k in range(a.cands)]
                cands = [(x["X"], x["u"], limit) for x in cases]
                got = c.pnp_ransac_multi(ctx, cands)
                one_call = timed(lambda: c.pnp_ransac_multi(ctx, cands))
                per_cand = timed(lambda: [c.pnp_ransac_multi(ctx, [x]) for x in cands])
                host = [float(l.split()[1]) for l in subprocess.run([pin, "time"], input=b"".join(Pc.pack(x) for x in cases), capture_output=True, check=True).stdout.decode().splitlines()]
                print(json.dumps({"cands": a.cands, "points": a.points, "inlier_share": share, "limit": limit, "iterations": [int(g["info"][1]) for g in got],
                                  "statuses": [g["status"] for g in got], "one_call_ms_device_wall": one_call, "one_call_per_candidate_ms_device_wall_sum": per_cand,
                                  "per_candidate_wall_ms": round(per_cand[1] / a.cands, 3), "host_pnp_ransac_ms_sum_one_thread": round(sum(host), 3),
                                  "host_ms_per_candidate_median": round(float(np.median(host)), 3), "host_ms_per_candidate_max": round(max(host), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
