#!/usr/bin/env python3
"""Times the 4-DoF pose-graph solver (csrc/pgo.hip, csrc/pgo_plan.h) on one commit: omni_pgo_solve_multi -- the device time between two events around the launch and
the wall time of the call (upload, launch, download) -- against omni_pgo_solve_host on one thread of the same machine, on graphs of 2 x 50, 5 x 50 and 16 x 256 poses
(tests/pgo_cases.py: noisy ego motion, 4 loops per drone, a quarter of them outliers) with 1, 8 and 64 starts (start k is the integrated odometry displaced by
k x 1 cm / 0.1 degree of noise), the results compared bit for bit.  Each figure, the host's included, is the median of --reps calls after one warm-up call; a host figure marked "(one call)" is a single call, taken where
--reps + 1 of them would exceed the host budget.  The largest graph runs under
caps (3 outer iterations, 500 conjugate-gradient steps per linear solve): a whole solve of it is not what the library promises.  The host's time for many starts is
measured when one start takes under --host-budget seconds / starts, and otherwise given as starts x the time of one.

    python tools/pgo_timing.py [--out profiles/pgo_timing.md] [--reps 3] [--host-budget 30]

Records figures; gates nothing."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2, 50, {}), (5, 50, {}), (16, 256, dict(max_iterations=3, max_cg_iterations=500)))
STARTS = (1, 8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgo_timing.md"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-budget", type=float, default=30.0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import omni_loader
    omni = omni_loader.load()
    from tests import pgo_cases as PC
    c = omni.capi
    ctx = c.Context(0)
    pgo = c.Pgo(ctx)
    lines = ["# Pose-graph solver: the GPU against one host thread", "", f"Device: {ctx.device_info()}", "",
             "| poses | edges | starts | outer its (start 0) | CG steps (start 0) | CG steps (all) | kernel ms | call ms | host ms | host / call |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for drones, length, kw in SIZES:
        g = PC.Graph(100 + drones, drones=drones, length=length, loops=4 * drones, outliers=drones)
        pr = c.pgo_params(**kw)
        rng = np.random.default_rng(drones)
        host_one = None
        for K in STARTS:
            starts = np.stack([g.init + k * np.array([0.01, 0.01, 0.01, 0.00175]) * rng.normal(size=g.init.shape) for k in range(K)])
            starts[:, 0] = g.init[0]
            kern, wall = [], []
            for rep in range(args.reps + 1):
                t = time.perf_counter()
                got = pgo.solve(starts, g.fixed, g.edges, pr, time_kernel=True)
                if rep:
                    wall.append((time.perf_counter() - t) * 1e3)
                    kern.append(pgo.last_kernel_us / 1e3)
            measured = host_one is None or host_one * K <= args.host_budget * 1e3
            if measured:
                hosts = []
                for rep in range(args.reps + 1 if host_one is None or host_one * K * (args.reps + 1) <= args.host_budget * 1e3 else 1):
                    t = time.perf_counter()
                    want = c.pgo_solve_host(starts, g.fixed, g.edges, pr)
                    hosts.append((time.perf_counter() - t) * 1e3)
                host = float(np.median(hosts[1:])) if len(hosts) > 1 else hosts[0]
                single = len(hosts) == 1
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2], "the GPU and the host build differ"
                if K == 1:
                    host_one = host
            else:
                host, single = host_one * K, False
            st = got[1]
            lines.append(f"| {drones} x {length} | {len(g.edges)} | {K} | {st[0]['iterations']} | {st[0]['cg_iterations']} | {int(st['cg_iterations'].sum())} | "
                         f"{np.median(kern):.2f} | {np.median(wall):.2f} | {host:.1f}{'' if measured else ' (starts x one)'}{' (one call)' if single else ''} | {host / np.median(wall):.2f} |")
            print(lines[-1], flush=True)
    lines += ["", "kernel ms: between two events around the launch.  call ms: omni_pgo_solve_multi as the caller sees it.  host ms: omni_pgo_solve_host, one thread, the same",
              "starts one after the other, the median taken as for the GPU unless marked.  Every measured row's poses, costs, counts and statuses equal the host build's bit for bit.", ""]
    pgo.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
