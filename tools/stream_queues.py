#!/usr/bin/env python
"""Which HIP stream ran on which hardware queue, from a rocprofv3 kernel trace (rocpd results.db): over the same steady-state span as
tools/pipeline_busy.py (third to last MobileNetVLAD stem launch), one row per stream -- its queue(s), dispatches, kernel time, what it mostly ran --
and the groups of busy streams that share one queue (two streams on one hardware queue run strictly one after the other, csrc/stream_plan.h).

    rocprofv3 --kernel-trace -d out/q_trace -o q -- python bench.py --gpus 1 --steps 200 --warmup 32        (on the GPU box, a run of its own)
    python tools/stream_queues.py out/q_trace/*/q_results.db "label" > out/q_queues.md
"""
import sqlite3
import sys
from collections import Counter, defaultdict

ROLES = (("conv3x3", "SuperPoint"), ("sp_", "SuperPoint"), ("vlad", "MobileNetVLAD"), ("ip_scan", "detector"), ("topk", "detector"), ("bf_", "matcher"))
BUSY_SHARE = 0.01          # a stream counts as busy when it holds at least this share of the span's kernel time


def pick(cols, *names):
    for n in names:
        if n in cols:
            return n
    return None


def role_of(names):
    votes = Counter()
    for name, t in names.items():
        for key, role in ROLES:
            if key in name:
                votes[role] += t
                break
    return votes.most_common(1)[0][0] if votes else "other"


def main(db, label):
    con = sqlite3.connect(db)
    cur = con.execute("select * from kernels limit 1")
    cols = [d[0].lower() for d in cur.description]
    s_col, q_col = pick(cols, "stream_id", "stream"), pick(cols, "queue_id", "queue")
    print(f"# streams and hardware queues {label}\n")
    print(f"source: `{db}`; columns of `kernels`: {', '.join(cols)}\n")
    if not s_col or not q_col:
        print("no stream / queue column in this trace")
        return 1
    rows = con.execute(f"select name, start, end, {s_col}, {q_col} from kernels order by start").fetchall()
    stem = [r for r in rows if "vlad_stem_b0" in r[0]]
    t0, t1 = stem[2][1], stem[-1][1]
    per = defaultdict(lambda: {"queues": Counter(), "n": 0, "t": 0, "names": Counter()})
    for name, s, e, stream, queue in rows:
        if t0 <= s < t1:
            p = per[stream]
            p["queues"][queue] += 1
            p["n"] += 1
            p["t"] += e - s
            p["names"][name[:60]] += e - s
    total = sum(p["t"] for p in per.values()) or 1
    print(f"span {(t1 - t0) / 1e6:.3f} ms, {len(stem) - 3} units, {sum(p['n'] for p in per.values())} dispatches on {len(per)} streams and "
          f"{len({q for p in per.values() for q in p['queues']})} queues\n")
    print("| stream | queue(s) | dispatches | kernel ms | share | mostly | top kernel |")
    print("|---|---|---|---|---|---|---|")
    on_queue = defaultdict(list)
    for stream, p in sorted(per.items(), key=lambda kv: -kv[1]["t"]):
        qs = ", ".join(f"{q}" + (f" x{n}" if len(p["queues"]) > 1 else "") for q, n in p["queues"].most_common())
        busy = p["t"] / total >= BUSY_SHARE
        print(f"| {stream} | {qs} | {p['n']} | {p['t'] / 1e6:.3f} | {p['t'] / total * 100:.1f} % | {role_of(p['names'])} | `{p['names'].most_common(1)[0][0]}` |")
        if busy:
            for q in p["queues"]:
                on_queue[q].append(stream)
    # the span above holds the host barriers between the bench's warm-up, priming and timed run() calls; the last 20 units lie inside the timed one
    if len(stem) > 24:
        a, b = stem[-21][1], stem[-1][1]
        sel = sorted((r[1], r[2]) for r in rows if a <= r[1] < b)
        busy, (cs, ce), gaps = 0, sel[0], []
        for s, e in sel[1:]:
            if s > ce:
                busy += ce - cs
                gaps.append(s - ce)
                cs, ce = s, e
            else:
                ce = max(ce, e)
        busy += ce - cs
        big = [g for g in gaps if g > 50e3]
        iv = sorted(y[1] - x[1] for x, y in zip(stem[-21:], stem[-20:]))
        print(f"\nlast 20 units: {(b - a) / 20e6:.3f} ms per unit (stem to stem: min {iv[0] / 1e6:.2f}, median {iv[10] / 1e6:.2f}, max {iv[-1] / 1e6:.2f} ms), "
              f"busy fraction {busy / (b - a):.4f}, {len(big)} gaps over 50 us ({sum(big) / 1e6:.3f} ms)")
    shared = {q: s for q, s in on_queue.items() if len(s) > 1}
    print(f"\nbusy streams (>= {BUSY_SHARE * 100:.0f} % of the kernel time): {sum(len(s) for s in on_queue.values())} on {len(on_queue)} queues")
    if shared:
        for q, s in sorted(shared.items(), key=lambda kv: str(kv[0])):
            print(f"- queue {q} is shared by streams {', '.join(str(x) for x in s)}")
    else:
        print("- no two busy streams share a queue")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""))
