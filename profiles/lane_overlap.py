#!/usr/bin/env python3
"""Concurrency of a rocprofv3 --kernel-trace CSV: summed kernel time, busy time (union of the kernels' intervals), the time
during which two or more kernels run at once, and the span from the first to the last solver kernel - per kernel class and
per hardware queue.  Compares one-lane and several-lane runs of the same command.

    python profiles/lane_overlap.py <kernel_trace.csv> [--steps N]

Only the solver's kernels (vof::) count, without the synthetic stack's generator (k_texture_*).  --steps divides the
totals (a bench run with --warmup 1 --steps 1 holds two steps).
"""
import argparse
import csv
import re
from collections import defaultdict


def klass(name):
    n = re.sub(r"\(.*", "", name).replace("void ", "").strip()
    if n.startswith("vof::k_sweep0r<2, false"):
        return "level-0 pre-smoothing pass"
    if n.startswith("vof::k_sweep0r<2, true"):
        return "level-0 post-smoothing pass"
    if n.startswith("vof::k_sweep0"):
        return "level-0 other passes"
    if n.startswith("vof::k_sweep_st") or n.startswith("vof::k_sweep<"):
        return "stored-level sweeps"
    if n.startswith("vof::k_tail_cycle"):
        return "coarse tail (k_tail_cycle)"
    if n.startswith(("vof::k_resrestrict_u", "vof::k_prolong_add", "vof::k_restrict", "vof::k_apply<", "vof::k_coarse")):
        return "coarse levels: transfer / residual / coarse solve"
    if n.startswith(("vof::k_galerkin", "vof::k_store_fine")):
        return "hierarchy set-up"
    if n.startswith(("vof::k_stream_apply0", "vof::k_stream_resrestrict0", "vof::k_apply0")):
        return "level-0 operator"
    return "vectors, reductions, scalars, epilogue"


def union(iv):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        tot += cur_e - cur_s
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()
    iv, per_class, per_queue = [], defaultdict(lambda: [0, 0]), defaultdict(lambda: [0, 0])
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "vof::" not in name or "k_texture" in name:
                continue
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            iv.append((s, e))
            c = per_class[klass(name)]
            c[0] += 1; c[1] += e - s
            q = per_queue[r.get("Queue_Id", "?")]
            q[0] += 1; q[1] += e - s
    k = a.steps
    summed = sum(e - s for s, e in iv)
    busy = union(iv)
    ev = sorted([(s, 1) for s, _ in iv] + [(e, -1) for _, e in iv])
    depth, last, multi = 0, None, 0
    for t, d in ev:
        if depth >= 2:
            multi += t - last
        depth += d
        last = t
    span = max(e for _, e in iv) - min(s for s, _ in iv)
    print(f"| per step | ms |\n|---|---:|")
    print(f"| summed kernel time | {summed / 1e6 / k:.1f} |")
    print(f"| busy time (union of the kernels' intervals) | {busy / 1e6 / k:.1f} |")
    print(f"| time with two or more kernels running | {multi / 1e6 / k:.1f} |")
    print(f"| span of the solver's kernels (incl. gaps) | {span / 1e6 / k:.1f} |")
    print(f"| idle inside the span (host waits, launch gaps) | {(span - busy) / 1e6 / k:.1f} |")
    print(f"\n{len(iv)} dispatches.\n\n| kernel class | calls per step | summed ms per step |\n|---|---:|---:|")
    for name, (n, d) in sorted(per_class.items(), key=lambda kv: -kv[1][1]):
        print(f"| {name} | {n / k:.0f} | {d / 1e6 / k:.1f} |")
    print("\n| hardware queue | calls per step | summed ms per step |\n|---|---:|---:|")
    for q, (n, d) in sorted(per_queue.items()):
        print(f"| {q} | {n / k:.0f} | {d / 1e6 / k:.1f} |")


if __name__ == "__main__":
    main()
