#!/usr/bin/env python3
"""The sweeps between two visits of the W-cycle's revisited level, from rocprofv3 output (profiles/r17_revisit_summary.md).

Two k_sweep_st launches that follow each other on one queue with nothing in between are the post-smoothing sweep of one visit
and the pre-smoothing sweep of the next (every other sweep of a stored level is followed by k_resrestrict_u, k_prolong_add or a
level-0 pass); k_sweep_st2 is the pass that replaces such a pair.

    python profiles/revisit_launches.py trace <kernel_trace.csv>          times, us
    python profiles/revisit_launches.py pmc <counter_collection.csv>      the counter of a --pmc run, per launch
"""
import csv
import re
import sys
from collections import defaultdict
from statistics import median


def short(name):
    return re.sub(r"\(.*", "", name).replace("void ", "").replace("vof::", "").strip()


def rows_of(mode, path):
    """per queue: (order key, kernel, grid in threads, value) in launch order"""
    per_queue = defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            if mode == "trace":
                grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1)
                t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                per_queue[r.get("Queue_Id", "?")].append((t0, short(r["Kernel_Name"]), grid, (t1 - t0) / 1e3))
            else:
                per_queue[r.get("Queue_Id", "?")].append((int(r["Dispatch_Id"]), short(r["Kernel_Name"]), int(r["Grid_Size"]),
                                                         float(r["Counter_Value"])))
    for q in per_queue.values():
        q.sort()
    return per_queue


def main():
    mode, path = sys.argv[1], sys.argv[2]
    per_queue = rows_of(mode, path)
    total = sum(v for q in per_queue.values() for _, _, _, v in q)
    single = defaultdict(list)     # (kernel, grid) -> values of every launch
    pairs = defaultdict(list)      # (grid of the first, grid of the second) -> (first, second)
    fused = defaultdict(list)      # grid -> values
    for q in per_queue.values():
        i = 0
        while i < len(q):
            _, name, grid, v = q[i]
            if name.startswith("k_sweep_st2<"):
                fused[grid].append(v)
            elif name.startswith("k_sweep_st<"):
                single[(name, grid)].append(v)
                if i + 1 < len(q) and q[i + 1][1].startswith("k_sweep_st<"):
                    single[(q[i + 1][1], q[i + 1][2])].append(q[i + 1][3])
                    pairs[(grid, q[i + 1][2])].append((v, q[i + 1][3]))
                    i += 1
            i += 1
    unit = "us" if mode == "trace" else "counter"
    print(f"all kernels: {total:.1f} {unit}")
    print(f"\n| k_sweep_st launches | grid (threads) | launches | total | median |\n|---|---:|---:|---:|---:|")
    for (name, grid), v in sorted(single.items(), key=lambda kv: -sum(kv[1])):
        print(f"| `{name}` | {grid} | {len(v)} | {sum(v):.1f} | {median(v):.1f} |")
    print(f"\n| back-to-back pairs: grids | pairs | total | median first | median second | median of the sum |\n|---|---:|---:|---:|---:|---:|")
    for (ga, gb), v in sorted(pairs.items(), key=lambda kv: -sum(a + b for a, b in kv[1])):
        print(f"| {ga} + {gb} | {len(v)} | {sum(a + b for a, b in v):.1f} | {median(a for a, _ in v):.1f} | {median(b for _, b in v):.1f} | "
              f"{median(a + b for a, b in v):.1f} |")
    print(f"\n| k_sweep_st2: grid | launches | total | median |\n|---|---:|---:|---:|")
    for grid, v in sorted(fused.items(), key=lambda kv: -sum(kv[1])):
        print(f"| {grid} | {len(v)} | {sum(v):.1f} | {median(v):.1f} |")


if __name__ == "__main__":
    main()
