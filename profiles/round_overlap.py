#!/usr/bin/env python3
"""Rounds of a rocprofv3 --kernel-trace CSV: every hardware queue's sequence of solver kernels cut into rounds (one BiCGStab
iteration of a batch: two multigrid cycles plus the vector kernels) at its k_update_xr launches, and how much of the
under-filled rounds another queue's dense rounds cover (profiles/r06_lane_groups_summary.md).

    python profiles/round_overlap.py <kernel_trace.csv> [--steps N] [--straggler 0.10] [--quiet] [--launches]

A round is the kernels of a queue after one k_update_xr up to and including the next (the first round of a batch also
holds the hierarchy set-up and the epilogue of the batch before it; what follows a queue's last k_update_xr is listed as
"tail").  Launches of a round cover only the pairs still active, so the duration of its k_update_xr relative to the
queue's longest is a proxy for the share of pairs the round serves.  A round below --straggler on that proxy is a straggler
round.  Its wall span counts as covered where a round that is not a straggler is under way on another queue.

Only the solver's kernels (vof::) count, without the synthetic stack's generator (k_texture_*).  --steps divides the
per-step totals (a bench run with --warmup 1 --steps 1 holds two steps).  --launches adds the launches of the straggler rounds
per (kernel, grid in threads): count and minimum / median / maximum duration (profiles/r16_active_list_summary.md).
"""
import argparse
import csv
import re
import statistics
from collections import defaultdict


def rounds_of(kernels):
    """kernels: (start, end, name) sorted by start.  -> list of dicts, one per round."""
    out, cur = [], []
    for k in kernels:
        s, e, name = k[:3]
        cur.append(k)
        if "k_update_xr" in name:
            out.append({"iv": cur, "upd": e - s})
            cur = []
    if cur:
        out.append({"iv": cur, "upd": None})
    for r in out:
        r["start"] = min(k[0] for k in r["iv"])
        r["end"] = max(k[1] for k in r["iv"])
        r["sum"] = sum(k[1] - k[0] for k in r["iv"])
    return out


def merged(iv):
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def overlap(s, e, cover):
    return sum(max(0, min(e, b) - max(s, a)) for a, b in cover)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--straggler", type=float, default=0.10)
    ap.add_argument("--quiet", action="store_true", help="totals only, no per-round table")
    ap.add_argument("--launches", action="store_true", help="the straggler rounds' launches per (kernel, grid)")
    a = ap.parse_args()
    per_queue = defaultdict(list)
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "vof::" not in name or "k_texture" in name:
                continue
            grid = "x".join(r.get("Grid_Size_" + d, "?") for d in "XYZ")
            per_queue[r.get("Queue_Id", "?")].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, grid))
    t0 = min(k[0] for ks in per_queue.values() for k in ks)
    rounds = {}
    for q, ks in per_queue.items():
        ks.sort()
        rs = rounds_of(ks)
        longest = max((r["upd"] for r in rs if r["upd"] is not None), default=1)
        for r in rs:
            r["share"] = None if r["upd"] is None else r["upd"] / longest
            r["straggler"] = r["share"] is not None and r["share"] < a.straggler
        rounds[q] = rs
    dense = {q: merged([(r["start"], r["end"]) for r in rs if r["share"] is not None and not r["straggler"]])
             for q, rs in rounds.items()}
    tot_span = tot_sum = tot_cov = 0
    n_str = 0
    if not a.quiet:
        print("| queue | round | start ms | wall span ms | summed kernel ms | launches | k_update_xr ms | share of the queue's longest | straggler | covered ms |")
        print("|---|---:|---:|---:|---:|---:|---:|---:|---|---:|")
    for q in sorted(rounds):
        cover = merged([iv for p, ivs in dense.items() if p != q for iv in ivs])
        for i, r in enumerate(rounds[q]):
            span = r["end"] - r["start"]
            cov = overlap(r["start"], r["end"], cover) if r["straggler"] else 0
            if r["straggler"]:
                tot_span += span; tot_sum += r["sum"]; tot_cov += cov; n_str += 1
            if not a.quiet:
                upd = "tail" if r["upd"] is None else f"{r['upd'] / 1e6:.3f}"
                share = "" if r["share"] is None else f"{100 * r['share']:.1f} %"
                tail = f"yes | {cov / 1e6:.2f}" if r["straggler"] else " | "
                print(f"| {q} | {i} | {(r['start'] - t0) / 1e6:.1f} | {span / 1e6:.2f} | {r['sum'] / 1e6:.2f} | {len(r['iv'])} | {upd} | {share} | {tail} |")
    k = a.steps
    all_iv = [(x[0], x[1]) for ks in per_queue.values() for x in ks]
    span_all = max(e for _, e in all_iv) - min(s for s, _ in all_iv)
    print(f"\n| per step ({k} steps in the trace) | |\n|---|---:|")
    print(f"| queues with solver kernels | {len(rounds)} |")
    print(f"| rounds | {sum(len(rs) for rs in rounds.values()) / k:.1f} |")
    print(f"| straggler rounds (k_update_xr below {100 * a.straggler:.0f} % of the queue's longest) | {n_str / k:.1f} |")
    print(f"| wall span of the straggler rounds, ms | {tot_span / 1e6 / k:.2f} |")
    print(f"| summed kernel time of the straggler rounds, ms | {tot_sum / 1e6 / k:.2f} |")
    print(f"| of the wall span: covered by a dense round of another queue, ms | {tot_cov / 1e6 / k:.2f} |")
    print(f"| of the wall span: not covered, ms | {(tot_span - tot_cov) / 1e6 / k:.2f} |")
    print(f"| first to last solver kernel, ms (all steps, with the gaps between them) | {span_all / 1e6:.1f} |")
    if a.launches:
        by = defaultdict(list)
        for rs in rounds.values():
            for r in rs:
                if r["straggler"]:
                    for s, e, name, grid in r["iv"]:
                        by[(re.sub(r"\(.*", "", name).replace("void ", "").replace("vof::", "").strip()[:70], grid)].append(e - s)
        print("\n| kernel (straggler rounds) | grid (threads) | launches | total ms | min us | median us | max us |")
        print("|---|---|---:|---:|---:|---:|---:|")
        for (name, grid), d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
            print(f"| `{name}` | {grid} | {len(d)} | {sum(d) / 1e6:.3f} | {min(d) / 1e3:.1f} | {statistics.median(d) / 1e3:.1f} | {max(d) / 1e3:.1f} |")


if __name__ == "__main__":
    main()
