#!/usr/bin/env python3
"""Times of the two-channel comparison (compare_channel_flows, stats only, the reference script's arguments: box 31, sigma 3,
50 speed / 50 direction / 50 relative-angle and 50 x 50 joint speed bins) on two float64 texture stacks of --frames x n x n,
against the composition it replaces: conduct_optical_flow once per channel (output="numpy": six field stacks come to the host)
and the numpy post-processing of tests/compare_restatement.py on them.

The two are run in turn, --rounds times after a warm-up at --warm-frames frames, every timed region ends with a device
synchronise and is taken with the host clock; the baseline's two phases are reported separately.  The device-resident entry
(output="torch", movies already on the device) is timed as well.  --new-only skips the baseline (for a kernel trace: the
bytes the joint kernel reads are 48 per pixel and pair, printed here as joint_bytes).
usage: gpu_compare_rate.py [--n 1024] [--frames 256] [--rounds 2] [--warm-frames 5] [--new-only] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--warm-frames", type=int, default=5)
ap.add_argument("--new-only", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch  # noqa: E402
from opticalflow_amd import _native, optical_flow as of, synthetic  # noqa: E402
from compare_restatement import compare_summaries  # noqa: E402

dev = torch.device("cuda", 0)
n, T = args.n, args.frames
rows = []


def report(**row):
    rows.append(row)
    print(json.dumps(row), flush=True)


with _native.Solver(n, n, 1) as solver:
    movies_dev = [synthetic.texture_stack_torch(n, T, seed, dev, solver=solver) for seed in (0, 1)]
    torch.cuda.synchronize(dev)
movies = [m.cpu().numpy() for m in movies_dev]
BINS = dict(histogram_bins=50, histogram_range=(0.0, 2.0), angle_bins=50, relative_angle_bins=50, joint_speed_bins=(50, 50),
            joint_speed_ranges=((0.0, 2.0), (0.0, 2.0)), joint_speed_min_b=0.1)
timings = {}


def timed(kind, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    timings.setdefault(kind, []).append(time.perf_counter() - t0)
    return out


def new_numpy(frames):
    return of.compare_channel_flows(movies[0][:frames], movies[1][:frames], 31, smoothing_sigma=3, **BINS)


def new_torch(frames):
    return of.compare_channel_flows(movies_dev[0][:frames], movies_dev[1][:frames], 31, smoothing_sigma=3, output="torch", **BINS)


def baseline(frames, record):
    def flows():
        return [of.conduct_optical_flow(m[:frames], 31, smoothing_sigma=3) for m in movies]
    two = timed("baseline_flows", flows) if record else flows()

    def post():
        return compare_summaries(two[0], two[1], **BINS)
    return timed("baseline_numpy", post) if record else post()


# warm-up: code objects, the context and its scratch, at a size that costs nothing
warm_new, warm_dev = new_numpy(args.warm_frames), new_torch(args.warm_frames)
if not args.new_only:
    warm_old = baseline(args.warm_frames, False)
    differ = [k for k in ("speed_histograms", "angle_histograms", "relative_angle_histogram", "joint_speed_histogram", "nonfinite_counts",
                          "joint_nonfinite_count", "relative_angle_dropped")
              if not np.array_equal(warm_new[k], warm_old[k]) or not np.array_equal(warm_dev[k], warm_old[k])]
    report(kind="warm-up", frames=args.warm_frames, integer_summaries_that_differ=differ)

for r in range(args.rounds):
    res = timed("new_numpy", lambda: new_numpy(T))
    timed("new_torch", lambda: new_torch(T))
    if not args.new_only:
        old = baseline(T, True)
        if r == 0:
            report(kind="check", relative_angle_histograms_equal=bool(np.array_equal(res["relative_angle_histogram"],
                                                                                     old["relative_angle_histogram"])),
                   joint_speed_histograms_equal=bool(np.array_equal(res["joint_speed_histogram"], old["joint_speed_histogram"])),
                   dropped=[res["relative_angle_dropped"], old["relative_angle_dropped"]])
        del old
for k, v in timings.items():
    report(kind=k, n=n, frames=T, rounds=len(v), median_s=float(np.median(v)), min_s=float(min(v)), max_s=float(max(v)))
if not args.new_only:
    old_s = np.median(timings["baseline_flows"]) + np.median(timings["baseline_numpy"])
    report(ratio="baseline / new_numpy", baseline_s=float(old_s), value=float(old_s / np.median(timings["new_numpy"])))
report(joint_bytes=48.0 * (T - 1) * n * n, pairs=T - 1)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
