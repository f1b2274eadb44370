#!/usr/bin/env python3
"""Times of the blur sweep (vary_blursize, stats only: 145 sigmas of np.arange(0.5, 15, 0.1), box 21, 50 speed and 50
direction bins) against the loop it replaces, conduct_optical_flow(..., smoothing_sigma=s) once per sigma with output="numpy"
and with output="torch", on a float64 texture stack of --frames x n x n; and of the blur alone, tiled against k_blur1d, per
radius.

The loop is the parent commit's: the sweep adds entry points, and the one thing it changes on the path of conduct_optical_flow,
the kernel the blur takes, is switched back with VOF_BLUR_TILED=0 while the loop runs.  The loop is timed without the numpy
reductions the scripts do on its results (a lower bound of what it replaces).  The three are run in turn, --rounds times, and
the median of each is reported with its spread; every timed region ends with a device synchronise and is taken with the host
clock.  The blur is timed with events around --blur-reps calls of vof_blur_stack_dev on 16 frames, the two kernels in turn.
usage: gpu_blursweep_rate.py [--n 512] [--frames 17] [--rounds 5] [--blur-reps 20] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--frames", type=int, default=17)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--blur-reps", type=int, default=20)
ap.add_argument("--skip-loops", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch  # noqa: E402
from opticalflow_amd import _native, optical_flow as of, synthetic  # noqa: E402

dev = torch.device("cuda", 0)
n, T = args.n, args.frames
sigmas = np.arange(0.5, 15, 0.1)
rows = []


def report(**row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


with _native.Solver(n, n, 1) as solver:
    movie_dev = synthetic.texture_stack_torch(n, T, 0, dev, solver=solver)
    torch.cuda.synchronize(dev)
movie = movie_dev.cpu().numpy()
kw = dict(boxsize=21, histogram_bins=50, histogram_range=(0.0, 5.0), angle_bins=50)


def sweep_numpy():
    of.vary_blursize(movie, sigmas, **kw)


def sweep_torch():
    of.vary_blursize(movie_dev, sigmas, output="torch", **kw)


def loop(arg, output):
    os.environ["VOF_BLUR_TILED"] = "0"
    try:
        for s in sigmas:
            res = of.conduct_optical_flow(arg, 21, smoothing_sigma=float(s), output=output)
            del res
    finally:
        del os.environ["VOF_BLUR_TILED"]


kinds = [("sweep_numpy", sweep_numpy), ("sweep_torch", sweep_torch)]
if not args.skip_loops:
    kinds += [("loop_numpy", lambda: loop(movie, "numpy")), ("loop_torch", lambda: loop(movie_dev, "torch"))]
times = {k: [] for k, _ in kinds}
for r in range(args.rounds + 1):                 # round 0 warms up
    for k, fn in kinds:
        t = timed(fn)
        if r:
            times[k].append(t)
for k, _ in kinds:
    report(kind=k, n=n, frames=T, sigmas=int(sigmas.size), rounds=len(times[k]), median_s=float(np.median(times[k])),
           min_s=float(min(times[k])), max_s=float(max(times[k])))
if not args.skip_loops:
    for out in ("numpy", "torch"):
        report(ratio=f"loop_{out} / sweep_{out}", value=float(np.median(times["loop_" + out]) / np.median(times["sweep_" + out])))

# the blur alone: 16 frames, tiled (where the radius allows it) and k_blur1d in turn
stream = torch.cuda.current_stream(dev)
with _native.Solver(n, n, 1, stream=stream.cuda_stream) as solver:
    src = movie_dev[:1].repeat(16, 1, 1).contiguous()
    dst = torch.empty_like(src)
    for radius in (2, 10, 24, 48, 60, 64):
        taps = of.gaussian_taps(radius / 4.0)
        assert taps.size == 2 * radius + 1
        per = {"tiled": [], "k_blur1d": []}
        for r in range(args.rounds + 1):
            for which in per:
                os.environ["VOF_BLUR_TILED"] = "1" if which == "tiled" else "0"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.blur_reps):
                    solver.blur_dev(src, dst, 16, taps)
                e1.record(stream)
                e1.synchronize()
                if r:
                    per[which].append(e0.elapsed_time(e1) * 1e3 / args.blur_reps)
        del os.environ["VOF_BLUR_TILED"]
        report(kind="blur", n=n, frames=16, radius=radius, tiled_us=float(np.median(per["tiled"])),
               k_blur1d_us=float(np.median(per["k_blur1d"])), tiled_min_us=float(min(per["tiled"])),
               k_blur1d_min_us=float(min(per["k_blur1d"])))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
