#!/usr/bin/env python3
"""Rate of the box-size sweep (vof_vary_boxsize_dev, stats only) on the device-resident benchmark texture against the loop
it replaces: conduct_optical_flow(..., output="torch") once per box size.  boxsizes = np.arange(5, 150, 2) (the 73 sizes of
the reference's compare_rho_and_actin.py:387), with and without the remodelling term.  The sweep is timed with HIP events
on the stream the library launches on, the loop with the host clock around a device synchronise (it runs on the cached
context's own stream); warm-up + timed calls, median and spread.  Both clocks bracket a call that blocks the host until
the device is done, so the two ways of timing differ by microseconds on calls of seconds.
The loop runs in this checkout, not in the parent commit: vary_boxsize adds entry points and leaves the path of
conduct_optical_flow (box_flow_pairs and its kernels) as the parent has it, so the loop here is the parent's loop.
usage: gpu_boxsweep_rate.py [--n 1024] [--frames 256] [--calls 5] [--warmup 2] [--loop-calls 5] [--loop-warmup 2] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--loop-calls", type=int, default=5)
ap.add_argument("--loop-warmup", type=int, default=2)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch  # noqa: E402
from opticalflow_amd import _native, optical_flow, synthetic  # noqa: E402

dev = torch.device("cuda", 0)
n, T = args.n, args.frames
boxes = np.arange(5, 150, 2)
stream = torch.cuda.current_stream(dev)
rows = []


def summary(kind, rem, times):
    t = float(np.median(times))
    row = dict(kind=kind, remodelling=rem, n=n, frames=T, boxes=int(boxes.size), calls=len(times), median_s=t,
               min_s=float(min(times)), max_s=float(max(times)), ms_per_pair=1e3 * t / (T - 1))
    rows.append(row)
    print(json.dumps(row), flush=True)
    return t


with _native.Solver(n, n, 1, stream=stream.cuda_stream) as solver:
    movie = synthetic.texture_stack_torch(n, T, 0, dev, solver=solver)
    for rem in (False, True):
        times = []
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            stats, _hist, _probes = solver.vary_boxsize_dev(movie, T, boxes, 1.0, 1.0, rem, True)
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                times.append(e0.elapsed_time(e1) * 1e-3)
        t_sweep = summary("sweep", rem, times)
        times = []
        for k in range(args.loop_warmup + args.loop_calls):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for box in boxes:
                res = optical_flow.conduct_optical_flow(movie, int(box), include_remodelling=rem, output="torch")
                del res
            torch.cuda.synchronize(dev)
            if k >= args.loop_warmup:
                times.append(time.perf_counter() - t0)
        t_loop = summary("loop", rem, times)
        print(json.dumps(dict(remodelling=rem, loop_over_sweep=t_loop / t_sweep)), flush=True)
        rows.append(dict(remodelling=rem, loop_over_sweep=t_loop / t_sweep))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
