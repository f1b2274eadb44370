#!/usr/bin/env python3
"""Rate of the box least-squares flow (vof_box_flow_dev) on the device-resident benchmark texture: pairs/s and the bytes a
call has to move (one frame in + 3 or 4 planes out per pixel and pair) over its time, as a fraction of 8 TB/s; fused LDS
kernel and general three-kernel path (VOF_BOXFLOW_FUSED=0), boxes 15 and 31, with and without the remodelling term.
HIP events on the stream the library launches on; warm-up + timed calls.
usage: gpu_boxflow_rate.py [--n 1024] [--frames 256] [--calls 10] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch  # noqa: E402
from opticalflow_amd import _native, synthetic  # noqa: E402

dev = torch.device("cuda", 0)
n, T = args.n, args.frames
stream = torch.cuda.current_stream(dev)
rows = []
with _native.Solver(n, n, 1, stream=stream.cuda_stream) as solver:
    movie = synthetic.texture_stack_torch(n, T, 0, dev, solver=solver)
    out = [torch.empty((T - 1, n, n), dtype=torch.float64, device=dev) for _ in range(4)]
    for path in ("fused", "general"):
        os.environ["VOF_BOXFLOW_FUSED"] = "1" if path == "fused" else "0"
        for box in (15, 31):
            for rem in (False, True):
                times = []
                for k in range(args.warmup + args.calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    solver.box_flow_dev(movie, T, box, 1.0, 1.0, rem, True, out[0], out[1], out[2], out[3] if rem else None)
                    e1.record(stream)
                    e1.synchronize()
                    if k >= args.warmup:
                        times.append(e0.elapsed_time(e1) * 1e-3)
                t = float(np.median(times))
                moved = (T * n * n + (4 if rem else 3) * (T - 1) * n * n) * 8.0
                row = dict(path=path, box=box, remodelling=rem, n=n, frames=T, calls=len(times), median_s=t,
                           min_s=float(min(times)), max_s=float(max(times)), pairs_per_s=(T - 1) / t, moved_bytes=moved,
                           fraction_of_8TBs=moved / t / 8e12)
                rows.append(row)
                print(json.dumps(row), flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
