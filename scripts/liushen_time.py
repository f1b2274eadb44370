#!/usr/bin/env python3
"""Rate of the Liu-Shen Jacobi flow (vof_liu_shen_dev) on the device-resident benchmark texture: pixel-iterations per second
and the bytes a call has to move over its time, as a fraction of 8 TB/s.  The fusion depths (VOF_LIUSHEN_FUSE; "default" =
variable unset) alternate call by call in one session, so that clock and thermal drift hit all of them alike.
Bytes a call has to move per pixel and pair: 48 per launch (p, c, v_x, v_y in, v_x, v_y out; halo re-reads not counted) +
16 (initial fields out) + 48 (fields in, four planes out).  HIP events on the stream the library launches on.
usage: liushen_time.py [--n 1024] [--pairs 32] [--iterations 100] [--depths 1,default] [--calls 7] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--iterations", type=int, default=100)
ap.add_argument("--depths", default="1,default")
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch  # noqa: E402
from opticalflow_amd import _native, synthetic  # noqa: E402

DEFAULT_DEPTH = 4      # LS_KDEF of csrc/vof_liushen.hpp
dev = torch.device("cuda", 0)
n, P, iters = args.n, args.pairs, args.iterations
depths = args.depths.split(",")
stream = torch.cuda.current_stream(dev)
times = {d: [] for d in depths}
with _native.Solver(n, n, 1, stream=stream.cuda_stream) as solver:
    movie = synthetic.texture_stack_torch(n, P + 1, 0, dev, solver=solver)
    out = [torch.empty((P, n, n), dtype=torch.float64, device=dev) for _ in range(4)]
    for k in range(args.warmup + args.calls):
        for d in depths:
            if d == "default":
                os.environ.pop("VOF_LIUSHEN_FUSE", None)
            else:
                os.environ["VOF_LIUSHEN_FUSE"] = d
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            solver.liu_shen_dev(movie, P + 1, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0, iters, *out)
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                times[d].append(e0.elapsed_time(e1) * 1e-3)
    assert bool(torch.isfinite(out[2]).all())
rows = []
for d in depths:
    depth = DEFAULT_DEPTH if d == "default" else int(d)
    t = float(np.median(times[d]))
    launches = -(-iters // depth)
    moved = (48.0 * launches + 64.0) * P * n * n
    row = dict(depth=d, iterations_per_launch=depth, n=n, pairs=P, iterations=iters, calls=len(times[d]), median_s=t,
               min_s=float(min(times[d])), max_s=float(max(times[d])), pixel_iterations_per_s=P * n * n * iters / t,
               moved_bytes=moved, bytes_per_s=moved / t, fraction_of_8TBs=moved / t / 8e12)
    rows.append(row)
    print(json.dumps(row), flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
