"""Kernel times of downsample_movie (vof_resize_area_dev) with the library's event profiler (vof_profile_*, class
"preprocess", level 6), next to the algorithmic bytes the launch reports and the resulting GB/s.

    python profiles/resize_kernels.py [--frames 64] [--size 1024] [--runs 7] [--frames-in-flight 0] [--out FILE.md]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/resize_kernels.py      (kernel names k_rs_area / k_rs_fast)

The stack is device-resident float64, as every preprocessing call receives it; "uint8" is a stack of integers 0 .. 255 in the
uint8 arithmetic, "float64" a smooth field with noise in the float64 arithmetic.  Targets 200 x 200 (scale 5.12, general path)
and 256 x 256 (scale 4, fast path).  Algorithmic bytes per frame: 8 per source pixel read once + 8 per output pixel written; the
re-read of the source row two output rows share on a fractional scale (1 / scale_y of the rows) is not counted."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STAGE = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--targets", type=int, nargs="+", default=[200, 256])
    ap.add_argument("--frames-in-flight", type=int, default=0, help="frames per launch (0: the library's choice, 16 at most)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from opticalflow_amd import _native
    T, N = a.frames, a.size
    g = torch.Generator(device="cuda").manual_seed(5)
    i = torch.arange(N, device="cuda", dtype=torch.float64)
    smooth = (120 + 90 * torch.sin(i[:, None] / 90) * torch.cos(i[None, :] / 70))[None] + \
        12 * torch.randn((T, N, N), generator=g, device="cuda", dtype=torch.float64)
    movies = {"uint8": (smooth.clamp(0, 255).floor().contiguous(), _native.RESIZE_U8), "float64": (smooth - 100.0, _native.RESIZE_F64)}
    lines = [f"{T} x {N} x {N} float64 frames, device-resident, {a.runs} runs after 2 warm-up calls, frames_in_flight {a.frames_in_flight}", "",
             "| arithmetic | target | path | launches | kernel ms median | ms min .. max | algorithmic MB | GB/s | whole call ms median |",
             "|---|---|---|---|---|---|---|---|---|"]
    with _native.Solver(N, N, 1) as s:
        for name, (movie, arithmetic) in movies.items():
            for r in a.targets:
                out = torch.empty((T, r, r), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()

                def call():
                    s.resize_area_dev(movie, out, T, r, r, arithmetic, frames_in_flight=a.frames_in_flight)
                call(); call()
                wall = []
                for _r in range(a.runs):                         # whole calls, profiler off
                    t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
                s.profile_enable(True)
                recs = []
                for _r in range(a.runs):
                    s.profile_reset()
                    call()
                    n, ms = s.profile_get("preprocess", STAGE)
                    recs.append((n, ms, s.profile_bytes("preprocess", STAGE)))
                s.profile_enable(False)
                ms = np.array([q[1] for q in recs])
                med = float(np.median(ms))
                path = "fast" if N % r == 0 else "general"
                lines.append(f"| {name} | {r} x {r} | {path} | {recs[0][0]} | {med:.3f} | {ms.min():.3f} .. {ms.max():.3f} | {recs[0][2] / 1e6:.1f} | "
                             f"{recs[0][2] / med / 1e6:.0f} | {np.median(wall):.3f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
