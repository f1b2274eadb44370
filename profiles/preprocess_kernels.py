"""Per-kernel times of apply_clahe and apply_adaptive_threshold with the library's event profiler (vof_profile_*, class
"preprocess", level = stage), next to the algorithmic bytes each kernel reports and the resulting TB/s.

    python profiles/preprocess_kernels.py [--frames 32] [--size 1024] [--runs 7] [--out FILE.md]

The stack is device-resident; the arguments are the reference scripts': tile_number=10, clipLimit=50000, window_size=151,
threshold=-5.  Every run is one call of each function after two warm-up calls; the table gives the median and the spread."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STAGES = ["range", "row sums", "threshold", "histograms", "tables", "blend"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from opticalflow_amd import _native, optical_flow as of
    T, N = a.frames, a.size
    g = torch.Generator(device="cuda").manual_seed(5)
    i = torch.arange(N, device="cuda", dtype=torch.float64)
    movie = (20000 + 15000 * torch.sin(i[:, None] / 90) * torch.cos(i[None, :] / 70))[None] + \
        3000 * torch.randn((T, N, N), generator=g, device="cuda", dtype=torch.float64)
    movie = movie.clamp_(0, 65535).floor_().contiguous()
    tiles = of.clahe_tile_grid((T, N, N), 10)
    clahed = torch.empty_like(movie)
    mask = torch.empty((T, N, N), dtype=torch.bool, device="cuda")
    lines = []
    with _native.Solver(N, N, 1) as s:
        def clahe():
            s.clahe_dev(movie, clahed, T, 50000.0, tiles[0], tiles[1])

        def threshold():
            s.adaptive_threshold_dev(clahed, mask, T, 151, -5.0)
        calls = {"apply_clahe": (clahe, (0, 3, 4, 5)), "apply_adaptive_threshold": (threshold, (0, 1, 2))}
        torch.cuda.synchronize()
        for fn, _ in calls.values():
            fn(); fn()
        wall = {k: [] for k in calls}
        for name, (fn, _) in calls.items():                      # whole calls, profiler off
            for _r in range(a.runs):
                t0 = time.perf_counter(); fn(); wall[name].append(time.perf_counter() - t0)
        s.profile_enable(True)
        rows = {}
        for _r in range(a.runs):
            for name, (fn, stages) in calls.items():
                s.profile_reset()
                fn()
                for st in stages:
                    n, ms = s.profile_get("preprocess", st)
                    rows.setdefault((name, st), []).append((n, ms, s.profile_bytes("preprocess", st), s.profile_moved("preprocess", st)))
        s.profile_enable(False)
        lines.append(f"{T} x {N} x {N} float64, device-resident, {a.runs} runs after 2 warm-up calls; tile grid {tiles[0]} x {tiles[1]}, "
                     f"clipLimit 50000, window 151, threshold -5; mask share {float(mask.float().mean()):.3f}")
        lines.append("")
        lines.append("| call | kernel (stage) | launches | ms median | ms min .. max | algorithmic MB | TB/s (algorithmic) | minimal MB | TB/s (minimal) |")
        lines.append("|---|---|---|---|---|---|---|---|---|")
        for (name, st), recs in rows.items():
            ms = np.array([r[1] for r in recs])
            med = float(np.median(ms))
            lines.append(f"| {name} | {STAGES[st]} ({st}) | {recs[0][0]} | {med:.3f} | {ms.min():.3f} .. {ms.max():.3f} | {recs[0][2] / 1e6:.1f} | "
                         f"{recs[0][2] / med / 1e9:.2f} | {recs[0][3] / 1e6:.1f} | {recs[0][3] / med / 1e9:.2f} |")
        lines.append("")
        for name, w in wall.items():
            w = np.array(w) * 1e3
            lines.append(f"{name}, whole call (host clock, ends in a stream synchronise): median {np.median(w):.2f} ms, min {w.min():.2f}, max {w.max():.2f}")
    host_movie = movie.cpu().numpy()                                  # the host entries: staged uploads and downloads included
    for name, fn in (("apply_clahe", lambda: of.apply_clahe(host_movie, 50000, 10)),
                     ("apply_adaptive_threshold", lambda: of.apply_adaptive_threshold(host_movie, 151, -5))):
        fn()
        w = []
        for _r in range(3):
            t0 = time.perf_counter(); fn(); w.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"{name}, host arrays in and out (3 runs after a warm-up): median {np.median(w):.1f} ms, min {min(w):.1f}, max {max(w):.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
