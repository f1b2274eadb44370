"""correct_intensity_change: the fused call (vof_intensity_correct_dev: blur, then the two fused passes) against the same chain
made of the existing device blur (vof_blur_stack_dev) and torch subtractions, in one process on a device-resident stack, and
intensity_histograms next to them.

    python profiles/intensity_kernels.py [--frames 32] [--size 1024] [--runs 7] [--out FILE.md]

Arguments are the reference script's: smoothing_sigma 3, filter_size 5, target "blurred".  Every run is one whole call after two
warm-up calls, timed on the host clock around a call that ends in a stream synchronise; the table gives the median and the spread,
ms per frame, and GB/s of the algorithmic bytes: 10 planes of 8 bytes per frame for the fused call (4 + 3 + 3), 14 for the
composition (4 + 3 + 4 + 3).  The two fused passes together are also timed by the library's event profiler (class "preprocess":
stages 16 and 17, which the profiler's 16 slots per class sum in slot 15).  The two results are compared bit for bit before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


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
    movie = (120 + 60 * torch.sin(i[:, None] / 90) * torch.cos(i[None, :] / 70))[None] + \
        torch.arange(T, device="cuda", dtype=torch.float64)[:, None, None] + 12 * torch.randn((T, N, N), generator=g, device="cuda", dtype=torch.float64)
    movie = movie.clamp_(0, 255).floor_().contiguous()
    w1, w2 = of.gaussian_taps(3), of.gaussian_taps(5)
    edges = np.linspace(0, 255, 256)
    out, blurred, diff, drift, composed = (torch.empty_like(movie) for _ in range(5))
    lines = []
    with _native.Solver(N, N, 1) as s:
        def fused():
            s.intensity_correct(movie, T, w1, w2, 0, 0, out)

        def composition():
            s.blur(movie, blurred, T, w1)
            torch.sub(blurred, blurred[0], out=diff)
            torch.cuda.synchronize()
            s.blur(diff, drift, T, w2)
            torch.sub(blurred, drift, out=composed)
            torch.cuda.synchronize()

        def histograms():
            s.intensity_hist(movie, T, edges)
        calls = {"fused call": (fused, 10), "composition": (composition, 14), "intensity_histograms, 255 bins": (histograms, 1)}
        torch.cuda.synchronize()
        for fn, _ in calls.values():
            fn(); fn()
        same = bool(torch.equal(out.view(torch.int64), composed.view(torch.int64)))
        wall = {k: [] for k in calls}
        for _r in range(a.runs):
            for name, (fn, _) in calls.items():
                t0 = time.perf_counter(); fn(); wall[name].append(time.perf_counter() - t0)
        lines.append(f"{T} x {N} x {N} float64, device-resident, {a.runs} runs after 2 warm-up calls; smoothing_sigma 3 (radius 12), filter_size 5 "
                     f"(radius 20), target blurred; fused result equals the composition bit for bit: {same}")
        lines.append("")
        lines.append("| call | planes per frame | ms median | ms min .. max | ms per frame | GB/s (algorithmic) |")
        lines.append("|---|---|---|---|---|---|")
        frame_bytes = 8.0 * N * N
        for name, (fn, planes) in calls.items():
            w = np.array(wall[name]) * 1e3
            med = float(np.median(w))
            lines.append(f"| {name} | {planes} | {med:.3f} | {w.min():.3f} .. {w.max():.3f} | {med / T:.4f} | {planes * frame_bytes * T / med / 1e6:.0f} |")
        ratio = float(np.median(wall["composition"]) / np.median(wall["fused call"]))
        lines.append("")
        lines.append(f"composition / fused call: {ratio:.2f}")
        s.profile_enable(True)
        rows = {}
        for _r in range(a.runs):
            s.profile_reset()
            fused()
            n, ms = s.profile_get("preprocess", 15)               # stages 16 and 17: the profiler's last slot holds both
            rows.setdefault(15, []).append((n, ms, s.profile_bytes("preprocess", 15)))
            n, ms = s.profile_get("rhs")
            rows.setdefault("blur", []).append((n, ms, 32.0 * N * N * (T + 1)))
        s.profile_enable(False)
        lines.append("")
        lines.append("| kernels of the fused call (event profiler) | launch scopes | ms median | ms min .. max | algorithmic MB | GB/s |")
        lines.append("|---|---|---|---|---|---|")
        for st, recs in rows.items():
            ms = np.array([r[1] for r in recs])
            med = float(np.median(ms))
            label = {15: "the two fused passes: axis 0 with the difference, axis 1 with the subtraction", "blur": "first blur, two passes (rhs)"}[st]
            lines.append(f"| {label} | {recs[0][0]} | {med:.3f} | {ms.min():.3f} .. {ms.max():.3f} | {recs[0][2] / 1e6:.1f} | {recs[0][2] / med / 1e6:.0f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
