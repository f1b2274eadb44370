"""Whole-call time of upsample_PIV_vectors (the dense part of convert_PIV_result) on the host clock, split into the host
preparation (scipy's Delaunay and gradient estimate per frame, optical_flow.piv_tables) and the device part
(Solver.piv_upsample into device tensors); the three kernels with the library's event profiler (vof_profile_*, class "reduce",
level = stage of csrc/vof_piv.hpp); and the same call made of scipy.interpolate.griddata on this machine's host - what the
reference does.

    python profiles/piv_convert_kernels.py [--frames 32] [--size 1024] [--grid 63] [--missing 0.05] [--runs 5] [--out FILE.md]

The case: --frames frames of --size x --size pixels, a --grid x --grid PIV grid centred on the image, a fraction --missing of
the vectors NaN, drawn per frame (so every frame is triangulated: nothing is reused).  Each step runs as a child process under a
time limit of its own (--step is the child's entry)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

STAGES = {4: "k_piv_coeffs (control values)", 5: "k_piv_locate (the map)", 6: "k_piv_eval (evaluation)"}


def case(a):
    from piv_restatement import smooth_vectors
    rng = np.random.default_rng(48)
    step = a.size // (a.grid + 1)
    at = (a.size - step * (a.grid - 1)) // 2 + step * np.arange(a.grid, dtype=np.float64)
    gy, gx = np.meshgrid(at, at, indexing="ij")
    x, y = np.repeat(gx[None], a.frames, 0), np.repeat(gy[None], a.frames, 0)
    vx, vy = np.empty_like(x), np.empty_like(x)
    for k in range(a.frames):
        vx[k], vy[k] = smooth_vectors(gx / 8.0, gy / 8.0, k, rng)
        vx[k][rng.random(gx.shape) < a.missing] = np.nan
    return x, y, vx, vy


def median_ms(call, runs, sync):
    call()
    sync()
    w = []
    for _ in range(runs):
        t0 = time.perf_counter(); call(); sync(); w.append(time.perf_counter() - t0)
    return np.median(w) * 1e3, min(w) * 1e3, max(w) * 1e3


def step_wall(a):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    x, y, vx, vy = case(a)
    F, N = a.frames, a.size
    print(f"{F} frames of {N} x {N}, a {a.grid} x {a.grid} PIV grid, {int(np.isnan(vx).sum())} of {vx.size} vectors missing; host clock")
    med, lo, hi = median_ms(lambda: of.piv_tables(x, y, vx, vy), min(a.runs, 3), lambda: None)
    tables = of.piv_tables(x, y, vx, vy)
    print(f"host preparation (Delaunay + gradients per frame, {int(tables['triangle_offsets'][-1])} triangles in all): median {med:.1f} ms "
          f"(min {lo:.1f}, max {hi:.1f}), {med / F:.2f} ms per frame")
    outs = [torch.empty((F, N, N), dtype=torch.float64, device="cuda") for _ in range(3)]
    with _native.Solver(N, N, 1) as s:
        med, lo, hi = median_ms(lambda: s.piv_upsample(tables, F, *outs), a.runs, torch.cuda.synchronize)
        counts = s.piv_upsample(tables, F, *outs)
    print(f"device part (tables up, three kernels, counts back; outputs stay on the device): median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}) "
          f"of {a.runs} runs after a warm-up; {int(counts[0])} pixels outside every triangle, {int(counts[1])} frames on the host")
    med, lo, hi = median_ms(lambda: of.upsample_PIV_vectors(x, y, vx, vy, (N, N), output="torch"), min(a.runs, 3), torch.cuda.synchronize)
    print(f"upsample_PIV_vectors(output='torch'), the whole call: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f})")


def step_kernels(a):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    x, y, vx, vy = case(a)
    F, N = a.frames, a.size
    tables = of.piv_tables(x, y, vx, vy)
    outs = [torch.empty((F, N, N), dtype=torch.float64, device="cuda") for _ in range(3)]
    with _native.Solver(N, N, 1) as s:
        torch.cuda.synchronize()
        s.piv_upsample(tables, F, *outs)
        s.profile_enable(True)
        s.profile_reset()
        s.piv_upsample(tables, F, *outs)
        rows = {st: (s.profile_get("reduce", st), s.profile_bytes("reduce", st)) for st in STAGES}
        s.profile_enable(False)
    print(f"one call with the event profiler on ({F} frames of {N} x {N}, {int(tables['triangle_offsets'][-1])} triangles)")
    print("")
    print("| kernel (stage) | launches | ms | counted GB | TB/s (counted) |")
    print("|---|---|---|---|---|")
    for st, ((n, ms), b) in sorted(rows.items()):
        rate = f"{b / max(ms, 1e-9) / 1e9:.2f}" if b else ""
        print(f"| {STAGES[st]} ({st}) | {n} | {ms:.3f} | {b / 1e9:.3f} | {rate} |")
    print("")
    print("counted: 352 + 160 bytes per triangle (coefficients written, tables read) and 4 + 24 bytes per pixel (map read, three "
          "fields written); the map kernel is not counted in bytes")


def step_griddata(a):
    import scipy.interpolate
    x, y, vx, vy = case(a)
    n = min(a.frames, a.griddata_frames)
    qy, qx = np.meshgrid(np.arange(a.size), np.arange(a.size), indexing="ij")
    t0 = time.perf_counter()
    for k in range(n):
        ok = ~np.isnan(vx[k]) & ~np.isnan(vy[k])
        for v in (vx, vy):
            scipy.interpolate.griddata((x[k][ok], y[k][ok]), v[k][ok], (qx, qy), method="cubic")
    dt = time.perf_counter() - t0
    print(f"scipy.interpolate.griddata(method='cubic') twice per frame on the host, {n} frames of {a.size} x {a.size}, one run: {dt:.2f} s, "
          f"{dt / n * 1e3:.0f} ms per frame; a device consumer would then wait for {3 * 8 * n * a.size * a.size / 1e9:.2f} GB through PCIe")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=63)
    ap.add_argument("--missing", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--griddata-frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["wall", "kernels", "griddata"], default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.step:
        return {"wall": step_wall, "kernels": step_kernels, "griddata": step_griddata}[a.step](a)
    text = []
    for step in ("wall", "kernels", "griddata"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                                                                            ("frames", "size", "grid", "missing", "runs", "griddata_frames")]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.step_timeout)
        print(done.stdout, end="", flush=True)
        text.append(done.stdout)
        if done.returncode != 0:                       # nothing more is started on the device after a failed step
            sys.exit(f"step {step} ended with status {done.returncode}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(text))


if __name__ == "__main__":
    main()
