"""Whole-call time of conduct_piv's native call (Solver.piv_flow on a device-resident stack) on the host clock; its kernels with the
library's event profiler (vof_profile_*, class "reduce", level = stage of csrc/vof_pivflow.hpp: 7 the offsets, 8 + p the
correlation of pass p) and, from the counted multiplications and additions, the achieved FP64 rate; and the numpy restatement
(tests/piv_flow_restatement.py) on a few pairs of the same case on this machine's host.

    python profiles/piv_flow_kernels.py [--pairs 32] [--size 1024] [--runs 5] [--host-pairs 2] [--out FILE.md]

The case: --pairs + 1 frames of --size x --size pixels, the translating texture of opticalflow_amd.synthetic scaled to [0, 255] and
rounded (integer-valued float64), moved by (2.3, -3.6) pixels per frame; the default passes (64, 16, 32) and (32, 4, 16).  Each step
runs as a child process under a time limit of its own (--step is the child's entry)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

PASSES = ((64, 32), (16, 4), (32, 16))          # window sizes, radii, steps
FP64_VECTOR_PEAK = 78.6e12                      # FLOP/s: the MI355X's vector FP64 rate, half its 157.3 TFLOPS FP32 vector rate, a fused multiply-add counted as 2


def case(a, frames=None):
    from opticalflow_amd import synthetic
    return np.rint(255.0 * synthetic.texture_stack_numpy(a.size, frames or a.pairs + 1, seed=11, shift=(2.3, -3.6)))


def work(a):
    """Per pass: windows, multiply-add pairs of the S_ab loop and of the row sums of the search region, per frame pair."""
    from opticalflow_amd import optical_flow as of
    rows = []
    for g in of.piv_grid((a.size, a.size), *PASSES):
        w, r, D, S = g["w"], g["r"], 2 * g["r"] + 1, g["w"] + 2 * g["r"]
        n = g["R"] * g["C"]
        rows.append(dict(windows=n, w=w, r=r, hot=n * D * D * w * w, sums=n * (S * D * w * 2 + w * w * 2 + D * D * w * 2), run=5 if r >= 10 else 3))
    return rows


def median_ms(call, runs, sync):
    call()
    sync()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter(); call(); sync(); t.append(time.perf_counter() - t0)
    return np.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3


def outputs(a, torch):
    from opticalflow_amd import optical_flow as of
    g = of.piv_grid((a.size, a.size), *PASSES)[-1]
    return [torch.empty((a.pairs, g["R"], g["C"]), dtype=torch.float64, device="cuda") for _ in range(3)]


def step_wall(a):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    movie = torch.as_tensor(case(a), device="cuda")
    outs = outputs(a, torch)
    print(f"{a.pairs} pairs of {a.size} x {a.size}, passes (w, r, s) = {list(zip(*PASSES))}; host clock")
    with _native.Solver(a.size, a.size, 1) as s:
        torch.cuda.synchronize()
        med, lo, hi = median_ms(lambda: s.piv_flow(movie, a.pairs, *PASSES, *outs), a.runs, torch.cuda.synchronize)
        counts = s.piv_flow(movie, a.pairs, *PASSES, *outs)
    print(f"Solver.piv_flow, movie and outputs on the device: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}) of {a.runs} runs after a warm-up: "
          f"{a.pairs / med * 1e3:.0f} pairs/s; counts (flat, border, threshold) per pass {counts.tolist()}")
    u, v = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    print(f"mean u {np.nanmean(u):.4f}, mean v {np.nanmean(v):.4f} (the texture moves by -3.6, 2.3)")
    med, lo, hi = median_ms(lambda: of.conduct_piv(movie), min(a.runs, 3), torch.cuda.synchronize)
    print(f"conduct_piv(movie on the device), the whole call with the results brought to the host: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f})")


def step_kernels(a):
    import torch
    from opticalflow_amd import _native
    movie = torch.as_tensor(case(a), device="cuda")
    outs = outputs(a, torch)
    with _native.Solver(a.size, a.size, 1) as s:
        torch.cuda.synchronize()
        s.piv_flow(movie, a.pairs, *PASSES, *outs)
        s.profile_enable(True)
        s.profile_reset()
        s.piv_flow(movie, a.pairs, *PASSES, *outs)
        stages = {st: s.profile_get("reduce", st) for st in (7, 8, 9)}
        s.profile_enable(False)
    print(f"one call with the event profiler on ({a.pairs} pairs of {a.size} x {a.size})")
    print("")
    print("| kernel (stage) | launches | ms | windows per pair | multiply-add pairs per pair | T multiply-add pairs/s | FP64 TFLOP/s | of the vector FP64 rate | LDS bytes read per multiply-add (hot loop) |")
    print("|---|---|---|---|---|---|---|---|---|")
    n, ms = stages[7]
    print(f"| k_pivflow_offsets (7) | {n} | {ms:.3f} | | | | | | |")
    for p, row in enumerate(work(a)):
        n, ms = stages[8 + p]
        pairs = (row["hot"] + row["sums"]) * a.pairs
        rate = pairs / max(ms, 1e-9) / 1e9
        print(f"| k_pivflow_correlate<{row['run']}>, pass {p}: w = {row['w']}, r = {row['r']} ({8 + p}) | {n} | {ms:.3f} | {row['windows']} | "
              f"{row['hot'] + row['sums']:.3e} ({row['hot'] / (row['hot'] + row['sums']):.0%} in the S_ab loop) | {rate:.2f} | {2 * rate:.1f} | "
              f"{2 * rate * 1e12 / FP64_VECTOR_PEAK:.0%} | {16 / row['run']:.1f} |")
    print("")
    print("counted: one multiplication and one addition per window pixel and displacement (S_ab), per pixel of a row sum of the search "
          "region and of the window (two sums each), and per row of S_b and S_bb; a multiply-add pair is 2 FLOP, issued as two "
          f"instructions (the products are rounded before they are added); vector FP64 rate {FP64_VECTOR_PEAK / 1e12:.1f} TFLOP/s counts a "
          "fused multiply-add as 2")


def step_host(a):
    import piv_flow_restatement as pf
    frames = case(a, a.host_pairs + 1)
    t0 = time.perf_counter()
    u, v, _, counts, _ = pf.piv(frames, *PASSES)
    dt = time.perf_counter() - t0
    print(f"tests/piv_flow_restatement.py (numpy, one process) on {a.host_pairs} pairs of the same case: {dt:.1f} s, {dt / a.host_pairs:.1f} s per pair; "
          f"mean u {np.nanmean(u):.4f}, mean v {np.nanmean(v):.4f}, counts {counts.tolist()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["wall", "kernels", "host"], default=None)
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.step:
        return {"wall": step_wall, "kernels": step_kernels, "host": step_host}[a.step](a)
    text = []
    for step in ("wall", "kernels", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                                                                            ("pairs", "size", "runs", "host_pairs")]
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
