"""Whole-call and per-pass times of compare_flow_results and filter_PIV_flow_result with the library's event profiler
(vof_profile_*, class "reduce", level = stage of csrc/vof_flowcompare.hpp), next to the bytes each pass reads and writes, and
the time the numpy restatement of tests/flow_compare_restatement.py takes for the same stack on the host - what a user does today.

    python profiles/flow_compare_kernels.py [--pairs 64] [--size 1024] [--runs 5] [--out FILE.md]

The two results are device-resident float64 tensors: a is normal noise, b = 0.6 a + 0.8 noise, speed = |v|; the movie of the
filter is uint8 noise.  Whole calls are timed with the profiler off (median of --runs after a warm-up call); the per-pass table
comes from one more call of each entry point with it on.  Each step runs as a child process under a time limit of its own
(--step is the child's entry)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

STAGES = {1: ("filter mask", 56), 2: ("extremes pass", 48), 3: ("histogram pass", 48)}       # stage: (name, bytes per sample)
STREAM = "profiles/r03_stream_rate.md: 6.1-7.0 TB/s reading, 4.5-5.0 TB/s with 5 reads + 2 writes"


def results(P, N):
    import torch
    g = torch.Generator(device="cuda").manual_seed(46)
    out = []
    va = torch.randn((2, P, N, N), generator=g, device="cuda", dtype=torch.float64)
    vb = 0.6 * va + 0.8 * torch.randn((2, P, N, N), generator=g, device="cuda", dtype=torch.float64)
    for v in (va, vb):
        out.append(dict(v_x=v[0].contiguous(), v_y=v[1].contiguous(), speed=torch.sqrt(v[0] ** 2 + v[1] ** 2)))
    return out


def median_ms(call, runs):
    import torch
    call()
    torch.cuda.synchronize()
    w = []
    for _ in range(runs):
        t0 = time.perf_counter(); call(); torch.cuda.synchronize(); w.append(time.perf_counter() - t0)
    return np.median(w) * 1e3, min(w) * 1e3, max(w) * 1e3


def step_wall(a):
    import torch
    from opticalflow_amd import optical_flow as of
    ra, rb = results(a.pairs, a.size)
    samples = a.pairs * a.size * a.size
    print(f"two results of {a.pairs} x {a.size} x {a.size} float64 (v_x, v_y, speed), device tensors; summaries to the host")
    for name, kw, passes in (("automatic ranges (two passes)", {}, 2),
                             ("every range explicit (one pass)", dict(joint_speed_ranges=((0, 4), (0, 4)), angle_range=(0, np.pi)), 1)):
        med, lo, hi = median_ms(lambda: of.compare_flow_results(ra, rb, **kw), a.runs)
        print(f"compare_flow_results, {name}: median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}) of {a.runs} runs after a warm-up; "
              f"{passes * 48 * samples / med / 1e9:.2f} TB/s on {passes} x 48 bytes per sample, host clock, call ends synchronised")
    r = of.compare_flow_results(ra, rb)
    print(f"joint_count {r['joint_count']}, angle_count {r['angle_count']}, angle_dropped {r['angle_dropped']} of {samples} samples")
    movie = torch.randint(0, 256, (a.pairs + 1, a.size, a.size), device="cuda", dtype=torch.uint8)
    ra["original_data"] = movie
    med, lo, hi = median_ms(lambda: of.filter_PIV_flow_result(ra, 100.0), a.runs)
    print(f"filter_PIV_flow_result (uint8 movie, converted to float64 per call): median {med:.2f} ms (min {lo:.2f}, max {hi:.2f})")


def step_kernels(a):
    import torch
    from opticalflow_amd import _native
    from opticalflow_amd.optical_flow import gaussian_taps
    P, N = a.pairs, a.size
    ra, rb = results(P, N)
    stacks = [r[k] for r in (ra, rb) for k in ("v_x", "v_y", "speed")]
    movie = torch.randint(0, 256, (P, N, N), device="cuda", dtype=torch.uint8).to(torch.float64)
    edges = np.linspace(0.0, 4.0, 51)
    with _native.Solver(N, N, 1) as s:
        def call():
            s.flow_extremes(stacks, P, 0.1, 0.5)
            s.flow_compare(stacks, P, 0.1, 0.5, True, edges, edges, np.linspace(0, np.pi, 21), True)
            s.flow_filter(movie, gaussian_taps(3), P, 100.0, 7.0, False, stacks[0], stacks[1], stacks[2])
        torch.cuda.synchronize()
        call()
        s.profile_enable(True)
        s.profile_reset()
        call()
        rows = {st: (s.profile_get("reduce", st), s.profile_bytes("reduce", st)) for st in STAGES}
        blur = s.profile_get("rhs", 0)
        s.profile_enable(False)
    print(f"one call of each entry point with the event profiler on ({P} pairs of {N} x {N}); 50 x 50 and 20 bins")
    print("")
    print("| pass (stage) | launches | ms | bytes per sample | counted GB | TB/s (counted) |")
    print("|---|---|---|---|---|---|")
    for st, ((n, ms), b) in sorted(rows.items()):
        print(f"| {STAGES[st][0]} ({st}) | {n} | {ms:.3f} | {STAGES[st][1]} | {b / 1e9:.2f} | {b / max(ms, 1e-9) / 1e9:.2f} |")
    print(f"| the filter's blur, sigma 3 (class rhs) | {blur[0]} | {blur[1]:.3f} | | | |")
    print("")
    print("streaming rate of this chip, " + STREAM)


def step_numpy(a):
    from flow_compare_restatement import compare_restatement, make_result
    P, N = a.pairs, a.size
    va = np.random.default_rng(46).normal(0, 1, (2, P, N, N))
    vb = 0.6 * va + 0.8 * np.random.default_rng(47).normal(0, 1, (2, P, N, N))
    ra, rb = make_result(va[0], va[1]), make_result(vb[0], vb[1])
    del va, vb
    t0 = time.perf_counter()
    r = compare_restatement(ra, rb)
    dt = time.perf_counter() - t0
    print(f"numpy restatement on the host, the same shape ({P} x {N} x {N}), one run: {dt:.2f} s (joint_count {r['joint_count']}); a "
          f"device-resident pair of results would first cross PCIe: {6 * 8 * P * N * N / 1e9:.2f} GB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["wall", "kernels", "numpy"], default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.step:
        return {"wall": step_wall, "kernels": step_kernels, "numpy": step_numpy}[a.step](a)
    text = []
    for step in ("wall", "kernels", "numpy"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--pairs", str(a.pairs), "--size", str(a.size), "--runs", str(a.runs)]
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
