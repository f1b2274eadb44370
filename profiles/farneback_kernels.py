"""Pairs per second and per-kernel times of conduct_opencv_flow with the library's event profiler (vof_profile_*, class
"preprocess", level = stage), next to the bytes each kernel class reports.

    python profiles/farneback_kernels.py [--frames 17] [--size 1024] [--runs 5] [--window gaussian|box] [--winsize 50] [--out FILE.md]

The stack is uint8-valued and device-resident, tensors in and out; the arguments are those of the reference's
analyse_short_timeinterval_data.py: levels=5, winsize=50, iterations=50, poly_n=5, poly_sigma=1.1 (pyr_scale=0.5).  Whole calls
are timed with the profiler off (median of --runs after a warm-up call); the per-kernel table comes from one more call with it on.
--window box measures OpenCV's default window instead (conduct_opencv_flow(..., window="box"); stages 14 and 15 in place of 11
and 12, and its own minimal byte count); --winsize changes the window's size.
Each step runs as a child process under a time limit of its own (--step is the child's entry)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

STAGES = {7: "level images (blur, blur, resize)", 8: "polynomial expansion", 9: "flow carried to a level", 10: "matrices",
          11: "window rows (vertical pass)", 12: "window columns + solve + update", 13: "results"}
ARGS = dict(pyr_scale=0.5, levels=5, winsize=50, iterations=50, poly_n=5, poly_sigma=1.1)
LOOP_BYTES = 20 + 20 + 20 + 20 + 8          # per pixel and iteration: M read, R0, R1 gathered once, M written, flow
# the box window: M read once (the row that leaves the window comes from the caches), V in double written and read once
# (likewise the column), R0, R1, flow, M written
BOX_STAGES = {14: "window rows (vertical running sum)", 15: "window columns (horizontal running sum) + solve + update"}
BOX_LOOP_BYTES = 20 + 40 + 40 + 20 + 20 + 8 + 20


def setup(a):
    """(arguments, stage names, the two loop stages, minimal loop bytes) of the window that is measured."""
    args = dict(ARGS, winsize=a.winsize)
    if a.window == "gaussian":
        return args, STAGES, (11, 12), LOOP_BYTES
    stages = {st: name for st, name in STAGES.items() if st not in (11, 12)}
    stages.update(BOX_STAGES)
    return args, stages, (14, 15), BOX_LOOP_BYTES


def movie(T, N):
    import torch
    i = torch.arange(N, device="cuda", dtype=torch.float64)
    t = torch.arange(T, device="cuda", dtype=torch.float64)[:, None, None]
    u, v = i[None, :, None] - 0.7 * t, i[None, None, :] + 0.4 * t
    f = torch.sin(u / 5.0 + v / 9.0) + torch.sin(u / 3.0 - v / 4.0) + torch.sin(u / 23.0) * torch.sin(v / 17.0)
    return (127.5 + 40.0 * f).round_().to(torch.uint8).contiguous()


def step_wall(a):
    import torch
    from opticalflow_amd import optical_flow as of
    m = movie(a.frames, a.size)
    ARGS = setup(a)[0]
    call = lambda: of.conduct_opencv_flow(m, output="torch", window=a.window, **ARGS)
    r = call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(r["speed"]).all())
    w = []
    for _ in range(a.runs):
        t0 = time.perf_counter(); call(); torch.cuda.synchronize(); w.append(time.perf_counter() - t0)
    w = np.array(w)
    pairs = a.frames - 1
    print(f"{a.frames} x {a.size} x {a.size} uint8, device tensors in and out, {'box window, ' if a.window == 'box' else ''}{ARGS}")
    print(f"whole call (host clock, ends in a device synchronise), {a.runs} runs after a warm-up: median {np.median(w) * 1e3:.1f} ms, "
          f"min {w.min() * 1e3:.1f}, max {w.max() * 1e3:.1f}; {pairs / np.median(w):.2f} pairs/s, {np.median(w) / pairs * 1e3:.2f} ms per pair")
    print(f"median |v| of the last run: v_x {float(r['v_x'].median()):.3f} (texture moves +0.4 columns), v_y {float(r['v_y'].median()):.3f} (-0.7 rows)")
    print("OpenCV itself: not measured (not installed)")


def step_kernels(a):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    T, N = a.frames, a.size
    ARGS, STAGES, loop, LOOP_BYTES = setup(a)
    m = movie(T, N).to(torch.float64)
    plan = of.farneback_plan(N, N, ARGS["pyr_scale"], ARGS["levels"], ARGS["winsize"], ARGS["poly_n"], ARGS["poly_sigma"])
    out = [torch.empty((T - 1, N, N), dtype=torch.float64, device="cuda") for _ in range(3)]
    with _native.Solver(N, N, 1) as s:
        call = lambda: s.farneback_dev(m[:-1], m[1:], T - 1, plan, ARGS["iterations"], 1.0, *out, box=a.window == "box")
        torch.cuda.synchronize()
        call()
        s.profile_enable(True)
        s.profile_reset()
        call()
        rows = {st: (s.profile_get("preprocess", st), s.profile_bytes("preprocess", st)) for st in STAGES}
        s.profile_enable(False)
    total = sum(ms for (_, ms), _ in rows.values())
    print(f"one call with the event profiler on ({T - 1} pairs; sizes {plan['sizes']}): {total:.1f} ms in kernels")
    print("")
    print("| kernel class (stage) | launches | ms | share | counted GB | TB/s (counted) |")
    print("|---|---|---|---|---|---|")
    for st, ((n, ms), b) in sorted(rows.items()):
        print(f"| {STAGES[st]} ({st}) | {n} | {ms:.2f} | {100 * ms / total:.1f} % | {b / 1e9:.2f} | {b / max(ms, 1e-9) / 1e9:.2f} |")
    pixels = sum(h * w for h, w in plan["sizes"]) * (T - 1)
    loop_ms = rows[loop[0]][0][1] + rows[loop[1]][0][1]
    need = LOOP_BYTES * pixels * ARGS["iterations"]
    print("")
    print(f"loop (stages {loop[0]} + {loop[1]}): {loop_ms:.1f} ms for {pixels * ARGS['iterations'] / 1e9:.2f} G pixel-iterations; on the minimal "
          f"{LOOP_BYTES} bytes per pixel and iteration ({need / 1e9:.1f} GB) that is {need / loop_ms / 1e9:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window", choices=["gaussian", "box"], default="gaussian")
    ap.add_argument("--winsize", type=int, default=ARGS["winsize"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["wall", "kernels"], default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.step:
        return {"wall": step_wall, "kernels": step_kernels}[a.step](a)
    text = []
    for step in ("wall", "kernels"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--frames", str(a.frames), "--size", str(a.size), "--runs", str(a.runs),
               "--window", a.window, "--winsize", str(a.winsize)]
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
