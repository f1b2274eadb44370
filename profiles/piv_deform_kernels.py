"""conduct_piv's two options on the device: the whole native call (Solver.piv_flow on a device-resident stack) on the host clock and its
kernels with the library's event profiler (vof_profile_*, class "reduce", level = stage of csrc/vof_pivflow.hpp: 7 the offsets and the
median test, 8 + p the correlation of pass p), for the plain call, with deformation, with the median test, and with both.

    python profiles/piv_deform_kernels.py [--pairs 32] [--size 1024] [--runs 5] [--out FILE.md]

The case is that of profiles/piv_flow_kernels.py: --pairs + 1 frames of --size x --size pixels, the translating texture scaled to
[0, 255] and rounded, moved by (2.3, -3.6) pixels per frame; the default passes (64, 16, 32) and (32, 4, 16).  Each step runs as a
child process under a time limit of its own (--step is the child's entry)."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

from piv_flow_kernels import PASSES, case, median_ms, outputs          # noqa: E402  the same case, the same clock

VARIANTS = (("plain", dict()), ("deformation", dict(deformation=True)), ("median test", dict(outlier_threshold=2.0)),
            ("deformation and median test", dict(deformation=True, outlier_threshold=2.0)),
            ("deformation, median test on the returned vectors too", dict(deformation=True, outlier_threshold=2.0, validate_last=True)))


def step_wall(a):
    import torch
    from opticalflow_amd import _native
    movie = torch.as_tensor(case(a), device="cuda")
    outs = outputs(a, torch)
    print(f"{a.pairs} pairs of {a.size} x {a.size}, passes (w, r, s) = {list(zip(*PASSES))}; host clock, median of {a.runs} runs after a warm-up")
    print("")
    print("| Solver.piv_flow, movie and outputs on the device | ms (min .. max) | pairs/s | mean u | mean v | counts per pass | validation counts per pass |")
    print("|---|---|---|---|---|---|---|")
    with _native.Solver(a.size, a.size, 1) as s:
        torch.cuda.synchronize()
        for name, options in VARIANTS:
            med, lo, hi = median_ms(lambda: s.piv_flow(movie, a.pairs, *PASSES, *outs, **options), a.runs, torch.cuda.synchronize)
            got = s.piv_flow(movie, a.pairs, *PASSES, *outs, **options)
            counts, validation = got if isinstance(got, tuple) else (got, None)
            u, v = outs[0].cpu().numpy(), outs[1].cpu().numpy()
            print(f"| {name} | {med:.1f} ({lo:.1f} .. {hi:.1f}) | {a.pairs / med * 1e3:.0f} | {np.nanmean(u):.4f} | {np.nanmean(v):.4f} | {counts.tolist()} | "
                  f"{'' if validation is None else validation.tolist()} |")
    print("")
    print("the texture moves by (-3.6, 2.3)")


def step_kernels(a):
    import torch
    from opticalflow_amd import _native
    movie = torch.as_tensor(case(a), device="cuda")
    outs = outputs(a, torch)
    print(f"one call each with the event profiler on ({a.pairs} pairs of {a.size} x {a.size}); ms over the call, launches in brackets")
    print("")
    print("| | stage 7: offsets / median test | stage 8: pass 0, w = 64, r = 16 | stage 9: pass 1, w = 32, r = 4 |")
    print("|---|---|---|---|")
    with _native.Solver(a.size, a.size, 1) as s:
        torch.cuda.synchronize()
        for name, options in VARIANTS:
            s.piv_flow(movie, a.pairs, *PASSES, *outs, **options)
            s.profile_enable(True)
            s.profile_reset()
            s.piv_flow(movie, a.pairs, *PASSES, *outs, **options)
            stages = [s.profile_get("reduce", st) for st in (7, 8, 9)]
            s.profile_enable(False)
            print(f"| {name} | " + " | ".join(f"{ms:.3f} ({n})" for n, ms in stages) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["wall", "kernels"], default=None)
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.step:
        return {"wall": step_wall, "kernels": step_kernels}[a.step](a)
    text = []
    for step in ("wall", "kernels"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [f"--{k}={getattr(a, k)}" for k in ("pairs", "size", "runs")]
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
