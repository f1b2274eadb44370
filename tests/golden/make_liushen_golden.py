"""Generate the Liu-Shen fixtures g12a_liushen.npz ... g12e_liushen.npz from the REFERENCE itself
(``liu_shen_optical_flow_jit``, OF.py:426-673), imported with the stand-ins of make_golden.py (the numba decorators become
the identity, so the decorated loop runs as plain numpy, at about 4e4 pixel-iterations per second).  Numeric arrays only.

Every case holds the call's arguments (``movie, delta_x, delta_t, alpha, initial_v_x, initial_v_y, initial_remodelling,
max_iterations``) and its five results (``v_x, v_y, speed, remodelling, last_iteration``).  Case e is one pair and also holds
the step record ``v_x_steps, v_y_steps, speed_steps, remodelling_steps`` of ``iteration_stepsize``, composed here by calling
the reference function in chunks as conduct_variational_optical_flow_deprecated (OF.py:1420-1500) would if it unpacked all
five values: restart from the previous scaled result.

Every stored field must be finite, the restatement of tests/liushen_restatement.py must agree with it, and its two mutations
(mirrored 8-neighbour sums, n = 8 everywhere) must not; all of that is printed and asserted here as well as in the tests.

Usage:  python tests/golden/make_liushen_golden.py
"""
import contextlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

BOUND = 1e-13


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def check(name, args, ref):
    from liushen_restatement import liu_shen, error
    assert all(np.isfinite(f).all() for f in ref[:4]), name
    e = error(*liu_shen(*args)[:2], ref[0], ref[1])
    em = error(*liu_shen(*args, mirror_bar=True)[:2], ref[0], ref[1])
    en = error(*liu_shen(*args, n_eight=True)[:2], ref[0], ref[1])
    print(f"  {name}: max|v| {max(np.abs(ref[0]).max(), np.abs(ref[1]).max()):.3g}, restatement {e:.2e}, "
          f"mirrored sums {em:.2e}, n = 8 {en:.2e}")
    assert e <= BOUND and em >= 1e3 * BOUND and en >= 1e3 * BOUND, (name, e, em, en)


def case(OF, name, movie, dx, dt, alpha, ivx, ivy, irem, iterations, stepsize=None):
    t0 = time.time()
    args = (movie, dx, dt, alpha, 1.0, ivx, ivy, irem, iterations)
    ref = quiet(OF.liu_shen_optical_flow_jit, *args)
    check(name, args, ref)
    out = dict(movie=movie, delta_x=np.float64(dx), delta_t=np.float64(dt), alpha=np.float64(alpha),
               initial_v_x=np.asarray(ivx, dtype=np.float64), initial_v_y=np.asarray(ivy, dtype=np.float64),
               initial_remodelling=np.asarray(irem, dtype=np.float64), max_iterations=np.int64(iterations),
               v_x=ref[0], v_y=ref[1], speed=ref[2], remodelling=ref[3], last_iteration=np.int64(ref[4]))
    if stepsize is not None:
        assert movie.shape[0] == 2
        n_i, n_j = movie.shape[1:]
        plane = [np.full((n_i, n_j), float(g)) for g in (ivx, ivy, irem)]
        records = iterations // stepsize
        steps = [np.zeros((1, records + 1, n_i, n_j)) for _ in range(4)]
        steps[0][:, 0], steps[1][:, 0], steps[3][:, 0] = plane[0], plane[1], plane[2]
        steps[2][:, 0] = np.sqrt(plane[0] ** 2 + plane[1] ** 2)
        this = plane
        for r in range(1, records + 1):
            res = quiet(OF.liu_shen_optical_flow_jit, movie, dx, dt, alpha, 1.0, this[0], this[1], this[2],
                        max_iterations=stepsize, tolerance=1e-10, include_remodelling=True)
            for f in range(4):
                steps[f][:, r] = res[f]
            this = [res[0][0], res[1][0], res[3][0]]
        assert all(np.isfinite(s).all() for s in steps)
        out.update(iteration_stepsize=np.int64(stepsize), v_x_steps=steps[0], v_y_steps=steps[1], speed_steps=steps[2],
                   remodelling_steps=steps[3])
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path)} bytes, {time.time() - t0:.1f} s")


def main():
    from make_golden import import_reference
    from oracle import vof_oracle as orc
    OF = import_reference()
    tex = orc.make_texture_stack(64, 3, seed=0)
    # a: float texture, 40 x 56, two pairs, small alpha, scalar initial fields
    case(OF, "g12a_liushen.npz", np.ascontiguousarray(tex[:, :40, :56]), 0.25, 0.5, 0.05, 0.1, -0.05, 0.5, 25)
    # b: float texture, 56 x 40, one pair, the long run
    case(OF, "g12b_liushen.npz", np.ascontiguousarray(tex[:2, :56, :40]), 1.0, 2.0, 1.0, 0.0, 0.0, 0.0, 150)
    # c: uint8 input, alpha = 1e4
    tex8 = orc.make_texture_stack(56, 3, seed=11) * 255.0
    case(OF, "g12c_liushen.npz", np.round(tex8[:, :40, :56]).astype(np.uint8), 0.0913, 10.0, 1e4, 0.0, 0.0, 0.0, 30)
    # d: 8-bit-range float data, alpha = 1, (N_i, N_j) planes as initial fields
    rng = np.random.default_rng(12)
    ii, jj = np.meshgrid(np.arange(44.0), np.arange(36.0), indexing="ij")
    ivx = 0.3 * np.sin(ii / 7.0) + 0.05 * rng.standard_normal((44, 36))
    ivy = 0.2 * np.cos(jj / 5.0) + 0.05 * rng.standard_normal((44, 36))
    case(OF, "g12d_liushen.npz", np.ascontiguousarray(tex8[:2, 4:48, 10:46]), 0.5, 1.0, 1.0, ivx, ivy, rng.random((44, 36)), 20)
    # e: one pair with the step record of the wrapper (guesses 0.1, 0.1, 0.5 as its defaults)
    case(OF, "g12e_liushen.npz", np.ascontiguousarray(tex[1:, 8:32, 16:48]), 0.5, 0.25, 0.5, 0.1, 0.1, 0.5, 14, stepsize=4)


if __name__ == "__main__":
    main()
