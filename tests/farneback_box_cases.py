"""The inputs of the box-window Farneback tests: the moving textures of farneback_cases.py, seeded by the case's position here."""
import functools

import numpy as np

from farneback_cases import texture

# name -> (shape (T, N_i, N_j), depth, per-frame shift (rows, columns), the six OpenCV arguments); what each is there for:
# tests/test_gpu_farneback_box.py asserts it on the restatement's record
BASE = dict(pyr_scale=0.5, levels=1, winsize=9, iterations=2, poly_n=5, poly_sigma=1.1)
CASES = {
    "box_smallest": ((3, 40, 52), "u8", (0.6, -0.4), dict(BASE)),                                   # one image, three frames
    "box_script": ((2, 75, 91), "f64", (1.3, -0.9), dict(BASE, levels=1, winsize=20, iterations=3, poly_n=3)),   # compare_rho_and_actin.py:903: two images, even winsize
    "box_m1": ((2, 40, 52), "f64", (0.6, -0.4), dict(BASE, winsize=2)),                             # m = 1: no start rows, 3 x 3 over 4
    "box_w3": ((2, 40, 52), "u8", (0.6, -0.4), dict(BASE, winsize=3)),
    "box_over": ((2, 16, 16), "u8", (0.4, 0.3), dict(BASE, winsize=41)),                            # m = 20 > 16: both start loops run past the last row and column
    "box_wide_window": ((2, 40, 52), "f64", (0.6, -0.4), dict(BASE, winsize=51)),                   # m = 25 > 40 / 2
    "box_max": ((2, 40, 52), "f64", (0.6, -0.4), dict(BASE, winsize=129)),                          # m = 64 > both sides
    "box_wide": ((2, 33, 333), "f64", (0.3, 1.2), dict(BASE)),                                      # many column tiles, odd pitch
    "box_tall": ((2, 333, 33), "f64", (1.2, 0.3), dict(BASE)),                                      # a long vertical chain, several row bands
    "box_translation": ((2, 64, 80), "f64", (0.6, -0.4), dict(pyr_scale=0.5, levels=0, winsize=15, iterations=3, poly_n=5, poly_sigma=1.1)),
    "no_iterations": ((2, 75, 91), "f64", (1.3, -0.9), dict(BASE, levels=3, iterations=0)),
    "one_iteration": ((2, 75, 91), "f64", (1.3, -0.9), dict(BASE, levels=3, iterations=1)),
    "blurred": ((4, 40, 52), "f64", (0.6, -0.4), dict(BASE)),                                       # run with smoothing_sigma = 1.3
}


@functools.lru_cache(maxsize=None)
def case_input(name):
    (T, N_i, N_j), depth, shift, _ = CASES[name]
    m = texture(T, N_i, N_j, shift, seed=list(CASES).index(name))
    if depth == "u8":
        m = np.rint(m).astype(np.uint8)
    else:
        m = m + 1e-3 * np.sin(np.arange(m.size).reshape(m.shape) * 0.7)      # full mantissas
    m.setflags(write=False)
    return m


def case_arguments(name):
    return dict(CASES[name][3])
