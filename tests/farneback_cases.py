"""The inputs of the Farneback tests (GPU, CPU and the cv2 comparison): moving textures built from integers and sines."""
import functools

import numpy as np

# name -> (shape (T, N_i, N_j), depth, per-frame shift (rows, columns), the six OpenCV arguments); what each is there for:
# tests/test_gpu_farneback.py asserts it on the restatement's record
BASE = dict(pyr_scale=0.5, levels=1, winsize=9, iterations=2, poly_n=5, poly_sigma=1.1)
CASES = {
    "smallest": ((3, 40, 52), "u8", (0.6, -0.4), dict(BASE)),                                       # one level (40 * 0.5 < 32), three frames
    "two_levels": ((2, 75, 91), "f64", (1.3, -0.9), dict(BASE, levels=3, winsize=11, iterations=3)),   # 38 x 46: both roundings are ties
    "three_levels": ((2, 128, 160), "f64", (2.1, 1.4), dict(BASE, pyr_scale=0.7, levels=2, winsize=7)),
    "outside": ((2, 40, 52), "u8", (0.0, 9.0), dict(BASE, winsize=5, iterations=4)),                # a shift of 9 columns
    "wide_window": ((2, 40, 52), "f64", (0.6, -0.4), dict(BASE, winsize=51)),                       # m = 25 > 40 / 2
    "no_window": ((2, 40, 52), "f64", (0.6, -0.4), dict(BASE, winsize=1)),                          # m = 0
    "poly_7": ((2, 40, 52), "u8", (0.6, -0.4), dict(BASE, poly_n=7, poly_sigma=1.5)),
    "poly_sigma_0": ((2, 40, 52), "f64", (0.6, -0.4), dict(BASE, poly_sigma=0)),                    # sigma = 0.3 n
    "wide": ((2, 33, 333), "f64", (0.3, 1.2), dict(BASE)),                                          # two row workgroups, odd pitch
    "tiny": ((2, 16, 16), "u8", (0.4, 0.3), dict(BASE, winsize=5)),                                 # every pixel in the border band
    "no_iterations": ((2, 75, 91), "f64", (1.3, -0.9), dict(BASE, levels=3, iterations=0)),
    "one_iteration": ((2, 75, 91), "f64", (1.3, -0.9), dict(BASE, levels=3, iterations=1)),
    "blurred": ((4, 40, 52), "f64", (0.6, -0.4), dict(BASE)),                                       # run with smoothing_sigma = 1.3
    "translation": ((2, 64, 80), "f64", (0.6, -0.4), dict(pyr_scale=0.5, levels=0, winsize=15, iterations=3, poly_n=5, poly_sigma=1.1)),
}


def texture(T, N_i, N_j, shift, seed=0):
    """float64 frames in 20 .. 235: a sum of sines with periods of 8 pixels and more whose frame t is frame 0 moved by t * shift
    (rows, columns) - feature at (i, j) in frame 0 sits at (i + t * shift[0], j + t * shift[1]) in frame t."""
    t, i, j = np.meshgrid(np.arange(T), np.arange(N_i), np.arange(N_j), indexing="ij")
    u = i - shift[0] * t
    v = j - shift[1] * t
    k = 2 * np.pi
    f = (np.sin(k * (u / 17 + v / 29) + seed) + np.sin(k * (u / 11 - v / 13) + 1 + seed) + np.sin(k * u / 8 + 2) * np.sin(k * v / 9 + 3)
         + 0.5 * np.sin(k * (3 * u + 5 * v) / 97))
    return 127.5 + 30.0 * f


@functools.lru_cache(maxsize=None)
def case_input(name):
    (T, N_i, N_j), depth, shift, _ = CASES[name]
    m = texture(T, N_i, N_j, shift, seed=sorted(CASES).index(name))
    if depth == "u8":
        m = np.rint(m).astype(np.uint8)
    else:
        m = m + 1e-3 * np.sin(np.arange(m.size).reshape(m.shape) * 0.7)      # full mantissas
    m.setflags(write=False)
    return m


def case_arguments(name):
    return dict(CASES[name][3])
