"""The inputs of the resize tests (GPU, CPU and the cv2 comparison), from fixed seeds."""
import functools

import numpy as np

# name -> (input shape (T, N_i, N_j), (n_i, n_j)); what each is there for: tests/test_gpu_resize.py asserts it on the record
CASES = {
    "dropped_entries": ((3, 26, 21), (10, 9)),       # general; a head entry (rows, d = 5) and a tail entry (columns) below 1e-3
    "mixed_counts": ((3, 41, 53), (8, 10)),          # general; scales 5.125 and 5.3: 6 and 7 entries along one axis
    "one_integer_axis": ((3, 40, 50), (13, 25)),     # general; the integer axis carries weights float32(1 / 2)
    "rows_only": ((3, 40, 50), (3, 50)),             # general; columns 1 : 1
    "clipped_cell": ((3, 10, 50), (3, 6)),           # general; 10 -> 3: the last cell's cw is ssize - f1
    "fast_area2": ((3, 40, 50), (40, 25)),           # fast 1 x 2
    "fast_2x2": ((3, 40, 50), (20, 25)),             # fast 2 x 2: the half-up rounding of uint8
    "fast_3x5": ((3, 39, 50), (13, 10)),             # fast, area 15: three groups of four and a rest of three
    "identity": ((3, 37, 53), (37, 53)),
    "wide": ((2, 300, 333), (70, 130)),              # several column blocks per row, odd segment starts
    "long_rows": ((2, 6, 4500), (4, 3)),             # general; one output pixel reads 1500 columns: the segment comes in pieces
    "long_rows_fast": ((2, 6, 4400), (3, 2)),        # fast 2 x 2200: the same for the block sums
}


def _seed(name):
    return 1000 + sorted(CASES).index(name)


@functools.lru_cache(maxsize=None)
def u8_input(name):
    """uint8 noise; on a checkerboard of the 2 x 2 blocks the block is [[a, a], [a + 1, a + 1]] with a even, so that block
    sums 4 q + 2 with even q (the ties that half-up and half-to-even round apart) are certain to occur."""
    shape = CASES[name][0]
    rng = np.random.default_rng(_seed(name))
    m = rng.integers(0, 256, size=shape, dtype=np.uint8)
    T, N_i, N_j = shape
    a = (rng.integers(0, 127, size=(T, N_i // 2, N_j // 2)) * 2).astype(np.uint8)
    bi, bj = np.meshgrid(np.arange(N_i // 2), np.arange(N_j // 2), indexing="ij")
    pick = (bi + bj) % 3 == 0
    for oi, oj, add in ((0, 0, 0), (0, 1, 0), (1, 0, 1), (1, 1, 1)):
        view = m[:, oi:2 * (N_i // 2):2, oj:2 * (N_j // 2):2]
        view[:, pick] = a[:, pick] + add
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def f64_input(name):
    """A smooth float64 field with negative values and full mantissas."""
    T, N_i, N_j = CASES[name][0]
    rng = np.random.default_rng(_seed(name) + 500)
    t, i, j = np.meshgrid(np.arange(T), np.arange(N_i), np.arange(N_j), indexing="ij")
    m = 700.0 * np.sin(0.37 * i + 0.11 * t) * np.cos(0.23 * j - 0.05 * t) + 90.0 * np.sin(0.071 * (i + 2 * j)) - 40.0
    m = m + 1e-3 * rng.standard_normal(m.shape)
    m.setflags(write=False)
    return m


def case_input(name, depth):
    return u8_input(name) if depth == "u8" else f64_input(name)
