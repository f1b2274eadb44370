"""The cases of the tests that pin the direct preconditioner (tests/test_direct_restatement_cpu.py, tests/test_gpu_direct_pin.py): the
smallest image shapes at which each edge of csrc/vof_direct.hpp and of its driver in csrc/vof.hip exists - the last one-workgroup
inverse and the first blocked one, identity padding of the tiles or none, tall and wide images, the derivative quirk off, several
pairs per batch - in the regimes of DESIGN.md section 7:
    T: 8-bit data, speed_alpha 1e4, remodelling_alpha 1e2        W: 8-bit data, speed_alpha 2e3, remodelling_alpha 1
    N: unit data, speed_alpha 1, remodelling_alpha 1e4           and unit data with speed_alpha 0.1.
A set-up costs n_i rounds of launches, so the short side of a blocked case is the image height.

kind:
  "one step"         the restated preconditioner leaves a true one-step residual <= ADMISSION with BOTH inverses of
                     tests/direct_restatement.py, so the library must converge to rtol 1e-10 in exactly one Krylov step;
  "residual only"    a float64 elimination does not reach ADMISSION here, or only just (measured figures beside the case): only the
                     residual after one step is compared with the restatement's;
  "ill-conditioned"  the grad-div dominated corner (alpha / I^2 ~ 5e-6) on a stack (its own seed) where both inverses of the restatement
                     are left near the tolerance, at the level rounding allows (direct_restatement.attainable: 3.5e-12); the residual
                     after one step is held against that level, plus the full solve."""
import collections
import functools

import numpy as np

from oracle import vof_oracle as orc

import direct_restatement as dr

ADMISSION = 1e-12     # two decades under the tight rtol 1e-10: two float64 eliminations in different summation order differ by up to 17 x
TEXTURE_SEED = 5

Case = collections.namedtuple("Case", "n_i n_j T alpha beta scale quirks kind seed", defaults=(TEXTURE_SEED,))

T_, W_, N_ = (1e4, 1e2, 255.0), (2e3, 1.0, 255.0), (1.0, 1e4, 1.0)

CASES = [
    #                                         true one-step residual of the restatement, LAPACK / tile inverse
    Case(12, 66, 2, *T_, True, "one step"),            # m = 192: the last one-workgroup inverse              6e-14 / 9e-14
    Case(12, 67, 2, *T_, True, "one step"),            # m = 195: the first blocked size, ld 256 (61 padded)  4e-14 / 7e-14
    Case(67, 12, 2, *W_, True, "one step"),            # tall and narrow                                      2e-14 / 2e-14
    Case(67, 12, 2, *T_, True, "residual only"),       # the same in regime T sits on the bar                 1.0e-12 / 7.7e-13
    Case(131, 9, 2, *W_, True, "one step"),            # tall and narrow, m = 21                              1.7e-13 / 1.4e-13
    Case(9, 130, 2, *W_, True, "one step"),            # m = 384: exactly 6 tiles, no padding                 1.7e-13 / 5.0e-13
    Case(9, 131, 2, *T_, True, "one step"),            # m = 387: ld 448, one column past a tile multiple     6e-14 / 1.4e-13
    Case(9, 131, 2, *W_, True, "residual only"),       #                                                      4.7e-13 / 8.0e-12
    Case(14, 195, 2, *T_, False, "one step"),          # m = 579, ld 640; derivative quirk off                6e-14 / 1.7e-13
    Case(6, 259, 2, 0.1, 1e2, 1.0, True, "one step"),  # m = 771: 13 tiles, ld 832                            1.3e-13 / 1.5e-13
    Case(6, 259, 2, *T_, True, "residual only"),       # the 13-tile edge in regime T                         1.7e-13 / 1.5e-12
    Case(30, 99, 2, *T_, True, "one step"),            # m = 291, ld 320, 28 image rows                       6e-14 / 3.1e-13
    Case(5, 5, 2, 1.0, 1.0, 1.0, True, "one step"),    # 3 x 3 interior: a single-level grid                  2e-14 / 2e-14
    Case(20, 195, 2, 0.1, 1e2, 1.0, True, "residual only"),  # speed_alpha 0.1 at m = 579: under the bar, but by less than a third
                                                             # (with another BLAS 1.9e-13 / 8.2e-13)           1.6e-13 / 6.9e-13
    Case(70, 40, 2, *N_, False, "one step"),           # regime N, one-workgroup inverse at m = 114           5e-14 / 4e-14
    Case(40, 70, 2, 0.3, 0.1, 255.0, True, "ill-conditioned", 1),   # m = 204, ld 256; seed 1 (seed 5: 1.4e-13 / 1.5e-13)  5.3e-12 / 3.0e-11
    Case(12, 67, 4, *T_, True, "one step"),            # three pairs whose data differ, blocked               <= 5e-14 / 8e-14
]
BATCH_CASE = 16       # the three-pair blocked case: run with max_pairs_in_flight None, 1 and 2
assert CASES[BATCH_CASE].T == 4 and dr.path_rule(CASES[BATCH_CASE].n_j)["blocked"]

ONE_STEP = [i for i, c in enumerate(CASES) if c.kind == "one step"]


def case_id(i):
    c = CASES[i]
    return f"{i}-{c.n_i}x{c.n_j}x{c.T}-a{c.alpha:g}-b{c.beta:g}-s{c.scale:g}{'' if c.quirks else '-noquirk'}"


@functools.lru_cache(maxsize=None)
def movie(i):
    """The stack of case i: the texture of the oracle cut to (n_i, n_j), scaled, rounded to integers when 8-bit.  Read-only."""
    c = CASES[i]
    mv = orc.make_texture_stack(max(c.n_i, c.n_j, 16), c.T, seed=c.seed)[:, :c.n_i, :c.n_j] * c.scale
    if c.scale == 255.0:
        mv = np.round(mv)
    mv = np.ascontiguousarray(mv)
    mv.setflags(write=False)
    return mv


@functools.lru_cache(maxsize=None)
def restated(i, inverse):
    """Per pair of case i: (x, steps, true relative residual) of one Krylov step with the restated preconditioner, from the zero guess."""
    c, mv = CASES[i], movie(i)
    return tuple(dr.one_step(mv[k], mv[k + 1], c.alpha, c.beta, c.quirks, None, inverse) for k in range(c.T - 1))


@functools.lru_cache(maxsize=None)
def attainable(i):
    """Per pair of case i: eps ||A|| ||x|| / ||b||, the residual level that rounding alone leaves (direct_restatement.attainable)."""
    c, mv = CASES[i], movie(i)
    return tuple(dr.attainable(*dr.system(mv[k], mv[k + 1], c.alpha, c.beta, c.quirks)) for k in range(c.T - 1))
