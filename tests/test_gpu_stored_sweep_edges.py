"""The fused sweeps of the stored levels (k_sweep for the float32 / float64 stencils, k_sweep_st for the packed
ones) at the edges of their strip geometry, in every stencil format, with float64 and float32 vectors, in both colour orders,
from a given x and from zero.  Two properties per level that has a smoother:
 (a) the sweep is the four per-colour kernels (debug_gs) in the same colour order, to rounding (float64 vectors: the reference
     smoother works on those only);
 (b) a sweep told that x is zero (from_zero: no x rows are read, and in the forward order a packed format requests only the
     stencil blocks that can meet a non-zero neighbour) gives the bits of the same sweep on an x of zeros."""
import functools

import numpy as np
import pytest

from oracle import vof_oracle as orc

pytestmark = pytest.mark.gpu

PAIRS = 2

# frame shape -> the interior of level 1, where the strips of 128 owned columns meet what the case is about
FRAMES = [
    ((70, 258), (34, 128)),      # one strip, exactly full
    ((70, 262), (34, 130)),      # a full strip and a strip of two columns
    ((71, 259), (35, 129)),      # odd sizes, a strip of one orphan column
    ((262, 522), (130, 260)),    # three strips, several bands
]
FORMATS = [(cp, vp) for cp in (0, 1, 2, 3) for vp in (0, 1)]     # coarse_precision x vcycle_precision


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def native():
    from opticalflow_amd import _native
    _native.load_library()
    return _native


@functools.lru_cache(maxsize=None)
def movie_of(shape):
    return np.ascontiguousarray(orc.make_texture_stack(max(shape), PAIRS + 1, seed=11)[:, :shape[0], :shape[1]])


@pytest.mark.parametrize("coarse_precision,vcycle_precision", FORMATS)
@pytest.mark.parametrize("shape,level1", FRAMES, ids=lambda v: "x".join(map(str, v)))
def test_sweep_at_the_strip_edges(native, shape, level1, coarse_precision, vcycle_precision):
    p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, coarse_precision=coarse_precision,
                              vcycle_precision=vcycle_precision)
    rng = np.random.default_rng(11)
    with native.Solver(shape[0], shape[1], PAIRS) as s:
        s.debug_setup(movie_of(shape), p)
        assert s.level_shape(0) == (shape[0] - 2, shape[1] - 2) and s.level_shape(1) == level1
        assert s.num_levels >= 3                                   # level 1 has a smoother
        for lvl in range(1, s.num_levels - 1):
            x = rng.standard_normal((PAIRS, 3) + s.level_shape(lvl))
            b = rng.standard_normal(x.shape)
            zeros = np.zeros_like(x)
            for reverse in (False, True):
                key = (lvl, s.level_shape(lvl), reverse)
                got = s.debug_sweep(lvl, x, b, reverse=reverse)
                got_z = s.debug_sweep(lvl, zeros, b, reverse=reverse)
                got_fz = s.debug_sweep(lvl, zeros, b, reverse=reverse, from_zero=True)
                assert np.isfinite(got).all() and np.isfinite(got_fz).all(), key
                if vcycle_precision == 0:
                    want, want_z = x, zeros
                    for colour in ((3, 2, 1, 0) if reverse else (0, 1, 2, 3)):
                        want = s.debug_gs(lvl, want, b, colour)
                        want_z = s.debug_gs(lvl, want_z, b, colour)
                    ea, ez, efz = relerr(got, want), relerr(got_z, want_z), relerr(got_fz, want_z)
                    print(key, "relerr", ea, ez, efz)
                    assert ea < 1e-13 and ez < 1e-13 and efz < 1e-13, key
                differ = int(np.count_nonzero(got_fz != got_z))
                print(key, "from zero:", differ, "of", got_z.size, "differ")
                assert np.array_equal(got_fz, got_z), key
