"""The two-sweep pass of the revisited level (k_sweep_st2): between two visits of the W-cycle's revisited
stored level the post-smoothing sweep of one visit and the pre-smoothing sweep of the next run as one pass over the level.  The
pass performs the same point updates in the same colour order, and a block Gauss-Seidel sweep in a fixed colour order has one
result whatever the bands and strips, so with VOF_FUSE_REVISIT=0 (two k_sweep_st launches, as before) every result is the same
bits.  The switch is read when a context is created: each run has a context of its own."""
import numpy as np
import pytest

from oracle import vof_oracle as orc

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("iterations", "converged", "relative_residual", "L1_functional", "speed_functional", "remodelling_functional",
               "batch_pairs", "reserved")   # every field of vof_pair_stats but batch_ms


@pytest.fixture
def native():
    from opticalflow_amd import _native
    _native.load_library()
    return _native


def set_switch(monkeypatch, on):
    if on:
        monkeypatch.delenv("VOF_FUSE_REVISIT", raising=False)
    else:
        monkeypatch.setenv("VOF_FUSE_REVISIT", "0")


def one_cycle(native, monkeypatch, on, movie, params, rhs, level, level_shape):
    """(result of one cycle on rhs, launches of the `gs` class on `level` during it)"""
    set_switch(monkeypatch, on)
    with native.Solver(movie.shape[1], movie.shape[2], movie.shape[0] - 1) as s:
        s.debug_setup(movie, params)
        assert s.level_shape(level) == level_shape and level < s.num_levels - 1
        s.profile_enable(True)
        e = s.debug_vcycle(rhs)
        launches, _ = s.profile_get("gs", level)
        s.profile_enable(False)
    return e, launches


# frame shape -> the shape of level 2 and what it meets there (level 1 for w_cycle_level = 0)
CYCLE_CASES = [
    ((130, 258), 1, (32, 64)),      # one strip, one band
    ((131, 259), 1, (33, 65)),      # odd sizes, orphan row and column
    ((262, 522), 1, (65, 130)),     # two strips, three bands of pick_band_height
    ((134, 1034), 1, (33, 258)),    # three strips, the last one two columns wide
    ((130, 258), 0, (64, 128)),     # level 1 is the revisited level; its last visit writes float64 with vcycle_precision 3
]


@pytest.mark.parametrize("shape,w_level,revisited_shape", CYCLE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_cycle_is_the_same_bits_and_takes_the_pass(native, monkeypatch, shape, w_level, revisited_shape):
    """One cycle on a seeded random right-hand side, two pairs; 2 and 3 visits, both packed stencil formats, float64 and float32
    vectors below level 0.  Launches of the revisited level's sweeps per cycle: visits + 1 with the pass (the first
    pre-smoothing, one pass per revisit, the last post-smoothing), 2 * visits without."""
    movie = np.ascontiguousarray(orc.make_texture_stack(max(shape), 3, seed=11)[:, :shape[0], :shape[1]])
    rhs = np.random.default_rng(11).standard_normal((2, 3, shape[0] - 2, shape[1] - 2))
    level = w_level + 1
    for visits in (2, 3):
        for cp in (2, 3):
            for vp in (0, 3):
                p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, w_cycle_level=w_level, w_cycle_visits=visits,
                                          coarse_precision=cp, vcycle_precision=vp)
                e_on, n_on = one_cycle(native, monkeypatch, True, movie, p, rhs, level, revisited_shape)
                e_off, n_off = one_cycle(native, monkeypatch, False, movie, p, rhs, level, revisited_shape)
                key = (visits, cp, vp)
                print(key, "launches", n_on, n_off, "max |diff|", float(np.abs(e_on - e_off).max()))
                assert np.isfinite(e_on).all(), key
                assert (n_on, n_off) == (visits + 1, 2 * visits), key
                assert np.array_equal(e_on, e_off), key


def test_solve_with_finished_pairs_is_the_same_bits(native, monkeypatch):
    """130 x 258 x 7 with repeated frames (f0 f0 f1 f2 f2 f3 f4): the pairs of equal frames are finished before the first round, so
    the rounds run over the active list; fields and per-pair statistics with and without the pass."""
    tex = orc.make_texture_stack(258, 5, seed=5)
    movie = np.ascontiguousarray(tex[[0, 0, 1, 2, 2, 3, 4]][:, :130, :])
    p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=0)
    res = []
    for on in (True, False):
        set_switch(monkeypatch, on)
        with native.Solver(130, 258, 6) as s:
            res.append(s.solve_host(movie, p))
    on, off = res
    it = on[4]["iterations"]
    print("iterations", it.tolist(), "relres", on[4]["relative_residual"].tolist())
    assert it.min() < it.max(), it          # the active set was mixed
    for name, a, b in zip(("v_x", "v_y", "remodelling", "speed"), on[:4], off[:4]):
        assert np.array_equal(a, b), name
    for f in STAT_FIELDS:
        assert np.array_equal(on[4][f], off[4][f]), f
