"""Lanes: the device solve of one stack as concurrent pair groups on streams of their own (VOF_LANES).

Every test solves the same stack with one lane and with several, through the device-resident drop-in call
(output="torch", the path of vof_solve_stack_dev), and asks for the same per-pair arithmetic: the same iteration counts and
converged flags, and fields that agree to 1e-9 of each field's max-abs.  Launch grids that depend on the pairs in a launch
(band heights, hence the number of per-block partial sums) change the order in which dot products are added, so bit-identity
is not required; the tests solve to rtol 1e-10, where the answer is pinned well below that bar (at 1e-6, BiCGStab's short
recurrences carry rounding-order differences of the dot products into the iterate at the 1e-8 level).  VOF_LANES_MIN_MPIX=0 lets lanes run on
stacks far below the default threshold.
"""
import os

import numpy as np
import pytest

from oracle import vof_oracle as orc

pytestmark = pytest.mark.gpu

FIELDS = ("v_x", "v_y", "remodelling", "speed")


@pytest.fixture(scope="module")
def of():
    from opticalflow_amd import optical_flow
    return optical_flow


def solve(of, movie, lanes, **kw):
    old = {k: os.environ.get(k) for k in ("VOF_LANES", "VOF_LANES_MIN_MPIX")}
    os.environ["VOF_LANES"] = str(lanes)
    os.environ["VOF_LANES_MIN_MPIX"] = "0"
    try:
        res = of.variational_optical_flow(movie, output="torch", return_stats=True, **kw)
        return {k: res[k].cpu().numpy() for k in FIELDS}, res["stats"]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def assert_same(one, many, good=None):
    (f1, s1), (f2, s2) = one, many
    np.testing.assert_array_equal(s1["iterations"], s2["iterations"])
    np.testing.assert_array_equal(s1["converged"], s2["converged"])
    good = np.ones(len(s1), bool) if good is None else good
    for k in FIELDS:
        a, b = f1[k][good], f2[k][good]
        scale = max(float(np.abs(a).max()), 1e-300)
        assert float(np.abs(a - b).max()) <= 1e-9 * scale, k


def texture(n, frames, seed=3):
    import torch
    from opticalflow_amd import synthetic
    return synthetic.texture_stack_torch(n, frames, seed, torch.device("cuda", 0))


# 1024^2 with 16 or more phase-1 pairs: the two-phase warm start is on (>= 16 Mpixel per phase), so the lanes split both phases
@pytest.mark.parametrize("frames,stride,lanes", [
    (49, 3, 2),    # P = 48, a multiple of 3
    (51, 3, 2),    # P = 50: the lanes' cut falls between a warm pair and its phase-1 source
    (50, 3, 3),    # P = 49, odd, three lanes
    (18, 0, 2),    # every pair from the constant initial fields (plain batches)
    (18, 3, 2),    # P = 17, odd: below the two-phase threshold, plain batches
])
def test_lanes_match_one_lane(of, frames, stride, lanes):
    movie = texture(1024, frames)
    kw = dict(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=stride, rtol=1e-10)
    one = solve(of, movie, 1, **kw)
    many = solve(of, movie, lanes, **kw)
    assert one[1]["converged"].all()
    assert many[1]["relative_residual"].max() < 1e-10
    assert_same(one, many)


def test_lanes_small_batches(of):
    """More pairs than a lane's slots: each lane runs several batches of its share of the context's slots."""
    movie = texture(256, 24)
    kw = dict(speed_alpha=1.0, remodelling_alpha=1e4, rtol=1e-10, max_pairs_in_flight=5)
    assert_same(solve(of, movie, 1, **kw), solve(of, movie, 2, **kw))


def test_nan_frame_in_one_lane(of):
    """A NaN pixel in frame 9 (pairs 8 and 9, both in the second lane): those two pairs are reported unconverged, every
    other pair is solved as with one lane."""
    movie = texture(512, 13)
    movie[9, 300, 301] = float("nan")
    kw = dict(speed_alpha=1.0, remodelling_alpha=1e4, rtol=1e-10, max_iterations=60)
    one = solve(of, movie, 1, **kw)
    many = solve(of, movie, 2, **kw)
    assert np.flatnonzero(many[1]["converged"] == 0).tolist() == [8, 9]
    good = many[1]["converged"] == 1
    assert many[1]["relative_residual"][good].max() < 1e-10
    assert_same(one, many, good)


def test_direct_fallback_after_the_lanes(of):
    """A grad-div dominated regime (tests/test_gpu_parity.py: rescued by the direct preconditioner): the multigrid attempt
    runs in lanes, the direct re-solve of what it leaves unconverged after they join."""
    movie = orc.make_texture_stack(66, 5, seed=5) * 255.0
    kw = dict(speed_alpha=1e4, remodelling_alpha=1e2, rtol=1e-9, max_iterations=60)
    one = solve(of, movie, 1, **kw)
    many = solve(of, movie, 2, **kw)
    assert many[1]["converged"].all() and many[1]["relative_residual"].max() <= 1e-9
    assert_same(one, many)
