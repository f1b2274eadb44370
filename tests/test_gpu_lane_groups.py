"""Lane groups: the two-phase solve of a stack cut into groups of pairs, each lane running phase 1 then phase 2 of its groups
without a join between the phases (VOF_LANES, VOF_LANE_GROUPS).

Same bar as tests/test_gpu_lanes.py: against one lane, the same iteration counts and converged flags, and fields that agree
to 1e-9 of each field's max-abs, solved to rtol 1e-10 with VOF_LANES_MIN_MPIX=0.  Only which pairs share a batch changes, so
per pair the arithmetic is the same up to the order in which dot-product partials are added.

At 1024^2 with warm_start_stride 3 and 16 or more phase-1 pairs the two-phase warm start is on.  The group boundaries are
multiples of the stride; the last pair before a boundary takes its guess from the first phase-1 pair of the next group,
which another lane solves.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("v_x", "v_y", "remodelling", "speed")
SWITCHES = ("VOF_LANES", "VOF_LANE_GROUPS", "VOF_LANES_MIN_MPIX")


@pytest.fixture(scope="module")
def of():
    from opticalflow_amd import optical_flow
    return optical_flow


def solve(of, movie, lanes, groups, **kw):
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ.update(VOF_LANES=str(lanes), VOF_LANE_GROUPS=str(groups), VOF_LANES_MIN_MPIX="0")
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
    print("iterations", s2["iterations"].tolist())
    np.testing.assert_array_equal(s1["iterations"], s2["iterations"])
    np.testing.assert_array_equal(s1["converged"], s2["converged"])
    good = np.ones(len(s1), bool) if good is None else good
    for k in FIELDS:
        a, b = f1[k][good], f2[k][good]
        scale = max(float(np.abs(a).max()), 1e-300)
        diff = float(np.abs(a - b).max())
        print(k, "max difference / max-abs:", diff / scale)
        assert diff <= 1e-9 * scale, k


def texture(n, frames, seed=3):
    import torch
    from opticalflow_amd import synthetic
    return synthetic.texture_stack_torch(n, frames, seed, torch.device("cuda", 0))


@pytest.mark.parametrize("frames,lanes,groups", [
    (49, 2, 2),    # P = 48: 16 phase-1 pairs, four groups
    (51, 2, 2),    # P = 50: a group boundary between a warm pair and its source, and a last stride that is not full
    (50, 3, 2),    # P = 49, three lanes, six groups
    (52, 3, 1),    # P = 51, three lanes, one group each: no join between the phases, equal shares
])
def test_groups_match_one_lane(of, frames, lanes, groups):
    movie = texture(1024, frames)
    kw = dict(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=3, rtol=1e-10)
    one = solve(of, movie, 1, 1, **kw)
    many = solve(of, movie, lanes, groups, **kw)
    assert one[1]["converged"].all()
    assert many[1]["relative_residual"].max() < 1e-10
    assert_same(one, many)


def nan_case(of, size, frames, bad_frame):
    movie = texture(size, frames)
    movie[bad_frame, 300, 301] = float("nan")
    kw = dict(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=3, rtol=1e-10, max_iterations=60)
    one = solve(of, movie, 1, 1, **kw)
    many = solve(of, movie, 2, 2, **kw)
    bad = [bad_frame - 1, bad_frame]
    assert np.flatnonzero(one[1]["converged"] == 0).tolist() == bad
    assert np.flatnonzero(many[1]["converged"] == 0).tolist() == bad
    good = many[1]["converged"] == 1
    assert many[1]["relative_residual"][good].max() < 1e-10
    assert_same(one, many, good)


def test_nan_frame_in_a_foreign_source_small(of):
    """A NaN pixel in frame 7 of 13 at 512^2: pairs 6 and 7 fail.  Pair 6 is a phase-1 pair at a multiple of the stride, the
    guess of pairs 5 and 7.  (A stack this small is below the two-phase threshold of 16 Mpixel of phase-1 pairs, so it is
    solved in plain batches; the case below is the one that goes through the groups.)"""
    nan_case(of, 512, 13, 7)


def test_nan_frame_in_a_foreign_source(of):
    """1024^2, 49 frames, two lanes with two groups each: the groups start at the pairs 0, 9, 24 and 39.  A NaN pixel in frame
    25 makes the pairs 24 and 25 fail.  Pair 24 is the first phase-1 pair of the third group (lane 0) and the guess of pair
    23, the last of the second group (lane 1): pair 23 is solved from the constant fields exactly as with one lane, and the
    failing pairs are the same list."""
    nan_case(of, 1024, 49, 25)
