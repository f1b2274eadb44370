"""The active list: after a batch's first count the launches of a Krylov round cover the pairs still
being solved instead of every slot of the batch.  Blocks of finished pairs did nothing before, so the list changes which blocks
exist and nothing they compute: with VOF_ACTIVE_LIST=0 (every launch over all slots, as before) the fields and the per-pair
statistics are the same bits.

Every case makes the active set mixed by construction: in a stack with repeated frames the pairs of two equal frames have a zero
right-hand side and are finished before the first round, and warm_start_stride=0 keeps the other pairs from starting at their
(zero) solutions.  Each solve runs in a context of its own, because the switch is read when a context is created."""
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


def stack_with_repeats(n, frames, seed, scale=None):
    """frames frames of the synthetic texture in the order f0 f0 f1 f2 f2 f3 f4 f4 f5 ...: every third pair is a pair of equal
    frames."""
    distinct = frames - (frames + 1) // 3
    tex = orc.make_texture_stack(n, distinct, seed=seed)
    if scale is not None:
        tex = np.round(tex * scale)
    order, k = [], 0
    for i in range(frames):
        order.append(k)
        if i % 3 != 0:
            k += 1
    assert order[:7] == [0, 0, 1, 2, 2, 3, 4] and order[-1] == distinct - 1
    return np.ascontiguousarray(tex[order])


def solve_host(native, movie, params):
    with native.Solver(movie.shape[1], movie.shape[2], movie.shape[0] - 1) as s:
        return s.solve_host(movie, params)


def solve_dev(native, movie, params):
    import torch
    dev = torch.device("cuda", 0)
    mv = torch.from_numpy(movie).to(dev)
    out = [torch.empty((movie.shape[0] - 1,) + movie.shape[1:], dtype=torch.float64, device=dev) for _ in range(4)]
    with native.Solver(movie.shape[1], movie.shape[2], movie.shape[0] - 1) as s:
        stats = s.solve_dev(mv, movie.shape[0], params, *out)
        torch.cuda.synchronize()
    return (*[o.cpu().numpy() for o in out], stats)


def with_and_without_list(monkeypatch, solve, native, movie, params):
    monkeypatch.delenv("VOF_ACTIVE_LIST", raising=False)
    on = solve(native, movie, params)
    monkeypatch.setenv("VOF_ACTIVE_LIST", "0")
    off = solve(native, movie, params)
    return on, off


def assert_same_bits(on, off):
    it = on[4]["iterations"]
    print("iterations", it.tolist(), "converged", on[4]["converged"].tolist(), "relres", on[4]["relative_residual"].tolist())
    assert it.min() < it.max(), it          # the active set was mixed: some launches ran with fewer listed pairs than slots
    for name, a, b in zip(("v_x", "v_y", "remodelling", "speed"), on[:4], off[:4]):
        assert np.array_equal(a, b), name
    for f in STAT_FIELDS:
        assert np.array_equal(on[4][f], off[4][f]), f


@pytest.mark.parametrize("min_blocks", ["0", None], ids=["k_sweep0r", "k_sweep0m"])
def test_level0_passes_take_the_list(native, monkeypatch, min_blocks):
    """130 x 258, 6 pairs.  VOF_SWEEP0R_MIN_BLOCKS=0: the register-resident pass with the folded vector updates (BF), the coarse
    right-hand side as its trailing stage (TRAIL = 2) and the float32 hand-off; default threshold: the LDS-ring pass k_sweep0m."""
    if min_blocks is None:
        monkeypatch.delenv("VOF_SWEEP0R_MIN_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("VOF_SWEEP0R_MIN_BLOCKS", min_blocks)
    movie = stack_with_repeats(258, 7, seed=5)[:, :130, :]
    p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=0)
    assert_same_bits(*with_and_without_list(monkeypatch, solve_host, native, np.ascontiguousarray(movie), p))


def test_hard_regime_restarts_with_the_list(native, monkeypatch):
    """66 x 66 in the regime of test_native_sweep_resolves_hard_regime_in_both_branches (8-bit data, speed_alpha 1e4,
    remodelling_alpha 1e2, rtol 1e-9), which the cycle does not settle quickly: the pairs leave the BiCGStab rounds one by one,
    and the restart rounds or the GMRES hand-over run with a list."""
    movie = stack_with_repeats(66, 7, seed=5, scale=255.0)
    p = native.default_params(speed_alpha=1e4, remodelling_alpha=1e2, rtol=1e-9, warm_start_stride=0)
    assert_same_bits(*with_and_without_list(monkeypatch, solve_host, native, movie, p))


def test_lane_views_of_the_list(native, monkeypatch):
    """130 x 258 x 13 frames on two lanes of six pairs: each lane fills and reads its own view of the list and of its mirror, and
    each holds two pairs of equal frames."""
    monkeypatch.setenv("VOF_LANES", "2")
    monkeypatch.setenv("VOF_LANES_MIN_MPIX", "0")
    movie = np.ascontiguousarray(stack_with_repeats(258, 13, seed=5)[:, :130, :])
    p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=0)
    on, off = with_and_without_list(monkeypatch, solve_dev, native, movie, p)
    it = on[4]["iterations"]
    assert it[:6].min() < it[:6].max() and it[6:].min() < it[6:].max(), it   # mixed in both lanes
    assert_same_bits(on, off)
