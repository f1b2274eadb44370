"""GPU tests of the Liu-Shen Jacobi flow (liu_shen_optical_flow_jit / conduct_variational_optical_flow_deprecated /
vof_liu_shen_*): the fused LDS kernel and the one-iteration kernel against the reference's fixtures and the numpy
restatement.

Bound: e = max|gpu - ref| / max(|ref v_x|, |ref v_y|) <= 1e-12 over both fields, every pixel.  It is set from the error of
the restatement against the reference (operation order and the closed-form inverse are the only differences: at most
2.2e-15 after up to 150 iterations), with a margin of about 300, never from what the GPU gives.  Every comparison prints
its error before it asserts.  Results of different fusion depths, tile positions and entry points must be bit-equal: the
iteration is Jacobi and every pixel's update is one expression."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from liushen_restatement import liu_shen, error  # noqa: E402
from test_liushen_cpu import arguments  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 1e-12
CASES = ["a", "b", "c", "d", "e"]
# the wrapper takes scalar guesses only: case d (planes as initial fields) goes through the function alone
RUNS = [(c, e) for c in CASES for e in ("function", "wrapper") if not (c == "d" and e == "wrapper")]


def to_numpy(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def set_depth(monkeypatch, depth):
    if depth is None:
        monkeypatch.delenv("VOF_LIUSHEN_FUSE", raising=False)
    else:
        monkeypatch.setenv("VOF_LIUSHEN_FUSE", str(depth))


def texture(n_i, n_j, frames=2, seed=5):
    from oracle import vof_oracle as orc
    n = max(n_i, n_j)
    return np.ascontiguousarray(orc.make_texture_stack(n, frames, seed=seed)[:, :n_i, :n_j])


def check(got_x, got_y, ref_x, ref_y, label):
    got_x, got_y = to_numpy(got_x), to_numpy(got_y)
    assert got_x.shape == ref_x.shape and got_y.shape == ref_y.shape, label
    assert np.isfinite(got_x).all() and np.isfinite(got_y).all(), label
    e = error(got_x, got_y, ref_x, ref_y)
    print(f"{label}: e = {e:.3g}")
    assert e <= BOUND, (label, e)
    return e


@pytest.mark.parametrize("output", ["numpy", "torch"])
@pytest.mark.parametrize("case,entry", RUNS)
def test_fixture_cases(case, entry, output):
    from opticalflow_amd import optical_flow as of
    g = load_golden(f"g12{case}_liushen.npz")
    args = arguments(g)
    if entry == "function":
        v_x, v_y, speed, remodelling, last = of.liu_shen_optical_flow_jit(*args, output=output)
        assert last == int(g["last_iteration"])
    else:
        movie, dx, dt, alpha, _, gx, gy, gr, iterations = args
        res = of.conduct_variational_optical_flow_deprecated(movie, dx, dt, alpha, 1.0, gx, gy, gr, iterations, use_liu_shen=True,
                                                             output=output)
        v_x, v_y, speed, remodelling = res["v_x"], res["v_y"], res["speed"], res["remodelling"]
        assert res["original_data"] is movie and res["blurred_data"] is movie
        assert (res["delta_x"], res["delta_t"], res["max_iterations"], res["total_iterations"]) == (dx, dt, iterations, iterations)
        assert sorted(res) == sorted(["v_x", "v_y", "speed", "remodelling", "original_data", "blurred_data", "delta_x", "delta_t",
                                      "max_iterations", "total_iterations"])
    if output == "torch":
        import torch
        assert all(isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.float64 for f in (v_x, v_y, speed, remodelling))
    label = f"{case} {entry} {output}"
    check(v_x, v_y, g["v_x"], g["v_y"], label)
    check(speed, speed, g["speed"], g["speed"], label + " speed")
    assert np.array_equal(to_numpy(remodelling), g["remodelling"]), label
    v_x, v_y, speed = to_numpy(v_x), to_numpy(v_y), to_numpy(speed)
    assert np.array_equal(speed, np.sqrt(v_x ** 2 + v_y ** 2)), label


@pytest.mark.parametrize("depth", [1, None])
def test_many_tiles_against_the_restatement(depth, monkeypatch):
    """130 x 258, 3 pairs, 40 iterations: tiles in both directions, partial tiles on both far edges."""
    from opticalflow_amd import optical_flow as of
    set_depth(monkeypatch, depth)
    movie = texture(130, 258, frames=4, seed=7)
    rng = np.random.default_rng(3)
    i_x, i_r = 0.1 * rng.standard_normal((130, 258)), rng.random((3, 130, 258))
    args = (movie, 0.5, 0.25, 0.3, 1.0, i_x, -0.05, i_r, 40)
    ref = liu_shen(*args)
    got = of.liu_shen_optical_flow_jit(*args)
    check(got[0], got[1], ref[0], ref[1], f"130x258 depth {depth}")
    check(got[2], got[2], ref[2], ref[2], f"130x258 depth {depth} speed")
    assert np.array_equal(got[3], i_r) and got[4] == 39


@pytest.mark.parametrize("shape,iterations", [((100, 150), 23), ((67, 33), 9), ((4, 4), 7)])
def test_fusion_depths_are_bit_equal(shape, iterations, monkeypatch):
    """VOF_LIUSHEN_FUSE = 1, intermediate depths, the default and the largest: the same bits, with iteration counts that are no
    multiple of the depth (23 = 5 * 4 + 3 = 7 * 3 + 2 = 2 * 8 + 7) and images of several, partial and single tiles."""
    from opticalflow_amd import optical_flow as of
    movie = texture(*shape, frames=3, seed=9) * 255.0
    args = (movie, 0.5, 2.0, 10.0, 1.0, 0.1, 0.2, 0.0, iterations)
    results = {}
    for depth in (1, 3, None, 8):
        set_depth(monkeypatch, depth)
        results[depth] = of.liu_shen_optical_flow_jit(*args)
    assert np.isfinite(results[1][0]).all() and results[1][0].any()
    for depth in (3, None, 8):
        for f in range(4):
            diff = np.abs(results[depth][f] - results[1][f]).max()
            print(f"{shape} depth {depth} field {f}: max difference {diff}")
            assert np.array_equal(results[depth][f], results[1][f]), (shape, depth, f, diff)


def test_invalid_fusion_depth_is_an_error(monkeypatch):
    from opticalflow_amd import optical_flow as of, _native
    for bad in ("0", "9", "x"):
        monkeypatch.setenv("VOF_LIUSHEN_FUSE", bad)
        with pytest.raises(_native.VofError, match="VOF_LIUSHEN_FUSE"):
            of.liu_shen_optical_flow_jit(texture(16, 16), max_iterations=2)


def torch_output_against_the_host_path(kind, n_i, n_j, frames, iterations):
    import torch
    from opticalflow_amd import optical_flow as of
    movie = texture(n_i, n_j, frames=frames, seed=2)
    rng = np.random.default_rng(8)
    pairs = (frames - 1, n_i, n_j)
    shape = {"scalar": (), "plane": pairs[1:], "stack": pairs}[kind]
    init = [0.2 * rng.standard_normal(shape) for _ in range(3)]
    if kind == "scalar":
        init = [float(f) for f in init]
    host = of.liu_shen_optical_flow_jit(movie, 0.3, 0.7, 0.2, 1.0, *init, iterations)
    dev_init = init if kind == "scalar" else [torch.as_tensor(f).cuda() for f in init]
    dev = of.liu_shen_optical_flow_jit(torch.as_tensor(movie).cuda(), 0.3, 0.7, 0.2, 1.0, *dev_init, iterations, output="torch")
    assert host[4] == dev[4] == iterations - 1
    assert np.isfinite(host[0]).all() and host[0].any()
    for f in range(4):
        assert np.array_equal(host[f], dev[f].cpu().numpy()), (kind, f)
    assert np.array_equal(host[3], np.broadcast_to(init[2], pairs))
    # mixed forms are passed in the widest one
    mixed = of.liu_shen_optical_flow_jit(movie, 0.3, 0.7, 0.2, 1.0, init[0], init[1], 0.25, iterations)
    assert np.array_equal(mixed[0], host[0]) and np.all(mixed[3] == 0.25)


@pytest.mark.parametrize("kind", ["scalar", "plane", "stack"])
def test_torch_output_is_bit_equal_to_the_host_path(kind):
    torch_output_against_the_host_path(kind, 70, 90, 4, 11)


@pytest.mark.parametrize("depth", [None, 1])
@pytest.mark.parametrize("kind", ["scalar", "plane", "stack"])
def test_torch_output_is_bit_equal_to_the_host_path_of_two_chunks(kind, depth, monkeypatch):
    """11 frames of 12 x 20: host arrays go through the library as chunks of 8 and 2 pairs, with the initial stacks offset
    by the chunk, the device tensors as one chunk of 10."""
    set_depth(monkeypatch, depth)
    torch_output_against_the_host_path(kind, 12, 20, 11, 7)


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_step_record(output):
    """The wrapper's record: bit-equal to chunked calls of the project's own function, and within the bound of the record the
    reference function wrote when called in chunks (case e)."""
    from opticalflow_amd import optical_flow as of
    g = load_golden("g12e_liushen.npz")
    movie, dx, dt, alpha, _, gx, gy, gr, iterations = arguments(g)
    step = int(g["iteration_stepsize"])
    res = of.conduct_variational_optical_flow_deprecated(movie, dx, dt, alpha, 1.0, gx, gy, gr, iterations, return_iterations=True,
                                                         iteration_stepsize=step, use_liu_shen=True, output=output)
    records = iterations // step
    assert res["iteration_stepsize"] == step and res["total_iterations"] == iterations
    steps = {k: to_numpy(res[k + "_steps"]) for k in ("v_x", "v_y", "speed", "remodelling")}
    for k, s in steps.items():
        assert s.shape == (1, records + 1) + movie.shape[1:] == g[k + "_steps"].shape
        assert np.array_equal(to_numpy(res[k]), s[:, -1])
    assert np.all(steps["v_x"][:, 0] == gx) and np.all(steps["v_y"][:, 0] == gy) and np.all(steps["remodelling"] == gr)
    assert np.array_equal(steps["speed"][:, 0], g["speed_steps"][:, 0])
    this = (gx, gy, gr)
    for r in range(1, records + 1):
        own = of.liu_shen_optical_flow_jit(movie, dx, dt, alpha, 1.0, *this, step)
        for f, k in enumerate(("v_x", "v_y", "speed", "remodelling")):
            assert np.array_equal(steps[k][:, r], own[f]), (r, k)
        check(steps["v_x"][:, r], steps["v_y"][:, r], g["v_x_steps"][:, r], g["v_y_steps"][:, r], f"record {r} {output}")
        check(steps["speed"][:, r], steps["speed"][:, r], g["speed_steps"][:, r], g["speed_steps"][:, r], f"record {r} {output} speed")
        this = (own[0], own[1], own[3])


def test_step_record_restarts_per_pair():
    """More than one pair (the reference's wrapper cannot broadcast there): pair k restarts from its own record, so every pair
    equals the one-pair run of its two frames."""
    from opticalflow_amd import optical_flow as of
    movie = texture(40, 48, frames=3, seed=4)
    kw = dict(speed_alpha=0.4, max_iterations=9, return_iterations=True, iteration_stepsize=3, use_liu_shen=True)
    both = of.conduct_variational_optical_flow_deprecated(movie, 0.5, 0.25, **kw)
    assert both["v_x_steps"].shape == (2, 4, 40, 48)
    for k in range(2):
        one = of.conduct_variational_optical_flow_deprecated(movie[k:k + 2], 0.5, 0.25, **kw)
        for name in ("v_x_steps", "v_y_steps", "speed_steps", "remodelling_steps"):
            assert np.array_equal(both[name][k], one[name][0]), (k, name)


def test_wrapper_blurs_first():
    from opticalflow_amd import optical_flow as of
    movie = texture(48, 40, frames=3, seed=6)
    res = of.conduct_variational_optical_flow_deprecated(movie, speed_alpha=0.5, max_iterations=5, smoothing_sigma=1.5,
                                                         use_liu_shen=True)
    blurred = of.blur_movie(movie, smoothing_sigma=1.5)
    assert np.array_equal(res["blurred_data"], blurred) and res["original_data"] is movie
    own = of.liu_shen_optical_flow_jit(blurred, 1.0, 1.0, 0.5, 1000.0, 0.1, 0.1, 0.5, 5)
    assert np.array_equal(res["v_x"], own[0]) and np.array_equal(res["speed"], own[2])
    dev = of.conduct_variational_optical_flow_deprecated(movie, speed_alpha=0.5, max_iterations=5, smoothing_sigma=1.5,
                                                         use_liu_shen=True, output="torch")
    assert np.array_equal(dev["v_x"].cpu().numpy(), res["v_x"])


def test_value_errors():
    from opticalflow_amd import optical_flow as of
    movie = texture(16, 16, frames=3)
    with pytest.raises(ValueError, match="max_iterations"):
        of.liu_shen_optical_flow_jit(movie, max_iterations=0)
    with pytest.raises(ValueError, match="sides"):
        of.liu_shen_optical_flow_jit(movie[:, :2], max_iterations=2)
    with pytest.raises(ValueError, match="initial fields"):
        of.liu_shen_optical_flow_jit(movie, initial_v_x=np.zeros((10, 10)), max_iterations=2)
    with pytest.raises(ValueError, match="initial fields"):
        of.liu_shen_optical_flow_jit(movie, initial_v_x=np.zeros((10, 10)), max_iterations=2, output="torch")
    with pytest.raises(ValueError, match="liu shen"):
        of.conduct_variational_optical_flow_deprecated(movie, use_liu_shen=False)
    with pytest.raises(ValueError, match="output"):
        of.liu_shen_optical_flow_jit(movie, max_iterations=2, output="cupy")


def test_singular_block_stores_what_ieee_division_gives():
    """A zero frame pair with alpha = 0: every 2 x 2 block is the zero matrix (the reference raises there)."""
    from opticalflow_amd import optical_flow as of
    v_x, v_y, speed, remodelling, _ = of.liu_shen_optical_flow_jit(np.zeros((2, 8, 8)), alpha=0.0, max_iterations=1)
    assert np.isnan(v_x).all() and np.isnan(v_y).all() and not remodelling.any()
