"""CPU tests of the box window of Farnebaeck's flow (conduct_opencv_flow(..., window="box"), calcOpticalFlowFarneback): the
restatement's running sums against a direct clamped window sum - close to it, and not equal to it, so the GPU tests can tell
OpenCV's order of additions from a re-associated sum - the axis and sign convention, and the argument checks that need no device."""
import functools

import numpy as np
import pytest

import farneback_box_restatement as B
import farneback_restatement as R
from farneback_box_cases import CASES, case_arguments, case_input

FLOWS = ("v_x", "v_y")
# |flow from the running sums - flow from the direct sum| over a whole run.  1e-4 everywhere but on the two 3 x 3 windows, whose
# sums of nine values leave the smallest determinants: measured 1.01e-4 on box_m1 (it reaches 1e-4, so the bound is raised above it)
# and 8.4e-5 on box_w3; at most 3.1e-6 on every other case.
BOUND = {name: 1e-4 for name in CASES}
BOUND["box_m1"] = 1.5e-4


def direct_sums(M, m):
    """The clamped (2 m + 1)^2 window sums in double, row offsets first, each axis summed offset by offset from -m to m."""
    _, h, w = M.shape
    rows, cols = np.arange(h), np.arange(w)
    V = np.zeros(M.shape)
    for d in range(-m, m + 1):
        V = V + M[:, np.clip(rows + d, 0, h - 1), :].astype(np.float64)
    g = np.zeros(M.shape)
    for d in range(-m, m + 1):
        g = g + V[:, :, np.clip(cols + d, 0, w - 1)]
    return g


def iterate_direct(M, winsize):
    return B.solve(direct_sums(M, winsize // 2), winsize)


@functools.lru_cache(maxsize=None)
def both(name):
    """The whole restatement with OpenCV's running sums, and with the direct sum in their place."""
    rec = {}
    running = B.conduct_opencv_flow_box(case_input(name), rec=rec, **case_arguments(name))
    direct = B.conduct_opencv_flow_box(case_input(name), iterate=iterate_direct, **case_arguments(name))
    return running, direct, rec["pairs"]


@pytest.mark.parametrize("winsize", [2, 3, 9, 20, 41, 129])
def test_running_sums_of_a_constant_are_exact(winsize):
    m = winsize // 2
    M = np.full((5, 19, 23), 0.375, dtype=np.float32) * np.arange(1, 6, dtype=np.float32)[:, None, None]
    g = B.running_sums(M, m)
    assert g.dtype == np.float64 and np.array_equal(g, M.astype(np.float64) * (2 * m + 1) ** 2)
    assert np.array_equal(g, direct_sums(M, m))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_close_to_a_direct_window_sum(name):
    running, direct, pairs = both(name)
    assert all(np.isfinite(running[k]).all() for k in FLOWS + ("speed",))
    assert pairs[0]["m"] == case_arguments(name)["winsize"] // 2 >= 1
    worst = max(float(np.abs(running[k] - direct[k]).max()) for k in FLOWS)
    print(f"{name}: largest |running - direct| {worst:.3g} (bound {BOUND[name]:g})")
    assert worst <= BOUND[name]


@pytest.mark.parametrize("name", ["box_smallest", "box_wide", "box_tall", "box_m1"])
def test_restatement_differs_from_a_direct_window_sum_in_bits(name):
    """What lets np.array_equal on the GPU tell an in-order sum from a re-associated one."""
    running, direct, _ = both(name)
    differing = np.mean([float(np.mean(running[k] != direct[k])) for k in FLOWS])
    print(f"{name}: {100 * differing:.0f} % of the flow values differ")
    assert differing > 0


def test_axis_and_sign_convention():
    """A texture moved by (+0.6 rows, -0.4 columns) per frame: channel 0 (v_x) runs along the columns, channel 1 along the rows."""
    movie = case_input("box_translation")
    assert movie.shape == (2, 64, 80)
    r = B.conduct_opencv_flow_box(movie, **case_arguments("box_translation"))
    v_x, v_y = r["v_x"][0, 12:-12, 12:-12].mean(), r["v_y"][0, 12:-12, 12:-12].mean()
    print(f"centre means: v_x {v_x:.4f} (shift -0.4 columns), v_y {v_y:.4f} (shift +0.6 rows)")
    assert abs(v_x - (-0.4)) <= 0.02 and abs(v_y - 0.6) <= 0.02
    pair = B.farneback_pair_box(movie[0], movie[1], **case_arguments("box_translation"))
    assert pair.dtype == np.float32 and pair.shape == (64, 80, 2) and np.array_equal(pair[:, :, 0], r["v_x"][0])


def test_box_result_differs_from_the_gaussian_one():
    name = "box_smallest"
    box = B.conduct_opencv_flow_box(case_input(name), **case_arguments(name))
    gaussian = R.conduct_opencv_flow(case_input(name), **case_arguments(name))
    assert box["v_x"].shape == gaussian["v_x"].shape and float(np.abs(box["v_x"] - gaussian["v_x"]).max()) > 1e-3


def test_restatement_excludes_winsize_1():
    with pytest.raises(ValueError, match="winsize"):
        B.conduct_opencv_flow_box(case_input("box_smallest"), **dict(case_arguments("box_smallest"), winsize=1))


def test_errors_that_need_no_device():
    from opticalflow_amd.optical_flow import calcOpticalFlowFarneback, conduct_opencv_flow
    movie = case_input("box_smallest")
    args = case_arguments("box_smallest")
    positional = [args[k] for k in R.NAMES]
    with pytest.raises(ValueError, match="window"):
        conduct_opencv_flow(movie, window="boxx", **args)
    with pytest.raises(ValueError, match="winsize"):
        conduct_opencv_flow(movie, window="box", **dict(args, winsize=1))
    with pytest.raises(TypeError, match="flags"):
        conduct_opencv_flow(movie, window="box", flags=0, **args)
    with pytest.raises(TypeError, match="flags"):
        conduct_opencv_flow(movie, flags=256, **args)
    for flags in (4, 1, 260):
        with pytest.raises(ValueError, match="not built|are built"):
            calcOpticalFlowFarneback(movie[0], movie[1], None, *positional, flags)
    with pytest.raises(ValueError, match="winsize"):
        calcOpticalFlowFarneback(movie[0], movie[1], None, *[1 if k == "winsize" else args[k] for k in R.NAMES], 0)
    with pytest.raises(ValueError, match="shape"):
        calcOpticalFlowFarneback(movie[0], movie[1][:, :-1], None, *positional, 0)
    with pytest.raises(ValueError, match="shape"):
        calcOpticalFlowFarneback(movie[:2], movie[1:], None, *positional, 0)
    with pytest.raises(ValueError, match="cast"):
        calcOpticalFlowFarneback(movie[0].astype(np.float32), movie[1].astype(np.float32), None, *positional, 0)
    with pytest.raises(ValueError, match="cast"):
        calcOpticalFlowFarneback(movie[0], movie[1].astype(np.float64), None, *positional, 0)
    with pytest.raises(ValueError, match="output"):
        calcOpticalFlowFarneback(movie[0], movie[1], None, *positional, 0, output="cupy")
    for change in (dict(pyr_scale=1.0), dict(levels=-1), dict(winsize=130), dict(iterations=-1), dict(poly_n=11), dict(poly_sigma=-1.0)):
        with pytest.raises(ValueError):
            calcOpticalFlowFarneback(movie[0], movie[1], None, *[dict(args, **change)[k] for k in R.NAMES], 0)
    with pytest.raises(ValueError):
        calcOpticalFlowFarneback(movie[0][:15], movie[1][:15], None, *positional, 0)
    with pytest.raises(TypeError):
        calcOpticalFlowFarneback(movie[0], movie[1], None, *[1.5 if k == "levels" else args[k] for k in R.NAMES], 0)


def test_no_cpu_fallback():
    """Without a HIP device the calls raise; they never compute on the CPU (with one, they compute there)."""
    import torch
    from opticalflow_amd import _native
    from opticalflow_amd.optical_flow import calcOpticalFlowFarneback, conduct_opencv_flow
    movie, args = case_input("box_smallest"), case_arguments("box_smallest")
    positional = [args[k] for k in R.NAMES]
    if torch.cuda.is_available():
        assert np.isfinite(conduct_opencv_flow(movie, window="box", **args)["speed"]).all()
        assert np.isfinite(calcOpticalFlowFarneback(movie[0], movie[1], None, *positional, 0)).all()
        return
    with pytest.raises(_native.VofError):
        conduct_opencv_flow(movie, window="box", **args)
    with pytest.raises(_native.VofError):
        calcOpticalFlowFarneback(movie[0], movie[1], None, *positional, 0)


def test_exports():
    import opticalflow_amd
    from opticalflow_amd import _native, optical_flow
    assert opticalflow_amd.calcOpticalFlowFarneback is optical_flow.calcOpticalFlowFarneback
    assert (opticalflow_amd.OPTFLOW_USE_INITIAL_FLOW, opticalflow_amd.OPTFLOW_FARNEBACK_GAUSSIAN) == (4, 256)
    for name in ("calcOpticalFlowFarneback", "OPTFLOW_USE_INITIAL_FLOW", "OPTFLOW_FARNEBACK_GAUSSIAN", "conduct_opencv_flow"):
        assert name in optical_flow.__all__
    assert {"vof_farneback_box_dev", "vof_farneback_box_host"} <= set(_native.SIGNATURES)
