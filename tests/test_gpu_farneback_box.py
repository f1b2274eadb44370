"""GPU tests of the box window of Farnebaeck's flow: conduct_opencv_flow(..., window="box") and calcOpticalFlowFarneback equal
the numpy restatement (tests/farneback_box_restatement.py) bit for bit - np.array_equal, no tolerance; the restatement adds in
OpenCV's order, and tests/test_farneback_box_cpu.py shows that a re-associated sum gives other bits.  Each test first asserts, on
the restatement's record, that its input takes the path it is there for."""
import functools

import numpy as np
import pytest

import farneback_box_restatement as B
import farneback_restatement as R
from farneback_box_cases import CASES, case_arguments, case_input

pytestmark = pytest.mark.gpu

FIELDS = ("v_x", "v_y", "speed")


@functools.lru_cache(maxsize=None)
def reference(name):
    rec = {}
    out = B.conduct_opencv_flow_box(case_input(name), rec=rec, **case_arguments(name))
    for k in FIELDS:
        out[k].setflags(write=False)
    return out, rec["pairs"]


def of():
    from opticalflow_amd import optical_flow
    return optical_flow


def same(got, want):
    for k in FIELDS:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))


def check(name, **extra):
    movie = case_input(name)
    (T, N_i, N_j), depth, _, _ = CASES[name]
    assert movie.shape == (T, N_i, N_j) and movie.dtype == (np.uint8 if depth == "u8" else np.float64)
    want, _ = reference(name)
    got = of().conduct_opencv_flow(movie, window="box", **case_arguments(name), **extra)
    assert sorted(got) == ["delta_t", "delta_x", "original_data", "speed", "v_x", "v_y"]
    assert got["original_data"] is movie and got["v_x"].shape == (T - 1, N_i, N_j)
    same(got, want)
    return got


def test_smallest_whole_run():
    want, pairs = reference("box_smallest")
    assert len(pairs) == 2 and pairs[0]["sizes"] == [(40, 52)] and len(pairs[0]["flows"][0]) == 1 + 2 and pairs[0]["m"] == 4
    assert not np.array_equal(want["v_x"][0], want["v_x"][1])
    assert np.isfinite(want["speed"]).all() and want["speed"].max() > 0.3
    got = check("box_smallest")
    gaussian = of().conduct_opencv_flow(case_input("box_smallest"), **case_arguments("box_smallest"))
    assert not np.array_equal(gaussian["v_x"], got["v_x"])                       # the default is still the Gaussian window
    same(gaussian, R.conduct_opencv_flow(case_input("box_smallest"), **case_arguments("box_smallest")))


def test_the_script_s_call():
    """compare_rho_and_actin.py:903: levels=1 (two images), an even winsize (21 x 21 values over 400), poly_n=3."""
    _, pairs = reference("box_script")
    p = pairs[0]
    assert p["sizes"] == [(75, 91), (38, 46)] and p["winsize"] == 20 and p["m"] == 10 and (2 * p["m"] + 1) ** 2 != p["winsize"] ** 2
    assert len(p["poly"]["g"]) == 7 and np.abs(p["flows"][0][0]).max() > 0      # level 0 starts from the upsampled coarse flow
    check("box_script")


@pytest.mark.parametrize("name", ["box_m1", "box_w3"])
def test_smallest_windows(name):
    _, pairs = reference(name)
    assert pairs[0]["m"] == 1 and pairs[0]["winsize"] == (2 if name == "box_m1" else 3)     # no start rows: range(1, m) is empty
    check(name)


@pytest.mark.parametrize("name", ["box_over", "box_wide_window", "box_max"])
def test_windows_wider_than_the_image(name):
    _, pairs = reference(name)
    h, w = pairs[0]["sizes"][0]
    m = pairs[0]["m"]
    if name == "box_over":
        assert (h, w, m) == (16, 16, 20) and m - 1 > h - 1 and m - 1 > w - 1    # both start loops run past the last row and column
    elif name == "box_wide_window":
        assert m == 25 and m > h // 2                                           # rows clamp on both sides at once
    else:
        assert m == 64 and m > h and m > w
    check(name)


@pytest.mark.parametrize("name", ["box_wide", "box_tall"])
def test_many_tiles_and_bands(name):
    _, pairs = reference(name)
    h, w = pairs[0]["sizes"][0]
    if name == "box_wide":
        assert (h, w) == (33, 333) and w > 10 * 32 and w % 32 and w % 2 == 1 and h % 8    # 11 column tiles of 32, the last one partial, as is the last row band
    else:
        assert (h, w) == (333, 33) and h > 10 * 32 and h % 8 and w > 32         # a chain of 333 rows over many row bands (the last one partial), two column tiles
    check(name)


def test_translation():
    want, _ = reference("box_translation")
    assert abs(want["v_x"][0, 12:-12, 12:-12].mean() + 0.4) <= 0.02 and abs(want["v_y"][0, 12:-12, 12:-12].mean() - 0.6) <= 0.02
    check("box_translation")


def test_no_iterations_and_one():
    want, pairs = reference("no_iterations")
    assert len(pairs[0]["sizes"]) == 2 and all(len(f) == 1 for f in pairs[0]["flows"])
    assert not want["v_x"].any() and not want["speed"].any()
    got = check("no_iterations")
    assert not got["v_y"].any()
    _, pairs = reference("one_iteration")
    assert all(len(f) == 2 for f in pairs[0]["flows"]) and pairs[0]["M"][0] is not None
    check("one_iteration")


def test_blurred_first_image_and_units():
    movie = case_input("blurred")
    args = case_arguments("blurred")
    got = of().conduct_opencv_flow(movie, 0.5, 2, 1.3, window="box", **args)
    blurred = got["original_data"]
    assert blurred is not movie and blurred.shape == movie.shape and sorted(got) == ["delta_t", "delta_x", "original_data", "speed", "v_x", "v_y"]
    assert np.array_equal(blurred, of().blur_movie(movie, 1.3)) and (got["delta_x"], got["delta_t"]) == (0.5, 2)
    want = B.conduct_opencv_flow_box(movie, 0.5, 2, blurred=blurred, **args)
    same(got, want)
    plain, _ = reference("blurred")
    assert not np.array_equal(want["v_x"], plain["v_x"] * 0.25)                  # the blurred first image changes the result


@pytest.mark.parametrize("name", ["box_smallest", "box_script"])
def test_calc_optical_flow_farneback(name):
    import torch
    movie, args = case_input(name), case_arguments(name)
    positional = [args[k] for k in R.NAMES]
    h, w = movie.shape[1:]
    want_box = B.farneback_pair_box(movie[0], movie[1], **args)
    want_gaussian = R.farneback_pair(movie[0], movie[1], **args)
    assert want_box.dtype == np.float32 and want_box.shape == (h, w, 2) and not np.array_equal(want_box, want_gaussian)
    want, _ = reference(name)
    assert np.array_equal(want_box[:, :, 0], want["v_x"][0]) and np.array_equal(want_box[:, :, 1], want["v_y"][0])
    cv = of().calcOpticalFlowFarneback
    for flags, expected in ((0, want_box), (of().OPTFLOW_FARNEBACK_GAUSSIAN, want_gaussian)):
        got = cv(movie[0], movie[1], None, *positional, flags)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (h, w, 2)
        assert np.array_equal(got, expected), flags
        buffer = np.zeros((h, w, 2), dtype=np.float32)                          # flow: accepted and ignored
        assert np.array_equal(cv(movie[0], movie[1], buffer, *positional, flags=flags), expected) and not buffer.any()
        prev, nxt = (torch.as_tensor(f.copy()).cuda() for f in (movie[0], movie[1]))
        dev = cv(prev, nxt, None, *positional, flags, output="torch")
        assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (h, w, 2)
        assert np.array_equal(dev.cpu().numpy(), expected), flags


def test_cross_checks():
    import torch
    from opticalflow_amd import _native
    name = "box_smallest"
    movie, args = case_input(name), case_arguments(name)
    want, _ = reference(name)
    first = check(name)
    same(of().conduct_opencv_flow(movie, window="box", **args), first)                              # a second call
    tensor = torch.as_tensor(movie.copy()).cuda()
    dev = of().conduct_opencv_flow(tensor, output="torch", window="box", **args)
    assert all(dev[k].dtype == torch.float64 and dev[k].is_cuda for k in FIELDS) and dev["original_data"] is tensor
    same({k: dev[k].cpu().numpy() for k in FIELDS}, want)
    plan = of().farneback_plan(40, 52, **{k: v for k, v in args.items() if k != "iterations"})
    frames = movie.astype(np.float64)
    with _native.Solver(40, 52, 1) as solver:
        d = tensor.to(torch.float64)
        for flight in (1, 2, 0):
            got = solver.farneback_host(frames[:-1], frames[1:], plan, args["iterations"], frames_in_flight=flight, box=True)
            same(dict(zip(FIELDS, got)), want)
            out = [torch.zeros((2, 40, 52), dtype=torch.float64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            solver.farneback_dev(d[:-1], d[1:], 2, plan, args["iterations"], 1.0, *out, frames_in_flight=flight, box=True)
            same({k: o.cpu().numpy() for k, o in zip(FIELDS, out)}, want)
        # two aliased views of one movie against two separate copies
        got = solver.farneback_host(frames[:-1].copy(), frames[1:].copy(), plan, args["iterations"], box=True)
        same(dict(zip(FIELDS, got)), want)


# ---- one context: the two per-pair scratch sizes (27 and 32 planes) and a resize re-carve one buffer ----------------------------
def run_sequence(after_each_call=lambda solver: None):
    """Gaussian _host, box _host, Gaussian _dev, box _dev, then a uint8 resize on one context; every result is checked against
    its restatement and is finite."""
    import torch
    import resize_restatement
    from opticalflow_amd import _native
    name = "box_smallest"
    movie, args = case_input(name), case_arguments(name)
    frames = movie.astype(np.float64)
    plan = of().farneback_plan(40, 52, **{k: v for k, v in args.items() if k != "iterations"})
    box, _ = reference(name)
    gaussian = R.conduct_opencv_flow(movie, **args)
    results = []
    with _native.Solver(40, 52, 1) as solver:
        def done(got, want):
            after_each_call(solver)
            same(dict(zip(FIELDS, got)), want)
            assert all(np.isfinite(g).all() for g in got)
            results.append(got)

        done(solver.farneback_host(frames[:-1], frames[1:], plan, args["iterations"]), gaussian)
        done(solver.farneback_host(frames[:-1], frames[1:], plan, args["iterations"], box=True), box)
        d = torch.as_tensor(frames).cuda()
        for is_box, want in ((False, gaussian), (True, box)):
            fields = [torch.zeros((2, 40, 52), dtype=torch.float64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            solver.farneback_dev(d[:-1], d[1:], 2, plan, args["iterations"], 1.0, *fields, box=is_box)
            done(tuple(f.cpu().numpy() for f in fields), want)
        small = solver.resize_area_host(frames, 8, 10, _native.RESIZE_U8, frames_in_flight=2)
        after_each_call(solver)
        assert np.array_equal(small, resize_restatement.resize_area(movie, 8, 10)) and np.isfinite(small).all()
        results.append((small,))
    return results


@functools.lru_cache(maxsize=None)
def plain_sequence():
    return run_sequence()


def test_one_context_serves_both_windows_and_a_resize():
    assert len(plain_sequence()) == 5


def test_scratch_buffer_under_guard_regions_and_poison(monkeypatch):
    """The same sequence with guard regions around every device buffer and poisoned (0xFF: NaN) allocations: no guard region is
    touched, and the results are those of the plain run (finite: run_sequence asserts it)."""
    plain = plain_sequence()
    monkeypatch.setenv("VOF_DEBUG_CANARY", "1")
    monkeypatch.setenv("VOF_DEBUG_POISON", "1")
    guarded = run_sequence(lambda solver: solver.check_canaries())
    for got, want in zip(guarded, plain):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_errors_leave_the_context_usable():
    name = "box_smallest"
    movie, args = case_input(name), case_arguments(name)
    positional = [args[k] for k in R.NAMES]
    check(name)
    nan = movie.astype(np.float64)
    nan[1, 7, 9] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        of().conduct_opencv_flow(nan, window="box", **args)
    check(name)
    with pytest.raises(ValueError, match="non-finite"):
        of().calcOpticalFlowFarneback(nan[0], nan[1], None, *positional, 0)
    check(name)
    bad = [(ValueError, movie, dict(args, window="boxx")), (ValueError, movie, dict(args, window="box", winsize=1)),
           (ValueError, movie, dict(args, window="box", winsize=130)), (ValueError, movie.astype(np.float32), dict(args, window="box")),
           (TypeError, movie, dict(args, window="box", flags=0))]
    for error, m, a in bad:
        with pytest.raises(error):
            of().conduct_opencv_flow(m, **a)
        check(name)                                                             # the context still serves a good call
    for flags in (4, 1, 260):
        with pytest.raises(ValueError):
            of().calcOpticalFlowFarneback(movie[0], movie[1], None, *positional, flags)
        check(name)
    # the native entry refuses winsize 1 itself (return code -1: VofError), and the context survives that too
    from opticalflow_amd import _native
    plan = of().farneback_plan(40, 52, **{k: v for k, v in dict(args, winsize=1).items() if k != "iterations"})
    frames = movie.astype(np.float64)
    with _native.Solver(40, 52, 1) as solver:
        with pytest.raises(_native.VofError, match="winsize"):
            solver.farneback_host(frames[:-1], frames[1:], plan, args["iterations"], box=True)
        got = solver.farneback_host(frames[:-1], frames[1:], of().farneback_plan(40, 52, **{k: v for k, v in args.items() if k != "iterations"}),
                                    args["iterations"], box=True)
    same(dict(zip(FIELDS, got)), reference(name)[0])
