"""GPU tests of conduct_opencv_flow: v_x, v_y and speed equal the numpy restatement (tests/farneback_restatement.py) bit for
bit - np.array_equal, no tolerance.  Each test first asserts, on the restatement's record, that its input takes the path it is
there for."""
import functools

import numpy as np
import pytest

import farneback_restatement as R
from farneback_cases import CASES, case_arguments, case_input

pytestmark = pytest.mark.gpu

FIELDS = ("v_x", "v_y", "speed")


@functools.lru_cache(maxsize=None)
def reference(name):
    rec = {}
    out = R.conduct_opencv_flow(case_input(name), rec=rec, **case_arguments(name))
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
    got = of().conduct_opencv_flow(movie, **case_arguments(name), **extra)
    assert sorted(got) == ["delta_t", "delta_x", "original_data", "speed", "v_x", "v_y"]       # no blurred_data key
    assert got["original_data"] is movie and got["v_x"].shape == (T - 1, N_i, N_j)
    same(got, want)
    return got


def band(shape):
    b = np.ones(shape, dtype=bool)
    b[5:-5, 5:-5] = False
    return b


def test_smallest_whole_run():
    want, pairs = reference("smallest")
    assert len(pairs) == 2 and pairs[0]["sizes"] == [(40, 52)] and len(pairs[0]["flows"][0]) == 1 + 2
    assert not np.array_equal(want["v_x"][0], want["v_x"][1])                   # the third frame is not the first: pairs differ
    assert np.isfinite(want["speed"]).all() and want["speed"].max() > 0.3
    check("smallest")


def test_two_levels_with_tie_rounded_sizes():
    _, pairs = reference("two_levels")
    assert pairs[0]["sizes"] == [(75, 91), (38, 46)] and 75 * 0.5 == 37.5 and 91 * 0.5 == 45.5
    assert pairs[0]["ksizes"] == [3, 3] and not np.array_equal(pairs[0]["presmooth_taps"][1], pairs[0]["presmooth_taps"][0])
    assert np.abs(pairs[0]["flows"][0][0]).max() > 0                           # level 0 starts from the upsampled coarse flow
    check("two_levels")


def test_three_levels_non_dyadic():
    _, pairs = reference("three_levels")
    p = pairs[0]
    assert len(p["sizes"]) == 3 and p["sizes"][0] == (128, 160) and p["ksizes"][1] == 3
    assert p["presmooth_taps"][1][1] != np.float32(0.5)                         # ksize = 3 with sigma > 0: computed taps
    assert float(np.float32(1 / 0.7)) != 1 / 0.7                                     # the float32 scalar of the carried flow
    check("three_levels")


def test_outside_branch_beside_and_away_from_the_border_band():
    _, pairs = reference("outside")
    out = pairs[0]["outside"][0]
    b = band(out.shape)
    assert (out & b).sum() > 0 and (out & ~b).sum() > 0
    check("outside")


@pytest.mark.parametrize("name", ["wide_window", "no_window"])
def test_window_extremes(name):
    _, pairs = reference(name)
    m = len(pairs[0]["window_taps"]) - 1
    assert m == (25 if name == "wide_window" else 0)
    if name == "wide_window":
        assert m > 40 // 2                                                      # rows clamp on both sides at once
    else:
        assert pairs[0]["window_taps"][0] == np.float32(1)
    check(name)


@pytest.mark.parametrize("name", ["poly_7", "poly_sigma_0"])
def test_polynomial_tables(name):
    _, pairs = reference(name)
    g = pairs[0]["poly"]["g"]
    assert len(g) == (15 if name == "poly_7" else 11)
    if name == "poly_sigma_0":
        assert np.array_equal(g, R.poly_tables(5, 5 * 0.3)["g"]) and not np.array_equal(g, R.poly_tables(5, 1.1)["g"])    # 0.3 n
    check(name)


@pytest.mark.parametrize("name", ["wide", "tiny"])
def test_row_shapes(name):
    _, pairs = reference(name)
    h, w = pairs[0]["sizes"][0]
    if name == "wide":
        assert w > 256 and w % 2 == 1 and h == 33                               # two row workgroups, rows off 8-byte boundaries
    else:
        assert (h, w) == (16, 16) and band((16, 16)).sum() == 256 - 36          # all but the 6 x 6 centre lies in a border band
    check(name)


def test_no_iterations_and_one():
    want, pairs = reference("no_iterations")
    assert len(pairs[0]["sizes"]) == 2 and all(len(f) == 1 for f in pairs[0]["flows"])
    assert not want["v_x"].any() and not want["speed"].any()                    # zero, upsampled: zero
    got = check("no_iterations")
    assert not got["v_y"].any()
    _, pairs = reference("one_iteration")
    assert all(len(f) == 2 for f in pairs[0]["flows"]) and pairs[0]["M"][0] is not None
    check("one_iteration")
    # one level without iterations
    movie = case_input("smallest")
    r = of().conduct_opencv_flow(movie, **dict(case_arguments("smallest"), iterations=0))
    assert all(not r[k].any() and r[k].shape == (2, 40, 52) for k in FIELDS)


def test_blurred_first_image_and_units():
    movie = case_input("blurred")
    args = case_arguments("blurred")
    got = of().conduct_opencv_flow(movie, 0.5, 2, 1.3, **args)
    blurred = got["original_data"]
    assert blurred is not movie and blurred.shape == movie.shape and sorted(got) == ["delta_t", "delta_x", "original_data", "speed", "v_x", "v_y"]
    assert np.array_equal(blurred, of().blur_movie(movie, 1.3)) and (got["delta_x"], got["delta_t"]) == (0.5, 2)
    want = R.conduct_opencv_flow(movie, 0.5, 2, blurred=blurred, **args)
    same(got, want)
    unmixed = R.conduct_opencv_flow(blurred, 0.5, 2, **args)                    # both images blurred: another result
    assert not np.array_equal(unmixed["v_x"], want["v_x"])
    plain, _ = reference("blurred")
    assert np.array_equal(R.conduct_opencv_flow(movie, 0.5, 2, **args)["v_x"], plain["v_x"] * 0.25)


def test_cross_checks():
    import torch
    from opticalflow_amd import _native
    name = "smallest"
    movie, args = case_input(name), case_arguments(name)
    want, _ = reference(name)
    first = check(name)
    same(of().conduct_opencv_flow(movie, **args), first)                                         # a second call
    tensor = torch.as_tensor(movie.copy()).cuda()
    dev = of().conduct_opencv_flow(tensor, output="torch", **args)                               # the torch entry, device tensor
    assert all(dev[k].dtype == torch.float64 and dev[k].is_cuda for k in FIELDS) and dev["original_data"] is tensor
    same({k: dev[k].cpu().numpy() for k in FIELDS}, want)
    host = of().conduct_opencv_flow(movie.copy(), output="torch", **args)                        # the torch entry, host array
    same({k: host[k].cpu().numpy() for k in FIELDS}, want)
    plan = of().farneback_plan(40, 52, **{k: v for k, v in args.items() if k != "iterations"})
    frames = movie.astype(np.float64)
    with _native.Solver(40, 52, 1) as solver:
        d = tensor.to(torch.float64)
        for flight in (1, 2, 0):
            got = solver.farneback_host(frames[:-1], frames[1:], plan, args["iterations"], frames_in_flight=flight)
            same(dict(zip(FIELDS, got)), want)
            out = [torch.zeros((2, 40, 52), dtype=torch.float64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            solver.farneback_dev(d[:-1], d[1:], 2, plan, args["iterations"], 1.0, *out, frames_in_flight=flight)
            same({k: o.cpu().numpy() for k, o in zip(FIELDS, out)}, want)
        # two aliased views of one movie against two separate copies
        got = solver.farneback_host(frames[:-1].copy(), frames[1:].copy(), plan, args["iterations"])
        same(dict(zip(FIELDS, got)), want)


def plan_of(name, N_i, N_j):
    return of().farneback_plan(N_i, N_j, **{k: v for k, v in case_arguments(name).items() if k != "iterations"})


@functools.lru_cache(maxsize=None)
def reversed_reference():
    """"smallest" with its frames in reverse order."""
    out = R.conduct_opencv_flow(np.ascontiguousarray(case_input("smallest")[::-1]), **case_arguments("smallest"))
    return {k: out[k] for k in FIELDS}


def test_nothing_staged_survives_a_call():
    """One context, two views of one host array at one address: both stacks are staged whole (frames_in_flight=0), the array is
    overwritten in place (the frames in reverse order, so both stacks change), and the second call sees the new frames."""
    from opticalflow_amd import _native
    name = "smallest"
    iterations = case_arguments(name)["iterations"]
    frames = case_input(name).astype(np.float64)
    with _native.Solver(40, 52, 1) as solver:
        first = solver.farneback_host(frames[:-1], frames[1:], plan_of(name, 40, 52), iterations, frames_in_flight=0)
        frames[...] = frames[::-1].copy()
        second = solver.farneback_host(frames[:-1], frames[1:], plan_of(name, 40, 52), iterations, frames_in_flight=0)
    same(dict(zip(FIELDS, first)), reference(name)[0])
    same(dict(zip(FIELDS, second)), reversed_reference())
    assert not np.array_equal(second[0], first[0])


def test_range_is_accumulated_over_chunks_and_stacks():
    """One pair in flight; a NaN in the last frame of the movie is in `second` alone, one in frame 0 is in the first chunk of
    `first` alone - not in the chunk its range reduction leaves staged."""
    from opticalflow_amd import _native
    name = "smallest"
    iterations = case_arguments(name)["iterations"]
    movie = case_input(name).astype(np.float64)
    with _native.Solver(40, 52, 1) as solver:
        for frame in (2, 0):
            frames = movie.copy()
            frames[frame, 7, 9] = np.nan
            with pytest.raises(ValueError, match="non-finite"):
                solver.farneback_host(frames[:-1], frames[1:], plan_of(name, 40, 52), iterations, frames_in_flight=1)
        got = solver.farneback_host(movie[:-1], movie[1:], plan_of(name, 40, 52), iterations, frames_in_flight=1)
    same(dict(zip(FIELDS, got)), reference(name)[0])


# ---- one context, every owner of the frame-chunk scratch buffer in turn -----------------------------------------------------
# 41 x 53, the shape of the resize case "mixed_counts"; the other inputs are committed cases padded to it by repeating their
# last row / column: "smallest" (40 x 52) for the flow, "blurred" (37 x 53) for the threshold, "A" (37 x 53) for CLAHE.
def padded(movie):
    return np.pad(movie, ((0, 0), (0, 41 - movie.shape[1]), (0, 53 - movie.shape[2])), mode="edge")


@functools.lru_cache(maxsize=None)
def sequence_inputs():
    from preprocess_cases import clahe_input, threshold_input
    from resize_cases import case_input as resize_input
    return {"flow": padded(case_input("smallest")).astype(np.float64), "resize": resize_input("mixed_counts", "u8").astype(np.float64),
            "threshold": padded(threshold_input("blurred")), "clahe": padded(clahe_input("A"))}


@functools.lru_cache(maxsize=None)
def sequence_references():
    import preprocess_restatement
    import resize_restatement
    inputs = sequence_inputs()
    flow = R.conduct_opencv_flow(inputs["flow"].astype(np.uint8), **case_arguments("smallest"))
    rec = {}
    clahe = preprocess_restatement.clahe(inputs["clahe"], 50000, 4, rec)
    return {"flow": {k: flow[k] for k in FIELDS}, "resize": resize_restatement.resize_area(inputs["resize"].astype(np.uint8), 8, 10),
            "threshold": preprocess_restatement.adaptive_threshold(inputs["threshold"], 11, 2.5), "clahe": clahe,
            "tiles": (rec["tilesX"], rec["tilesY"])}


def run_sequence(after_each_call=lambda solver: None):
    """Farnebaeck _host (the largest request), uint8 resize _host with two frames in flight, threshold _host, CLAHE _dev,
    Farnebaeck _dev on one context; every result is checked against its restatement.  Between them a blur _host and a box-size
    sweep _host, checked against fresh contexts."""
    import torch
    from opticalflow_amd import _native
    inputs, want = sequence_inputs(), sequence_references()
    iterations = case_arguments("smallest")["iterations"]
    plan = plan_of("smallest", 41, 53)
    flow = inputs["flow"]
    results = []
    with _native.Solver(41, 53, 1) as solver:
        def done(got, key):
            after_each_call(solver)
            if key == "flow":
                same(dict(zip(FIELDS, got)), want[key])
            else:
                assert np.array_equal(got, want[key]), key
            assert all(np.isfinite(g).all() for g in (got if key == "flow" else [got])), key
            results.append(got)

        def as_on_a_fresh_context(call):
            """The blur and the box-size sweep take their scratch from the same buffer: each equals its run on a context of its own."""
            got = call(solver)
            after_each_call(solver)
            with _native.Solver(41, 53, 1) as fresh:
                want_fresh = call(fresh)
            for g, w in zip(got, want_fresh):
                assert g.dtype == w.dtype and g.shape == w.shape and (g.tobytes() == w.tobytes() or np.array_equal(g, w, equal_nan=True))

        done(solver.farneback_host(flow[:-1], flow[1:], plan, iterations), "flow")
        as_on_a_fresh_context(lambda s: (s.blur_host(flow, of().gaussian_taps(1.5)),))
        done(solver.resize_area_host(inputs["resize"], 8, 10, _native.RESIZE_U8, frames_in_flight=2), "resize")
        as_on_a_fresh_context(lambda s: (lambda r: (r[0], r[1], *r[3]))(s.vary_boxsize_host(
            flow, (5, 12), include_remodelling=True, histogram_edges=np.linspace(0.0, 4.0, 9), return_fields=True)))
        done(solver.adaptive_threshold_host(inputs["threshold"], 11, 2.5), "threshold")
        frames = torch.as_tensor(inputs["clahe"]).cuda()
        out = torch.zeros(frames.shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        solver.clahe_dev(frames, out, frames.shape[0], 50000, *want["tiles"])
        done(out.cpu().numpy(), "clahe")
        d = torch.as_tensor(flow).cuda()
        fields = [torch.zeros((2, 41, 53), dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        solver.farneback_dev(d[:-1], d[1:], 2, plan, iterations, 1.0, *fields)
        done(tuple(f.cpu().numpy() for f in fields), "flow")
    return results


@functools.lru_cache(maxsize=None)
def plain_sequence():
    return run_sequence()


def test_one_context_serves_every_owner_of_the_scratch_buffer():
    """A smaller request is carved anew inside the buffer a larger one left behind."""
    assert len(plain_sequence()) == 5


def test_scratch_buffer_under_guard_regions_and_poison(monkeypatch):
    """The same sequence with guard regions around every device buffer and poisoned (0xFF: NaN) allocations: no guard region is
    touched by any call, and the results are those of the plain run (finite: run_sequence asserts it)."""
    plain = plain_sequence()
    monkeypatch.setenv("VOF_DEBUG_CANARY", "1")
    monkeypatch.setenv("VOF_DEBUG_POISON", "1")
    guarded = run_sequence(lambda solver: solver.check_canaries())
    for got, want in zip(guarded, plain):
        for g, w in zip(got, want) if isinstance(got, tuple) else [(got, want)]:
            assert np.array_equal(g, w)


def test_errors_leave_the_context_usable():
    name = "smallest"
    movie, args = case_input(name), case_arguments(name)
    check(name)
    nan = movie.astype(np.float64)
    nan[1, 7, 9] = np.nan
    inf = movie.astype(np.float64)
    inf[2, 39, 51] = np.inf
    bad = [(ValueError, movie.astype(np.float32), args), (ValueError, movie.astype(np.int64), args), (ValueError, movie[:, :15], args),
           (ValueError, movie[0], args), (ValueError, movie[:1], args), (ValueError, nan, args), (ValueError, inf, args),
           (ValueError, movie, dict(args, pyr_scale=1.0)), (ValueError, movie, dict(args, pyr_scale=0.0)), (ValueError, movie, dict(args, levels=-1)),
           (ValueError, movie, dict(args, winsize=0)), (ValueError, movie, dict(args, winsize=130)), (ValueError, movie, dict(args, iterations=-1)),
           (ValueError, movie, dict(args, poly_n=0)), (ValueError, movie, dict(args, poly_n=11)),
           (TypeError, movie, {k: v for k, v in args.items() if k != "poly_sigma"}), (TypeError, movie, dict(args, box_size=3)),
           (TypeError, movie, dict(args, flags=256))]
    for error, m, a in bad:
        with pytest.raises(error):
            of().conduct_opencv_flow(m, **a)
        check(name)                                                             # the context still serves a good call


def test_clahe_into_flow_stays_on_the_device():
    import torch
    movie = case_input("smallest")
    tensor = torch.as_tensor(movie.astype(np.float64) * 200.0).cuda()
    clahed = of().apply_clahe(tensor, 50000, 4, output="torch")
    assert clahed.is_cuda and clahed.dtype == torch.float64
    args = case_arguments("smallest")
    r = of().conduct_opencv_flow(clahed, output="torch", **args)
    assert r["original_data"] is clahed and all(r[k].is_cuda and tuple(r[k].shape) == (2, 40, 52) for k in FIELDS)
    want = R.conduct_opencv_flow(clahed.cpu().numpy(), **args)
    same({k: r[k].cpu().numpy() for k in FIELDS}, want)
