"""GPU tests of conduct_piv / conduct_piv_flow (vof_piv_flow_*, csrc/vof_pivflow.hpp).

The device is held to tests/piv_flow_restatement.py bit for bit - u, v, the correlation, the NaN pattern and the counts - for
every case, from host arrays and from device tensors, at frames_in_flight 1, 2 and the library's choice, and twice in a row.  The
restatement itself is held to an independent formulation by tests/test_piv_flow_cpu.py, which also asserts that no peak of these
cases hangs on the last bits (outside the crafted exact tie, which the first-in-raster-order rule decides).  Shapes:
piv_flow_restatement.CASES, the smallest at which the kernels can go wrong (a window that is no power of two, a step with a
remainder, search ranges that are and are not a multiple of the lanes' run of 3, rows that are and are not a multiple of the
double block of 6 steps, the largest window and radius the LDS takes, two passes with an offset that falls back)."""
import numpy as np
import pytest

import piv_flow_restatement as pf

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", pf.CASES)
def test_device_equals_restatement(name):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    c = pf.case(name)
    want_u, want_v, want_c, want_counts, _ = pf.restated(name)
    arguments = {k: c[k] for k in ("window_sizes", "search_radii", "steps", "min_correlation")}
    for movie in (c["movie"], torch.as_tensor(np.array(c["movie"]), device="cuda")):
        got = of.conduct_piv(movie, **arguments)
        for key, w in (("u_original", want_u), ("v_original", want_v), ("correlation", want_c)):
            finite = np.isfinite(w)
            print(name, key, "largest difference from the restatement", np.abs(got[key][finite] - w[finite]).max(initial=0.0), "NaN", int(np.isnan(w).sum()))
            assert isinstance(got[key], np.ndarray) and same_bits(got[key], w), key
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want_counts), got["counts"]
    last = of.piv_grid(c["movie"].shape, c["window_sizes"], c["search_radii"], c["steps"])[-1]
    assert got["x"].shape == want_u.shape and np.array_equal(got["x"][-1], last["x"]) and np.array_equal(got["y"][0], last["y"])
    frames = np.array(c["movie"], dtype=np.float64)
    d_frames = torch.as_tensor(frames, device="cuda")
    P, N_i, N_j = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
    with _native.Solver(N_i, N_j, 1) as solver:
        for flight in (1, 2, 0):
            for repeat in range(2):
                outs = [np.empty(want_u.shape) for _ in range(3)]
                counts = solver.piv_flow(frames, P, c["window_sizes"], c["search_radii"], c["steps"], *outs, c["min_correlation"], flight)
                assert np.array_equal(counts, want_counts), (flight, counts)
                assert all(same_bits(o, w) for o, w in zip(outs, (want_u, want_v, want_c))), (flight, repeat)
            d_outs = [torch.empty(want_u.shape, dtype=torch.float64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            counts = solver.piv_flow(d_frames, P, c["window_sizes"], c["search_radii"], c["steps"], *d_outs, c["min_correlation"], flight)
            assert np.array_equal(counts, want_counts), (flight, counts)
            assert all(same_bits(host(o), w) for o, w in zip(d_outs, (want_u, want_v, want_c))), flight


def test_blurred_movie_is_the_blur_then_the_restatement():
    """smoothing_sigma: the frames blur_movie gives, then the same arithmetic."""
    from opticalflow_amd import optical_flow as of
    c = pf.case("float_blurred")
    blurred = of.blur_movie(c["movie"], 1.5)
    want = pf.piv(blurred, c["window_sizes"], c["search_radii"], c["steps"])
    got = of.conduct_piv(c["movie"], c["window_sizes"], c["search_radii"], c["steps"], smoothing_sigma=1.5)
    assert same_bits(got["u_original"], want[0]) and same_bits(got["v_original"], want[1]) and same_bits(got["correlation"], want[2])
    assert np.array_equal(got["counts"], want[3])


def test_the_library_refuses_what_python_refuses():
    """The ABI's own validation (Solver.piv_flow goes past the Python checks): a VofError with a message, nothing computed."""
    from opticalflow_amd import _native
    frames = np.zeros((2, 40, 40))
    outs = [np.zeros((1, 40, 40)) for _ in range(3)]                         # room for any grid, were a request taken after all
    with _native.Solver(40, 40, 1) as solver:
        for w, r, s in (((3,), (2,), (1,)), ((65,), (2,), (1,)), ((8,), (0,), (4,)), ((8,), (17,), (4,)), ((8,), (2,), (0,)),
                        ((8, 16), (2, 2), (4, 4)), ((38,), (2,), (4,)), ((16, 8), (8, 9), (8, 4))):
            with pytest.raises(_native.VofError, match="PIV"):
                solver.piv_flow(frames, 1, w, r, s, *outs)


def test_flow_result_feeds_the_filter_and_the_comparison():
    """conduct_piv_flow(output="torch") -> filter_PIV_flow_result -> compare_flow_results on device tensors: the summaries of the
    numpy route."""
    import torch
    from opticalflow_amd import optical_flow as of
    c = pf.case("odd_edges")
    arguments = dict(window_sizes=c["window_sizes"], search_radii=c["search_radii"], steps=c["steps"])
    movie = np.array(c["movie"])
    on_host = of.conduct_piv_flow(movie, 0.5, 2.0, **arguments)
    on_device = of.conduct_piv_flow(torch.as_tensor(movie, device="cuda"), 0.5, 2.0, output="torch", **arguments)
    want = pf.restated("odd_edges")
    assert same_bits(on_host["PIV_correlation"], want[2]) and same_bits(on_device["PIV_correlation"], want[2])
    assert same_bits(on_host["PIV_v_x"], want[0] * 0.5 / 2.0) and same_bits(on_device["PIV_v_y"], want[1] * 0.5 / 2.0)
    for key in ("v_x", "v_y", "speed"):
        assert on_device[key].is_cuda and on_host[key].shape == (3, 37, 45) and same_bits(host(on_device[key]), on_host[key]), key
        assert np.isfinite(on_host[key]).any()
    # the vectors are whole pixels times 0.25: speeds 0.354 in pairs 0 and 2, 0.25 in pair 1, which alone stays under the filter's 0.3
    of.filter_PIV_flow_result(on_host, 100.0, 0.3, reference_quirks=False)
    of.filter_PIV_flow_result(on_device, 100.0, 0.3, reference_quirks=False)
    for key in ("v_x", "v_y", "speed"):
        assert same_bits(host(on_device[key]), on_host[key]), key
    print("largest speed the filter left, per pair:", [float(np.nanmax(s)) for s in on_host["speed"]])
    assert (on_host["speed"][0] == 0.0).any() and (on_host["speed"][1] > 0.05).any()

    def other(r):
        return dict(v_x=r["v_y"], v_y=r["v_x"], speed=r["speed"])
    a = of.compare_flow_results(on_host, other(on_host), speed_threshold=0.05, angle_threshold=0.05)
    b = of.compare_flow_results(on_device, other(on_device), speed_threshold=0.05, angle_threshold=0.05)
    assert sorted(a) == sorted(b) and a["joint_count"] > 0
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
