"""GPU tests of conduct_piv's window deformation and outlier validation (vof_piv_flow_ex_*, csrc/vof_pivflow.hpp).

The device is held to tests/piv_deform_restatement.py bit for bit - u, v, the correlation, the NaN pattern, the counts and the
validation counts - for every case, from host arrays and from device tensors, at frames_in_flight 1, 2 and the library's choice, and
twice in a row.  The restatement itself is held to independent formulations by tests/test_piv_deform_cpu.py, which also asserts that
no decision of these cases hangs on the last bits.  Shapes: piv_deform_restatement.CASES, the smallest at which the kernels can go
wrong (grids of the two passes that differ in origin, step and size, a predictor from a deformed pass, a pass before with one row of
windows, the largest LDS need in a deformed pass, neighbourhoods of 3 to 8 valid vectors and of fewer than 3, fills and outliers,
the median test on the returned vectors, two frame pairs in flight)."""
import numpy as np
import pytest

import piv_deform_restatement as pd

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", pd.CASES)
def test_device_equals_restatement(name):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    c = pd.case(name)
    validating = c["outlier_threshold"] is not None
    movie = np.array(c["movie"])
    want_u, want_v, want_c, want_counts, want_validation, _ = pd.restated(name)
    assert movie.shape[0] == 3                                                # two pairs: frames_in_flight 1 and 2 split them differently
    if validating:
        assert want_validation.any()
    arguments = pd.arguments(name)
    for stack in (movie, torch.as_tensor(movie, device="cuda")):
        got = of.conduct_piv(stack, **arguments)
        for key, w in (("u_original", want_u), ("v_original", want_v), ("correlation", want_c)):
            finite = np.isfinite(w)
            print(name, key, "largest difference from the restatement", np.abs(got[key][finite] - w[finite]).max(initial=0.0), "NaN", int(np.isnan(w).sum()))
            assert isinstance(got[key], np.ndarray) and same_bits(got[key], w), key
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want_counts), got["counts"]
        assert ("validation_counts" in got) == validating
        if validating:
            assert got["validation_counts"].dtype == np.int64 and np.array_equal(got["validation_counts"], want_validation), got["validation_counts"]
    options = {k: c[k] for k in pd.OPTION_NAMES[1:]}
    d_movie = torch.as_tensor(movie, device="cuda")
    P, N_i, N_j = movie.shape[0] - 1, movie.shape[1], movie.shape[2]

    def check(returned, outs, where):
        counts, validation = returned if validating else (returned, None)
        assert np.array_equal(counts, want_counts), (where, counts)
        assert validation is None or np.array_equal(validation, want_validation), (where, validation)
        assert all(same_bits(o, w) for o, w in zip(outs, (want_u, want_v, want_c))), where

    with _native.Solver(N_i, N_j, 1) as solver:
        for flight in (1, 2, 0):
            for repeat in range(2):
                outs = [np.empty(want_u.shape) for _ in range(3)]
                check(solver.piv_flow(movie, P, c["window_sizes"], c["search_radii"], c["steps"], *outs, c["min_correlation"], flight, **options), outs,
                      (flight, repeat))
            d_outs = [torch.empty(want_u.shape, dtype=torch.float64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            returned = solver.piv_flow(d_movie, P, c["window_sizes"], c["search_radii"], c["steps"], *d_outs, c["min_correlation"], flight, **options)
            check(returned, [host(o) for o in d_outs], flight)


def test_the_library_refuses_what_python_refuses():
    """The ABI's own validation of the new arguments (Solver.piv_flow hands them on as they are): a VofError with a message."""
    from opticalflow_amd import _native
    frames = np.zeros((2, 40, 40))
    outs = [np.zeros((1, 40, 40)) for _ in range(3)]                         # room for any grid, were a request taken after all
    with _native.Solver(40, 40, 1) as solver:
        for options in (dict(outlier_threshold=0.0), dict(outlier_threshold=-1.0), dict(outlier_threshold=float("inf")),
                        dict(outlier_threshold=2.0, outlier_epsilon=-0.1), dict(outlier_threshold=2.0, outlier_epsilon=float("inf")),
                        dict(outlier_threshold=2.0, outlier_epsilon=float("nan")), dict(outlier_epsilon=-1.0), dict(deformation=2),
                        dict(deformation=-1), dict(outlier_threshold=2.0, validate_last=2), dict(validate_last=True)):
            with pytest.raises(_native.VofError, match="PIV"):
                solver.piv_flow(frames, 1, (8, 8), (2, 2), (4, 4), *outs, **options)
        with pytest.raises(_native.VofError, match="PIV"):                   # and what the plain call refuses, through the new entry
            solver.piv_flow(frames, 1, (8, 16), (2, 2), (4, 4), *outs, deformation=True)


def test_flow_result_on_host_and_device():
    """conduct_piv_flow with both options and validate_last: the same bits from a host array and from a device tensor, PIV_v_x the
    restatement's u times delta_x / delta_t, and no vector missing for the triangulation where the median test filled it."""
    import torch
    from opticalflow_amd import optical_flow as of
    c = pd.case("validation_last")
    arguments = dict(pd.arguments("validation_last"), deformation=True, outlier_threshold=2.0, validate_last=True)
    assert arguments == pd.arguments("validation_last")
    movie = np.array(c["movie"])
    on_host = of.conduct_piv_flow(movie, 0.5, 2.0, **arguments)
    on_device = of.conduct_piv_flow(torch.as_tensor(movie, device="cuda"), 0.5, 2.0, output="torch", **arguments)
    want = pd.restated("validation_last")
    assert same_bits(on_host["PIV_correlation"], want[2]) and same_bits(on_device["PIV_correlation"], want[2])
    assert same_bits(on_host["PIV_v_x"], want[0] * 0.5 / 2.0) and same_bits(on_device["PIV_v_x"], want[0] * 0.5 / 2.0)
    assert same_bits(on_host["PIV_v_y"], want[1] * 0.5 / 2.0) and same_bits(on_device["PIV_v_y"], want[1] * 0.5 / 2.0)
    for key in ("v_x", "v_y", "speed"):
        assert on_device[key].is_cuda and on_host[key].shape == (2,) + movie.shape[1:] and same_bits(host(on_device[key]), on_host[key]), key
        assert np.isfinite(on_host[key]).any()
