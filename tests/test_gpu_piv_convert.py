"""GPU tests of upsample_PIV_vectors / convert_PIV_result (vof_piv_upsample_*, csrc/vof_piv.hpp).

The device is held to tests/piv_restatement.py bit for bit - values, the NaN pattern, speed and the counts - on host arrays and on
device tensors, at frames_in_flight 1, 2 and the library's choice, and from call to call.  The restatement itself is held to scipy
by tests/test_piv_convert_cpu.py, which also asserts that no inclusion decision of these cases hangs on the last bits.  A frame
on the host fallback is scipy's own evaluation, bit for bit.  Shapes: piv_restatement.CASES, the smallest at which the kernels can
go wrong (table offsets that differ per frame, a concave hull, slivers, several blocks with a partial last one)."""
import numpy as np
import pytest

import piv_restatement as pr

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", pr.CASES)
def test_device_equals_restatement(name):
    import torch
    from opticalflow_amd import _native, optical_flow as of
    c, want = pr.case(name), pr.restated(name)
    F, (N_i, N_j) = len(c["x"]), c["shape"]
    got = of.upsample_PIV_vectors(c["x"], c["y"], c["vx"], c["vy"], c["shape"])
    on_device = of.upsample_PIV_vectors(list(c["x"]), list(c["y"]), list(c["vx"]), list(c["vy"]), c["shape"], output="torch")
    for key, g, t, w in zip(("v_x", "v_y", "speed"), got, on_device, want):
        assert t.is_cuda and t.dtype == torch.float64
        print(name, key, "largest difference from the restatement", np.nanmax(np.abs(g - w)), "NaN pixels", int(np.isnan(g).sum()))
        assert same_bits(g, w), key
        assert same_bits(host(t), w), key
    tables = of.piv_tables(c["x"], c["y"], c["vx"], c["vy"])
    with _native.Solver(N_i, N_j, 1) as solver:
        for flight in (1, 2, 0):
            for repeat in range(2):
                outs = [np.empty((F, N_i, N_j)) for _ in range(3)]
                counts = solver.piv_upsample(tables, F, *outs, flight)
                assert np.array_equal(counts, want[3]), (flight, counts)
                assert all(same_bits(o, w) for o, w in zip(outs, want)), flight
            d_outs = [torch.empty((F, N_i, N_j), dtype=torch.float64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            counts = solver.piv_upsample(tables, F, *d_outs, flight)
            assert np.array_equal(counts, want[3]), (flight, counts)
            assert all(same_bits(host(o), w) for o, w in zip(d_outs, want)), flight


@pytest.mark.parametrize("output", ("numpy", "torch"))
def test_host_fallback_frame_is_scipys(monkeypatch, output):
    """Frame 1 of odd_grid forced onto the host fallback: scipy's evaluation of that frame bit for bit, the restatement's elsewhere."""
    from opticalflow_amd import optical_flow as of
    c, want, scipys = pr.case("odd_grid"), pr.restated("odd_grid"), pr.gridded("odd_grid")
    asked = []
    monkeypatch.setattr(of, "_piv_frame_on_host", lambda tri: asked.append(tri) or len(asked) == 2)
    outs, counts = of._upsample_PIV_vectors(c["x"], c["y"], c["vx"], c["vy"], c["shape"], 0, output)
    assert len(asked) == 4
    outs = [o if output == "numpy" else host(o) for o in outs]
    for o, w, s in zip(outs, want, scipys):
        assert same_bits(o[1], s[1])
        assert same_bits(o[[0, 2, 3]], w[[0, 2, 3]])
    assert counts[1] == 1 and counts[0] == want[3][0] == np.isnan(outs[0]).sum()


def test_result_feeds_the_filter_and_the_comparison():
    """convert_PIV_result(output="torch") -> filter_PIV_flow_result -> compare_flow_results on device tensors: the summaries of the
    same result as numpy arrays; delta_x = 0.5 and delta_t = 2 give the fields of the half_pixel case scaled by 0.25."""
    import torch
    from opticalflow_amd import optical_flow as of
    c = pr.case("odd_grid")
    PIV = pr.pivlab_result(c["x"][:2], c["y"][:2], c["vx"][:2], c["vy"][:2])
    movie = np.random.default_rng(194).integers(0, 256, (3, 37, 53)).astype(np.uint8)
    on_host = of.convert_PIV_result(PIV, movie, 0.5, 2)
    on_device = of.convert_PIV_result(PIV, torch.as_tensor(movie, device="cuda"), 0.5, 2, output="torch")
    half = pr.case("half_pixel")
    want = pr.upsample(half["x"], half["y"], c["vx"][:2] * 0.5 / 2, c["vy"][:2] * 0.5 / 2, (37, 53))
    for key, w in zip(("v_x", "v_y", "speed"), want):
        assert on_device[key].is_cuda and same_bits(on_host[key], w) and same_bits(host(on_device[key]), w), key
    for key in ("x_locations", "y_locations", "PIV_v_x", "PIV_v_y"):
        assert isinstance(on_device[key], np.ndarray) and same_bits(on_device[key], on_host[key])
    of.filter_PIV_flow_result(on_host, 100.0, 1.0, reference_quirks=False)
    of.filter_PIV_flow_result(on_device, 100.0, 1.0, reference_quirks=False)
    for key in ("v_x", "v_y", "speed"):
        assert same_bits(host(on_device[key]), on_host[key]) and (on_host[key] == 0.0).any() and np.isnan(on_host[key]).any(), key

    def other(r):
        return dict(v_x=r["v_y"], v_y=r["v_x"], speed=r["speed"])
    a = of.compare_flow_results(on_host, other(on_host), speed_threshold=0.05, angle_threshold=0.05)
    b = of.compare_flow_results(on_device, other(on_device), speed_threshold=0.05, angle_threshold=0.05)
    assert sorted(a) == sorted(b) and a["joint_count"] > 0 and a["angle_count"] > 0
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
