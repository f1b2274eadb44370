"""GPU tests of correct_intensity_change (vof_intensity_correct_*) and intensity_histograms (vof_intensity_hist_*).

Bounds, none of them taken from what the GPU gives:
* the correction, bit for bit against the unfused chain made of the library's own public pieces - blur_movie three times and numpy
  subtractions - whatever the device blur's last bit is; bit for bit against tests/intensity_restatement.py (IEEE multiply / add in
  the stated order, contraction off); against the scipy chain within 16 * eps * 255: the project's bar for one device blur is 4 ulp
  of the data range (tests/test_gpu_consumers.py), and the chain stacks two blurs of the data, one of a difference bounded by the
  range and two subtractions.  The largest difference is printed; 0 is expected;
* the reference frame's output is Tg[reference_frame] and its drift +0.0, bit for bit;
* histogram counts equal np.histogram exactly.  Every exact comparison first asserts on the values alone that none lies within 1e-9
  of an interior edge unless exactly on it (uint8 values on the integer edges of 255 bins over (0, 255) are exactly on them, and a
  value on an edge is binned by comparisons against the same edges in numpy and in the kernel); the float and blurred stacks have
  no value on an edge at all.

Shapes are the smallest at which the kernels take another path: see intensity_restatement.GPU_CASES."""
import functools

import numpy as np
import pytest

import intensity_restatement as ir

pytestmark = pytest.mark.gpu
BOUND = 16 * ir.EPS * 255


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def references(case, target):
    """(restatement out, restatement drift, scipy out) of a case at reference_frame 0, computed once."""
    shape, s1, s2 = ir.GPU_CASES[case]
    out, drift = ir.correct(ir.case_stack(shape), s1, s2, target, 0)
    want = ir.scipy_correct(ir.case_stack(shape), s1, s2, target, 0)
    for a in (out, drift, want):
        a.setflags(write=False)
    return out, drift, want


def unfused_chain(of, movie, s1, s2, target, ref):
    frames = np.asarray(movie, dtype=np.float64)
    B = frames if s1 is None else of.blur_movie(frames, s1)
    E = of.blur_movie(B - B[ref], s2)
    return (B if target == "blurred" else frames) - E, E, (B if target == "blurred" else frames)


@pytest.mark.parametrize("target", ir.TARGETS)
@pytest.mark.parametrize("case", range(len(ir.GPU_CASES)))
def test_correction_cases(case, target):
    import torch
    from opticalflow_amd import optical_flow as of
    shape, s1, s2 = ir.GPU_CASES[case]
    movie = ir.case_stack(shape)
    out, drift = of.correct_intensity_change(movie, s1, s2, target=target, return_drift=True)
    assert out.dtype == drift.dtype == np.float64 and out.shape == drift.shape == shape
    t_out, t_drift = of.correct_intensity_change(torch.as_tensor(np.array(movie), device="cuda"), s1, s2, target=target, return_drift=True,
                                                 output="torch")
    assert t_out.is_cuda and t_drift.is_cuda and t_out.dtype == torch.float64
    assert same_bits(host(t_out), out) and same_bits(host(t_drift), drift)
    assert same_bits(of.correct_intensity_change(movie, s1, s2, target=target), out)              # without the drift's store
    chain_out, chain_drift, Tg = unfused_chain(of, movie, s1, s2, target, 0)
    r_out, r_drift, s_out = references(case, target)
    print(shape, s1, s2, target, "largest difference: unfused chain", np.abs(out - chain_out).max(), "restatement", np.abs(out - r_out).max(),
          "scipy chain", np.abs(out - s_out).max())
    assert same_bits(out, chain_out) and same_bits(drift, chain_drift)
    assert same_bits(out, r_out) and same_bits(drift, r_drift)
    assert np.abs(out - s_out).max() <= BOUND
    assert same_bits(out[0], Tg[0]) and not drift[0].any() and not np.signbit(drift[0]).any()


@functools.lru_cache(maxsize=None)
def chunk_reference(target, ref):
    shape, s1, s2 = ir.CHUNK_CASE
    out, drift = ir.correct(ir.case_stack(shape), s1, s2, target, ref)
    out.setflags(write=False), drift.setflags(write=False)
    return out, drift


@pytest.mark.parametrize("target", ir.TARGETS)
def test_reference_frame_in_another_chunk(target):
    """18 frames of 8 x 12: more than BLUR_CHUNK and than the 16 frames in flight the library picks, reference_frame 17 and -18 through
    the public entry; frames_in_flight 1, 5 and 0 through Solver, on host arrays and on device tensors."""
    import torch
    from opticalflow_amd import _native, optical_flow as of
    shape, s1, s2 = ir.CHUNK_CASE
    movie = ir.case_stack(shape)
    frames = movie.astype(np.float64)
    for ref in (17, -18):
        out, drift = of.correct_intensity_change(movie, s1, s2, target=target, reference_frame=ref, return_drift=True)
        r_out, r_drift = chunk_reference(target, ref)
        chain_out, chain_drift, Tg = unfused_chain(of, movie, s1, s2, target, ref)
        assert same_bits(out, r_out) and same_bits(drift, r_drift)
        assert same_bits(out, chain_out) and same_bits(drift, chain_drift)
        assert same_bits(out[ref], Tg[ref]) and not drift[ref].any() and not np.signbit(drift[ref]).any()
    which = _native.INTENSITY_TARGETS.index(target)
    r_out, r_drift = chunk_reference(target, 17)
    with _native.Solver(shape[1], shape[2], 1) as solver:
        for flight in (1, 5, 0):
            out, drift = np.empty(shape), np.empty(shape)
            solver.intensity_correct(frames, shape[0], ir.taps(s1), ir.taps(s2), 17, which, out, drift, flight)
            assert same_bits(out, r_out) and same_bits(drift, r_drift), flight
            d_frames = torch.as_tensor(frames, device="cuda")
            d_out, d_drift = torch.empty_like(d_frames), torch.empty_like(d_frames)
            torch.cuda.synchronize()
            solver.intensity_correct(d_frames, shape[0], ir.taps(s1), ir.taps(s2), 17, which, d_out, d_drift, flight)
            assert same_bits(host(d_out), r_out) and same_bits(host(d_drift), r_drift), flight


@pytest.mark.parametrize("target", ir.TARGETS)
def test_nan_propagates_through_the_taps(target):
    from opticalflow_amd import optical_flow as of
    movie = ir.integer_stack((2, 12, 20), 5).astype(np.float64)
    movie[1, 4, 7] = np.nan
    out, drift = of.correct_intensity_change(movie, target=target, return_drift=True)
    r_out, r_drift = ir.correct(movie, 3, 5, target, 0)
    assert np.isnan(r_out[1]).any() and np.isfinite(r_out[0]).all()
    assert np.array_equal(out, r_out, equal_nan=True) and np.array_equal(drift, r_drift, equal_nan=True)


# ---- histograms ---------------------------------------------------------------------------------------------------------------
def check_histograms(got, F, bins, value_range, on_edges):
    """got against np.histogram of the float64 stack F; on_edges: values exactly on an interior edge are expected (and allowed)."""
    gap = ir.edge_gap(F, bins, value_range)
    edges = np.linspace(value_range[0], value_range[1], bins + 1)
    exact = int(np.isin(F[np.isfinite(F)], edges[1:-1]).sum())
    print(f"    {F.shape}, {bins} bins: smallest non-zero distance to an interior edge {gap:.3e}, {exact} values exactly on one")
    assert gap > ir.GAP_BOUND, "a value within 1e-9 of an edge: the exact comparison would not be meaningful; choose another seed"
    assert on_edges or exact == 0
    counts, nonfinite = ir.histograms(F, bins, value_range)
    assert sorted(got) == ["counts", "edges", "nonfinite"]
    assert got["counts"].dtype == np.int64 and got["nonfinite"].dtype == np.int64 and got["counts"].shape == (F.shape[0], bins)
    assert np.array_equal(got["edges"], edges)
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(got["nonfinite"], nonfinite)
    assert np.array_equal(got["counts"].sum(1) + ir.dropped(F, value_range), np.full(F.shape[0], F[0].size))


def test_histograms_of_a_uint8_stack():
    """255 bins over (0, 255): the edges are the integers, 254 and 255 share the last bin; host array and device tensor."""
    import torch
    from opticalflow_amd import optical_flow as of
    movie = ir.integer_stack((5, 37, 53), 11)
    assert (movie == 254).any() and (movie == 255).any()
    got = of.intensity_histograms(movie)
    check_histograms(got, movie.astype(np.float64), 255, (0, 255), on_edges=True)
    assert got["counts"][:, 254].sum() == np.count_nonzero(movie >= 254)
    dev = of.intensity_histograms(torch.as_tensor(movie, device="cuda"), output="torch")
    for key in got:
        assert np.array_equal(dev[key], got[key]), key


def test_histograms_of_the_blurred_stack():
    from opticalflow_amd import optical_flow as of
    movie = ir.integer_stack((5, 37, 53), 11)
    got = of.intensity_histograms(movie, smoothing_sigma=1.3)
    check_histograms(got, of.blur_movie(movie, 1.3), 255, (0, 255), on_edges=False)


def test_histograms_past_the_lds_counters():
    from opticalflow_amd import optical_flow as of
    movie = np.random.default_rng(12).random((3, 37, 53)) * 255.0
    got = of.intensity_histograms(movie, bins=1500, value_range=(0, 255))
    check_histograms(got, movie, 1500, (0, 255), on_edges=False)


def test_histograms_do_not_depend_on_frames_in_flight():
    import torch
    from opticalflow_amd import _native
    movie = np.random.default_rng(13).random((18, 8, 12)) * 255.0
    edges = np.linspace(0, 255, 256)
    w = ir.taps(1.0)
    plain, blurred = ir.histograms(movie, 255, (0, 255)), None
    with _native.Solver(8, 12, 1) as solver:
        F = solver.blur_host(movie, w)
        assert ir.edge_gap(movie, 255, (0, 255)) > ir.GAP_BOUND and ir.edge_gap(F, 255, (0, 255)) > ir.GAP_BOUND
        blurred = ir.histograms(F, 255, (0, 255))
        for flight in (1, 5, 0):
            for taps, want in ((None, plain), (w, blurred)):
                counts, nonfinite = solver.intensity_hist(movie, 18, edges, taps, flight)
                assert np.array_equal(counts, want[0]) and np.array_equal(nonfinite, want[1]), flight
                d_movie = torch.as_tensor(movie, device="cuda")
                torch.cuda.synchronize()
                counts, nonfinite = solver.intensity_hist(d_movie, 18, edges, taps, flight)
                assert np.array_equal(counts, want[0]) and np.array_equal(nonfinite, want[1]), flight


def test_histograms_drop_what_numpy_drops():
    """Values below lo, above hi, NaN and +-Inf: all dropped, the non-finite ones counted per frame."""
    from opticalflow_amd import optical_flow as of
    rng = np.random.default_rng(14)
    movie = rng.uniform(-50.0, 300.0, (4, 21, 30))
    movie[0, 1, 2], movie[0, 3, 4], movie[2, 5, 6], movie[2, 7, 8], movie[2, 9, 10] = np.nan, np.inf, -np.inf, np.nan, np.nan
    movie[1, 0, 0], movie[1, 0, 1], movie[3, 20, 29] = 0.0, 255.0, 255.0          # the two ends of the range are inside
    got = of.intensity_histograms(movie, bins=64, value_range=(0, 255))
    check_histograms(got, movie, 64, (0, 255), on_edges=False)
    assert list(got["nonfinite"]) == [2, 0, 3, 0]
    assert (ir.dropped(movie, (0, 255)) > 50).all() and got["counts"][1, 0] >= 1 and got["counts"][3, 63] >= 1


def test_pipeline_stays_on_the_device():
    """downsample_movie -> correct_intensity_change -> variational_optical_flow on device tensors: no stage returns host memory."""
    import torch
    from opticalflow_amd import optical_flow as of
    rng = np.random.default_rng(15)
    i, j = np.meshgrid(np.arange(96), np.arange(80), indexing="ij")
    movie = np.stack([np.clip(120 + 10 * k + 60 * np.sin((i + 1.5 * k) / 7.0) * np.cos((j - k) / 9.0) + rng.normal(0, 2, i.shape), 0, 255)
                      for k in range(3)]).astype(np.uint8)
    small = of.downsample_movie(torch.as_tensor(movie, device="cuda"), (48, 40), output="torch")
    corrected = of.correct_intensity_change(small, 3, 7.5, target="original", output="torch")
    assert small.is_cuda and corrected.is_cuda and tuple(corrected.shape) == (3, 48, 40) and corrected.dtype == torch.float64
    assert torch.equal(corrected[0], small[0])
    result = of.variational_optical_flow(corrected, speed_alpha=255.0 ** 2, remodelling_alpha=1e3, output="torch")
    for key in ("v_x", "v_y", "remodelling", "speed"):
        assert result[key].is_cuda and tuple(result[key].shape) == (2, 48, 40), key
        assert bool(torch.isfinite(result[key]).all()), key
