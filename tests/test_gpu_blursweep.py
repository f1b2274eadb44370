"""GPU tests of the blur sweep (vary_blursize / vof_vary_blursize_*) and of the LDS-tiled blur it brings.

Bounds, none of them taken from what the GPU gives:
* blur: bit-identical to k_blur1d (VOF_BLUR_TILED=0), the same values are added in the same order;
* fields of a sigma: bit-identical to conduct_optical_flow(..., smoothing_sigma=s) of this checkout, the same kernels run;
* counts, histograms (speed, direction, intensity) and probes: exact against numpy on the returned fields.  acos on the device
  and np.arccos may differ in their last bits, so the direction comparison is guarded: no numpy direction value may lie within
  1e-9 of an interior edge unless it is exactly on it (the smallest distance over all cases here is above 1e-7);
* means / standard deviations: rtol 1e-12 against numpy (the tolerance of tests/test_gpu_boxsweep.py for the same reduction);
* speed-weighted direction sums: |gpu - numpy| <= N * 2**-52 * bin_sum with N the number of samples: all weights are >= 0, so
  this bounds the difference of any two summation orders; and bit-identical from call to call and for every chunking.
Every comparison prints its figure before it asserts.

Inputs: (A) a 40 x 52 cut of the benchmark texture, N_j > N_i, so the column-clamp quirk leaves empty windows (NaN speeds and
NaN means); (B) 52 x 40 random 8-bit frames, every speed finite and every direction bin occupied.  Radius 60 (sigma 15) on a
40-pixel side is among the sigmas of (A).
Planes of 2080 samples are one-block launches of k_bz_angles (and at most three blocks of k_bs_moments): several blocks per pair,
the block caps, 128 direction bins, histograms past the LDS counters and more pairs than a launch holds are in
tests/test_gpu_summary_launch_shapes.py."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIELDS = ("v_x", "v_y", "speed", "net_remodelling")
SIGMAS = {"A": (0.5, 1.3, 2.48, 6.0, 15.0), "B": (0.5, 1.0, 2.48, 6.0)}
BOXES = {"A": (7, 21), "B": (7, 15)}
DXDT = dict(delta_x=0.0913, delta_t=10)
SUMMARIES = ("blursizes", "speed_means", "speed_stds", "nonfinite_counts", "speed_histograms", "histogram_edges", "angle_histograms",
             "weighted_angle_histograms", "angle_edges", "intensity_histograms", "intensity_edges", "probe_speeds")
_movies = {}


def movie_of(name):
    if not _movies:
        from oracle import vof_oracle as orc
        _movies["A"] = np.ascontiguousarray(orc.make_texture_stack(64, 3, seed=0)[:, :40, :52])
        _movies["B"] = np.random.default_rng(44).integers(0, 256, (3, 52, 40)).astype(np.uint8)
        for m in _movies.values():
            m.setflags(write=False)
    return _movies[name]


def as_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def call(movie, sigmas, box, entry="host", **kw):
    from opticalflow_amd import optical_flow as of
    if entry == "torch":
        import torch
        return of.vary_blursize(torch.as_tensor(movie).cuda(), sigmas, box, output="torch", **DXDT, **kw)
    return of.vary_blursize(movie, sigmas, box, **DXDT, **kw)


def stat_kw(movie, speed_hi):
    n_i, n_j = movie.shape[1:]
    return dict(histogram_bins=50, histogram_range=(0.0, speed_hi), angle_bins=50, intensity_bins=50,
                intensity_range=(float(movie.min()), float(movie.max())),
                probe_locations=[(0, 0), (5, 7), (n_i - 1, n_j - 1), (n_i - 1, 0)])


def same(a, b, keys):
    return [k for k in keys if not np.array_equal(as_numpy(a[k]), as_numpy(b[k]), equal_nan=True)]


# ---- 1. the tiled blur ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 52), (52, 40), (70, 131)])
def test_tiled_blur_has_the_bits_of_k_blur1d(shape, monkeypatch):
    """Radii 2, 10, 24, 60 (>= the side of the two small shapes), 64 (the last tiled one) and 65 (the first one left to
    k_blur1d); (70, 131) is more than one tile along both axes and no multiple of the 32 / 16 rows or 64 columns of a tile.
    blur_movie and the device entry with the tiled kernel against blur_movie with the switch off, and the sweep's own blurred
    stack through its intensity histogram."""
    import torch
    from opticalflow_amd import optical_flow as of, _native
    movie = np.random.default_rng(3).random((3,) + shape) * 255.0
    sigmas = (0.5, 2.48, 6.0, 15.0, 16.0, 16.2)
    assert [of.gaussian_taps(s).size // 2 for s in sigmas] == [2, 10, 24, 60, 64, 65]
    monkeypatch.setenv("VOF_BLUR_TILED", "0")
    old = [of.blur_movie(movie, s) for s in sigmas]
    old_sweep = call(movie, sigmas, 5, intensity_bins=64, intensity_range=(0.0, 255.0))
    monkeypatch.delenv("VOF_BLUR_TILED")
    dev_in = torch.as_tensor(movie).cuda()
    dev_out = torch.empty_like(dev_in)
    torch.cuda.synchronize()                                         # the library launches on its own stream
    with _native.Solver(shape[0], shape[1], 1) as solver:
        for s, ref in zip(sigmas, old):
            assert np.isfinite(ref).all()
            assert np.array_equal(of.blur_movie(movie, s), ref), (shape, s)
            solver.blur_dev(dev_in, dev_out, 3, of.gaussian_taps(s))
            assert np.array_equal(dev_out.cpu().numpy(), ref), (shape, s, "device entry")
    new_sweep = call(movie, sigmas, 5, intensity_bins=64, intensity_range=(0.0, 255.0))
    assert np.array_equal(new_sweep["intensity_histograms"], old_sweep["intensity_histograms"])
    for i, ref in enumerate(old):
        assert np.array_equal(new_sweep["intensity_histograms"][i], np.histogram(ref.ravel(), 64, (0.0, 255.0))[0]), (shape, sigmas[i])
    assert np.array_equal(new_sweep["speed_means"], old_sweep["speed_means"], equal_nan=True)


# ---- 2. per sigma the fields of conduct_optical_flow ------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "torch"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_fields_equal_conduct_optical_flow(name, entry):
    from opticalflow_amd import optical_flow as of
    movie, sigmas = movie_of(name), SIGMAS[name]
    runs = [(box, rem, quirks, None) for box in BOXES[name] for rem in (False, True) for quirks in (True, False)]
    runs.append((BOXES[name][0], True, True, float(np.median(movie))))          # one run with background
    runs.append((33, name == "B", True, None))                                  # past the fused kernel: the general path
    for box, rem, quirks, background in runs:
        kw = dict(include_remodelling=rem, reference_quirks=quirks, background=background)
        res = call(movie, sigmas, box, entry, return_fields=True, **kw)
        assert np.array_equal(res["blursizes"], sigmas)
        assert ("net_remodelling" in res) == rem
        for i, s in enumerate(sigmas):
            arg = movie
            if entry == "torch":
                import torch
                arg = torch.as_tensor(movie).cuda()
            one = of.conduct_optical_flow(arg, box, smoothing_sigma=s, output="torch" if entry == "torch" else "numpy", **DXDT, **kw)
            for k in FIELDS[:4 if rem else 3]:
                got = res[k][i]
                assert entry == "host" or (got.is_cuda and str(got.dtype) == "torch.float64")
                assert np.array_equal(as_numpy(got), as_numpy(one[k]), equal_nan=True), (name, entry, box, rem, quirks, background, s, k)


# ---- 3. independence of the list and of the chunking ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_a_sigma_does_not_depend_on_the_list_or_the_chunks(name):
    from opticalflow_amd import optical_flow as of, _native
    movie, sigmas, box = movie_of(name), SIGMAS[name], BOXES[name][1]
    rem, quirks = name == "B", name == "A"                           # (A): NaN speeds of the quirk; (B): net_remodelling and a filled speed
    kw = dict(stat_kw(movie, 0.05), include_remodelling=rem, reference_quirks=quirks, return_fields=True)
    keys = [k for k in FIELDS[:4 if rem else 3] + SUMMARIES[1:] + (("remodelling_means", "remodelling_stds") if rem else ())
            if not k.endswith("_edges")]
    full = call(movie, sigmas, box, **kw)
    order = (3, 0, 0, 2)                                             # another order, a duplicate, entries left out
    part = call(movie, [sigmas[i] for i in order], box, **kw)
    for at, i in enumerate(order):
        for k in keys:
            assert np.array_equal(part[k][at], full[k][i], equal_nan=True), (name, k, sigmas[i])
    alone = call(movie, sigmas[-1:], box, **kw)
    assert not [k for k in keys if not np.array_equal(alone[k][0], full[k][-1], equal_nan=True)]
    # one pair slot (two chunks of one pair) against a context that holds both pairs
    args = (movie, [of.gaussian_taps(s) for s in sigmas], box, 0.0913, 10, rem, quirks, full["histogram_edges"], 50,
            full["intensity_edges"], kw["probe_locations"], True)
    got = []
    for slots in (1, 2):
        with _native.Solver(movie.shape[1], movie.shape[2], slots) as solver:
            got.append(solver.vary_blursize_host(*args))
    for a, b in zip(got[0][:6], got[1][:6]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got[0][6][:4 if rem else 3], got[1][6][:4 if rem else 3]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(got[1][3], full["weighted_angle_histograms"]) and np.array_equal(got[1][2], full["angle_histograms"])
    assert np.array_equal(got[0][6][2], full["speed"], equal_nan=True)
    assert (got[0][2].sum(axis=1) > 0).all()


# ---- 4. statistics -----------------------------------------------------------------------------------------------------
def direction(v_x, v_y, speed):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.arccos(v_y / speed) * np.sign(v_x) / np.pi


@pytest.mark.parametrize("entry", ["host", "torch"])
@pytest.mark.parametrize("name,box", [("A", 7), ("A", 21), ("B", 7), ("B", 15)])
def test_statistics(name, box, entry):
    from opticalflow_amd import optical_flow as of
    movie, sigmas = movie_of(name), SIGMAS[name]
    fields = call(movie, sigmas, box, entry, return_fields=True)
    v_x, v_y, speed = (as_numpy(fields[k]) for k in FIELDS[:3])
    finite = speed[np.isfinite(speed)]
    kw = stat_kw(movie, float(finite.max()))
    full = call(movie, sigmas, box, entry, return_fields=True, **kw)
    stats_only = call(movie, sigmas, box, entry, **kw)
    again = call(movie, sigmas, box, entry, **kw)
    assert sorted(set(full) - set(stats_only)) == ["speed", "v_x", "v_y"]
    assert sorted(stats_only) == sorted(SUMMARIES + ("delta_x", "delta_t"))
    assert not same(full, stats_only, SUMMARIES) and not same(again, stats_only, SUMMARIES)       # with / without fields; twice
    assert np.array_equal(as_numpy(full["speed"]), speed, equal_nan=True)
    n, P = len(sigmas), movie.shape[0] - 1
    for k in ("speed_histograms", "angle_histograms", "intensity_histograms"):
        assert stats_only[k].dtype == np.int64 and stats_only[k].shape == (n, 50), k
    assert stats_only["weighted_angle_histograms"].dtype == np.float64 and stats_only["weighted_angle_histograms"].shape == (n, 50)
    assert np.array_equal(stats_only["histogram_edges"], np.linspace(*kw["histogram_range"], 51))
    assert np.array_equal(stats_only["angle_edges"], np.linspace(-1.0, 1.0, 51))
    assert np.array_equal(stats_only["intensity_edges"], np.linspace(*kw["intensity_range"], 51))
    assert stats_only["probe_speeds"].shape == (n, P, 4)
    interior = stats_only["angle_edges"][1:-1]
    for i, s in enumerate(sigmas):
        assert np.array_equal(stats_only["speed_histograms"][i], np.histogram(speed[i].ravel(), 50, kw["histogram_range"])[0]), s
        blurred = of.conduct_optical_flow(movie, box, smoothing_sigma=s, **DXDT)["blurred_data"]
        assert np.array_equal(stats_only["intensity_histograms"][i], np.histogram(blurred.ravel(), 50, kw["intensity_range"])[0]), s
        # directions: np.histogram drops NaN only with a range; a non-finite speed counts nowhere
        ok = np.isfinite(speed[i])
        a, w = direction(v_x[i][ok], v_y[i][ok], speed[i][ok]), speed[i][ok]
        a, w = a[~np.isnan(a)], w[~np.isnan(a)]
        gap = np.abs(a[:, None] - interior[None, :])
        gap = gap[gap > 0]
        print(f"{name} box {box} sigma {s}: {a.size} directions, smallest distance to an interior edge {gap.min():.3e}")
        assert gap.min() > 1e-9, "a direction within 1e-9 of an edge: the exact comparison would not be meaningful"
        counts = np.histogram(a, 50, (-1, 1))[0]
        sums = np.histogram(a, 50, (-1, 1), weights=w)[0]
        assert np.array_equal(stats_only["angle_histograms"][i], counts), s
        err = np.abs(stats_only["weighted_angle_histograms"][i] - sums)
        bound = speed[i].size * 2.0 ** -52 * sums
        print(f"    weighted sums: largest |gpu - numpy| / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
        assert (err <= bound).all(), s
        with np.errstate(invalid="ignore"):
            m, sd = np.mean(speed[i]), np.std(speed[i])
        print(f"    mean {full['speed_means'][i]} / {m}, std {full['speed_stds'][i]} / {sd}")
        np.testing.assert_allclose(full["speed_means"][i], m, rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(full["speed_stds"][i], sd, rtol=1e-12, atol=0, equal_nan=True)
        assert full["nonfinite_counts"][i] == (~np.isfinite(speed[i])).sum()
        for l, (pi, pj) in enumerate(kw["probe_locations"]):
            assert np.array_equal(full["probe_speeds"][i, :, l], speed[i, :, pi, pj], equal_nan=True)
    if name == "A":          # the column-clamp quirk leaves columns with empty windows
        assert np.isnan(full["speed_means"]).all() and (full["nonfinite_counts"] > 0).all()
        h = box // 2                                   # the columns j >= N_i + h of the two pairs
        assert (full["nonfinite_counts"] == 2 * 40 * (52 - 40 - h)).all()
    else:
        assert np.isfinite(full["speed_means"]).all() and (full["nonfinite_counts"] == 0).all()
        assert (full["angle_histograms"] > 0).all()


def test_remodelling_statistics():
    """net_remodelling's mean and standard deviation (reference_quirks=False, where speed is filled as well)."""
    movie, sigmas = movie_of("B"), SIGMAS["B"]
    kw = dict(include_remodelling=True, reference_quirks=False)
    full = call(movie, sigmas, 7, return_fields=True, **kw)
    stats_only = call(movie, sigmas, 7, **kw)
    keys = ("speed_means", "speed_stds", "remodelling_means", "remodelling_stds", "nonfinite_counts")
    assert not same(full, stats_only, keys)
    for i in range(len(sigmas)):
        for what, field in (("speed", "speed"), ("remodelling", "net_remodelling")):
            print(f"sigma {sigmas[i]} {what}: {full[what + '_means'][i]} / {np.mean(full[field][i])}")
            np.testing.assert_allclose(full[what + "_means"][i], np.mean(full[field][i]), rtol=1e-12, atol=0)
            np.testing.assert_allclose(full[what + "_stds"][i], np.std(full[field][i]), rtol=1e-12, atol=0)


# ---- 5. the wrapper ------------------------------------------------------------------------------------------------------
def test_filename_round_trip_and_torch_output(tmp_path):
    import torch
    movie, sigmas = movie_of("A"), SIGMAS["A"]
    kw = dict(stat_kw(movie, 0.05), include_remodelling=True, return_fields=True, background=float(np.median(movie)))
    path = str(tmp_path / "blur_sweep.npy")
    host = call(movie, sigmas, 7, filename=path, **kw)
    loaded = np.load(path, allow_pickle=True).item()
    assert sorted(loaded) == sorted(host)
    for k in host:
        assert np.array_equal(loaded[k], host[k], equal_nan=True), k
    dev = call(movie, sigmas, 7, "torch", **kw)
    assert sorted(dev) == sorted(host)
    for k in host:
        if k in FIELDS:
            assert dev[k].is_cuda and dev[k].dtype == torch.float64
        else:
            assert not hasattr(dev[k], "is_cuda")
        assert np.array_equal(as_numpy(dev[k]), host[k], equal_nan=True), k


def test_argument_errors():
    from opticalflow_amd import optical_flow as of, _native
    movie = movie_of("B")
    for bad, kw in (([], {}), ([1.0, 0.0], {}), ([-2.0], {}), ([np.nan], {}), ([1.0], dict(histogram_bins=50)),
                    ([1.0], dict(intensity_bins=50)), ([1.0], dict(probe_locations=[(52, 0)])), ([1.0], dict(probe_locations=[(0, 40)])),
                    ([1.0], dict(output="cupy")), ([1.0], dict(angle_bins=0))):
        with pytest.raises(ValueError):
            of.vary_blursize(movie, bad, **kw)
    frames = np.ascontiguousarray(movie, dtype=np.float64)
    with _native.Solver(52, 40, 1) as solver:
        with pytest.raises(_native.VofError, match="empty"):
            solver.vary_blursize_host(frames, [], 7)
        with pytest.raises(_native.VofError, match="two frames"):
            solver.vary_blursize_host(frames[:1], [of.gaussian_taps(1.0)], 7)
        with pytest.raises(_native.VofError, match="box_size"):
            solver.vary_blursize_host(frames, [of.gaussian_taps(1.0)], 0)
        with pytest.raises(_native.VofError, match="angle_bins"):
            solver.vary_blursize_host(frames, [of.gaussian_taps(1.0)], 7, angle_bins=129)
        with pytest.raises(_native.VofError, match="probe outside"):
            solver.vary_blursize_host(frames, [of.gaussian_taps(1.0)], 7, probe_locations=[(52, 0)])
        stats, *_rest = solver.vary_blursize_host(frames, [of.gaussian_taps(1.0)], 7)      # the context is still good
        assert np.isfinite(stats["speed_mean"]).all() and list(stats["sigma_index"]) == [0]


# ---- 6. one statistics tail for both sweeps -----------------------------------------------------------------------------
TAIL_SEED, TAIL_SIGMA = 237, 0.1
TAIL_STATS = ("speed_mean", "speed_variance", "remodelling_mean", "remodelling_variance", "nonfinite_count")


@pytest.mark.parametrize("rem", [False, True])
def test_box_one_has_the_bits_of_the_box_size_sweep(rem):
    """vary_boxsize(movie, [1], smoothing_sigma=s) against vary_blursize(movie, [s], boxsize=1): at half width 0 the ring growth
    and the direct sums add the same terms in the same order, so fields and every shared summary agree bit for bit - through
    the wrappers (both pairs in one chunk) and through the _host entries of a one-slot context (two chunks).

    A one-pixel window makes det = dx^2 dy^2 - (dx dy)^2, which rounds to exactly 0 at about every other pixel and is 0 on the
    border lines, where the derivatives are: over the seeds 0 .. 299 tests/boxsweep_restatement.py leaves 0.477 +- 0.010 of the
    speed samples finite.  The seed is the one with the largest share, 977 of 1920 (0.509); with remodelling det is a sum of
    five such terms and 644 of 1920 (0.335) stay finite, no seed comes near a half, so that run asks for a quarter.  sigma 0.1
    has the single tap 1.0: both sweeps launch their blur, which changes no bit, so the shares counted on the CPU are those of
    the kernels (a wider blur differs from the oracle's in last bits, which redraws the zeros of det)."""
    from opticalflow_amd import optical_flow as of, _native
    from oracle import vof_oracle as orc
    movie = np.ascontiguousarray(orc.make_texture_stack(40, 3, seed=TAIL_SEED)[:, :24, :40])
    probes = [(0, 0), (5, 7), (23, 39), (23, 0), (0, 39)]
    kw = dict(DXDT, include_remodelling=rem, reference_quirks=False, histogram_bins=50, histogram_range=(0.0, 0.05),
              probe_locations=probes, return_fields=True)
    box = of.vary_boxsize(movie, [1], smoothing_sigma=TAIL_SIGMA, **kw)
    blur = of.vary_blursize(movie, [TAIL_SIGMA], boxsize=1, **kw)
    keys = FIELDS[:4 if rem else 3] + ("speed_means", "speed_stds", "nonfinite_counts", "speed_histograms", "probe_speeds")
    keys += ("remodelling_means", "remodelling_stds") if rem else ()
    share = np.isfinite(box["speed"]).mean()
    print(f"rem {rem}: {share:.4f} of the speed samples finite, {box['speed_histograms'].sum()} in the histogram's range, "
          f"differing keys {same(box, blur, keys)}")
    assert share >= (0.25 if rem else 0.5)
    assert not same(box, blur, keys)
    assert box["nonfinite_counts"][0] == (~np.isfinite(box["speed"])).sum()
    # two chunks of one pair
    frames, taps, edges = np.ascontiguousarray(movie, dtype=np.float64), of.gaussian_taps(TAIL_SIGMA), box["histogram_edges"]
    with _native.Solver(24, 40, 1) as solver:
        b_stats, b_hist, b_probes, b_fields = solver.vary_boxsize_host(frames, [1], 0.0913, 10, rem, False, taps, edges, probes, True)
        z_stats, z_hist, _, _, _, z_probes, z_fields = solver.vary_blursize_host(frames, [taps], 1, 0.0913, 10, rem, False, edges, None,
                                                                                 None, probes, True)
    for k in TAIL_STATS:
        assert b_stats[k].tobytes() == z_stats[k].tobytes(), k
    assert np.array_equal(b_hist, z_hist) and np.array_equal(b_probes, z_probes, equal_nan=True)
    for f in range(4 if rem else 3):
        assert np.array_equal(b_fields[f], z_fields[f], equal_nan=True), FIELDS[f]
        assert np.array_equal(b_fields[f], box[FIELDS[f]], equal_nan=True), FIELDS[f]
    assert np.array_equal(b_hist, box["speed_histograms"]) and np.array_equal(b_probes, box["probe_speeds"], equal_nan=True)
