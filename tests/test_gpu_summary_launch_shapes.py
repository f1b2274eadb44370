"""GPU tests of the summary kernels at the launches the library's defaults make: more than one block per pair, the block caps, and
more pairs than one launch holds (tests/summary_launch_cases.py has the shapes and why; tests/test_gpu_flow_compare.py,
test_gpu_blursweep.py, test_gpu_boxsweep.py and test_gpu_compare.py cover the one-block launches of small planes).

Bounds, the project's own and none of them taken from what the GPU gives:
* counts, histograms, extremes and edges: exact against numpy (tests/flow_compare_restatement.py, tests/compare_restatement.py,
  np.histogram on the returned fields).  acos on the device and np.arccos may differ in their last bits, so every exact comparison
  of angles first asserts on the inputs (or on the returned fields) that no numpy angle lies within 1e-9 of an interior edge
  unless exactly on it - a condition on the inputs, never a reason to leave a sample out;
* means and standard deviations: rtol 1e-12 against numpy on the returned fields;
* weighted sums: |gpu - numpy| <= N * 2**-52 * bin_sum with N the number of samples (all weights are >= 0), and bit-identical
  from call to call and for every chunking;
* vof_field_moments_dev: rel 1e-15 (mean) and rel 1e-10 (variance) against np.longdouble.
Every comparison prints its figure before it asserts."""
import functools

import numpy as np
import pytest

import summary_launch_cases as sl
from compare_restatement import compare_summaries, direction, relative_angle
from flow_compare_restatement import compare_restatement, filter_restatement, make_result, sample_values

pytestmark = pytest.mark.gpu
FIELDS = ("v_x", "v_y", "speed")
DXDT = dict(delta_x=0.0913, delta_t=10)
LATTICE_SEED = 51
MOVIE_SEED = 61


def quirks_of(name, box=7):
    """reference_quirks for a box flow at shape `name`: with the quirk the columns j >= N_i + box // 2 have empty windows and NaN
    speeds (tests/test_gpu_blursweep.py covers that); here every speed is to be finite, so that means and sums say something."""
    n_i, n_j = sl.SHAPES[name]
    return n_j <= n_i + box // 2


def as_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def on_device(result):
    import torch
    return {k: torch.as_tensor(np.array(v), device="cuda") for k, v in result.items()}


@functools.lru_cache(maxsize=None)
def lattice(name, pairs):
    a, b = sl.lattice_results((pairs,) + sl.SHAPES[name], LATTICE_SEED)
    for r in (a, b):
        for v in r.values():
            v.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def movie_of(name, frames, seed=MOVIE_SEED):
    return sl.random_movie(sl.SHAPES[name], frames, seed)


def compare(a, b, **kw):
    from opticalflow_amd import optical_flow as of
    return of.compare_flow_results(a, b, **kw)


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        differ = int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))) if g.shape == w.shape else -1
        print(f"{what} {key}: {differ} entries differ; sum {np.nansum(g)} / {np.nansum(w)}")
        assert g.shape == w.shape and g.dtype == w.dtype, key
        assert np.array_equal(g, w, equal_nan=True), key


def assert_bits(got, first, what):
    for key in sorted(first):
        same = np.asarray(got[key]).tobytes() == np.asarray(first[key]).tobytes()
        print(f"{what} {key}: {'same bits' if same else 'DIFFERENT'}")
        assert same, (what, key)


# ---- (a) compare_flow_results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirks", [True, False])
def test_flow_compare_over_more_pairs_than_a_launch(quirks):
    """MID, 17 pairs: 5 blocks per pair, a lane's unroll tail inside the plane, 16 pairs in a launch = 80 extremes records (more
    than one stride of the fold) and a second chunk of one pair.  Host arrays and device tensors, frames_in_flight 0, 1, 5, 17."""
    a, b = lattice("MID", 17)
    assert sl.fc_blocks(sl.samples(sl.MID)) * sl.PRE_MAX_FLIGHT > 64
    kw = dict(angle_bins=21, reference_quirks=quirks)
    figures, want = sl.launch_input_conditions(a, b, **kw)
    print(figures)
    assert figures["above_one"] > 0 if quirks else figures["above_one"] == 0
    first = compare(a, b, **kw)
    assert_same(first, want, "host")
    assert first["angle_dropped"] == (figures["above_one"] if quirks else 0)
    ta, tb = on_device(a), on_device(b)
    assert_same(compare(ta, tb, **kw), want, "device")
    for flight in (0, 1, 5, 17):
        assert_bits(compare(a, b, frames_in_flight=flight, **kw), first, f"host, {flight} in flight:")
        assert_bits(compare(ta, tb, frames_in_flight=flight, **kw), first, f"device, {flight} in flight:")


@pytest.mark.parametrize("name", ["FC_CAP", "FC_BELOW"])
def test_flow_compare_at_the_block_cap(name):
    """Two pairs of 1026 x 1027 (257 blocks capped at 256) and of 1023 x 1025 (255 blocks): automatic ranges, then explicit ranges
    with samples planted on the edges, in the first, a middle and the last block of the first and the last pair."""
    a, b = lattice(name, 2)
    fs = sl.samples(sl.SHAPES[name])
    assert (sl.uncapped(sl.fc_blocks, fs) > sl.FC_MAX_BLOCKS) == (name == "FC_CAP")
    figures, want = sl.launch_input_conditions(a, b)
    print(figures)
    assert_same(compare(a, b, angle_bins=21), want, "automatic")
    ta, tb = on_device(a), on_device(b)
    assert_same(compare(ta, tb, angle_bins=21), want, "automatic, device")
    # explicit ranges, edges planted
    pa, pb = sl.copy_of(a), sl.copy_of(b)
    ranges = ((0, 6), (0, 6))
    edges = [np.histogram_bin_edges(np.zeros(0), n, range=(0, 6)) for n in sl.PLANTED_BINS]
    planted = sl.plant_edges(pa, pb, *edges)
    kw = dict(joint_speed_bins=sl.PLANTED_BINS, joint_speed_ranges=ranges, angle_range=(0, np.pi), angle_bins=21)
    figures, want = sl.launch_input_conditions(pa, pb, planted=planted, **kw)
    print(len(planted), "planted;", figures)
    got = compare(pa, pb, **kw)
    assert_same(got, want, "planted")
    assert list(got["nan_speed_counts"]) == [1, 1] and got["infinite_count"] == 2
    assert got["joint_speed_histogram"].sum() < got["joint_count"]                     # the samples one ulp outside are dropped


@pytest.mark.parametrize("bins", [(64, 64), (64, 65)])
def test_flow_compare_joint_histogram_at_the_lds_boundary(bins):
    """64 x 64 = CP_LDS_JOINT counters are the last that are counted in LDS, 64 x 65 the first that go to global atomics; 63
    angle bins (64, the maximum, puts pi / 4 and pi / 2 within an ulp of an edge on lattice inputs: see the maximum below)."""
    a, b = lattice("MID", 17)
    assert (bins[0] * bins[1] <= sl.CP_LDS_JOINT) == (bins == (64, 64))
    for ranges in (None, ((0, 6), (0, 6))):
        kw = dict(joint_speed_bins=bins, angle_bins=63, joint_speed_ranges=ranges, angle_range=None if ranges is None else (0, np.pi))
        figures, want = sl.launch_input_conditions(a, b, **kw)
        print(bins, ranges, figures)
        got = compare(a, b, **kw)
        assert_same(got, want, f"{bins} {ranges}")
        assert got["joint_speed_histogram"].shape == bins and got["joint_speed_histogram"].sum() == got["joint_count"]


@pytest.mark.parametrize("quirks", [True, False])
def test_flow_compare_extremes_past_the_first_fold_stride(quirks):
    """Continuous inputs, 17 pairs at MID, automatic ranges: each of the six extremes is one planted sample whose record of
    k_fc_extremes lies past the first 64 of the 80 of the launch (on lattice inputs every block holds every extreme), so the edges
    of all three histograms hang on the fold's second stride.  angle_bins = 64, the documented maximum (on lattice inputs pi / 4 and
    pi / 2 are edges of 64 bins)."""
    a, b, records = sl.continuous_results(17)
    assert min(records) >= 64 and max(records) < sl.fc_blocks(sl.samples(sl.MID)) * sl.PRE_MAX_FLIGHT
    kw = dict(angle_bins=sl.CP_MAX_THETA_BINS, joint_speed_bins=(64, 65), reference_quirks=quirks)
    figures, want = sl.launch_input_conditions(a, b, **kw)
    print(figures)
    assert np.array_equal(want["speed_extremes"], [[np.nextafter(0.1, np.inf), 12.0], [np.nextafter(0.1, np.inf), 13.0]])
    assert np.array_equal(want["cos_extremes"], [-1.0, 1.0])
    first = compare(a, b, **kw)
    assert_same(first, want, "64 angle bins")
    for flight in (1, 5):
        assert_bits(compare(a, b, frames_in_flight=flight, **kw), first, f"{flight} in flight:")


@pytest.mark.parametrize("clamp", [0, 1])
def test_flow_compare_native_clamp_branches(clamp):
    """The native entry with an angle range narrower than the data: without clamp_angle a theta outside is dropped, with it it
    is counted in bin 0 or in the last bin - from every block of 17 pairs."""
    from opticalflow_amd import _native
    a, b = lattice("MID", 17)
    stacks = [np.array(r[k]) for r in (a, b) for k in FIELDS]
    angle_edges = np.linspace(0.5, 2.5, 22)
    edges = np.histogram_bin_edges(np.zeros(0), 50, range=(0, 6))
    figures, want = sl.launch_input_conditions(a, b, joint_speed_ranges=((0, 6), (0, 6)), angle_range=(0.5, 2.5), angle_edges=angle_edges)
    print(figures)
    assert np.array_equal(want["angle_edges"], angle_edges)
    _, _, _, theta, _, m2, _ = sample_values(a, b, 0.1, 0.5, True)
    kept = theta[m2 & ~np.isnan(theta)]
    below, above = int((kept < angle_edges[0]).sum()), int((kept > angle_edges[-1]).sum())
    expect = want["angle_histogram"].copy()
    if clamp:
        expect[0] += below
        expect[-1] += above
    with _native.Solver(sl.MID[0], sl.MID[1], 1) as solver:
        results = [solver.flow_compare(stacks, 17, 0.1, 0.5, True, edges, edges, angle_edges, bool(clamp), flight) for flight in (0, 5)]
    for joint, angles, counts in results:
        print(f"clamp {clamp}: {below} below, {above} above; histogram sum {angles.sum()} of {counts[4]}; "
              f"{int(np.sum(angles != expect))} bins differ")
        assert below > 1000 and above > 1000
        assert np.array_equal(angles, expect) and np.array_equal(joint, want["joint_speed_histogram"])
        assert angles.sum() == (counts[4] if clamp else counts[4] - below - above)
        assert counts[4] == want["angle_count"] and counts[5] == want["angle_dropped"] and counts[3] == want["joint_count"]


# ---- (b) filter_PIV_flow_result -------------------------------------------------------------------------------------------------
def filter_case(name, frames):
    from opticalflow_amd import optical_flow as of
    shape = (frames,) + sl.SHAPES[name]
    movie = np.random.default_rng(48).integers(0, 256, shape).astype(np.uint8)
    v = np.random.default_rng(49).normal(0, 4, (2,) + shape)
    result = make_result(v[0], v[1])
    result["speed"][0, 1, 2] = np.nan
    result["speed"][frames - 1, shape[1] - 3, shape[2] - 5] = np.inf
    blurred = of.blur_movie(movie, 3)
    return movie, result, blurred, float(np.median(blurred))


@pytest.mark.parametrize("name,frames,flights", [("FC_CAP", 4, (0, 1)), ("MID", 17, (0, 5))])
def test_filter_at_the_block_cap_and_over_chunks(name, frames, flights):
    """FC_CAP, 4 frames in one chunk: 2058 blocks of k_fc_mask capped at 2048, and one frame per chunk; MID, 17 frames: 16 + 1.
    Fields and both counts exact against the restatement fed with blur_movie's output."""
    from opticalflow_amd import _native
    from opticalflow_amd.optical_flow import gaussian_taps
    movie, result, blurred, threshold = filter_case(name, frames)
    n = frames * sl.samples(sl.SHAPES[name])
    assert (-(-n // (8 * sl.FC_BLOCK)) > sl.MASK_MAX_BLOCKS) == (name == "FC_CAP")
    frames64 = np.ascontiguousarray(movie, dtype=np.float64)
    for quirks in (True, False):
        want = filter_restatement(result, blurred, threshold, 7, quirks)
        low, fast = int(want[3].sum()), int(want[4].sum())
        assert 0 < low < n and 0 < fast < n
        with _native.Solver(*sl.SHAPES[name], 1) as solver:
            for flight in flights:
                fields = [np.array(result[k]) for k in FIELDS]
                counts = solver.flow_filter(frames64, gaussian_taps(3), frames, threshold, 7.0, not quirks, *fields, frames_in_flight=flight)
                differ = [int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))) for g, w in zip(fields, want[:3])]
                print(f"{name} quirks {quirks} flight {flight}: counts {list(counts)} / {[low, fast]}; differing samples {differ}")
                assert list(counts) == [low, fast]
                assert differ == [0, 0, 0]


def test_filter_on_device_tensors_at_the_block_cap():
    from opticalflow_amd import optical_flow as of
    import torch
    movie, result, blurred, threshold = filter_case("FC_CAP", 4)
    want = filter_restatement(result, blurred, threshold, 7, True)
    given = on_device(result)
    given["original_data"] = torch.as_tensor(movie, device="cuda")
    assert of.filter_PIV_flow_result(given, threshold, 7) is None
    for k, w in zip(FIELDS, want[:3]):
        g = given[k].cpu().numpy()
        print(k, int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))), "samples differ")
        assert np.array_equal(g, w, equal_nan=True), k


# ---- (c) vary_blursize ----------------------------------------------------------------------------------------------------------
def check_direction_gap(what, values, edges):
    gap = sl.edge_gap(values, edges)
    print(f"    {what}: {values.size} values, smallest distance to an interior edge {gap:.3e}")
    assert gap > sl.GAP_BOUND, f"a {what} within 1e-9 of an edge: the exact comparison would not be meaningful; choose another seed"


def check_blursweep_statistics(summaries, fields, blurred, hist_edges, angle_bins, intensity_edges, what):
    """summaries: (stats, hist, ahist, awhist, ihist) of a sweep; fields: (v_x, v_y, speed) of shape (n, P, N_i, N_j); blurred: a list
    of the blurred stacks per entry.  Everything against numpy on the returned fields."""
    stats, hist, ahist, awhist, ihist = summaries
    v_x, v_y, speed = (as_numpy(f) for f in fields[:3])
    for i in range(speed.shape[0]):
        f = dict(v_x=v_x[i], v_y=v_y[i], speed=speed[i])
        if hist_edges is not None:
            want = np.histogram(speed[i].ravel(), hist_edges)[0]
            print(f"{what} entry {i}: speed histogram of {hist.shape[1]} bins, {int(np.sum(hist[i] != want))} differ, total {hist[i].sum()}")
            assert np.array_equal(hist[i], want)
        if intensity_edges is not None:
            want = np.histogram(blurred[i].ravel(), intensity_edges)[0]
            print(f"{what} entry {i}: intensity histogram of {ihist.shape[1]} bins, {int(np.sum(ihist[i] != want))} differ, total {ihist[i].sum()}")
            assert np.array_equal(ihist[i], want) and ihist[i].sum() == blurred[i].size
        if angle_bins:
            edges = np.linspace(-1.0, 1.0, angle_bins + 1)
            ok = np.isfinite(speed[i])
            a, w = direction(f)[ok], speed[i][ok]
            a, w = a[~np.isnan(a)], w[~np.isnan(a)]
            check_direction_gap(f"{what} entry {i} direction", a, edges)
            counts = np.histogram(a, angle_bins, (-1, 1))[0]
            sums = np.histogram(a, angle_bins, (-1, 1), weights=w)[0]
            print(f"    direction counts: {int(np.sum(ahist[i] != counts))} of {angle_bins} bins differ, total {ahist[i].sum()}")
            assert np.array_equal(ahist[i], counts)
            err, bound = np.abs(awhist[i] - sums), speed[i].size * 2.0 ** -52 * sums
            print(f"    weighted sums: largest |gpu - numpy| / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
            assert (err <= bound).all()
        m, sd = np.mean(speed[i]), np.std(speed[i])
        print(f"    mean {stats['speed_mean'][i]} / {m}, std {np.sqrt(stats['speed_variance'][i])} / {sd}")
        np.testing.assert_allclose(stats["speed_mean"][i], m, rtol=1e-12, atol=0)
        np.testing.assert_allclose(np.sqrt(stats["speed_variance"][i]), sd, rtol=1e-12, atol=0)
        assert stats["nonfinite_count"][i] == (~np.isfinite(speed[i])).sum() == 0


BLUR_SIGMAS = (1.0, 2.48)


@pytest.mark.parametrize("name", ["MID", "MID_T"])
def test_blursweep_over_more_pairs_than_a_launch(name):
    """34 frames of 143 x 151 and of 151 x 143, two sigmas, box 7, 50 bins each: 10 direction blocks, 22 moment blocks and 21 to
    675 k_bs_counts blocks per launch; contexts of 1, 5 and 40 slots (33 chunks, 7 chunks, 32 + 1 pairs) and the device entry."""
    import torch
    from opticalflow_amd import optical_flow as of, _native
    movie = movie_of(name, 34)
    n_i, n_j = sl.SHAPES[name]
    quirks = quirks_of(name)
    frames = np.ascontiguousarray(movie, dtype=np.float64)
    taps = [of.gaussian_taps(s) for s in BLUR_SIGMAS]
    blurred = [of.blur_movie(movie, s) for s in BLUR_SIGMAS]
    iedges = np.linspace(0.0, 255.0, 51)
    got = {}
    with _native.Solver(n_i, n_j, 5) as solver:
        *_s, fields = solver.vary_blursize_host(frames, taps, 7, 0.0913, 10, False, quirks, None, None, None, None, True)
    hi = float(fields[2][np.isfinite(fields[2])].max())
    hedges = np.linspace(0.0, hi, 51)
    for slots in (1, 5, 40):
        with _native.Solver(n_i, n_j, slots) as solver:
            got[slots] = solver.vary_blursize_host(frames, taps, 7, 0.0913, 10, False, quirks, hedges, 50, iedges, None, False)[:5]
    dev = torch.as_tensor(frames, device="cuda")
    torch.cuda.synchronize()
    with _native.Solver(n_i, n_j, 1) as solver:
        got["dev"] = solver.vary_blursize_dev(dev, 34, taps, 7, 0.0913, 10, False, quirks, hedges, 50, iedges)[:5]
    check_blursweep_statistics(got[5], fields, blurred, hedges, 50, iedges, name)
    for key in (1, 40, "dev"):
        for label, x, y in zip(("stats", "speed", "direction", "weighted direction", "intensity"), got[key], got[5]):
            same = x.tobytes() == y.tobytes()
            print(f"{name} {key} against 5 slots, {label}: {'same bits' if same else 'DIFFERENT'}")
            assert same, (key, label)


@pytest.mark.parametrize("name", ["BZ_CAP", "BZ_BELOW"])
def test_blursweep_at_the_direction_block_cap(name):
    """Three frames of 726 x 727 (257 direction blocks capped at 256) and of 723 x 727 (256): both pairs in one launch are more
    than 1024 k_bs_counts blocks, the three blurred frames too.  9 direction bins."""
    from opticalflow_amd import optical_flow as of
    movie = movie_of(name, 3)
    fs = sl.samples(sl.SHAPES[name])
    assert (sl.uncapped(sl.direction_blocks, fs) > sl.BZ_ANGLE_MAX_BLOCKS) == (name == "BZ_CAP")
    assert sl.uncapped(sl.counts_blocks, 2 * fs) > sl.COUNTS_MAX_BLOCKS
    first = of.vary_blursize(movie, [1.0], 7, return_fields=True, reference_quirks=quirks_of(name), **DXDT)
    hi = float(first["speed"].max())
    kw = dict(reference_quirks=quirks_of(name), histogram_bins=50, histogram_range=(0.0, hi), angle_bins=9, intensity_bins=50, intensity_range=(0.0, 255.0))
    res = of.vary_blursize(movie, [1.0], 7, **DXDT, **kw)
    again = of.vary_blursize(movie, [1.0], 7, **DXDT, **kw)
    stats = dict(speed_mean=res["speed_means"], speed_variance=res["speed_stds"] ** 2, nonfinite_count=res["nonfinite_counts"])
    check_blursweep_statistics((stats, res["speed_histograms"], res["angle_histograms"], res["weighted_angle_histograms"],
                                res["intensity_histograms"]), [first[k] for k in FIELDS], [of.blur_movie(movie, 1.0)],
                               res["histogram_edges"], 9, res["intensity_edges"], name)
    assert res["weighted_angle_histograms"].tobytes() == again["weighted_angle_histograms"].tobytes()
    assert res["speed_histograms"].sum() == 2 * fs                                       # the largest speed is the last edge: counted


def test_blursweep_128_direction_bins():
    """angle_bins = 128, the documented maximum: 128 x 64 doubles of LDS per block of k_bz_angles."""
    from opticalflow_amd import optical_flow as of
    movie = movie_of("MID", 4)
    first = of.vary_blursize(movie, [1.0], 7, return_fields=True, reference_quirks=False, **DXDT)
    res = of.vary_blursize(movie, [1.0], 7, angle_bins=sl.BZ_MAX_ANGLE_BINS, reference_quirks=False, **DXDT)
    assert res["angle_histograms"].shape == (1, 128) and np.array_equal(res["angle_edges"], np.linspace(-1, 1, 129))
    stats = dict(speed_mean=res["speed_means"], speed_variance=res["speed_stds"] ** 2, nonfinite_count=res["nonfinite_counts"])
    check_blursweep_statistics((stats, None, res["angle_histograms"], res["weighted_angle_histograms"], None), [first[k] for k in FIELDS],
                               None, None, 128, None, "128 bins")
    assert (res["angle_histograms"] > 0).all()


@pytest.mark.parametrize("name,frames", [("MID", 4), ("BZ_CAP", 3)])
@pytest.mark.parametrize("bins", [1024, 1025, 1500])
def test_blursweep_histograms_past_the_lds_counters(name, frames, bins):
    """k_bs_counts with BS_LDS_BINS = 1024 bins (the last counted in LDS), 1025 and 1500 (global atomics), for the speed and for
    the intensity histogram; at BZ_CAP together with the cap of 1024 blocks."""
    from opticalflow_amd import optical_flow as of
    movie = movie_of(name, frames)
    assert (bins <= sl.BS_LDS_BINS) == (bins == 1024)
    first = of.vary_blursize(movie, [1.0], 7, return_fields=True, reference_quirks=quirks_of(name), **DXDT)
    lo, hi = float(first["speed"].min()), float(first["speed"].max())
    res = of.vary_blursize(movie, [1.0], 7, reference_quirks=quirks_of(name), histogram_bins=bins, histogram_range=(lo, hi), intensity_bins=bins, intensity_range=(0.0, 255.0), **DXDT)
    stats = dict(speed_mean=res["speed_means"], speed_variance=res["speed_stds"] ** 2, nonfinite_count=res["nonfinite_counts"])
    check_blursweep_statistics((stats, res["speed_histograms"], None, None, res["intensity_histograms"]), [first[k] for k in FIELDS],
                               [of.blur_movie(movie, 1.0)], res["histogram_edges"], 0, res["intensity_edges"], f"{name} {bins} bins")
    assert res["speed_histograms"].sum() == first["speed"].size and res["speed_histograms"][0, 0] > 0 and res["speed_histograms"][0, -1] > 0


# ---- (d) vary_boxsize -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames,bins", [("CP_CAP", 2, 50), ("MID", 34, 50), ("MID", 34, 1500)])
def test_boxsweep_statistics(name, frames, bins):
    """CP_CAP, one pair: 258 moment blocks capped at 256; MID, 33 pairs: 32 + 1 in flight on the device entry, 22 moment blocks each.
    The histogram range runs from the smallest to the largest finite speed returned: first-edge and last-edge hits are certain."""
    from opticalflow_amd import optical_flow as of
    movie = movie_of(name, frames)
    fs = sl.samples(sl.SHAPES[name])
    assert (sl.uncapped(sl.pair_moments_blocks, fs) > sl.MOMENTS_MAX_BLOCKS) == (name == "CP_CAP")
    boxes = (7, 21)
    kw = dict(DXDT, reference_quirks=quirks_of(name))
    first = of.vary_boxsize(movie, boxes, return_fields=True, **kw)
    speed = first["speed"]
    lo, hi = float(speed.min()), float(speed.max())
    results = [of.vary_boxsize(movie, boxes, histogram_bins=bins, histogram_range=(lo, hi), **kw),
               of.vary_boxsize(movie, boxes, histogram_bins=bins, histogram_range=(lo, hi), output="torch", **kw)]
    edges = np.linspace(lo, hi, bins + 1)
    for entry, res in zip(("host", "device"), results):
        hits = [0, 0]
        for i, box in enumerate(boxes):
            want = np.histogram(speed[i].ravel(), bins, (lo, hi))[0]
            m, sd = np.mean(speed[i]), np.std(speed[i])
            print(f"{name} {entry} box {box}: {int(np.sum(res['speed_histograms'][i] != want))} of {bins} bins differ; "
                  f"mean {res['speed_means'][i]} / {m}, std {res['speed_stds'][i]} / {sd}")
            assert np.array_equal(res["speed_histograms"][i], want) and want.sum() == speed[i].size
            np.testing.assert_allclose(res["speed_means"][i], m, rtol=1e-12, atol=0)
            np.testing.assert_allclose(res["speed_stds"][i], sd, rtol=1e-12, atol=0)
            assert res["nonfinite_counts"][i] == 0
            hits[0] += int((speed[i] == lo).sum())
            hits[1] += int((speed[i] == hi).sum())
        assert min(hits) >= 1 and np.array_equal(res["histogram_edges"], edges)
    for key in ("speed_means", "speed_stds", "speed_histograms"):
        assert results[0][key].tobytes() == results[1][key].tobytes(), key


# ---- (e) compare_channel_flows --------------------------------------------------------------------------------------------------
def channel_flows(res):
    return [{k: as_numpy(res[ch][k]) for k in FIELDS} for ch in "ab"]


def check_channel_summaries(got, flows, kw, what):
    quirks = kw["reference_quirks"]
    want = compare_summaries(flows[0], flows[1], **kw)
    n_samples = flows[0]["speed"].size
    both = np.isfinite(flows[0]["speed"]) & np.isfinite(flows[1]["speed"])
    theta, _w = relative_angle(flows[0], flows[1], quirks)
    theta = theta[both]
    check_direction_gap(what + " theta", theta[~np.isnan(theta)], want["relative_angle_edges"])
    if kw.get("angle_bins") is not None:
        for ch, f in enumerate(flows):
            a = direction(f)[np.isfinite(f["speed"])]
            check_direction_gap(what + " direction of " + "ab"[ch], a[~np.isnan(a)], want["angle_edges"])
    int_keys = [k for k in ("speed_histograms", "angle_histograms", "relative_angle_histogram", "joint_speed_histogram", "nonfinite_counts",
                            "joint_nonfinite_count", "relative_angle_dropped") if k in want]
    for k in int_keys:
        differ = int(np.sum(np.asarray(got[k]) != np.asarray(want[k])))
        print(f"    {what} {k}: {differ} entries differ, total {np.sum(got[k])}")
        assert np.array_equal(got[k], want[k]), k
    for k in ("weighted_angle_histograms", "weighted_relative_angle_histogram"):
        if k in want:
            err, bound = np.abs(got[k] - want[k]), n_samples * 2.0 ** -52 * want[k]
            print(f"    {what} {k}: largest |gpu - numpy| / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
            assert (err <= bound).all(), k
    print(f"    {what} means {got['speed_means']} / {want['speed_means']}, stds {got['speed_stds']} / {want['speed_stds']}")
    np.testing.assert_allclose(got["speed_means"], want["speed_means"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["speed_stds"], want["speed_stds"], rtol=1e-12, atol=0)
    return want


def channel_kw(flows, joint_bins, angle_bins, relative_bins):
    hi = [float(f["speed"].max()) for f in flows]
    return dict(histogram_bins=50, histogram_range=(0.0, max(hi)), angle_bins=angle_bins, relative_angle_bins=relative_bins,
                joint_speed_bins=joint_bins, joint_speed_ranges=((0.0, hi[0]), (0.0, hi[1])),
                joint_speed_min_b=float(np.median(flows[1]["speed"])))


def call_channels(movies, **kw):
    from opticalflow_amd import optical_flow as of
    return of.compare_channel_flows(movies[0], movies[1], 7, **DXDT, **kw)


@pytest.mark.parametrize("name", ["CP_CAP", "CP_BELOW"])
@pytest.mark.parametrize("quirks", [True, False])
def test_channel_comparison_at_the_block_cap(name, quirks):
    """One pair of 513 x 514 (257 blocks of k_cp_joint and 258 of k_bs_moments, capped at 256) and of 511 x 513 (255 and 256)."""
    movies = (movie_of(name, 2, 61), movie_of(name, 2, 62))
    fs = sl.samples(sl.SHAPES[name])
    assert (sl.uncapped(sl.cp_blocks, fs) > sl.CP_MAX_BLOCKS) == (name == "CP_CAP")
    flows = channel_flows(call_channels(movies, return_fields=True, histogram_bins=None, reference_quirks=quirks))
    kw = dict(channel_kw(flows, (50, 50), 49, 49), reference_quirks=quirks)
    got = call_channels(movies, **kw)
    want = check_channel_summaries(got, flows, kw, name)
    assert 0 < got["joint_speed_histogram"].sum() < fs
    again = call_channels(movies, **kw)
    assert again["weighted_relative_angle_histogram"].tobytes() == got["weighted_relative_angle_histogram"].tobytes()
    assert want["relative_angle_histogram"].sum() + want["relative_angle_dropped"] == fs


@pytest.mark.parametrize("name,joint_bins,angle_bins", [("MID_T", (64, 64), 64), ("MID", (64, 65), 63)])
def test_channel_comparison_over_more_pairs_than_a_launch(name, joint_bins, angle_bins):
    """34 frames of 143 x 151: 21 blocks of k_cp_joint per pair; 1, 5 and the library's 32 + 1 pairs in flight; the documented
    maxima of 64 direction and 64 relative-angle bins; the joint histogram at 4096 (LDS) and 4160 (global) counters."""
    from opticalflow_amd import optical_flow as of, _native
    movies = (movie_of(name, 34, 61), movie_of(name, 34, 62))
    quirks = quirks_of(name)                         # MID_T: cos unclipped, its excess over 1 dropped; MID: clipped
    flows = channel_flows(call_channels(movies, return_fields=True, histogram_bins=None, reference_quirks=quirks))
    kw = dict(channel_kw(flows, joint_bins, angle_bins, angle_bins), reference_quirks=quirks)
    assert (joint_bins[0] * joint_bins[1] <= sl.CP_LDS_JOINT) == (joint_bins == (64, 64))
    got = call_channels(movies, **kw)
    check_channel_summaries(got, flows, kw, f"{name} {joint_bins}")
    dev = of.compare_channel_flows(movies[0], movies[1], 7, output="torch", **DXDT, **kw)       # 32 + 1 pairs
    keys = [k for k in got if k not in ("delta_x", "delta_t")]
    for k in keys:
        assert np.asarray(dev[k]).tobytes() == np.asarray(got[k]).tobytes(), k
    args = (np.ascontiguousarray(movies[0], dtype=np.float64), np.ascontiguousarray(movies[1], dtype=np.float64), 7, 0.0913, 10, False,
            quirks, None, None, got["histogram_edges"], angle_bins, angle_bins, (got["joint_speed_edges_a"], got["joint_speed_edges_b"]),
            kw["joint_speed_min_b"], False)
    for slots in (1, 5):
        with _native.Solver(*sl.SHAPES[name], slots) as solver:
            stats, hist, ahist, awhist, thist, twhist, jhist, jcounts, _ = solver.compare_flows_host(*args)
        for mine, key in ((hist, "speed_histograms"), (ahist, "angle_histograms"), (awhist, "weighted_angle_histograms"),
                          (thist, "relative_angle_histogram"), (twhist, "weighted_relative_angle_histogram"), (jhist, "joint_speed_histogram"),
                          (stats["speed_mean"], "speed_means"), (stats["nonfinite_count"], "nonfinite_counts")):
            same = mine.tobytes() == got[key].tobytes()
            print(f"{slots} slots {key}: {'same bits' if same else 'DIFFERENT'}")
            assert same, (slots, key)
        assert (int(jcounts[0]), int(jcounts[1])) == (got["joint_nonfinite_count"], got["relative_angle_dropped"])


# ---- (f) vof_field_moments_dev --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, 3 * sl.samples(sl.BZ_CAP)])
def test_field_moments_at_one_sample_and_at_a_large_stack(n):
    import torch
    from opticalflow_amd import _native
    x = sl.moments_field(n)
    ref_mean = float(np.mean(x.astype(np.longdouble)))
    ref_var = float(np.var(x.astype(np.longdouble)))
    xd = torch.as_tensor(x, device="cuda:0")
    torch.cuda.synchronize()
    with _native.Solver(50, 61, 3) as s:
        m, v = s.field_moments_dev(xd, n)
        again = s.field_moments_dev(xd, n)
    print(f"n {n}: mean {m!r} / {ref_mean!r}, variance {v!r} / {ref_var!r}")
    assert (m, v) == again
    assert m == pytest.approx(ref_mean, rel=1e-15)
    assert v == pytest.approx(ref_var, rel=1e-10, abs=0.0)
