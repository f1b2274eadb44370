"""GPU tests of the two-channel comparison (compare_channel_flows / vof_compare_flows_*).

Bounds, none of them taken from what the GPU gives:
* fields of a channel: bit-identical to conduct_optical_flow of this checkout with the channel's arguments, the same kernels run;
* every integer summary: exact against tests/compare_restatement.py on the returned fields.  acos on the device and np.arccos
  may differ in their last bits, so the comparison first asserts that no numpy theta and no numpy direction lies within 1e-9 of
  an interior edge unless it is exactly on it (the restatement of the box flow gave 2.3e-6 as the smallest distance for (B)).
  That is an assertion on the inputs, never a reason to leave a sample or a case out;
* means / standard deviations: rtol 1e-12 against numpy (the tolerance of tests/test_gpu_blursweep.py for the same reduction);
* weighted sums: |gpu - numpy| <= N * 2**-52 * bin_sum with N the number of samples: all weights are >= 0, so this bounds the
  difference of any two summation orders; the density is the host formula on the returned sums, exactly;
* bit-identical summaries from call to call, with and without the fields, and for 1 and 2 pairs in flight.
Every comparison prints its figure before it asserts.

delta_x = 0.0913, delta_t = 10 throughout.  A plane has 2080 samples: two blocks of the joint kernel per pair, the lanes of
which do not all hold the same number of samples, and N_j != N_i.  Inputs:
(A) 40 x 52 cuts of the benchmark texture, seeds 0 and 1: N_j > N_i, so the column-clamp quirk leaves NaN speeds;
(B) 52 x 40 random 8-bit frames of default_rng(44) and default_rng(45): every theta bin occupied at boxes 7 and 15;
(C) the first movie of (B) as both channels: cos is 1 up to rounding, the excess over 1 is what the quirk drops;
(D) the first two frames of (B)'s first movie against the same two in reverse order: v_b = -v_a exactly on integer frames.
With two blocks of k_cp_joint and one of k_bz_angles per pair these are the smallest launches: 21 and 255 blocks, the cap of 256,
64 angle bins, 64 x 64 and 64 x 65 joint counters and more pairs than a launch holds are in tests/test_gpu_summary_launch_shapes.py."""

import numpy as np
import pytest

from compare_restatement import compare_summaries, direction, relative_angle

pytestmark = pytest.mark.gpu
FIELDS = ("v_x", "v_y", "speed", "net_remodelling")
DXDT = dict(delta_x=0.0913, delta_t=10)
INT_KEYS = ("speed_histograms", "angle_histograms", "relative_angle_histogram", "joint_speed_histogram", "nonfinite_counts",
            "joint_nonfinite_count", "relative_angle_dropped")
SUMMARIES = INT_KEYS + ("speed_means", "speed_stds", "weighted_angle_histograms", "weighted_relative_angle_histogram",
                        "weighted_relative_angle_density", "histogram_edges", "angle_edges", "relative_angle_edges",
                        "joint_speed_edges_a", "joint_speed_edges_b")
_movies = {}


def movies_of(name):
    if not _movies:
        from oracle import vof_oracle as orc
        b1 = np.random.default_rng(44).integers(0, 256, (3, 52, 40)).astype(np.uint8)
        b2 = np.random.default_rng(45).integers(0, 256, (3, 52, 40)).astype(np.uint8)
        _movies["A"] = tuple(np.ascontiguousarray(orc.make_texture_stack(64, 3, seed=s)[:, :40, :52]) for s in (0, 1))
        _movies["B"] = (b1, b2)
        _movies["C"] = (b1, b1)
        _movies["D"] = (np.ascontiguousarray(b1[:2]), np.ascontiguousarray(b1[:2][::-1]))
        for pair in _movies.values():
            for m in pair:
                m.setflags(write=False)
    return _movies[name]


def as_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def call(movies, box, entry="host", **kw):
    from opticalflow_amd import optical_flow as of
    if entry == "torch":
        import torch
        return of.compare_channel_flows(torch.as_tensor(movies[0]).cuda(), torch.as_tensor(movies[1]).cuda(), box, output="torch",
                                        **DXDT, **kw)
    return of.compare_channel_flows(movies[0], movies[1], box, **DXDT, **kw)


def same(a, b, keys):
    return [k for k in keys if not np.array_equal(as_numpy(a[k]), as_numpy(b[k]), equal_nan=True)]


def channel_fields(res):
    return [{k: as_numpy(res[ch][k]) for k in FIELDS[:3]} for ch in "ab"]


def stat_kw(flows):
    """Bin arguments from the fields: the script's 50 / 50 / 50 x 50 bins, ranges up to the largest finite speed, and a threshold
    on speed_b that keeps some samples of the 2-D histogram but not all (the median of the finite speeds of b)."""
    finite = [f["speed"][np.isfinite(f["speed"])] for f in flows]
    hi = [float(x.max()) for x in finite]
    return dict(histogram_bins=50, histogram_range=(0.0, max(hi)), angle_bins=50, relative_angle_bins=50, joint_speed_bins=(50, 50),
                joint_speed_ranges=((0.0, hi[0]), (0.0, hi[1])), joint_speed_min_b=float(np.median(finite[1])))


# ---- 1. per channel the fields of conduct_optical_flow --------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "torch"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_fields_equal_conduct_optical_flow(name, entry):
    from opticalflow_amd import optical_flow as of
    movies = movies_of(name)
    runs = [dict(boxsize=box, reference_quirks=quirks) for box in (7, 15, 33) for quirks in (True, False)]      # 33: the general path
    runs.append(dict(boxsize=7, include_remodelling=True, reference_quirks=False))
    runs.append(dict(boxsize=15, smoothing_sigma=(1.0, 1.3), background=(float(np.median(movies[0])), float(np.median(movies[1])))))
    runs.append(dict(boxsize=7, smoothing_sigma=2.0, background=float(np.median(movies[0]))))                   # scalars: both channels
    for run in runs:
        kw = dict(run)
        box = kw.pop("boxsize")
        res = call(movies, box, entry, return_fields=True, histogram_bins=None, **kw)
        rem = kw.get("include_remodelling", False)
        for ch, key in enumerate("ab"):
            one_kw = dict(kw)
            for arg in ("smoothing_sigma", "background"):
                if isinstance(one_kw.get(arg), tuple):
                    one_kw[arg] = one_kw[arg][ch]
            arg = movies[ch]
            if entry == "torch":
                import torch
                arg = torch.as_tensor(arg).cuda()
            one = of.conduct_optical_flow(arg, box, output="torch" if entry == "torch" else "numpy", **DXDT, **one_kw)
            assert sorted(res[key]) == sorted(one), (run, key)
            assert ("net_remodelling" in res[key]) == rem
            for k in FIELDS[:4 if rem else 3] + ("blurred_data",):
                got = res[key][k]
                assert entry == "host" or k == "blurred_data" or (got.is_cuda and str(got.dtype) == "torch.float64")
                assert np.array_equal(as_numpy(got), as_numpy(one[k]), equal_nan=True), (name, entry, run, key, k)
            assert res[key]["delta_x"] == 0.0913 and res[key]["delta_t"] == 10


# ---- 2. 3. the statistics against the restatement on the returned fields ------------------------------------------------------
def check_gap(what, values, edges):
    interior = edges[1:-1]
    gap = np.abs(values[:, None] - interior[None, :])
    gap = gap[gap > 0]
    print(f"    {what}: {values.size} values, smallest distance to an interior edge {gap.min():.3e}")
    assert gap.min() > 1e-9, f"a {what} within 1e-9 of an edge: the exact comparison would not be meaningful"


@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("name,box,entry", [("A", 7, "host"), ("A", 15, "host"), ("B", 7, "host"), ("B", 15, "host"), ("B", 7, "torch"),
                                            ("C", 7, "host"), ("C", 15, "host"), ("D", 7, "host"), ("D", 15, "host")])
def test_statistics(name, box, entry, quirks):
    movies = movies_of(name)
    flows = channel_fields(call(movies, box, entry, return_fields=True, histogram_bins=None, reference_quirks=quirks))
    kw = stat_kw(flows)
    full = call(movies, box, entry, return_fields=True, reference_quirks=quirks, **kw)
    stats_only = call(movies, box, entry, reference_quirks=quirks, **kw)
    again = call(movies, box, entry, reference_quirks=quirks, **kw)
    assert sorted(set(full) - set(stats_only)) == ["a", "b"]
    assert sorted(stats_only) == sorted(SUMMARIES + ("delta_x", "delta_t"))
    assert not same(full, stats_only, SUMMARIES) and not same(again, stats_only, SUMMARIES)      # with / without fields; twice
    assert not [k for k in SUMMARIES if as_numpy(again[k]).tobytes() != as_numpy(stats_only[k]).tobytes()]
    for ch, f in enumerate(channel_fields(full)):
        for k in FIELDS[:3]:
            assert np.array_equal(f[k], flows[ch][k], equal_nan=True)
    want = compare_summaries(flows[0], flows[1], reference_quirks=quirks, **kw)
    n_samples = flows[0]["speed"].size
    print(f"{name} box {box} quirks {quirks}: {n_samples} samples, non-finite {want['nonfinite_counts']}, jointly "
          f"{want['joint_nonfinite_count']}, theta dropped {want['relative_angle_dropped']}")

    # the inputs: nothing so close to an edge that the last bits of acos could decide the bin
    both = np.isfinite(flows[0]["speed"]) & np.isfinite(flows[1]["speed"])
    theta, _w = relative_angle(flows[0], flows[1], quirks)
    theta = theta[both]
    check_gap("theta", theta[~np.isnan(theta)], want["relative_angle_edges"])
    for ch, f in enumerate(flows):
        a = direction(f)[np.isfinite(f["speed"])]
        check_gap("direction of " + "ab"[ch], a[~np.isnan(a)], want["angle_edges"])

    # counts
    for k in INT_KEYS:
        got = stats_only[k]
        assert isinstance(got, int) or got.dtype == np.int64, k
        differ = int(np.sum(np.asarray(got) != np.asarray(want[k])))
        print(f"    {k}: {differ} entries differ, total {np.sum(got)}")
        assert np.array_equal(got, want[k]), k
    for k in ("histogram_edges", "angle_edges", "relative_angle_edges", "joint_speed_edges_a", "joint_speed_edges_b"):
        assert np.array_equal(stats_only[k], want[k]), k
    assert stats_only["speed_histograms"].shape == (2, 50) and stats_only["joint_speed_histogram"].shape == (50, 50)
    everyone = compare_summaries(flows[0], flows[1], reference_quirks=quirks, **dict(kw, joint_speed_min_b=None))["joint_speed_histogram"]
    print(f"    2-D histogram: {stats_only['joint_speed_histogram'].sum()} of {everyone.sum()} samples above joint_speed_min_b")
    assert 0 < stats_only["joint_speed_histogram"].sum() < everyone.sum()
    no_min = call(movies, box, entry, reference_quirks=quirks, **dict(kw, joint_speed_min_b=None))
    assert np.array_equal(no_min["joint_speed_histogram"], everyone)
    assert not same(no_min, stats_only, [k for k in SUMMARIES if k != "joint_speed_histogram"])

    # weighted sums, moments, density
    for k in ("weighted_angle_histograms", "weighted_relative_angle_histogram"):
        got = stats_only[k]
        assert got.dtype == np.float64 and got.shape == want[k].shape
        err, bound = np.abs(got - want[k]), n_samples * 2.0 ** -52 * want[k]
        print(f"    {k}: largest |gpu - numpy| / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
        assert (err <= bound).all(), k
    print(f"    means {stats_only['speed_means']} / {want['speed_means']}, stds {stats_only['speed_stds']} / {want['speed_stds']}")
    np.testing.assert_allclose(stats_only["speed_means"], want["speed_means"], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(stats_only["speed_stds"], want["speed_stds"], rtol=1e-12, atol=0, equal_nan=True)
    sums, edges = stats_only["weighted_relative_angle_histogram"], stats_only["relative_angle_edges"]
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(stats_only["weighted_relative_angle_density"], sums / np.diff(edges) / sums.sum(), equal_nan=True)

    # what the inputs are there for
    hist, dropped, finite = stats_only["relative_angle_histogram"], stats_only["relative_angle_dropped"], int(both.sum())
    assert hist.sum() + dropped == finite and finite + stats_only["joint_nonfinite_count"] == n_samples
    if name == "A" and quirks:       # the column-clamp quirk leaves the columns j >= N_i + h of the two pairs with empty windows
        assert list(stats_only["nonfinite_counts"]) == [2 * 40 * (52 - 40 - box // 2)] * 2
        assert stats_only["joint_nonfinite_count"] == 2 * 40 * (52 - 40 - box // 2)
        assert np.isnan(stats_only["speed_means"]).all()
    if name in "BCD":
        assert list(stats_only["nonfinite_counts"]) == [0, 0] and np.isfinite(stats_only["speed_means"]).all()
    if name == "B":
        assert (hist > 0).all() and (stats_only["angle_histograms"] > 0).all()
    if name == "C":                  # the same field twice: cos is 1 up to rounding
        assert hist[0] + dropped == finite
        assert dropped > 0 if quirks else dropped == 0
    if name == "D":                  # v_b = -v_a: cos is -1 up to rounding
        assert np.array_equal(flows[1]["v_x"], -flows[0]["v_x"]) and np.array_equal(flows[1]["v_y"], -flows[0]["v_y"])
        assert hist[-1] + dropped == finite
        if not quirks:
            assert hist[-1] == finite and dropped == 0


# ---- 4. determinism and chunking ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_summaries_do_not_depend_on_the_pairs_in_flight(name):
    from opticalflow_amd import optical_flow as of, _native
    movies = movies_of(name)
    flows = channel_fields(call(movies, 15, return_fields=True, histogram_bins=None, smoothing_sigma=(1.0, 1.3)))
    kw = stat_kw(flows)
    wrapped = call(movies, 15, smoothing_sigma=(1.0, 1.3), **kw)
    args = (np.ascontiguousarray(movies[0], dtype=np.float64), np.ascontiguousarray(movies[1], dtype=np.float64), 15, 0.0913, 10, False,
            True, of.gaussian_taps(1.0), of.gaussian_taps(1.3), wrapped["histogram_edges"], 50, 50,
            (wrapped["joint_speed_edges_a"], wrapped["joint_speed_edges_b"]), kw["joint_speed_min_b"], True)
    got = []
    for slots in (1, 2, 1):                       # two chunks of one pair, one chunk of two pairs, and the first again
        with _native.Solver(movies[0].shape[1], movies[0].shape[2], slots) as solver:
            got.append(solver.compare_flows_host(*args))
    for other in got[1:]:
        for a, b in zip(got[0][:8], other[:8]):
            assert a.tobytes() == b.tobytes()
        for ch in range(2):
            for a, b in zip(got[0][8][ch][:3], other[8][ch][:3]):
                assert np.array_equal(a, b, equal_nan=True)
    stats, hist, ahist, awhist, thist, twhist, jhist, jcounts, fields = got[0]
    assert np.array_equal(fields[0][2], flows[0]["speed"], equal_nan=True) and np.array_equal(fields[1][0], flows[1]["v_x"], equal_nan=True)
    assert list(stats["channel"]) == [0, 1]
    for mine, key in ((hist, "speed_histograms"), (ahist, "angle_histograms"), (awhist, "weighted_angle_histograms"),
                      (thist, "relative_angle_histogram"), (twhist, "weighted_relative_angle_histogram"), (jhist, "joint_speed_histogram"),
                      (stats["speed_mean"], "speed_means"), (stats["nonfinite_count"], "nonfinite_counts")):
        assert mine.tobytes() == wrapped[key].tobytes(), key
    assert (int(jcounts[0]), int(jcounts[1])) == (wrapped["joint_nonfinite_count"], wrapped["relative_angle_dropped"])
    assert thist.sum() > 0 and twhist.sum() > 0


# ---- 5. the wrapper --------------------------------------------------------------------------------------------------------------
def test_torch_output_allocates_no_field_stack():
    """Stats only on float64 device tensors: torch's peak allocation during the call stays below one field stack
    ((T - 1) x N_i x N_j float64) above what was allocated before it; the summaries are those of the host entry."""
    import torch
    from opticalflow_amd import optical_flow as of
    movies = movies_of("B")
    flows = channel_fields(call(movies, 7, return_fields=True, histogram_bins=None, smoothing_sigma=1.0))
    kw = dict(stat_kw(flows), smoothing_sigma=1.0)
    host = call(movies, 7, **kw)
    dev_movies = [torch.as_tensor(m).to(device="cuda", dtype=torch.float64) for m in movies]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dev = of.compare_channel_flows(dev_movies[0], dev_movies[1], 7, output="torch", **DXDT, **kw)
    peak = torch.cuda.max_memory_allocated() - before
    stack = (movies[0].shape[0] - 1) * movies[0].shape[1] * movies[0].shape[2] * 8
    print(f"torch peak above the inputs: {peak} bytes, one field stack: {stack} bytes")
    assert peak < stack
    assert sorted(dev) == sorted(host) and not same(dev, host, SUMMARIES)
    assert not any(hasattr(v, "is_cuda") for v in dev.values())


def test_filename_round_trip(tmp_path):
    movies = movies_of("A")
    path = str(tmp_path / "compare.npy")
    res = call(movies, 7, filename=path, histogram_range=(0.0, 0.05), joint_speed_bins=(8, 1024), joint_speed_ranges=((0.0, 0.05), (0.0, 0.04)),
               include_remodelling=True, reference_quirks=False)
    loaded = np.load(path, allow_pickle=True).item()
    assert sorted(loaded) == sorted(res) and "remodelling_means" in res and res["remodelling_means"].shape == (2,)
    for k in res:
        assert np.array_equal(loaded[k], res[k], equal_nan=True), k
    assert res["joint_speed_histogram"].shape == (8, 1024) and res["joint_speed_histogram"].sum() > 0        # past the LDS counters


def test_native_argument_errors():
    from opticalflow_amd import _native
    a, b = (np.ascontiguousarray(m, dtype=np.float64) for m in movies_of("B"))
    edges = np.linspace(0.0, 1.0, 11)
    with _native.Solver(52, 40, 1) as solver:
        with pytest.raises(_native.VofError, match="two frames"):
            solver.compare_flows_host(a[:1], b[:1], 7)
        with pytest.raises(_native.VofError, match="box_size"):
            solver.compare_flows_host(a, b, 0)
        with pytest.raises(_native.VofError, match="relative_angle_bins"):
            solver.compare_flows_host(a, b, 7, relative_angle_bins=65)
        with pytest.raises(_native.VofError, match="angle_bins"):
            solver.compare_flows_host(a, b, 7, angle_bins=65)
        with pytest.raises(_native.VofError, match="joint_speed_bins"):
            solver.compare_flows_host(a, b, 7, joint_speed_edges=(edges, np.linspace(0.0, 1.0, 1026)))
        with pytest.raises(_native.VofError, match="increase"):
            solver.compare_flows_host(a, b, 7, joint_speed_edges=(edges, edges[::-1].copy()))
        stats, *_rest = solver.compare_flows_host(a, b, 7)                # the context is still good
        assert np.isfinite(stats["speed_mean"]).all() and list(stats["channel"]) == [0, 1]
