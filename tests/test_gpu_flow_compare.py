"""GPU tests of the comparison of two finished flow results and of the result filter (compare_flow_results /
vof_flow_extremes_* / vof_flow_compare_*, filter_PIV_flow_result / vof_flow_filter_*).

Bounds, none of them taken from what the GPU gives:
* every histogram, count, extreme and edge array: exact against tests/flow_compare_restatement.py (numpy on whole stacks).  acos
  on the device and np.arccos may differ in their last bits, so every exact comparison first asserts on the inputs alone that no
  numpy theta and no speed lies within 1e-9 of an interior edge unless exactly on it, and that np.arccos is monotone at the
  extremes (on a CPU the smallest gaps of these seeds are 1.1e-5 for theta and 3.0e-6 for the speeds).  Those are conditions on
  the inputs, never a reason to leave a sample or a case out;
* the filter: exact against the restatement fed with blur_movie's own output (the blur has its own tests);
* bit-identical summaries for host arrays and device tensors, from call to call and for 1, 2 and the library's pairs in flight.

Planes are 40 x 52 (2080 samples: one block of the kernels per pair whose lanes do not all hold the same number of samples,
N_i != N_j), P = 3: the launches hold 1, 2 or 3 pairs.  Inputs: flow_compare_restatement.inputs_a and filter_inputs.
These are one-block launches: several blocks per pair, the block caps, more than 64 extremes records, more pairs than a launch
holds and samples on the bin edges are in tests/test_gpu_summary_launch_shapes.py."""
import numpy as np
import pytest

from flow_compare_restatement import (compare_restatement, filter_inputs, filter_restatement, input_conditions, inputs_a, negated,
                                      sample_values)

pytestmark = pytest.mark.gpu
FIELDS = ("v_x", "v_y", "speed")
_cache = {}


def results():
    if "a" not in _cache:
        _cache["a"], _cache["b"] = inputs_a()
        for r in (_cache["a"], _cache["b"]):
            for key in FIELDS:
                r[key].setflags(write=False)
    return _cache["a"], _cache["b"]


def on_device(result):
    import torch
    return {k: (torch.as_tensor(np.array(v), device="cuda") if isinstance(v, np.ndarray) else v) for k, v in result.items()}


def compare(a, b, **kw):
    from opticalflow_amd import optical_flow as of
    return of.compare_flow_results(a, b, **kw)


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        print(key, g.ravel()[:6], w.ravel()[:6])
        assert g.shape == w.shape and g.dtype == w.dtype, key
        assert np.array_equal(g, w, equal_nan=True), key


@pytest.mark.parametrize("thresholds", [(0.1, 0.5), (0.5, 1.0)])
def test_automatic_ranges_match_numpy(thresholds):
    a, b = results()
    print(input_conditions(a, b, *thresholds))
    kw = dict(speed_threshold=thresholds[0], angle_threshold=thresholds[1])
    got, want = compare(a, b, **kw), compare_restatement(a, b, **kw)
    assert_same(got, want)
    assert got["joint_speed_histogram"].dtype == np.int64 and got["angle_histogram"].dtype == np.int64
    assert list(got["nan_speed_counts"]) == [5, 0] and got["infinite_count"] == 1
    assert 0 < got["angle_count"] < got["joint_count"] < a["speed"].size
    assert got["angle_histogram"].sum() == got["angle_count"]
    assert (got["angle_histogram"] > 0).all()


def test_explicit_ranges_and_large_joint_histogram():
    a, b = results()
    kw = dict(joint_speed_ranges=((0, 2), (0, 2)), angle_range=(0, np.pi))
    print(input_conditions(a, b, 0.1, 0.5, **kw))
    got, want = compare(a, b, **kw), compare_restatement(a, b, **kw)
    assert_same(got, want)
    assert got["joint_speed_histogram"].sum() < got["joint_count"]                   # samples outside the range are dropped
    assert np.isnan(got["speed_extremes"]).all() and np.isnan(got["cos_extremes"]).all()      # the first pass was skipped
    mixed = dict(joint_speed_ranges=(None, (0, 2)), angle_range=(0.5, 2.5))          # one axis automatic; angles outside dropped
    print(input_conditions(a, b, 0.1, 0.5, **mixed))
    got, want = compare(a, b, **mixed), compare_restatement(a, b, **mixed)
    assert_same(got, want)
    assert got["angle_histogram"].sum() < got["angle_count"]
    # 8 x 1024 counters do not fit the LDS: global integer atomics.  Edges of 1024 bins lie 5e-3 apart at most: the gap condition
    # is asserted for these edges too.
    large = dict(joint_speed_bins=(8, 1024))
    print(input_conditions(a, b, 0.1, 0.5, joint_speed_bins=(8, 1024)))
    got, want = compare(a, b, **large), compare_restatement(a, b, **large)
    assert_same(got, want)
    assert got["joint_speed_histogram"].shape == (8, 1024) and got["joint_speed_histogram"].sum() == got["joint_count"]


def test_identical_and_opposite_fields():
    a, _ = results()
    for quirks in (True, False):
        kw = dict(angle_range=(0, np.pi), reference_quirks=quirks)
        got, want = compare(a, a, **kw), compare_restatement(a, a, **kw)
        assert_same(got, want)
        assert got["angle_histogram"][0] == got["angle_count"] > 0                   # only bin 0 is occupied
        _, _, cos, _, _, m2, _ = sample_values(a, a, 0.1, 0.5, True)
        with np.errstate(invalid="ignore"):
            above = int((m2 & (cos > 1.0)).sum())
        print("cos > 1:", above, "dropped:", got["angle_dropped"])
        assert above > 0 and got["angle_dropped"] == (above if quirks else 0)
    kw = dict(angle_range=(0, np.pi))
    got, want = compare(a, negated(a), **kw), compare_restatement(a, negated(a), **kw)
    assert_same(got, want)
    assert got["angle_histogram"][-1] == got["angle_count"] > 0                      # only the last bin is occupied


def test_determinism_and_residency():
    import torch
    a, b = results()
    before = [x.copy() for r in (a, b) for x in (r[k] for k in FIELDS)]
    first = compare(a, b)
    assert_same(compare(a, b), first)
    for flight in (1, 2, 0):
        assert_same(compare(a, b, frames_in_flight=flight), first)
    ta, tb = on_device(a), on_device(b)
    copies = [t.clone() for r in (ta, tb) for t in (r[k] for k in FIELDS)]
    compare(ta, tb)                                                                  # the context and its scratch exist now
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = compare(ta, tb)
    peak = torch.cuda.max_memory_allocated() - base
    print("torch peak during the call:", peak, "bytes; one field stack:", a["speed"].nbytes)
    assert peak < a["speed"].nbytes
    assert_same(got, first)
    for flight in (1, 2):
        assert_same(compare(ta, tb, frames_in_flight=flight), first)
    for x, y in zip(before, [r[k] for r in (a, b) for k in FIELDS]):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(copies, [r[k] for r in (ta, tb) for k in FIELDS]):
        assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) and torch.equal(x.isnan(), y.isnan())


def test_ground_truth():
    a, b = results()
    start = np.array([[3, 7], [0, 0], [39, 51], [5, 2], [20, 30]])
    end = start + np.array([[1, 2], [2, -1], [-3, 1], [0, 4], [-2, -2]])
    end = np.clip(end, 0, [39, 51])
    got = compare(a, b, ground_truth=(1, start, end))
    want = compare_restatement(a, b, ground_truth=(1, start, end))
    assert_same(got, want)
    assert got["relative_errors"].shape == (2, 5) and np.isinf(got["relative_errors"][1, 0])      # b's v_x is infinite at (1, 3, 7)
    assert_same(compare(on_device(a), on_device(b), ground_truth=(1, start, end)), want)
    with pytest.raises(ValueError, match="outside"):
        compare(a, b, ground_truth=(1, np.array([[40, 0]]), np.array([[1, 1]])))
    with pytest.raises(ValueError, match="outside"):
        compare(a, b, ground_truth=(1, np.array([[-1, 0]]), np.array([[1, 1]])))


def filter_reference():
    if "filter" not in _cache:
        from opticalflow_amd import optical_flow as of
        result = filter_inputs()
        blurred = of.blur_movie(result["original_data"], 3)
        _cache["filter"] = (result, blurred, float(np.median(blurred[:-1])))
    result, blurred, threshold = _cache["filter"]
    return {k: v.copy() for k, v in result.items()}, blurred, threshold


@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("tensors", [False, True])
def test_filter(quirks, tensors):
    from opticalflow_amd import optical_flow as of

    def run(speed_threshold, frames):
        fresh, _, _ = filter_reference()
        fresh["original_data"] = fresh["original_data"][:frames]
        given = on_device(fresh) if tensors else fresh
        held = {k: given[k] for k in FIELDS}
        kept = {k: (v.data_ptr() if tensors else v.ctypes.data) for k, v in held.items()}
        assert of.filter_PIV_flow_result(given, threshold, speed_threshold, reference_quirks=quirks) is None
        for k in FIELDS:                                                             # in place: the same arrays, the same memory
            assert given[k] is held[k] and (held[k].data_ptr() if tensors else held[k].ctypes.data) == kept[k]
        return [held[k].cpu().numpy() if tensors else held[k] for k in FIELDS]

    result, blurred, threshold = filter_reference()
    want = filter_restatement(result, blurred, threshold, 7, quirks)
    low, fast = want[3], want[4]
    print("low:", low.sum(), "fast:", fast.sum(), "of", low.size)
    assert 0 < low.sum() < low.size and 0 < fast.sum() < fast.size
    got = run(7, 4)
    for k, g, w in zip(FIELDS, got, want):
        assert np.array_equal(g, w, equal_nan=True), k
    # a NaN speed is never fast: it is kept unless the sample is low and speed is zeroed there; +inf is fast
    assert np.isnan(got[2][0, 1, 2]) == (quirks or not low[0, 1, 2]) and got[2][2, 30, 40] == 0.0 and got[0][2, 30, 40] == 0.0
    for k, g, w in zip(FIELDS, run(7, 3), want):                                     # T - 1 frames of original_data: the same
        assert np.array_equal(g, w, equal_nan=True), k
    other = run(3, 4)
    changed = any(not np.array_equal(g, w, equal_nan=True) for g, w in zip(other, want))
    assert changed == (not quirks)                                                   # with quirks the limit is 7 whatever is said
    if not quirks:
        for k, g, w in zip(FIELDS, other, filter_restatement(result, blurred, threshold, 3, False)):
            assert np.array_equal(g, w, equal_nan=True), k


def test_native_counts_and_argument_errors():
    """The two counts of the filter, and that a refused call leaves the context usable."""
    from opticalflow_amd import _native
    from opticalflow_amd.optical_flow import gaussian_taps
    a, b = results()
    stacks = [np.array(r[k]) for r in (a, b) for k in FIELDS]
    result, blurred, threshold = filter_reference()
    want = filter_restatement(result, blurred, threshold, 7, True)
    edges = np.linspace(0.0, 4.0, 9)
    with _native.Solver(40, 52, 1) as solver:
        fields = [result[k] for k in FIELDS]
        movie = np.ascontiguousarray(result["original_data"][:3], dtype=np.float64)
        counts = solver.flow_filter(movie, gaussian_taps(3), 3, threshold, 7.0, False, *fields)
        assert list(counts) == [want[3].sum(), want[4].sum()]
        for flight in (1, 2):                                                        # more than one chunk: the same fields and counts
            again = [filter_reference()[0][k] for k in FIELDS]
            counts = solver.flow_filter(movie, gaussian_taps(3), 3, threshold, 7.0, False, *again, frames_in_flight=flight)
            assert list(counts) == [want[3].sum(), want[4].sum()]
            assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(again, want[:3]))
            import torch
            tensors = [torch.as_tensor(filter_reference()[0][k], device="cuda") for k in FIELDS]
            frames = torch.as_tensor(movie, device="cuda")
            torch.cuda.synchronize()
            counts = solver.flow_filter(frames, gaussian_taps(3), 3, threshold, 7.0, False, *tensors, frames_in_flight=flight)
            assert list(counts) == [want[3].sum(), want[4].sum()]
            assert all(np.array_equal(g.cpu().numpy(), w, equal_nan=True) for g, w in zip(tensors, want[:3]))
        good = solver.flow_compare(stacks, 3, 0.1, 0.5, True, edges, edges, np.linspace(0, np.pi, 21), False)
        refused = [
            lambda: solver.flow_compare(stacks, 0, 0.1, 0.5, True, edges, edges, edges, False),                      # n_pairs < 1
            lambda: solver.flow_compare(stacks, 3, 0.1, 0.5, True, np.linspace(0, 1, 1026), edges, edges, False),    # 1025 bins
            lambda: solver.flow_compare(stacks, 3, 0.1, 0.5, True, edges, edges, np.linspace(0, 1, 66), False),      # 65 angle bins
            lambda: solver.flow_compare(stacks, 3, 0.1, 0.5, True, edges[::-1], edges, edges, False),                # decreasing
            lambda: solver.flow_compare(stacks, 3, 0.1, 0.5, True, edges, np.zeros(9), edges, False),                # not increasing
            lambda: solver.flow_compare(stacks[:5] + [None], 3, 0.1, 0.5, True, edges, edges, edges, False),         # NULL
            lambda: solver.flow_compare(stacks, 3, np.nan, 0.5, True, edges, edges, edges, False),
            lambda: solver.flow_extremes(stacks, 0, 0.1, 0.5),
            lambda: solver.flow_extremes([None] + stacks[1:], 3, 0.1, 0.5),
            lambda: solver.flow_filter(movie, gaussian_taps(3), 0, threshold, 7.0, False, *fields),
            lambda: solver.flow_filter(movie, gaussian_taps(3), 3, np.nan, 7.0, False, *fields),
            lambda: solver.flow_filter(None, gaussian_taps(3), 3, threshold, 7.0, False, *fields),
        ]
        for call in refused:
            with pytest.raises(_native.VofError, match=r"\(-1\)"):
                call()
            again = solver.flow_compare(stacks, 3, 0.1, 0.5, True, edges, edges, np.linspace(0, np.pi, 21), False)
            assert all(np.array_equal(x, y) for x, y in zip(again, good))
