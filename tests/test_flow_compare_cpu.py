"""CPU tests of the comparison of two finished flow results and of the result filter (compare_flow_results,
filter_PIV_flow_result): the boundary of the new entry points (header, library, binding, Python names and defaults), the
argument errors raised before the library is touched, and the conditions on the committed test inputs that the exact GPU
comparison of tests/test_gpu_flow_compare.py rests on."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from flow_compare_restatement import (compare_restatement, filter_inputs, filter_restatement, input_conditions, inputs_a,
                                      make_result, negated)

ENTRY_POINTS = {"vof_flow_filter": 13, "vof_flow_extremes": 13, "vof_flow_compare": 22}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = header_text()
    for stem, n_args in ENTRY_POINTS.items():
        for name in (stem + "_dev", stem + "_host"):
            decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
            assert decl, name
            assert hasattr(lib, name)
            res, args = _native.SIGNATURES[name]
            assert len(args) == len(decl.group(1).split(",")) == n_args
        assert _native.SIGNATURES[stem + "_dev"] == _native.SIGNATURES[stem + "_host"]
    for method in ("flow_filter", "flow_extremes", "flow_compare"):
        assert hasattr(_native.Solver, method)
    assert "vof_flowcompare.hpp" in build.default_deps(build.CSRC, build.SOURCES[0])
    assert lib.vof_version() == 202 and len(_native.K_NAMES) == 17      # additive: the version and the profiler classes stay


def test_limits_agree_on_every_layer():
    """The bin limits are those of compare_channel_flows on every layer, and the histogram kernel's static LDS - the 2-D
    counters, one set of theta counters per wave, six counters, the three edge vectors - stays inside the default 64 KiB of a
    workgroup."""
    from opticalflow_amd import optical_flow as of
    src = open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_flowcompare.hpp")).read()
    old = open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_compare.hpp")).read()
    old += open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_shared.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int ((?:FC|CP)_[A-Z_]+) = (\d+);", src + old)}
    assert const["CP_MAX_THETA_BINS"] == of.COMPARE_MAX_ANGLE_BINS == 64 and const["CP_MAX_SPEED_BINS"] == of.COMPARE_MAX_SPEED_BINS == 1024
    assert const["FC_BLOCK"] % 64 == 0
    edges = 2 * (const["CP_MAX_SPEED_BINS"] + 1) + const["CP_MAX_THETA_BINS"] + 1
    assert (const["CP_LDS_JOINT"] + const["FC_BLOCK"] // 64 * const["CP_MAX_THETA_BINS"] + 6) * 4 + edges * 8 <= 65536
    assert const["CP_LDS_JOINT"] >= 50 * 50
    doc = of.compare_flow_results.__doc__
    assert "1 .. 1024 per axis" in doc and "1 .. 64" in doc
    header = open(os.path.join(ROOT, "include", "vof.h")).read()
    assert "angle_bins: 1 .. 64" in header


def test_python_names_and_signatures():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    for name in ("compare_flow_results", "filter_PIV_flow_result"):
        assert getattr(shim, name) is getattr(of, name) and name in of.__all__
    p = inspect.signature(of.filter_PIV_flow_result).parameters
    assert [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD] == [
        ("flow_result", inspect.Parameter.empty), ("intensity_threshold", 10), ("speed_threshold", 7)]
    assert [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == [("device", 0), ("reference_quirks", True)]
    p = inspect.signature(of.compare_flow_results).parameters
    assert [n for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD] == ["flow_a", "flow_b"]
    assert [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == [
        ("speed_threshold", 0.1), ("angle_threshold", 0.5), ("joint_speed_bins", (50, 50)), ("joint_speed_ranges", None),
        ("angle_bins", 20), ("angle_range", None), ("ground_truth", None), ("reference_quirks", True), ("device", 0),
        ("frames_in_flight", 0)]


def small_result(seed, shape=(2, 8, 6)):
    v = np.random.default_rng(seed).normal(0, 1, (2,) + shape)
    return make_result(v[0], v[1])


def test_argument_errors_need_no_gpu(monkeypatch):
    from opticalflow_amd import optical_flow as of, _native

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load_library", no_library)
    a, b = small_result(0), small_result(1)
    points = np.array([[1, 2], [3, 4]])
    compare_cases = [
        ((a, small_result(1, (2, 8, 5))), {}, "same shape"),
        ((a, small_result(1, (3, 8, 6))), {}, "same shape"),
        ((a, dict(b, speed=b["speed"].astype(np.float32))), {}, "cast it"),
        ((dict(a, v_x=a["v_x"].astype(np.int64)), b), {}, "cast it"),
        ((a, dict(b, v_y=b["v_y"][:, :, :5])), {}, "contiguous"),
        ((a, dict(b, v_y=b["v_y"][:, :, :5].copy())), {}, "common shape"),
        ((a, dict(v_x=b["v_x"], v_y=b["v_y"])), {}, "'speed'"),
        ((a, dict(b, speed=b["speed"].tolist())), {}, "numpy array or a device tensor"),
        ((small_result(0, (2, 3, 6)), small_result(1, (2, 3, 6))), {}, "4x4"),
        ((a, b), dict(speed_threshold=np.nan), "NaN"),
        ((a, b), dict(joint_speed_bins=50), "pair"),
        ((a, b), dict(joint_speed_bins=(0, 50)), "1 .. 1024"),
        ((a, b), dict(joint_speed_bins=(50, 1025)), "1 .. 1024"),
        ((a, b), dict(angle_bins=0), "1 .. 64"),
        ((a, b), dict(angle_bins=65), "1 .. 64"),
        ((a, b), dict(angle_bins=None), "1 .. 64"),
        ((a, b), dict(joint_speed_ranges=((0, 1),)), "joint_speed_ranges"),
        ((a, b), dict(joint_speed_ranges=((0, 1), (2, 1))), "joint_speed_ranges"),
        ((a, b), dict(joint_speed_ranges=((0, 1), (0, np.inf))), "joint_speed_ranges"),
        ((a, b), dict(angle_range=(0, 1, 2)), "angle_range"),
        ((a, b), dict(angle_range=(np.pi, 0)), "angle_range"),
        ((a, b), dict(frames_in_flight=-1), "frames_in_flight"),
        ((a, b), dict(ground_truth=(0, points)), "ground_truth"),
        ((a, b), dict(ground_truth=(2, points, points)), "frame"),
        ((a, b), dict(ground_truth=(-1, points, points)), "frame"),
        ((a, b), dict(ground_truth=(0, points.astype(float), points)), "integer"),
        ((a, b), dict(ground_truth=(0, points, points[:1])), "same shape"),
        ((a, b), dict(ground_truth=(0, np.array([[8, 0]]), np.array([[1, 1]]))), "outside"),
        ((a, b), dict(ground_truth=(0, np.array([[0, 6]]), np.array([[1, 1]]))), "outside"),
        ((a, b), dict(ground_truth=(0, np.array([[-1, 0]]), np.array([[1, 1]]))), "outside"),      # no negative wrap
        ((a, b), dict(ground_truth=(0, np.array([[1, 1]]), np.array([[1, -2]]))), "outside"),
    ]
    for results, kw, match in compare_cases:
        with pytest.raises(ValueError, match=match):
            of.compare_flow_results(*results, **kw)
    movie = np.zeros((3, 8, 6), dtype=np.uint8)
    filter_cases = [
        (dict(a), {}, "original_data"),
        (dict(a, original_data=movie[:1]), {}, "2 or 3 frames"),
        (dict(a, original_data=np.zeros((3, 8, 7))), {}, "frames of 8 x 6"),
        (dict(a, original_data=movie.astype(np.complex128)), {}, "real dtype"),
        (dict(a, original_data=movie.tolist()), {}, "all numpy arrays"),
        (dict(a, original_data=movie, speed=a["speed"].astype(np.float32)), {}, "cast it"),
        (dict(a, original_data=movie), dict(intensity_threshold=np.nan), "NaN"),
    ]
    for result, kw, match in filter_cases:
        with pytest.raises(ValueError, match=match):
            of.filter_PIV_flow_result(result, **kw)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    a, b = small_result(0), small_result(1)
    with pytest.raises(_native.VofError):
        optical_flow.compare_flow_results(a, b)
    with pytest.raises(_native.VofError):
        optical_flow.filter_PIV_flow_result(dict(a, original_data=np.zeros((3, 8, 6), dtype=np.uint8)))


# ---- the committed inputs of the GPU test: what its exact comparison rests on -------------------------------------------------
@pytest.mark.parametrize("thresholds, m1, m2", [((0.1, 0.5), 6172, 4886), ((0.5, 1.0), 4886, 2565)])
def test_conditions_on_the_inputs(thresholds, m1, m2):
    a, b = inputs_a()
    found = input_conditions(a, b, *thresholds)
    print(found)
    assert (found["m1"], found["m2"]) == (m1, m2) and found["m1"] < a["speed"].size == 6240
    assert found["above_one"] == 0 and found["angle_bins_occupied"] == 20


def test_restatement_counts_and_shapes():
    a, b = inputs_a()
    s = compare_restatement(a, b)
    assert list(s["nan_speed_counts"]) == [5, 0] and s["infinite_count"] == 1
    assert 0 < s["angle_count"] < s["joint_count"] < a["speed"].size
    assert s["angle_histogram"].sum() == s["angle_count"] and s["angle_dropped"] == 0
    assert s["joint_speed_histogram"].shape == (50, 50) and s["joint_speed_histogram"].sum() == s["joint_count"]
    assert s["speed_extremes"].shape == (2, 2) and s["cos_extremes"].shape == (2,)
    assert np.array_equal(s["angle_edges"], np.histogram_bin_edges(np.arccos(s["cos_extremes"][::-1]), 20))
    explicit = compare_restatement(a, b, joint_speed_ranges=((0, 2), (0, 2)), angle_range=(0, np.pi))
    assert explicit["joint_speed_histogram"].sum() < explicit["joint_count"] == s["joint_count"]          # samples outside are dropped
    assert np.isnan(explicit["speed_extremes"]).all() and np.isnan(explicit["cos_extremes"]).all()
    opposite = compare_restatement(a, negated(a), angle_range=(0, np.pi))
    assert opposite["angle_histogram"][-1] == opposite["angle_count"] > 0
    same = compare_restatement(a, a, angle_range=(0, np.pi))
    assert same["angle_histogram"][0] == same["angle_count"] and same["angle_dropped"] > 0                # cos rounds above 1
    assert compare_restatement(a, a, angle_range=(0, np.pi), reference_quirks=False)["angle_dropped"] == 0


def test_restatement_of_the_filter():
    result = filter_inputs()
    blurred = np.full(result["original_data"].shape, 20.0)
    blurred[0, :, :10] = 5.0
    blurred[-1] = 0.0                                          # the last frame takes no part
    v_x, v_y, speed, low, fast = filter_restatement(result, blurred)
    assert low.sum() == 400 and 0 < fast.sum() < speed.size
    assert (v_x[low | fast] == 0).all() and (v_y[low | fast] == 0).all() and (speed[fast] == 0).all()
    keep = ~(low | fast)
    assert np.array_equal(v_x[keep], result["v_x"][keep]) and np.array_equal(speed[~fast], result["speed"][~fast], equal_nan=True)
    assert np.isnan(speed[0, 1, 2]) and speed[2, 30, 40] == 0.0 and v_x[2, 30, 40] == 0.0                # NaN kept, +inf is fast
    again = filter_restatement(result, blurred, speed_threshold=3)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(again, (v_x, v_y, speed, low, fast)))
    plain = filter_restatement(result, blurred, speed_threshold=3, reference_quirks=False)
    assert plain[4].sum() > fast.sum() and (plain[2][low] == 0).all() and not (speed[low] == 0).all()
