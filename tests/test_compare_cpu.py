"""CPU tests of the two-channel comparison (compare_channel_flows): the boundary of the new entry points (header, library,
binding, Python name and defaults, no CPU fallback), the argument errors, and the numpy restatement of its statistics on
hand-built fields."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

C_SIZES = {"double": 8, "int64_t": 8, "int32_t": 4}
C_DTYPES = {"double": np.float64, "int64_t": np.int64, "int32_t": np.int32}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = header_text()
    for name in ("vof_compare_flows_dev", "vof_compare_flows_host"):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        assert hasattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert len(args) == len(decl.group(1).split(",")) == 38
    assert hasattr(_native.Solver, "compare_flows_host") and hasattr(_native.Solver, "compare_flows_dev")
    assert "vof_compare.hpp" in build.default_deps(build.CSRC, build.SOURCES[0])


def test_stats_record_matches_the_header():
    from opticalflow_amd import _native
    body = re.search(r"typedef struct vof_compare_stats \{(.*?)\} vof_compare_stats;", header_text(), flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"\b(double|int64_t|int32_t)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    offset = 0
    for _name, ctype in fields:
        assert offset % C_SIZES[ctype] == 0         # naturally aligned without padding
        offset += C_SIZES[ctype]
    rec = _native.COMPARE_DTYPE
    assert rec.itemsize == offset == 48
    assert list(rec.names) == [n for n, _ in fields]
    assert [rec[n] for n in rec.names] == [np.dtype(C_DTYPES[t]) for _, t in fields]
    assert [n.replace("channel", "sigma_index") for n in rec.names] == list(_native.BLURSIZE_DTYPE.names)


def test_bin_limits_agree_on_every_layer():
    """The limits the docstring states are those of the kernel header, and the kernel's LDS at the limits stays inside the default
    64 KiB of a workgroup: (bins x 64) float64 columns, the theta counters, the 2-D counters and two static counters."""
    from opticalflow_amd import optical_flow as of
    src = open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_compare.hpp")).read()
    src += open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_shared.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (CP_[A-Z_]+) = (\d+);", src)}
    assert const["CP_MAX_THETA_BINS"] == of.COMPARE_MAX_ANGLE_BINS == 64
    assert const["CP_MAX_SPEED_BINS"] == of.COMPARE_MAX_SPEED_BINS == 1024
    assert const["CP_MAX_THETA_BINS"] * 64 * 8 + (const["CP_MAX_THETA_BINS"] + const["CP_LDS_JOINT"]) * 4 + 8 <= 65536
    assert const["CP_LDS_JOINT"] >= 50 * 50
    doc = of.compare_channel_flows.__doc__
    assert "1 .. 64" in doc and "1 .. 1024" in doc
    header = open(os.path.join(ROOT, "include", "vof.h")).read()
    assert "relative_angle_bins: 1 .. 64" in header and "1 .. 1024 bins per axis" in header


def test_python_name_and_signature():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    assert shim.compare_channel_flows is of.compare_channel_flows and "compare_channel_flows" in of.__all__
    p = inspect.signature(of.compare_channel_flows).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert positional == [("movie_a", inspect.Parameter.empty), ("movie_b", inspect.Parameter.empty), ("boxsize", 31), ("delta_x", 1.0),
                          ("delta_t", 1.0), ("smoothing_sigma", None), ("background", None), ("include_remodelling", False),
                          ("filename", None)]
    keyword = [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY]
    assert keyword == [("histogram_bins", 50), ("histogram_range", None), ("angle_bins", 50), ("relative_angle_bins", 50),
                       ("joint_speed_bins", None), ("joint_speed_ranges", None), ("joint_speed_min_b", None), ("return_fields", False),
                       ("reference_quirks", True), ("device", 0), ("output", "numpy")]


def test_argument_errors_need_no_gpu(monkeypatch):
    from opticalflow_amd import optical_flow as of, _native

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load_library", no_library)
    a = np.random.default_rng(0).random((3, 16, 12))
    b = np.random.default_rng(1).random((3, 16, 12))
    ok = dict(histogram_range=(0.0, 1.0))
    cases = [
        ((a, b[:, :, :11]), ok, "same shape"),
        ((a, b[:2]), ok, "same shape"),
        ((a[:1], b[:1]), ok, "two frames"),
        ((a[0], b[0]), ok, "3-D"),
        ((a, b), {}, "histogram_range"),
        ((a, b), dict(histogram_bins=0, histogram_range=(0.0, 1.0)), "histogram_bins"),
        ((a, b), dict(ok, angle_bins=0), "angle_bins"),
        ((a, b), dict(ok, angle_bins=65), "angle_bins"),
        ((a, b), dict(ok, relative_angle_bins=0), "relative_angle_bins"),
        ((a, b), dict(ok, relative_angle_bins=65), "relative_angle_bins"),
        ((a, b), dict(ok, relative_angle_bins=None), "relative_angle_bins"),
        ((a, b), dict(ok, joint_speed_bins=(50, 50)), "joint_speed_ranges"),
        ((a, b), dict(ok, joint_speed_bins=50, joint_speed_ranges=((0, 1), (0, 1))), "pair"),
        ((a, b), dict(ok, joint_speed_bins=(50, 50, 50), joint_speed_ranges=((0, 1), (0, 1))), "pair"),
        ((a, b), dict(ok, joint_speed_bins=(50, 50), joint_speed_ranges=(0, 1)), "pair"),
        ((a, b), dict(ok, joint_speed_bins=(50, 50), joint_speed_ranges=((0, 1), (0, 1), (0, 1))), "pair"),
        ((a, b), dict(ok, joint_speed_bins=(0, 50), joint_speed_ranges=((0, 1), (0, 1))), "1 .. 1024"),
        ((a, b), dict(ok, joint_speed_bins=(50, 1025), joint_speed_ranges=((0, 1), (0, 1))), "1 .. 1024"),
        ((a, b), dict(ok, joint_speed_bins=(50, 50), joint_speed_ranges=((0, 1), (1, 1))), "joint_speed"),
        ((a, b), dict(ok, smoothing_sigma=(1.0, 2.0, 3.0)), "pair"),
        ((a, b), dict(ok, smoothing_sigma=(1.0,)), "pair"),
        ((a, b), dict(ok, background=(1.0, 2.0, 3.0)), "pair"),
        ((a, b), dict(ok, smoothing_sigma=0.0), "smoothing_sigma"),
        ((a, b), dict(ok, boxsize=0), "boxsize"),
        ((a, b), dict(ok, output="cupy"), "output"),
    ]
    for movies, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            of.compare_channel_flows(*movies, **kw)
    # the script's own 50, 50 and 50 x 50 pass the checks
    of._compare_arguments(a, b, 31, 3, None, 50, (0.0, 1.0), 50, 50, (50, 50), ((0.0, 1.0), (0.0, 1.0)), "numpy")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    a = np.random.default_rng(0).random((3, 16, 16))
    b = np.random.default_rng(1).random((3, 16, 16))
    with pytest.raises(_native.VofError):
        optical_flow.compare_channel_flows(a, b, boxsize=5, histogram_range=(0.0, 1.0))


# ---- the restatement on hand-built fields ---------------------------------------------------------------------------------
def flow(vectors):
    v = np.asarray(vectors, dtype=np.float64).reshape(1, 1, -1, 2)
    v_x, v_y = v[..., 0], v[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        return dict(v_x=v_x, v_y=v_y, speed=np.sqrt(v_x * v_x + v_y * v_y))


def test_restatement_on_hand_built_fields():
    from compare_restatement import compare_summaries, relative_angle
    a = flow([(3.0, 4.0), (2.0, 0.0), (3.0, 4.0), (0.0, 0.0), (1.0, 1.0), (np.nan, 1.0)])
    b = flow([(6.0, 8.0), (0.0, 5.0), (-6.0, -8.0), (1.0, 0.0), (1.0, 0.0), (1.0, 0.0)])
    theta, w = relative_angle(a, b)
    assert theta.ravel()[0] == 0.0 and theta.ravel()[1] == 0.5 and theta.ravel()[2] == 1.0          # parallel, orthogonal, antiparallel
    assert np.isnan(theta.ravel()[3]) and w.ravel()[3] == 0.0                                       # a zero speed
    s = compare_summaries(a, b, relative_angle_bins=50)
    hist = s["relative_angle_histogram"]
    assert hist.dtype == np.int64 and hist.shape == (50,)
    assert hist[0] == 1                               # parallel: bin 0
    assert hist[25] == 1 and hist[24] == 0            # orthogonal: exactly on the 0.5 edge, in the upper bin
    assert hist[49] == 1                              # antiparallel: the closed last bin
    assert hist[12] == 1 and hist.sum() == 4          # 45 degrees; nothing else
    assert s["relative_angle_dropped"] == 1           # the zero speed
    assert s["joint_nonfinite_count"] == 1            # the NaN speed
    assert np.array_equal(s["relative_angle_edges"], np.linspace(0.0, 1.0, 51)) and s["relative_angle_edges"][25] == 0.5
    sums = s["weighted_relative_angle_histogram"]
    assert sums[0] == 50.0 and sums[25] == 10.0 and sums[49] == 50.0 and sums[12] == np.sqrt(2.0)
    assert np.array_equal(s["weighted_relative_angle_density"], sums / np.diff(s["relative_angle_edges"]) / sums.sum())
    assert list(s["nonfinite_counts"]) == [1, 0]


def test_restatement_cos_above_one():
    """A pair of equal vectors whose rounded dot product exceeds the rounded product of the speeds: NaN with the reference's
    quirks, bin 0 without them."""
    from compare_restatement import compare_summaries, relative_angle
    found = None
    rng = np.random.default_rng(5)
    for v in rng.random((200, 2)):
        f = flow([v])
        with np.errstate(invalid="ignore"):
            cos = (f["v_x"] * f["v_x"] + f["v_y"] * f["v_y"]) / (f["speed"] * f["speed"])
        if cos.ravel()[0] > 1.0:
            found = f
            break
    assert found is not None, "no vector among 200 rounds above 1"
    theta, _ = relative_angle(found, found, reference_quirks=True)
    assert np.isnan(theta).all()
    quirky = compare_summaries(found, found, relative_angle_bins=50, reference_quirks=True)
    assert quirky["relative_angle_dropped"] == 1 and quirky["relative_angle_histogram"].sum() == 0
    assert quirky["joint_nonfinite_count"] == 0
    clipped = compare_summaries(found, found, relative_angle_bins=50, reference_quirks=False)
    assert clipped["relative_angle_dropped"] == 0 and clipped["relative_angle_histogram"][0] == 1


def test_restatement_joint_speeds_and_channels():
    from compare_restatement import compare_summaries
    a = flow([(0.5, 0.0), (0.0, 1.5), (2.0, 0.0), (0.0, 4.0), (np.nan, 0.0), (0.0, 2.5)])
    b = flow([(1.0, 0.0), (0.0, 0.5), (3.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, 9.0)])
    kw = dict(histogram_bins=4, histogram_range=(0.0, 4.0), angle_bins=4, joint_speed_bins=(4, 3), joint_speed_ranges=((0.0, 4.0), (0.0, 3.0)))
    s = compare_summaries(a, b, **kw)
    assert s["joint_speed_histogram"].dtype == np.int64 and s["joint_speed_histogram"].shape == (4, 3)
    want = np.zeros((4, 3), dtype=np.int64)
    want[0, 1] = want[1, 0] = want[2, 2] = want[3, 1] = 1          # 4.0 in the closed last bin of a; NaN and 9.0 dropped
    assert np.array_equal(s["joint_speed_histogram"], want)
    strict = compare_summaries(a, b, joint_speed_min_b=1.0, **kw)["joint_speed_histogram"]      # speed_b > 1.0, strictly
    want[0, 1] = want[3, 1] = want[1, 0] = 0
    assert np.array_equal(strict, want)
    assert np.array_equal(s["speed_histograms"], [[1, 1, 2, 1], [1, 3, 0, 1]])
    # directions: +x is 0.5, +y is 0; a NaN speed counts nowhere
    assert np.array_equal(s["angle_histograms"], [[0, 0, 3, 2], [0, 0, 3, 3]])
    assert np.array_equal(s["weighted_angle_histograms"][0], [0.0, 0.0, 1.5 + 4.0 + 2.5, 0.5 + 2.0])
    assert np.isnan(s["speed_means"][0]) and s["speed_means"][1] == np.mean(b["speed"])
