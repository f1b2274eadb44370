"""CPU tests of the box-size sweep (vary_boxsize): the numpy restatement of the ring-growing recurrence against every
fixture the reference wrote, and the boundary of the new entry points (header, library, binding, Python names, no CPU
fallback)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from boxflow_restatement import box_flow  # noqa: E402
from boxsweep_restatement import box_flow_extended, box_sweep  # noqa: E402
from test_boxflow_cpu import assert_matches, runs_of  # noqa: E402

FIELDS = ("v_x", "v_y", "speed", "net_remodelling")


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_recurrence_matches_the_reference(case):
    for label, movie, box, dx, dt, rem, ref in runs_of(case):
        r = box_sweep(movie, [box], dx, dt, include_remodelling=rem)[0]
        assert_matches(r, ref, r["kappa"], 64, label)


def test_recurrence_is_exact_on_integer_data():
    for label, movie, box, dx, dt, rem, ref in runs_of("d"):
        r = box_sweep(movie, [box], dx, dt, include_remodelling=rem)[0]
        for k in ("v_x", "v_y", "net_remodelling"):
            if k in ref:
                assert np.array_equal(r[k], ref[k]), (label, k)


@pytest.mark.parametrize("quirks", [True, False])
def test_recurrence_matches_the_direct_sums(quirks):
    """Unsorted list with a duplicate, an even / odd pair, h = 0 and a box larger than the image; both image orientations."""
    rng = np.random.default_rng(7)
    boxes = (9, 3, 16, 15, 9, 1, 100)
    for shape in ((12, 20), (20, 12)):
        movie = rng.random((3,) + shape)
        for rem in (False, True):
            sweep = box_sweep(movie, boxes, 0.5, 2.0, include_remodelling=rem, reference_quirks=quirks)
            for box, r in zip(boxes, sweep):
                d = box_flow(movie, box, 0.5, 2.0, include_remodelling=rem, reference_quirks=quirks)
                assert_matches(r, {k: d[k] for k in FIELDS}, d["kappa"], 64, f"{shape} box {box} rem {rem} quirks {quirks}")
            assert all(np.array_equal(sweep[0][k], sweep[4][k], equal_nan=True) for k in FIELDS)


def test_extended_precision_evaluation_agrees():
    movie = np.random.default_rng(3).random((2, 20, 28))
    for rem in (False, True):
        d = box_flow(movie, 7, include_remodelling=rem)
        x = box_flow_extended(movie, 7, include_remodelling=rem)
        assert x["v_x"].dtype == np.longdouble
        assert_matches({k: x[k].astype(np.float64) for k in FIELDS}, {k: d[k] for k in FIELDS}, d["kappa"], 64, f"extended rem {rem}")


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)
    for name in ("vof_vary_boxsize_dev", "vof_vary_boxsize_host"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert len(args) == 22
    assert re.search(r"\}\s*vof_boxsize_stats\s*;", header)
    assert _native.BOXSIZE_DTYPE.itemsize == 48
    assert lib.vof_version() == 202
    assert hasattr(_native.Solver, "vary_boxsize_host") and hasattr(_native.Solver, "vary_boxsize_dev")


def test_python_name_and_signature():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    assert shim.vary_boxsize is of.vary_boxsize and "vary_boxsize" in of.__all__
    p = inspect.signature(of.vary_boxsize).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert [n for n, _ in positional] == ["movie", "boxsizes", "delta_x", "delta_t", "smoothing_sigma", "background",
                                          "include_remodelling", "filename"]
    assert np.array_equal(positional[1][1], np.arange(5, 150, 2))
    assert [d for _, d in positional[2:]] == [1.0, 1.0, None, None, False, None]
    keyword = [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY]
    assert keyword == [("histogram_bins", None), ("histogram_range", None), ("probe_locations", None), ("return_fields", False),
                       ("reference_quirks", True), ("device", 0), ("output", "numpy")]


def test_argument_errors_need_no_gpu():
    from opticalflow_amd import optical_flow as of
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(ValueError, match="histogram_range"):
        of.vary_boxsize(movie, [5], histogram_bins=50)
    with pytest.raises(ValueError, match="probe outside"):
        of.vary_boxsize(movie, [5], probe_locations=[(3, 16)])
    with pytest.raises(ValueError):
        of.vary_boxsize(movie, [])
    with pytest.raises(ValueError):
        of.vary_boxsize(movie, [0.4])


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(_native.VofError):
        optical_flow.vary_boxsize(movie, [5, 9])
