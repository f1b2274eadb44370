"""CPU tests of the two preprocessing calls (apply_adaptive_threshold, apply_clahe): the boundary of the new entry points
(header, library, binding, Python names and defaults, no CPU fallback), the argument errors, and the numpy restatement on
hand-built cases."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

ENTRY_POINTS = {"vof_adaptive_threshold_dev": 8, "vof_adaptive_threshold_host": 8, "vof_clahe_dev": 9, "vof_clahe_host": 9}


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)
    for name, n_args in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        assert hasattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert len(args) == len(decl.group(1).split(",")) == n_args
    for method in ("adaptive_threshold_host", "adaptive_threshold_dev", "clahe_host", "clahe_dev"):
        assert hasattr(_native.Solver, method)
    assert "vof_preprocess.hpp" in build.default_deps(build.CSRC, build.SOURCES[0])
    assert "preprocess" in _native.K_NAMES and lib.vof_kernel_name(_native.K_NAMES.index("preprocess")).decode() == "preprocess"


def test_limits_agree_on_every_layer():
    from opticalflow_amd import optical_flow as of
    src = open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_preprocess.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (PP_[A-Z_]+) = (\d+);", src)}
    assert const["PP_MAX_WINDOW"] == of.THRESHOLD_MAX_WINDOW == 4095 and 255 * 4095 ** 2 < 2 ** 32
    assert const["PP_MAX_ROW"] == of.THRESHOLD_MAX_ROW and const["PP_MAX_ROW"] * 4 + 16 <= 65536      # LDS of the row pass
    assert const["PP_BINS"] == 65536
    assert "3 .. 4095" in of.apply_adaptive_threshold.__doc__ and "15360" in of.apply_adaptive_threshold.__doc__


def test_python_names_and_signatures():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    want = {"apply_adaptive_threshold": [("movie", inspect.Parameter.empty), ("window_size", 51), ("threshold", 0.0)],
            "apply_clahe": [("movie", inspect.Parameter.empty), ("clipLimit", 50000), ("tile_number", 10)]}
    for name, positional in want.items():
        assert getattr(shim, name) is getattr(of, name) and name in of.__all__
        p = inspect.signature(getattr(of, name)).parameters
        assert [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD] == positional
        assert [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == [("device", 0), ("output", "numpy")]


def test_argument_errors_need_no_gpu(monkeypatch):
    from opticalflow_amd import optical_flow as of, _native

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load_library", no_library)
    monkeypatch.setattr(_native, "Solver", no_library)
    m = np.random.default_rng(0).random((2, 16, 12)) * 100
    for kw, match in [(dict(window_size=4), "odd"), (dict(window_size=1), "odd"), (dict(window_size=0), "odd"), (dict(window_size=-3), "odd"),
                      (dict(window_size=5.5), "odd"), (dict(window_size=4097), "4095"), (dict(threshold=float("nan")), "NaN"),
                      (dict(output="cupy"), "output")]:
        with pytest.raises(ValueError, match=match):
            of.apply_adaptive_threshold(m, **kw)
    for bad in (m[0], m[None], m[:, :3], m[:0]):
        with pytest.raises(ValueError, match="3-D|4x4"):
            of.apply_adaptive_threshold(bad)
        with pytest.raises(ValueError, match="3-D|4x4"):
            of.apply_clahe(bad)
    # the tile grid against the image: tilesX = tile_number <= N_j - 1 = 11, tilesY = round(tile_number * 12 / 16) <= N_i - 1 = 15
    for kw, match in [(dict(tile_number=12), "tile grid"), (dict(tile_number=0), "tile grid"), (dict(tile_number=2.5), "integer"),
                      (dict(output="cupy"), "output"), (dict(clipLimit=float("nan")), "NaN")]:
        with pytest.raises(ValueError, match=match):
            of.apply_clahe(m, **kw)
    with pytest.raises(ValueError, match="tile grid"):
        of.apply_clahe(np.zeros((1, 5, 40)), tile_number=1)           # tilesY = 8 > N_i - 1
    with pytest.raises(ValueError, match="tile grid"):
        of.apply_clahe(np.zeros((1, 40, 5)), tile_number=2)           # tilesY = round(0.25) = 0
    assert of.clahe_tile_grid((1, 37, 53), 4) == (4, 6) and of.clahe_tile_grid((1, 1024, 1024), 10) == (10, 10)
    assert of.clahe_tile_grid((1, 40, 50), 10) == (10, 12)            # 12.5: Python's round, half to even


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    m = np.random.default_rng(0).random((2, 16, 16)) * 100
    with pytest.raises(_native.VofError):
        optical_flow.apply_adaptive_threshold(m, 5)
    with pytest.raises(_native.VofError):
        optical_flow.apply_clahe(m, tile_number=2)


# ---- the restatement on hand-built cases ----------------------------------------------------------------------------------
def test_restatement_constant_frame():
    from preprocess_restatement import adaptive_threshold
    m = np.full((2, 9, 7), 3.5)
    for t in (0.5, 1, 7.2):
        assert adaptive_threshold(m, 5, t).all()
    for t in (0.0, -0.5, -1, -7.2):
        assert not adaptive_threshold(m, 5, t).any()
    assert adaptive_threshold(m, 5, 1).dtype == np.bool_


def test_restatement_single_bright_pixel():
    from preprocess_restatement import adaptive_threshold
    m = np.zeros((1, 9, 9))
    m[0, 4, 4] = 10.0
    rec = {}
    mask = adaptive_threshold(m, 3, 0.0, rec)
    assert rec["u"][0, 4, 4] == 255 and rec["u"].sum() == 255
    assert (rec["S"][0, 3:6, 3:6] == 255).all() and rec["S"].sum() == 9 * 255
    assert (rec["mean"][0, 3:6, 3:6] == 28).all()                     # 255 / 9 = 28.33
    want = np.zeros((1, 9, 9), dtype=bool)
    want[0, 4, 4] = True                                              # 255 - 28 > 0; its neighbours 0 - 28, the rest 0 - 0
    assert np.array_equal(mask, want)
    far = adaptive_threshold(m, 3, 1)                                 # > -1: everything but the ring around the pixel
    want = np.ones((1, 9, 9), dtype=bool)
    want[0, 3:6, 3:6] = False
    want[0, 4, 4] = True
    assert np.array_equal(far, want)
    # the truncation of step 2: 9.99 / 10 * 255 = 254.7 -> 254
    m[0, 0, 0] = 9.99
    rec = {}
    adaptive_threshold(m, 3, 0.0, rec)
    assert rec["u"][0, 0, 0] == 254
    assert rec["S"][0, 0, 0] == 4 * 254                               # the corner counts (1 + 1)^2 times in its own window


def test_restatement_window_larger_than_image():
    from preprocess_restatement import adaptive_threshold
    rng = np.random.default_rng(4)
    m = rng.integers(0, 256, (1, 4, 5)).astype(np.float64)
    m[0, 0, 0] = 255.0
    rec = {}
    mask = adaptive_threshold(m, 11, -3, rec)
    u = m[0].astype(np.int64)
    assert np.array_equal(rec["u"][0], u)
    for i in range(4):
        for j in range(5):
            s = sum(u[min(max(i + a, 0), 3), min(max(j + b, 0), 4)] for a in range(-5, 6) for b in range(-5, 6))
            assert rec["S"][0, i, j] == s
            mean = int(np.floor(s / 121.0 + 0.5))
            assert rec["mean"][0, i, j] == mean
            assert mask[0, i, j] == (u[i, j] - mean > 3)
    for t in (-3.0, -2.5, -2.000001):                                 # ceil: all of them -> 3
        assert np.array_equal(adaptive_threshold(m, 11, t), mask)
    with pytest.raises(ValueError):
        adaptive_threshold(m, 10)
    with pytest.raises(ValueError):
        adaptive_threshold(m, 1)
    for bad in (np.nan, np.inf, -1.0):
        b = m.copy()
        b[0, 1, 1] = bad
        with pytest.raises(ValueError):
            adaptive_threshold(b, 3)
    with pytest.raises(ValueError):
        adaptive_threshold(np.zeros((1, 4, 5)), 3)


def test_restatement_reflect_101_and_geometry():
    from preprocess_restatement import clahe_geometry, reflect101
    assert list(reflect101(np.arange(9), 5)) == [0, 1, 2, 3, 4, 3, 2, 1, 0]
    g = clahe_geometry(37, 53, 4, 50000)
    assert (g["tilesX"], g["tilesY"], g["pad_i"], g["pad_j"], g["tw"], g["th"], g["clip"]) == (4, 6, 5, 3, 14, 7, 74)
    g = clahe_geometry(40, 50, 5, 3000)                               # the width divides, the height does not: a full 5 columns
    assert (g["tilesX"], g["tilesY"], g["pad_i"], g["pad_j"], g["tw"], g["th"]) == (5, 6, 2, 5, 11, 7)
    g = clahe_geometry(40, 40, 4, 3000)
    assert (g["pad_i"], g["pad_j"], g["tw"], g["th"], g["clip"]) == (0, 0, 10, 10, 4)
    assert clahe_geometry(40, 40, 4, 1)["clip"] == 1 and clahe_geometry(40, 40, 4, 0)["clip"] == 0
    assert clahe_geometry(1024, 1024, 10, 50000)["clip"] == int(50000 * 103 * 103 / 65536)


def test_restatement_clahe_constant_closed_form():
    """200 x 250 of one value, one tile, clip 1: all 49 999 clipped counts go one each to the bins 0 .. 49 998, so the sum up to
    bin v is (v + 1) + 1 and the output rint((v + 2) * 65535 / 50000)."""
    from preprocess_restatement import clahe
    rec = {}
    out = clahe(np.full((1, 200, 250), 77.0), 1, 1, rec)
    assert tuple(rec["tiles"][0, 0]) == (1, 49999, 49999, 0, 1)
    assert (out == 104.0).all() and np.rint(np.float32(79) * (np.float32(65535) / np.float32(50000))) == 104
    assert out.dtype == np.float64
    unclipped = clahe(np.full((1, 200, 250), 77.0), 0, 1)             # no clipping: the sum jumps to the area at bin 77
    assert (unclipped == 65535.0).all()
    for bad in (65536.0, -1.0, np.nan):
        m = np.full((1, 8, 8), 5.0)
        m[0, 2, 2] = bad
        with pytest.raises(ValueError):
            clahe(m, 1, 1)
