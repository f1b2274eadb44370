"""CPU tests of the blur sweep (vary_blursize): the boundary of the new entry points (header, library, binding, Python names,
no CPU fallback), the argument errors, and the taps the sweep hands to the device blur."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

C_SIZES = {"double": 8, "int64_t": 8, "int32_t": 4}
C_DTYPES = {"double": np.float64, "int64_t": np.int64, "int32_t": np.int32}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = header_text()
    for name in ("vof_vary_blursize_dev", "vof_vary_blursize_host"):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        assert hasattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert len(args) == len(decl.group(1).split(",")) == 28
    assert lib.vof_version() == 202
    assert hasattr(_native.Solver, "vary_blursize_host") and hasattr(_native.Solver, "vary_blursize_dev")


def test_stats_record_matches_the_header():
    """sizeof(vof_blursize_stats) from the header's own field list (no field of it needs padding: 8-byte fields first) against
    the numpy record of the binding: same names, types, order and size; vof_boxsize_stats with sigma_index for box_size."""
    from opticalflow_amd import _native
    body = re.search(r"typedef struct vof_blursize_stats \{(.*?)\} vof_blursize_stats;", header_text(), flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"\b(double|int64_t|int32_t)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    offset = 0
    for _name, ctype in fields:
        assert offset % C_SIZES[ctype] == 0         # naturally aligned without padding
        offset += C_SIZES[ctype]
    assert offset % 8 == 0
    rec = _native.BLURSIZE_DTYPE
    assert rec.itemsize == offset == 48
    assert list(rec.names) == [n for n, _ in fields]
    assert [rec[n] for n in rec.names] == [np.dtype(C_DTYPES[t]) for _, t in fields]
    assert [rec.fields[n][1] for n in rec.names] == list(np.cumsum([0] + [C_SIZES[t] for _, t in fields[:-1]]))
    assert [n.replace("sigma_index", "box_size") for n in rec.names] == list(_native.BOXSIZE_DTYPE.names)


def test_blur_switch_is_documented():
    src = open(os.path.join(ROOT, "opticalflow_amd", "csrc", "vof_pairs.hip")).read()
    assert 'getenv("VOF_BLUR_TILED")' in src
    assert "VOF_BLUR_TILED=0" in open(os.path.join(ROOT, "include", "vof.h")).read()


def test_python_name_and_signature():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    assert shim.vary_blursize is of.vary_blursize and "vary_blursize" in of.__all__
    p = inspect.signature(of.vary_blursize).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert [n for n, _ in positional] == ["movie", "blursizes", "boxsize", "delta_x", "delta_t", "background", "include_remodelling",
                                          "filename"]
    assert np.array_equal(positional[1][1], np.arange(0.5, 15, 0.1)) and positional[1][1].size == 145
    assert [d for _, d in positional[2:]] == [21, 1.0, 1.0, None, False, None]
    keyword = [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY]
    assert keyword == [("histogram_bins", None), ("histogram_range", None), ("angle_bins", None), ("intensity_bins", None),
                       ("intensity_range", None), ("probe_locations", None), ("return_fields", False), ("reference_quirks", True),
                       ("device", 0), ("output", "numpy")]


def test_argument_errors_need_no_gpu():
    from opticalflow_amd import optical_flow as of
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(ValueError, match="empty"):
        of.vary_blursize(movie, [])
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite and > 0"):
            of.vary_blursize(movie, [1.0, bad])
    with pytest.raises(ValueError, match="histogram_range"):
        of.vary_blursize(movie, [1.0], histogram_bins=50)
    with pytest.raises(ValueError, match="intensity_range"):
        of.vary_blursize(movie, [1.0], intensity_bins=50)
    with pytest.raises(ValueError, match="angle_bins"):
        of.vary_blursize(movie, [1.0], angle_bins=0)
    with pytest.raises(ValueError, match="angle_bins"):
        of.vary_blursize(movie, [1.0], angle_bins=129)
    with pytest.raises(ValueError, match="probe outside"):
        of.vary_blursize(movie, [1.0], probe_locations=[(3, 16)])
    with pytest.raises(ValueError, match="output"):
        of.vary_blursize(movie, [1.0], output="cupy")
    with pytest.raises(ValueError, match="3-D"):
        of.vary_blursize(movie[0], [1.0])


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(_native.VofError):
        optical_flow.vary_blursize(movie, [0.5, 2.0], boxsize=5)


def test_gaussian_taps_are_unchanged():
    """The sweep's taps are gaussian_taps(s): stored values of the function as it was before the sweep, three sigmas (radii 2,
    10 and 60).  exp may differ in its last bit from one libm to the next: four units."""
    from opticalflow_amd import optical_flow as of
    g = load_golden("g13_gaussian_taps.npz")
    assert list(g["sigmas"]) == [0.5, 2.48, 15.0]
    for i, (sigma, radius) in enumerate(zip(g["sigmas"], (2, 10, 60))):
        taps = of.gaussian_taps(sigma)
        assert taps.shape == g[f"taps_{i}"].shape == (2 * radius + 1,)
        np.testing.assert_allclose(taps, g[f"taps_{i}"], rtol=4 * np.finfo(np.float64).eps, atol=0)
        assert np.array_equal(taps, taps[::-1])
