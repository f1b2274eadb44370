"""CPU tests of correct_intensity_change and intensity_histograms: the numpy restatement against scipy and against the reference
scripts' own lines, the argument checks, and the new symbols of the C ABI.

The restatement's blur keeps the kernels' summation order, which is scipy's (NI_Correlate1D, symmetric branch); the subtractions
are single IEEE operations.  The restatement therefore equals the scipy chain bit for bit, and the tests say so."""
import os
import re

import numpy as np
import pytest

import intensity_restatement as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("target", ir.TARGETS)
@pytest.mark.parametrize("case", range(len(ir.SCIPY_CASES)))
def test_restatement_equals_scipy_chain_bit_for_bit(case, target):
    shape, s1, s2 = ir.SCIPY_CASES[case]
    movie = ir.case_stack(shape)
    got, drift = ir.correct(movie, s1, s2, target, 0)
    want = ir.scipy_correct(movie, s1, s2, target, 0)
    print(shape, s1, s2, target, "largest difference", np.abs(got - want).max())
    assert got.dtype == np.float64 and got.shape == shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    Tg = movie.astype(np.float64) if target == "original" or s1 is None else ir.blur(movie, s1)
    assert np.array_equal(got[0].view(np.uint64), Tg[0].view(np.uint64)) and not drift[0].any() and not np.signbit(drift[0]).any()


def test_the_two_script_snippets():
    """analyse_short_timeinterval_data.py:245-252 and :135-144 on frames [8:10] of a stack, with skimage.filters.gaussian(f, sigma,
    preserve_range=True) written as the scipy call it makes."""
    from scipy.ndimage import gaussian_filter

    def gaussian(f, sigma):
        return gaussian_filter(f, sigma, mode="nearest", truncate=4.0)
    movie = ir.integer_stack((10, 31, 45), 77)[8:10]
    original_movie = movie.astype("float")
    blurred_movie = np.stack([gaussian(f, 3) for f in original_movie])
    # :249-252
    difference = blurred_movie[1, :, :] - blurred_movie[0, :, :]
    blurred_difference = gaussian(difference, 5)
    corrected_second_frame = blurred_movie[1, :, :] - blurred_difference
    got, drift = ir.correct(movie, 3, 5, "blurred", 0)
    assert np.array_equal(got[1], corrected_second_frame) and np.array_equal(got[0], blurred_movie[0])
    assert np.array_equal(drift[1], blurred_difference)
    # :138-144
    blurred_difference = gaussian(difference, 7.5)
    corrected_movie = np.copy(original_movie)
    corrected_movie[1, :, :] = original_movie[1, :, :] - blurred_difference
    got, _ = ir.correct(movie, 3, 7.5, "original", 0)
    assert np.array_equal(got, corrected_movie)


def test_restatement_histograms_are_numpy():
    movie = ir.integer_stack((2, 5, 7), 3).astype(np.float64)
    movie[0, 0, 0], movie[1, 1, 1], movie[1, 2, 2] = 255.0, np.nan, np.inf
    counts, nonfinite = ir.histograms(movie, 255, (0, 255))
    assert counts.shape == (2, 255) and counts.dtype == np.int64 and list(nonfinite) == [0, 2]
    assert list(counts.sum(1) + ir.dropped(movie, (0, 255))) == [35, 35]
    assert counts[0, 254] == np.count_nonzero(movie[0] >= 254)


MOVIE = np.zeros((3, 6, 7))


@pytest.mark.parametrize("kwargs", [
    dict(reference_frame=3), dict(reference_frame=-4), dict(reference_frame=0.5), dict(reference_frame=None),
    dict(target="previous"), dict(target=None),
    dict(smoothing_sigma=0), dict(smoothing_sigma=-1.0), dict(smoothing_sigma=np.nan), dict(smoothing_sigma=np.inf),
    dict(filter_size=0), dict(filter_size=-2), dict(filter_size=np.nan), dict(filter_size=np.inf), dict(filter_size=None),
    dict(movie=np.zeros((6, 7))), dict(movie=np.zeros((2, 3, 6, 7))), dict(movie=np.zeros((3, 3, 7))), dict(movie=np.zeros((3, 7, 3))),
    dict(movie=np.zeros((0, 6, 7))), dict(output="cupy"),
])
def test_correct_intensity_change_refuses_before_the_library_is_touched(kwargs, monkeypatch):
    from opticalflow_amd import _native, optical_flow as of

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "load_library", no_library)
    kwargs = dict(kwargs)
    movie = kwargs.pop("movie", MOVIE)
    with pytest.raises(ValueError):
        of.correct_intensity_change(movie, **kwargs)


@pytest.mark.parametrize("kwargs", [
    dict(bins=0), dict(bins=-3), dict(bins=2.5), dict(bins=2 ** 20 + 1),
    dict(value_range=(0, np.inf)), dict(value_range=(np.nan, 1)), dict(value_range=(1, 1)), dict(value_range=(2, 1)), dict(value_range=(0, 1, 2)),
    dict(smoothing_sigma=0), dict(smoothing_sigma=-1), dict(smoothing_sigma=np.nan), dict(smoothing_sigma=np.inf),
    dict(movie=np.zeros((6, 7))), dict(movie=np.zeros((3, 3, 7))), dict(output="cupy"),
])
def test_intensity_histograms_refuses_before_the_library_is_touched(kwargs, monkeypatch):
    from opticalflow_amd import _native, optical_flow as of

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "load_library", no_library)
    kwargs = dict(kwargs)
    movie = kwargs.pop("movie", MOVIE)
    with pytest.raises(ValueError):
        of.intensity_histograms(movie, **kwargs)


def test_names_are_exported():
    import opticalflow_amd
    from opticalflow_amd import optical_flow as of
    for name in ("correct_intensity_change", "intensity_histograms"):
        assert getattr(opticalflow_amd, name) is getattr(of, name) and name in of.__all__


NEW_SYMBOLS = ["vof_intensity_correct_dev", "vof_intensity_correct_host", "vof_intensity_hist_dev", "vof_intensity_hist_host"]


def test_new_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    header = open(os.path.join(ROOT, "include", "vof.h")).read()
    assert re.search(r"#define VOF_VERSION 202\b", header)
    declared = re.findall(r"\b(vof_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    build.build_native(verbose=False)
    lib = _native.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert len(_native.SIGNATURES[name][1]) == len(_native.TWINS[name.rsplit("_", 1)[0]])
    assert len(_native.TWINS["vof_intensity_correct"]) == 12 and len(_native.TWINS["vof_intensity_hist"]) == 10
    assert lib.vof_version() == 202
    for method in ("intensity_correct", "intensity_hist"):
        assert callable(getattr(_native.Solver, method))
