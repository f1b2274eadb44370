"""CPU tests of downsample_movie: the boundary of the new entry points (header, library, binding, Python names, no CPU
fallback), the argument errors, and the numpy restatement (tests/resize_restatement.py) against an independent formulation
and on hand-built cases - the restatement is what the GPU tests compare with, so it is kept honest here."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import resize_restatement as R
from conftest import ROOT
from resize_cases import CASES, case_input

ENTRY_POINTS = {"vof_resize_area_dev": 8, "vof_resize_area_host": 8}


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)
    for name, n_args in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        assert hasattr(lib, name)
        _res, args = _native.SIGNATURES[name]
        assert len(args) == len(decl.group(1).split(",")) == n_args
    values = dict(re.findall(r"\b(VOF_RESIZE_[A-Z0-9]+)\s*=\s*(\d+)", header))
    assert values == {"VOF_RESIZE_U8": str(_native.RESIZE_U8), "VOF_RESIZE_F64": str(_native.RESIZE_F64)}
    for method in ("resize_area_host", "resize_area_dev"):
        assert hasattr(_native.Solver, method)
    assert "vof_resize.hpp" in build.default_deps(build.CSRC, build.SOURCES[0])
    assert len(_native.K_NAMES) == 17                                  # the profiler classes did not change: stage 6 of "preprocess"


def test_python_name_and_signature():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    import opticalflow_amd
    from opticalflow_amd import optical_flow as of
    assert shim.downsample_movie is of.downsample_movie is opticalflow_amd.downsample_movie and "downsample_movie" in of.__all__
    p = inspect.signature(of.downsample_movie).parameters
    assert [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD] == [("movie", inspect.Parameter.empty),
                                                                                            ("resolution", inspect.Parameter.empty)]
    assert [(n, v.default) for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == [("device", 0), ("output", "numpy")]


def test_argument_errors_need_no_gpu(monkeypatch):
    from opticalflow_amd import optical_flow as of, _native

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load_library", no_library)
    monkeypatch.setattr(_native, "Solver", no_library)
    m = np.zeros((2, 16, 12))
    for dtype in (np.float32, np.int64, np.uint16, np.bool_):
        with pytest.raises(ValueError, match="cast"):
            of.downsample_movie(m.astype(dtype), 8)
    for resolution in (0, -3, 13, 17, (17, 4), (4, 13), (0, 4), 4.5, (4, 4, 4), True):
        with pytest.raises(ValueError, match="resolution"):
            of.downsample_movie(m, resolution)
        with pytest.raises(ValueError, match="resolution"):
            of.downsample_movie(m.astype(np.uint8), resolution)
    for bad in (m[0], m[None], m[:, :3], m[:0]):
        with pytest.raises(ValueError, match="3-D|4x4"):
            of.downsample_movie(bad, 2)
    with pytest.raises(ValueError, match="output"):
        of.downsample_movie(m, 8, output="cupy")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    with pytest.raises(_native.VofError):
        optical_flow.downsample_movie(np.zeros((2, 16, 16)), 8)
    with pytest.raises(_native.VofError):
        optical_flow.downsample_movie(np.zeros((2, 16, 16), dtype=np.uint8), (8, 4))


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_exact_area_mean(name):
    """Two float32 weights of relative error 2^-24 each multiply every sample and the weights of an output pixel sum to 1, so the
    float64 restatement is within 3 * 2^-24 * max|S| of the exact mean; the uint8 one adds its rounding to an integer (1 / 2)."""
    _shape, (n_i, n_j) = CASES[name]
    for depth in ("u8", "f64"):
        movie = case_input(name, depth)
        got = R.resize_area(movie, n_i, n_j)
        assert got.dtype == np.float64 and got.shape == (movie.shape[0], n_i, n_j)
        exact = np.stack([R.exact_area_mean(f, n_i, n_j) for f in movie])
        diff = np.abs(got - exact).max()
        print(name, depth, "max |restatement - exact mean| =", diff)
        if depth == "f64":
            assert diff <= 3 * 2.0 ** -24 * np.abs(movie).max()
        else:
            assert diff <= 0.51
            assert (got == np.rint(got)).all() and got.min() >= 0 and got.max() <= 255


@pytest.mark.parametrize("ssize,dsize", [(26, 10), (21, 9), (41, 8), (53, 10), (40, 13), (10, 3), (300, 70), (333, 130), (1024, 100),
                                         (1024, 150), (1024, 200), (50, 50), (50, 25), (7, 1)])
def test_table_properties(ssize, dsize):
    entries, detail = R.axis_table(ssize, dsize)
    assert len(entries) == dsize
    for (idx, w), det in zip(entries, detail):
        assert w.dtype == np.float32 and len(idx) == len(w) >= 1
        assert (w > 0).all()                                            # every weight is positive
        assert (np.diff(idx) == 1).all()                                # the entries of one output index are consecutive
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 4 * 2.0 ** -24
        assert idx[0] >= 0 and idx[-1] <= ssize - 1                     # the last index never exceeds ssize - 1
        assert len(idx) == int(det["head"]) + (det["s2"] - det["s1"]) + int(det["tail"])
    firsts = [int(i[0]) for i, _ in entries]
    ends = [int(i[-1]) + 1 for i, _ in entries]
    assert firsts == sorted(firsts) and ends == sorted(ends)            # the runs move right with the output index
    assert firsts[0] == 0 and ends[-1] == ssize


def test_a_constant_uint8_frame_stays_constant_on_every_path():
    paths = set()
    for (_T, N_i, N_j), (n_i, n_j) in CASES.values():
        for value in (0, 1, 77, 254, 255):
            rec = {}
            out = R.resize_area(np.full((1, N_i, N_j), value, dtype=np.uint8), n_i, n_j, rec)
            assert (out == value).all(), (rec["path"], N_i, N_j, n_i, n_j, value)
            paths.add(rec["path"])
    assert paths == {"general", "fast", "fast2x2"}


def test_the_identity_returns_the_input():
    for depth in ("u8", "f64"):
        movie = case_input("identity", depth)
        rec = {}
        out = R.resize_area(movie, *movie.shape[1:], rec)
        assert rec["path"] == "fast" and rec["area"] == 1 and float(rec["scale_f"]) == 1.0
        assert np.array_equal(out, movie.astype(np.float64))


def test_hand_built_blocks():
    """The three roundings of the fast path on numbers small enough to do by hand."""
    two = np.array([[[1, 2, 4, 4], [2, 1, 5, 5], [0, 0, 255, 255], [0, 1, 255, 254]]], dtype=np.uint8)
    # 2 x 2 sums 6, 18, 1, 1019: (s + 2) >> 2 = 2, 5, 0, 255;  rint(s / 4) would give 2, 4, 0, 255
    rec = {}
    assert np.array_equal(R.resize_area(two, 2, 2, rec)[0], [[2, 5], [0, 255]]) and rec["path"] == "fast2x2"
    assert np.array_equal(rec["rint"][0], [[2, 4], [0, 255]])
    # 1 x 2 sums 3, 8, 3, 10 / ... : rint(s * 0.5f) is half to even: 1.5 -> 2, 2.5 -> 2
    pairs = np.array([[[1, 2, 4, 4], [2, 3, 5, 5], [0, 0, 3, 2], [0, 1, 255, 254]]], dtype=np.uint8)
    assert np.array_equal(R.resize_area(pairs, 4, 2)[0], [[2, 4], [2, 5], [0, 2], [0, 254]])
    # float64, 1 x 5: ((a + b) + c) + d first, then e: 2^60 + 1 + 1 + 1 loses every 1, and so does the rest of one; left to right too
    BIG = 2.0 ** 60
    row = np.array([[[BIG, 1.0, 1.0, 1.0, 1.0]] * 4], dtype=np.float64)
    assert R.unrolled_sum(np.array([BIG, 1.0, 1.0, 1.0, 1.0])) == BIG
    assert R.unrolled_sum(np.array([1.0, BIG, -BIG, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0])) == 8.0   # (0 + 1) + (1 + 1 + 1 + 1) + 3, not 9
    out = R.resize_area(row, 4, 1)
    assert out.shape == (1, 4, 1) and (out == BIG * np.float64(np.float32(1.0) / np.float32(5.0))).all()
    # the general path, 3 x 2 -> 2 x 1: columns float32(1 / 2) twice (exact), rows float32(1 / 1.5) and float32(0.5 / 1.5)
    b0, b1 = np.float64(np.float32(1.0 / 1.5)), np.float64(np.float32(0.5 / 1.5))
    rec = {}
    out = R.resize_area(np.array([[[3.0, 4.0], [5.0, 8.0], [1.0, 1.0]]]), 2, 1, rec)
    assert rec["path"] == "general" and [list(i) for i, _ in rec["ytab"]] == [[0, 1], [1, 2]]
    assert out[0, 0, 0] == b0 * 3.5 + b1 * 6.5 and out[0, 1, 0] == b1 * 6.5 + b0 * 1.0


def test_restatement_rejects_what_the_product_rejects():
    for bad, res in ((np.zeros((1, 8, 8), dtype=np.float32), (4, 4)), (np.zeros((1, 8, 8)), (9, 4)), (np.zeros((1, 8, 8)), (4, 0)),
                     (np.zeros((8, 8)), (4, 4))):
        with pytest.raises(ValueError):
            R.resize_area(bad, *res)
