"""GPU tests of apply_adaptive_threshold and apply_clahe: every result equals the numpy restatement
(tests/preprocess_restatement.py) bit for bit - np.array_equal, no tolerance.  Each test first asserts, on the restatement's
record, that its input takes the path it is there for."""
import functools
import math

import numpy as np
import pytest

import preprocess_restatement as R
from preprocess_cases import CLAHE_CASES, THRESHOLD_CASES, clahe_input, threshold_input

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def threshold_reference(name, w, t):
    rec = {}
    mask = R.adaptive_threshold(threshold_input(name), w, t, rec)
    return mask, rec


@functools.lru_cache(maxsize=None)
def clahe_reference(case):
    name, clip_limit, tile_number = CLAHE_CASES[case]
    rec = {}
    out = R.clahe(clahe_input(name), clip_limit, tile_number, rec)
    return out, rec


def of():
    from opticalflow_amd import optical_flow
    return optical_flow


# ---- adaptive threshold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,t", THRESHOLD_CASES)
@pytest.mark.parametrize("name", ["raw", "blurred"])
def test_threshold_equals_the_restatement(name, w, t):
    movie = threshold_input(name)
    want, rec = threshold_reference(name, w, t)
    assert movie.shape == (3, 37, 53) and 37 % 64 and 53 % 64
    assert 0.3 < want.mean() < 0.6                                     # neither side of the comparison is rare
    assert np.array_equal(rec["mean"], rec["mean_float32"]) and np.array_equal(rec["mean"], rec["mean_float64"])
    if w == 151:
        assert w // 2 > max(movie.shape[1:])                           # every window reaches over all four edges
    if w == 3:
        assert rec["S"].max() <= 9 * 255 and (rec["mean"] != rec["u"]).any()
    if t != int(t) or t < 0:                                           # ceil, not floor or round-half-away: the masks differ
        assert math.ceil(t) != math.floor(t) or t < 0
        other = (rec["u"].astype(np.int64) - rec["mean"]) > -(math.floor(t) if t != int(t) else int(t) - 1)
        assert not np.array_equal(other, want)
    got = of().apply_adaptive_threshold(movie, w, t)
    assert got.dtype == np.bool_ and got.shape == movie.shape
    assert np.array_equal(got, want)


def test_threshold_interior_and_clamped_windows():
    movie = threshold_input("wide")
    want, rec = threshold_reference("wide", 151, -5)
    assert movie.shape == (2, 300, 300) and 300 - 2 * 75 > 0           # rows / columns 75 .. 224 see no edge, the others are clamped
    assert 300 > 256 and 300 > 4 * 64                                  # more than one scan tile per row, more than one strip of rows
    assert 0.2 < want.mean() < 0.8
    assert np.array_equal(rec["mean"], rec["mean_float32"]) and np.array_equal(rec["mean"], rec["mean_float64"])
    got = of().apply_adaptive_threshold(movie, window_size=151, threshold=-5)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 75:225, 75:225], want[:, 75:225, 75:225]) and np.array_equal(got[:, :75], want[:, :75])


def test_threshold_float32_movie_is_computed_in_float64():
    movie = threshold_input("blurred").astype(np.float32)
    want = R.adaptive_threshold(movie.astype(np.float64), 11, 2.5)
    assert np.array_equal(of().apply_adaptive_threshold(movie, 11, 2.5), want)


def test_threshold_cross_checks():
    import torch
    from opticalflow_amd import _native
    movie = threshold_input("blurred")
    want, _ = threshold_reference("blurred", 11, 2.5)
    first = of().apply_adaptive_threshold(movie, 11, 2.5)
    assert np.array_equal(of().apply_adaptive_threshold(movie, 11, 2.5), first)                 # a second call
    dev = of().apply_adaptive_threshold(torch.as_tensor(movie.copy()).cuda(), 11, 2.5, output="torch")
    assert dev.dtype == torch.bool and dev.is_cuda and tuple(dev.shape) == movie.shape
    assert np.array_equal(dev.cpu().numpy(), first)                                             # the torch entry
    assert np.array_equal(of().apply_adaptive_threshold(movie, 11, 2.5, output="torch").cpu().numpy(), first)
    with _native.Solver(37, 53, 1) as solver:                                                   # 1 frame in flight, 2, all
        for flight in (1, 2, 0):
            assert np.array_equal(solver.adaptive_threshold_host(movie, 11, 2.5, frames_in_flight=flight), want), flight
        frames = torch.as_tensor(movie.copy()).cuda()
        for flight in (1, 3):
            mask = torch.zeros(movie.shape, dtype=torch.bool, device="cuda")
            torch.cuda.synchronize()
            solver.adaptive_threshold_dev(frames, mask, 3, 11, 2.5, frames_in_flight=flight)
            assert np.array_equal(mask.cpu().numpy(), want), flight


def test_threshold_nothing_staged_survives_a_call():
    """One context, one host array at one address: the whole stack is staged (frames_in_flight=0), the array is overwritten in
    place, and the second call sees the new frames."""
    from opticalflow_amd import _native
    m = threshold_input("blurred").copy()
    with _native.Solver(37, 53, 1) as solver:
        first = solver.adaptive_threshold_host(m, 11, 2.5, frames_in_flight=0)
        m[...] = threshold_input("raw")
        second = solver.adaptive_threshold_host(m, 11, 2.5, frames_in_flight=0)
    assert np.array_equal(first, threshold_reference("blurred", 11, 2.5)[0])
    assert np.array_equal(second, threshold_reference("raw", 11, 2.5)[0]) and not np.array_equal(second, first)


def test_threshold_range_is_accumulated_over_chunks():
    """One frame in flight, the offending value in frame 0 only: it is not in the chunk the range reduction leaves staged."""
    from opticalflow_amd import _native
    movie = threshold_input("raw")
    with _native.Solver(37, 53, 1) as solver:
        for bad, message in ((np.nan, "non-finite"), (-1.0, "negative")):
            m = movie.copy()
            m[0, 3, 5] = bad
            with pytest.raises(ValueError, match=message):
                solver.adaptive_threshold_host(m, 11, 2.5, frames_in_flight=1)
        assert np.array_equal(solver.adaptive_threshold_host(movie, 11, 2.5, frames_in_flight=1), threshold_reference("raw", 11, 2.5)[0])


def test_threshold_value_errors():
    import torch
    movie = threshold_input("raw").copy()
    for bad in (np.nan, np.inf, -1.0):
        m = movie.copy()
        m[2, 36, 52] = bad
        with pytest.raises(ValueError, match="non-finite|negative"):
            of().apply_adaptive_threshold(m, 11)
        with pytest.raises(ValueError, match="non-finite|negative"):
            of().apply_adaptive_threshold(torch.as_tensor(m).cuda(), 11, output="torch")
        with pytest.raises(ValueError):
            R.adaptive_threshold(m, 11)
    with pytest.raises(ValueError, match="maximum"):
        of().apply_adaptive_threshold(np.zeros((2, 37, 53)), 11)
    assert np.array_equal(of().apply_adaptive_threshold(movie, 11), R.adaptive_threshold(movie, 11))   # the context still works


# ---- CLAHE ----------------------------------------------------------------------------------------------------------------
def clahe_paths(case, rec):
    """What the case's input is there for, asserted on the restatement's record."""
    tiles = rec["tiles"]
    clip, clipped, residual, batch, step = (tiles[..., k] for k in range(5))
    grid = (rec["tilesX"], rec["tilesY"], rec["tw"], rec["th"], rec["pad_i"], rec["pad_j"])
    if case == "A":
        assert grid == (4, 6, 14, 7, 5, 3) and (clipped == 0).all()
    elif case == "B3000":
        assert rec["clip"] == 4 and (clipped[0] > 0).sum() == 19 and (clipped[0] == 0).sum() == 5
    elif case == "B1500":
        assert rec["clip"] == 2 and (clipped > 0).all() and (step > 1).all()
    elif case == "B1":
        assert rec["clip"] == 1 == max(int(1 * 98 / 65536), 1) and (clipped > 0).all() and (step > 1).all()
    elif case == "C":
        assert grid == (5, 6, 11, 7, 2, 5) and 50 % 5 == 0 and (clipped > 0).any()         # the dividing width gets a full 5 columns
    elif case == "D":
        assert grid[4:] == (0, 0) and (clipped[0] > 0).sum() == 5 and (clipped[0] == 0).sum() == 11
    elif case == "E":
        assert grid[:2] == (1, 1) and (clipped >= 65536).all() and (batch == 1).all() and (residual > 0).all()
    elif case == "F":
        assert (residual > 32768).all() and (step == 1).all() and (batch == 0).all()
    elif case == "G":
        v = clahe_input("G")
        assert v.max() >= 65535 and v.min() == 0 and (v != np.trunc(v)).any()
    if case.startswith("B"):
        assert len({tuple(t) for t in tiles[0]}) > 1                                        # the tiles differ: the blend matters


@pytest.mark.parametrize("case", sorted(CLAHE_CASES))
def test_clahe_equals_the_restatement(case):
    name, clip_limit, tile_number = CLAHE_CASES[case]
    movie = clahe_input(name)
    want, rec = clahe_reference(case)
    clahe_paths(case, rec)
    got = of().apply_clahe(movie, clip_limit, tile_number)
    assert got.dtype == np.float64 and got.shape == movie.shape
    assert np.array_equal(got, want)
    if case == "E":
        assert (got[0] == 1237.0).all()
    if case == "F":
        assert (got == 104.0).all()


def test_clahe_without_clipping():
    movie = clahe_input("B")
    want = R.clahe(movie, 0, 4)
    assert not np.array_equal(want, clahe_reference("B3000")[0])
    assert np.array_equal(of().apply_clahe(movie, 0, 4), want)


def test_clahe_cross_checks():
    import torch
    from opticalflow_amd import _native
    name, clip_limit, tile_number = CLAHE_CASES["C"]
    movie = clahe_input(name)
    want, rec = clahe_reference("C")
    assert movie.shape[0] == 2 and not np.array_equal(want[0], want[1])
    first = of().apply_clahe(movie, clip_limit, tile_number)
    assert np.array_equal(first, want)
    assert np.array_equal(of().apply_clahe(movie, clip_limit, tile_number), first)              # a second call
    dev = of().apply_clahe(torch.as_tensor(movie.copy()).cuda(), clip_limit, tile_number, output="torch")
    assert dev.dtype == torch.float64 and dev.is_cuda
    assert np.array_equal(dev.cpu().numpy(), first)                                             # the torch entry
    with _native.Solver(40, 50, 1) as solver:                                                   # 1 frame in flight, all
        for flight in (1, 0):
            assert np.array_equal(solver.clahe_host(movie, clip_limit, rec["tilesX"], rec["tilesY"], frames_in_flight=flight), want), flight
        frames = torch.as_tensor(movie.copy()).cuda()
        for flight in (1, 2):
            out = torch.zeros(movie.shape, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            solver.clahe_dev(frames, out, 2, clip_limit, rec["tilesX"], rec["tilesY"], frames_in_flight=flight)
            assert np.array_equal(out.cpu().numpy(), want), flight


def test_clahe_nothing_staged_survives_a_call():
    """As test_threshold_nothing_staged_survives_a_call; the second movie is the first with its two frames exchanged."""
    from opticalflow_amd import _native
    name, clip_limit, _ = CLAHE_CASES["A"]
    want, rec = clahe_reference("A")
    assert want.shape[0] == 2 and not np.array_equal(want[0], want[1])
    m = clahe_input(name).copy()
    with _native.Solver(37, 53, 1) as solver:
        first = solver.clahe_host(m, clip_limit, rec["tilesX"], rec["tilesY"], frames_in_flight=0)
        m[...] = clahe_input(name)[::-1]
        second = solver.clahe_host(m, clip_limit, rec["tilesX"], rec["tilesY"], frames_in_flight=0)
    assert np.array_equal(first, want)
    assert np.array_equal(second, want[::-1]) and not np.array_equal(second, first)


def test_clahe_range_is_accumulated_over_chunks():
    from opticalflow_amd import _native
    name, clip_limit, _ = CLAHE_CASES["A"]
    want, rec = clahe_reference("A")
    m = clahe_input(name).copy()
    m[0, 3, 5] = 65536.0                                                                        # frame 0 of 2, one frame in flight
    with _native.Solver(37, 53, 1) as solver:
        with pytest.raises(ValueError, match="65536"):
            solver.clahe_host(m, clip_limit, rec["tilesX"], rec["tilesY"], frames_in_flight=1)
        assert np.array_equal(solver.clahe_host(clahe_input(name), clip_limit, rec["tilesX"], rec["tilesY"], frames_in_flight=1), want)


def test_clahe_value_errors():
    import torch
    movie = clahe_input("A").copy()
    for bad in (65536.0, -1.0, np.nan):
        m = movie.copy()
        m[1, 36, 52] = bad
        with pytest.raises(ValueError, match="65536|non-finite"):
            of().apply_clahe(m, 50000, 4)
        with pytest.raises(ValueError, match="65536|non-finite"):
            of().apply_clahe(torch.as_tensor(m).cuda(), 50000, 4, output="torch")
        with pytest.raises(ValueError):
            R.clahe(m, 50000, 4)
    m = movie.copy()
    m[1, 36, 52] = 65535.9                                                                      # the largest value that does not wrap
    assert np.array_equal(of().apply_clahe(m, 50000, 4), R.clahe(m, 50000, 4))
