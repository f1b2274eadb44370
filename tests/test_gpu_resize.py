"""GPU tests of downsample_movie: every result equals the numpy restatement (tests/resize_restatement.py) bit for bit -
np.array_equal, no tolerance.  Each test first asserts, on the restatement's record, that its input takes the path it is there
for."""
import functools

import numpy as np
import pytest

import resize_restatement as R
from resize_cases import CASES, case_input

pytestmark = pytest.mark.gpu

DEPTHS = ("u8", "f64")


@functools.lru_cache(maxsize=None)
def reference(name, depth):
    rec = {}
    out = R.resize_area(case_input(name, depth), *CASES[name][1], rec)
    out.setflags(write=False)
    return out, rec


def of():
    from opticalflow_amd import optical_flow
    return optical_flow


def check(name, depth):
    movie = case_input(name, depth)
    want, _rec = reference(name, depth)
    assert movie.dtype == (np.uint8 if depth == "u8" else np.float64) and movie.shape == CASES[name][0]
    got = of().downsample_movie(movie, CASES[name][1])
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want)
    return got


def counts(table):
    return [len(i) for i, _ in table]


@pytest.mark.parametrize("depth", DEPTHS)
def test_entries_below_the_threshold_are_dropped(depth):
    _, rec = reference("dropped_entries", depth)
    assert rec["path"] == "general"
    head = [d for d, det in enumerate(rec["ydetail"]) if 0 < det["s1"] - det["f1"] <= 1e-3]
    tail = [d for d, det in enumerate(rec["xdetail"]) if 0 < det["f2"] - det["s2"] <= 1e-3]
    assert head == [5] and not rec["ydetail"][5]["head"] and len(tail) == 1 and not rec["xdetail"][tail[0]]["tail"]
    assert counts(rec["ytab"])[5] == 3 and 4 in counts(rec["ytab"])
    check("dropped_entries", depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_mixed_entry_counts(depth):
    _, rec = reference("mixed_counts", depth)
    assert rec["path"] == "general" and (rec["scale_y"], rec["scale_x"]) == (5.125, 5.3)
    assert set(counts(rec["xtab"])) == {6, 7} and set(counts(rec["ytab"])) == {6}
    check("mixed_counts", depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_one_fractional_and_one_integer_axis(depth):
    _, rec = reference("one_integer_axis", depth)
    assert rec["path"] == "general" and rec["scale_x"] == 2.0 and rec["scale_y"] != rec["iscale_y"]
    assert all(list(w) == [np.float32(0.5)] * 2 for _, w in rec["xtab"])
    check("one_integer_axis", depth)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", ["rows_only", "clipped_cell"])
def test_the_last_cell_is_clipped(name, depth):
    _, rec = reference(name, depth)
    assert rec["path"] == "general"
    last = rec["ydetail"][-1]
    assert last["cw"] < rec["scale_y"] and last["cw"] == CASES[name][0][1] - last["f1"]     # cw = ssize - f1 on 40 -> 3 and 10 -> 3
    if name == "rows_only":
        assert rec["scale_x"] == 1.0 and set(counts(rec["xtab"])) == {1}
    check(name, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_fast_path_area_2(depth):
    _, rec = reference("fast_area2", depth)
    assert rec["path"] == "fast" and (rec["iscale_y"], rec["iscale_x"], rec["area"]) == (1, 2, 2)
    got = check("fast_area2", depth)
    if depth == "u8":
        s = rec["block_sum"]
        assert (s % 2 == 1).any()                                      # odd sums: s / 2 is a tie
        assert not np.array_equal((s + 1) >> 1, got)                   # ... and rounding them half up would change the result


def test_fast_path_2x2_rounds_half_up():
    want, rec = reference("fast_2x2", "u8")
    assert rec["path"] == "fast2x2" and (rec["block_sum"] % 8 == 2).any()     # sums 4 q + 2 with even q
    assert not np.array_equal(rec["rint"], want)                       # rint(sum * 0.25f) would give another result
    check("fast_2x2", "u8")


def test_fast_path_2x2_float64():
    _, rec = reference("fast_2x2", "f64")
    assert rec["path"] == "fast" and rec["area"] == 4
    check("fast_2x2", "f64")


@pytest.mark.parametrize("depth", DEPTHS)
def test_fast_path_3x5(depth):
    want, rec = reference("fast_3x5", depth)
    assert rec["path"] == "fast" and (rec["iscale_y"], rec["iscale_x"], rec["area"]) == (3, 5, 15)
    if depth == "f64":
        assert not np.array_equal(rec["left_to_right"], want)          # the unrolled order differs from plain left to right
    check("fast_3x5", depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_identity(depth):
    _, rec = reference("identity", depth)
    assert rec["path"] == "fast" and rec["area"] == 1
    assert np.array_equal(check("identity", depth), case_input("identity", depth).astype(np.float64))


@pytest.mark.parametrize("depth", DEPTHS)
def test_several_column_blocks(depth):
    """333 columns: the rows of a frame start alternately on and off a 16-byte boundary, so the staged pieces begin both ways."""
    _, rec = reference("wide", depth)
    assert rec["path"] == "general" and CASES["wide"][0][2] % 2 == 1
    assert {int(i[0]) % 2 for i, _ in rec["xtab"]} == {0, 1}
    check("wide", depth)
    # 300 output columns: more than the 256 columns of one workgroup, so two column blocks per row
    movie = case_input("wide", depth)
    rec2 = {}
    want = R.resize_area(movie, 70, 300, rec2)
    assert rec2["path"] == "general" and len(rec2["xtab"]) > 256 and int(rec2["xtab"][256][0][0]) > 0
    assert np.array_equal(of().downsample_movie(movie, (70, 300)), want)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", ["long_rows", "long_rows_fast"])
def test_a_segment_longer_than_the_staging_buffer(name, depth):
    _, rec = reference(name, depth)
    assert rec["path"] == ("general" if name == "long_rows" else "fast") and CASES[name][0][2] > 2 * 2048   # RS_SEG: three pieces
    if name == "long_rows":
        assert set(counts(rec["xtab"])) == {1500}
    elif depth == "f64":
        assert not np.array_equal(rec["left_to_right"], reference(name, depth)[0])
    check(name, depth)


def test_cross_checks():
    import torch
    from opticalflow_amd import _native
    for depth, arithmetic in (("u8", _native.RESIZE_U8), ("f64", _native.RESIZE_F64)):
        movie = case_input("mixed_counts", depth)
        want, _ = reference("mixed_counts", depth)
        assert not np.array_equal(want[0], want[1])
        first = of().downsample_movie(movie, (8, 10))
        assert np.array_equal(first, want)
        assert np.array_equal(of().downsample_movie(movie, (8, 10)), first)                  # a second call
        tensor = torch.as_tensor(movie.copy()).cuda()
        dev = of().downsample_movie(tensor, (8, 10), output="torch")                         # the torch entry, device tensor
        assert dev.dtype == torch.float64 and dev.is_cuda and tuple(dev.shape) == (3, 8, 10)
        assert np.array_equal(dev.cpu().numpy(), want)
        assert np.array_equal(of().downsample_movie(movie.copy(), (8, 10), output="torch").cpu().numpy(), want)
        with _native.Solver(41, 53, 1) as solver:
            frames = tensor.to(torch.float64)
            for flight in (1, 2, 0):
                assert np.array_equal(solver.resize_area_host(movie, 8, 10, arithmetic, frames_in_flight=flight), want), flight
                out = torch.zeros((3, 8, 10), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                solver.resize_area_dev(frames, out, 3, 8, 10, arithmetic, frames_in_flight=flight)
                assert np.array_equal(out.cpu().numpy(), want), flight
    # the int form of `resolution` is (r, r) whatever the aspect ratio
    movie = case_input("mixed_counts", "f64")
    assert np.array_equal(of().downsample_movie(movie, 7), R.resize_area(movie, 7, 7))
    # the uint8 arithmetic on a stack that is not uint8-valued: refused by the library, not computed
    with _native.Solver(41, 53, 1) as solver:
        for bad in (256.0, -1.0, np.nan):
            m = case_input("mixed_counts", "u8").astype(np.float64)
            m[2, 40, 52] = bad
            with pytest.raises(ValueError, match="0 .. 255|non-finite"):
                solver.resize_area_host(m, 8, 10, _native.RESIZE_U8)
        assert np.array_equal(solver.resize_area_host(case_input("mixed_counts", "u8"), 8, 10, _native.RESIZE_U8), reference("mixed_counts", "u8")[0])


def test_nothing_staged_survives_a_call():
    """uint8 arithmetic, one context, one host array at one address: the whole stack is staged for the range reduction
    (frames_in_flight=0), the array is overwritten in place (the frames in reverse order), and the second call sees the new frames."""
    from opticalflow_amd import _native
    want, _ = reference("mixed_counts", "u8")
    m = case_input("mixed_counts", "u8").astype(np.float64)
    with _native.Solver(41, 53, 1) as solver:
        first = solver.resize_area_host(m, 8, 10, _native.RESIZE_U8, frames_in_flight=0)
        m[...] = m[::-1].copy()
        second = solver.resize_area_host(m, 8, 10, _native.RESIZE_U8, frames_in_flight=0)
    assert np.array_equal(first, want)
    assert np.array_equal(second, want[::-1]) and not np.array_equal(second, first)


def test_range_is_accumulated_over_chunks():
    """One frame in flight, 256 in frame 0 only: it is not in the chunk the range reduction leaves staged."""
    from opticalflow_amd import _native
    movie = case_input("mixed_counts", "u8")
    m = movie.astype(np.float64)
    m[0, 3, 5] = 256.0
    with _native.Solver(41, 53, 1) as solver:
        with pytest.raises(ValueError, match="0 .. 255"):
            solver.resize_area_host(m, 8, 10, _native.RESIZE_U8, frames_in_flight=1)
        assert np.array_equal(solver.resize_area_host(movie, 8, 10, _native.RESIZE_U8, frames_in_flight=1), reference("mixed_counts", "u8")[0])


def test_value_errors_leave_the_context_usable():
    movie = case_input("mixed_counts", "f64")
    want, _ = reference("mixed_counts", "f64")
    assert np.array_equal(of().downsample_movie(movie, (8, 10)), want)
    for bad, resolution in ((movie.astype(np.float32), (8, 10)), (movie.astype(np.int64), (8, 10)), (movie, 42), (movie, (8, 54)),
                            (movie, 0), (movie[0], (8, 10)), (movie[:, :3, :3], 2)):
        with pytest.raises(ValueError):
            of().downsample_movie(bad, resolution)
        assert np.array_equal(of().downsample_movie(movie, (8, 10)), want)                   # the context still serves a good call


def test_nan_propagates():
    movie = case_input("mixed_counts", "f64").copy()
    movie[1, 17, 29] = np.nan
    want = R.resize_area(movie, 8, 10)
    assert 0 < np.isnan(want).sum() < 4 and not np.isnan(want[0]).any()
    got = of().downsample_movie(movie, (8, 10))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)
    fast = case_input("fast_3x5", "f64").copy()
    fast[2, 38, 49] = np.nan
    want = R.resize_area(fast, 13, 10)
    assert np.isnan(want).sum() == 1 and np.isnan(want[2, 12, 9])
    assert np.array_equal(of().downsample_movie(fast, (13, 10)), want, equal_nan=True)


def test_downsample_blur_solve_stays_on_the_device():
    import torch
    rng = np.random.default_rng(77)
    i, j = np.meshgrid(np.arange(96), np.arange(96), indexing="ij")
    frames = [120 + 80 * np.sin(0.11 * (i + 1.5 * t)) * np.cos(0.07 * (j - 2.0 * t)) + rng.integers(0, 20, (96, 96)) for t in range(3)]
    m_u8 = np.stack(frames).astype(np.uint8)
    rec = {}
    want = R.resize_area(m_u8, 24, 24, rec)
    assert rec["path"] == "fast" and rec["area"] == 16
    m_u8_dev = torch.as_tensor(m_u8).cuda()
    r = of().variational_optical_flow(of().downsample_movie(m_u8_dev, 24, output="torch"), speed_alpha=1e3, remodelling_alpha=10, output="torch")
    assert r["original_data"].is_cuda and np.array_equal(r["original_data"].cpu().numpy(), want)
    assert r["v_x"].is_cuda and tuple(r["v_x"].shape) == (2, 24, 24) and bool(torch.isfinite(r["v_x"]).all())
