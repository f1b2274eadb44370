"""CPU tests of conduct_piv's specification: tests/piv_flow_restatement.py against an independent formulation, the margins its
decisions have, the window grid, the argument checks and the accuracy on a moving texture.  The device is held to the restatement
bit for bit by tests/test_gpu_piv_flow.py."""
import numpy as np
import pytest

import piv_flow_restatement as pf

# The largest difference between a correlation value of the restatement and of the independent formulation (mean-subtracted
# windows through scipy.signal.correlate2d) over every window, pass and pair of piv_flow_restatement.CASES, as measured, and the
# tolerance asserted: 8 times that, 1.92e-12.  Neither formulation is exact: both round some thousand products and sums per value,
# and the largest difference, 2.39e-13, is in a window of `two_pass` that reaches into the constant block, where little variance is left.
MEASURED_DIFFERENCE = 2.4e-13
TOLERANCE = 8 * MEASURED_DIFFERENCE
# Outside the crafted exact tie the two highest correlations of a window lie at least this far apart: 2.4e-7 (measured: 5.7e-5 at least)
SMALLEST_GAP = 1e6 * MEASURED_DIFFERENCE


def independent_surface(A, B):
    """ZNCC of the window ``A`` over the region ``B`` from mean-subtracted windows: sum (A - mean A) (B_d - mean B_d) / sqrt(sum
    (A - mean A)^2 sum (B_d - mean B_d)^2); the mean of B_d drops out of the numerator because A - mean A sums to zero."""
    from scipy.signal import correlate2d
    n = A.size
    A0 = A - A.mean()
    ones = np.ones_like(A)
    s_b, s_bb = correlate2d(B, ones, mode="valid"), correlate2d(B * B, ones, mode="valid")
    with np.errstate(invalid="ignore", divide="ignore"):
        return correlate2d(B, A0, mode="valid") / np.sqrt((A0 * A0).sum() * (s_bb - s_b * s_b / n))


def windows(name):
    """Every window of every pass and pair of a case that is not flat: (pass, pair, a, b, A, B, surface, peak, gap)."""
    c = pf.case(name)
    frames = np.asarray(c["movie"], dtype=np.float64)
    passes = pf.grid(frames.shape[1:], c["window_sizes"], c["search_radii"], c["steps"])
    details = pf.restated(name)[4]
    for p, q in enumerate(passes):
        w, r, s, m = q["w"], q["r"], q["s"], q["m"]
        for k, det in enumerate(details[p]):
            for a in range(q["R"]):
                for b in range(q["C"]):
                    if np.isnan(det["gap"][a, b]):
                        continue
                    i0, j0 = m + a * s, m + b * s
                    top, left = i0 + det["offset"][a, b, 0] - r, j0 + det["offset"][a, b, 1] - r
                    yield (p, k, a, b, frames[k, i0:i0 + w, j0:j0 + w], frames[k + 1, top:top + w + 2 * r, left:left + w + 2 * r],
                           det["surface"][a, b], det["peak"][a, b], det["gap"][a, b])


def tied(name, p, a, b):
    return name == "flat_ties_border" and (a, b) in pf.FLAT_TIES_TIED


@pytest.mark.parametrize("name", pf.CASES)
def test_restatement_agrees_with_mean_subtracted_correlate2d(name):
    """Every integer peak equal, every correlation value within TOLERANCE = 8 x the largest difference seen over the cases
    (MEASURED_DIFFERENCE = 2.4e-13: 2.39e-13 in `two_pass`, in a window that reaches into the constant block; 9.3e-14 at most on the plain
    [0, 1] textures, 6e-15 on the uint8 cases).
    In the windows of the crafted exact tie the independent values tie only to rounding, so there the restatement's peak must be
    a maximum of the independent surface to within the tolerance."""
    worst, count = 0.0, 0
    for p, k, a, b, A, B, surface, peak, gap in windows(name):
        other = independent_surface(A, B)
        finite = np.isfinite(surface)
        assert finite.any() and np.isfinite(other[finite]).all()
        worst = max(worst, np.abs(other[finite] - surface[finite]).max())
        r = (surface.shape[0] - 1) // 2
        at = np.unravel_index(np.argmax(np.where(finite, other, -np.inf)), other.shape)
        if tied(name, p, a, b):
            assert other[peak[0] + r, peak[1] + r] >= other[at] - TOLERANCE
        else:
            assert (at[0] - r, at[1] - r) == tuple(peak), (p, k, a, b)
        count += 1
    print(name, count, "windows, largest difference of a correlation value", worst)
    assert count > 0 and worst <= TOLERANCE


@pytest.mark.parametrize("name", pf.CASES)
def test_no_decision_hangs_on_the_last_bits(name):
    """Outside the crafted exact tie the two highest correlations of every window are at least SMALLEST_GAP = 10^6 x
    MEASURED_DIFFERENCE apart (measured: 5.7e-5 at least, the issue's prototype saw 9e-5); in the tie they are equal, and the
    first in raster order, (-3, -3), is the peak.  No peak correlation lies that close to the threshold either."""
    c = pf.case(name)
    smallest, ties = np.inf, []
    for p, k, a, b, A, B, surface, peak, gap in windows(name):
        if tied(name, p, a, b):
            assert gap == 0.0 and tuple(peak) == (-3, -3)
            ties.append((a, b))
        else:
            smallest = min(smallest, gap)
        if c["min_correlation"] is not None:
            assert abs(surface.max() - c["min_correlation"]) >= SMALLEST_GAP
    print(name, "smallest gap between the two highest correlations of a window", smallest)
    assert smallest >= SMALLEST_GAP
    assert ties == (pf.FLAT_TIES_TIED if name == "flat_ties_border" else [])


@pytest.mark.parametrize("name", pf.INTEGER_CASES)
def test_integer_data_is_order_independent(name):
    """uint8 movies: every sum is an integer below 2^53, so plain np.sum gives the bits of the defined order."""
    assert pf.case(name)["movie"].dtype == np.uint8
    for a, b in zip(pf.restated(name)[:3], pf.restated(name, False)[:3]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(pf.restated(name)[3], pf.restated(name, False)[3])


def test_cases_cover_what_they_are_for():
    u, v, _, counts, details = pf.restated("integer_shift")
    assert counts.tolist() == [[0, 0, 0]] and (details[0][0]["peak"] == (2, -1)).all() and (details[0][1]["peak"] == (-1, 2)).all()
    assert np.abs(u[0] + 1).max() < 0.1 and np.abs(v[0] - 2).max() < 0.1
    g = pf.grid((37, 45), (10,), (2,), (7,))[0]
    assert (37 - 10 - 4) % 7 and (45 - 10 - 4) % 7 and (g["R"], g["C"]) == (4, 5)
    u, v, corr, counts, details = pf.restated("flat_ties_border")
    assert np.isnan(u[0, 0, 0]) and np.isnan(corr[0, 0, 0]) and counts[0, 0] == 1
    assert (details[0][0]["peak"][:, :3, 1] == 3).sum() >= 10 and counts[0, 1] >= 25      # the 5-pixel move: the border at d_j = 3
    u, v, corr, counts, details = pf.restated("two_pass")
    assert counts[0].tolist() == [1, 0, 0] and counts[1, 0] == 4 and np.isnan(u[0, :2, :2]).all()
    assert (details[1][0]["offset"][:2, :2] == 0).all() and (details[1][0]["offset"][4:, 4:] == (2, -4)).all()
    counts = pf.restated("thresholded")[3]
    assert 0 < counts[0, 2] < pf.restated("thresholded")[0].size
    assert pf.restated("largest")[0].shape == (1, 1, 2) and pf.case("largest")["window_sizes"] == (64,) and pf.case("largest")["search_radii"] == (16,)


@pytest.mark.parametrize("shape, w, r, s", [((1024, 1024), (64, 32), (16, 4), None), ((37, 45), (10,), (2,), (7,)), ((96, 80), (32, 16), (6, 2), (16, 8)),
                                            ((96, 112), (64,), (16,), (16,)), ((3, 50, 61), (12, 12, 6), (3, 2, 1), (5, 4, 1))])
def test_piv_grid(shape, w, r, s):
    from opticalflow_amd import optical_flow as of
    N_i, N_j = shape[-2:]
    grids = of.piv_grid(shape, w, r, s)
    assert len(grids) == len(w)
    margin = 0
    for p, g in enumerate(grids):
        step = w[p] // 2 if s is None else s[p]
        previous, margin = margin, margin + r[p]
        assert (g["w"], g["r"], g["s"], g["m"]) == (w[p], r[p], step, margin)
        assert g["R"] == (N_i - w[p] - 2 * margin) // step + 1 >= 1 and g["C"] == (N_j - w[p] - 2 * margin) // step + 1 >= 1
        assert g["x"].shape == g["y"].shape == (g["R"], g["C"]) and g["x"].dtype == np.float64
        i0, j0 = margin + step * np.arange(g["R"]), margin + step * np.arange(g["C"])
        assert np.array_equal(g["y"], np.repeat((i0 + (w[p] - 1) / 2)[:, None], g["C"], 1))
        assert np.array_equal(g["x"], np.repeat((j0 + (w[p] - 1) / 2)[None], g["R"], 0))
        for offset in (-previous, previous):                          # the largest offsets the pass before can hand on
            assert i0[0] + offset - r[p] >= 0 and j0[0] + offset - r[p] >= 0
            assert i0[-1] + offset + r[p] + w[p] <= N_i and j0[-1] + offset + r[p] + w[p] <= N_j
    mine = pf.grid(shape[-2:], w, r, [g["s"] for g in grids])
    assert [(g["m"], g["R"], g["C"]) for g in grids] == [(g["m"], g["R"], g["C"]) for g in mine]


@pytest.mark.parametrize("arguments", [
    dict(window_sizes=(3,), search_radii=(2,)), dict(window_sizes=(65,), search_radii=(2,)), dict(window_sizes=(8,), search_radii=(0,)),
    dict(window_sizes=(8,), search_radii=(17,)), dict(window_sizes=(8,), search_radii=(2,), steps=(0,)),
    dict(window_sizes=(8, 16), search_radii=(2, 2)), dict(window_sizes=(38,), search_radii=(2,)),
    dict(window_sizes=(16, 8), search_radii=(8, 9)), dict(window_sizes=(8, 8), search_radii=(2,)), dict(window_sizes=(8,), search_radii=(2,), steps=(4, 4)),
    dict(window_sizes=(), search_radii=()), dict(window_sizes=(8,) * 9, search_radii=(1,) * 9), dict(window_sizes=(8.5,), search_radii=(2,)),
    dict(window_sizes=(8,), search_radii=(2,), min_correlation="high"), dict(window_sizes=(8,), search_radii=(2,), smoothing_sigma=0.0)])
def test_value_errors_before_the_library_is_touched(arguments, monkeypatch):
    from opticalflow_amd import _native, optical_flow as of

    def untouched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "Solver", untouched)
    movie = np.zeros((2, 40, 40))
    with pytest.raises(ValueError):
        of.conduct_piv(movie, **arguments)
    with pytest.raises(ValueError):
        of.conduct_piv_flow(movie, **arguments)
    if not {"min_correlation", "smoothing_sigma"} & set(arguments):
        with pytest.raises(ValueError):
            of.piv_grid(movie.shape, **arguments)


def test_too_few_frames_and_bad_movies(monkeypatch):
    from opticalflow_amd import _native, optical_flow as of
    monkeypatch.setattr(_native, "Solver", None)
    for movie in (np.zeros((1, 40, 40)), np.zeros((40, 40))):
        with pytest.raises(ValueError):
            of.conduct_piv(movie, (8,), (2,))
        with pytest.raises(ValueError):
            of.conduct_piv_flow(movie, window_sizes=(8,), search_radii=(2,))
    with pytest.raises(ValueError):
        of.conduct_piv_flow(np.zeros((2, 40, 40)), output="cupy", window_sizes=(8,), search_radii=(2,))
    with pytest.raises(ValueError):
        of.conduct_piv(np.zeros((2, 95, 120)))                             # the default passes need 64 + 2 * 16 = 96 pixels


def test_lds_need_of_every_accepted_window_is_within_the_limit():
    """The largest accepted configuration, w = 64 and r = 16, needs 8 (64 * 65 + 96 * 97 + 2 * 96 * 33) = 158 464 bytes of the
    160 KiB less 2 KiB the kernel may ask for, and no other accepted pair needs more."""
    from opticalflow_amd import optical_flow as of
    assert of._piv_lds_bytes(64, 16) == 158464 <= of.PIV_LDS_LIMIT == 160 * 1024 - 2048
    assert max(of._piv_lds_bytes(w, r) for w in range(4, 65) for r in range(1, 17)) == 158464


def test_accuracy_on_a_moving_texture():
    """synthetic.texture_stack_numpy(96, 2, seed=3, shift=(0.3, 0.6)), one pass w = 32, r = 4, s = 16: mean u and v within 0.02 of 0.6
    and 0.3 (measured 0.5918 and 0.3103).  The two-pass case: last-pass means within 0.15 of (-3.6, 2.3) (measured -3.6174 and
    2.2469) and no border peaks."""
    from opticalflow_amd import synthetic
    u, v, _, counts, _ = pf.piv(synthetic.texture_stack_numpy(96, 2, seed=3, shift=(0.3, 0.6)), (32,), (4,), (16,))
    print("one pass: mean u", u.mean(), "mean v", v.mean(), "counts", counts.tolist())
    assert abs(u.mean() - 0.6) <= 0.02 and abs(v.mean() - 0.3) <= 0.02 and counts.tolist() == [[0, 0, 0]]
    u, v, _, counts, _ = pf.restated("two_pass")
    print("two passes: mean u", np.nanmean(u), "mean v", np.nanmean(v), "counts", counts.tolist())
    assert abs(np.nanmean(u) + 3.6) <= 0.15 and abs(np.nanmean(v) - 2.3) <= 0.15
    assert counts[:, 1].tolist() == [0, 0]
