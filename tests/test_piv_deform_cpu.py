"""CPU tests of the specification of conduct_piv's window deformation and outlier validation: tests/piv_deform_restatement.py against
independent formulations (scipy's map_coordinates for the predictor and the resampling, numpy's medians for the median test), the
margins its decisions have, what the cases cover, the accuracy gained and the argument checks.  The device is held to the
restatement bit for bit by tests/test_gpu_piv_deform.py."""
import itertools

import numpy as np
import pytest

import piv_deform_restatement as pd
import piv_flow_restatement as pf

# The largest difference between a pixel of a deformed search region of the restatement and of the independent formulation
# (scipy.ndimage.map_coordinates, order 1, for the predictor and for the sample) over every deformed pass of piv_deform_restatement.CASES,
# as measured, and the tolerance asserted: 8 times that.  The frames lie in [0, 1]; the two formulations round the two interpolation
# weights differently (map_coordinates forms (1 - t) a + t b).
MEASURED_DIFFERENCE = 3.2e-15                                                 # 3.11e-15, in the validation case; 9.5e-16 at most in the others
TOLERANCE = 8 * MEASURED_DIFFERENCE
SMALLEST_GAP = 1e6 * MEASURED_DIFFERENCE

DEFORMED = tuple(name for name in pd.CASES if pd.case(name)["deformation"])
VALIDATED = tuple(name for name in pd.CASES if pd.case(name)["outlier_threshold"] is not None)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_sorting_network_sorts():
    """The zero-one principle: a network that sorts every sequence of zeros and ones sorts every sequence."""
    for bits in itertools.product((0.0, 1.0), repeat=8):
        assert pd.sorted8(bits) == sorted(bits)
    rng = np.random.default_rng(5)
    for k in range(3, 9):
        values = list(rng.standard_normal(k)) + [pd.INF] * (8 - k)
        assert pd.median8(rng.permutation(values), k) == np.median(values[:k])


@pytest.mark.parametrize("name", pf.CASES)
def test_everything_off_is_the_integer_restatement(name):
    c = pf.case(name)
    want = pf.restated(name)
    for options in (dict(), dict(deformation=len(c["window_sizes"]) == 1)):      # one pass: deformation changes nothing
        got = pd.piv(c["movie"], c["window_sizes"], c["search_radii"], c["steps"], c["min_correlation"], **options)
        assert all(same_bits(g, w) for g, w in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])
        assert got[4].shape == (len(c["window_sizes"]), 2) and not got[4].any()
        for p, per_pair in enumerate(want[4]):
            for k, det in enumerate(per_pair):
                assert all(np.array_equal(det[key], got[5][p][k][key], equal_nan=True) for key in ("peak", "offset", "gap", "surface"))


def independent_warp(second, q, pu, pv):
    """Frame ``k + 1`` resampled by the vectors of pass ``q``, through scipy: the grid coordinate of a pixel is (i - c) / s."""
    from scipy.ndimage import map_coordinates
    valid = ~(np.isnan(pu) | np.isnan(pv))
    c = q["m"] + (q["w"] - 1) / 2
    i, j = np.meshgrid(np.arange(second.shape[0], dtype=np.float64), np.arange(second.shape[1], dtype=np.float64), indexing="ij")
    at = [(i - c) / q["s"], (j - c) / q["s"]]
    U, V = (map_coordinates(np.where(valid, f, 0.0), at, order=1, mode="nearest") for f in (pu, pv))
    return map_coordinates(second, [i + V, j + U], order=1, mode="nearest")


def vectors_before(name, p, k):
    """The vectors pass ``p`` of pair ``k`` starts from."""
    det = pd.restated(name)[5][p - 1][k]
    return (det["validation"]["u"], det["validation"]["v"]) if "validation" in det else det["raw"]


@pytest.mark.parametrize("name", DEFORMED)
def test_deformed_regions_agree_with_map_coordinates(name):
    """Every pixel of every search region of every deformed pass within TOLERANCE = 8 x MEASURED_DIFFERENCE of scipy's."""
    c = pd.case(name)
    frames = np.asarray(c["movie"], dtype=np.float64)
    passes = pf.grid(frames.shape[1:], c["window_sizes"], c["search_radii"], c["steps"])
    details = pd.restated(name)[5]
    worst = 0.0
    for p in range(1, len(passes)):
        g = passes[p]
        for k, det in enumerate(details[p]):
            other = independent_warp(frames[k + 1], passes[p - 1], *vectors_before(name, p, k))
            covered = np.zeros(frames.shape[1:], dtype=bool)
            for top, left in det["region_at"].reshape(-1, 2):
                covered[top:top + g["w"] + 2 * g["r"], left:left + g["w"] + 2 * g["r"]] = True
            assert (det["offset"] == 0).all() and covered.any()
            worst = max(worst, np.abs(other - det["second"])[covered].max())
    print(name, "largest difference of a pixel of a deformed region", worst)
    assert worst <= TOLERANCE


def independent_validation(u, v, threshold, epsilon):
    """The median test from numpy's medians over NaN-padded 3 x 3 neighbourhoods."""
    valid = ~(np.isnan(u) | np.isnan(v))
    R, C = u.shape
    pu, pv = (np.pad(np.where(valid, f, np.nan), 1, constant_values=np.nan) for f in (u, v))
    out_u, out_v, action = u.copy(), v.copy(), np.zeros((R, C), dtype=np.int64)
    ratios = np.full((R, C, 2), np.nan)
    centre = np.ones((3, 3), dtype=bool)
    centre[1, 1] = False
    for a in range(R):
        for b in range(C):
            un, vn = pu[a:a + 3, b:b + 3][centre], pv[a:a + 3, b:b + 3][centre]
            if (~np.isnan(un)).sum() < 3:
                action[a, b] = pd.TOO_FEW
                continue
            um, vm = np.nanmedian(un), np.nanmedian(vn)
            assert um == np.median(un[~np.isnan(un)])
            if not valid[a, b]:
                out_u[a, b], out_v[a, b], action[a, b] = um, vm, pd.FILLED
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                ratios[a, b] = abs(u[a, b] - um) / (np.nanmedian(np.abs(un - um)) + epsilon), abs(v[a, b] - vm) / (np.nanmedian(np.abs(vn - vm)) + epsilon)
            if (ratios[a, b] > threshold).any():
                out_u[a, b], out_v[a, b], action[a, b] = um, vm, pd.OUTLIER
    return out_u, out_v, action, ratios


@pytest.mark.parametrize("name", VALIDATED)
def test_median_test_agrees_with_numpy_medians(name):
    """Medians are selections and means of two: the same bits from np.median and np.nanmedian; every action equal."""
    c = pd.case(name)
    _, _, _, _, validation_counts, details = pd.restated(name)
    seen = 0
    for p, per_pair in enumerate(details):
        outliers = filled = 0
        for det in per_pair:
            if "validation" not in det:
                continue
            record = det["validation"]
            out_u, out_v, action, ratios = independent_validation(*det["raw"], c["outlier_threshold"], c["outlier_epsilon"])
            assert np.array_equal(action, record["action"])
            assert same_bits(out_u, record["u"]) and same_bits(out_v, record["v"])
            assert np.array_equal(ratios, record["ratio"], equal_nan=True)
            outliers, filled, seen = outliers + (action == pd.OUTLIER).sum(), filled + (action == pd.FILLED).sum(), seen + 1
        assert validation_counts[p].tolist() == [outliers, filled]
    assert seen == len(details[0]) * (len(details) if c["validate_last"] else len(details) - 1)


@pytest.mark.parametrize("name", pd.CASES)
def test_no_decision_hangs_on_the_last_bits(name):
    """The two highest correlations of every window at least SMALLEST_GAP = 10^6 x MEASURED_DIFFERENCE apart (no case has a crafted tie),
    no residual of the median test that close to the threshold, no peak correlation that close to min_correlation."""
    c = pd.case(name)
    details = pd.restated(name)[5]
    gap, to_threshold, to_minimum = np.inf, np.inf, np.inf
    for per_pair in details:
        for det in per_pair:
            found = ~np.isnan(det["gap"])
            gap = min(gap, det["gap"][found].min())
            if c["min_correlation"] is not None:
                to_minimum = min(to_minimum, np.abs(det["surface"][found].max(axis=(-2, -1)) - c["min_correlation"]).min())
            if "validation" in det:
                ratios = det["validation"]["ratio"]
                to_threshold = min(to_threshold, np.abs(ratios[~np.isnan(ratios)] - c["outlier_threshold"]).min())
    print(name, "smallest gap", gap, "closest residual to the threshold", to_threshold, "closest peak to min_correlation", to_minimum)
    assert min(gap, to_threshold, to_minimum) >= SMALLEST_GAP


def test_cases_cover_what_they_are_for():
    g0, g1 = pf.grid((50, 61), (12, 10), (3, 2), (5, 5))
    assert (50 - 12 - 6) % 5 and (61 - 12 - 6) % 5 and (g0["m"], g1["m"]) == (3, 5) and g0["w"] != g1["w"]
    c = pd.case("three_pass")
    assert c["window_sizes"][1] == c["window_sizes"][2] and len(c["window_sizes"]) == 3
    c = pd.case("one_row_largest")
    g0, g1 = pf.grid(c["movie"].shape[1:], c["window_sizes"], c["search_radii"], c["steps"])
    assert (g0["R"], g0["C"]) == (1, 2) and (g1["w"], g1["r"]) == (64, 16) and c["deformation"]
    # the validation case, integer offsets
    _, _, _, counts, validation_counts, details = pd.restated("validation_integer")
    record, raw = details[0][0]["validation"], details[0][0]["raw"]
    assert np.isnan(raw[0]).sum() == 2 and (record["action"] == pd.OUTLIER).sum() >= 1 and (record["action"] == pd.FILLED).sum() == 2
    assert validation_counts[0, 0] >= 1 and validation_counts[0, 1] >= 2 and not validation_counts[1].any()
    for flat in pd.VALIDATION_FLAT:
        assert np.isnan(raw[0][flat]) and record["action"][flat] == pd.FILLED and np.isfinite(record["u"][flat])
    assert record["action"][pd.VALIDATION_FOREIGN] == pd.OUTLIER
    assert abs(raw[0][pd.VALIDATION_FOREIGN] - pd.FOREIGN_SHIFT[1]) < 1.5 and abs(record["u"][pd.VALIDATION_FOREIGN] - pd.SHIFT[1]) < 0.5
    assert record["action"][pd.VALIDATION_FEW] == pd.TOO_FEW and record["neighbours"][pd.VALIDATION_FEW] == 2
    assert same_bits(record["u"][pd.VALIDATION_FEW], raw[0][pd.VALIDATION_FEW])
    assert record["neighbours"][pd.VALIDATION_THREE] == 3 and record["action"][pd.VALIDATION_THREE] == pd.KEPT
    acted = record["neighbours"][record["action"] != pd.TOO_FEW]
    assert (acted % 2 == 0).any() and (acted % 2 == 1).any()
    # without validation the pass-1 windows over the flat window take a zero prediction, with it that of the neighbours
    without = pd.restated("validation_integer", outlier_threshold=None)[5]
    over_flat = (without[1][0]["offset"][:2, :2] == 0).all(axis=-1)
    assert over_flat.all() and (details[1][0]["offset"][:2, :2] == (2, -4)).all()
    without = pd.restated("validation_deformed", outlier_threshold=None)[5]
    assert np.abs(without[1][0]["base"][0, 0]).max() < 0.5 and np.abs(pd.restated("validation_deformed")[5][1][0]["base"][0, 0] - pd.SHIFT).max() < 0.5
    # validate_last fills the last pass; the thresholded variant fills vectors the threshold removed
    u, _, _, counts, validation_counts, details = pd.restated("validation_last")
    assert validation_counts[1, 0] >= 1 and validation_counts[1, 1] >= 1 and np.isnan(details[1][0]["raw"][0]).sum() > np.isnan(u[0]).sum()
    _, _, corr, counts, _, details = pd.restated("validation_thresholded")
    thresholded = np.isnan(details[1][0]["raw"][0]) & (corr[0] < pd.case("validation_thresholded")["min_correlation"])
    assert counts[1, 2] >= thresholded.sum() >= 1 and (details[1][0]["validation"]["action"][thresholded] == pd.FILLED).any()


# RMS error of the last pass against the true displacement at the window centres, as measured with the restatement
# (pixels): 0.28526 and 0.11692 on the shift, 0.08965 and 0.06543 on the shear.  The shear's gain depends on how fine the texture is:
# measured at a shortest period of 16, 10.7, 8, 6.4 and 5.3 pixels (the case's) it is 0.178 -> 0.176, 0.160 -> 0.115, 0.116 -> 0.100,
# 0.103 -> 0.107 (a loss) and 0.090 -> 0.065: windows of 10 and 12 pixels hold too little of a coarse texture for either path.
RMS = dict(three_pass=(0.2853, 0.1169), shear=(0.0897, 0.0654))                      # name: (integer offsets, deformation)


def truth(name, y):
    if name == "shear":
        return pd.SHEAR * (y - pd.SHEAR_ROW), 0.0 * y
    return pd.SHIFT[1] + 0.0 * y, pd.SHIFT[0] + 0.0 * y


@pytest.mark.parametrize("name", sorted(RMS))
def test_deformation_is_more_accurate(name):
    """Deformation has the smaller RMS error, by at least half the improvement measured (RMS)."""
    from opticalflow_amd import optical_flow as of
    c = pd.case(name)
    y = of.piv_grid(c["movie"].shape, c["window_sizes"], c["search_radii"], c["steps"])[-1]["y"]
    true_u, true_v = truth(name, y)
    rms = []
    for deformation in (False, True):
        u, v = pd.restated(name, deformation=deformation)[:2]
        rms.append(float(np.sqrt(np.mean((u[0] - true_u) ** 2 + (v[0] - true_v) ** 2))))
    print(name, "RMS error with integer offsets", rms[0], "with deformation", rms[1])
    assert rms[0] - rms[1] >= 0.5 * (RMS[name][0] - RMS[name][1]) > 0


@pytest.mark.parametrize("arguments", [
    dict(outlier_threshold=0.0), dict(outlier_threshold=-1.0), dict(outlier_threshold=float("inf")), dict(outlier_threshold=float("nan")),
    dict(outlier_threshold="two"), dict(outlier_threshold=True), dict(outlier_threshold=2.0, outlier_epsilon=-0.1),
    dict(outlier_threshold=2.0, outlier_epsilon=float("inf")), dict(outlier_threshold=2.0, outlier_epsilon=float("nan")),
    dict(outlier_threshold=2.0, outlier_epsilon=None), dict(outlier_epsilon=-1.0), dict(deformation=1), dict(deformation="yes"), dict(deformation=None),
    dict(outlier_threshold=2.0, validate_last=1), dict(validate_last=True), dict(validate_last=None)])
def test_value_errors_before_the_library_is_touched(arguments, monkeypatch):
    from opticalflow_amd import _native, optical_flow as of

    def untouched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "Solver", untouched)
    movie = np.zeros((2, 40, 40))
    with pytest.raises(ValueError):
        of.conduct_piv(movie, (8, 8), (2, 2), **arguments)
    with pytest.raises(ValueError):
        of.conduct_piv_flow(movie, window_sizes=(8, 8), search_radii=(2, 2), **arguments)


def test_accepted_options_reach_the_library(monkeypatch):
    """What is accepted gets as far as the library: one pass with deformation, every valid spelling of the options."""
    from opticalflow_amd import _native, optical_flow as of

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached
    monkeypatch.setattr(_native, "Solver", reached)
    for arguments in (dict(deformation=True), dict(outlier_threshold=2), dict(outlier_threshold=1.5, outlier_epsilon=0, validate_last=True),
                      dict(deformation=np.True_, outlier_threshold=np.float32(2.0))):
        with pytest.raises(Reached):
            of.conduct_piv(np.zeros((2, 40, 40)), (8,), (2,), **arguments)
