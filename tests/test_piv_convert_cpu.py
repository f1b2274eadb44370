"""CPU tests of convert_PIV_result / upsample_PIV_vectors: the restatement the kernels are held to (tests/piv_restatement.py) against
scipy, the Python entry's unpacking against the reference's own dictionary (tests/golden/g19_piv_convert.npz), and the argument
checks.  No GPU: where the entry's dense part is needed it is computed by the restatement.

The restatement differs from scipy.interpolate.griddata(..., method='cubic') in two respects only: the triangle taken for a pixel
on a shared edge or vertex (the lowest index instead of the end of scipy's walk) and products instead of pow for the cubes.  With
scipy's own triangle and the C library's pow it gives scipy's bits on every value of every case (test_formulas_give_scipys_bits).
Measured on the case list below, max |restatement - griddata| / max |v| per case: odd_grid 5.3e-16, scattered 2.8e-16,
several_blocks 2.7e-16, half_pixel 4.0e-16 (max |v| 6.4 .. 6.8), and 5.6e-16 between the entry and the reference's own dictionary
on the golden fixture; the NaN pattern identical everywhere.  The bound asserted is 4 x the largest, MEASURED = 5.6e-16: the
difference is a few roundings whose number depends on the triangle, anything larger is a formula error."""
import numpy as np
import pytest

import piv_restatement as pr
from conftest import load_golden
from opticalflow_amd import optical_flow as of
from opticalflow_amd.optical_flow import convert_PIV_result, upsample_PIV_vectors

MEASURED = 5.6e-16
BOUND = 4 * MEASURED


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def relative_difference(got, want):
    scale = max(np.nanmax(np.abs(want[0])), np.nanmax(np.abs(want[1])))
    return max(np.nanmax(np.abs(g - w)) for g, w in zip(got[:3], want[:3])) / scale


@pytest.mark.parametrize("name", pr.CASES)
def test_nan_pattern_is_griddatas(name):
    got, want = pr.restated(name), pr.gridded(name)
    for g, w in zip(got[:3], want):
        assert np.array_equal(np.isnan(g), np.isnan(w))
    assert got[3][0] == np.isnan(want[0]).sum() > 0 and got[3][1] == 0


@pytest.mark.parametrize("name", pr.CASES)
def test_values_agree_with_griddata(name):
    rel = relative_difference(pr.restated(name), pr.gridded(name))
    print(name, "max |restatement - griddata| / max |v| =", rel)
    assert rel <= BOUND


@pytest.mark.parametrize("name", pr.CASES)
def test_formulas_give_scipys_bits(name):
    """scipy's own find_simplex choice and pow for the cubes: every value equals griddata's bit for bit."""
    shape, want = pr.case(name)["shape"], pr.gridded(name)
    qx, qy = pr.targets(shape)
    for k, (tri, values, grad) in enumerate(pr.frame_list(name)):
        simplex = tri.find_simplex(np.stack([qx.ravel(), qy.ravel()], axis=1))
        got = pr.evaluate(tri, values, grad, shape, simplex=simplex, powers="pow")
        for comp in range(2):
            assert np.array_equal(got[comp], want[comp][k], equal_nan=True), (k, comp)


@pytest.mark.parametrize("name", pr.CASES)
def test_input_conditions(name):
    """No inclusion decision hangs on the last bits: no barycentric coordinate of a pixel with respect to any triangle lies in
    (-1e-9, -eps) or (1 + eps, 1 + 1e-9); and no triangulation has a degenerate simplex."""
    for tri, _, _ in pr.frame_list(name):
        assert not np.isnan(tri.transform).any()
        assert not pr.locate(tri, pr.case(name)["shape"])[1]


def test_reuse_is_what_a_fresh_triangulation_gives():
    """Frames 1 and 2 of odd_grid share locations and mask: piv_tables keeps the triangulation, and its tables are those of one made
    per frame; triangle counts differ between the other frames."""
    c = pr.case("odd_grid")
    tables = of.piv_tables(c["x"], c["y"], c["vx"], c["vy"])
    frames = pr.frame_list("odd_grid")
    assert not tables["host_frames"]
    assert list(np.diff(tables["triangle_offsets"])) == [len(tri.simplices) for tri, _, _ in frames]
    assert len(set(np.diff(tables["triangle_offsets"]))) == 3
    assert np.array_equal(tables["simplices"], np.concatenate([tri.simplices.ravel() for tri, _, _ in frames]))
    assert np.array_equal(tables["neighbours"], np.concatenate([tri.neighbors.ravel() for tri, _, _ in frames]))
    assert same_bits(tables["transforms"], np.concatenate([tri.transform.ravel() for tri, _, _ in frames]))
    assert same_bits(tables["gradients"], np.concatenate([grad.ravel() for _, _, grad in frames]))
    assert same_bits(tables["values"], np.concatenate([values.ravel() for _, values, _ in frames]))


def restated_upsample(x, y, vx, vy, shape, *, device=0, output="numpy"):
    return pr.upsample(x, y, vx, vy, shape)[:3]


def test_entry_reproduces_the_reference(monkeypatch):
    """Keys, shapes, the PIV_* arrays and the locations bit for bit; the fields (computed by the restatement) within the bound."""
    g = load_golden("g19_piv_convert.npz")
    monkeypatch.setattr(of, "upsample_PIV_vectors", restated_upsample)
    movie = g["movie"]
    boxed = pr.pivlab_result(g["x"], g["y"], g["u_original"], g["v_original"])
    plain = {k: [np.array(a) for a in g[k]] for k in of.PIV_KEYS}
    for PIV_result in (boxed, plain):
        res = convert_PIV_result(PIV_result, movie, float(g["kw_delta_x"]), float(g["kw_delta_t"]))
        assert sorted(res) == sorted([k[4:] for k in g if k.startswith("out_")] + ["original_data"])
        assert res["original_data"] is movie
        assert res["delta_x"] == g["out_delta_x"] and res["delta_t"] == g["out_delta_t"]
        for key in ("x_locations", "y_locations", "PIV_v_x", "PIV_v_y"):
            assert res[key].shape == (3, 7, 7)
            assert np.array_equal(res[key].view(np.uint64), g["out_" + key].view(np.uint64)), key
        fields = [res[k] for k in ("v_x", "v_y", "speed")]
        want = [g["out_" + k] for k in ("v_x", "v_y", "speed")]
        for f, w in zip(fields, want):
            assert f.shape == w.shape == (2, 40, 40) and f.dtype == np.float64
            assert np.array_equal(np.isnan(f), np.isnan(w))
        rel = relative_difference(fields, want)
        print("golden: max |entry - reference| / max |v| =", rel)
        assert rel <= BOUND


def test_scaling_quirk_is_kept(monkeypatch):
    """delta_x = 0.5, delta_t = 2: locations x delta_x, vectors x delta_x / delta_t, targets still the pixel indices."""
    seen = {}

    def spy(x, y, vx, vy, shape, **kw):
        seen.update(x=x, y=y, vx=vx, vy=vy, shape=tuple(shape))
        return (np.zeros((len(x),) + tuple(shape)),) * 3
    monkeypatch.setattr(of, "upsample_PIV_vectors", spy)
    c = pr.case("odd_grid")
    res = convert_PIV_result(pr.pivlab_result(c["x"], c["y"], c["vx"], c["vy"]), np.zeros((4, 37, 53)), 0.5, 2)
    assert seen["shape"] == (37, 53) and len(seen["x"]) == 3 and res["x_locations"].shape == (4, 6, 9)
    assert same_bits(seen["x"], c["x"][:3] * 0.5) and same_bits(seen["y"], c["y"][:3] * 0.5)
    assert np.array_equal(seen["vx"], c["vx"][:3] * 0.5 / 2, equal_nan=True) and np.array_equal(res["PIV_v_y"], c["vy"] * 0.5 / 2, equal_nan=True)
    assert same_bits(pr.case("half_pixel")["x"], c["x"][:2] * 0.5)


def test_argument_errors():
    c = pr.case("odd_grid")
    PIV = pr.pivlab_result(c["x"], c["y"], c["vx"], c["vy"])
    with pytest.raises(ValueError, match="holds 4 frames, the movie needs 5"):
        convert_PIV_result(PIV, np.zeros((6, 37, 53)))
    with pytest.raises(ValueError, match="output must be"):
        convert_PIV_result(PIV, np.zeros((5, 37, 53)), output="cupy")
    with pytest.raises(ValueError, match="3-D"):
        convert_PIV_result(PIV, np.zeros((37, 53)))
    with pytest.raises(ValueError, match="one 2-D array per frame"):
        convert_PIV_result({k: v for k, v in PIV.items() if k != "y"}, np.zeros((5, 37, 53)))
    with pytest.raises(ValueError, match="same number of frames"):
        convert_PIV_result(dict(PIV, u_original=PIV["u_original"][:3]), np.zeros((3, 37, 53)))
    with pytest.raises(ValueError, match="output must be"):
        upsample_PIV_vectors(c["x"], c["y"], c["vx"], c["vy"], (37, 53), output="cupy")
    with pytest.raises(ValueError, match="one common shape"):
        upsample_PIV_vectors(c["x"], c["y"][:, :5], c["vx"], c["vy"], (37, 53))
    with pytest.raises(ValueError, match=r"\(F, R, C\)"):
        upsample_PIV_vectors(c["x"][0], c["y"][0], c["vx"][0], c["vy"][0], (37, 53))
    for shape in ((37,), (37, 53, 2), (37.5, 53), (3, 53), "ab"):
        with pytest.raises(ValueError, match="shape must be"):
            upsample_PIV_vectors(c["x"], c["y"], c["vx"], c["vy"], shape)
