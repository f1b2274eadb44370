"""CPU tests of conduct_opencv_flow: the host plan (farneback_plan) against the numpy restatement bit for bit, the table
identities, the level rule, the axis and sign convention (on the restatement) and the argument checks that need no device."""
import numpy as np
import pytest

import farneback_restatement as R
from farneback_cases import case_arguments, case_input, texture

PLANS = [(75, 91, 0.5, 3, 15, 5, 1.1), (40, 52, 0.5, 5, 9, 5, 1.1), (128, 160, 0.7, 2, 51, 7, 1.5), (64, 80, 0.5, 0, 1, 5, 0.0),
         (1024, 1024, 0.5, 5, 50, 5, 1.1), (300, 200, 0.8, 9, 129, 10, 10.0), (16, 16, 0.3, 2, 2, 1, 0.5)]


def plan(*a):
    from opticalflow_amd.optical_flow import farneback_plan
    return farneback_plan(*a)


@pytest.mark.parametrize("a", PLANS)
def test_plan_equals_the_restatement(a):
    N_i, N_j, pyr_scale, levels, winsize, poly_n, poly_sigma = a
    p = plan(*a)
    want = R.level_sizes(N_i, N_j, pyr_scale, levels)
    assert p["sizes"] == [(h, w) for h, w, _, _ in want] and p["ksizes"] == [k for _, _, k, _ in want]
    for got, (_, _, ksize, sigma) in zip(p["presmooth_taps"], want):
        assert got.dtype == np.float32 and np.array_equal(got, R.presmooth_taps(ksize, sigma))
    tab = R.poly_tables(poly_n, float(poly_sigma))
    for k in ("g", "xg", "xxg"):
        assert p[k].dtype == np.float32 and np.array_equal(p[k], tab[k]), k
    assert np.array_equal(p["G"], tab["G"]) and np.array_equal(p["invG"], tab["invG"])
    assert (p["ig11"], p["ig03"], p["ig33"], p["ig55"]) == (tab["ig11"], tab["ig03"], tab["ig33"], tab["ig55"])
    assert p["window_taps"].dtype == np.float32 and np.array_equal(p["window_taps"], R.window_taps(winsize))
    assert p["flow_scale"] == np.float32(1.0 / pyr_scale) and isinstance(p["flow_scale"], np.float32)


@pytest.mark.parametrize("a", PLANS)
def test_table_identities(a):
    p = plan(*a)
    k = p["window_taps"].astype(np.float64)
    m = len(k) - 1
    assert m == a[4] // 2 and abs(k[0] + 2 * k[1:].sum() - 1) <= (2 * m + 1) * 2.0 ** -24
    for taps in p["presmooth_taps"]:
        assert len(taps) % 2 == 1 and np.array_equal(taps, taps[::-1]) and abs(taps.astype(np.float64).sum() - 1) <= len(taps) * 2.0 ** -24
    n = a[5]
    assert len(p["g"]) == 2 * n + 1 and np.array_equal(p["xg"], -p["xg"][::-1]) and p["xg"][n] == 0          # xg is odd
    assert np.array_equal(p["g"], p["g"][::-1]) and np.array_equal(p["xxg"], p["xxg"][::-1])
    assert abs(p["g"].astype(np.float64).sum() - 1) <= (2 * n + 1) * 2.0 ** -24
    assert np.abs(p["G"] @ p["invG"] - np.eye(6)).max() <= 1e-12


def test_level_rule():
    assert plan(75, 91, 0.5, 3, 9, 5, 1.1)["sizes"] == [(75, 91), (38, 46)]         # 37.5 and 45.5: ties to even; 75 / 4 < 32 ends it
    assert plan(40, 52, 0.5, 5, 9, 5, 1.1)["sizes"] == [(40, 52)]                   # no extra level
    three = plan(128, 160, 0.7, 2, 9, 5, 1.1)["sizes"]
    assert len(three) == 3 and three[0] == (128, 160)                               # levels = 2 scalings that fit: three images
    assert len(plan(128, 160, 0.5, 1, 9, 5, 1.1)["sizes"]) == 2                     # levels = 1 gives two
    assert plan(128, 160, 0.5, 0, 9, 5, 1.1)["sizes"] == [(128, 160)]
    assert plan(40, 52, 0.5, 5, 9, 5, 1.1)["presmooth_taps"][0].tolist() == [0.25, 0.5, 0.25]


def test_axis_and_sign_convention():
    """A texture moved by (+0.6 rows, -0.4 columns) per frame: v_x is the displacement along the columns (axis 2), v_y along the
    rows (axis 1).  A check of axis order and sign on the restatement, not an accuracy claim."""
    movie = case_input("translation")
    assert movie.shape == (2, 64, 80)
    r = R.conduct_opencv_flow(movie, **case_arguments("translation"))
    v_x, v_y = np.median(r["v_x"][0, 12:-12, 12:-12]), np.median(r["v_y"][0, 12:-12, 12:-12])
    print(f"median v_x {v_x:.4f} (shift -0.4 columns), median v_y {v_y:.4f} (shift +0.6 rows)")
    assert abs(v_x - (-0.4)) <= 0.5 * 0.4 and abs(v_y - 0.6) <= 0.5 * 0.6
    # the same texture moved the other way round changes both signs
    back = texture(2, 64, 80, (-0.6, 0.4), seed=0)
    r = R.conduct_opencv_flow(back, **case_arguments("translation"))
    assert np.median(r["v_x"][0, 12:-12, 12:-12]) > 0.2 and np.median(r["v_y"][0, 12:-12, 12:-12]) < -0.3


def test_restatement_blurs_the_first_image_only():
    import scipy.ndimage
    movie = case_input("blurred")
    args = case_arguments("blurred")
    blurred = np.stack([scipy.ndimage.gaussian_filter(f, 1.3, mode="nearest", truncate=4.0) for f in movie])
    rec = {}
    mixed = R.conduct_opencv_flow(movie, blurred=blurred, rec=rec, **args)
    assert mixed["original_data"] is blurred and "blurred_data" not in mixed
    for k, pair in enumerate(rec["pairs"]):
        first, second = pair["level_images"][0]
        assert np.array_equal(first, R.resize_linear(R.presmooth(blurred[k].astype(np.float32), pair["presmooth_taps"][0]), 40, 52))
        assert np.array_equal(second, R.resize_linear(R.presmooth(movie[k + 1].astype(np.float32), pair["presmooth_taps"][0]), 40, 52))
    assert not np.array_equal(mixed["v_x"], R.conduct_opencv_flow(movie, **args)["v_x"])
    assert not np.array_equal(mixed["v_x"], R.conduct_opencv_flow(blurred, **args)["v_x"])


def test_restatement_stages():
    """The restatement's own pieces on inputs whose result is known: a constant image stays constant through the blur, the resize
    and the expansion (its first-order and mixed planes vanish), and the flow of two equal images is zero in the interior."""
    img = np.full((40, 52), 7.0, dtype=np.float32)
    assert np.array_equal(R.presmooth(img, R.presmooth_taps(3, 0.0)), img)
    assert np.allclose(R.resize_linear(img, 20, 26), 7.0, rtol=1e-6)
    assert np.array_equal(R.resize_linear(img, 40, 52), img)
    poly = R.poly_exp(img, 5, R.poly_tables(5, 1.1))
    assert poly.shape == (5, 40, 52) and np.abs(poly[:2]).max() < 1e-5 and np.abs(poly[4]).max() < 1e-5
    movie = case_input("smallest")
    same = np.stack([movie[0], movie[0]])
    r = R.conduct_opencv_flow(same, **case_arguments("smallest"))
    # ... away from the last row and column, whose pixels take the outside branch (x1 = w - 1) and feed the windows around them
    assert not r["v_x"][0, :24, :36].any() and not r["v_y"][0, :24, :36].any() and r["v_x"][0, :, -1].any()


def test_errors_that_need_no_device():
    from opticalflow_amd.optical_flow import conduct_opencv_flow
    movie = case_input("smallest")
    args = case_arguments("smallest")
    for name in args:
        with pytest.raises(TypeError, match=name):
            conduct_opencv_flow(movie, **{k: v for k, v in args.items() if k != name})
    with pytest.raises(TypeError, match="box_size"):
        conduct_opencv_flow(movie, box_size=3, **args)
    with pytest.raises(TypeError, match="flags"):
        conduct_opencv_flow(movie, flags=256, **args)
    with pytest.raises(TypeError):
        conduct_opencv_flow(movie, **dict(args, levels=1.5))
    for m in (movie.astype(np.float32), movie.astype(np.uint16), movie.astype(np.int64)):
        with pytest.raises(ValueError, match="cast"):
            conduct_opencv_flow(m, **args)
    for m in (movie[:, :15], movie[:, :, :15], movie[0], movie[:1]):
        with pytest.raises(ValueError):
            conduct_opencv_flow(m, **args)
    for change in (dict(pyr_scale=1.0), dict(pyr_scale=0.0), dict(pyr_scale=-0.5), dict(pyr_scale=float("nan")), dict(levels=-1), dict(winsize=0),
                   dict(winsize=130), dict(iterations=-1), dict(poly_n=0), dict(poly_n=11), dict(poly_sigma=-1.0), dict(poly_sigma=float("inf"))):
        with pytest.raises(ValueError):
            conduct_opencv_flow(movie, **dict(args, **change))
    with pytest.raises(ValueError, match="output"):
        conduct_opencv_flow(movie, output="cupy", **args)


def test_no_cpu_fallback():
    """Without a HIP device the call raises; it never computes on the CPU (with one, it computes there)."""
    import torch
    from opticalflow_amd import _native
    from opticalflow_amd.optical_flow import conduct_opencv_flow
    if torch.cuda.is_available():
        assert np.isfinite(conduct_opencv_flow(case_input("smallest"), **case_arguments("smallest"))["speed"]).all()
        return
    with pytest.raises(_native.VofError):
        conduct_opencv_flow(case_input("smallest"), **case_arguments("smallest"))


def test_exports():
    import opticalflow_amd
    from opticalflow_amd import optical_flow
    assert opticalflow_amd.conduct_opencv_flow is optical_flow.conduct_opencv_flow
    assert "conduct_opencv_flow" in optical_flow.__all__ and "farneback_plan" in optical_flow.__all__
