"""The numpy restatement of conduct_opencv_flow against the real OpenCV, wherever ``cv2`` can be imported (nowhere in this
repository's own environments: the file is skipped there).  The exposed stages - cv2.GaussianBlur and cv2.resize(INTER_LINEAR) on
float32 images - are held to a derived forward bound; for the whole flow the difference is printed and only the level count and
finiteness are asserted: OpenCV's SIMD paths may fuse multiply-adds, so no bound on the iterated flow is fixed here."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import farneback_restatement as R                              # noqa: E402
from farneback_cases import case_arguments, case_input        # noqa: E402

EPS = 2.0 ** -23


def level_image_inputs():
    for name in ("smallest", "two_levels", "three_levels"):
        yield name, case_input(name)[0].astype(np.float32)


def test_gaussian_blur_stage():
    """Each pass sums ksize products: |error| <= ksize * 2^-23 * sum |w| |S| per pass, the second pass carrying the first one's."""
    for name, img in level_image_inputs():
        for _, _, ksize, sigma in R.level_sizes(*img.shape, case_arguments(name)["pyr_scale"], case_arguments(name)["levels"]):
            w = R.presmooth_taps(ksize, sigma)
            got = R.presmooth(img, w)
            want = cv2.GaussianBlur(img, (ksize, ksize), sigma, sigmaY=sigma, borderType=cv2.BORDER_REFLECT_101)
            bound = 2 * ksize * EPS * R.presmooth(np.abs(img), np.abs(w)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - want)
            print(f"{name} ksize {ksize}: max |restatement - cv2.GaussianBlur| = {err.max():.3g} (bound {bound.max():.3g})")
            assert (err <= bound).all()


def test_linear_resize_stage():
    """Two terms per axis: |error| <= 4 * 2^-23 * (bilinear mean of |S|)."""
    for name, img in level_image_inputs():
        for h, w, _, _ in R.level_sizes(*img.shape, case_arguments(name)["pyr_scale"], case_arguments(name)["levels"]):
            got = R.resize_linear(img, h, w)
            want = cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR)
            bound = 4 * EPS * R.resize_linear(np.abs(img), h, w).astype(np.float64)
            err = np.abs(got.astype(np.float64) - want)
            print(f"{name} -> {h} x {w}: max |restatement - cv2.resize| = {err.max():.3g} (bound {bound.max():.3g})")
            assert (err <= bound).all()


@pytest.mark.parametrize("name", ["smallest", "two_levels", "three_levels"])
def test_whole_flow(name):
    movie, args = case_input(name), case_arguments(name)
    ours = R.conduct_opencv_flow(movie, **args)
    for k in range(movie.shape[0] - 1):
        theirs = cv2.calcOpticalFlowFarneback(movie[k], movie[k + 1], None, flags=cv2.OPTFLOW_FARNEBACK_GAUSSIAN, **args)
        assert np.isfinite(theirs).all()
        dx = np.abs(ours["v_x"][k] - theirs[:, :, 0]).max()
        dy = np.abs(ours["v_y"][k] - theirs[:, :, 1]).max()
        print(f"{name} pair {k}: max |restatement - cv2| = {dx:.3g} (v_x), {dy:.3g} (v_y); max |flow| {np.abs(theirs).max():.3g}")


def test_level_count():
    """`levels` scalings that fit give levels + 1 images: where a further level fits the frame, asking for it changes cv2's result,
    and where none fits (40 x 52) it does not."""
    movie, args = case_input("three_levels"), case_arguments("three_levels")
    flows = [cv2.calcOpticalFlowFarneback(movie[0], movie[1], None, flags=cv2.OPTFLOW_FARNEBACK_GAUSSIAN, **dict(args, levels=n)) for n in (0, 1, 2, 3)]
    sizes = [len(R.level_sizes(128, 160, args["pyr_scale"], n)) for n in (0, 1, 2, 3)]
    assert sizes == [1, 2, 3, 4]
    for a, b in zip(flows, flows[1:]):
        assert not np.array_equal(a, b)
    movie, args = case_input("smallest"), case_arguments("smallest")
    one = cv2.calcOpticalFlowFarneback(movie[0], movie[1], None, flags=cv2.OPTFLOW_FARNEBACK_GAUSSIAN, **dict(args, levels=0))
    five = cv2.calcOpticalFlowFarneback(movie[0], movie[1], None, flags=cv2.OPTFLOW_FARNEBACK_GAUSSIAN, **dict(args, levels=5))
    assert np.array_equal(one, five) and np.isfinite(one).all()
