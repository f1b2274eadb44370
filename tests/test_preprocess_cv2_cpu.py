"""The numpy restatement of apply_adaptive_threshold / apply_clahe against the real OpenCV, on the inputs of the GPU tests.
Skipped wherever cv2 cannot be imported - it is not a dependency of this project; until this file has run somewhere, parity
of the restatement (and so of the GPU path) with OpenCV rests on the reading of OpenCV 4's source alone."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import preprocess_restatement as R                      # noqa: E402
from preprocess_cases import CLAHE_CASES, THRESHOLD_CASES, clahe_input, threshold_input    # noqa: E402


@pytest.mark.parametrize("name", ["raw", "blurred", "wide"])
def test_adaptive_threshold_equals_cv2(name):
    movie = threshold_input(name)
    u = R.scale_to_uint8(movie)
    assert np.array_equal(u, np.array(movie / np.max(movie) * 255.0, dtype="uint8"))           # OF.py:330
    for w, t in (THRESHOLD_CASES if name != "wide" else [(151, -5)]):
        want = np.stack([cv2.adaptiveThreshold(f, 1.0, cv2.ADAPTIVE_THRESH_MEAN_C, cv2.THRESH_BINARY, w, t) for f in u]) == 1.0
        assert np.array_equal(R.adaptive_threshold(movie, w, t), want), (w, t)


@pytest.mark.parametrize("case", sorted(CLAHE_CASES))
def test_clahe_equals_cv2(case):
    name, clip_limit, tile_number = CLAHE_CASES[case]
    movie = clahe_input(name)
    converted = movie.astype(np.uint16)                                                        # OF.py:364
    aspect_ratio = movie.shape[2] / movie.shape[1]
    f = cv2.createCLAHE(clipLimit=clip_limit, tileGridSize=(tile_number, round(tile_number * aspect_ratio)))
    want = np.stack([f.apply(frame) for frame in converted]).astype(np.float64)
    assert np.array_equal(R.clahe(movie, clip_limit, tile_number), want)
