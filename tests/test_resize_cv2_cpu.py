"""The numpy restatement of downsample_movie against the real OpenCV, on every input of the GPU tests.  It settles the two
points of the specification that rest on memory of OpenCV's source - the unrolled float64 summation order of the fast path and
its float32 reciprocal of the area - wherever ``cv2`` can be imported; where it cannot, this file is skipped and the
restatement alone is the bar."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import resize_restatement as R                                  # noqa: E402
from resize_cases import CASES, case_input                       # noqa: E402


@pytest.mark.parametrize("depth", ["u8", "f64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_cv2(name, depth):
    movie = case_input(name, depth)
    n_i, n_j = CASES[name][1]
    want = np.zeros((movie.shape[0], n_i, n_j))
    for k, frame in enumerate(movie):
        want[k] = cv2.resize(frame, dsize=(n_j, n_i), interpolation=cv2.INTER_AREA)
    assert np.array_equal(R.resize_area(movie, n_i, n_j), want)
