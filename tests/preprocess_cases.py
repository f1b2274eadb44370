"""The seeded inputs the preprocessing tests share (tests/test_gpu_preprocess.py against the GPU, tests/test_preprocess_cv2_cpu.py
against the real OpenCV): small frames, each there for one path of the restatement."""
import functools

import numpy as np

THRESHOLD_CASES = [(3, 0.0), (11, 2.5), (11, -5), (53, -0.5), (151, -5), (151, 0.0)]


def blurred(stack, sigma=2):
    from scipy.ndimage import gaussian_filter
    return np.stack([gaussian_filter(f, sigma) for f in stack])


@functools.lru_cache(maxsize=None)
def threshold_input(name):
    """"raw": (3, 37, 53) integers 0 .. 255; "blurred": the same through a Gaussian of sigma 2; "wide": (2, 300, 300) blurred."""
    if name == "wide":
        out = blurred(np.random.default_rng(12).integers(0, 256, (2, 300, 300)).astype(np.float64))
    else:
        out = np.random.default_rng(11).integers(0, 256, (3, 37, 53)).astype(np.float64)
        if name == "blurred":
            out = blurred(out)
    out.setflags(write=False)
    return out


def waves(shape, seed=3, frames=1, scale=1.0):
    """floor(128 + 100 sin(i / 9) cos(j / 7) + N(0, 6)) clipped to 0 .. 255 (times ``scale``): smooth, so tiles differ and clip."""
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    noise = np.random.default_rng(seed).normal(0, 6, (frames,) + tuple(shape))
    return np.clip(np.floor(128 + 100 * np.sin(i / 9) * np.cos(j / 7) + noise), 0, 255) * scale


@functools.lru_cache(maxsize=None)
def clahe_input(name):
    """The movie of a CLAHE case; the cases (movie name, clipLimit, tile_number) are CLAHE_CASES."""
    rng = np.random.default_rng(11)
    if name == "A":
        out = rng.integers(0, 256, (2, 37, 53)).astype(np.float64)
    elif name == "B":
        out = waves((37, 53))
    elif name == "C":
        out = np.concatenate([waves((40, 50), scale=16.0), rng.integers(0, 4096, (1, 40, 50)).astype(np.float64)])
    elif name == "D":
        out = waves((40, 40))
    elif name == "E":
        out = np.full((2, 256, 260), 1234.0)
        out[1, 80:160] = 100.0
        out[1, 160:] = 40000.0
    elif name == "F":
        out = np.full((1, 200, 250), 77.0)
    elif name == "G":
        out = rng.integers(0, 65536, (1, 37, 53)).astype(np.float64)
        out[0, 0, 0], out[0, 36, 52], out[0, 17, 5] = 65535.0, 0.0, 65535.5       # the top bin, bin 0, a fraction that truncates
    else:
        raise KeyError(name)
    out.setflags(write=False)
    return out


CLAHE_CASES = {
    "A": ("A", 50000, 4), "B3000": ("B", 3000, 4), "B1500": ("B", 1500, 4), "B1": ("B", 1, 4), "C": ("C", 3000, 5), "D": ("D", 3000, 4),
    "E": ("E", 1, 1), "F": ("F", 1, 1), "G": ("G", 50000, 4),
}
