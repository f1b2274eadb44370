"""Plain-numpy restatement of correct_intensity_change and intensity_histograms, and the cases their CPU and
GPU tests share.

blur(): scipy.ndimage.gaussian_filter(f, sigma, mode='nearest', truncate=4.0) in the kernels' summation order - per axis, centre tap
first, then k = -r .. -1 as acc += (a + b) * w[k + r], a product and a sum rounded separately, indices clamped to the edge.
correct(): the chain B = blur(movie), D = B - B[ref], E = blur(D), out = Tg - E on whole stacks.  histograms(): np.histogram."""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
GAP_BOUND = 1e-9              # no value may lie this close to an interior edge unless exactly on it

# (shape, smoothing_sigma, filter_size): the scipy cases of tests/test_intensity_cpu.py, seeded integer stacks 0 .. 255
SCIPY_CASES = [((3, 9, 70), 3, 5), ((2, 70, 9), 3, 5), ((4, 37, 131), 3, 7.5), ((3, 33, 65), 1.3, 5), ((3, 40, 200), None, 16)]
# the correction cases of tests/test_gpu_intensity.py at reference_frame 0
GPU_CASES = [((3, 9, 70), 3, 5),         # rows fewer than radius 20; one full 64-lane tile plus 6 columns
             ((2, 70, 9), 3, 5),         # the transpose of the above
             ((4, 37, 131), 3, 7.5),     # two BL_TI row tiles, three BL_TR row tiles, a ragged third column tile
             ((3, 40, 66), 3, 16.3),     # radius 65: the global-memory twins
             ((3, 33, 65), None, 5),     # no first blur
             ((2, 40, 66), None, 16)]    # radius 64 = BL_RMAX: the axis-0 tile takes 80 KiB of LDS, past the default limit
CHUNK_CASE = ((18, 8, 12), 1, 1.5)       # more frames than BLUR_CHUNK and than the library's frames in flight
TARGETS = ("blurred", "original")


def taps(sigma, truncate=4.0):
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def blur_axis(f, w, axis):
    r, n = w.size // 2, f.shape[axis]
    at = np.arange(n)
    acc = f * w[r]
    for k in range(-r, 0):
        a = np.take(f, np.clip(at + k, 0, n - 1), axis=axis)
        b = np.take(f, np.clip(at - k, 0, n - 1), axis=axis)
        acc = acc + (a + b) * w[k + r]
    return acc


def blur(stack, sigma):
    """Every frame of a float64 (T, N_i, N_j) stack: axis 0 of the frame, then axis 1."""
    w = taps(sigma)
    return blur_axis(blur_axis(np.asarray(stack, dtype=np.float64), w, 1), w, 2)


def correct(movie, smoothing_sigma=3, filter_size=5, target="blurred", reference_frame=0):
    """(out, drift) of the chain, float64 stacks."""
    movie = np.asarray(movie, dtype=np.float64)
    B = movie if smoothing_sigma is None else blur(movie, smoothing_sigma)
    D = B - B[reference_frame]
    E = blur(D, filter_size)
    return {"blurred": B, "original": movie}[target] - E, E


def scipy_correct(movie, smoothing_sigma, filter_size, target, reference_frame=0):
    """The same chain made of scipy.ndimage.gaussian_filter calls, frame by frame."""
    from scipy.ndimage import gaussian_filter

    def G(f, s):
        return gaussian_filter(f, s, mode="nearest", truncate=4.0)
    movie = np.asarray(movie, dtype=np.float64)
    first = (lambda f: f) if smoothing_sigma is None else (lambda f: G(f, smoothing_sigma))
    ref = first(movie[reference_frame])
    return np.stack([(first(f) if target == "blurred" else f) - G(first(f) - ref, filter_size) for f in movie])


def integer_stack(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_stack(shape):
    stack = integer_stack(shape, 1800 + sum(shape))
    stack.setflags(write=False)
    return stack


def histograms(F, bins, value_range):
    """(counts, nonfinite) of a float64 stack: np.histogram frame by frame."""
    with np.errstate(invalid="ignore"):
        counts = np.stack([np.histogram(f.ravel(), bins, value_range)[0] for f in F]).astype(np.int64)
    return counts, (~np.isfinite(F)).reshape(F.shape[0], -1).sum(1).astype(np.int64)


def dropped(F, value_range):
    """Per frame, the values np.histogram leaves out: NaN and those outside the range."""
    with np.errstate(invalid="ignore"):
        inside = (F >= value_range[0]) & (F <= value_range[1])
    return (~inside).reshape(F.shape[0], -1).sum(1)


def edge_gap(F, bins, value_range):
    """The smallest non-zero distance of a finite value in range to an interior edge (inf if there is none)."""
    edges = np.linspace(value_range[0], value_range[1], bins + 1)[1:-1]
    v = F[np.isfinite(F)].ravel()
    v = v[(v >= value_range[0]) & (v <= value_range[1])]
    if edges.size == 0 or v.size == 0:
        return np.inf
    at = np.clip(np.searchsorted(edges, v), 1, max(edges.size - 1, 1))
    lo, hi = edges[at - 1], edges[np.minimum(at, edges.size - 1)]
    d = np.minimum(np.abs(v - lo), np.abs(v - hi))
    d = d[d > 0]
    return float(d.min()) if d.size else np.inf
