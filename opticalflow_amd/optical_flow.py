"""Drop-in for the hot path of the reference module ``source/optical_flow.py``.

``variational_optical_flow`` keeps the reference's signature and result dictionary
(source/optical_flow.py:715-724, 1193-1205) so that ``analysis/analyse_variational_optical_flow.py``
can call it unchanged; the per-pair scipy.sparse assembly + PETSc KSP solve (OF.py:833-1145) is
replaced by the batched HIP solver in ``csrc/`` (BiCGStab + geometric multigrid).
The solve always runs on an MI355X through libvof.so; there is no CPU path in this module.
"""
from __future__ import annotations

import atexit
import contextlib
import threading
import time

import numpy as np

from . import _native

# ---------------------------------------------------------------------------------------------------------
# One native context (device workspace) is kept between calls: creating / destroying tens of GB of device memory costs
# 0.15-1.9 s per call, more than the solve of a whole stack.  It is re-used when the image size and the device match and
# its batch is large enough, replaced otherwise, and released by ``release_device_memory()`` or at interpreter exit.
# A context serves one thread at a time: a second thread calling concurrently gets a private, short-lived context.
# ---------------------------------------------------------------------------------------------------------
_cache_lock = threading.Lock()
_cache = {"key": None, "solver": None}


@contextlib.contextmanager
def _device_context(n_i, n_j, pairs, device, exact=False):
    device = int(device)
    if not _cache_lock.acquire(blocking=False):
        with _native.Solver(n_i, n_j, pairs, device=device) as solver:
            yield solver
        return
    try:
        solver = _cache["solver"]
        # exact: the caller asked for this batch size (max_pairs_in_flight): honour it instead of a larger cached batch
        if (solver is None or not solver.h or _cache["key"] != (n_i, n_j, device) or solver.max_pairs < pairs
                or (exact and solver.max_pairs != pairs)):
            release_device_memory(_locked=True)
            solver = _native.Solver(n_i, n_j, pairs, device=device)
            _cache["key"], _cache["solver"] = (n_i, n_j, device), solver
        try:
            yield solver
        except BaseException:
            release_device_memory(_locked=True)      # do not keep a context whose call failed half-way
            raise
    finally:
        _cache_lock.release()


def release_device_memory(_locked=False):
    """Free the device workspace kept between calls (it is re-created on the next call)."""
    if not _locked:
        with _cache_lock:
            return release_device_memory(_locked=True)
    if _cache["solver"] is not None:
        _cache["solver"].close()
    _cache["key"], _cache["solver"] = None, None


atexit.register(release_device_memory)

__all__ = ["variational_optical_flow", "conduct_optical_flow", "conduct_optical_flow_jit", "liu_shen_optical_flow_jit",
           "conduct_variational_optical_flow_deprecated", "vary_regularisation", "vary_boxsize", "vary_blursize", "compare_channel_flows", "make_fake_data_frame", "blur_movie",
           "compare_flow_results", "filter_PIV_flow_result", "convert_PIV_result", "upsample_PIV_vectors", "piv_tables", "conduct_piv", "conduct_piv_flow", "piv_grid", "correct_intensity_change", "intensity_histograms",
           "apply_adaptive_threshold", "apply_clahe", "downsample_movie", "conduct_opencv_flow", "farneback_plan",
           "calcOpticalFlowFarneback", "OPTFLOW_USE_INITIAL_FLOW", "OPTFLOW_FARNEBACK_GAUSSIAN",
           "format_elapsed_time", "apply_constant_boundary_condition", "choose_pairs_in_flight",
           "subsample_velocities_for_visualisation", "costum_imshow", "make_velocity_overlay_movie",
           "make_joint_overlay_movie", "release_device_memory"]


def make_fake_data_frame(x_position, y_position, sigma=1.0, width=20.0, include_noise=False, dimension=1000):
    """Synthetic Gaussian-hat frame, same arguments and return value as OF.py:376-423:
    ``frame[i, j] = exp((-(x_i - x0)^2 - (y_j - y0)^2) / sigma^2)`` on ``linspace(0, width, dimension)``;
    returns ``(frame, delta_x)``."""
    x = np.linspace(0, width, dimension)
    y = np.linspace(0, width, dimension)
    frame = np.exp((-(x[:, None] - x_position) ** 2 - (y[None, :] - y_position) ** 2) / sigma ** 2)
    delta_x = x[1] - x[0]
    if include_noise:
        frame = np.abs(frame + np.random.rand(dimension, dimension) * 0.0000001)
    return frame, delta_x


def gaussian_taps(sigma, truncate=4.0):
    """The normalised 1-D taps scipy.ndimage.gaussian_filter uses for ``sigma`` (skimage passes truncate=4.0):
    ``radius = int(truncate * sigma + 0.5)``, ``w = exp(-0.5 x^2 / sigma^2) / sum``."""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


# ---------------------------------------------------------------------------------------------------------
# Where the arrays of a call live.  An entry that takes ``output=`` is written once against it: ``_side(output, device)``, the checks,
# a ``_device_context`` and one ``Solver`` method, which takes the _host or the _dev twin of the library by what it is handed.
# ---------------------------------------------------------------------------------------------------------
class _Side:
    def blurred(self, stack, taps, solver):
        """``stack`` (of ``frames``) blurred with ``taps`` through ``solver``, as a new stack."""
        out = self.empty(stack.shape)
        self.wait()
        solver.blur(stack, out, stack.shape[0], taps)
        return out

    def analysed(self, movie, background, solver):
        """The float64 stack ``conduct_optical_flow`` analyses: the movie, less ``background`` if one is given."""
        return self.frames(movie) if background is None else self.subtract_background(movie, background, solver)


class _HostSide(_Side):
    """``output="numpy"``: host arrays, which the library stages."""

    def frames(self, movie):
        """``movie`` as a float64 contiguous array on this side (itself if it is one)."""
        return np.require(np.asarray(movie), np.float64, "C")

    def empty(self, shape, dtype="float64"):
        return np.empty(shape, dtype=dtype)

    def wait(self):
        """The caller's stream is waited for before a native call reads its arrays: nothing to wait for here."""

    def subtract_background(self, movie, background, solver):
        """OF.py:195-198: ``movie - background``, taken in the movie's own dtype as the reference takes it, where the movie blurred with
        sigma 10 exceeds ``background``, zero elsewhere."""
        source = np.asarray(movie)
        threshold = self.blurred(self.frames(source), gaussian_taps(10), solver)
        analysed = np.zeros_like(threshold)
        mask = threshold > background
        analysed[mask] = source[mask] - background
        return analysed

    def untouched(self, movie, frames):
        """``blurred_data`` of a movie nothing was applied to: the caller's own object, as in the reference."""
        return movie

    def box_flow_pairs(self, n_pairs):
        """The pairs a context of the box flow, the sweeps and ``compare_channel_flows`` must hold: the library stages at most the
        context's pairs at a time (at most 8 here); the kernels need no per-pair workspace."""
        return max(1, min(int(n_pairs), 8))


class _DeviceSide(_Side):
    """``output="torch"``: float64 tensors on one device, which torch only allocates, converts and masks.  Nothing else imports torch,
    so a numpy-only call never does."""

    def __init__(self, device):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", int(device))

    def frames(self, movie):
        return self.torch.as_tensor(movie).to(device=self.dev, dtype=self.torch.float64).contiguous()

    def empty(self, shape, dtype="float64"):
        return self.torch.empty(tuple(shape), dtype=getattr(self.torch, dtype), device=self.dev)

    def wait(self):
        self.torch.cuda.synchronize(self.dev)            # the library launches on its own stream

    def subtract_background(self, movie, background, solver):
        """The same on the float64 stack (for an integer movie the subtraction is therefore not the host's)."""
        frames = self.frames(movie)
        threshold = self.blurred(frames, gaussian_taps(10), solver)
        return self.torch.where(threshold > background, frames - background, self.torch.zeros_like(frames))

    def untouched(self, movie, frames):
        return frames

    def box_flow_pairs(self, n_pairs):
        return 1


def _side(output, device):
    if output == "numpy":
        return _HostSide()
    if output == "torch":
        return _DeviceSide(device)
    raise ValueError("output must be 'numpy' or 'torch'")


def _movie_shape(movie, min_frames=2, min_side=None):
    """``(T, N_i, N_j)`` of a movie - an array, a tensor or anything ``np.asarray`` takes - with the checks the entries share, made
    before the library is touched: three axes, ``min_frames`` frames (0: any number) and, for the preprocessing calls, ``min_side``."""
    shape = tuple(movie.shape) if hasattr(movie, "shape") else np.asarray(movie).shape
    if len(shape) != 3:
        raise ValueError("movie must be a 3-D array (frames, x, y)")
    if min_side is not None and (shape[0] < min_frames or min(shape[1:]) < min_side):
        raise ValueError(f"movie needs at least one frame of at least {min_side}x{min_side} pixels")
    if shape[0] < min_frames:
        raise ValueError("movie needs at least two frames")
    return shape


FARNEBACK_ARGUMENTS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma")
FARNEBACK_MIN_SIDE = 16
FARNEBACK_MAX_WINSIZE = 129          # FB_MAX_WINSIZE of csrc/vof_farneback.hpp: a row segment and its two margins live in LDS
FARNEBACK_MAX_POLY_N = 10            # FB_MAX_POLY_N
FARNEBACK_WINDOWS = ("gaussian", "box")
OPTFLOW_USE_INITIAL_FLOW = 4         # cv2's flag bits
OPTFLOW_FARNEBACK_GAUSSIAN = 256


def _f32(value):
    """A Python float rounded to float32 (and back: every float32 is a float)."""
    return float(np.float32(value))


def _left_to_right_sum(values):
    total = 0.0
    for v in values:
        total += v
    return total


def _half_even(value):
    """OpenCV's cvRound: to the nearest integer, ties to the even one - Python's round."""
    return int(round(value))


def farneback_plan(N_i, N_j, pyr_scale, levels, winsize, poly_n, poly_sigma):
    """Everything ``cv2.calcOpticalFlowFarneback(..., flags=OPTFLOW_FARNEBACK_GAUSSIAN)`` derives from its arguments before it
    touches a pixel, for frames of ``N_i`` x ``N_j``.  The native call takes these tables as arrays and
    evaluates no ``exp`` itself; here every ``exp`` is ``math.exp`` of a Python float.  A dict:

    ``sizes``           ``(height, width)`` of the pyramid's images, finest first: ``scale`` is multiplied by ``pyr_scale`` up to
                        ``levels`` times and the loop stops as soon as a side times ``scale`` falls below 32; the ``k`` it has
                        reached is the coarsest image, so ``levels`` scalings that all fit give ``levels + 1`` images
    ``ksizes``, ``presmooth_taps``   per image the tap count ``max(cvRound(5 sigma) | 1, 3)`` with ``sigma = (1 / scale_k - 1) / 2``
                        and the float32 taps of the Gaussian blur applied to the frame before it is resized to that image
                        (``[0.25, 0.5, 0.25]`` at level 0)
    ``g, xg, xxg``      the float32 tables of the polynomial expansion for the offsets ``-poly_n .. poly_n`` (``sigma = 0.3 poly_n``
                        where ``poly_sigma < FLT_EPSILON``); ``G``, ``invG`` the 6 x 6 moment matrix and its inverse in float64,
                        ``ig11, ig03, ig33, ig55`` the four entries of the inverse that are used
    ``window_taps``     the ``winsize // 2 + 1`` float32 taps ``k[0 ..]`` of the Gaussian window (``sigma = 0.3 (winsize // 2)``)
    ``flow_scale``      ``float32(1 / pyr_scale)``, applied to the flow carried from an image to the next finer one
    and ``winsize``, ``poly_n`` as given."""
    import math
    pyr_scale, poly_sigma = float(pyr_scale), float(poly_sigma)
    scale, coarsest = 1.0, 0
    while coarsest < levels:
        scale *= pyr_scale
        if N_j * scale < 32 or N_i * scale < 32:
            break
        coarsest += 1
    sizes, ksizes, presmooth = [], [], []
    for k in range(coarsest + 1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        ksize = max(_half_even(sigma * 5) | 1, 3)
        if ksize == 3 and sigma <= 0:
            taps = [0.25, 0.5, 0.25]
        else:
            scale2x = -0.5 / (sigma * sigma)
            raw = []
            for i in range(ksize):
                x = i - (ksize - 1) * 0.5
                raw.append(math.exp(scale2x * x * x))
            norm = 1.0 / _left_to_right_sum(raw)
            taps = [t * norm for t in raw]
        sizes.append((_half_even(N_i * scale), _half_even(N_j * scale)))
        ksizes.append(ksize)
        presmooth.append(np.array(taps, dtype=np.float64).astype(np.float32))
    n = int(poly_n)
    sigma = n * 0.3 if poly_sigma < float(np.finfo(np.float32).eps) else poly_sigma
    offsets = list(range(-n, n + 1))
    g = [_f32(math.exp(-x * x / (2 * sigma * sigma))) for x in offsets]
    norm = 1.0 / _left_to_right_sum(g)
    g = [_f32(v * norm) for v in g]
    xg = [_f32(x * v) for x, v in zip(offsets, g)]
    xxg = [_f32(x * x * v) for x, v in zip(offsets, g)]
    G00 = G11 = G33 = G55 = 0.0
    for y, gy in zip(offsets, g):
        for x, gx in zip(offsets, g):
            gg = gy * gx
            G00 += gg
            G11 += gg * x * x
            G33 += gg * x * x * x * x
            G55 += gg * x * x * y * y
    G = np.zeros((6, 6), dtype=np.float64)
    G[0, 0] = G00
    for at in ((1, 1), (2, 2), (0, 3), (0, 4), (3, 0), (4, 0)):
        G[at] = G11
    G[3, 3] = G[4, 4] = G33
    G[3, 4] = G[4, 3] = G[5, 5] = G55
    invG = np.linalg.inv(G)
    m = int(winsize) // 2
    sigma = m * 0.3
    window = [1.0] + [_f32(math.exp(-i * i / (2 * sigma * sigma))) for i in range(1, m + 1)]
    total = 1.0
    for v in window[1:]:
        total += v * 2
    norm = 1.0 / total
    window = [v * norm for v in window]
    as_f32 = lambda values: np.array(values, dtype=np.float64).astype(np.float32)
    return dict(sizes=sizes, ksizes=ksizes, presmooth_taps=presmooth, g=as_f32(g), xg=as_f32(xg), xxg=as_f32(xxg), G=G, invG=invG,
                ig11=float(invG[1, 1]), ig03=float(invG[0, 3]), ig33=float(invG[3, 3]), ig55=float(invG[5, 5]),
                window_taps=as_f32(window), flow_scale=np.float32(1.0 / pyr_scale), winsize=int(winsize), poly_n=n)


def _farneback_arguments(shape, kwargs):
    """The six OpenCV arguments of ``conduct_opencv_flow`` checked as ``cv2`` checks their names (``TypeError``) and against the
    limits of this build (``ValueError``), before the library is touched."""
    if "flags" in kwargs:
        raise TypeError("conduct_opencv_flow() passes flags=cv2.OPTFLOW_FARNEBACK_GAUSSIAN itself, as the reference does: "
                        "got multiple values for argument 'flags'")
    unknown = sorted(set(kwargs) - set(FARNEBACK_ARGUMENTS))
    if unknown:
        raise TypeError(f"conduct_opencv_flow() got an unexpected keyword argument {unknown[0]!r}")
    missing = [name for name in FARNEBACK_ARGUMENTS if name not in kwargs]
    if missing:
        raise TypeError(f"conduct_opencv_flow() missing required argument {missing[0]!r} of cv2.calcOpticalFlowFarneback")
    for name in ("levels", "winsize", "iterations", "poly_n"):
        if isinstance(kwargs[name], bool) or int(kwargs[name]) != kwargs[name]:
            raise TypeError(f"{name} must be an integer")
    a = dict(pyr_scale=float(kwargs["pyr_scale"]), levels=int(kwargs["levels"]), winsize=int(kwargs["winsize"]),
             iterations=int(kwargs["iterations"]), poly_n=int(kwargs["poly_n"]), poly_sigma=float(kwargs["poly_sigma"]))
    if shape[1] < FARNEBACK_MIN_SIDE or shape[2] < FARNEBACK_MIN_SIDE:
        raise ValueError(f"frames must be at least {FARNEBACK_MIN_SIDE} x {FARNEBACK_MIN_SIDE} pixels")
    if not 0.0 < a["pyr_scale"] < 1.0:
        raise ValueError("0 < pyr_scale < 1 is required")
    if a["levels"] < 0:
        raise ValueError("levels must be >= 0")
    if not 1 <= a["winsize"] <= FARNEBACK_MAX_WINSIZE:
        raise ValueError(f"winsize must be 1 .. {FARNEBACK_MAX_WINSIZE}")
    if a["iterations"] < 0:
        raise ValueError("iterations must be >= 0")
    if not 1 <= a["poly_n"] <= FARNEBACK_MAX_POLY_N:
        raise ValueError(f"poly_n must be 1 .. {FARNEBACK_MAX_POLY_N}")
    if not np.isfinite(a["poly_sigma"]) or a["poly_sigma"] < 0:
        raise ValueError("poly_sigma must be finite and >= 0")
    return a


def _farneback_window(window, winsize):
    """``window`` checked; True for the box window, whose limits on ``winsize`` are checked too."""
    if window not in FARNEBACK_WINDOWS:
        raise ValueError(f"window must be one of {FARNEBACK_WINDOWS}, not {window!r}")
    if window == "box" and winsize < 2:
        raise ValueError("the box window needs winsize >= 2: at winsize=1 OpenCV's running sums start with row 0 and column 0 counted "
                         "once too often and never lose the surplus, which this build does not restate")
    return window == "box"


def conduct_opencv_flow(movie, delta_x=1.0, delta_t=1.0, smoothing_sigma=None, *, device=0, output="numpy", window="gaussian", **kwargs):
    """Farnebaeck's dense flow of every frame pair on the GPU; positional arguments and the result dict as
    source/optical_flow.py:220-279, which calls ``cv2.calcOpticalFlowFarneback(blurred[k], movie[k + 1], ..., flags=
    cv2.OPTFLOW_FARNEBACK_GAUSSIAN, **kwargs)`` per pair.

    ``kwargs`` are OpenCV's names ``pyr_scale, levels, winsize, iterations, poly_n, poly_sigma``; all six are required, and a
    missing one, an unknown one or ``flags`` is a ``TypeError`` as with ``cv2``.  The reference never asks for
    ``OPTFLOW_USE_INITIAL_FLOW`` - the flow it passes on is an output buffer only - so the pairs are independent and run as one batch.

    Returns ``v_x``, ``v_y``, ``speed`` (float64 ``(T-1, N_i, N_j)``), ``original_data``, ``delta_x`` and ``delta_t``.  The
    reference's quirks are kept: ``v_x`` is OpenCV's channel 0, the displacement **along axis 2** (columns), and ``v_y`` channel 1,
    along axis 1 - unlike every other estimator of the module; with ``smoothing_sigma`` pair ``k`` takes its first image from the
    blurred movie and its second from the unblurred ``movie[k + 1]``, and ``original_data`` is the blurred movie; there is no
    ``blurred_data`` key.  The fields are the float32 flow promoted to float64 and multiplied by ``delta_x / delta_t``;
    ``speed = sqrt(v_x**2 + v_y**2)`` in float64.

    OpenCV's arithmetic is restated operation by operation from OpenCV 4's ``optflowgf.cpp`` (DESIGN.md section 16 has all of
    it and names the points where a real ``cv2`` may differ); parity with an installed ``cv2`` is tested only where one can be
    imported (tests/test_farneback_cv2_cpu.py).  OpenCV converts a frame to float32 first, and that conversion depends on the
    depth, so only the two depths the scripts use are served: **uint8** and **float64** movies; another dtype raises
    ``ValueError``: cast the movie.  ``ValueError`` also for a NaN or Inf in the movie, for frames smaller than 16 x 16 and
    outside ``0 < pyr_scale < 1``, ``levels >= 0``, ``1 <= winsize <= 129``, ``iterations >= 0``, ``1 <= poly_n <= 10``.
    ``output="torch"``: ``movie`` may be a device tensor and every array of the result stays on the device (float64 tensors).

    ``window="box"`` (not in the reference's signature) runs OpenCV's default window instead, the one ``flags=0`` selects: the
    ``2 (winsize // 2) + 1`` box, summed as OpenCV sums it - two running sums in double - and divided by ``winsize**2``;
    it needs ``winsize >= 2``.  Any other value than ``"gaussian"`` or ``"box"`` is a ``ValueError``; ``flags`` stays a ``TypeError``."""
    side = _side(output, device)
    a = _farneback_arguments(_movie_shape(movie, 0), kwargs)
    box = _farneback_window(window, a["winsize"])
    T, N_i, N_j = _movie_shape(movie, 2)
    name = _movie_dtype_name(movie)
    if name not in ("uint8", "float64"):
        raise ValueError(f"conduct_opencv_flow serves uint8 and float64 movies only (OpenCV converts each depth to float32 in its own way), "
                         f"not {name}: cast the movie")
    plan = farneback_plan(N_i, N_j, a["pyr_scale"], a["levels"], a["winsize"], a["poly_n"], a["poly_sigma"])
    frames = side.frames(movie)
    v_x, v_y, speed = (side.empty((T - 1, N_i, N_j)) for _ in range(3))
    with _device_context(N_i, N_j, 1, device) as solver:
        first = frames if smoothing_sigma is None else side.blurred(frames, gaussian_taps(smoothing_sigma), solver)
        side.wait()
        solver.farneback(first[:-1], frames[1:], T - 1, plan, a["iterations"], delta_x / delta_t, v_x, v_y, speed, box=box)
    return dict(v_x=v_x, v_y=v_y, speed=speed, original_data=movie if smoothing_sigma is None else first, delta_x=delta_x, delta_t=delta_t)


def calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags, *, device=0, output="numpy"):
    """``cv2.calcOpticalFlowFarneback`` of one frame pair on the GPU, with ``cv2``'s positional signature: the float32 flow
    ``(N_i, N_j, 2)`` in OpenCV's channel order (channel 0 along the columns, channel 1 along the rows).

    ``flags=0`` is OpenCV's default, the box window (``conduct_opencv_flow(..., window="box")``); ``flags=
    OPTFLOW_FARNEBACK_GAUSSIAN`` (256) is the Gaussian window, the same bits as ``conduct_opencv_flow`` gives.  ``flow`` is
    accepted and ignored: without ``OPTFLOW_USE_INITIAL_FLOW`` it is an output buffer in ``cv2``.  ``OPTFLOW_USE_INITIAL_FLOW`` (4)
    is not built - the reference never passes it - and it or any other bit is a ``ValueError``.

    ``prev`` and ``next`` are 2-D, of equal shape, both uint8 or both float64 (as ``conduct_opencv_flow``: OpenCV converts each
    depth to float32 in its own way).  Limits and error types are those of ``conduct_opencv_flow``; in addition the box window
    needs ``winsize >= 2``.  ``output="torch"``: the frames may be device tensors and the result stays on the device."""
    side = _side(output, device)
    if isinstance(flags, bool) or int(flags) != flags:
        raise TypeError("flags must be an integer")
    flags = int(flags)
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        raise ValueError("OPTFLOW_USE_INITIAL_FLOW is not built: the reference never passes an initial flow")
    if flags & ~OPTFLOW_FARNEBACK_GAUSSIAN:
        raise ValueError(f"flags={flags}: only 0 (the box window) and OPTFLOW_FARNEBACK_GAUSSIAN = 256 are built")
    shapes = [tuple(f.shape) if hasattr(f, "shape") else np.asarray(f).shape for f in (prev, next)]
    if len(shapes[0]) != 2 or shapes[0] != shapes[1]:
        raise ValueError(f"prev and next must be 2-D images of one shape, not {shapes[0]} and {shapes[1]}")
    names = [_movie_dtype_name(f) for f in (prev, next)]
    if names[0] != names[1] or names[0] not in ("uint8", "float64"):
        raise ValueError(f"calcOpticalFlowFarneback serves two uint8 or two float64 frames only (OpenCV converts each depth to float32 "
                         f"in its own way), not {names[0]} and {names[1]}: cast the frames")
    N_i, N_j = shapes[0]
    a = _farneback_arguments((1, N_i, N_j), dict(pyr_scale=pyr_scale, levels=levels, winsize=winsize, iterations=iterations, poly_n=poly_n,
                                                 poly_sigma=poly_sigma))
    box = _farneback_window("gaussian" if flags & OPTFLOW_FARNEBACK_GAUSSIAN else "box", a["winsize"])
    plan = farneback_plan(N_i, N_j, a["pyr_scale"], a["levels"], a["winsize"], a["poly_n"], a["poly_sigma"])
    first, second = (side.frames(f)[None] for f in (prev, next))
    v_x, v_y, speed = (side.empty((1, N_i, N_j)) for _ in range(3))
    with _device_context(N_i, N_j, 1, device) as solver:
        side.wait()
        solver.farneback(first, second, 1, plan, a["iterations"], 1.0, v_x, v_y, speed, box=box)
    flow = side.empty((N_i, N_j, 2), "float32")                             # exact: float32 values promoted, times 1.0
    flow[:, :, 0], flow[:, :, 1] = v_x[0], v_y[0]
    return flow


def blur_movie(movie, smoothing_sigma, device=0, _solver=None):
    """Per-frame Gaussian blur on the GPU, same arguments and result as OF.py:282-306.  The reference calls
    ``skimage.filters.gaussian(frame, sigma, preserve_range=True)``, i.e. ``scipy.ndimage.gaussian_filter(frame,
    sigma, mode='nearest', truncate=4.0)``: two 1-D correlations (axis 0, then axis 1) with clamped edges; the
    HIP kernel keeps scipy's summation order, so the result agrees with the host filter to rounding."""
    movie = np.asarray(movie)
    _movie_shape(movie, 0)
    taps = gaussian_taps(smoothing_sigma)
    frames = np.ascontiguousarray(movie, dtype=np.float64)
    if _solver is not None:
        return _solver.blur_host(frames, taps)
    with _device_context(max(4, movie.shape[1]), max(4, movie.shape[2]), 1, device) as solver:
        if (solver.n_i, solver.n_j) != movie.shape[1:]:
            raise ValueError("frames must be at least 4x4")
        return solver.blur_host(frames, taps)


THRESHOLD_MAX_WINDOW = 4095          # PP_MAX_WINDOW of csrc/vof_preprocess.hpp: 255 * w^2 < 2^32, every window sum fits 32 bits
THRESHOLD_MAX_ROW = 15360            # PP_MAX_ROW: a row's prefix sums live in LDS


def _run_preprocess(movie, shape, device, side, call, dtype="float64", out_shape=None):
    """The frames as float64 on ``side`` and an empty result of ``dtype`` - of the movie's shape unless ``out_shape`` names another -
    through the cached context to ``call(solver, frames, out, T)``, one of the native calls; returns the result."""
    frames = side.frames(movie)
    out = side.empty(out_shape or shape, dtype)
    with _device_context(shape[1], shape[2], 1, device) as solver:
        side.wait()
        call(solver, frames, out, shape[0])
    return out


def apply_adaptive_threshold(movie, window_size=51, threshold=0.0, *, device=0, output="numpy"):
    """OpenCV's adaptive mean threshold of every frame on the GPU; positional arguments and the bool ``(T, N_i, N_j)`` result
    as OF.py:308-338, which calls ``cv2.adaptiveThreshold(frame, 1.0, cv2.ADAPTIVE_THRESH_MEAN_C, cv2.THRESH_BINARY,
    window_size, threshold)`` on ``np.array(movie / np.max(movie) * 255.0, dtype='uint8')`` and compares with 1.

    The movie is read as float64 (a float32 movie is therefore computed in float64).  With ``m`` the maximum of the whole stack:
    ``u = (uint8) trunc((x / m) * 255.0)``; ``S`` the sum of ``u`` over the ``window_size`` x ``window_size`` window centred on the
    pixel, indices outside the image clamped to the edge (BORDER_REPLICATE; the window may be larger than the image);
    ``mean = floor((2 * S + w**2) / (2 * w**2))``, ``S / w**2`` rounded to nearest (``w`` is odd: no tie); result
    ``(u - mean) > -ceil(threshold)``.  All of it is integer arithmetic, restated from OpenCV 4's source; parity with an
    installed ``cv2`` is tested only where one can be imported (tests/test_preprocess_cv2_cpu.py).

    ``window_size`` must be odd and 3 .. 4095 (every window sum then fits 32 bits) and ``N_j <= 15360``: ``ValueError``
    otherwise.  Two deviations from the reference: a stack with a NaN / Inf, a negative value or a maximum ``<= 0`` raises
    ``ValueError`` - the reference's ``uint8`` cast of such values is platform-dependent; and frames smaller than 4 x 4 pixels
    raise ``ValueError`` - the device context serves no smaller image.
    ``output="torch"``: ``movie`` may be a device tensor and the result is a ``torch.bool`` tensor on the device."""
    side = _side(output, device)
    shape = _movie_shape(movie, 1, 4)
    if int(window_size) != window_size or int(window_size) % 2 == 0 or int(window_size) <= 1:
        raise ValueError("window_size must be an odd integer > 1")
    if int(window_size) > THRESHOLD_MAX_WINDOW:
        raise ValueError(f"window_size must be <= {THRESHOLD_MAX_WINDOW}")
    if shape[2] > THRESHOLD_MAX_ROW:
        raise ValueError(f"frames may have {THRESHOLD_MAX_ROW} columns at most")
    if np.isnan(float(threshold)):
        raise ValueError("threshold is NaN")
    w, t = int(window_size), float(threshold)
    return _run_preprocess(movie, shape, device, side, lambda solver, frames, out, T: solver.adaptive_threshold(frames, out, T, w, t), "bool")


def clahe_tile_grid(shape, tile_number):
    """``(tilesX, tilesY)`` the reference hands to ``cv2.createCLAHE`` for a ``(T, N_i, N_j)`` movie (OF.py:365-366):
    ``tilesX = tile_number`` runs along ``N_j`` - OpenCV's ``Size(width, height)`` - and ``tilesY = round(tile_number * N_j /
    N_i)`` along ``N_i``; the mix-up of the axes is the reference's and is kept.  ``ValueError`` unless ``1 <= tilesX <= N_j - 1``
    and ``1 <= tilesY <= N_i - 1`` (the reflected padding needs it)."""
    _T, N_i, N_j = shape
    if int(tile_number) != tile_number:
        raise ValueError("tile_number must be an integer")
    tiles_x = int(tile_number)
    tiles_y = round(tile_number * (N_j / N_i))
    if not (1 <= tiles_x <= N_j - 1 and 1 <= tiles_y <= N_i - 1):
        raise ValueError(f"tile grid {tiles_x} x {tiles_y} does not fit frames of {N_i} x {N_j} pixels: "
                         "1 <= tilesX <= N_j - 1 and 1 <= tilesY <= N_i - 1 are required")
    return tiles_x, tiles_y


def apply_clahe(movie, clipLimit=50000, tile_number=10, *, device=0, output="numpy"):
    """OpenCV's contrast-limited adaptive histogram equalisation of every frame on the GPU; positional arguments and the
    float64 ``(T, N_i, N_j)`` result as OF.py:340-374, which calls ``cv2.createCLAHE(clipLimit, (tile_number,
    round(tile_number * N_j / N_i))).apply`` on ``movie.astype(np.uint16)``.  The reference's ``print(np.max(...))`` is not
    reproduced.

    Per frame, restated from OpenCV 4's ``clahe.cpp`` for 16-bit input (65536 bins): ``v = (uint16) trunc(x)``; the tile grid of
    ``clahe_tile_grid``; if either axis does not divide by its grid, the right side is extended by ``tilesX - N_j % tilesX``
    columns and the bottom by ``tilesY - N_i % tilesY`` rows (BORDER_REFLECT_101) - a dividing axis then receives a full
    ``tiles`` of padding, as in OpenCV; ``clip = max(int(clipLimit * area / 65536), 1)`` for ``clipLimit > 0``, no clipping
    otherwise; per tile the histogram is clipped, the excess is redistributed (``excess // 65536`` to every bin, the rest
    one each to every ``max(65536 // rest, 1)``-th bin) and summed into a uint16 table ``rint(float32(sum) * float32(65535) /
    float32(area))``; every pixel blends the tables of its four neighbouring tiles bilinearly in float32.  Integer up to the
    table, so bit-reproducible; parity with an installed ``cv2`` is tested only where one can be imported.

    ``ValueError`` for a tile grid that does not fit and - the deviations from the reference - for a stack with a NaN / Inf
    or a value outside ``[0, 65536)``, which the reference wraps, and for frames smaller than 4 x 4 pixels, which the device
    context does not serve.  Device memory: ``65536 * 6`` bytes per tile and frame in flight.
    ``output="torch"``: ``movie`` may be a device tensor and the result is a float64 tensor on the device."""
    side = _side(output, device)
    shape = _movie_shape(movie, 1, 4)
    tiles_x, tiles_y = clahe_tile_grid(shape, tile_number)
    if np.isnan(float(clipLimit)):
        raise ValueError("clipLimit is NaN")
    clip = float(clipLimit)
    return _run_preprocess(movie, shape, device, side, lambda solver, frames, out, T: solver.clahe(frames, out, T, clip, tiles_x, tiles_y))


def _movie_dtype_name(movie):
    """'uint8', 'float64', ... of a numpy array, a torch tensor or anything ``np.asarray`` takes."""
    dtype = movie.dtype if hasattr(movie, "dtype") else np.asarray(movie).dtype
    return str(dtype).replace("torch.", "")


def downsample_movie(movie, resolution, *, device=0, output="numpy"):
    """OpenCV's area resize of every frame on the GPU: the loop of the reference's small-grid experiments
    (analyse_variational_optical_flow.py:534-539, 625-630; analyse_short_timeinterval_data.py:754-759),

        for k, frame in enumerate(movie):
            downsampled[k] = cv2.resize(frame, dsize=(resolution, resolution), interpolation=cv2.INTER_AREA)

    with ``downsampled`` a float64 array.  ``movie`` is ``(T, N_i, N_j)``; ``resolution`` is an int ``r`` - the result is
    ``(T, r, r)`` whatever the aspect ratio, as in the scripts - or a pair ``(n_i, n_j)`` of output rows and columns.  The result
    is float64 ``(T, n_i, n_j)``.

    OpenCV's arithmetic depends on the depth of the frame, so the dtype of ``movie`` selects it and only the two depths the
    scripts use are served: **uint8** (float32 sums, or integer block sums where both scales are integers, rounded to
    0 .. 255) and **float64**.  Any other dtype raises ``ValueError``: cast the movie to the depth whose arithmetic is meant.
    Restated from OpenCV 4's ``resize.cpp`` (``resizeArea_`` with the tables of ``computeResizeAreaTab``; ``resizeAreaFast_``
    where ``N / n`` is an integer on both axes, with its half-up rounding of uint8 2 x 2 blocks and its unrolled float64
    sums); DESIGN.md section 15 has every operation.  Parity with an installed ``cv2`` is tested only where one can be
    imported (tests/test_resize_cv2_cpu.py).  A NaN or Inf of a float64 movie propagates as it does in OpenCV.

    ``ValueError`` unless ``1 <= n_i <= N_i`` and ``1 <= n_j <= N_j`` - OpenCV takes another code path as soon as one axis is
    enlarged, and that path is not built - and for frames smaller than 4 x 4 pixels, which the device context does not serve.
    ``output="torch"``: ``movie`` may be a device tensor and the result is a float64 tensor on the device, ready for
    ``variational_optical_flow(..., output="torch")``."""
    side = _side(output, device)
    shape = _movie_shape(movie, 1, 4)
    name = _movie_dtype_name(movie)
    if name not in ("uint8", "float64"):
        raise ValueError(f"downsample_movie serves uint8 and float64 movies only (OpenCV's arithmetic differs by depth), not {name}: "
                         "cast the movie to the depth whose arithmetic is meant")
    pair = resolution if isinstance(resolution, (tuple, list)) else (resolution, resolution)
    if len(pair) != 2 or any(isinstance(r, bool) or int(r) != r for r in pair):
        raise ValueError("resolution must be an integer or a pair (n_i, n_j) of integers")
    n_i, n_j = int(pair[0]), int(pair[1])
    if not (1 <= n_i <= shape[1] and 1 <= n_j <= shape[2]):
        raise ValueError(f"resolution {n_i} x {n_j} does not downsample frames of {shape[1]} x {shape[2]} pixels: "
                         "1 <= n_i <= N_i and 1 <= n_j <= N_j are required")
    arithmetic = _native.RESIZE_U8 if name == "uint8" else _native.RESIZE_F64
    return _run_preprocess(movie, shape, device, side, lambda solver, frames, out, T: solver.resize_area(frames, out, T, n_i, n_j, arithmetic),
                           out_shape=(shape[0], n_i, n_j))


BLUR_MAX_RADIUS = 4096               # the largest tap radius the native blur takes
HISTOGRAM_MAX_BINS = 1 << 20         # IH_MAX_BINS of csrc/vof_intensity.hpp


def _blur_taps(name, sigma):
    """``gaussian_taps(sigma)`` of a positive, finite ``sigma`` whose radius the library serves; ``ValueError`` otherwise."""
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a positive number") from None
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"{name} must be positive and finite")
    if int(4.0 * sigma + 0.5) > BLUR_MAX_RADIUS:
        raise ValueError(f"{name} is too large: the blur's radius int(4 sigma + 0.5) may be {BLUR_MAX_RADIUS} at most")
    return gaussian_taps(sigma)


def correct_intensity_change(movie, smoothing_sigma=3, filter_size=5, *, target="blurred", reference_frame=0, return_drift=False,
                             device=0, output="numpy"):
    """The illumination correction of the reference's real-data scripts on the GPU: what ``correct_intensity_change``
    (analysis/analyse_short_timeinterval_data.py:241-301) and ``visualise_ground_truth_displacement`` (:128-145) do to a movie
    whose overall brightness drifts between frames, before an estimator sees it.

    ``movie`` is ``(T, N_i, N_j)`` with ``T >= 1``, read as float64 like ``blur_movie``.  With ``G(f, s)`` the filter of ``blur_movie``
    - ``scipy.ndimage.gaussian_filter(f, s, mode='nearest', truncate=4.0)``, taps from ``gaussian_taps`` - the arithmetic is, per
    frame ``k``, in this order and nothing else:

    - ``B[k] = G(movie[k], smoothing_sigma)``; with ``smoothing_sigma=None``, ``B = movie``;
    - ``D[k] = B[k] - B[reference_frame]``, one float64 subtraction per pixel;
    - ``E[k] = G(D[k], filter_size)``, the drift;
    - ``out[k] = Tg[k] - E[k]`` with ``Tg = B`` for ``target="blurred"`` and ``Tg = movie`` for ``target="original"``.

    ``target="blurred"`` with the defaults is the reference's ``:250-252`` (sigma 3, filter 5, a two-frame movie);
    ``target="original"`` with ``filter_size=7.5`` its ``:140-144`` (frame 0 kept, frame 1 corrected).  The result is the float64
    ``(T, N_i, N_j)`` stack ``out``; with ``return_drift=True`` it is ``(out, E)``.  The reference frame is no special case: its ``D``
    is ``+0.0`` everywhere and its drift exactly 0, so its output is ``Tg[reference_frame]`` bit for bit.  NaN and Inf propagate through
    the taps as in ``blur_movie``; there is no range check.  The fused passes give the bits of the chain made of ``blur_movie`` and
    numpy subtractions.

    ``reference_frame`` is a Python index in ``-T .. T - 1``.  ``ValueError``, before the library is touched, for a
    ``reference_frame`` outside that, a ``target`` that is neither name, a non-positive or non-finite sigma, a movie that is not
    3-D, frames under 4 x 4 pixels and an unknown ``output``.
    ``output="torch"``: ``movie`` may be a device tensor and the results are float64 tensors on the device, ready for
    ``variational_optical_flow(..., output="torch")``."""
    side = _side(output, device)
    shape = _movie_shape(movie, 1, 4)
    if target not in _native.INTENSITY_TARGETS:
        raise ValueError(f"target must be one of {_native.INTENSITY_TARGETS}")
    try:
        inside = not isinstance(reference_frame, bool) and int(reference_frame) == reference_frame and -shape[0] <= reference_frame < shape[0]
    except (TypeError, ValueError):
        inside = False
    if not inside:
        raise ValueError(f"reference_frame must be an integer in {-shape[0]} .. {shape[0] - 1}")
    reference = int(reference_frame) % shape[0]
    smoothing = None if smoothing_sigma is None else _blur_taps("smoothing_sigma", smoothing_sigma)
    taps = _blur_taps("filter_size", filter_size)
    which = _native.INTENSITY_TARGETS.index(target)
    frames = side.frames(movie)
    out = side.empty(shape)
    drift = side.empty(shape) if return_drift else None
    with _device_context(shape[1], shape[2], 1, device) as solver:
        side.wait()
        solver.intensity_correct(frames, shape[0], smoothing, taps, reference, which, out, drift)
    return (out, drift) if return_drift else out


def intensity_histograms(movie, bins=255, value_range=(0, 255), smoothing_sigma=None, *, device=0, output="numpy"):
    """The per-frame intensity histograms the reference's scripts read their background and intensity thresholds off
    (``investigate_intensities``, analyse_short_timeinterval_data.py:303-335 and compare_rho_and_actin.py:98-118;
    ``investigate_intensity_thresholds``, :198-226; ``make_thresholded_movies``, :281-299) on the GPU.

    Returns a dict: ``counts``, int64 ``(T, bins)``; ``edges``, ``np.linspace(lo, hi, bins + 1)``; ``nonfinite``, int64 ``(T,)``,
    the NaN / Inf values of every frame.  ``counts[k]`` is ``np.histogram(F[k].ravel(), bins, value_range)[0]`` exactly, ``F`` the
    movie (read as float64) or, with ``smoothing_sigma``, ``blur_movie(movie, smoothing_sigma)`` - the same bits, blurred a chunk
    of frames at a time in device scratch and never a stack.  The scripts' whole-movie histogram is ``counts.sum(0)``.  As in
    numpy the bin index is corrected against the edges, the last bin is closed on the right, and NaN and values outside the range
    are dropped.

    ``ValueError`` for ``bins < 1`` (or above 2**20), a range that is not finite or not increasing, a bad sigma, a movie that is
    not 3-D and frames under 4 x 4 pixels.  ``output="torch"``: ``movie`` may be a device tensor, which is read where it lies; the
    three results are small and numpy arrays either way."""
    side = _side(output, device)
    shape = _movie_shape(movie, 1, 4)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= HISTOGRAM_MAX_BINS:
        raise ValueError(f"bins must be an integer in 1 .. {HISTOGRAM_MAX_BINS}")
    if np.ndim(value_range) != 1 or len(value_range) != 2:
        raise ValueError("value_range must be a pair (lo, hi)")
    lo, hi = float(value_range[0]), float(value_range[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("value_range must be finite with lo < hi")
    taps = None if smoothing_sigma is None else _blur_taps("smoothing_sigma", smoothing_sigma)
    edges = np.linspace(lo, hi, int(bins) + 1)
    frames = side.frames(movie)
    with _device_context(shape[1], shape[2], 1, device) as solver:
        side.wait()
        counts, nonfinite = solver.intensity_hist(frames, shape[0], edges, taps)
    return {"counts": counts, "edges": edges, "nonfinite": nonfinite}


def format_elapsed_time(time_difference):
    """(minutes, seconds, milliseconds) of a ``time.time()`` difference, OF.py:1212-1238."""
    minutes = int(time_difference // 60)
    seconds = int(time_difference % 60)
    milliseconds = int((time_difference - int(time_difference)) * 1000)
    return minutes, seconds, milliseconds


def apply_constant_boundary_condition(image):
    """In-place mirror of the border lines (OF.py:1304-1316): rows first, then columns."""
    image[0, :] = image[2, :]
    image[-1, :] = image[-3, :]
    image[:, 0] = image[:, 2]
    image[:, -1] = image[:, -3]


def choose_pairs_in_flight(n_i, n_j, n_pairs, device=0, memory_fraction=0.6, cap=128, params=None, staging=True):
    """Largest batch of frame pairs whose workspace fits in ``memory_fraction`` of the free HBM (``params``: the solver
    parameters of the call - the stencil storage is sized by their ``coarse_precision``)."""
    free, _total = _native.device_memory(device)
    budget = free * memory_fraction
    fmt = (None, None) if params is None else (int(params.coarse_precision), int(params.vcycle_precision))
    per_pair = _native.query_workspace(n_i, n_j, 1, *fmt) + (9 * n_i * n_j * 8 if staging else 0)  # + host-API staging (two output sets)
    return int(max(1, min(n_pairs, cap, budget // max(per_pair, 1))))


def _float64_copy(a, n_threads=4, wait=True):
    """``a.astype(np.float64)`` (always a copy, OF.py:769); stacks of more than 128 MB are converted by a few threads
    (numpy copies release the GIL; the single-threaded copy of a 2 GB movie takes 0.16 s, a sixth of the whole call).
    ``wait=False``: returns ``(out, join)`` with the copy still running - ``join()`` waits for it."""
    if a.ndim < 1 or a.shape[0] < n_threads or a.size < (1 << 24):
        out = a.astype(np.float64)
        return out if wait else (out, lambda: None)
    out = np.empty(a.shape, dtype=np.float64)
    bounds = np.linspace(0, a.shape[0], n_threads + 1).astype(int)

    def work(i0, i1):
        out[i0:i1] = a[i0:i1]
    threads = [threading.Thread(target=work, args=(bounds[k], bounds[k + 1])) for k in range(n_threads)]
    for t in threads:
        t.start()

    def join():
        for t in threads:
            t.join()
    if wait:
        join()
        return out
    return out, join


def _solver_params(speed_alpha, remodelling_alpha, delta_x, delta_t, initial_v_x, initial_v_y, initial_remodelling,
                   use_direct_solver, rtol, max_iterations, reference_quirks, coarse_precision, vcycle_precision,
                   multigrid_sweeps, w_cycle_level, krylov_method="auto", gmres_restart=None, warm_start_stride=None,
                   preconditioner=None):
    """vof_params from the keyword arguments of ``variational_optical_flow``.  ``krylov_method`` may be a tuple
    ``("auto", fallback_after)``: BiCGStab iterations before GMRES takes over."""
    fallback_after = None
    if isinstance(krylov_method, (tuple, list)):
        krylov_method, fallback_after = krylov_method[0], int(krylov_method[1])
    if rtol is None:
        rtol = 1e-10 if use_direct_solver else 1e-6     # direct branch: the accuracy a sparse LU itself attains on these systems
    params = _native.default_params(
        speed_alpha=float(speed_alpha), remodelling_alpha=float(remodelling_alpha), delta_x=float(delta_x),
        delta_t=float(delta_t), initial_v_x=float(initial_v_x), initial_v_y=float(initial_v_y),
        initial_remodelling=float(initial_remodelling), rtol=float(rtol), max_iterations=int(max_iterations),
        reference_quirks=int(bool(reference_quirks)),
        coarse_precision={"float64": 0, "float32": 1, "bfloat16": 2, "float8": 3}[coarse_precision],
        vcycle_precision={"float64": 0, "float32": 1, "auto": 2, "coarse_float32": 3}[vcycle_precision])
    if multigrid_sweeps is not None:     # (pre, post) on level 0 [, (pre, post) on the coarse levels]
        ms = tuple(int(v) for v in multigrid_sweeps)
        params.nu_pre, params.nu_post = ms[0], ms[1]
        if len(ms) == 4:
            params.nu_pre_coarse, params.nu_post_coarse = ms[2], ms[3]
    if w_cycle_level is not None:        # -1: plain V-cycle; l or (l, visits): level l visits level l+1 several times
        if isinstance(w_cycle_level, (tuple, list)):
            params.w_cycle_level, params.w_cycle_visits = int(w_cycle_level[0]), int(w_cycle_level[1])
        else:
            params.w_cycle_level = int(w_cycle_level)
    params.krylov_method = {"bicgstab": 0, "gmres": 1, "auto": 2}[krylov_method]
    if gmres_restart is not None:
        params.gmres_restart = int(gmres_restart)
    if fallback_after is not None:
        params.fallback_after = fallback_after
    if warm_start_stride is not None:
        params.warm_start_stride = int(warm_start_stride)
    if preconditioner is None:           # the reference's direct branch: the direct preconditioner (falls back if it cannot fit)
        preconditioner = "direct" if use_direct_solver else "auto"
    params.preconditioner = {"multigrid": 0, "direct": 1, "auto": 2}[preconditioner]
    return params


def _direct_unavailable(exc):
    """True if a native call failed only because the direct preconditioner cannot be used here (too large for the free
    device memory): ``use_direct_solver=True`` then falls back to the multigrid path at rtol 1e-10."""
    msg = str(exc)
    return "direct preconditioner does not fit" in msg


def variational_optical_flow(movie,
                             delta_x=1.0,
                             delta_t=1.0,
                             speed_alpha=1.0,
                             remodelling_alpha=1000.0,
                             smoothing_sigma=None,
                             initial_v_x=0.0,
                             initial_v_y=0.0,
                             initial_remodelling=0.0,
                             use_direct_solver=False,
                             *,
                             rtol=None,
                             max_iterations=1000,
                             reference_quirks=True,
                             device=0,
                             max_pairs_in_flight=None,
                             coarse_precision="float8",
                             vcycle_precision="coarse_float32",
                             multigrid_sweeps=None,
                             w_cycle_level=None,
                             krylov_method="auto",
                             gmres_restart=None,
                             warm_start_stride=None,
                             preconditioner=None,
                             verbose=False,
                             return_stats=False,
                             output="numpy",
                             _solver=None):
    """Variational optical flow with remodelling on an image stack, on one MI355X.

    Positional/keyword arguments up to ``use_direct_solver`` have the reference's meaning
    (OF.py:725-762).  ``movie`` is ``(T, N_i, N_j)``, any real dtype; the result ``k`` is the flow
    from frame ``k`` to ``k+1``.  Returns the reference's result dict (OF.py:1193-1205): ``v_x``,
    ``v_y``, ``speed``, ``remodelling`` (float64 ``(T-1, N_i, N_j)``), ``original_data``,
    ``blurred_data``, ``delta_x``, ``delta_t``, ``converged`` (flag of the LAST pair, as in the
    reference), ``L1_functional``, ``remodelling_functional``, ``speed_functional``.

    Differences, all opt-in or invisible at the reference's tolerance:
      * all pairs are solved concurrently instead of warm-starting pair k from pair k-1 (OF.py:803-806): from the same
        constant initial guess, or (device-resident mode, large stacks) every 3rd pair first and the others from their
        solved neighbour; the converged answer is the same to solver tolerance;
      * ``use_direct_solver=True`` (SuperLU in the reference, OF.py:1146-1147) selects the direct preconditioner - a
        block-tridiagonal LU of the system by image rows on the GPU - inside the same Krylov iteration, converged to
        rtol=1e-10 (one or two iterations); if its buffers (``n_i (3 n_j)^2`` doubles per pair) do not fit, the multigrid
        path is run to rtol=1e-10 instead;
      * keyword-only extras: ``rtol`` (default 1e-6 = OF.py:1120), ``max_iterations`` (1000),
        ``reference_quirks`` (True keeps OF.py:698-699 'dy'=='dx' and the OF.py:1205
        ``speed_functional`` assignment), ``device``, ``max_pairs_in_flight``, ``coarse_precision`` (storage of the Galerkin
        stencils of the multigrid preconditioner: "float8" (default: 8-bit float off-diagonal blocks whose rounding errors
        are folded into a float32 diagonal block, so block row sums are exact - 1 % more iterations than "float32" on a third
        of the bytes), "bfloat16" (the same with 16-bit off-diagonal blocks: iteration counts of "float32"), "float32",
        "float64") / ``vcycle_precision`` (storage of the V-cycle vectors: "coarse_float32" (default: float64 on
        level 0, float32 on the coarser levels), "float64", "float32" or "auto" = float32; the float32 modes return to
        float64 for pairs that need more than 8 iterations; all arithmetic, the Krylov iteration, the stopping rule and the
        result are float64 either way), ``multigrid_sweeps``
        (block-GS sweeps per V-cycle: ``(pre, post)`` on level 0 and optionally ``(pre, post)`` on the coarse levels),
        ``w_cycle_level`` (-1: V-cycle; ``l``: level ``l`` visits level ``l+1`` twice per cycle),
        ``krylov_method`` ("bicgstab": the reference's KSP type, OF.py:1081; "gmres": restarted GMRES with the same
        preconditioner and stopping rule; "auto" (default): BiCGStab, and GMRES(``gmres_restart``, default 100) for the
        pairs that have not converged after 25 iterations - the grad-div dominated regimes),
        ``preconditioner`` ("auto" (default): the multigrid cycle, and pairs it leaves unconverged - the grad-div dominated
        regimes, e.g. 8-bit data with ``speed_alpha`` below ~1e5 - are solved once more with the direct preconditioner when
        that fits; "multigrid"; "direct"),
        ``warm_start_stride`` (both modes, stacks whose first phase fills the chip: every n-th pair of a batch is solved
        first, the others start from their solved neighbour, cf. OF.py:803-806; default 3, 0 = every pair from the
        constant initial fields),
        ``verbose``, ``return_stats`` (adds ``result['stats']``: per-pair iterations / residual /
        converged / functionals), ``output`` ("numpy": host arrays as in the reference; "torch": ``movie`` may be a
        torch tensor already on the device and every array of the result stays on the device as a float64 torch
        tensor - blur, solve and epilogue without PCIe traffic, see ``subsample_velocities_for_visualisation``).
    """
    side = _side(output, device)
    direct_fallback = bool(use_direct_solver and preconditioner is None)     # not an explicit preconditioner="direct"
    if output == "torch":
        return _variational_optical_flow_device(side, movie, smoothing_sigma, device, max_pairs_in_flight, verbose, return_stats,
                                                reference_quirks, _solver_params(
                                                    speed_alpha, remodelling_alpha, delta_x, delta_t, initial_v_x, initial_v_y,
                                                    initial_remodelling, use_direct_solver, rtol, max_iterations,
                                                    reference_quirks, coarse_precision, vcycle_precision, multigrid_sweeps,
                                                    w_cycle_level, krylov_method, gmres_restart, warm_start_stride, preconditioner),
                                                delta_x, delta_t, direct_fallback)
    source = np.asarray(movie)
    T, N_i, N_j = _movie_shape(source, 2)
    # OF.py:769: the reference works on (and returns, as 'original_data') a float64 COPY of the movie.  A stack that already is
    # float64 and contiguous is only read by the solver, so the copy the result needs is made WHILE the solve runs (46 ms of a
    # 0.39-s call at 1024 x 1024 x 256); anything else is converted first, as the reference does
    if source.dtype == np.float64 and source.flags.c_contiguous:
        movie, copy_done = _float64_copy(source, wait=False)
        movie_in = source
    else:
        movie = _float64_copy(source)
        copy_done = None
        movie_in = movie
    params = _solver_params(speed_alpha, remodelling_alpha, delta_x, delta_t, initial_v_x, initial_v_y, initial_remodelling,
                            use_direct_solver, rtol, max_iterations, reference_quirks, coarse_precision, vcycle_precision,
                            multigrid_sweeps, w_cycle_level, krylov_method, gmres_restart, warm_start_stride, preconditioner)
    exact = max_pairs_in_flight is not None
    if max_pairs_in_flight is None and _solver is None:
        max_pairs_in_flight = choose_pairs_in_flight(N_i, N_j, T - 1, device, params=params)
    t0 = time.time()
    # a caller-owned context (_solver) or the module's cached one; blur and solve share it
    try:
        with (contextlib.nullcontext(_solver) if _solver is not None
              else _device_context(N_i, N_j, max_pairs_in_flight, device, exact)) as solver:
            if smoothing_sigma is not None:                                 # OF.py:770-773
                movie_to_analyse = side.blurred(side.frames(movie_in), gaussian_taps(smoothing_sigma), solver)
            else:
                movie_to_analyse = movie_in
            out = [side.empty((T - 1, N_i, N_j)) for _ in range(4)]
            stats = _solve(solver, side.frames(movie_to_analyse), params, out, direct_fallback)     # (the copy keeps a Fortran order)
    finally:
        if copy_done is not None:
            copy_done()
    if smoothing_sigma is None:
        movie_to_analyse = movie             # (the reference's 'blurred_data' is its float64 copy when nothing is blurred)
    if verbose:
        m, s, ms = format_elapsed_time(time.time() - t0)
        print(f"Elapsed time for solve: {m} minutes, {s} seconds, {ms} milliseconds")
        for k in range(T - 1):
            print(f"pair {k + 1}: iterations {stats['iterations'][k]}, relative residual "
                  f"{stats['relative_residual'][k]:.3e}, converged {bool(stats['converged'][k])}")
        if not stats["converged"].all():
            print("the solver has not actually converged, the result will be incorrect or inaccurate")
    return _variational_result(out, stats, movie, movie_to_analyse, delta_x, delta_t, reference_quirks, return_stats)


def _solve(solver, movie, params, out, direct_fallback):
    """The solve of a float64 stack into the four stacks ``out = [v_x, v_y, remodelling, speed]`` on its side; returns the per-pair
    records.  ``direct_fallback``: a stack too large for the direct preconditioner is solved by multigrid to the same tight tolerance."""
    try:
        return solver.solve(movie, movie.shape[0], params, *out)
    except _native.VofError as exc:
        if not (direct_fallback and _direct_unavailable(exc)):
            raise
        params.preconditioner = 2
        return solver.solve(movie, movie.shape[0], params, *out)


def _variational_result(out, stats, movie, movie_to_analyse, delta_x, delta_t, reference_quirks, return_stats):
    """The reference's result dict (OF.py:1193-1205) from the four stacks ``_solve`` filled and its per-pair records."""
    result = dict(v_x=out[0], v_y=out[1], speed=out[3], remodelling=out[2], original_data=movie, delta_x=delta_x, delta_t=delta_t,
                  blurred_data=movie_to_analyse, converged=bool(stats["converged"][-1]),                  # OF.py:1202: last pair only
                  L1_functional=float(np.sum(stats["L1_functional"])),
                  remodelling_functional=float(np.sum(stats["remodelling_functional"])))
    # OF.py:1205 stores the remodelling sum under 'speed_functional'
    result["speed_functional"] = result["remodelling_functional"] if reference_quirks else float(np.sum(stats["speed_functional"]))
    if return_stats:
        result["stats"] = stats
    return result


def _variational_optical_flow_device(side, movie, smoothing_sigma, device, max_pairs_in_flight, verbose, return_stats,
                                     reference_quirks, params, delta_x, delta_t, direct_fallback=False):
    """``output="torch"`` branch of ``variational_optical_flow``, which differs from the host branch before the solve: no float64 copy
    of the caller's movie, a batch sized without staging buffers, and one wait for the caller's stream ahead of blur and solve."""
    movie = side.frames(movie)                                                            # OF.py:769
    T, N_i, N_j = _movie_shape(movie, 2)
    exact = max_pairs_in_flight is not None
    if max_pairs_in_flight is None:
        # device-resident call: no staging buffers, and what is free now is free of the caller's tensors already
        max_pairs_in_flight = choose_pairs_in_flight(N_i, N_j, T - 1, int(device), memory_fraction=0.8, params=params, staging=False)
    out = [side.empty((T - 1, N_i, N_j)) for _ in range(4)]
    side.wait()
    with _device_context(N_i, N_j, max_pairs_in_flight, device, exact) as solver:
        movie_to_analyse = movie
        if smoothing_sigma is not None:                                                  # OF.py:770-773
            movie_to_analyse = side.empty(movie.shape)
            solver.blur(movie, movie_to_analyse, T, gaussian_taps(smoothing_sigma))
        stats = _solve(solver, movie_to_analyse, params, out, direct_fallback)
    if verbose:
        print(f"iterations {stats['iterations'].tolist()}, converged {stats['converged'].astype(bool).tolist()}")
    return _variational_result(out, stats, movie, movie_to_analyse, delta_x, delta_t, reference_quirks, return_stats)


# ---------------------------------------------------------------------------------------------------------
# Box least-squares flow (Vig et al. 2016): the reference's other estimator, OF.py:24-218.
# ---------------------------------------------------------------------------------------------------------
def conduct_optical_flow_jit(movie, box_size=15, delta_x=1.0, delta_t=1.0, include_remodelling=False, *,
                             reference_quirks=True, device=0):
    """Windowed least-squares flow of every frame pair on the GPU; arguments and the returned 4-tuple
    ``(v_x, v_y, speed, net_remodelling)`` as OF.py:24-157 (float64 ``(T-1, N_i, N_j)``; ``net_remodelling`` all zero
    without ``include_remodelling``).  Field ``k`` is computed from frames ``k`` and ``k + 1``.  See ``conduct_optical_flow``
    for ``reference_quirks``."""
    side = _HostSide()
    T, N_i, N_j = _movie_shape(movie, 2)
    if int(box_size) < 1:
        raise ValueError("box_size must be >= 1")
    with _device_context(N_i, N_j, side.box_flow_pairs(T - 1), device) as solver:
        return solver.box_flow_host(side.frames(movie), int(box_size), delta_x, delta_t, include_remodelling, reference_quirks)


def _box_flow_result(fields, movie, analysed, delta_x, delta_t, include_remodelling):
    """The result dict of the box flow (OF.py:205-218) from its field stacks ``[v_x, v_y, speed[, net_remodelling]]``."""
    result = dict(v_x=fields[0], v_y=fields[1], speed=fields[2], original_data=movie, delta_x=delta_x, delta_t=delta_t,
                  blurred_data=analysed)
    if include_remodelling:
        result["net_remodelling"] = fields[3]
    return result


def conduct_optical_flow(movie, boxsize=15, delta_x=1.0, delta_t=1.0, smoothing_sigma=None, background=None,
                         include_remodelling=False, *, reference_quirks=True, device=0, output="numpy"):
    """Optical flow as in Vig et al., Biophysical Journal 110, 1469-1475 (2016), on one MI355X; positional arguments and
    result dict as OF.py:159-218.

    Per frame pair the products of the image derivatives (central differences of the two frames' mean, zero on the border
    lines) and of the frame difference are summed over the ``boxsize`` x ``boxsize`` window of every pixel (half width
    ``int(boxsize / 2)``, clipped at the image edge) and a 2 x 2 system - 3 x 3 with ``include_remodelling`` - is solved in
    closed form.  ``background``: the movie is blurred with sigma 10, ``movie - background`` is kept where the blurred value
    exceeds ``background`` and zero elsewhere; then the optional blur with ``smoothing_sigma`` (OF.py:195-203).

    Returns ``v_x``, ``v_y``, ``speed`` (float64 ``(T-1, N_i, N_j)``, in ``delta_x / delta_t`` units), ``original_data``
    (the array passed in), ``blurred_data`` (the analysed movie: the input itself when nothing was blurred or
    subtracted), ``delta_x``, ``delta_t`` and, with ``include_remodelling``, ``net_remodelling``.  A pixel whose system is
    singular holds what IEEE division gives (NaN / Inf), as in the reference.

    Keyword-only extras: ``reference_quirks`` (True reproduces OF.py:108, the column window clamped with ``N_i`` - for
    ``N_j > N_i`` the columns ``j >= N_i + h`` have empty windows -, ``n = boxsize**2`` also for clipped windows and even
    ``boxsize``, and with ``include_remodelling`` an all-zero ``speed`` and zeros at pixels whose determinant is exactly 0;
    False: the window is clamped with ``N_j``, ``n`` is the number of pixels in the window, ``speed`` is filled and such
    pixels are NaN), ``device``, ``output`` ("numpy", or "torch": ``movie`` may be a device tensor and every array of the
    result stays on the device as a float64 tensor; ``blurred_data`` is then float64 even for an integer movie)."""
    side = _side(output, device)
    T, N_i, N_j = _movie_shape(movie, 2)
    if int(boxsize) < 1:
        raise ValueError("boxsize must be >= 1")
    with _device_context(N_i, N_j, side.box_flow_pairs(T - 1), device) as solver:
        analysed = side.analysed(movie, background, solver)
        if smoothing_sigma is not None:                                     # OF.py:202-203
            analysed = side.blurred(analysed, gaussian_taps(smoothing_sigma), solver)
        # without include_remodelling the _dev twin is handed no fourth stack; the _host twin is, and zero-fills it, as it always was
        fields = [side.empty((T - 1, N_i, N_j)) for _ in range(4 if include_remodelling or output == "numpy" else 3)]
        side.wait()
        solver.box_flow(analysed, T, int(boxsize), delta_x, delta_t, include_remodelling, reference_quirks, *fields)
    if background is None and smoothing_sigma is None:
        analysed = side.untouched(movie, analysed)
    return _box_flow_result(fields, movie, analysed, delta_x, delta_t, include_remodelling)


def _sweep_edges(name, bins, value_range):
    """None, or the ``np.linspace`` edges ``np.histogram(x, bins, value_range)`` uses."""
    if bins is None:
        return None
    if value_range is None:
        raise ValueError(f"{name}_bins needs a {name}_range")
    lo, hi = float(value_range[0]), float(value_range[1])
    if int(bins) < 1 or not np.isfinite([lo, hi]).all() or not hi > lo:
        raise ValueError(f"{name}_bins must be >= 1 and {name}_range finite and increasing")
    return np.linspace(lo, hi, int(bins) + 1, endpoint=True, dtype=np.float64)


def _sweep_probes(probe_locations, N_i, N_j):
    if probe_locations is None:
        return None
    probes = np.asarray(probe_locations)
    if probes.ndim != 2 or probes.shape[1] != 2 or probes.shape[0] < 1:
        raise ValueError("probe_locations must have shape (n_loc, 2)")
    probes = probes.astype(np.int64)
    if (probes < 0).any() or (probes[:, 0] >= N_i).any() or (probes[:, 1] >= N_j).any():
        raise ValueError("probe outside the image")
    return probes


FIELD_NAMES = ("v_x", "v_y", "speed", "net_remodelling")


def _run_sweep(name, args, movie, n, background, include_remodelling, probe_locations, return_fields, device, output):
    """What the sweeps of the box flow share around their native call ``Solver.<name>``: the movie becomes a float64 stack on the side
    ``output`` names, ``background`` is applied as in ``conduct_optical_flow`` and the stacks of the ``n`` entries are allocated.
    ``args`` are the arguments of the call between the frame count and the probe locations.  Returns the summaries of the call and
    the list of field stacks (None without ``return_fields``)."""
    side = _side(output, device)
    T, N_i, N_j = _movie_shape(movie, 2)
    probes = _sweep_probes(probe_locations, N_i, N_j)
    fields = None
    with _device_context(N_i, N_j, side.box_flow_pairs(T - 1), device) as solver:
        analysed = side.analysed(movie, background, solver)
        if return_fields:
            fields = [side.empty((n, T - 1, N_i, N_j)) for _ in range(4 if include_remodelling else 3)]
        side.wait()
        summaries = getattr(solver, name)(analysed, T, *args, probe_locations=probes, **dict(zip(FIELD_NAMES, fields or ())))
    return summaries, fields


def _sweep_result(listed, summaries, fields, own, edges, include_remodelling, delta_x, delta_t, filename):
    """The dict a sweep returns: ``listed`` (its list), the statistics every sweep has, ``own`` behind the speed histogram, the
    probes, the fields; saved with ``np.save`` if ``filename`` is given."""
    rec, hist, probe_speeds = summaries[0], summaries[1], summaries[-1]
    result = dict(listed)
    result["speed_means"] = rec["speed_mean"].copy()
    result["speed_stds"] = np.sqrt(rec["speed_variance"])
    result["nonfinite_counts"] = rec["nonfinite_count"].copy()
    if include_remodelling:
        result["remodelling_means"] = rec["remodelling_mean"].copy()
        result["remodelling_stds"] = np.sqrt(rec["remodelling_variance"])
    if edges is not None:
        result["speed_histograms"] = hist
        result["histogram_edges"] = edges
    result.update(own)
    if probe_speeds is not None:
        result["probe_speeds"] = probe_speeds
    if fields is not None:
        result["v_x"], result["v_y"], result["speed"] = fields[0], fields[1], fields[2]
        if include_remodelling:
            result["net_remodelling"] = fields[3]
    result["delta_x"] = delta_x
    result["delta_t"] = delta_t
    if filename is not None:
        np.save(filename, result)
    return result


def vary_boxsize(movie, boxsizes=np.arange(5, 150, 2), delta_x=1.0, delta_t=1.0, smoothing_sigma=None, background=None,
                 include_remodelling=False, filename=None, *, histogram_bins=None, histogram_range=None,
                 probe_locations=None, return_fields=False, reference_quirks=True, device=0, output="numpy"):
    """The box-size sweep the reference's scripts run around ``conduct_optical_flow`` (compare_rho_and_actin.py:387-419 and
    853-894) as one native call (``vof_vary_boxsize_*``): the movie goes up once, ``background`` / ``smoothing_sigma`` are
    applied once exactly as in ``conduct_optical_flow``, the per-pair derivative planes are computed once, the window grows
    by one ring per step (each box costs O(1) per pixel) and only the summaries come back.

    Every entry of ``boxsizes`` (any order, duplicates allowed) is made an integer with the builtin ``round`` and then
    treated as ``conduct_optical_flow(boxsize=b)`` treats it; the fields of a box do not depend on the rest of the list.

    Returns a dict with ``boxsizes``, ``speed_means``, ``speed_stds`` (``np.mean`` / ``np.std`` of the box's speed stack; NaN
    propagates), ``nonfinite_counts``, ``delta_x``, ``delta_t`` and
    with ``include_remodelling``: ``remodelling_means``, ``remodelling_stds`` (of ``net_remodelling``);
    with ``histogram_bins`` (``histogram_range=(lo, hi)`` is then required): ``speed_histograms``, int64 ``(n_boxes, bins)``,
    equal to ``np.histogram(speed.ravel(), bins, range)[0]``, and ``histogram_edges``;
    with ``probe_locations`` of shape ``(n_loc, 2)``: ``probe_speeds`` of shape ``(n_boxes, T-1, n_loc)``, ``speed[k, i, j]``;
    with ``return_fields``: ``v_x``, ``v_y``, ``speed`` and, if asked for, ``net_remodelling`` of shape
    ``(n_boxes, T-1, N_i, N_j)``.  Without it no full-size field stack exists on either side.
    ``filename``: the dict is saved with ``np.save``.  ``output="torch"``: ``movie`` may be a device tensor and the field
    stacks stay on the device as float64 tensors; the summaries are numpy arrays in both modes."""
    boxes = [int(round(float(b))) for b in np.asarray(boxsizes).ravel()]
    if not boxes:
        raise ValueError("boxsizes is empty")
    if min(boxes) < 1:
        raise ValueError("every box size must be >= 1")
    edges = _sweep_edges("histogram", histogram_bins, histogram_range)
    taps = None if smoothing_sigma is None else gaussian_taps(smoothing_sigma)
    summaries, fields = _run_sweep("vary_boxsize", (boxes, delta_x, delta_t, include_remodelling, reference_quirks, taps, edges), movie,
                                   len(boxes), background, include_remodelling, probe_locations, return_fields, device, output)
    return _sweep_result({"boxsizes": np.asarray(boxes)}, summaries, fields, {}, edges, include_remodelling, delta_x, delta_t, filename)


def vary_blursize(movie, blursizes=np.arange(0.5, 15, 0.1), boxsize=21, delta_x=1.0, delta_t=1.0, background=None,
                  include_remodelling=False, filename=None, *, histogram_bins=None, histogram_range=None, angle_bins=None,
                  intensity_bins=None, intensity_range=None, probe_locations=None, return_fields=False, reference_quirks=True,
                  device=0, output="numpy"):
    """The blur sweep the reference's scripts run around ``conduct_optical_flow`` (compare_rho_and_actin.py:485-614, and
    120-196 for the intensity histogram) as one native call (``vof_vary_blursize_*``): the movie goes up once, ``background``
    is applied once exactly as in ``conduct_optical_flow``, and per entry of ``blursizes`` the frames are blurred with
    ``gaussian_taps(s)``, the box flow of ``boxsize`` runs on them and only the summaries come back.

    Every entry ``s`` (finite and ``> 0``; any order, duplicates allowed) is treated as ``conduct_optical_flow(movie, boxsize,
    delta_x, delta_t, smoothing_sigma=s, background=background, include_remodelling=...)`` treats it, bit for bit; the fields
    of an entry do not depend on the rest of the list.

    Returns a dict with ``blursizes``, ``speed_means``, ``speed_stds`` (``np.mean`` / ``np.std`` of the entry's speed stack;
    NaN propagates), ``nonfinite_counts``, ``delta_x``, ``delta_t`` and
    with ``include_remodelling``: ``remodelling_means``, ``remodelling_stds`` (of ``net_remodelling``);
    with ``histogram_bins`` (``histogram_range=(lo, hi)`` is then required): ``speed_histograms``, int64 ``(n, bins)``, equal
    to ``np.histogram(speed.ravel(), bins, range)[0]``, and ``histogram_edges``;
    with ``angle_bins`` (at most 128): ``angle_histograms``, int64 ``(n, angle_bins)``, ``np.histogram(a, angle_bins, (-1, 1))[0]``
    of the flow direction ``a = np.arccos(v_y / speed) * np.sign(v_x) / np.pi``, ``weighted_angle_histograms``, float64, the
    same with ``weights=speed`` (bit-identical from call to call and for every number of pairs in flight), and
    ``angle_edges``; a sample whose speed is not finite counts in neither;
    with ``intensity_bins`` (``intensity_range`` is then required): ``intensity_histograms``, int64, ``np.histogram`` of the
    whole blurred, analysed stack of the entry, and ``intensity_edges``;
    with ``probe_locations`` of shape ``(n_loc, 2)``: ``probe_speeds`` of shape ``(n, T-1, n_loc)``, ``speed[k, i, j]``;
    with ``return_fields``: ``v_x``, ``v_y``, ``speed`` and, if asked for, ``net_remodelling`` of shape ``(n, T-1, N_i, N_j)``.
    Without it no full-size field stack exists on either side.
    ``filename``: the dict is saved with ``np.save``.  ``output="torch"``: ``movie`` may be a device tensor and the field
    stacks stay on the device as float64 tensors; the summaries are numpy arrays in both modes."""
    sigmas = np.asarray(blursizes, dtype=np.float64).ravel()
    if sigmas.size == 0:
        raise ValueError("blursizes is empty")
    if not (np.isfinite(sigmas).all() and (sigmas > 0).all()):
        raise ValueError("every blur size must be finite and > 0")
    if int(boxsize) < 1:
        raise ValueError("boxsize must be >= 1")
    edges = _sweep_edges("histogram", histogram_bins, histogram_range)
    intensity_edges = _sweep_edges("intensity", intensity_bins, intensity_range)
    if angle_bins is not None and not 1 <= int(angle_bins) <= 128:
        raise ValueError("angle_bins must be 1 .. 128")
    taps = [gaussian_taps(s) for s in sigmas]
    args = (taps, int(boxsize), delta_x, delta_t, include_remodelling, reference_quirks, edges, angle_bins, intensity_edges)
    summaries, fields = _run_sweep("vary_blursize", args, movie, len(taps), background, include_remodelling, probe_locations,
                                   return_fields, device, output)
    own = dict()
    if angle_bins is not None:
        own["angle_histograms"], own["weighted_angle_histograms"] = summaries[2], summaries[3]
        own["angle_edges"] = np.linspace(-1.0, 1.0, int(angle_bins) + 1, endpoint=True, dtype=np.float64)
    if intensity_edges is not None:
        own["intensity_histograms"] = summaries[4]
        own["intensity_edges"] = intensity_edges
    return _sweep_result({"blursizes": sigmas}, summaries, fields, own, edges, include_remodelling, delta_x, delta_t, filename)


COMPARE_MAX_ANGLE_BINS = 64          # CP_MAX_THETA_BINS of csrc/vof_compare.hpp: angle_bins and relative_angle_bins
COMPARE_MAX_SPEED_BINS = 1024        # CP_MAX_SPEED_BINS: per axis of joint_speed_bins


def _channel_pair(name, value):
    """``(a, b)`` of an argument that is a scalar or None (both channels) or a pair."""
    if isinstance(value, (tuple, list)) or (isinstance(value, np.ndarray) and value.ndim > 0):
        if len(value) != 2:
            raise ValueError(f"{name} must be a scalar or a pair (a, b)")
        return value[0], value[1]
    return value, value


def _compare_arguments(movie_a, movie_b, boxsize, smoothing_sigma, background, histogram_bins, histogram_range, angle_bins,
                       relative_angle_bins, joint_speed_bins, joint_speed_ranges, output):
    """The argument checks of ``compare_channel_flows`` (``output`` is checked by its ``_side``), all before the library is touched;
    returns the shape, the per-channel sigmas and backgrounds, the speed edges and the pair of joint speed edges (or None)."""
    shape = _movie_shape(movie_a, 2)
    if tuple(movie_b.shape if hasattr(movie_b, "shape") else np.asarray(movie_b).shape) != shape:
        raise ValueError("movie_a and movie_b must have the same shape (frames, x, y)")
    if int(boxsize) < 1:
        raise ValueError("boxsize must be >= 1")
    sigmas = _channel_pair("smoothing_sigma", smoothing_sigma)
    for s in sigmas:
        if s is not None and not (np.isfinite(float(s)) and float(s) > 0):
            raise ValueError("smoothing_sigma must be finite and > 0")
    backgrounds = _channel_pair("background", background)
    edges = _sweep_edges("histogram", histogram_bins, histogram_range)
    if angle_bins is not None and not 1 <= int(angle_bins) <= COMPARE_MAX_ANGLE_BINS:
        raise ValueError(f"angle_bins must be 1 .. {COMPARE_MAX_ANGLE_BINS}")
    if relative_angle_bins is None or not 1 <= int(relative_angle_bins) <= COMPARE_MAX_ANGLE_BINS:
        raise ValueError(f"relative_angle_bins must be 1 .. {COMPARE_MAX_ANGLE_BINS}")
    joint_edges = None
    if joint_speed_bins is not None:
        if np.ndim(joint_speed_bins) != 1 or len(joint_speed_bins) != 2:
            raise ValueError("joint_speed_bins must be a pair (bins_a, bins_b)")
        if joint_speed_ranges is None:
            raise ValueError("joint_speed_bins needs joint_speed_ranges")
        if len(joint_speed_ranges) != 2 or any(np.ndim(r) != 1 or len(r) != 2 for r in joint_speed_ranges):
            raise ValueError("joint_speed_ranges must be a pair ((lo, hi), (lo, hi))")
        if not all(1 <= int(b) <= COMPARE_MAX_SPEED_BINS for b in joint_speed_bins):
            raise ValueError(f"joint_speed_bins must be 1 .. {COMPARE_MAX_SPEED_BINS} per axis")
        joint_edges = tuple(_sweep_edges("joint_speed", b, r) for b, r in zip(joint_speed_bins, joint_speed_ranges))
    return shape, sigmas, backgrounds, edges, joint_edges


def compare_channel_flows(movie_a, movie_b, boxsize=31, delta_x=1.0, delta_t=1.0, smoothing_sigma=None, background=None,
                          include_remodelling=False, filename=None, *, histogram_bins=50, histogram_range=None, angle_bins=50,
                          relative_angle_bins=50, joint_speed_bins=None, joint_speed_ranges=None, joint_speed_min_b=None,
                          return_fields=False, reference_quirks=True, device=0, output="numpy"):
    """The comparison of two channels of one movie the reference's scripts run around ``conduct_optical_flow``
    (compare_rho_and_actin.py:616-767: Rho and actin, box 31, sigma 3) as one native call (``vof_compare_flows_*``): the box
    flow of both channels, their per-channel statistics and the joint statistics of the two velocity fields; only the
    summaries come back.

    ``movie_a`` and ``movie_b`` have the same shape ``(T, N_i, N_j)``, ``T >= 2``.  ``smoothing_sigma`` and ``background`` are a
    scalar (both channels) or a pair ``(a, b)``.  Each channel is treated as ``conduct_optical_flow(movie, boxsize, delta_x,
    delta_t, smoothing_sigma, background, include_remodelling, reference_quirks=...)`` treats it, bit for bit.

    Returns a dict of numpy summaries.  Per channel, leading axis of length 2, a first: ``speed_means``, ``speed_stds``
    (``np.mean`` / ``np.std`` of the channel's speed stack; NaN propagates), ``nonfinite_counts`` and
    with ``include_remodelling``: ``remodelling_means``, ``remodelling_stds``;
    with ``histogram_bins`` (``histogram_range=(lo, hi)`` is then required; pass ``histogram_bins=None`` for none):
    ``speed_histograms``, int64 ``(2, bins)``, equal to ``np.histogram(speed.ravel(), bins, range)[0]``, and ``histogram_edges``;
    with ``angle_bins`` (None, or 1 .. 64): ``angle_histograms``, ``weighted_angle_histograms`` and ``angle_edges`` as
    ``vary_blursize`` defines them, the direction ``np.arccos(v_y / speed) * np.sign(v_x) / np.pi`` on (-1, 1), weighted by ``speed``.

    Joint, over all ``T - 1`` pairs and all pixels, per sample in float64 and in this order: ``dot = v_x_a * v_x_b + v_y_a *
    v_y_b``, ``w = speed_a * speed_b``, ``cos = dot / w``, ``theta = np.arccos(cos) / np.pi``.  A sample takes part only if both
    speeds are finite; the others are counted in ``joint_nonfinite_count``.  With ``reference_quirks=True`` ``cos`` is not
    clipped, as in the script, so a rounding excess over 1 (about a third of the pixels when both channels are the same 8-bit
    movie) gives a NaN ``theta``; ``reference_quirks=False`` clips ``cos`` to [-1, 1] first.  A sample whose ``theta`` is NaN
    (also: a zero speed) is in no bin and counted in ``relative_angle_dropped``.
    ``relative_angle_histogram``: int64, ``np.histogram(theta, relative_angle_bins, (0, 1))[0]`` (1 .. 64 bins);
    ``weighted_relative_angle_histogram``: float64, the same with ``weights=w``, bit-identical from call to call and for every
    number of pairs in flight; ``weighted_relative_angle_density``: what ``density=True`` makes of it, ``sums /
    np.diff(edges) / sums.sum()``; ``relative_angle_edges``.
    With ``joint_speed_bins=(ba, bb)`` (1 .. 1024 each; ``joint_speed_ranges=((lo, hi), (lo, hi))`` is then required):
    ``joint_speed_histogram``, int64 ``(ba, bb)``, equal to ``np.histogram2d(speed_a[m], speed_b[m], bins, range)[0]`` with ``m =
    speed_b > joint_speed_min_b`` (``None``: all samples), ``joint_speed_edges_a`` and ``joint_speed_edges_b``.
    ``delta_x`` and ``delta_t`` are returned.  With ``return_fields``: ``a`` and ``b``, dicts as ``conduct_optical_flow`` returns
    them; without it no full-size field stack exists on either side beyond the pairs in flight.
    ``filename``: the dict is saved with ``np.save``.  ``output="torch"``: the movies may be device tensors and the arrays of ``a``
    and ``b`` stay on the device as float64 tensors; the summaries are numpy arrays in both modes."""
    side = _side(output, device)
    (T, N_i, N_j), sigmas, backgrounds, edges, joint_edges = _compare_arguments(
        movie_a, movie_b, boxsize, smoothing_sigma, background, histogram_bins, histogram_range, angle_bins, relative_angle_bins,
        joint_speed_bins, joint_speed_ranges, output)
    taps = [None if s is None else gaussian_taps(s) for s in sigmas]
    movies, fields = (movie_a, movie_b), (None, None)
    with _device_context(N_i, N_j, side.box_flow_pairs(T - 1), device) as solver:
        analysed = [side.analysed(movies[ch], backgrounds[ch], solver) for ch in range(2)]
        if return_fields:
            fields = [[side.empty((T - 1, N_i, N_j)) for _ in range(4 if include_remodelling else 3)] for _ in range(2)]
        side.wait()
        summaries = solver.compare_flows(analysed[0], analysed[1], T, int(boxsize), delta_x, delta_t, include_remodelling, reference_quirks,
                                         taps[0], taps[1], edges, angle_bins, int(relative_angle_bins), joint_edges, joint_speed_min_b,
                                         *fields)
        if return_fields:                                                  # the blurred stacks exist only for the result dicts
            blurred = [analysed[ch] if taps[ch] is None else side.blurred(analysed[ch], taps[ch], solver) for ch in range(2)]
    rec, hist, angle_hist, weighted_angle_hist, theta_hist, weighted_theta_hist, joint_hist, joint_counts = summaries
    own = dict()
    if angle_bins is not None:
        own["angle_histograms"], own["weighted_angle_histograms"] = angle_hist, weighted_angle_hist
        own["angle_edges"] = np.linspace(-1.0, 1.0, int(angle_bins) + 1, endpoint=True, dtype=np.float64)
    theta_edges = np.linspace(0.0, 1.0, int(relative_angle_bins) + 1, endpoint=True, dtype=np.float64)
    own["joint_nonfinite_count"], own["relative_angle_dropped"] = int(joint_counts[0]), int(joint_counts[1])
    own["relative_angle_histogram"] = theta_hist
    own["weighted_relative_angle_histogram"] = weighted_theta_hist
    with np.errstate(invalid="ignore", divide="ignore"):                  # np.histogram(..., density=True): nothing in range gives NaN
        own["weighted_relative_angle_density"] = weighted_theta_hist / np.diff(theta_edges) / weighted_theta_hist.sum()
    own["relative_angle_edges"] = theta_edges
    if joint_edges is not None:
        own["joint_speed_histogram"] = joint_hist
        own["joint_speed_edges_a"], own["joint_speed_edges_b"] = joint_edges
    result = _sweep_result({}, (rec, hist, None), None, own, edges, include_remodelling, delta_x, delta_t, None)
    if return_fields:
        for ch, key in enumerate("ab"):
            untouched = backgrounds[ch] is None and taps[ch] is None
            result[key] = _box_flow_result(fields[ch], movies[ch], movies[ch] if untouched else blurred[ch], delta_x, delta_t,
                                           include_remodelling)
    if filename is not None:
        np.save(filename, result)
    return result


# ---------------------------------------------------------------------------------------------------------
# A PIVlab result as a dense flow result (OF.py:2141-2230): scipy's Delaunay triangulation and gradient estimate per frame
# on the host, the Clough-Tocher interpolant at every pixel on the device.  DESIGN.md section 19.
# ---------------------------------------------------------------------------------------------------------
PIV_KEYS = ("x", "y", "u_original", "v_original")


def _piv_frame_on_host(tri):
    """A triangulation with a degenerate simplex (scipy marks it with NaN in ``tri.transform`` and treats it specially in
    ``find_simplex``): its frame is evaluated by scipy itself."""
    return bool(np.isnan(tri.transform).any())


def _piv_stacks(x_locations, y_locations, v_x, v_y):
    """The four inputs as float64 ``(F, R, C)`` arrays of one shape (each an array of that shape or ``F`` separate ``(R, C)`` arrays)."""
    stacks = []
    for name, a in zip(("x_locations", "y_locations", "v_x", "v_y"), (x_locations, y_locations, v_x, v_y)):
        try:
            a = np.asarray(a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be an (F, R, C) array or F arrays of one shape (R, C)") from None
        if a.ndim != 3 or a.shape[0] < 1:
            raise ValueError(f"{name} must be an (F, R, C) array or F arrays of one shape (R, C), with F >= 1")
        stacks.append(a)
    if any(a.shape != stacks[0].shape for a in stacks):
        raise ValueError("x_locations, y_locations, v_x and v_y must have one common shape (F, R, C)")
    return stacks


def piv_tables(x_locations, y_locations, v_x, v_y):
    """The host part of ``upsample_PIV_vectors``: per frame the valid points (neither ``v_x`` nor ``v_y`` is NaN, OF.py:2195), their
    ``scipy.spatial.Delaunay`` triangulation (scipy's defaults, what ``griddata`` makes) and the gradients
    ``CloughTocher2DInterpolator(tri, (v_x, v_y)).grad`` (tol 1e-6, maxiter 400): one triangulation and one estimate for both fields,
    which equals the reference's two ``griddata`` calls bit for bit.  A frame whose locations and valid mask are those of the frame
    before keeps its triangulation.  Returns the tables ``Solver.piv_upsample`` takes, by name, and under ``"host_frames"`` a dict
    ``{frame: interpolant}`` of the frames with a degenerate simplex, which are left without triangles."""
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    x, y, vx, vy = _piv_stacks(x_locations, y_locations, v_x, v_y)
    rows = {k: [] for k in ("points", "values", "gradients", "transforms", "simplices", "neighbours")}
    point_offsets, triangle_offsets, host_frames = [0], [0], {}
    previous, tri = None, None
    for k in range(x.shape[0]):
        valid = np.logical_and(~np.isnan(vx[k]), ~np.isnan(vy[k]))
        points = np.stack([x[k][valid].ravel(), y[k][valid].ravel()], axis=1)
        values = np.stack([vx[k][valid].ravel(), vy[k][valid].ravel()], axis=1)
        key = (points.tobytes(), valid.tobytes())
        if key != previous:
            tri, previous = Delaunay(points), key
        interpolant = CloughTocher2DInterpolator(tri, values)
        if _piv_frame_on_host(tri):
            host_frames[k] = interpolant
        else:
            rows["points"].append(points.ravel()), rows["values"].append(values.ravel())
            rows["gradients"].append(np.asarray(interpolant.grad, dtype=np.float64).ravel())
            rows["transforms"].append(np.asarray(tri.transform, dtype=np.float64).ravel())
            rows["simplices"].append(tri.simplices.astype(np.int32).ravel()), rows["neighbours"].append(tri.neighbors.astype(np.int32).ravel())
        here = k not in host_frames
        point_offsets.append(point_offsets[-1] + (points.shape[0] if here else 0))
        triangle_offsets.append(triangle_offsets[-1] + (tri.simplices.shape[0] if here else 0))
    tables = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int32 if k in ("simplices", "neighbours") else np.float64))
              for k, v in rows.items()}
    tables["point_offsets"] = np.asarray(point_offsets, dtype=np.int32)
    tables["triangle_offsets"] = np.asarray(triangle_offsets, dtype=np.int32)
    tables["host_frames"] = host_frames
    return tables


def _upsample_PIV_vectors(x_locations, y_locations, v_x, v_y, shape, device, output):
    """``upsample_PIV_vectors`` and the counts of the native call: pixels outside every triangle, frames evaluated on the host."""
    side = _side(output, device)
    stacks = _piv_stacks(x_locations, y_locations, v_x, v_y)
    try:
        N_i, N_j = (int(n) for n in shape)
        whole = (N_i, N_j) == tuple(shape)
    except (TypeError, ValueError):
        whole = False
    if not whole or min(N_i, N_j) < 4:
        raise ValueError("shape must be (N_i, N_j), two integers of at least 4")
    tables = piv_tables(*stacks)
    F = stacks[0].shape[0]
    outs = [side.empty((F, N_i, N_j)) for _ in range(3)]
    with _device_context(N_i, N_j, 1, device) as solver:
        side.wait()
        counts = solver.piv_upsample(tables, F, *outs)
    q_i, q_j = np.meshgrid(np.arange(N_i, dtype=np.float64), np.arange(N_j, dtype=np.float64), indexing="ij")
    for k, interpolant in tables["host_frames"].items():
        v = interpolant(q_j, q_i)
        fields = (v[..., 0], v[..., 1], np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]))
        for out, field in zip(outs, fields):
            if isinstance(out, np.ndarray):
                out[k] = field
            else:
                out[k].copy_(side.torch.as_tensor(np.ascontiguousarray(field)))
        counts[0] += int(np.isnan(fields[0]).sum())
    return tuple(outs), counts


def upsample_PIV_vectors(x_locations, y_locations, v_x, v_y, shape, *, device=0, output="numpy"):
    """PIV vectors on their own grid as dense fields: ``scipy.interpolate.griddata(..., method='cubic')`` of ``v_x`` and of ``v_y`` at
    every pixel of ``F`` frames of ``shape = (N_i, N_j)`` - the dense part of ``convert_PIV_result`` (OF.py:2193-2209), evaluated on the
    GPU.  Returns ``(v_x, v_y, speed)``, float64 ``(F, N_i, N_j)``.

    The four inputs are ``(F, R, C)`` arrays, or ``F`` separate ``(R, C)`` arrays each, with NaN for a missing vector - what
    ``analysis/postprocess_PIV.py:convert_PIV_result`` returns.  Per frame the valid points are those where neither ``v_x`` nor
    ``v_y`` is NaN; scipy triangulates them and estimates the gradients on the host (``piv_tables``), the device evaluates the
    Clough-Tocher element of every triangle:

    - ``out[k, i, j]`` is the interpolant at the point ``(x = j, y = i)``, which is what the reference's ``np.meshgrid`` gives for the
      square movies it can handle (for a non-square movie the reference raises a broadcast error; here the same rule serves it);
    - a pixel outside the convex hull of the frame's valid points is NaN in all three outputs;
    - ``speed = sqrt(v_x * v_x + v_y * v_y)``;
    - a pixel on an edge or a vertex belongs to the triangle of the lowest index, and powers are products, so the values differ from
      scipy's own evaluation by a few roundings (tests/test_piv_convert_cpu.py has the measured bound);
    - a frame whose triangulation has a degenerate simplex is evaluated by scipy on the host and copied into the outputs.

    ``ValueError``, before the library is touched, for inputs that are not four arrays of one shape ``(F, R, C)``, a ``shape`` that is
    not two integers of at least 4 and an unknown ``output``; scipy's own error for a frame that cannot be triangulated propagates.
    ``output="torch"``: the three results are float64 tensors on the device."""
    return _upsample_PIV_vectors(x_locations, y_locations, v_x, v_y, shape, device, output)[0]


def _piv_frames(PIV_result, key):
    """The 2-D arrays of ``PIV_result[key]``: ``scipy.io.loadmat``'s object array whose ``[k][0]`` is the frame, or a sequence of them."""
    try:
        listed = PIV_result[key]
        frames = [a[0] if isinstance(a, np.ndarray) and a.dtype == object else a for a in (listed[k] for k in range(len(listed)))]
        frames = [np.asarray(a) for a in frames]
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"PIV_result[{key!r}] must hold one 2-D array per frame (a PIVlab file as scipy.io.loadmat returns it)") from None
    if not frames or any(a.ndim != 2 or a.dtype == object or a.shape != frames[0].shape for a in frames):
        raise ValueError(f"PIV_result[{key!r}] must hold one 2-D array per frame, all of one shape")
    return frames


def convert_PIV_result(PIV_result, movie, delta_x=1.0, delta_t=1.0, *, device=0, output="numpy"):
    """The reference's ``convert_PIV_result`` (OF.py:2141-2230): a PIVlab result as a flow-result dictionary, the vectors upsampled
    to every pixel by ``upsample_PIV_vectors`` on the GPU instead of two ``scipy.interpolate.griddata`` calls per frame.

    ``PIV_result`` is what ``scipy.io.loadmat`` returns for a PIVlab file - ``PIV_result[key]`` an object array whose ``[k][0]`` is a
    2-D array, for the keys ``'x'``, ``'y'``, ``'u_original'``, ``'v_original'`` - or a plain sequence of 2-D arrays per key.
    ``movie`` is ``(T, N_i, N_j)``; only its shape is read.  Returns the reference's dictionary: ``v_x``, ``v_y``, ``speed`` (float64,
    ``(T - 1, N_i, N_j)``), ``delta_x``, ``delta_t``, ``original_data`` (``movie`` itself), ``x_locations``, ``y_locations``,
    ``PIV_v_x``, ``PIV_v_y`` (float64, one ``(R, C)`` frame per frame of ``PIV_result``).

    As in the reference (OF.py:2167-2181) the locations are ``x * delta_x`` and the vectors ``u * delta_x / delta_t``, numpy on the
    host, while the interpolation targets stay the pixel indices ``(x = j, y = i)``: that is consistent only for ``delta_x = 1``,
    which the reference's script uses, and it is kept.  Non-square movies are served by the same rule (the reference raises a
    broadcast error for them).  Frames of ``PIV_result`` past the first ``T - 1`` are unpacked and not upsampled, as in the reference;
    fewer than ``T - 1`` is a ``ValueError``.  ``output="torch"``: ``v_x``, ``v_y`` and ``speed`` are device tensors, which
    ``filter_PIV_flow_result`` and ``compare_flow_results`` take as they are (``original_data`` must then be a device tensor for the
    filter); everything else is host data."""
    _side(output, device)
    shape = _movie_shape(movie)
    frames = {key: _piv_frames(PIV_result, key) for key in PIV_KEYS}
    if len({(len(f), f[0].shape) for f in frames.values()}) != 1:
        raise ValueError("'x', 'y', 'u_original' and 'v_original' of PIV_result must hold the same number of frames of one shape")
    if len(frames["x"]) < shape[0] - 1:
        raise ValueError(f"PIV_result holds {len(frames['x'])} frames, the movie needs {shape[0] - 1}")
    unpacked = {key: np.zeros((len(frames[key]),) + frames[key][0].shape) for key in PIV_KEYS}
    for k in range(len(frames["x"])):
        unpacked["x"][k] = frames["x"][k] * delta_x
        unpacked["y"][k] = frames["y"][k] * delta_x
        unpacked["u_original"][k] = frames["u_original"][k] * delta_x / delta_t
        unpacked["v_original"][k] = frames["v_original"][k] * delta_x / delta_t
    P = shape[0] - 1
    v_x, v_y, speed = upsample_PIV_vectors(unpacked["x"][:P], unpacked["y"][:P], unpacked["u_original"][:P], unpacked["v_original"][:P],
                                           shape[1:], device=device, output=output)
    return {"v_x": v_x, "v_y": v_y, "speed": speed, "delta_x": delta_x, "delta_t": delta_t, "original_data": movie,
            "x_locations": unpacked["x"], "y_locations": unpacked["y"], "PIV_v_x": unpacked["u_original"],
            "PIV_v_y": unpacked["v_original"]}


# ---------------------------------------------------------------------------------------------------------
# The PIV vectors themselves: windowed cross-correlation of every frame pair on the device.  DESIGN.md section 20.
# ---------------------------------------------------------------------------------------------------------
PIV_MIN_WINDOW, PIV_MAX_WINDOW, PIV_MAX_RADIUS, PIV_MAX_PASSES = 4, 64, 16, 8    # PF_MIN_W, PF_MAX_W, PF_MAX_R, PF_MAX_PASSES of csrc/vof_pivflow.hpp
PIV_LDS_LIMIT = 160 * 1024 - 2048                                                 # PF_LDS_LIMIT


def _piv_lds_bytes(w, r):
    """pf_lds_doubles of csrc/vof_pivflow.hpp in bytes: the window, the search region and its row sums, rows at odd strides."""
    S, D = w + 2 * r, 2 * r + 1
    return 8 * (w * (w | 1) + S * (S | 1) + 2 * S * D)


def _piv_integers(name, values):
    try:
        listed = [values] if np.ndim(values) == 0 else list(values)
        whole = [int(n) for n in listed]
        if any(isinstance(n, bool) or n != m for n, m in zip(listed, whole)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be integers, one per pass") from None
    return whole


def _piv_passes(shape, window_sizes, search_radii, steps):
    """The passes as ``(w, r, s, m, R, C)`` tuples, with every check the library makes (include/vof.h) as a ``ValueError``."""
    w, r = _piv_integers("window_sizes", window_sizes), _piv_integers("search_radii", search_radii)
    s = [n // 2 for n in w] if steps is None else _piv_integers("steps", steps)
    if not (1 <= len(w) <= PIV_MAX_PASSES) or len(r) != len(w) or len(s) != len(w):
        raise ValueError(f"window_sizes, search_radii and steps must hold one entry per pass, 1 to {PIV_MAX_PASSES} passes")
    try:
        N_i, N_j = (int(n) for n in shape[-2:])
    except (TypeError, ValueError):
        raise ValueError("shape must end in (N_i, N_j)") from None
    passes, m = [], 0
    for p in range(len(w)):
        if not PIV_MIN_WINDOW <= w[p] <= PIV_MAX_WINDOW:
            raise ValueError(f"pass {p}: the window size must lie in [{PIV_MIN_WINDOW}, {PIV_MAX_WINDOW}], not {w[p]}")
        if not 1 <= r[p] <= PIV_MAX_RADIUS:
            raise ValueError(f"pass {p}: the search radius must lie in [1, {PIV_MAX_RADIUS}], not {r[p]}")
        if s[p] < 1:
            raise ValueError(f"pass {p}: the step must be at least 1, not {s[p]}")
        if p and w[p] > w[p - 1]:
            raise ValueError(f"pass {p}: window sizes must not increase from pass to pass ({w[p - 1]} then {w[p]})")
        if _piv_lds_bytes(w[p], r[p]) > PIV_LDS_LIMIT:
            raise ValueError(f"pass {p}: a {w[p]}-pixel window with radius {r[p]} does not fit the LDS of a compute unit")
        m += r[p]
        if min(N_i, N_j) < w[p] + 2 * m:
            raise ValueError(f"pass {p}: the grid is empty: frames of {N_i} x {N_j} are smaller than window + 2 * margin = {w[p] + 2 * m}")
        passes.append((w[p], r[p], s[p], m, (N_i - w[p] - 2 * m) // s[p] + 1, (N_j - w[p] - 2 * m) // s[p] + 1))
        if passes[-1][4] > 65535:
            raise ValueError(f"pass {p}: more than 65535 rows of windows do not fit one launch")
    return passes


def piv_grid(shape, window_sizes, search_radii, steps=None):
    """The window grid of ``conduct_piv`` for frames of ``shape = (N_i, N_j)`` (a movie's shape is taken by its last two entries): per
    pass a dict with the window size ``w``, radius ``r``, step ``s`` (``steps=None``: ``w // 2``), the margin ``m = r_0 + ... + r_p``,
    the grid ``R = (N_i - w - 2 m) // s + 1`` and ``C`` likewise, and the 0-based window centres ``x = j0 + (w - 1) / 2``,
    ``y = i0 + (w - 1) / 2`` as ``(R, C)`` arrays, window ``(a, b)`` having its top-left pixel at ``i0 = m + a s``, ``j0 = m + b s``.
    With these margins no search region leaves the frame, whatever offset the pass before hands on.  A pure host function;
    ``ValueError`` for everything ``conduct_piv`` refuses."""
    grids = []
    for w, r, s, m, R, C in _piv_passes(shape, window_sizes, search_radii, steps):
        y, x = np.meshgrid(m + s * np.arange(R) + (w - 1) / 2, m + s * np.arange(C) + (w - 1) / 2, indexing="ij")
        grids.append(dict(w=w, r=r, s=s, m=m, R=R, C=C, x=x, y=y))
    return grids


def _piv_options(deformation, outlier_threshold, outlier_epsilon, validate_last):
    """The options of ``conduct_piv`` as the library takes them, with every check it makes as a ``ValueError``."""
    if not isinstance(deformation, (bool, np.bool_)) or not isinstance(validate_last, (bool, np.bool_)):
        raise ValueError("deformation and validate_last must be bools")

    def number(name, value):
        try:
            if isinstance(value, (bool, np.bool_)):
                raise TypeError
            return float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number") from None
    if outlier_threshold is not None:
        outlier_threshold = number("outlier_threshold", outlier_threshold)
        if not (0 < outlier_threshold < np.inf):
            raise ValueError("outlier_threshold must be a positive finite number or None")
    outlier_epsilon = number("outlier_epsilon", outlier_epsilon)
    if not (0 <= outlier_epsilon < np.inf):
        raise ValueError("outlier_epsilon must be a non-negative finite number")
    if validate_last and outlier_threshold is None:
        raise ValueError("validate_last needs an outlier_threshold")
    return dict(deformation=bool(deformation), outlier_threshold=outlier_threshold, outlier_epsilon=outlier_epsilon, validate_last=bool(validate_last))


def conduct_piv(movie, window_sizes=(64, 32), search_radii=(16, 4), steps=None, min_correlation=None, smoothing_sigma=None, *,
                deformation=False, outlier_threshold=None, outlier_epsilon=0.1, validate_last=False, device=0, frames_in_flight=0):
    """Particle image velocimetry of every frame pair on the GPU: direct zero-normalised cross-correlation of interrogation windows,
    in ``len(window_sizes)`` passes, each pass searching around the rounded vector of the pass before.  The reference imports such
    vectors from PIVlab (``analysis/postprocess_PIV.py``); this makes them where the movie is.

    ``movie`` is ``(T, N_i, N_j)``, a numpy array or a device tensor of any real dtype (read as float64), blurred on the device first
    if ``smoothing_sigma`` is given.  Pass ``p`` correlates the ``w_p x w_p`` window of frame ``k`` at every point of ``piv_grid``
    with the windows of frame ``k + 1`` displaced by ``offset + d``, ``d`` in ``[-r_p, r_p]^2``; the peak is the first maximum in
    raster order, refined per axis by the three-point parabola unless it lies on the border of the search range (DESIGN.md section
    20 has all of the arithmetic; the device is held to ``tests/piv_flow_restatement.py`` bit for bit).  ``min_correlation`` (the
    ncorr script's 0.3, ``None``: off) makes the vectors of windows whose peak correlation is smaller NaN, in every pass.

    Returns a PIVlab-shaped dict, which ``convert_PIV_result`` takes: ``'x'``, ``'y'`` (0-based window centres, ``x`` along the
    columns), ``'u_original'`` (along the columns), ``'v_original'`` (along the rows), in pixels per frame, NaN for a missing vector
    (a flat window, or one under the threshold), and ``'correlation'`` - float64 host arrays ``(T - 1, R, C)`` of the last pass - and
    ``'counts'``, int64 ``(passes, 3)``: flat windows, peaks on the border of the search range, vectors under the threshold.

    Two options, independent of each other and off by default (DESIGN.md sections 20.7 to 20.9; the device is held to
    ``tests/piv_deform_restatement.py`` bit for bit):

    * ``deformation=True``: window deformation.  From the second pass on the search region is frame ``k + 1`` resampled
      (bilinearly) by the vectors of the pass before, interpolated (bilinearly) to every pixel, so the correlation finds only a
      residual around zero and the vector is the interpolated one at the window's centre plus that residual.  With one pass it
      changes nothing.
    * ``outlier_threshold`` (PIVlab's 2; ``None``: off): the normalised median test of Westerweel & Scarano (2005) on the vectors
      of a pass before the next one uses them.  A vector whose residual against the median of its (at least three) valid
      neighbours, ``|u - u_m| / (median |u_n - u_m| + outlier_epsilon)`` in ``u`` or in ``v``, exceeds the threshold is replaced by
      that median, and so is a missing vector.  ``validate_last=True`` applies it to the returned vectors too.  The result then has
      ``'validation_counts'``, int64 ``(passes, 2)``: outliers and filled vectors per pass (the last row zero without
      ``validate_last``); ``'counts'`` and ``'correlation'`` stay what the correlation found.

    ``ValueError`` before the library is touched: fewer than 2 frames, window sizes outside [4, 64] or growing from pass to pass, radii
    outside [1, 16], steps below 1, more than 8 passes, a frame smaller than ``w + 2 m`` of some pass, an ``outlier_threshold`` that is
    not positive and finite, an ``outlier_epsilon`` that is not non-negative and finite, a ``deformation`` or ``validate_last`` that is
    no bool, ``validate_last`` without a threshold.  The movie must be finite."""
    shape = _movie_shape(movie, 2)
    passes = _piv_passes(shape, window_sizes, search_radii, steps)
    options = _piv_options(deformation, outlier_threshold, outlier_epsilon, validate_last)
    if min_correlation is not None:
        try:
            min_correlation = float(min_correlation)
        except (TypeError, ValueError):
            raise ValueError("min_correlation must be a number or None") from None
    if smoothing_sigma is not None and not float(smoothing_sigma) > 0:
        raise ValueError("smoothing_sigma must be positive or None")
    on_device = _is_device_tensor(movie) and movie.is_cuda
    if on_device and movie.device.index is not None:
        device = movie.device.index
    side = _side("torch" if on_device else "numpy", device)
    T, (R, C) = shape[0], passes[-1][4:]
    frames = side.frames(movie)
    u, v, correlation = (side.empty((T - 1, R, C)) for _ in range(3))
    with _device_context(shape[1], shape[2], 1, device) as solver:
        if smoothing_sigma is not None:
            frames = side.blurred(frames, gaussian_taps(smoothing_sigma), solver)
        side.wait()
        counts = solver.piv_flow(frames, T - 1, *(tuple(p[k] for p in passes) for k in range(3)), u, v, correlation, min_correlation,
                                 frames_in_flight, **options)
    if not isinstance(u, np.ndarray):
        u, v, correlation = (a.cpu().numpy() for a in (u, v, correlation))
    last = piv_grid(shape, [p[0] for p in passes], [p[1] for p in passes], [p[2] for p in passes])[-1]
    x, y = (np.repeat(last[key][None], T - 1, axis=0) for key in ("x", "y"))
    result = {"x": x, "y": y, "u_original": u, "v_original": v, "correlation": correlation, "counts": counts}
    if options["outlier_threshold"] is not None:
        result["counts"], result["validation_counts"] = counts
    return result


def conduct_piv_flow(movie, delta_x=1.0, delta_t=1.0, smoothing_sigma=None, *, device=0, output="numpy", **piv_arguments):
    """``conduct_piv`` as a dense flow result: ``convert_PIV_result(conduct_piv(movie, smoothing_sigma=smoothing_sigma,
    **piv_arguments), movie, delta_x, delta_t)`` with the peak correlations under ``'PIV_correlation'`` - the dictionary
    ``filter_PIV_flow_result`` and ``compare_flow_results`` take, so PIV and the other estimators are compared without a PIVlab file.
    ``piv_arguments``: ``window_sizes``, ``search_radii``, ``steps``, ``min_correlation``, ``deformation``, ``outlier_threshold``,
    ``outlier_epsilon``, ``validate_last``, ``frames_in_flight``.  ``output="torch"``:
    ``v_x``, ``v_y`` and ``speed`` are device tensors (and ``movie`` should be one, for the filter).  Every frame pair needs at least
    three vectors that are not collinear: scipy's error for a frame that cannot be triangulated propagates."""
    _side(output, device)
    PIV_result = conduct_piv(movie, smoothing_sigma=smoothing_sigma, device=device, **piv_arguments)
    result = convert_PIV_result(PIV_result, movie, delta_x, delta_t, device=device, output=output)
    result["PIV_correlation"] = PIV_result["correlation"]
    return result


# ---------------------------------------------------------------------------------------------------------
# Two finished flow results: the reference's result filter (OF.py:2232-2250) and the comparison its scripts make of
# PIVlab's and Farnebäck's flow (analyse_short_timeinterval_data.py:640-745).  DESIGN.md section 17.
# ---------------------------------------------------------------------------------------------------------
FILTER_BLUR_SIGMA = 3                # OF.py:2242
FILTER_SPEED_LIMIT = 7               # OF.py:2247-2250 compare with 7 whatever speed_threshold says


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def _flow_fields(name, result):
    """``(v_x, v_y, speed)`` of a flow-result dict as the native calls take them - all numpy arrays or all device tensors,
    float64, C-contiguous, one shape ``(P, N_i, N_j)`` with frames of at least 4 x 4 pixels; ``ValueError`` otherwise, before the
    library is touched."""
    fields = []
    for key in ("v_x", "v_y", "speed"):
        try:
            f = result[key]
        except (KeyError, TypeError, IndexError):
            raise ValueError(f"{name} must be a flow-result dict with 'v_x', 'v_y' and 'speed'") from None
        if not (isinstance(f, np.ndarray) or _is_device_tensor(f)):
            raise ValueError(f"{name}[{key!r}] must be a numpy array or a device tensor")
        if _movie_dtype_name(f) != "float64":
            raise ValueError(f"{name}[{key!r}] is {_movie_dtype_name(f)}, not float64: cast it")
        if _is_device_tensor(f) and not f.is_cuda:
            raise ValueError(f"{name}[{key!r}] is a tensor in host memory: pass a numpy array or a device tensor")
        if not (f.flags["C_CONTIGUOUS"] if isinstance(f, np.ndarray) else f.is_contiguous()):
            raise ValueError(f"{name}[{key!r}] must be contiguous")
        fields.append(f)
    shape = tuple(fields[0].shape)
    if len(shape) != 3 or any(tuple(f.shape) != shape for f in fields):
        raise ValueError(f"'v_x', 'v_y' and 'speed' of {name} must have one common shape (pairs, x, y)")
    if shape[0] < 1 or shape[1] < 4 or shape[2] < 4:
        raise ValueError(f"{name} needs at least one pair of at least 4x4 pixels")
    if len({_is_device_tensor(f) for f in fields}) != 1:
        raise ValueError(f"the fields of {name} must be all numpy arrays or all device tensors")
    return fields


def _tensor_device(fields, device):
    """The torch device the tensors of a call share (``ValueError`` if they do not), synchronised: the library launches on its own
    stream."""
    import torch
    devices = {f.device for f in fields}
    if len(devices) != 1:
        raise ValueError("the tensors must lie on one device")
    dev = devices.pop()
    torch.cuda.synchronize(dev)
    return dev, int(device) if dev.index is None else dev.index


def filter_PIV_flow_result(flow_result, intensity_threshold=10, speed_threshold=7, *, device=0, reference_quirks=True):
    """The reference's filter of a flow result converted from PIV (OF.py:2232-2250) on the GPU, in place like the reference;
    returns ``None``.

    ``flow_result`` holds ``v_x``, ``v_y`` and ``speed`` of shape ``(T - 1, N_i, N_j)`` and ``original_data`` with ``T`` or ``T - 1``
    frames of any real dtype; the four are all numpy arrays - which keep their identity and are overwritten - or all device
    tensors, modified in place.  A field that is not float64 or not contiguous is a ``ValueError`` (cast it: a silent copy would
    not be filtered in place).

    Per sample: ``blurred`` is ``blur_movie(original_data, 3)`` restricted to the first ``T - 1`` frames, the same bits, blurred a
    chunk of frames at a time in device scratch (the last frame is not blurred at all, and no blurred stack exists);
    ``low = blurred < intensity_threshold``; ``fast = speed > S`` on the incoming ``speed``; ``v_x`` and ``v_y`` become ``0.0``
    where ``low or fast``, ``speed`` where ``fast``.  NaN compares false everywhere and is kept; ``+inf > S`` is true.
    With ``reference_quirks=True`` (the default) ``S`` is 7 whatever ``speed_threshold`` says and ``speed`` stays where only
    ``low`` holds, as in the reference; ``reference_quirks=False`` uses ``speed_threshold`` and zeroes ``speed`` under ``low`` too."""
    fields = _flow_fields("flow_result", flow_result)
    P, N_i, N_j = fields[0].shape
    try:
        movie = flow_result["original_data"]
    except KeyError:
        raise ValueError("flow_result has no 'original_data'") from None
    on_device = _is_device_tensor(fields[0])
    if _is_device_tensor(movie) != on_device or not (on_device or isinstance(movie, np.ndarray)):
        raise ValueError("'original_data' and the fields of flow_result must be all numpy arrays or all device tensors")
    if len(movie.shape) != 3 or tuple(movie.shape[1:]) != (N_i, N_j) or movie.shape[0] not in (P, P + 1):
        raise ValueError(f"'original_data' must have {P} or {P + 1} frames of {N_i} x {N_j} pixels")
    name = _movie_dtype_name(movie)
    if not name.startswith(("uint", "int", "float", "bfloat")):
        raise ValueError(f"'original_data' is {name}, not a real dtype")
    if np.isnan(float(intensity_threshold)) or np.isnan(float(speed_threshold)):
        raise ValueError("a threshold is NaN")
    limit = float(FILTER_SPEED_LIMIT if reference_quirks else speed_threshold)
    taps = gaussian_taps(FILTER_BLUR_SIGMA)
    index = _tensor_device(fields + [movie], device)[1] if on_device else device
    side = _side("torch" if on_device else "numpy", index)
    frames = side.frames(movie[:P])
    with _device_context(N_i, N_j, 1, index) as solver:
        side.wait()
        solver.flow_filter(frames, taps, P, float(intensity_threshold), limit, not reference_quirks, *fields)


def _explicit_edges(name, bins, value_range):
    """numpy's own edges of ``bins`` equal bins over an explicit ``(lo, hi)``, its widening of ``lo == hi`` included."""
    if np.ndim(value_range) != 1 or len(value_range) != 2:
        raise ValueError(f"{name} must be None or a pair (lo, hi)")
    lo, hi = float(value_range[0]), float(value_range[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"{name} must be finite with lo <= hi")
    return np.histogram_bin_edges(np.zeros(0), bins, range=(lo, hi))


def _automatic_edges(bins, lo, hi):
    """The edges ``plt.hist`` / ``plt.hist2d`` choose for samples whose extremes are ``lo`` and ``hi``: numpy's own, from the two
    values alone; an empty selection (``lo > hi``, or NaN) takes numpy's range (0, 1)."""
    if not lo <= hi:
        return np.histogram_bin_edges(np.zeros(0), bins)
    return np.histogram_bin_edges(np.array([lo, hi]), bins)


def _ground_truth_points(ground_truth, shape):
    """``(frame, start, end)`` with ``start`` and ``end`` int64 ``(n, 2)`` arrays of (x, y) inside the stack; ``ValueError`` otherwise."""
    if not isinstance(ground_truth, (tuple, list)) or len(ground_truth) != 3:
        raise ValueError("ground_truth must be (frame, start, end)")
    frame, start, end = ground_truth
    if isinstance(frame, bool) or int(frame) != frame or not 0 <= int(frame) < shape[0]:
        raise ValueError(f"ground_truth: frame must be an integer 0 .. {shape[0] - 1}")
    points = []
    for label, p in (("start", start), ("end", end)):
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f"ground_truth: {label} must be an integer (n, 2) array of (x, y) pixel positions")
        if p.size and (p.min() < 0 or p[:, 0].max() >= shape[1] or p[:, 1].max() >= shape[2]):
            raise ValueError(f"ground_truth: {label} holds a position outside the {shape[1]} x {shape[2]} image")
        points.append(p.astype(np.int64))
    if points[0].shape != points[1].shape:
        raise ValueError("ground_truth: start and end must have the same shape")
    return int(frame), points[0], points[1]


def _gather_points(field, frame, points):
    """``field[frame, x, y]`` of the ``n`` points as a host float64 vector; only the ``n`` values leave the device."""
    if isinstance(field, np.ndarray):
        return field[frame, points[:, 0], points[:, 1]]
    import torch
    index = torch.as_tensor(points, device=field.device)
    return field[frame, index[:, 0], index[:, 1]].cpu().numpy()


def compare_flow_results(flow_a, flow_b, *, speed_threshold=0.1, angle_threshold=0.5, joint_speed_bins=(50, 50),
                         joint_speed_ranges=None, angle_bins=20, angle_range=None, ground_truth=None, reference_quirks=True,
                         device=0, frames_in_flight=0):
    """What the reference's scripts do with two finished flow results, PIVlab's and Farnebäck's
    (analyse_short_timeinterval_data.py:640-745), for any two results on the GPU: the field stacks stay where they are, are
    never modified (the script overwrites the NaN speeds in its dicts) and only the summaries come back, as host numpy.

    ``flow_a`` and ``flow_b`` hold ``v_x``, ``v_y`` and ``speed`` of one common shape ``(P, N_i, N_j)``, float64 and contiguous, all
    six numpy arrays or all device tensors (``device`` names the GPU for numpy arrays).  Anything else is a ``ValueError``
    raised before the library is touched.

    Per sample, in float64, every operation explicit and in this order: ``sa``, ``sb``: the speeds with NaN replaced by 0
    (``nan_speed_counts`` of them); a sample whose ``sa`` or ``sb`` is infinite takes no part anywhere (``infinite_count``; numpy's
    automatic range would raise there); ``m1 = sa > speed_threshold and sb > speed_threshold`` - those ``joint_count`` samples go
    into ``joint_speed_histogram``, ``np.histogram2d(sa[m1], sb[m1], joint_speed_bins, joint_speed_ranges)[0]``; ``dot = v_x_b *
    v_x_a + v_y_b * v_y_a``, ``w = sb * sa``, ``cos = dot / w``, ``theta = arccos(cos)`` in radians; ``m2 = sa > angle_threshold and
    sb > angle_threshold`` - those samples go into ``angle_histogram``, ``np.histogram(theta[m2], angle_bins, angle_range)[0]``,
    except that a NaN ``theta`` is in no bin and counted in ``angle_dropped`` (numpy would raise); ``angle_count`` are the others.
    With ``reference_quirks=False`` ``cos`` is clipped to [-1, 1] first (NaN stays NaN), so a rounding excess over 1 is an angle
    of 0 instead of a dropped sample.

    A range that is ``None`` (also one axis of ``joint_speed_ranges``) is the minimum and maximum of the samples that take part,
    as ``plt.hist2d`` and ``plt.hist`` choose it: a first device pass returns the exact extremes - ``speed_extremes``, ``(2, 2)``:
    (min, max) of ``sa[m1]`` and of ``sb[m1]``; ``cos_extremes``: of ``cos`` over the ``m2`` samples with a ``theta`` - and the edges are
    numpy's own, ``np.histogram_bin_edges(np.array([lo, hi]), bins)``, for the angle with ``lo = np.arccos(cos_max)`` and ``hi =
    np.arccos(cos_min)``; no such sample: numpy's range (0, 1) and NaN extremes.  On an automatic angle range a ``theta`` outside
    the edges is counted in the first or last bin - every kept sample lies inside by construction, only the last bits of the
    device's ``acos`` could say otherwise; on an explicit one it is dropped as numpy drops it.  With every range explicit the
    first pass is skipped and the extremes are NaN.  ``joint_speed_bins``: 1 .. 1024 per axis; ``angle_bins``: 1 .. 64.

    ``ground_truth=(frame, start, end)``: integer ``(n, 2)`` arrays of (x, y) positions inside the image (no negative wrap:
    ``ValueError``); the ``v_x`` and ``v_y`` of both results at ``[frame, start[:, 0], start[:, 1]]`` are gathered and
    ``relative_errors``, ``(2, n)``, is ``sqrt((dy - v_y)**2 + (dx - v_x)**2) / sqrt(dy**2 + dx**2)`` with ``(dx, dy) = end - start``,
    formed on the host (analyse_short_timeinterval_data.py:658-666).

    Returns ``joint_speed_histogram`` (int64), ``joint_speed_edges_a``, ``joint_speed_edges_b``, ``angle_histogram`` (int64),
    ``angle_edges``, ``nan_speed_counts`` (2), ``infinite_count``, ``joint_count``, ``angle_count``, ``angle_dropped``,
    ``speed_extremes``, ``cos_extremes`` and, with ``ground_truth``, ``relative_errors``.  Integer atomics and exact extremes only:
    every summary is bit-identical from call to call and for any ``frames_in_flight`` (pairs read per launch; 0: the library's choice)."""
    a, b = _flow_fields("flow_a", flow_a), _flow_fields("flow_b", flow_b)
    shape = tuple(a[0].shape)
    if tuple(b[0].shape) != shape:
        raise ValueError("flow_a and flow_b must have the same shape (pairs, x, y)")
    stacks = a + b
    on_device = _is_device_tensor(stacks[0])
    if any(_is_device_tensor(s) != on_device for s in stacks):
        raise ValueError("flow_a and flow_b must be both numpy arrays or both device tensors")
    if np.isnan(float(speed_threshold)) or np.isnan(float(angle_threshold)):
        raise ValueError("a threshold is NaN")
    if np.ndim(joint_speed_bins) != 1 or len(joint_speed_bins) != 2:
        raise ValueError("joint_speed_bins must be a pair (bins_a, bins_b)")
    if not all(int(n) == n and 1 <= int(n) <= COMPARE_MAX_SPEED_BINS for n in joint_speed_bins):
        raise ValueError(f"joint_speed_bins must be 1 .. {COMPARE_MAX_SPEED_BINS} per axis")
    if angle_bins is None or int(angle_bins) != angle_bins or not 1 <= int(angle_bins) <= COMPARE_MAX_ANGLE_BINS:
        raise ValueError(f"angle_bins must be 1 .. {COMPARE_MAX_ANGLE_BINS}")
    if isinstance(frames_in_flight, bool) or int(frames_in_flight) != frames_in_flight or int(frames_in_flight) < 0:
        raise ValueError("frames_in_flight must be an integer >= 0")
    bins = [int(joint_speed_bins[0]), int(joint_speed_bins[1]), int(angle_bins)]
    if joint_speed_ranges is None:
        joint_speed_ranges = (None, None)
    if len(joint_speed_ranges) != 2:
        raise ValueError("joint_speed_ranges must be None or a pair of (lo, hi) or None")
    edges = [None if r is None else _explicit_edges("joint_speed_ranges", n, r) for n, r in zip(bins, joint_speed_ranges)]
    edges.append(None if angle_range is None else _explicit_edges("angle_range", bins[2], angle_range))
    truth = None if ground_truth is None else _ground_truth_points(ground_truth, shape)
    index = _tensor_device(stacks, device)[1] if on_device else device
    P, N_i, N_j = shape
    extremes = np.full((3, 2), np.nan)
    st, at, flight = float(speed_threshold), float(angle_threshold), int(frames_in_flight)
    with _device_context(N_i, N_j, 1, index) as solver:
        if any(e is None for e in edges):
            found = solver.flow_extremes(stacks, P, st, at, reference_quirks, flight)
            extremes = np.where(found[:, :1] <= found[:, 1:], found, np.nan)
            for axis in range(2):
                if edges[axis] is None:
                    edges[axis] = _automatic_edges(bins[axis], *found[axis])
            if edges[2] is None:
                with np.errstate(invalid="ignore"):                       # no sample: arccos of an infinity is NaN
                    edges[2] = _automatic_edges(bins[2], np.arccos(found[2, 1]), np.arccos(found[2, 0]))
        joint, angles, counts = solver.flow_compare(stacks, P, st, at, reference_quirks, edges[0], edges[1], edges[2],
                                                    angle_range is None, flight)
    result = dict(joint_speed_histogram=joint, joint_speed_edges_a=edges[0], joint_speed_edges_b=edges[1], angle_histogram=angles,
                  angle_edges=edges[2], nan_speed_counts=counts[:2].copy(), infinite_count=int(counts[2]), joint_count=int(counts[3]),
                  angle_count=int(counts[4]), angle_dropped=int(counts[5]), speed_extremes=extremes[:2].copy(),
                  cos_extremes=extremes[2].copy())
    if truth is not None:
        frame, start, end = truth
        d = (end - start).astype(np.float64)
        errors = np.empty((2, start.shape[0]), dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            for r, fields in enumerate((a, b)):
                v_x, v_y = _gather_points(fields[0], frame, start), _gather_points(fields[1], frame, start)
                errors[r] = np.sqrt((d[:, 1] - v_y) ** 2 + (d[:, 0] - v_x) ** 2) / np.sqrt(d[:, 1] ** 2 + d[:, 0] ** 2)
        result["relative_errors"] = errors
    return result


# ---------------------------------------------------------------------------------------------------------
# Liu-Shen physics-based flow as Jacobi iterations: the reference's third estimator, OF.py:426-673, and the wrapper
# that records its iterates, OF.py:1318-1529.
# ---------------------------------------------------------------------------------------------------------
def liu_shen_optical_flow_jit(movie, delta_x=1.0, delta_t=1.0, alpha=100, remodelling_alpha=1.0, initial_v_x=0.0,
                              initial_v_y=0.0, initial_remodelling=0.0, max_iterations=10, tolerance=1e-9,
                              include_remodelling=True, *, device=0, output="numpy"):
    """Physics-based optical flow of Liu and Shen without remodelling, exactly ``max_iterations`` Jacobi iterations per
    frame pair on one MI355X; positional arguments and the returned 5-tuple
    ``(v_x, v_y, speed, remodelling, max_iterations - 1)`` as OF.py:426-673.

    Pair ``k`` uses ``p`` = frame ``k`` and ``c`` = frame ``k + 1`` (float64, mirrored over the image edge: row -1 = row 1)
    and starts from ``initial_v_x * delta_t / delta_x``, ``initial_v_y * delta_t / delta_x``; there is no warm start
    between pairs.  Every iteration updates every pixel from the old iterate: the right-hand side of OF.py:621-630 (central
    differences and ``v[i+1] + v[i-1]`` read the mirrored border, the 8-neighbour sums take neighbours outside the image
    as zero) and the inverse of the pixel's constant 2 x 2 block, whose diagonal holds ``-n * alpha`` with ``n`` = 8 in the
    interior, 5 on an edge line and 3 in a corner.  The velocities come back times ``delta_x / delta_t``, ``speed`` is their
    norm, ``remodelling`` the initial one, untouched.  ``remodelling_alpha``, ``tolerance`` and ``include_remodelling``
    are accepted and ignored, as in the reference.

    Deviations from the reference: the initial fields may be scalars, ``(N_i, N_j)`` planes or ``(T-1, N_i, N_j)`` stacks
    and default to 0.0 (the reference's 10 x 10 default arrays cannot broadcast); ``max_iterations < 1`` and an image side
    below 3 raise ``ValueError`` (the device context itself needs sides of at least 4); a singular 2 x 2 block stores what
    IEEE division gives where the reference's ``numpy.linalg.inv`` raises.  The inverse is the closed form, so results
    agree with the reference to rounding, not bit for bit.

    Keyword-only extras: ``device``, ``output`` ("numpy", or "torch": ``movie`` and the initial fields may be device
    tensors and the four arrays come back as float64 device tensors)."""
    side = _side(output, device)
    T, N_i, N_j = _movie_shape(movie, 2)
    if min(N_i, N_j) < 3:
        raise ValueError("the Liu-Shen flow needs image sides of at least 3")
    if int(max_iterations) < 1:
        raise ValueError("max_iterations must be >= 1")
    pairs = (T - 1, N_i, N_j)
    frames = side.frames(movie)
    # a Python float must not pass through torch's default float32
    initial = [side.frames(f if _is_device_tensor(f) else np.asarray(f, dtype=np.float64))
               for f in (initial_v_x, initial_v_y, initial_remodelling)]
    initial, kind = _native.liu_shen_initial(initial, pairs)
    out = [side.empty(pairs) for _ in range(4)]
    with _device_context(N_i, N_j, 1, device) as solver:
        side.wait()
        solver.liu_shen(frames, T, delta_x, delta_t, alpha, *initial, kind, int(max_iterations), *out)
    return (*out, int(max_iterations) - 1)


def conduct_variational_optical_flow_deprecated(movie, delta_x=1.0, delta_t=1.0, speed_alpha=1.0, remodelling_alpha=1000.0,
                                                v_x_guess=0.1, v_y_guess=0.1, remodelling_guess=0.5, max_iterations=10,
                                                smoothing_sigma=None, return_iterations=False, iteration_stepsize=1,
                                                tolerance=1e-10, include_remodelling=True, use_liu_shen=False, *,
                                                device=0, output="numpy"):
    """The reference's wrapper around ``liu_shen_optical_flow_jit`` that can record the iterates; signature and result
    dict as OF.py:1318-1529.  ``use_liu_shen=False`` raises the reference's ``ValueError``.

    Returns ``v_x``, ``v_y``, ``speed``, ``remodelling`` (float64 ``(T-1, N_i, N_j)``), ``original_data``,
    ``blurred_data``, ``delta_x``, ``delta_t``, ``max_iterations``, ``total_iterations`` and, with ``return_iterations``,
    ``v_x_steps``, ``v_y_steps``, ``speed_steps``, ``remodelling_steps`` of shape
    ``(T-1, max_iterations // iteration_stepsize + 1, N_i, N_j)`` plus ``iteration_stepsize``.  Record 0 holds the guesses;
    record ``r`` is produced as the reference does: a fresh call of ``iteration_stepsize`` iterations that starts from
    record ``r - 1``, so the fields make the round trip through ``delta_x / delta_t`` and back between records, and the
    final fields are the last record (``max_iterations`` rounded down to a multiple of ``iteration_stepsize``).

    Deviations from the reference, whose wrapper cannot run as written: it unpacks 4 of the function's 5 return values -
    here all 5 are unpacked; its restart passes the ``(T-1, N_i, N_j)`` result as the initial field of every pair, which
    cannot broadcast for more than one pair - here the restart is per pair (pair ``k`` restarts from its own record);
    ``total_iterations`` is ``max_iterations`` also without ``return_iterations`` (undefined there); an
    ``iteration_stepsize`` outside ``1 .. max_iterations`` raises ``ValueError``; nothing is printed.

    Keyword-only extras: ``device``, ``output`` ("numpy", or "torch": every array of the result stays on the device)."""
    if not use_liu_shen:
        raise ValueError("I can currently only really do this for the liu shen jitted method")
    side = _side(output, device)
    _movie_shape(movie, 0)
    if return_iterations and not 1 <= int(iteration_stepsize) <= int(max_iterations):
        raise ValueError("iteration_stepsize must be between 1 and max_iterations")
    movie_to_analyse = movie
    if smoothing_sigma is not None:
        if output == "torch":
            with _device_context(movie.shape[1], movie.shape[2], 1, device) as solver:
                movie_to_analyse = side.blurred(side.frames(movie), gaussian_taps(smoothing_sigma), solver)
        else:
            movie_to_analyse = blur_movie(np.asarray(movie), smoothing_sigma=smoothing_sigma, device=device)
    guesses = (float(v_x_guess), float(v_y_guess), float(remodelling_guess))

    def flow(initial, iterations):
        return liu_shen_optical_flow_jit(movie_to_analyse, delta_x, delta_t, speed_alpha, remodelling_alpha, *initial,
                                         max_iterations=iterations, tolerance=tolerance,
                                         include_remodelling=include_remodelling, device=device, output=output)

    result = dict()
    if return_iterations:
        stepsize = int(iteration_stepsize)
        records = int(max_iterations) // stepsize
        this = flow(guesses, stepsize)
        steps = [f.new_zeros((f.shape[0], records + 1) + tuple(f.shape[1:])) if output == "torch"
                 else np.zeros((f.shape[0], records + 1) + f.shape[1:]) for f in this[:4]]
        steps[0][:, 0], steps[1][:, 0], steps[3][:, 0] = guesses
        steps[2][:, 0] = float(np.sqrt(np.float64(guesses[0]) ** 2 + np.float64(guesses[1]) ** 2))
        for record in range(1, records + 1):
            if record > 1:
                this = flow((this[0], this[1], this[3]), stepsize)
            for f in range(4):
                steps[f][:, record] = this[f]
        result["v_x"], result["v_y"], result["speed"], result["remodelling"] = (s[:, -1] for s in steps)
        result["v_x_steps"], result["v_y_steps"], result["speed_steps"], result["remodelling_steps"] = steps
        result["iteration_stepsize"] = iteration_stepsize
    else:
        result["v_x"], result["v_y"], result["speed"], result["remodelling"] = flow(guesses, max_iterations)[:4]
    result["original_data"] = movie
    result["delta_x"] = delta_x
    result["delta_t"] = delta_t
    result["blurred_data"] = movie_to_analyse
    result["max_iterations"] = max_iterations
    result["total_iterations"] = max_iterations
    return result


def vary_regularisation(movie,
                        speed_alpha_values=np.arange(500, 2000, 500),
                        remodelling_alpha_values=np.arange(500, 2000, 500),
                        filename=None,
                        **kwargs):
    """Vary both regularisation parameters and keep the summary statistics for heat-maps; same arguments,
    result dictionary and optional ``np.save`` as the reference (OF.py:1918-1998).  ``kwargs`` are the keyword
    arguments of ``variational_optical_flow`` (OF.py:1974-1977).

    Every ``(speed_alpha, remodelling_alpha)`` combination is an independent solve of the same movie.  The whole sweep
    is one native call (``vof_vary_regularisation_host``): the movie is uploaded and blurred once, each combination
    batches all frame pairs, and ``np.mean`` / ``np.var`` of the speed and remodelling stacks (OF.py:1978-1981) are
    two-pass reductions on the device, so only the summary scalars cross PCIe.

    Returns a dict with ``speed_alpha_values``, ``remodelling_alpha_values``, ``speed_means``,
    ``speed_variances``, ``remodelling_means``, ``remodelling_variances``, ``converged`` and ``functional``
    (``L1_functional + speed_functional + remodelling_functional``, OF.py:1983), each of shape
    ``(len(speed_alpha_values), len(remodelling_alpha_values))``.  Extra keyword: ``return_stats=True`` adds
    ``result['stats']`` (the native per-combination records: worst residual / iteration count, all-pairs flag).
    """
    movie = np.asarray(movie)
    T, N_i, N_j = _movie_shape(movie, 2)
    kw = dict(delta_x=1.0, delta_t=1.0, smoothing_sigma=None, initial_v_x=0.0, initial_v_y=0.0, initial_remodelling=0.0,
              use_direct_solver=False, rtol=None, max_iterations=1000, reference_quirks=True, device=0,
              max_pairs_in_flight=None, coarse_precision="float8", vcycle_precision="coarse_float32", multigrid_sweeps=None,
              w_cycle_level=None, krylov_method="auto", gmres_restart=None, warm_start_stride=None, preconditioner=None,
              verbose=False, return_stats=False)
    for k in kwargs:
        if k not in kw:
            raise TypeError(f"variational_optical_flow() got an unexpected keyword argument {k!r}")
    kw.update(kwargs)
    params = _solver_params(1.0, 1.0, kw["delta_x"], kw["delta_t"], kw["initial_v_x"], kw["initial_v_y"],
                            kw["initial_remodelling"], kw["use_direct_solver"], kw["rtol"], kw["max_iterations"],
                            kw["reference_quirks"], kw["coarse_precision"], kw["vcycle_precision"],
                            kw["multigrid_sweeps"], kw["w_cycle_level"], kw["krylov_method"], kw["gmres_restart"],
                            kw["warm_start_stride"], kw["preconditioner"])   # warm_start_stride: accepted for signature parity
    taps = None if kw["smoothing_sigma"] is None else gaussian_taps(kw["smoothing_sigma"])
    # short movies: several combinations share one batch as "virtual pairs" (see vof_vary_regularisation_host)
    n_comb = max(1, len(speed_alpha_values) * len(remodelling_alpha_values))
    pairs = kw["max_pairs_in_flight"] or choose_pairs_in_flight(N_i, N_j, (T - 1) * n_comb, kw["device"], params=params)
    with _device_context(N_i, N_j, pairs, kw["device"], kw["max_pairs_in_flight"] is not None) as solver:
        try:
            rec = solver.vary_regularisation_host(movie.astype(np.float64), params, speed_alpha_values,
                                                  remodelling_alpha_values, taps)
        except _native.VofError as exc:
            if not (kw["use_direct_solver"] and kw["preconditioner"] is None and _direct_unavailable(exc)):
                raise
            params.preconditioner = 2
            rec = solver.vary_regularisation_host(movie.astype(np.float64), params, speed_alpha_values,
                                                  remodelling_alpha_values, taps)
    if kw["verbose"]:
        for i, a in enumerate(speed_alpha_values):
            for j, b in enumerate(remodelling_alpha_values):
                print(f"speed_alpha {a}, remodelling_alpha {b}: max iterations {rec['max_iterations_used'][i, j]}, "
                      f"max relative residual {rec['max_relative_residual'][i, j]:.3e}, "
                      f"all converged {bool(rec['converged_all'][i, j])}")
    # OF.py:1205 stores the remodelling sum under 'speed_functional'; OF.py:1983 adds the three dict entries
    speed_functional = rec["remodelling_functional"] if kw["reference_quirks"] else rec["speed_functional"]
    result_dict = {}
    result_dict["speed_alpha_values"] = speed_alpha_values
    result_dict["remodelling_alpha_values"] = remodelling_alpha_values
    result_dict["speed_means"] = rec["speed_mean"].copy()
    result_dict["speed_variances"] = rec["speed_variance"].copy()
    result_dict["remodelling_means"] = rec["remodelling_mean"].copy()
    result_dict["remodelling_variances"] = rec["remodelling_variance"].copy()
    result_dict["converged"] = rec["converged_last"].astype(bool)       # OF.py:1982: flag of the last pair
    result_dict["functional"] = rec["L1_functional"] + speed_functional + rec["remodelling_functional"]
    if kw["return_stats"]:
        result_dict["stats"] = rec
    if filename is not None:
        np.save(filename, result_dict)
    return result_dict


# ---------------------------------------------------------------------------------------------------------
# Result consumers: the steps the reference's scripts run right after the solve.
# ---------------------------------------------------------------------------------------------------------
def subsample_velocities_for_visualisation(flow_result, iteration=None, arrow_boxsize=5):
    """Arrow positions and velocities for ``plt.quiver``, same arguments and return values as OF.py:1574-1646:
    one sample per ``arrow_boxsize`` x ``arrow_boxsize`` box, taken at pixel ``box_index * arrow_boxsize +
    round(arrow_boxsize / 2)`` (Python's ``round``, i.e. half-to-even, as in the reference); positions are in
    ``delta_x`` units.  Returns ``(x_positions, y_positions, v_x, v_y)`` with the velocities of shape
    ``(T-1, N_i // arrow_boxsize, N_j // arrow_boxsize)``.

    A device-resident result (``output="torch"``) is sampled by a HIP gather kernel and only the
    ``1 / arrow_boxsize^2`` samples cross PCIe.  ``iteration`` selects ``'v_x_steps'`` / ``'v_y_steps'`` entries
    (OF.py:1621-1625), which only the reference's iterative legacy solvers produce."""
    box = int(arrow_boxsize)
    if box < 1:
        raise ValueError("arrow_boxsize must be >= 1")
    offset = round(arrow_boxsize / 2)
    if iteration is not None:
        fields = [flow_result["v_x_steps"][:, iteration], flow_result["v_y_steps"][:, iteration]]
    else:
        fields = [flow_result["v_x"], flow_result["v_y"]]
    n_pairs = flow_result["original_data"].shape[0] - 1
    n_x, n_y = fields[0].shape[1], fields[1].shape[2]
    nbx, nby = n_x // box, n_y // box
    if hasattr(fields[0], "data_ptr") and fields[0].is_cuda:
        side, sub = _DeviceSide(fields[0].device.index), []
        with _device_context(n_x, n_y, 1, fields[0].device.index) as solver:
            for f in fields:
                out = side.empty((n_pairs, nbx, nby))
                side.wait()
                solver.subsample_dev(f[:n_pairs].contiguous(), n_pairs, box, offset, out)
                sub.append(out.cpu().numpy())
    else:
        sub = [np.array(np.asarray(f)[:n_pairs, offset:offset + (nbx - 1) * box + 1:box,
                                      offset:offset + (nby - 1) * box + 1:box], dtype=np.float64)
               if nbx and nby else np.zeros((n_pairs, nbx, nby)) for f in fields]
    delta_x = flow_result["delta_x"]
    x_positions = (np.arange(nbx) * box + offset).astype(float) / n_x * (n_x * delta_x)
    y_positions = (np.arange(nby) * box + offset).astype(float) / n_y * (n_y * delta_x)
    return x_positions, y_positions, sub[0], sub[1]


def costum_imshow(image, delta_x, cmap="gray_r", autoscale=False, v_min=0.0, v_max=255.0, unit=r"$\mathrm{\mu}$m"):
    """Show an image without anti-aliasing, axes in physical units (same name, arguments and look as OF.py:1531-1572;
    the figure / axes are created by the caller)."""
    import matplotlib.pyplot as plt
    limits = dict(vmin=None, vmax=None) if autoscale else dict(vmin=v_min, vmax=v_max)
    extent = [0, image.shape[1] * delta_x, image.shape[0] * delta_x, 0]
    plt.imshow(image, cmap=cmap, extent=extent, interpolation=None, **limits)
    plt.xlabel("y-position [" + unit + "]")
    plt.ylabel("x-position [" + unit + "]")


def _quiver(x_positions, y_positions, v_x, v_y, arrow_color, arrow_scale, arrow_width):
    # image rows run downwards: plot (y, x) with the x-velocity flipped (OF.py:1695)
    import matplotlib.pyplot as plt
    plt.quiver(y_positions, x_positions, v_y, -v_x, color=arrow_color, headwidth=5, scale=1.0 / arrow_scale,
               width=arrow_width)


def make_velocity_overlay_movie(flow_result, filename, arrow_boxsize=5, arrow_scale=1.0, cmap="gray_r", autoscale=False,
                                arrow_color="magenta", arrow_width=None, v_min=0.0, v_max=255.0, dpi=600):
    """Movie of the data with the flow arrows on top; arguments as OF.py:1649-1700 (``dpi`` is an extra)."""
    import matplotlib.pyplot as plt
    from matplotlib.animation import FuncAnimation
    movie = flow_result["original_data"]
    xs, ys, v_x, v_y = subsample_velocities_for_visualisation(flow_result, arrow_boxsize=arrow_boxsize)
    fig = plt.figure(figsize=(2.5, 2.5))

    def animate(i):
        plt.cla()
        costum_imshow(movie[i + 1], delta_x=flow_result["delta_x"], cmap=cmap, autoscale=autoscale, v_min=v_min, v_max=v_max)
        _quiver(xs, ys, v_x[i], v_y[i], arrow_color, arrow_scale, arrow_width)
        if i < 1:
            plt.tight_layout()
    FuncAnimation(fig, animate, frames=movie.shape[0] - 1).save(filename, dpi=dpi)
    plt.close(fig)


def make_joint_overlay_movie(flow_result, filename, arrow_boxsize=5, arrow_scale=1.0, arrow_width=None, cmap="gray_r",
                             autoscale=False, arrow_color="magenta", v_min=0.0, v_max=255.0, dpi=600):
    """Six-panel movie: data and blurred data with arrows, speed, net remodelling, v_x, v_y; arguments as
    OF.py:1825-1916 (``dpi`` is an extra)."""
    import matplotlib.pyplot as plt
    import matplotlib.ticker
    from matplotlib.animation import FuncAnimation
    xs, ys, v_x, v_y = subsample_velocities_for_visualisation(flow_result, arrow_boxsize=arrow_boxsize)
    dx = flow_result["delta_x"]
    data_panels = [(231, "original_data", "Original data"), (232, "blurred_data", "Blurred")]
    field_panels = [(233, "speed", "viridis", r"Motion speed [$\mathrm{\mu m}$/s]", False),
                    (234, "remodelling", "plasma", "Net remodelling", False),
                    (235, "v_x", "plasma", r"x velocity [$\mathrm{\mu m}$/s]", True),
                    (236, "v_y", "plasma", r"y velocity [$\mathrm{\mu m}$/s]", False)]
    ranges = {key: (np.min(flow_result[key]), np.max(flow_result[key])) for _, key, _, _, _ in field_panels}
    fig = plt.figure(figsize=(6.5, 4.5), constrained_layout=True)

    def animate(i):
        plt.clf()
        for pos, key, title in data_panels:
            plt.subplot(pos)
            costum_imshow(flow_result[key][i], delta_x=dx, cmap=cmap, autoscale=autoscale, v_min=v_min, v_max=v_max)
            _quiver(xs, ys, v_x[i], v_y[i], arrow_color, arrow_scale, arrow_width)
            plt.title(title)
        for pos, key, field_cmap, title, keep_ylabel in field_panels:
            plt.subplot(pos)
            costum_imshow(flow_result[key][i], delta_x=dx, autoscale=True, cmap=field_cmap)
            if not keep_ylabel:
                plt.ylabel("")
            colorbar = plt.colorbar(shrink=0.6)
            plt.clim(*ranges[key])
            colorbar.formatter = matplotlib.ticker.StrMethodFormatter("{x:.2f}")
            plt.title(title)
    FuncAnimation(fig, animate, frames=flow_result["original_data"].shape[0] - 1).save(filename, dpi=dpi)
    plt.close(fig)
