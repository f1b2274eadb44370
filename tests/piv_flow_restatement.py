"""numpy restatement of conduct_piv (vof_piv_flow_*, csrc/vof_pivflow.hpp) and the cases its tests share.

Direct zero-normalised cross-correlation PIV, multi-pass with integer window offsets from the pass before, float64, every operation
single.  Every window sum is two-level - a window row left to right from 0.0, the row sums top to bottom from 0.0, products rounded
before they are added; ``np.cumsum`` adds in sequence, so ``cumsum([0.0, ...])[-1]`` is that sum.  ``ordered=False`` sums with
``np.sum`` instead (pairwise): on integer-valued movies whose sums stay below 2^53 the two must agree bit for bit.

``piv(movie, window_sizes, search_radii, steps, min_correlation)`` returns ``(u, v, correlation, counts, details)``: the last pass
as ``(pairs, R, C)`` arrays, ``counts[pass] = (flat, border, below threshold)``, and per pass and pair the arrays of ``details``:
``peak`` (R, C, 2) the integer peak ``(d_i, d_j)``, ``offset`` (R, C, 2), ``gap`` (R, C) the difference of the two highest
correlations of the window (NaN for a flat window) and ``surface`` (R, C, D, D) the correlation values."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

NAN = float("nan")


def grid(shape, window_sizes, search_radii, steps):
    """Per pass ``dict(w, r, s, m, R, C)``: the margin ``m_p = r_0 + ... + r_p`` and the grid ``R_p = (N_i - w_p - 2 m_p) // s_p + 1``."""
    passes, m = [], 0
    for w, r, s in zip(window_sizes, search_radii, steps):
        m += r
        R, C = (shape[0] - w - 2 * m) // s + 1, (shape[1] - w - 2 * m) // s + 1
        assert R >= 1 and C >= 1
        passes.append(dict(w=int(w), r=int(r), s=int(s), m=int(m), R=int(R), C=int(C)))
    return passes


def seq_sum(x, ordered=True):
    """The sum over the last axis, left to right from 0.0 (``ordered``), or numpy's own."""
    if not ordered:
        return np.sum(x, axis=-1)
    return np.cumsum(np.concatenate([np.zeros(x.shape[:-1] + (1,)), x], axis=-1), axis=-1)[..., -1]


def window_sum(x, ordered=True):
    """The two-level sum over the last two axes: rows left to right, then the row sums top to bottom."""
    if not ordered:
        return np.sum(x, axis=(-2, -1))
    return seq_sum(seq_sum(x))


def surface(A, B, ordered=True):
    """The correlation values C[d_i, d_j] of the ``w x w`` window ``A`` over the ``(w + 2 r)``-square region ``B``, or None for a flat
    window (``!(D_a > 0)``)."""
    w = A.shape[0]
    n = float(w * w)
    S_a, S_aa = window_sum(A, ordered), window_sum(A * A, ordered)
    D_a = n * S_aa - S_a * S_a
    if not D_a > 0:
        return None
    if ordered:
        rows = sliding_window_view(B, w, axis=1)                              # [y, d_j, j]
        rb, rbb = seq_sum(rows), seq_sum(rows * rows)                         # [y, d_j]: formed once, shared by every d_i
        S_b = seq_sum(sliding_window_view(rb, w, axis=0))                     # [d_i, d_j, i] -> [d_i, d_j]
        S_bb = seq_sum(sliding_window_view(rbb, w, axis=0))
    else:
        windows = sliding_window_view(B, (w, w))
        S_b, S_bb = window_sum(windows, False), window_sum(windows * windows, False)
    windows = sliding_window_view(B, (w, w))                                  # [d_i, d_j, i, j]
    S_ab = np.stack([window_sum(windows[d] * A, ordered) for d in range(windows.shape[0])])
    D_b = n * S_bb - S_b * S_b
    with np.errstate(invalid="ignore", divide="ignore"):
        C = (n * S_ab - S_a * S_b) / np.sqrt(D_a * D_b)
    return np.where(D_b > 0, C, -np.inf)


def parabola(cm, c0, cp):
    if not (np.isfinite(cm) and np.isfinite(cp)):
        return 0.0
    den = 2.0 * ((cm - 2.0 * c0) + cp)
    return (cm - cp) / den if den < 0 else 0.0


def previous_index(at, w, q, n):
    """``clamp((2 (i0 - m') + w - w' + s') // (2 s'), 0, n - 1)``: the window of the pass before nearest to this one's centre."""
    return min(max((2 * (at - q["m"]) + w - q["w"] + q["s"]) // (2 * q["s"]), 0), n - 1)


def piv_pair(first, second, passes, min_correlation=None, ordered=True):
    """One frame pair through every pass: ``(u, v, correlation)`` of the last pass, ``counts`` and the details per pass."""
    counts = np.zeros((len(passes), 3), dtype=np.int64)
    details, u, v = [], None, None
    for k, p in enumerate(passes):
        w, r, s, m, R, C = (p[key] for key in ("w", "r", "s", "m", "R", "C"))
        D = 2 * r + 1
        pu, pv = u, v                                                        # the vectors of the pass before
        u, v, corr = (np.full((R, C), NAN) for _ in range(3))
        det = dict(peak=np.zeros((R, C, 2), dtype=np.int64), offset=np.zeros((R, C, 2), dtype=np.int64), gap=np.full((R, C), NAN),
                   surface=np.full((R, C, D, D), NAN))
        for a in range(R):
            for b in range(C):
                i0, j0 = m + a * s, m + b * s
                o_i = o_j = 0
                if k:
                    q = passes[k - 1]
                    ap, bp = previous_index(i0, w, q, q["R"]), previous_index(j0, w, q, q["C"])
                    if not (np.isnan(pu[ap, bp]) or np.isnan(pv[ap, bp])):
                        o_i, o_j = int(np.floor(pv[ap, bp] + 0.5)), int(np.floor(pu[ap, bp] + 0.5))
                    assert abs(o_i) <= q["m"] and abs(o_j) <= q["m"]
                det["offset"][a, b] = o_i, o_j
                top, left = i0 + o_i - r, j0 + o_j - r
                assert top >= 0 and left >= 0 and top + w + 2 * r <= first.shape[0] and left + w + 2 * r <= first.shape[1]
                Cd = surface(first[i0:i0 + w, j0:j0 + w], second[top:top + w + 2 * r, left:left + w + 2 * r], ordered)
                if Cd is None:
                    counts[k, 0] += 1
                    continue
                det["surface"][a, b] = Cd
                at = int(np.argmax(Cd))                                      # the first maximum in raster order
                c0 = Cd.ravel()[at]
                corr[a, b] = c0
                if c0 == -np.inf:
                    counts[k, 0] += 1
                    continue
                p_i, p_j = divmod(at, D)
                det["peak"][a, b] = p_i - r, p_j - r
                ranked = np.sort(Cd.ravel())
                det["gap"][a, b] = ranked[-1] - ranked[-2]
                delta_i = parabola(Cd[p_i - 1, p_j], c0, Cd[p_i + 1, p_j]) if 0 < p_i < D - 1 else 0.0
                delta_j = parabola(Cd[p_i, p_j - 1], c0, Cd[p_i, p_j + 1]) if 0 < p_j < D - 1 else 0.0
                if p_i in (0, D - 1) or p_j in (0, D - 1):
                    counts[k, 1] += 1
                v[a, b] = float(o_i + p_i - r) + delta_i
                u[a, b] = float(o_j + p_j - r) + delta_j
                if min_correlation is not None and c0 < min_correlation:
                    u[a, b] = v[a, b] = NAN
                    counts[k, 2] += 1
        details.append(det)
    return u, v, corr, counts, details


def piv(movie, window_sizes, search_radii, steps, min_correlation=None, ordered=True):
    frames = np.asarray(movie, dtype=np.float64)
    passes = grid(frames.shape[1:], window_sizes, search_radii, steps)
    pairs = [piv_pair(frames[k], frames[k + 1], passes, min_correlation, ordered) for k in range(frames.shape[0] - 1)]
    u, v, corr = (np.stack([pr[f] for pr in pairs]) for f in range(3))
    counts = sum(pr[3] for pr in pairs)
    details = [[pr[4][p] for pr in pairs] for p in range(len(passes))]       # [pass][pair]
    return u, v, corr, counts, details


# ---- the cases: the smallest at which the kernels can go wrong ------------------------------------------------------------------------
def _moved(canvas, shape, shifts, margin):
    """Frames of ``shape`` cut from ``canvas``: frame k shows the content of frame 0 moved by the sum of the first k ``shifts``."""
    frames, at = [], np.array([margin, margin])
    for shift in [(0, 0)] + list(shifts):
        at = at - np.asarray(shift)
        frames.append(canvas[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]])
    return np.stack(frames)


def _smooth_uint8(rng, shape, sigma):
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(rng.standard_normal(shape), sigma)
    return np.clip(np.rint(128 + 100 * f / np.abs(f).max()), 0, 255).astype(np.uint8)


def _texture(n, shape, frames, seed, shift):
    from opticalflow_amd import synthetic
    return np.ascontiguousarray(synthetic.texture_stack_numpy(n, frames, seed=seed, shift=shift)[:, :shape[0], :shape[1]])


def _integer_shift():
    canvas = np.random.default_rng(201).integers(0, 256, (60, 72)).astype(np.uint8)
    return dict(movie=_moved(canvas, (40, 52), [(2, -1), (-1, 2)], 10), passes=[(8, 3, 4)])


def _odd_edges():
    canvas = _smooth_uint8(np.random.default_rng(202), (57, 65), 1.2)
    return dict(movie=_moved(canvas, (37, 45), [(1, -1), (0, 1), (-1, 1)], 10), passes=[(10, 2, 7)])


def _float_blurred():
    return dict(movie=_texture(50, (41, 50), 3, 7, (1.4, -0.7)), passes=[(12, 3, 5)])


FLAT_TIES_TIED = [(a, b) for a in range(5) for b in (4, 5, 6)]               # the windows that lie in the periodic part


def _flat_ties_border():
    """48 x 64, one pair, w = 8, r = 3, s = 8: windows at 3 + 8 a.  Columns [0, 32): smooth integer texture moved 5 pixels along the
    columns, beyond r (border peaks); its window (0, 0) constant in the first frame (flat).  Columns [32, 64): a pattern of period 4
    on both axes moved by (1, 1): d and d + 4 tie exactly in the windows FLAT_TIES_TIED, and (-3, -3) is the first in raster order."""
    canvas = _smooth_uint8(np.random.default_rng(204), (68, 84), 2.0)
    movie = _moved(canvas, (48, 64), [(0, 5)], 10).copy()
    tile = np.random.default_rng(205).integers(0, 256, (4, 4)).astype(np.uint8)
    i, j = np.meshgrid(np.arange(48), np.arange(32), indexing="ij")
    movie[0, :, 32:] = tile[i % 4, j % 4]
    movie[1, :, 32:] = tile[(i - 1) % 4, (j - 1) % 4]
    movie[0, 3:11, 3:11] = 77
    return dict(movie=movie, passes=[(8, 3, 8)])


TWO_PASS_FLAT = (0, 0)                                                       # the pass-0 window made constant in the first frame


def _two_pass():
    """96 x 80, passes (32, 6, 16) and (16, 2, 8), the texture moved by (2.3, -3.6).  The pass-0 window (0, 0), rows and columns
    [6, 38), is constant in the first frame, so its vector is NaN and the four pass-1 windows that look it up take the offset 0.
    The block moves with the texture, by (2, -4) to the second frame: the windows that reach into it still find their peak."""
    movie = _texture(96, (96, 80), 2, 3, (2.3, -3.6))
    movie[0, 6:38, 6:38] = 0.5
    movie[1, 8:40, 2:34] = 0.5
    return dict(movie=movie, passes=[(32, 6, 16), (16, 2, 8)])


def _largest():
    return dict(movie=_texture(112, (96, 112), 2, 5, (3.3, -7.4)), passes=[(64, 16, 16)])


def _thresholded():
    """The float texture, the right half of the second and third frame under noise: the correlation falls there."""
    movie = _texture(50, (41, 50), 3, 7, (1.4, -0.7))
    movie[1:, :, 25:] += 0.25 * np.random.default_rng(207).standard_normal((2, 41, 25))
    return dict(movie=movie, passes=[(12, 3, 5)], min_correlation=0.6)


MAKERS = dict(integer_shift=_integer_shift, odd_edges=_odd_edges, float_blurred=_float_blurred, flat_ties_border=_flat_ties_border,
              two_pass=_two_pass, largest=_largest, thresholded=_thresholded)
CASES = tuple(MAKERS)
INTEGER_CASES = ("integer_shift", "odd_edges", "flat_ties_border")


@functools.lru_cache(maxsize=None)
def case(name):
    """``dict(movie, window_sizes, search_radii, steps, min_correlation)``; made once and shared: leave it unchanged."""
    c = MAKERS[name]()
    w, r, s = (tuple(p[k] for p in c["passes"]) for k in range(3))
    c["movie"].setflags(write=False)
    return dict(movie=c["movie"], window_sizes=w, search_radii=r, steps=s, min_correlation=c.get("min_correlation"))


@functools.lru_cache(maxsize=None)
def restated(name, ordered=True):
    """``piv`` of the case, computed once and shared: leave it unchanged."""
    c = case(name)
    return piv(c["movie"], c["window_sizes"], c["search_radii"], c["steps"], c["min_correlation"], ordered)
