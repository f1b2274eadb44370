"""numpy restatement of conduct_piv's window deformation and outlier validation between passes (vof_piv_flow_ex_*,
csrc/vof_pivflow.hpp, DESIGN.md sections 20.7 to 20.9) and the cases its tests share.  It builds on tests/piv_flow_restatement.py, which
it imports and leaves as it is: the sums, the correlation values, the peak and the subpixel fit are that module's.

float64, every operation single, only ``+ - * / sqrt floor fabs fmin fmax``:

* ``validate``: the normalised median test of Westerweel & Scarano (2005), Jacobi style, medians through ``SORT8``, the fixed
  sorting network of the kernel (a comparator exchanges only where ``y < x``, absent neighbours are +inf);
* ``predictor``: the vectors of the pass before, bilinear between window centres, clamped outside, a missing vector as (0, 0);
* ``warped``: frame ``k + 1`` sampled bilinearly at ``(i + V(i, j), j + U(i, j))`` - the search region of a deformed pass is a slice
  of it, since a sample is a function of its pixel alone.

``piv(movie, window_sizes, search_radii, steps, min_correlation, deformation, outlier_threshold, outlier_epsilon, validate_last)``
returns ``(u, v, correlation, counts, validation_counts, details)``; ``details[pass][pair]`` holds ``peak``, ``offset``, ``gap``,
``surface`` as in piv_flow_restatement, ``region_at`` (R, C, 2) the top-left pixel of the search region, ``base`` (R, C, 2) what is added
to ``d + delta`` as ``(along rows, along columns)``, ``second`` the frame the regions are cut from, and - where the vectors of the
pass were validated - ``validation``: ``dict(u, v, neighbours, action, ratio)`` with ``action`` 0 kept, 1 outlier, 2 filled, -1 fewer
than three neighbours."""
import functools

import numpy as np

import piv_flow_restatement as pf

NAN = float("nan")
INF = float("inf")

# the 19 comparators of the 8-input sorting network the kernel uses
SORT8 = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (1, 2), (5, 6), (0, 4), (3, 7), (1, 5), (2, 6), (1, 4), (3, 6),
         (2, 4), (3, 5), (3, 4))
KEPT, OUTLIER, FILLED, TOO_FEW = 0, 1, 2, -1


def sorted8(values):
    s = list(values)
    for x, y in SORT8:
        if s[y] < s[x]:
            s[x], s[y] = s[y], s[x]
    return s


def median8(values, k):
    """The median of the ``k`` finite entries among the eight ``values``, the others being +inf."""
    s = sorted8(values)
    return s[(k - 1) // 2] if k % 2 else (s[k // 2 - 1] + s[k // 2]) * 0.5


def validate(u, v, threshold, epsilon):
    """One grid ``(R, C)`` of vectors: ``(u, v, outliers, filled, record)``."""
    R, C = u.shape
    valid = ~(np.isnan(u) | np.isnan(v))
    out_u, out_v = u.copy(), v.copy()
    record = dict(neighbours=np.zeros((R, C), dtype=np.int64), action=np.zeros((R, C), dtype=np.int64), ratio=np.full((R, C, 2), NAN))
    outliers = filled = 0
    for a in range(R):
        for b in range(C):
            un, vn, k = [], [], 0
            for da in (-1, 0, 1):
                for db in (-1, 0, 1):
                    aa, bb = a + da, b + db
                    if (da or db):
                        there = 0 <= aa < R and 0 <= bb < C and valid[aa, bb]
                        un.append(float(u[aa, bb]) if there else INF)
                        vn.append(float(v[aa, bb]) if there else INF)
                        k += bool(there)
            record["neighbours"][a, b] = k
            if k < 3:
                record["action"][a, b] = TOO_FEW
                continue
            u_m, v_m = median8(un, k), median8(vn, k)
            if not valid[a, b]:
                out_u[a, b], out_v[a, b] = u_m, v_m
                record["action"][a, b] = FILLED
                filled += 1
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                r_u = np.float64(abs(u[a, b] - u_m)) / np.float64(median8([abs(x - u_m) if x < INF else INF for x in un], k) + epsilon)
                r_v = np.float64(abs(v[a, b] - v_m)) / np.float64(median8([abs(x - v_m) if x < INF else INF for x in vn], k) + epsilon)
            record["ratio"][a, b] = r_u, r_v
            if r_u > threshold or r_v > threshold:
                out_u[a, b], out_v[a, b] = u_m, v_m
                record["action"][a, b] = OUTLIER
                outliers += 1
    record["u"], record["v"] = out_u, out_v
    return out_u, out_v, outliers, filled, record


def split(position, c, s, n):
    """``(lo, hi, t)`` of real positions on an axis of ``n`` nodes at ``c + s * index``, clamped to the first and last node."""
    g = (np.asarray(position, dtype=np.float64) - c) / s
    g = np.fmin(np.fmax(g, 0.0), float(n - 1))
    lo = np.floor(g).astype(np.int64)
    lo = np.where(lo > n - 2, max(n - 2, 0), lo)
    return lo, np.minimum(lo + 1, n - 1), g - lo.astype(np.float64)


def bilinear(F, rows, columns):
    (la, ha, ta), (lb, hb, tb) = rows, columns
    top = F[la, lb] + tb * (F[la, hb] - F[la, lb])
    bot = F[ha, lb] + tb * (F[ha, hb] - F[ha, lb])
    return top + ta * (bot - top)


def predictor(q, pu, pv, y, x):
    """``(U, V)`` at the real positions ``(y, x)`` (broadcast against each other) from the vectors ``(pu, pv)`` of pass ``q``."""
    valid = ~(np.isnan(pu) | np.isnan(pv))
    U, V = np.where(valid, pu, 0.0), np.where(valid, pv, 0.0)
    c = float(q["m"]) + float(q["w"] - 1) / 2.0
    rows, columns = split(y, c, float(q["s"]), q["R"]), split(x, c, float(q["s"]), q["C"])
    return bilinear(U, rows, columns), bilinear(V, rows, columns)


def warped(second, q, pu, pv):
    """Frame ``k + 1`` at ``(i + V(i, j), j + U(i, j))`` for every pixel ``(i, j)``."""
    N_i, N_j = second.shape
    i, j = np.arange(N_i, dtype=np.float64)[:, None], np.arange(N_j, dtype=np.float64)[None, :]
    U, V = predictor(q, pu, pv, i, j)
    return bilinear(second, split(i + V, 0.0, 1.0, N_i), split(j + U, 0.0, 1.0, N_j))


def piv_pair(first, second, passes, min_correlation=None, deformation=False, outlier_threshold=None, outlier_epsilon=0.1, validate_last=False):
    counts = np.zeros((len(passes), 3), dtype=np.int64)
    validation_counts = np.zeros((len(passes), 2), dtype=np.int64)
    details, u, v = [], None, None
    for k, p in enumerate(passes):
        w, r, s, m, R, C = (p[key] for key in ("w", "r", "s", "m", "R", "C"))
        D = 2 * r + 1
        pu, pv = u, v                                                        # the vectors of the pass before, validated if asked
        q = passes[k - 1] if k else None
        source = warped(second, q, pu, pv) if k and deformation else second
        u, v, corr = (np.full((R, C), NAN) for _ in range(3))
        det = dict(peak=np.zeros((R, C, 2), dtype=np.int64), offset=np.zeros((R, C, 2), dtype=np.int64), gap=np.full((R, C), NAN),
                   surface=np.full((R, C, D, D), NAN), region_at=np.zeros((R, C, 2), dtype=np.int64), base=np.zeros((R, C, 2)), second=source)
        for a in range(R):
            for b in range(C):
                i0, j0 = m + a * s, m + b * s
                o_i = o_j = 0
                base_i = base_j = 0.0
                if k and deformation:
                    U_c, V_c = predictor(q, pu, pv, float(i0) + float(w - 1) / 2.0, float(j0) + float(w - 1) / 2.0)
                    base_i, base_j = float(V_c), float(U_c)
                elif k:
                    ap, bp = pf.previous_index(i0, w, q, q["R"]), pf.previous_index(j0, w, q, q["C"])
                    if not (np.isnan(pu[ap, bp]) or np.isnan(pv[ap, bp])):
                        o_i, o_j = int(np.floor(pv[ap, bp] + 0.5)), int(np.floor(pu[ap, bp] + 0.5))
                    assert abs(o_i) <= q["m"] and abs(o_j) <= q["m"]
                det["offset"][a, b] = o_i, o_j
                det["base"][a, b] = base_i, base_j
                top, left = i0 + o_i - r, j0 + o_j - r
                det["region_at"][a, b] = top, left
                assert top >= 0 and left >= 0 and top + w + 2 * r <= first.shape[0] and left + w + 2 * r <= first.shape[1]
                Cd = pf.surface(first[i0:i0 + w, j0:j0 + w], source[top:top + w + 2 * r, left:left + w + 2 * r])
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
                delta_i = pf.parabola(Cd[p_i - 1, p_j], c0, Cd[p_i + 1, p_j]) if 0 < p_i < D - 1 else 0.0
                delta_j = pf.parabola(Cd[p_i, p_j - 1], c0, Cd[p_i, p_j + 1]) if 0 < p_j < D - 1 else 0.0
                if p_i in (0, D - 1) or p_j in (0, D - 1):
                    counts[k, 1] += 1
                if k and deformation:
                    v[a, b] = base_i + (float(p_i - r) + delta_i)
                    u[a, b] = base_j + (float(p_j - r) + delta_j)
                else:
                    v[a, b] = float(o_i + p_i - r) + delta_i
                    u[a, b] = float(o_j + p_j - r) + delta_j
                if min_correlation is not None and c0 < min_correlation:
                    u[a, b] = v[a, b] = NAN
                    counts[k, 2] += 1
        det["raw"] = (u, v)
        if outlier_threshold is not None and (k < len(passes) - 1 or validate_last):
            u, v, validation_counts[k, 0], validation_counts[k, 1], det["validation"] = validate(u, v, outlier_threshold, outlier_epsilon)
        details.append(det)
    return u, v, corr, counts, validation_counts, details


def piv(movie, window_sizes, search_radii, steps, min_correlation=None, deformation=False, outlier_threshold=None, outlier_epsilon=0.1,
        validate_last=False):
    frames = np.asarray(movie, dtype=np.float64)
    passes = pf.grid(frames.shape[1:], window_sizes, search_radii, steps)
    pairs = [piv_pair(frames[k], frames[k + 1], passes, min_correlation, deformation, outlier_threshold, outlier_epsilon, validate_last)
             for k in range(frames.shape[0] - 1)]
    u, v, corr = (np.stack([pr[f] for pr in pairs]) for f in range(3))
    counts, validation_counts = sum(pr[3] for pr in pairs), sum(pr[4] for pr in pairs)
    details = [[pr[5][p] for pr in pairs] for p in range(len(passes))]       # [pass][pair]
    return u, v, corr, counts, validation_counts, details


# ---- the cases: the smallest at which the kernels can go wrong ------------------------------------------------------------------------
def analytic_texture(n, seed, i, j):
    """The texture of opticalflow_amd.synthetic at the real pixel positions ``(i, j)``, two arrays of one shape."""
    import math
    from opticalflow_amd import synthetic
    f, g, a, phi = synthetic.texture_parameters(n, seed)
    scale = 0.45 * math.sqrt(len(a)) / (3.0 * float(a.sum()))
    phase = 2 * math.pi * (f[:, None, None] * i[None] + g[:, None, None] * j[None]) / n + phi[:, None, None]
    return np.clip(0.5 + scale * np.tensordot(a, np.cos(phase), 1), 0.0, 1.0)


def displaced_pair(n, seed, shape, displacement, zoom=1.0):
    """Two frames of ``shape``: the texture, and the texture whose content at ``(i, j)`` came from ``(i - v(i, j), j - u(i, j))``,
    ``displacement(i, j) -> (u, v)``.  ``zoom``: the texture is shown that many times finer (its shortest period is 16 / zoom pixels)."""
    i, j = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    u, v = displacement(i, j)
    return np.stack([analytic_texture(n, seed, zoom * i, zoom * j), analytic_texture(n, seed, zoom * (i - v), zoom * (j - u))])


SHEAR, SHEAR_ROW = 0.08, 25.0                                                # u = SHEAR * (i - SHEAR_ROW), v = 0
SHIFT = (2.3, -3.6)                                                          # (v, u) of the three-pass case


def _shear():
    """50 x 61, the columns sheared by 0.08 pixels per row (u from -2 to 1.92); windows of 12 then 10 at a step of 5, which divides
    neither 50 - 12 - 6 nor 61 - 12 - 6: the grids of the passes differ in origin and size.  The texture is shown three times finer (shortest
    period 5.3 pixels), so that a window of 10 holds about two periods."""
    movie = displaced_pair(64, 21, (50, 61), lambda i, j: (SHEAR * (i - SHEAR_ROW), 0.0 * i), 3.0)
    return dict(movie=movie, passes=[(12, 3, 5), (10, 2, 5)])


def _three_pass():
    """72 x 80 moved by (2.3, -3.6); the last two passes at one window size: the last predictor comes from a deformed pass."""
    movie = displaced_pair(96, 3, (72, 80), lambda i, j: (SHIFT[1] + 0.0 * i, SHIFT[0] + 0.0 * i))
    return dict(movie=movie, passes=[(24, 5, 12), (12, 2, 6), (12, 2, 6)])


def _one_row_largest():
    """128 x 136, (64, 16, 40) then (64, 16, 32): pass 0 is one row of two windows (R = 1: the degenerate interpolation branch along
    the rows), pass 1 one window at the largest LDS need."""
    movie = displaced_pair(136, 5, (128, 136), lambda i, j: (-7.4 + 0.0 * i, 3.3 + 0.0 * i))
    return dict(movie=movie, passes=[(64, 16, 40), (64, 16, 32)])


VALIDATION_FLAT = ((0, 0), (2, 1))                                           # pass-0 windows constant in the first frame
VALIDATION_FOREIGN = (1, 1)                                                  # the pass-0 window over the block of foreign motion
VALIDATION_FEW = (2, 0)                                                      # the corner whose neighbour (2, 1) is flat: two valid neighbours
VALIDATION_THREE = (0, 2)                                                    # a corner with exactly three neighbours, all valid
FOREIGN_SHIFT = (-2.7, 3.4)


def _validation():
    """108 x 116, passes (32, 6, 32) and (16, 2, 8), the texture moved by (2.3, -3.6): a 3 x 3 grid of pass-0 windows that do not
    overlap, at rows and columns 6, 38, 70.  Windows (0, 0) and (2, 1) are constant in the first frame (their blocks move with the
    texture, by (2, -4)): NaN vectors, which the median test fills from three and from five neighbours; the corner (2, 0) keeps two
    valid neighbours and stays as it is; the corner (0, 2) has exactly three.  The second frame shows, in rows and columns [40, 68)
    inside window (1, 1), the texture moved by (-2.7, 3.4) instead: that window's vector is an outlier among its six valid
    neighbours, and so is that of (1, 2), whose search region reaches the block's edge and whose peak it pulls by a pixel."""
    movie = displaced_pair(108, 3, (108, 116), lambda i, j: (SHIFT[1] + 0.0 * i, SHIFT[0] + 0.0 * i))
    other = displaced_pair(108, 3, (108, 116), lambda i, j: (FOREIGN_SHIFT[1] + 0.0 * i, FOREIGN_SHIFT[0] + 0.0 * i))[1]
    movie[1, 40:68, 40:68] = other[40:68, 40:68]
    for a, b in VALIDATION_FLAT:
        i0, j0 = 6 + 32 * a, 6 + 32 * b
        movie[0, i0:i0 + 32, j0:j0 + 32] = 0.5
        movie[1, i0 + 2:i0 + 34, j0 - 4:j0 + 28] = 0.5
    return dict(movie=movie, passes=[(32, 6, 32), (16, 2, 8)])


VALIDATION = dict(outlier_threshold=2.0, outlier_epsilon=0.1)
MAKERS = dict(shear=_shear, three_pass=_three_pass, one_row_largest=_one_row_largest, validation=_validation)
# name -> (movie of MAKERS, options)
CASE_OPTIONS = dict(
    shear=("shear", dict(deformation=True)),
    three_pass=("three_pass", dict(deformation=True)),
    one_row_largest=("one_row_largest", dict(deformation=True)),
    validation_integer=("validation", dict(**VALIDATION)),
    validation_deformed=("validation", dict(deformation=True, **VALIDATION)),
    validation_last=("validation", dict(deformation=True, validate_last=True, **VALIDATION)),
    validation_thresholded=("validation", dict(min_correlation=0.8, validate_last=True, **VALIDATION)),
)
CASES = tuple(CASE_OPTIONS)
OPTION_NAMES = ("min_correlation", "deformation", "outlier_threshold", "outlier_epsilon", "validate_last")


@functools.lru_cache(maxsize=None)
def _made(name):
    """Three frames, the maker's two and the first again: the second pair is the first one backwards, so every case has two pairs for
    the chunks of a call to split."""
    c = MAKERS[name]()
    c["movie"] = np.concatenate([c["movie"], c["movie"][:1]])
    c["movie"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """``dict(movie, window_sizes, search_radii, steps, min_correlation, deformation, outlier_threshold, outlier_epsilon,
    validate_last)``; made once and shared: leave it unchanged."""
    maker, options = CASE_OPTIONS[name]
    c = _made(maker)
    w, r, s = (tuple(p[k] for p in c["passes"]) for k in range(3))
    full = dict(min_correlation=None, deformation=False, outlier_threshold=None, outlier_epsilon=0.1, validate_last=False)
    full.update(options)
    return dict(movie=c["movie"], window_sizes=w, search_radii=r, steps=s, **full)


def arguments(name):
    """The keyword arguments of ``conduct_piv`` for the case, without the movie."""
    c = case(name)
    return {k: c[k] for k in ("window_sizes", "search_radii", "steps") + OPTION_NAMES}


@functools.lru_cache(maxsize=None)
def restated(name, **changed):
    """``piv`` of the case (``changed``: options that replace the case's), computed once and shared: leave it unchanged."""
    c = dict(case(name))
    c.update(changed)
    return piv(c["movie"], c["window_sizes"], c["search_radii"], c["steps"], *(c[k] for k in OPTION_NAMES))
