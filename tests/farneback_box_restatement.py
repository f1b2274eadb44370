"""numpy restatement of the box window of OpenCV 4's calcOpticalFlowFarneback (flags without OPTFLOW_FARNEBACK_GAUSSIAN;
FarnebackUpdateFlow_Blur) as DESIGN.md section 16.1 specifies it, written independently of the package (nothing is imported from
it).  Everything but the iteration - levels, level images, the carried flow, the expansion, the matrices - is the Gaussian
restatement's (farneback_restatement), imported from there.

OpenCV keeps the window as two running sums in double, so a value depends on the order of the additions: the loops here run over
the rows, then over the columns, one addition per step in OpenCV's order; planes and the other axis are array axes.

``rec`` as in farneback_restatement, with ``winsize`` and ``m`` in place of ``window_taps``."""
import numpy as np

from farneback_restatement import F, NAMES, level_sizes, matrices, poly_exp, poly_tables, presmooth, presmooth_taps, resize_linear

D = np.float64


def running_sums(M, m):
    """The (2 m + 1)^2 clamped window sums of the float32 planes M (5, h, w) as OpenCV accumulates them: double (5, h, w)."""
    _, h, w = M.shape
    v = (M[:, 0, :] * F(m + 2)).astype(D)                      # one float32 product
    for y in range(1, m):
        v = v + M[:, min(y, h - 1), :].astype(D)
    V = np.empty(M.shape, dtype=D)
    for y in range(h):
        d = M[:, min(y + m, h - 1), :] - M[:, max(y - m - 1, 0), :]        # a float32 subtraction
        v = v + d.astype(D)
        V[:, y, :] = v
    a = V[:, :, 0] * D(m + 2)
    for x in range(1, m):
        a = a + V[:, :, min(x, w - 1)]
    g = np.empty(M.shape, dtype=D)
    for x in range(w):
        a = a + (V[:, :, min(x + m, w - 1)] - V[:, :, max(x - m - 1, 0)])  # the difference in double first
        g[:, :, x] = a
    return g


def solve(g, winsize):
    """The flow (2, h, w) from the window sums: scale = 1 / winsize^2 although the window is 2 (winsize // 2) + 1 wide."""
    scale = 1.0 / D(winsize * winsize)
    g11, g12, g22, h1, h2 = g * scale
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet]).astype(F)


def iterate_box(M, winsize):
    """One box blur of M and the 2 x 2 solve: the flow (2, h, w)."""
    if winsize < 2:
        raise ValueError("winsize = 1 (m = 0) is excluded: OpenCV's start values count row 0 and column 0 once too often there")
    return solve(running_sums(M, winsize // 2), winsize)


def farneback_pair_box(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, rec=None, iterate=iterate_box):
    """cv2.calcOpticalFlowFarneback(prev, nxt, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, 0): float32
    (h, w, 2).  ``iterate``: what stands in for iterate_box (the CPU tests pass a re-associated window sum)."""
    rec = {} if rec is None else rec
    N_i, N_j = prev.shape
    sizes = level_sizes(N_i, N_j, pyr_scale, levels)
    tab = poly_tables(poly_n, float(poly_sigma))
    rec.update(sizes=[(h, w) for h, w, _, _ in sizes], ksizes=[s[2] for s in sizes], winsize=winsize, m=winsize // 2, poly=tab,
               presmooth_taps=[presmooth_taps(s[2], s[3]) for s in sizes])
    for name in ("level_images", "R", "M", "flows", "outside"):
        rec[name] = [None] * len(sizes)
    inv_scale = F(1.0 / pyr_scale)
    frames = [np.asarray(prev).astype(F), np.asarray(nxt).astype(F)]
    flow = None
    for lv in range(len(sizes) - 1, -1, -1):
        h, w, _, _ = sizes[lv]
        taps = rec["presmooth_taps"][lv]
        images = [resize_linear(presmooth(f, taps), h, w) for f in frames]
        R0, R1 = (poly_exp(im, poly_n, tab) for im in images)
        if flow is None:
            flow = np.zeros((2, h, w), dtype=F)
        else:
            flow = np.stack([resize_linear(flow[0], h, w), resize_linear(flow[1], h, w)]) * inv_scale
        rec["level_images"][lv], rec["R"][lv], rec["flows"][lv] = images, (R0, R1), [flow]
        outside = np.zeros((h, w), dtype=bool)
        for it in range(iterations):
            if it == 0:
                M, out = matrices(R0, R1, flow)
                rec["M"][lv] = M
                outside |= out
            flow = iterate(M, winsize)
            rec["flows"][lv].append(flow)
            if it < iterations - 1:                           # all flows from the old M, then all of M from the new flows
                M, out = matrices(R0, R1, flow)
                outside |= out
        rec["outside"][lv] = outside
    return np.moveaxis(flow, 0, 2)


def conduct_opencv_flow_box(movie, delta_x=1.0, delta_t=1.0, blurred=None, rec=None, iterate=iterate_box, **kwargs):
    """farneback_restatement.conduct_opencv_flow over ``farneback_pair_box``."""
    if sorted(kwargs) != sorted(NAMES):
        raise TypeError("the six OpenCV arguments are required")
    first = movie if blurred is None else blurred
    T = movie.shape[0]
    v_x = np.zeros((T - 1,) + movie.shape[1:])
    v_y = np.zeros((T - 1,) + movie.shape[1:])
    recs = []
    for k in range(T - 1):
        r = {}
        flow = farneback_pair_box(first[k], movie[k + 1], rec=r, iterate=iterate, **kwargs)
        recs.append(r)
        v_x[k] = flow[:, :, 0]
        v_y[k] = flow[:, :, 1]
    v_x *= delta_x / delta_t
    v_y *= delta_x / delta_t
    if rec is not None:
        rec["pairs"] = recs
    return dict(v_x=v_x, v_y=v_y, speed=np.sqrt(v_x ** 2 + v_y ** 2), original_data=first, delta_x=delta_x, delta_t=delta_t)
