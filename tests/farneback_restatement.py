"""numpy restatement of conduct_opencv_flow: OpenCV 4's calcOpticalFlowFarneback with OPTFLOW_FARNEBACK_GAUSSIAN as DESIGN.md
section 16 specifies it, written independently of the package (nothing is imported from it).  Image arithmetic is float32 -
float32 arrays and np.float32 scalars, one rounding per written operation - except where the specification says double.  The
innermost loops run over taps; pixels are array axes.

``rec`` (a dict, optional) receives the stage outputs: ``sizes``, ``ksizes``, ``presmooth_taps``, ``window_taps``, ``poly`` and per
level (lists indexed by level, finest = 0) ``level_images``, ``R``, ``M`` (the first one of the level), ``flows`` (start value, then
one per iteration) and ``outside`` (the mask of the pixels that took the outside branch, or-ed over the level's constructions of M)."""
import math

import numpy as np

F = np.float32
FLT_EPSILON = 1.1920928955078125e-07
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
NAMES = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma")


def cv_round(x):
    return int(np.rint(x))                                   # half to even


def level_sizes(N_i, N_j, pyr_scale, levels):
    """[(height, width, ksize, sigma)] for k = 0 .. L."""
    scale, L = 1.0, 0
    for L in range(levels):
        scale *= pyr_scale
        if N_j * scale < 32 or N_i * scale < 32:
            break
    else:
        L = levels
    out = []
    for k in range(L + 1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        ksize = max(cv_round(sigma * 5) | 1, 3)
        out.append((cv_round(N_i * scale), cv_round(N_j * scale), ksize, sigma))
    return out


def presmooth_taps(ksize, sigma):
    if ksize == 3 and sigma <= 0:
        return np.array([0.25, 0.5, 0.25], dtype=F)
    scale2x = -0.5 / (sigma * sigma)
    t = []
    for i in range(ksize):
        x = i - (ksize - 1) * 0.5
        t.append(math.exp(scale2x * x * x))
    total = 0.0
    for v in t:
        total += v
    inv = 1.0 / total
    return np.array([v * inv for v in t], dtype=np.float64).astype(F)


def reflect101(idx, n):
    idx = np.asarray(idx).copy()
    while True:
        bad = (idx < 0) | (idx >= n)
        if not bad.any():
            return idx
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)


def presmooth(img, w):
    """Row pass (along the columns) first, then the column pass; REFLECT_101."""
    r = len(w) // 2
    for axis in (1, 0):
        n = img.shape[axis]
        pos = np.arange(n)
        s = F(w[r]) * img
        for i in range(1, r + 1):
            lo = np.take(img, reflect101(pos - i, n), axis=axis)
            hi = np.take(img, reflect101(pos + i, n), axis=axis)
            s = s + F(w[r + i]) * (lo + hi)
        img = s
    return img


def resize_axis(ssize, dsize):
    sc = 1.0 / (dsize / ssize)
    s_idx, frac, two = [], [], []
    for d in range(dsize):
        f = F((d + 0.5) * sc - 0.5)
        s = int(math.floor(f))
        f = F(f - F(s))
        if s < 0:
            s, f = 0, F(0)
        single = s >= ssize - 1
        if single:
            s, f = ssize - 1, F(0)
        s_idx.append(s); frac.append(f); two.append(not single)
    return np.array(s_idx), np.array(frac, dtype=F), np.array(two)


def resize_linear(img, height, width):
    """The horizontal pass first, then the vertical one, each S[s] * (1 - f) + S[s + 1] * f (one term at the last index)."""
    for axis, dsize in ((1, width), (0, height)):
        ssize = img.shape[axis]
        s, f, two = resize_axis(ssize, dsize)
        shape = (1, -1) if axis == 1 else (-1, 1)
        f, two = f.reshape(shape), two.reshape(shape)
        a = np.take(img, s, axis=axis) * (F(1) - f)
        b = np.take(img, np.minimum(s + 1, ssize - 1), axis=axis) * f
        img = np.where(two, a + b, a).astype(F)
    return img


def poly_tables(n, sigma):
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    g = np.array([math.exp(-x * x / (2 * sigma * sigma)) for x in range(-n, n + 1)], dtype=np.float64).astype(F)
    total = 0.0
    for v in g:
        total += float(v)
    s = 1.0 / total
    g = np.array([float(v) * s for v in g], dtype=np.float64).astype(F)
    xs = np.arange(-n, n + 1)
    xg = (xs.astype(F) * g).astype(F)
    xxg = ((xs * xs).astype(F) * g).astype(F)
    G00 = G11 = G33 = G55 = 0.0
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            gg = float(g[y + n]) * float(g[x + n])
            G00 += gg
            G11 += gg * x * x
            G33 += gg * x * x * x * x
            G55 += gg * x * x * y * y
    G = np.zeros((6, 6))
    G[0, 0] = G00
    G[1, 1] = G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G11
    G[3, 3] = G[4, 4] = G33
    G[3, 4] = G[4, 3] = G[5, 5] = G55
    inv = np.linalg.inv(G)
    return dict(g=g, xg=xg, xxg=xxg, G=G, invG=inv, ig11=inv[1, 1], ig03=inv[0, 3], ig33=inv[3, 3], ig55=inv[5, 5])


def poly_exp(img, n, tab):
    """(5, h, w) float32: the vertical pass in float32, the horizontal one in double."""
    h, w = img.shape
    g, xg, xxg = tab["g"][n:], tab["xg"][n:], tab["xxg"][n:]
    rows = np.arange(h)
    t0 = img * g[0]
    t1 = np.zeros_like(img)
    t2 = np.zeros_like(img)
    for k in range(1, n + 1):
        a = img[np.maximum(rows - k, 0)]
        b = img[np.minimum(rows + k, h - 1)]
        p = a + b
        t0 = t0 + g[k] * p
        t1 = t1 + xg[k] * (b - a)
        t2 = t2 + xxg[k] * p
    cols = np.arange(w)
    D = np.float64
    g0 = D(g[0])
    b1, b3, b5 = t0.astype(D) * g0, t1.astype(D) * g0, t2.astype(D) * g0
    b2, b4, b6 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    for k in range(1, n + 1):
        hi, lo = np.minimum(cols + k, w - 1), np.maximum(cols - k, 0)
        tg = (t0[:, hi] + t0[:, lo]).astype(D)                # sums and differences of two float32 values are float32
        b1 = b1 + tg * D(g[k])
        b4 = b4 + tg * D(xxg[k])
        b2 = b2 + (t0[:, hi] - t0[:, lo]).astype(D) * D(xg[k])
        b3 = b3 + (t1[:, hi] + t1[:, lo]).astype(D) * D(g[k])
        b6 = b6 + (t1[:, hi] - t1[:, lo]).astype(D) * D(xg[k])
        b5 = b5 + (t2[:, hi] + t2[:, lo]).astype(D) * D(g[k])
    ig11, ig03, ig33, ig55 = tab["ig11"], tab["ig03"], tab["ig33"], tab["ig55"]
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55]).astype(F)


def matrices(R0, R1, flow):
    """M (5, h, w) from the two expansions and the flow (2, h, w), and the mask of the pixels outside."""
    _, h, w = R0.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dx, dy = flow[0], flow[1]
    fx = x.astype(F) + dx
    fy = y.astype(F) + dy
    with np.errstate(invalid="ignore"):
        flx, fly = np.floor(fx), np.floor(fy)
        inside = (flx >= 0) & (flx < w - 1) & (fly >= 0) & (fly < h - 1)       # NaN and what fits no int: outside
    x1 = np.where(inside, flx, 0).astype(np.int64)
    y1 = np.where(inside, fly, 0).astype(np.int64)
    fx = np.where(inside, fx - x1.astype(F), F(0)).astype(F)
    fy = np.where(inside, fy - y1.astype(F), F(0)).astype(F)
    one = F(1)
    a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    r = []
    for c in range(5):
        P = R1[c]
        r.append(a00 * P[y1, x1] + a01 * P[y1, x1 + 1] + a10 * P[y1 + 1, x1] + a11 * P[y1 + 1, x1 + 1])
    r2, r3, r4, r5, r6 = r
    r4 = np.where(inside, (R0[2] + r4) * F(0.5), R0[2])
    r5 = np.where(inside, (R0[3] + r5) * F(0.5), R0[3])
    r6 = np.where(inside, (R0[4] + r6) * F(0.25), R0[4] * F(0.5))
    r2 = np.where(inside, r2, F(0))
    r3 = np.where(inside, r3, F(0))
    r2 = (R0[0] - r2) * F(0.5)
    r3 = (R0[1] - r3) * F(0.5)
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    bd = np.array(BORDER, dtype=F)
    sx = np.where(x < 5, bd[np.minimum(x, 4)], one) * np.where(x >= w - 5, bd[np.clip(w - x - 1, 0, 4)], one)
    sy = np.where(y < 5, bd[np.minimum(y, 4)], one)
    sy2 = np.where(y >= h - 5, bd[np.clip(h - y - 1, 0, 4)], one)
    scale = ((sx * sy) * sy2).astype(F)
    r2, r3, r4, r5, r6 = (v * scale for v in (r2, r3, r4, r5, r6))
    M = np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3]).astype(F)
    return M, ~inside


def window_taps(winsize):
    m = winsize // 2
    sigma = m * 0.3
    k = [F(1)] + [F(math.exp(-i * i / (2 * sigma * sigma))) for i in range(1, m + 1)]
    s = 1.0
    for v in k[1:]:
        s += float(v) * 2
    inv = 1.0 / s
    return np.array([float(v) * inv for v in k], dtype=np.float64).astype(F)


def iterate(M, k):
    """One blur of M with the window and the 2 x 2 solve: the flow (2, h, w)."""
    _, h, w = M.shape
    m = len(k) - 1
    rows, cols = np.arange(h), np.arange(w)
    v = M * k[0]
    for i in range(1, m + 1):
        v = v + (M[:, np.minimum(rows + i, h - 1)] + M[:, np.maximum(rows - i, 0)]) * k[i]
    b = v * k[0]
    for i in range(1, m + 1):
        b = b + k[i] * (v[:, :, np.maximum(cols - i, 0)] + v[:, :, np.minimum(cols + i, w - 1)])
    g11, g12, g22, h1, h2 = b.astype(np.float64)
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet]).astype(F)


def farneback_pair(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, rec=None):
    """cv2.calcOpticalFlowFarneback(prev, nxt, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
    OPTFLOW_FARNEBACK_GAUSSIAN): float32 (h, w, 2)."""
    rec = {} if rec is None else rec
    N_i, N_j = prev.shape
    sizes = level_sizes(N_i, N_j, pyr_scale, levels)
    tab = poly_tables(poly_n, float(poly_sigma))
    k = window_taps(winsize)
    rec.update(sizes=[(h, w) for h, w, _, _ in sizes], ksizes=[s[2] for s in sizes], window_taps=k, poly=tab,
               presmooth_taps=[presmooth_taps(s[2], s[3]) for s in sizes])
    for name in ("level_images", "R", "M", "flows", "outside"):
        rec[name] = [None] * len(sizes)
    inv_scale = F(1.0 / pyr_scale)
    frames = [np.asarray(prev).astype(F), np.asarray(nxt).astype(F)]
    flow = None
    for lv in range(len(sizes) - 1, -1, -1):
        h, w, ksize, sigma = sizes[lv]
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
            flow = iterate(M, k)
            rec["flows"][lv].append(flow)
            if it < iterations - 1:
                M, out = matrices(R0, R1, flow)
                outside |= out
        rec["outside"][lv] = outside
    return np.moveaxis(flow, 0, 2)


def conduct_opencv_flow(movie, delta_x=1.0, delta_t=1.0, blurred=None, rec=None, **kwargs):
    """The reference's loop (source/optical_flow.py:220-279) over ``farneback_pair``; ``blurred`` is the movie after the optional
    blur (pair k takes its first image from it and its second from ``movie[k + 1]``)."""
    if sorted(kwargs) != sorted(NAMES):
        raise TypeError("the six OpenCV arguments are required")
    first = movie if blurred is None else blurred
    T = movie.shape[0]
    v_x = np.zeros((T - 1,) + movie.shape[1:])
    v_y = np.zeros((T - 1,) + movie.shape[1:])
    recs = []
    for k in range(T - 1):
        r = {}
        flow = farneback_pair(first[k], movie[k + 1], rec=r, **kwargs)
        recs.append(r)
        v_x[k] = flow[:, :, 0]
        v_y[k] = flow[:, :, 1]
    v_x *= delta_x / delta_t
    v_y *= delta_x / delta_t
    if rec is not None:
        rec["pairs"] = recs
    return dict(v_x=v_x, v_y=v_y, speed=np.sqrt(v_x ** 2 + v_y ** 2), original_data=first, delta_x=delta_x, delta_t=delta_t)
