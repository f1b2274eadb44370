"""Plain-numpy restatement of the device part of convert_PIV_result / upsample_PIV_vectors, and the cases
its CPU and GPU tests share.  It is the specification the kernels of csrc/vof_piv.hpp are held to, bit for bit.

The triangulation (scipy.spatial.Delaunay, scipy's defaults) and the gradients (CloughTocher2DInterpolator(tri, values).grad,
tol 1e-6, maxiter 400) come from scipy, as in the product.  Restated here, every operation a single IEEE one in the order written:

* barycentric coordinates of the target q = (x = j, y = i) of out[i, j] in triangle t, T = tri.transform[t]:
  c0 = T00 (qx - rx) + T01 (qy - ry), c1 = T10 (qx - rx) + T11 (qy - ry), c2 = 1 - c0 - c1;
* inclusion: all three in [-EPS_IN, 1 + EPS_IN], EPS_IN = 100 * DBL_EPSILON (scipy's find_simplex tolerance);
* tie rule: of the triangles that include a pixel, the lowest index; none: NaN in v_x, v_y and speed;
* the 19 control values of the Clough-Tocher element per triangle and component (control_values);
* the value: m = min(c), b1..b3 = c - m, b4 = 3 m and the 19 terms summed left to right (cubic); powers are products, sq(b) = b * b
  and cube(b) = (b * b) * b, and a term is formed from the left: ((3 * sq(b1)) * b2) * c2100, ((3 * b1) * sq(b2)) * c1200,
  (((6 * b1) * b2) * b4) * c1101, cube(b1) * c3000;
* speed = sqrt(v_x * v_x + v_y * v_y).

With powers="pow" (cube(b) = pow(b, 3.0) of the C library, which is what b**3 is in scipy's compiled code; numpy's own array power
is a vectorised routine with other last bits) and scipy's own choice of triangle the same code gives scipy's bits: that pins the
formulas (tests/test_piv_convert_cpu.py)."""
import functools
import math

import numpy as np

EPS_IN = 100 * np.finfo(np.float64).eps
NONE = np.int32(2 ** 31 - 1)           # the map's "no triangle"
BAND = 1e-9                            # input_conditions: no coordinate in (-BAND, -EPS_IN) or (1 + EPS_IN, 1 + BAND)
LIBM_CUBE = np.frompyfunc(lambda b: math.pow(b, 3.0), 1, 1)


# ---- the host part, as the product makes it ------------------------------------------------------------------------------------
def frame_tables(points, values):
    """(tri, grad) of one frame: points (n, 2) as (x, y), values (n, 2) as (v_x, v_y)."""
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    tri = Delaunay(np.ascontiguousarray(points, dtype=np.float64))
    grad = CloughTocher2DInterpolator(tri, np.ascontiguousarray(values, dtype=np.float64)).grad
    return tri, np.ascontiguousarray(grad, dtype=np.float64)


def valid_points(x, y, vx, vy):
    """points (n, 2), values (n, 2) of one frame's (R, C) arrays: where neither vector component is NaN, in C order."""
    ok = np.logical_and(~np.isnan(vx), ~np.isnan(vy))
    return np.stack([x[ok].ravel(), y[ok].ravel()], axis=1), np.stack([vx[ok].ravel(), vy[ok].ravel()], axis=1)


# ---- the device part ------------------------------------------------------------------------------------------------------------
def barycentric(T, qx, qy):
    """T (..., 6) = (T00, T01, T10, T11, rx, ry) against targets of a broadcastable shape."""
    dx, dy = qx - T[..., 4], qy - T[..., 5]
    c0 = T[..., 0] * dx + T[..., 1] * dy
    c1 = T[..., 2] * dx + T[..., 3] * dy
    c2 = 1.0 - c0 - c1
    return c0, c1, c2


def transforms(tri):
    """(ntri, 6): the 2 x 2 inverse, row-major, then the offset r."""
    return np.ascontiguousarray(tri.transform.reshape(-1, 6))


def control_values(tri, values, grad):
    """(ntri, 2, 19) in the order of the sum: c3000 c2100 c2010 c2001 c1200 c1101 c1020 c1011 c1002 c0300 c0210 c0201 c0120 c0111
    c0102 c0030 c0021 c0012 c0003."""
    P, S, N, T = tri.points, tri.simplices, tri.neighbors, transforms(tri)
    p0, p1, p2 = P[S[:, 0]], P[S[:, 1]], P[S[:, 2]]
    e12, e23, e31 = p1 - p0, p2 - p1, p0 - p2
    g = []
    for k in range(3):                                   # the neighbour opposite vertex k
        nb = N[:, k]
        s = S[np.where(nb < 0, 0, nb)]
        yx = (P[s[:, 0], 0] + P[s[:, 1], 0] + P[s[:, 2], 0]) / 3
        yy = (P[s[:, 0], 1] + P[s[:, 1], 1] + P[s[:, 2], 1]) / 3
        y = barycentric(T, yx, yy)
        a, b = y[(k + 2) % 3], y[(k + 1) % 3]
        with np.errstate(all="ignore"):
            gk = (2 * a + b - 1) / (2 - 3 * a - 3 * b)
        g.append(np.where(nb < 0, -0.5, gk))
    out = np.empty((S.shape[0], 2, 19))
    for comp in range(2):
        f1, f2, f3 = values[S[:, 0], comp], values[S[:, 1], comp], values[S[:, 2], comp]
        g0, g1, g2 = grad[S[:, 0], comp], grad[S[:, 1], comp], grad[S[:, 2], comp]

        def dot(gv, e):
            return gv[:, 0] * e[:, 0] + gv[:, 1] * e[:, 1]
        df12, df21 = +dot(g0, e12), -dot(g1, e12)
        df23, df32 = +dot(g1, e23), -dot(g2, e23)
        df31, df13 = +dot(g2, e31), -dot(g0, e31)
        c3000 = f1
        c2100 = (df12 + 3 * c3000) / 3
        c2010 = (df13 + 3 * c3000) / 3
        c0300 = f2
        c1200 = (df21 + 3 * c0300) / 3
        c0210 = (df23 + 3 * c0300) / 3
        c0030 = f3
        c1020 = (df31 + 3 * c0030) / 3
        c0120 = (df32 + 3 * c0030) / 3
        c2001 = (c2100 + c2010 + c3000) / 3
        c0201 = (c1200 + c0300 + c0210) / 3
        c0021 = (c1020 + c0120 + c0030) / 3
        c0111 = (g[0] * (-c0300 + 3 * c0210 - 3 * c0120 + c0030) + (-c0300 + 2 * c0210 - c0120 + c0021 + c0201)) / 2
        c1011 = (g[1] * (-c0030 + 3 * c1020 - 3 * c2010 + c3000) + (-c0030 + 2 * c1020 - c2010 + c2001 + c0021)) / 2
        c1101 = (g[2] * (-c3000 + 3 * c2100 - 3 * c1200 + c0300) + (-c3000 + 2 * c2100 - c1200 + c2001 + c0201)) / 2
        c1002 = (c1101 + c1011 + c2001) / 3
        c0102 = (c1101 + c0111 + c0201) / 3
        c0012 = (c1011 + c0111 + c0021) / 3
        c0003 = (c1002 + c0102 + c0012) / 3
        out[:, comp] = np.stack([c3000, c2100, c2010, c2001, c1200, c1101, c1020, c1011, c1002, c0300, c0210, c0201, c0120, c0111,
                                 c0102, c0030, c0021, c0012, c0003], axis=1)
    return out


def cubic(c0, c1, c2, cv, powers="products"):
    """The value of the element with control values cv (..., 19) at barycentric coordinates c."""
    if powers == "products":
        sq, cube = (lambda b: b * b), (lambda b: (b * b) * b)
    else:                                                # scipy's compiled b**2 and b**3: the C library's pow, element by element
        sq, cube = (lambda b: b * b), (lambda b: LIBM_CUBE(b).astype(np.float64))
    m = c0
    m = np.where(c1 < m, c1, m)
    m = np.where(c2 < m, c2, m)
    b1, b2, b3, b4 = c0 - m, c1 - m, c2 - m, 3 * m
    k = [cv[..., n] for n in range(19)]
    w = cube(b1) * k[0]
    w = w + ((3 * sq(b1)) * b2) * k[1]
    w = w + ((3 * sq(b1)) * b3) * k[2]
    w = w + ((3 * sq(b1)) * b4) * k[3]
    w = w + ((3 * b1) * sq(b2)) * k[4]
    w = w + (((6 * b1) * b2) * b4) * k[5]
    w = w + ((3 * b1) * sq(b3)) * k[6]
    w = w + (((6 * b1) * b3) * b4) * k[7]
    w = w + ((3 * b1) * sq(b4)) * k[8]
    w = w + cube(b2) * k[9]
    w = w + ((3 * sq(b2)) * b3) * k[10]
    w = w + ((3 * sq(b2)) * b4) * k[11]
    w = w + ((3 * b2) * sq(b3)) * k[12]
    w = w + (((6 * b2) * b3) * b4) * k[13]
    w = w + ((3 * b2) * sq(b4)) * k[14]
    w = w + cube(b3) * k[15]
    w = w + ((3 * sq(b3)) * b4) * k[16]
    w = w + ((3 * b3) * sq(b4)) * k[17]
    w = w + cube(b4) * k[18]
    return w


def targets(shape):
    """(qx, qy) of an (N_i, N_j) frame: out[i, j] is interpolated at (x = j, y = i)."""
    qy, qx = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    return qx, qy


def locate(tri, shape):
    """int32 (N_i, N_j): the lowest index among the triangles that include the pixel, NONE where none does - every triangle against
    every pixel.  Also the smallest distance of a coordinate from the band input_conditions forbids (inf: no coordinate near it)."""
    qx, qy = targets(shape)
    T = transforms(tri)
    found = np.full(shape, NONE, dtype=np.int32)
    in_band = False
    for t in range(T.shape[0] - 1, -1, -1):
        c = barycentric(T[t], qx, qy)
        inside = np.ones(shape, dtype=bool)
        for ck in c:
            inside &= (ck >= -EPS_IN) & (ck <= 1.0 + EPS_IN)
            in_band |= bool((((ck > -BAND) & (ck < -EPS_IN)) | ((ck > 1.0 + EPS_IN) & (ck < 1.0 + BAND))).any())
        found[inside] = t
    return found, in_band


def evaluate(tri, values, grad, shape, simplex=None, powers="products"):
    """(v_x, v_y, speed) of one frame, float64 (N_i, N_j).  simplex: another choice of triangle per pixel (-1 or NONE: none)."""
    if simplex is None:
        simplex = locate(tri, shape)[0]
    simplex = np.asarray(simplex).reshape(shape)
    outside = (simplex < 0) | (simplex == NONE)
    t = np.where(outside, 0, simplex)
    qx, qy = targets(shape)
    c0, c1, c2 = barycentric(transforms(tri)[t], qx, qy)
    cv = control_values(tri, values, grad)[t]
    v = [np.where(outside, np.nan, cubic(c0, c1, c2, cv[..., comp, :], powers)) for comp in range(2)]
    return v[0], v[1], np.sqrt(v[0] * v[0] + v[1] * v[1])


def upsample(x, y, vx, vy, shape):
    """The restatement of upsample_PIV_vectors: (v_x, v_y, speed), float64 (F, N_i, N_j), and counts = (pixels outside every
    triangle, 0)."""
    out = np.empty((3, len(x)) + tuple(shape))
    for k in range(len(x)):
        points, values = valid_points(*(np.asarray(a[k], dtype=np.float64) for a in (x, y, vx, vy)))
        tri, grad = frame_tables(points, values)
        assert not np.isnan(tri.transform).any(), "a degenerate simplex: not a case of the restatement"
        out[:, k] = evaluate(tri, values, grad, shape)
    return out[0], out[1], out[2], np.array([np.isnan(out[0]).sum(), 0], dtype=np.int64)


def griddata(x, y, vx, vy, shape):
    """What the reference computes: scipy.interpolate.griddata(..., method='cubic') per frame and field; speed as it takes it."""
    import scipy.interpolate
    qx, qy = targets(shape)
    out = np.empty((3, len(x)) + tuple(shape))
    for k in range(len(x)):
        points, values = valid_points(*(np.asarray(a[k], dtype=np.float64) for a in (x, y, vx, vy)))
        for comp in range(2):
            out[comp, k] = scipy.interpolate.griddata((points[:, 0], points[:, 1]), values[:, comp], (qx, qy), method="cubic")
    out[2] = np.sqrt(out[0] ** 2 + out[1] ** 2)
    return out[0], out[1], out[2]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def smooth_vectors(x, y, frame, rng):
    """A smooth field with |v| <= 9 plus a little noise, as PIV gives it."""
    vx = 6.0 * np.sin(x / 11.0 + 0.4 * frame) * np.cos(y / 7.0) + 0.5 * rng.standard_normal(x.shape)
    vy = 5.0 * np.cos(x / 9.0) * np.sin(y / 13.0 - 0.3 * frame) + 0.5 * rng.standard_normal(x.shape)
    return vx, vy


def grid_case(shape, step, masks, seed, scale=1.0):
    """A PIV grid of `step` pixels, first vector at step / 2, over an (N_i, N_j) movie; masks: per frame the (row, column) grid
    positions without a vector.  scale: what convert_PIV_result's delta_x does to the locations."""
    rng = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.arange(step // 2, shape[0], step, dtype=np.float64), np.arange(step // 2, shape[1], step, dtype=np.float64),
                         indexing="ij")
    F = len(masks)
    x, y = np.repeat(gx[None] * scale, F, 0), np.repeat(gy[None] * scale, F, 0)
    vx, vy = np.empty_like(x), np.empty_like(x)
    for k, missing in enumerate(masks):
        vx[k], vy[k] = smooth_vectors(gx, gy, k, rng)
        for (r, c) in missing:
            vx[k, r, c] = np.nan
            if (r + c) % 2:
                vy[k, r, c] = np.nan                      # a vector is missing where either component is
    return dict(shape=shape, x=x, y=y, vx=vx, vy=vy)


def scattered_case(shape, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, shape[1] - 1.5, (1, 5, n // 5))
    y = rng.uniform(0.5, shape[0] - 1.5, (1, 5, n // 5))
    vx, vy = smooth_vectors(x[0], y[0], 0, rng)
    return dict(shape=shape, x=x, y=y, vx=vx[None], vy=vy[None])


# 37 x 53 (non-square, odd) with a 6 x 9 grid of step 6.  Frame 0: a corner, a border and an interior vector missing (a concave
# region, a diagonal hull edge, NaN pixels inside bounding boxes); frames 1 and 2: one mask (the reuse path), another border;
# frame 3: a third mask, complete but for the opposite corner - so triangle counts and table offsets differ from frame to frame.
ODD_MASKS = [[(0, 0), (3, 8), (2, 4)], [(5, 3), (0, 8)], [(5, 3), (0, 8)], [(5, 8)]]


@functools.lru_cache(maxsize=None)
def case(name):
    made = {"odd_grid": lambda: grid_case((37, 53), 6, ODD_MASKS, 190),
            "scattered": lambda: scattered_case((48, 40), 40, 191),          # slivers on the hull, boxes far larger than triangles
            "several_blocks": lambda: grid_case((200, 264), 16, [[(4, 7)]], 192),   # 52 800 pixels: 207 blocks of 256, the last partial
            "half_pixel": lambda: grid_case((37, 53), 6, ODD_MASKS[:2], 193, scale=0.5)}[name]()   # delta_x = 0.5: the scaling quirk
    for a in ("x", "y", "vx", "vy"):
        made[a].setflags(write=False)
    return made


CASES = ("odd_grid", "scattered", "several_blocks", "half_pixel")


@functools.lru_cache(maxsize=None)
def restated(name):
    """(v_x, v_y, speed, counts) of a case, computed once."""
    c = case(name)
    out = upsample(c["x"], c["y"], c["vx"], c["vy"], c["shape"])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frame_list(name):
    """[(tri, values, grad)] of a case's frames, as the host part makes them."""
    c = case(name)
    made = []
    for k in range(len(c["x"])):
        points, values = valid_points(c["x"][k], c["y"][k], c["vx"][k], c["vy"][k])
        made.append(frame_tables(points, values) + (values,))
    return [(tri, values, grad) for tri, grad, values in made]


@functools.lru_cache(maxsize=None)
def gridded(name):
    c = case(name)
    out = griddata(c["x"], c["y"], c["vx"], c["vy"], c["shape"])
    for a in out:
        a.setflags(write=False)
    return out


def pivlab_result(x, y, u, v):
    """The four (F, R, C) arrays as scipy.io.loadmat returns a PIVlab file: object arrays of shape (F, 1) whose [k][0] is 2-D."""
    def boxed(a):
        o = np.empty((len(a), 1), dtype=object)
        for k in range(len(a)):
            o[k, 0] = np.array(a[k])
        return o
    return {"x": boxed(x), "y": boxed(y), "u_original": boxed(u), "v_original": boxed(v)}
