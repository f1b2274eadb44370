"""Vectorised numpy restatement of the Liu-Shen Jacobi flow (the reference's liu_shen_optical_flow_jit, OF.py:426-673), for
image sizes and iteration counts no fixture covers.  Test infrastructure only.  Every pixel of a pair is updated from the old
iterate with shifted slices of reflect-padded planes and the closed-form inverse of its 2 x 2 block.

Two mutations switch the reference's edge rules off, for the check that the fixtures exercise them:
``mirror_bar``  the 8-neighbour sums read the mirrored border where the reference takes neighbours outside the image as zero
``n_eight``     the matrix uses n = 8 everywhere where the reference has 5 on an edge line and 3 in a corner."""
import numpy as np


def _pad(a):
    """One-pixel border as apply_constant_boundary_condition leaves it: rows first, then columns (reflection without the edge)."""
    return np.pad(a, 1, mode="reflect")


def _shifts(q):
    """The nine shifted views q[i + di, j + dj] of a padded plane, keyed by (di, dj)."""
    n_i, n_j = q.shape[0] - 2, q.shape[1] - 2
    return {(di, dj): q[1 + di:1 + di + n_i, 1 + dj:1 + dj + n_j] for di in (-1, 0, 1) for dj in (-1, 0, 1)}


def _bar(v, mirror):
    """Sum of the eight neighbours in the reference's order (OF.py:541-548); outside the image they count as zero."""
    s = _shifts(_pad(v) if mirror else np.pad(v, 1))
    return s[-1, 0] + s[1, 0] + s[0, 1] + s[0, -1] + s[-1, -1] + s[-1, 1] + s[1, -1] + s[1, 1]


def boundary_prefactor(n_i, n_j):
    n = np.full((n_i, n_j), 8.0)
    n[[0, -1], :] = 5.0
    n[:, [0, -1]] = 5.0
    for i in (0, -1):
        for j in (0, -1):
            n[i, j] = 3.0
    return n


def liu_shen(movie, delta_x=1.0, delta_t=1.0, alpha=100, remodelling_alpha=1.0, initial_v_x=0.0, initial_v_y=0.0,
             initial_remodelling=0.0, max_iterations=10, tolerance=1e-9, include_remodelling=True, *, mirror_bar=False,
             n_eight=False):
    """Returns ``(v_x, v_y, speed, remodelling, max_iterations - 1)`` as the reference does; the initial fields may be
    scalars, ``(N_i, N_j)`` planes or ``(T - 1, N_i, N_j)`` stacks."""
    movie = np.asarray(movie).astype(np.float64)
    T, n_i, n_j = movie.shape
    if max_iterations < 1 or min(n_i, n_j) < 3:
        raise ValueError("max_iterations >= 1 and image sides >= 3 are required")
    shape = (T - 1, n_i, n_j)
    all_v_x = np.array(np.broadcast_to(np.asarray(initial_v_x, dtype=np.float64) * delta_t / delta_x, shape))
    all_v_y = np.array(np.broadcast_to(np.asarray(initial_v_y, dtype=np.float64) * delta_t / delta_x, shape))
    remodelling = np.array(np.broadcast_to(np.asarray(initial_remodelling, dtype=np.float64), shape))
    n = np.full((n_i, n_j), 8.0) if n_eight else boundary_prefactor(n_i, n_j)
    for k in range(T - 1):
        p, c = _shifts(_pad(movie[k])), _shifts(_pad(movie[k + 1]))
        I = p[0, 0]
        Ix, Iy = (p[1, 0] - p[-1, 0]) / 2, (p[0, 1] - p[0, -1]) / 2
        Ixt = (c[1, 0] - c[-1, 0] - p[1, 0] + p[-1, 0]) / 2
        Iyt = (c[0, 1] - c[0, -1] - p[0, 1] + p[0, -1]) / 2
        Ixx = p[1, 0] + p[-1, 0] - 2 * I
        Iyy = p[0, 1] + p[0, -1] - 2 * I
        Ixy = (p[1, 1] - p[1, -1] - p[-1, 1] + p[-1, -1]) / 4
        a = I * Ixx - 2 * I ** 2 - n * alpha
        b = I * Ixy
        d = I * Iyy - 2 * I ** 2 - n * alpha
        with np.errstate(all="ignore"):
            det = a * d - b * b
        v_x, v_y = all_v_x[k], all_v_y[k]
        for _ in range(max_iterations):
            x, y = _shifts(_pad(v_x)), _shifts(_pad(v_y))
            dxVx, dyVx = (x[1, 0] - x[-1, 0]) / 2, (x[0, 1] - x[0, -1]) / 2
            dxyVx = (x[1, 1] - x[1, -1] - x[-1, 1] + x[-1, -1]) / 4
            dxVy, dyVy = (y[1, 0] - y[-1, 0]) / 2, (y[0, 1] - y[0, -1]) / 2
            dxyVy = (y[1, 1] - y[1, -1] - y[-1, 1] + y[-1, -1]) / 4
            F0 = (-I * Ixt - I * (2 * Ix * dxVx + Iy * dxVy + Ix * dyVy) - I ** 2 * ((x[1, 0] + x[-1, 0]) + dxyVy)
                  - alpha * _bar(v_x, mirror_bar))
            F1 = (-I * Iyt - I * (2 * Iy * dyVy + Ix * dyVx + Iy * dxVx) - I ** 2 * ((y[0, 1] + y[0, -1]) + dxyVx)
                  - alpha * _bar(v_y, mirror_bar))
            with np.errstate(all="ignore"):
                v_x, v_y = (d * F0 - b * F1) / det, (a * F1 - b * F0) / det
        all_v_x[k], all_v_y[k] = v_x, v_y
    all_v_x *= delta_x / delta_t
    all_v_y *= delta_x / delta_t
    return all_v_x, all_v_y, np.sqrt(all_v_x ** 2 + all_v_y ** 2), remodelling, max_iterations - 1


def error(got_x, got_y, ref_x, ref_y):
    """e = max|x - ref| / max(|ref v_x|, |ref v_y|) over both fields."""
    scale = max(float(np.abs(ref_x).max()), float(np.abs(ref_y).max()))
    return max(float(np.abs(np.asarray(got_x) - ref_x).max()), float(np.abs(np.asarray(got_y) - ref_y).max())) / scale
