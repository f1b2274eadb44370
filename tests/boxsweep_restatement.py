"""Numpy restatements for the box-size sweep (vary_boxsize).  Test infrastructure only.

``box_sweep``: the ring-growing recurrence of the sweep in float64 - per quantity a row-sum, a column-sum and a window-sum
plane that start as the pixel's own term and grow by one ring per step, terms only ever added - behind the closed form of
``boxflow_restatement.box_flow``.  ``box_flow_extended``: the same fields from direct window sums with every operation in
``np.longdouble``, the yardstick for the error of a float64 summation order."""
import numpy as np

from boxflow_restatement import _window_sum


def _derived(c, p, cend):
    dx, dy = np.zeros_like(c), np.zeros_like(c)
    dx[1:-1, 1:-1] = (c[2:, 1:-1] + p[2:, 1:-1] - c[:-2, 1:-1] - p[:-2, 1:-1]) / 4
    dy[1:-1, 1:-1] = (c[1:-1, 2:] + p[1:-1, 2:] - c[1:-1, :-2] - p[1:-1, :-2]) / 4
    dI = c - p
    for a in (dx, dy, dI):
        a[:, cend:] = 0
    return dx, dy, dI


def _terms(dx, dy, dI, include_remodelling):
    t = [dx * dx, dx * dy, dy * dy, dI * dx, dI * dy]
    return t + [dx, dy, dI] if include_remodelling else t


def _shift(a, di, dj):
    """b[i, j] = a[i + di, j + dj], 0 outside the array."""
    n_i, n_j = a.shape
    b = np.zeros_like(a)
    if abs(di) >= n_i or abs(dj) >= n_j:
        return b
    b[max(-di, 0):n_i - max(di, 0), max(-dj, 0):n_j - max(dj, 0)] = a[max(di, 0):n_i + min(di, 0), max(dj, 0):n_j + min(dj, 0)]
    return b


def _closed_form(S, n, include_remodelling, reference_quirks, scale):
    """The closed form of boxflow_restatement.box_flow on window sums ``S`` (any float dtype)."""
    A, B, D, s1, s2 = S[:5]
    with np.errstate(all="ignore"):
        if not include_remodelling:
            det = A * D - B * B
            Vx = (-D * s1 + B * s2) / det
            Vy = (-A * s2 + B * s1) / det
            speed = np.sqrt(Vx * Vx + Vy * Vy)
            gamma = np.zeros_like(Vx)
            kappa = (np.abs(A * D) + np.abs(B * B)) / np.abs(det)
        else:
            C, E, s3 = S[5:]
            t = [n * A * D, A * (E * E), n * (B * B), C * C * D, 2 * B * C * E]
            det = t[0] - t[1] - t[2] - t[3] + t[4]
            Vx = ((E * E - n * D) * s1 + (n * B - C * E) * s2 + (C * D - B * E) * s3) / det
            Vy = ((n * B - C * E) * s1 + (C * C - n * A) * s2 + (A * E - B * C) * s3) / det
            gamma = -((B * E - C * D) * s1 + (B * C - A * E) * s2 + (A * D - B * B) * s3) / det
            singular = det == 0
            if reference_quirks:
                speed = np.zeros_like(Vx)
                Vx, Vy, gamma = (np.where(singular, 0, f) for f in (Vx, Vy, gamma))
            else:
                speed = np.sqrt(Vx * Vx + Vy * Vy)
                Vx, Vy, gamma, speed = (np.where(singular, np.nan, f) for f in (Vx, Vy, gamma, speed))
            kappa = sum(np.abs(x) for x in t) / np.abs(det)
        kappa = np.where(det == 0, np.inf, kappa)
    return Vx * scale, Vy * scale, speed * scale, gamma, kappa


def _count(n_i, n_j, h, box, reference_quirks, dtype):
    ii, jj = np.arange(n_i)[:, None], np.arange(n_j)[None, :]
    count = (np.minimum(ii + h + 1, n_i) - np.maximum(ii - h, 0)) * (np.minimum(jj + h + 1, n_j) - np.maximum(jj - h, 0))
    return np.full((n_i, n_j), box * box, dtype=dtype) if reference_quirks else count.astype(dtype)


def box_sweep(movie, box_sizes, delta_x=1.0, delta_t=1.0, include_remodelling=False, reference_quirks=True):
    """One dict ``v_x, v_y, speed, net_remodelling, kappa`` of shape ``(T-1, N_i, N_j)`` per entry of ``box_sizes``."""
    movie = np.asarray(movie).astype(np.float64)
    T, n_i, n_j = movie.shape
    boxes = [int(b) for b in box_sizes]
    cend = min(n_i, n_j) if reference_quirks else n_j
    out = [{k: np.zeros((T - 1, n_i, n_j)) for k in ("v_x", "v_y", "speed", "net_remodelling", "kappa")} for _ in boxes]
    h_of = [min(int(b / 2), max(n_i, n_j)) for b in boxes]
    for k in range(1, T):
        t = _terms(*_derived(movie[k], movie[k - 1], cend), include_remodelling)
        R, C, W = [0.0 + q for q in t], [0.0 + q for q in t], [0.0 + q for q in t]
        for h in range(0, max(h_of) + 1):
            if h >= 1:
                C_prev = C
                R = [(r + _shift(q, 0, -h)) + _shift(q, 0, h) for r, q in zip(R, t)]
                W = [(((w + _shift(r, -h, 0)) + _shift(r, h, 0)) + _shift(c, 0, -h)) + _shift(c, 0, h) for w, r, c in zip(W, R, C_prev)]
                C = [(c + _shift(q, -h, 0)) + _shift(q, h, 0) for c, q in zip(C, t)]
            for b, box in enumerate(boxes):
                if h_of[b] == h:
                    n = _count(n_i, n_j, h, box, reference_quirks, np.float64)
                    fields = _closed_form(W, n, include_remodelling, reference_quirks, delta_x / delta_t)
                    for name, f in zip(("v_x", "v_y", "speed", "net_remodelling", "kappa"), fields):
                        out[b][name][k - 1] = f
    return out


def box_flow_extended(movie, box_size, delta_x=1.0, delta_t=1.0, include_remodelling=False, reference_quirks=True):
    """The fields of one box from direct window sums, every operation in ``np.longdouble``."""
    movie = np.asarray(movie).astype(np.longdouble)
    T, n_i, n_j = movie.shape
    h = int(box_size / 2)
    cend = min(n_i, n_j) if reference_quirks else n_j
    out = {k: np.zeros((T - 1, n_i, n_j), dtype=np.longdouble) for k in ("v_x", "v_y", "speed", "net_remodelling", "kappa")}
    n = _count(n_i, n_j, h, int(box_size), reference_quirks, np.longdouble)
    scale = np.longdouble(delta_x) / np.longdouble(delta_t)
    for k in range(1, T):
        S = [_window_sum(q, h) for q in _terms(*_derived(movie[k], movie[k - 1], cend), include_remodelling)]
        for name, f in zip(("v_x", "v_y", "speed", "net_remodelling", "kappa"), _closed_form(S, n, include_remodelling, reference_quirks, scale)):
            out[name][k - 1] = f
    return out
