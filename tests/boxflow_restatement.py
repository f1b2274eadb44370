"""Vectorised numpy restatement of the box least-squares flow (the reference's conduct_optical_flow_jit, OF.py:24-157), for
image and box sizes no fixture covers.  Test infrastructure only: separable DIRECT window sums (shifted slices, no running
windows), both settings of ``reference_quirks``, and per pixel the conditioning number of the closed form,
``kappa = sum |terms of the determinant| / |determinant|``."""
import numpy as np


def _window_sum(q, h):
    """out[i, j] = sum of q over rows i-h..i+h and columns j-h..j+h inside the array (q is zero where no window reaches)."""
    n_i, n_j = q.shape
    rows = np.zeros_like(q)
    for d in range(-min(h, n_j - 1), min(h, n_j - 1) + 1):
        if d >= 0:
            rows[:, :n_j - d] += q[:, d:]
        else:
            rows[:, -d:] += q[:, :n_j + d]
    out = np.zeros_like(q)
    for d in range(-min(h, n_i - 1), min(h, n_i - 1) + 1):
        if d >= 0:
            out[:n_i - d, :] += rows[d:, :]
        else:
            out[-d:, :] += rows[:n_i + d, :]
    return out


def box_flow(movie, box_size=15, delta_x=1.0, delta_t=1.0, include_remodelling=False, reference_quirks=True):
    """Returns a dict with ``v_x, v_y, speed, net_remodelling, kappa`` of shape ``(T-1, N_i, N_j)``; ``kappa`` is inf where
    the determinant is zero."""
    movie = np.asarray(movie).astype(np.float64)
    T, n_i, n_j = movie.shape
    h = int(box_size / 2)
    cend = min(n_i, n_j) if reference_quirks else n_j
    scale = delta_x / delta_t
    out = {k: np.zeros((T - 1, n_i, n_j)) for k in ("v_x", "v_y", "speed", "net_remodelling", "kappa")}
    ii, jj = np.arange(n_i)[:, None], np.arange(n_j)[None, :]
    count = ((np.minimum(ii + h + 1, n_i) - np.maximum(ii - h, 0)) * (np.minimum(jj + h + 1, n_j) - np.maximum(jj - h, 0))).astype(np.float64)
    n = np.full((n_i, n_j), float(box_size * box_size)) if reference_quirks else count
    for k in range(1, T):
        c, p = movie[k], movie[k - 1]
        dx, dy = np.zeros_like(c), np.zeros_like(c)
        dx[1:-1, 1:-1] = (c[2:, 1:-1] + p[2:, 1:-1] - c[:-2, 1:-1] - p[:-2, 1:-1]) / 4
        dy[1:-1, 1:-1] = (c[1:-1, 2:] + p[1:-1, 2:] - c[1:-1, :-2] - p[1:-1, :-2]) / 4
        dI = c - p
        for a in (dx, dy, dI):
            a[:, cend:] = 0.0
        A, B, D = _window_sum(dx * dx, h), _window_sum(dx * dy, h), _window_sum(dy * dy, h)
        s1, s2 = _window_sum(dI * dx, h), _window_sum(dI * dy, h)
        with np.errstate(all="ignore"):
            if not include_remodelling:
                det = A * D - B * B
                Vx = (-D * s1 + B * s2) / det
                Vy = (-A * s2 + B * s1) / det
                speed = np.sqrt(Vx * Vx + Vy * Vy)
                gamma = np.zeros_like(Vx)
                kappa = (np.abs(A * D) + np.abs(B * B)) / np.abs(det)
            else:
                C, E, s3 = _window_sum(dx, h), _window_sum(dy, h), _window_sum(dI, h)
                t = [n * A * D, A * (E * E), n * (B * B), C * C * D, 2 * B * C * E]
                det = t[0] - t[1] - t[2] - t[3] + t[4]
                Vx = ((E * E - n * D) * s1 + (n * B - C * E) * s2 + (C * D - B * E) * s3) / det
                Vy = ((n * B - C * E) * s1 + (C * C - n * A) * s2 + (A * E - B * C) * s3) / det
                gamma = -((B * E - C * D) * s1 + (B * C - A * E) * s2 + (A * D - B * B) * s3) / det
                singular = det == 0.0
                if reference_quirks:
                    speed = np.zeros_like(Vx)
                    Vx, Vy, gamma = (np.where(singular, 0.0, f) for f in (Vx, Vy, gamma))
                else:
                    speed = np.sqrt(Vx * Vx + Vy * Vy)
                    Vx, Vy, gamma, speed = (np.where(singular, np.nan, f) for f in (Vx, Vy, gamma, speed))
                kappa = sum(np.abs(x) for x in t) / np.abs(det)
            kappa = np.where(det == 0.0, np.inf, kappa)
        out["v_x"][k - 1], out["v_y"][k - 1], out["speed"][k - 1] = Vx * scale, Vy * scale, speed * scale
        out["net_remodelling"][k - 1], out["kappa"][k - 1] = gamma, kappa
    return out


def kappa_max(kappa, *reference_fields):
    """Largest conditioning number over the pixels where the determinant is non-zero and every given field is finite."""
    ok = np.isfinite(kappa)
    for f in reference_fields:
        ok &= np.isfinite(f)
    return float(kappa[ok].max()) if ok.any() else 1.0
