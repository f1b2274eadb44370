"""Right-preconditioned restarted GMRES in numpy float64, as gmres_phase (csrc/vof.hip) and the k_gm_* kernels (csrc/vof_device.hpp)
run it: classical Gram-Schmidt applied twice (CGS2), a Givens-rotated Hessenberg matrix, x = x_c + M (V_k y_k) at the end of a cycle,
restart from the true residual b - A x.  `A` and `M` are callables on arrays of one shape, so the same code runs on the oracle's
operator with the prototype's cycle and on a black box made of the library's debug entry points.

The restatement returns the iterate "as if the solve were cut after step k" for every k, which is what the public entry returns
with `max_iterations=k`.  The checks below are stated over such a list of iterates and need no knowledge of how it was made:

  optimality  r_k = b - A x_k is orthogonal to A (x_j - x_c) for every step j of the cycle of k up to k itself (x_c: the iterate the
              cycle started from).  This is the minimal-residual property over the nested spaces and needs no M.
  monotone    the residual norm never grows, inside a cycle or across a restart.
  span        x_k - x_c lies in M K_k(A M, r_c).

VARIANTS names three deliberately broken orthogonalisations / rotations, used to show what the checks see and what they do not.
"""
import numpy as np

# Steps whose relative residual is below this do not enter the optimality figure: rounding in r_k = b - A x_k takes over the ratio.
RESIDUAL_FLOOR = 1e-6
MONOTONE_SLACK = 1e-10
SPAN_STEPS = 12
# drop_v8: the coefficient of basis vector 8 (the first of the second chunk of GM_NV = 8) is left out of the update of w.
# flip_rotation: the sine of rotation 2 changes sign after its own column, so every later column is rotated wrongly.
# no_second_h: the second Gram-Schmidt pass corrects w but its coefficients are not added to h (harmless in exact arithmetic).
VARIANTS = ("drop_v8", "flip_rotation", "no_second_h")


def _dot(a, b):
    return float(np.vdot(a.ravel(), b.ravel()))


def _norm(a):
    return float(np.linalg.norm(a.ravel()))


def _dot_reversed(a, b):
    return float(np.vdot(a.ravel()[::-1], b.ravel()[::-1]))


def _norm_reversed(a):
    return float(np.sqrt(_dot_reversed(a, a)))


class Trace:
    """iterates[k]: x after k steps (iterates[0] the initial guess); estimates[k - 1]: |g[k]| / |b| of step k; cycle_starts: the step
    counts at which a cycle began; converged / stagnated: how the solve ended (neither: the step limit); false_ends: the cycles that
    ended because the estimate met the tolerance while the true residual at the restart did not."""

    def __init__(self):
        self.iterates, self.estimates, self.cycle_starts = [], [], []
        self.converged = self.stagnated = False
        self.false_ends = 0

    @property
    def iterations(self):
        return len(self.iterates) - 1


def restarted_gmres(A, M, b, x0=None, m=100, rtol=0.0, max_steps=24, variant=None, reverse_sums=False):
    """GMRES(m) with the library's rules: a cycle ends at m columns, when the residual estimate meets rtol |b|, on a breakdown or at
    the step limit; the next one starts from the true residual, which alone decides `converged`; a cycle that ended by its estimate
    and is followed by a true residual that has not even halved ends the solve (`stagnated`, k_gm_init).  `reverse_sums` adds up
    every dot product and norm from the other end: the same method in another, equally good order of the sums."""
    assert variant is None or variant in VARIANTS
    dot, norm = (_dot_reversed, _norm_reversed) if reverse_sums else (_dot, _norm)
    t = Trace()
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    bn = norm(b)
    t.iterates.append(x.copy())
    steps, previous, by_estimate = 0, np.inf, False
    while True:
        r = b - A(x)
        rn = norm(r)
        if rn <= rtol * bn:
            t.converged = True
            break
        t.false_ends += int(by_estimate)
        if steps >= max_steps or not np.isfinite(rn):
            break
        if previous < np.inf and by_estimate and rn * rn >= 0.25 * previous * previous:
            t.stagnated = True
            break
        by_estimate, previous = False, rn
        t.cycle_starts.append(steps)
        x_c = x
        V = [r / rn]
        R = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = rn
        for j in range(m):
            w = A(M(V[j]))
            h = np.zeros(j + 2)
            for second in (False, True):
                c = np.array([dot(V[i], w) for i in range(j + 1)])      # classical: every product against the same w
                if not second:
                    h[:j + 1] = c
                elif variant != "no_second_h":
                    h[:j + 1] += c
                for i in range(j + 1):
                    if variant == "drop_v8" and i == 8:
                        continue
                    w = w - c[i] * V[i]
            hn = norm(w)
            h[j + 1] = hn
            for i in range(j):
                h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], -sn[i] * h[i] + cs[i] * h[i + 1]
            d = float(np.hypot(h[j], h[j + 1]))
            cs[j], sn[j] = (h[j] / d, h[j + 1] / d) if d > 0.0 else (1.0, 0.0)
            h[j], h[j + 1] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            R[:j + 1, j] = h[:j + 1]
            if variant == "flip_rotation" and j == 2:
                sn[j] = -sn[j]
            steps += 1
            y = np.zeros(j + 1)
            for i in range(j, -1, -1):
                y[i] = (g[i] - R[i, i + 1:j + 1] @ y[i + 1:]) / R[i, i] if R[i, i] != 0.0 else 0.0
            x = x_c + M(sum(y[i] * V[i] for i in range(j + 1)))
            t.iterates.append(x.copy())
            t.estimates.append(abs(g[j + 1]) / bn)
            by_estimate = abs(g[j + 1]) <= rtol * bn
            if by_estimate or not hn > 0.0 or not d > 0.0 or steps >= max_steps:
                break
            V.append(w / hn)
    return t


def residuals(A, b, iterates):
    """|b - A x_k| / |b| for every iterate of the list."""
    bn = _norm(b)
    return [_norm(b - A(x)) / bn for x in iterates]


def cycle_base(k, m):
    """The step count at which the cycle of step k >= 1 began, for cycles that all ran to the restart length m: steps c + 1 ... c + m
    belong to the cycle that started from the iterate after c steps."""
    return ((k - 1) // m) * m


def optimality(A, b, iterates, m, floor=RESIDUAL_FLOOR):
    """(worst, counted): the largest |<r_k, u>| / (|r_k| |u|) over the steps k >= 1 whose relative residual is at least `floor`,
    u = A (x_j - x_c) for every step j of the cycle of k with j <= k, and the number of steps that entered.  `iterates[0]` is the
    iterate GMRES started from; the cycles are taken to be full (true while the residual is above the solve's tolerance)."""
    bn = _norm(b)
    u = {}
    worst, counted = 0.0, 0
    for k in range(1, len(iterates)):
        c0 = cycle_base(k, m)
        d = A(iterates[k] - iterates[c0])
        u[k] = (d, _norm(d))
        r = b - A(iterates[k])
        rn = _norm(r)
        if rn < floor * bn:
            continue
        counted += 1
        for j in range(c0 + 1, k + 1):
            if u[j][1] > 0.0:
                worst = max(worst, abs(_dot(r, u[j][0])) / (rn * u[j][1]))
    return worst, counted


def monotone(res, slack=MONOTONE_SLACK):
    """The largest res_k / res_{k-1} of the list; the property holds when it is at most 1 + slack."""
    return max((res[k] / res[k - 1] for k in range(1, len(res)) if res[k - 1] > 0.0), default=0.0)


def krylov_image(A, M, r_c, steps=SPAN_STEPS):
    """M q_1 ... M q_steps for an orthonormal basis q of K_steps(A M, r_c) (Arnoldi, modified Gram-Schmidt applied twice)."""
    q = [r_c / _norm(r_c)]
    image = []
    for k in range(steps):
        image.append(M(q[k]))
        w = A(image[k])
        for _ in range(2):
            for v in q:
                w = w - _dot(v, w) * v
        wn = _norm(w)
        if not wn > 0.0:
            break
        q.append(w / wn)
    return image


def span_defects(image, base, iterates):
    """Relative least-squares defect of x_k - base in span(image[:k]) for k = 1 ... min(len(iterates), len(image)); iterates[k - 1]
    is the iterate after k steps of the cycle that started from `base`."""
    out = []
    for k in range(1, min(len(iterates), len(image)) + 1):
        B = np.stack([v.ravel() for v in image[:k]], axis=1)
        d = (iterates[k - 1] - base).ravel()
        coef = np.linalg.lstsq(B, d, rcond=None)[0]
        out.append(_norm(d - B @ coef) / max(_norm(d), 1e-300))
    return out
