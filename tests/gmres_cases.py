"""The cases that pin restarted GMRES (tests/test_gmres_restatement_cpu.py, tests/test_gpu_gmres_pin.py): the smallest images at
which gmres_phase can still go wrong - two interior levels with the LDS tail (18 x 18, 34 x 34) and one non-square image - in the
regimes of DESIGN.md section 7, with restart lengths on both sides of the chunk of GM_NV = 8 basis vectors.

Every solve of these cases uses krylov_method="gmres", preconditioner="multigrid", warm_start_stride=0, zero initial fields and
vcycle_precision="float64", and is cut with max_iterations = 1 ... STEPS: the cuts cross columns 8, 9, 16 and 17 of a cycle and at
least two restarts of the lengths 5 and 9.
"""
import collections
import functools

import numpy as np

from oracle import mg_prototype as mg
from oracle import vof_oracle as orc

import direct_restatement as dr
import gmres_restatement as gr

STEPS = 24
CUT_RTOL = 1e-10                     # the tolerance of the cut solves: far below RESIDUAL_FLOOR, so every counted cycle is a full one
# (speed_alpha, remodelling_alpha): N the benchmark regime on float data, T and W grad-div dominated on 8-bit data (W the harder)
REGIMES = dict(N=(1.0, 1e4), T=(1e4, 1e2), W=(2e3, 1.0))
# the library's default cycle: (2, 2) sweeps on level 0, (1, 1) below, level 1 visits level 2 three times (vof_default_params)
CYCLE = dict(sweeps=(2, 2, 1, 1), w_cycle_level=1, visits=3)
# A case "claims chunk edges" when its cuts cross columns 9, 16 and 17 of a cycle with the residual still above RESIDUAL_FLOOR;
# tests/test_gmres_restatement_cpu.py holds the admission (at least CLAIM_STEPS such steps).
CLAIM_STEPS = 17

Case = collections.namedtuple("Case", "shape regime restart coarse quirks claims")

CASES = (
    # the rows of the prototype's table: coarse_precision="float64", the format the prototype's cycle restates
    Case((34, 34), "T", 100, "float64", True, False),
    Case((34, 34), "T", 9, "float64", True, False),
    Case((34, 34), "T", 5, "float64", True, False),
    Case((34, 34), "W", 100, "float64", True, True),
    Case((34, 34), "W", 17, "float64", True, True),
    Case((34, 34), "W", 9, "float64", True, False),
    Case((34, 34), "W", 5, "float64", True, False),
    Case((18, 18), "W", 100, "float64", True, True),
    Case((18, 18), "W", 17, "float64", True, True),
    Case((18, 18), "W", 9, "float64", True, False),
    Case((18, 18), "W", 5, "float64", True, False),
    # the default stencil format (the cycle is linear in either), the non-square image, GM_MAXM, reference_quirks off, the easy partner
    Case((34, 34), "W", 128, "float8", True, True),
    Case((20, 70), "W", 9, "float8", True, False),
    Case((20, 70), "T", 100, "float64", True, False),
    Case((34, 34), "W", 17, "float64", False, False),     # (its residual passes the floor after 16 steps: no claim)
    Case((34, 34), "N", 100, "float8", True, False),
)
EASY = len(CASES) - 1


def case_id(i):
    c = CASES[i] if isinstance(i, int) else i
    return "%dx%d-%s-m%d-%s%s" % (c.shape[0], c.shape[1], c.regime, c.restart, c.coarse, "" if c.quirks else "-noquirks")


@functools.lru_cache(maxsize=None)
def movie(shape, regime):
    """Two frames of the oracle's texture, cut to the shape; 8-bit (rounded to 0 ... 255) except in the float regime N."""
    tex = orc.make_texture_stack(max(shape), 2, seed=1)[:, :shape[0], :shape[1]]
    out = np.ascontiguousarray(tex if regime == "N" else np.round(tex * 255.0))
    out.setflags(write=False)
    return out


def solve_kwargs(c, **over):
    """Keyword arguments of variational_optical_flow for a case."""
    alpha, beta = REGIMES[c.regime]
    kw = dict(speed_alpha=alpha, remodelling_alpha=beta, reference_quirks=c.quirks, coarse_precision=c.coarse,
              vcycle_precision="float64", krylov_method="gmres", gmres_restart=c.restart, preconditioner="multigrid",
              warm_start_stride=0, rtol=CUT_RTOL, return_stats=True)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def system(shape, regime, quirks):
    """(A, M, b) of the case's pair on the CPU: the oracle's operator and right-hand side, the prototype's cycle as M."""
    mv = movie(shape, regime)
    alpha, beta = REGIMES[regime]
    H = mg.Hierarchy(mv[0], alpha, beta, quirks)
    return (lambda x: orc.apply_operator_interior(mv[0], x, alpha, beta, quirks),
            lambda r: H.cycle(r, **CYCLE),
            orc.rhs_interior(mv[0], mv[1], quirks))


@functools.lru_cache(maxsize=None)
def _restated(shape, regime, quirks, m, variant):
    A, M, b = system(shape, regime, quirks)
    t = gr.restarted_gmres(A, M, b, m=m, rtol=CUT_RTOL, max_steps=STEPS, variant=variant)
    res = gr.residuals(A, b, t.iterates)
    worst, counted = gr.optimality(A, b, t.iterates, m)
    return dict(trace=t, residuals=res, cosine=worst, counted=counted, growth=gr.monotone(res))


def restated(c, variant=None):
    """The restatement's STEPS cut iterates of a case with the prototype's M and their figures; computed once per process.  (Within
    STEPS steps every restart length above STEPS is the same method.)"""
    return _restated(c.shape, c.regime, c.quirks, min(c.restart, STEPS + 1), variant)


@functools.lru_cache(maxsize=None)
def restated_span(shape, regime, quirks):
    """The restatement's own span defects for the first cycle (steps 1 ... SPAN_STEPS, restart length above that)."""
    A, M, b = system(shape, regime, quirks)
    t = _restated(shape, regime, quirks, STEPS + 1, None)["trace"]
    return gr.span_defects(gr.krylov_image(A, M, b), t.iterates[0], t.iterates[1:gr.SPAN_STEPS + 1])


# the distinct (shape, regime, quirks) systems of the table, in its order
SYSTEMS = tuple(dict.fromkeys((c.shape, c.regime, c.quirks) for c in CASES))


@functools.lru_cache(maxsize=None)
def attainable(shape, regime, quirks):
    """eps |A| |x| / |b| of a system (direct_restatement.attainable): the level at which rounding alone moves a residual b - A x."""
    mv = movie(shape, regime)
    alpha, beta = REGIMES[regime]
    return dr.attainable(*dr.system(mv[0], mv[1], alpha, beta, quirks))
