"""Restarted GMRES (gmres_phase of csrc/vof.hip, the k_gm_* kernels of csrc/vof_device.hpp, GmresState of csrc/vof_shared.hpp) pinned through the public
entry, step by step.

The other GMRES tests ask for the converged answer, and a method that restarts from b - A x repairs almost any error inside a cycle
at the price of extra steps.  Here the iteration is cut with max_iterations = 1 ... STEPS and the cut iterates are checked for what
only a correct cycle gives (tests/gmres_restatement.py): the residual is orthogonal to A (x_j - x_c) for every earlier step of the
cycle, it never grows, the update lies in M K_k(A M, r_c), and the step counts are those of the restatement on the library's own A
and M.  Then the hand-over from BiCGStab, batches whose pairs leave a cycle at different steps, a context that has served another
restart length, lanes on a fresh context, and a tolerance below the attainable accuracy.

Every bar that is a multiple of a restatement value is stated beside OVER; the measured figures are in profiles/gmres_pin_summary.md.
"""
import functools

import numpy as np
import pytest

from oracle import vof_oracle as orc

import gmres_cases as gc
import gmres_restatement as gr
import test_gpu_lanes as lanes

pytestmark = pytest.mark.gpu

# Cosine and span defect of the GPU iterates: at most OVER times the restatement's own figure for the same case.  Both are zero
# in exact arithmetic, so either figure is rounding alone; library and restatement are the same method and differ in the order of
# the sums inside the dot products, the cycle and the operator.  Two decades is the margin tests/test_gpu_direct_pin.py gives a
# different but equivalent order; the mildest wrong method of tests/test_gmres_restatement_cpu.py sits more than three decades up.
OVER = 100.0
FIELDS = ("v_x", "v_y", "remodelling", "speed")
CASE_IDS = [gc.case_id(i) for i in range(len(gc.CASES))]


@pytest.fixture(scope="module")
def of():
    from opticalflow_amd import optical_flow
    return optical_flow


@pytest.fixture(scope="module")
def native():
    from opticalflow_amd import _native
    return _native


def interior(res, pair=0):
    return np.stack([np.asarray(res[k][pair]) for k in ("v_x", "v_y", "remodelling")])[:, 1:-1, 1:-1]


def oracle_system(c):
    """(A, b) of a case on the CPU: the oracle's interior operator and right-hand side."""
    mv = gc.movie(c.shape, c.regime)
    alpha, beta = gc.REGIMES[c.regime]
    return (lambda x: orc.apply_operator_interior(mv[0], x, alpha, beta, c.quirks)), orc.rhs_interior(mv[0], mv[1], c.quirks)


_cuts = {}


def cut_iterates(of, i):
    """Case i solved with max_iterations = 1 ... STEPS: (iterates with the zero guess in front, stats per cut); once per module."""
    if i not in _cuts:
        c = gc.CASES[i]
        xs, stats = [np.zeros((3, c.shape[0] - 2, c.shape[1] - 2))], []
        for k in range(1, gc.STEPS + 1):
            res = of.variational_optical_flow(gc.movie(c.shape, c.regime), max_iterations=k, **gc.solve_kwargs(c))
            xs.append(interior(res))
            stats.append(res["stats"][0].copy())
        _cuts[i] = (xs, stats)
    return _cuts[i]


def check_steps(stats, first=0):
    """`iterations` is the cut and `converged` false until the solve converges; from then on every cut returns that solve.  Returns
    the number of leading cuts that did not converge."""
    done = None
    for k, st in enumerate(stats, start=1):
        if done is None and st["converged"]:
            done = int(st["iterations"])
            assert done == first + k, (k, st)
        if done is None:
            assert st["iterations"] == first + k and not st["converged"], (k, st)
        else:
            assert st["iterations"] == done and st["converged"], (k, st)
    return len(stats) if done is None else done - first - 1


def residual_mismatch(c, stats, res):
    """The library's independent `relative_residual` of every cut against the CPU residual res[k] of the fields it returned, as the
    worst |difference| / (1e-6 res[k] + 2 level): at most 1 means equal to 1e-6 relative, up to the rounding of the two evaluations of
    b - A x, each of which moves a residual by level = eps |A| |x| / |b| (gmres_cases.attainable) whatever its size."""
    level = gc.attainable(c.shape, c.regime, c.quirks)
    return max(abs(float(st["relative_residual"]) - res[k]) / (1e-6 * res[k] + 2.0 * level) for k, st in enumerate(stats, start=1))


@pytest.mark.parametrize("i", range(len(gc.CASES)), ids=CASE_IDS)
def test_every_cut_iterate_is_the_minimiser_of_its_cycle(of, i):
    """(1) Per case: the step count of every cut, the library's residual against the CPU residual of the returned fields, the
    optimality of every step above the floor and a residual that never grows."""
    c = gc.CASES[i]
    A, b = oracle_system(c)
    xs, stats = cut_iterates(of, i)
    open_cuts = check_steps(stats)
    res = gr.residuals(A, b, xs)
    worst_rr = residual_mismatch(c, stats, res)
    cosine, counted = gr.optimality(A, b, xs, min(c.restart, gc.STEPS + 1))
    growth = gr.monotone(res)
    own = gc.restated(c)
    print("%s: GPU worst cosine %.3e over %d steps, restatement %.3e over %d, ratio %.2f; largest growth %.12g; residual after %d "
          "steps %.3e (restatement %.3e); relative_residual mismatch %.2e of its margin; cuts before convergence %d"
          % (gc.case_id(i), cosine, counted, own["cosine"], own["counted"], cosine / own["cosine"], growth, gc.STEPS, res[-1],
             own["residuals"][-1], worst_rr, open_cuts))
    assert worst_rr <= 1.0
    assert growth <= 1.0 + gr.MONOTONE_SLACK
    assert counted >= min(own["counted"], gc.CLAIM_STEPS if c.claims else 5)
    assert cosine <= OVER * own["cosine"]


class BlackBox:
    """A, M and b of a case from the library's debug entry points (float64 cycle vectors, as gmres_phase runs the cycle: with
    vcycle_precision="float64" neither vof_debug_vcycle nor gmres_phase stores a float32 vector, see handoff32_ok)."""

    def __init__(self, native, c):
        alpha, beta = gc.REGIMES[c.regime]
        p = native.default_params(speed_alpha=alpha, remodelling_alpha=beta, reference_quirks=int(c.quirks),
                                  coarse_precision={"float64": 0, "float32": 1, "bfloat16": 2, "float8": 3}[c.coarse], vcycle_precision=0)
        self.s = native.Solver(c.shape[0], c.shape[1], 1)
        self.s.debug_setup(gc.movie(c.shape, c.regime), p)
        self.b = self.s.debug_rhs()[0]

    def A(self, x):
        return self.s.debug_apply(0, x[None])[0]

    def M(self, r):
        return self.s.debug_vcycle(r[None])[0]


SPAN_CASES = [i for i, c in enumerate(gc.CASES) if c.restart > gr.SPAN_STEPS and c.quirks]


@pytest.mark.parametrize("i", SPAN_CASES, ids=[CASE_IDS[i] for i in SPAN_CASES])
def test_the_update_lies_in_the_krylov_space_of_the_librarys_own_operators(of, native, i):
    """(2) With A and M taken from the debug entry points: x_1 is parallel to M b, x_k - x_0 lies in M K_k(A M, b) for
    k <= SPAN_STEPS, and the solves to rtol 1e-6 and 1e-10 take the restatement's number of steps."""
    c = gc.CASES[i]
    xs, stats = cut_iterates(of, i)
    box = BlackBox(native, c)
    try:
        _A, b = oracle_system(c)
        assert np.linalg.norm(box.b - b) <= 1e-12 * np.linalg.norm(b)
        image = gr.krylov_image(box.A, box.M, box.b)
        own = gr.restarted_gmres(box.A, box.M, box.b, m=c.restart, rtol=gc.CUT_RTOL, max_steps=gr.SPAN_STEPS)
        counts = {rtol: [gr.restarted_gmres(box.A, box.M, box.b, m=c.restart, rtol=rtol, max_steps=400, reverse_sums=rev)
                         for rev in (False, True)] for rtol in (1e-6, 1e-10)}
    finally:
        box.s.close()
    upto = min(gr.SPAN_STEPS, own.iterations)
    ref = gr.span_defects(image, own.iterates[0], own.iterates[1:upto + 1])
    got = gr.span_defects(image, xs[0], xs[1:upto + 1])
    print("%s: span defects GPU %s\n    restatement %s\n    worst GPU %.3e, restatement %.3e, ratio %.2f"
          % (gc.case_id(i), ["%.1e" % v for v in got], ["%.1e" % v for v in ref], max(got), max(ref), max(got) / max(ref)))
    assert got[0] <= OVER * max(ref[0], np.finfo(np.float64).eps)      # step 1: x_1 parallel to M b (floor: one rounding)
    assert max(got) <= OVER * max(ref)
    for rtol, traces in counts.items():
        if c.coarse == "float64":         # the prototype's M restates these stencils: the same method on a second A and M
            A, M, _b = gc.system(c.shape, c.regime, c.quirks)
            traces = traces + [gr.restarted_gmres(A, M, b, m=c.restart, rtol=rtol, max_steps=400, reverse_sums=rev) for rev in (False, True)]
        res = of.variational_optical_flow(gc.movie(c.shape, c.regime), **gc.solve_kwargs(c, rtol=rtol))["stats"][0]
        steps = [t.iterations for t in traces]
        print("%s: rtol %g: GPU %d steps (converged %d, residual %.3e); restatement on the library's A and M %d, every sum reversed %d%s; "
              "cycles ended early by the estimate %s; estimates around the end %s"
              % (gc.case_id(i), rtol, res["iterations"], res["converged"], res["relative_residual"], steps[0], steps[1],
                 ", on the oracle's A with the prototype's M %d and %d" % tuple(steps[2:]) if len(steps) > 2 else "",
                 [t.false_ends for t in traces], ["%.2e" % v for v in traces[0].estimates[max(steps[0] - 2, 0):steps[0]]]))
        assert all(t.converged for t in traces) and res["converged"]
        if min(steps) == max(steps):
            # the issue's rule: the restatement's count, a difference of one only where its estimate at the deciding step is within
            # 10 % of the tolerance
            allowed = set()
            for t in traces:
                n, est = t.iterations, t.estimates
                allowed.add(n)
                if abs(est[n - 1] / rtol - 1.0) <= 0.1:
                    allowed.add(n + 1)
                if n >= 2 and abs(est[n - 2] / rtol - 1.0) <= 0.1:
                    allowed.add(n - 1)
        else:
            # The restatement does not agree with itself: the same method, with its sums in another order or on the other equally
            # exact A and M, takes another number of steps (34 x 34, W, restart 100 at 1e-10: 49 on the library's operators, 46 on
            # the oracle's; the first cycle ends by its estimate near column 36-40 with the true residual still at 6e-10, and rounding
            # decides how long the second one gets).  No single count is the reference there, so the library's must lie within the
            # restatement's own spread, widened by the one step the rule allows at either end.
            assert rtol < 1e-6                # at the reference's own tolerance the count is well defined in every case
            allowed = set(range(min(steps) - 1, max(steps) + 2))
        assert int(res["iterations"]) in allowed, (int(res["iterations"]), sorted(allowed))


HANDOVER = 4          # 34 x 34, W, restart 17
FORMATS = ("float64", "float8")          # the prototype's stencils and the default ones


@pytest.mark.parametrize("coarse", FORMATS)
@pytest.mark.parametrize("n", [3, 25])
def test_hand_over_from_bicgstab(of, n, coarse):
    """(3) krylov_method=("auto", n) cut at n steps returns the bits of BiCGStab cut at n steps; cut at n + k it returns the k-th GMRES
    iterate from that base, which must pass the checks of (1).  The bar of the cosine: the restatement run from the same base (with the
    prototype's M in either format: the property needs no M, and the figure is rounding of b - A x at residuals of the same size)."""
    c = gc.CASES[HANDOVER]._replace(coarse=coarse)
    mv = gc.movie(c.shape, c.regime)
    A, b = oracle_system(c)
    bicg = of.variational_optical_flow(mv, max_iterations=n, **gc.solve_kwargs(c, krylov_method="bicgstab"))
    auto = of.variational_optical_flow(mv, max_iterations=n, **gc.solve_kwargs(c, krylov_method=("auto", n)))
    assert bicg["stats"]["iterations"][0] == n and not bicg["stats"]["converged"][0]
    for k in FIELDS:
        np.testing.assert_array_equal(auto[k], bicg[k], err_msg=k)
    for k in ("iterations", "converged", "relative_residual"):
        np.testing.assert_array_equal(auto["stats"][k], bicg["stats"][k], err_msg=k)
    xs, stats = [interior(bicg)], []
    for k in range(1, gc.STEPS + 1):
        res = of.variational_optical_flow(mv, max_iterations=n + k, **gc.solve_kwargs(c, krylov_method=("auto", n)))
        xs.append(interior(res))
        stats.append(res["stats"][0].copy())
    check_steps(stats, first=n)
    res = gr.residuals(A, b, xs)
    cosine, counted = gr.optimality(A, b, xs, c.restart)
    _A, M, _b = gc.system(c.shape, c.regime, c.quirks)
    own = gr.restarted_gmres(A, M, b, x0=xs[0], m=c.restart, rtol=gc.CUT_RTOL, max_steps=gc.STEPS)
    own_cosine, own_counted = gr.optimality(A, b, own.iterates, c.restart)
    worst_rr = residual_mismatch(c, stats, res)
    print("hand-over after %d, %s: base residual %.3e, GPU worst cosine %.3e over %d steps, restatement from the same base %.3e over %d, "
          "ratio %.2f; growth %.12g; residual after %d GMRES steps %.3e; relative_residual mismatch %.2e of its margin"
          % (n, coarse, res[0], cosine, counted, own_cosine, own_counted, cosine / own_cosine, gr.monotone(res), gc.STEPS, res[-1], worst_rr))
    assert worst_rr <= 1.0
    assert gr.monotone(res) <= 1.0 + gr.MONOTONE_SLACK
    assert counted >= min(own_counted, gc.CLAIM_STEPS)
    assert cosine <= OVER * own_cosine


def assert_pair_matches_own_solve(batch, pair, own, what):
    """tests/test_gpu_lanes.py's rule for one pair of a batch against its own solve."""
    for k in ("iterations", "converged"):
        assert batch["stats"][k][pair] == own["stats"][k][0], (what, k, batch["stats"][k][pair], own["stats"][k][0])
    bits = True
    for k in FIELDS:
        a, b = np.asarray(own[k][0]), np.asarray(batch[k][pair])
        assert float(np.abs(a - b).max()) <= 1e-9 * max(float(np.abs(a).max()), 1e-300), (what, k)
        bits = bits and np.array_equal(a, b)
    return bits


SWEEP_ALPHAS = (2e3, 1e4, 1e7)          # with the remodelling values: W at (2e3, 1), T at (1e4, 1e2), easy at 1e7
SWEEP_BETAS = (1.0, 1e2, 1e4)


@pytest.mark.parametrize("restart", [9, 100])
def test_pairs_of_one_batch_leave_their_cycle_at_different_steps(of, restart):
    """(4) vary_regularisation under GMRES alone: nine (speed_alpha, remodelling_alpha) combinations of one 8-bit 34 x 34 pair share
    a batch with per-pair parameters and leave the lockstep cycle after a handful of steps to not at all (max_iterations=60).  The
    sweep returns statistics, not fields, so each combination is compared with its own single solve by them: iterations and the
    converged flag equal, mean and variance of speed and remodelling within 1e-9 of the field's max-abs (squared for the variance)."""
    mv = gc.movie((34, 34), "W")
    kw = dict(krylov_method="gmres", preconditioner="multigrid", vcycle_precision="float64", gmres_restart=restart, rtol=1e-10,
              max_iterations=60, warm_start_stride=0, return_stats=True)
    r = of.vary_regularisation(mv, speed_alpha_values=np.array(SWEEP_ALPHAS), remodelling_alpha_values=np.array(SWEEP_BETAS), **kw)
    st = r["stats"]
    print("restart %d: iterations %s converged %s" % (restart, st["max_iterations_used"].tolist(), st["converged_all"].tolist()))
    its = st["max_iterations_used"]
    assert its.min() <= 12 and its.max() > 24 and len(set(its.ravel().tolist())) >= 4         # the premise: a mixed batch
    for a, alpha in enumerate(SWEEP_ALPHAS):
        for b, beta in enumerate(SWEEP_BETAS):
            own = of.variational_optical_flow(mv, speed_alpha=alpha, remodelling_alpha=beta, **kw)
            assert own["stats"]["iterations"][0] == its[a, b], (alpha, beta)
            assert own["stats"]["converged"][0] == st["converged_all"][a, b], (alpha, beta)
            assert st["max_relative_residual"][a, b] == pytest.approx(own["stats"]["relative_residual"][0], rel=1e-6), (alpha, beta)
            for field, mean, var in (("speed", "speed_means", "speed_variances"),
                                     ("remodelling", "remodelling_means", "remodelling_variances")):
                scale = float(np.abs(own[field]).max())
                assert abs(r[mean][a, b] - np.mean(own[field])) <= 1e-9 * scale, (alpha, beta, field)
                assert abs(r[var][a, b] - np.var(own[field])) <= 1e-9 * scale * scale, (alpha, beta, field)


@functools.lru_cache(maxsize=None)
def mixed_stack():
    """Seven 8-bit 34 x 34 frames in the order f0 f0 f1 f2 f2 f3 f4 (tests/test_gpu_active_list.py's stack_with_repeats: pairs 0 and
    3 have a zero right-hand side), the distinct frames at different brightness: the matrix of a pair is built from its first frame,
    so the pairs differ in speed_alpha / I^2 and leave the cycle at different steps."""
    tex = orc.make_texture_stack(34, 5, seed=5)
    frames = np.round(tex * np.array([255.0, 64.0, 255.0, 16.0, 128.0])[:, None, None])
    return np.ascontiguousarray(frames[[0, 0, 1, 2, 2, 3, 4]])


def test_a_batch_with_zero_right_hand_sides_under_gmres_alone(of):
    """(4) A stack whose pairs differ and of which two have b = 0, in one batch: every pair against its own two-frame solve."""
    mv = mixed_stack()
    alpha, beta = gc.REGIMES["T"]
    kw = dict(speed_alpha=alpha, remodelling_alpha=beta, krylov_method="gmres", preconditioner="multigrid", vcycle_precision="float64",
              gmres_restart=9, rtol=1e-10, max_iterations=60, warm_start_stride=0, return_stats=True)
    batch = of.variational_optical_flow(mv, **kw)
    st = batch["stats"]
    print("iterations", st["iterations"].tolist(), "converged", st["converged"].tolist(), "batch_pairs", st["batch_pairs"].tolist())
    assert (st["batch_pairs"] == len(st)).all()                                     # the premise: one batch
    assert st["iterations"][0] == 0 and st["iterations"][3] == 0                    # b = 0: nothing to iterate on
    assert len(set(st["iterations"].tolist())) >= 4
    bits = [assert_pair_matches_own_solve(batch, p, of.variational_optical_flow(mv[p:p + 2], **kw), "pair %d" % p) for p in range(len(st))]
    assert all(bits), bits                # (the rule above allows 1e-9; measured: the same bits, so a batch may not change them)


MEMORY = 6            # 34 x 34, W: GMRES(5) needs far more steps than GMRES(100)


@pytest.mark.parametrize("coarse", FORMATS)
@pytest.mark.parametrize("first,second", [(5, None), (None, 5)], ids=["5-then-default", "default-then-5"])
def test_no_memory_of_an_earlier_restart_length(of, first, second, coarse):
    """(5) The cached context sizes the GMRES basis in the first call that needs it.  A call with another restart length on the
    same context must return what it returns on a fresh one: the basis is re-sized at the start of a call that asks for more than
    it holds (gmres_release_short_basis)."""
    c = gc.CASES[MEMORY]._replace(coarse=coarse)
    mv = gc.movie(c.shape, c.regime)
    kw = gc.solve_kwargs(c, rtol=1e-6, max_iterations=200)
    del kw["gmres_restart"]

    def run(restart):
        return of.variational_optical_flow(mv, gmres_restart=restart, **kw)
    of.release_device_memory()
    fresh = run(second)
    of.release_device_memory()
    before = run(first)
    after = run(second)
    print(coarse, "restart %s then %s: iterations %d then %d (fresh: %d), converged %d (fresh: %d)"
          % (first, second, before["stats"]["iterations"][0], after["stats"]["iterations"][0], fresh["stats"]["iterations"][0],
             after["stats"]["converged"][0], fresh["stats"]["converged"][0]))
    assert before["stats"]["iterations"][0] != fresh["stats"]["iterations"][0]      # the premise: the restart length matters here
    assert after["stats"]["iterations"][0] == fresh["stats"]["iterations"][0]
    assert after["stats"]["converged"][0] == fresh["stats"]["converged"][0]
    for k in FIELDS:
        np.testing.assert_array_equal(after[k], fresh[k], err_msg=k)


def test_lanes_on_a_fresh_context(of, monkeypatch):
    """(6) 66 x 66 x 9 frames, 8-bit, regime T, default formats, on two lanes of a fresh context: both lanes ask for the basis (the
    locked first allocation) and work on views of it at their lane_lo; against one lane by tests/test_gpu_lanes.py's rule.  That two
    lanes ran is read from `batch_pairs`, the size of the batch a pair was solved in: the whole stack with one lane, a share of it
    with two.  Under krylov_method="gmres" every step is a GMRES step, so the iteration counts only show that each share iterated."""
    import torch
    monkeypatch.setenv("VOF_LANES_MIN_MPIX", "0")
    movie = torch.from_numpy(np.round(orc.make_texture_stack(66, 9, seed=5) * 255.0)).to("cuda:0")
    alpha, beta = gc.REGIMES["T"]
    kw = dict(speed_alpha=alpha, remodelling_alpha=beta, krylov_method="gmres", preconditioner="multigrid", rtol=1e-10,
              warm_start_stride=0)
    of.release_device_memory()
    many = lanes.solve(of, movie, 2, **kw)
    one = lanes.solve(of, movie, 1, **kw)
    print("iterations", many[1]["iterations"].tolist(), "residual", many[1]["relative_residual"].tolist())
    assert many[1]["converged"].all() and many[1]["relative_residual"].max() <= 1e-10
    print("batch_pairs one lane", one[1]["batch_pairs"].tolist(), "two lanes", many[1]["batch_pairs"].tolist())
    assert (one[1]["batch_pairs"] == 8).all() and (many[1]["batch_pairs"] < 8).all()
    assert (many[1]["iterations"] > 8).all()
    lanes.assert_same(one, many)


@pytest.mark.parametrize("coarse", FORMATS)
def test_a_tolerance_below_the_attainable_accuracy_ends_by_the_stagnation_rule(of, coarse):
    """(7) rtol=1e-16 on the easy case: the rule of k_gm_init ends the solve unconverged after the restatement's number of steps to
    its own stagnation plus at most two of its cycles, far below max_iterations=1000, and the residual it leaves is within two
    decades of eps |A| |x| / |b|.  The restatement runs the prototype's M (float64 stencils); the default format is held to the
    same bound, which is a bound and claims no equal count."""
    c = gc.CASES[gc.EASY]._replace(coarse=coarse)
    mv = gc.movie(c.shape, c.regime)
    A, M, b = gc.system(c.shape, c.regime, c.quirks)
    own = gr.restarted_gmres(A, M, b, m=c.restart, rtol=1e-16, max_steps=1000)
    assert own.stagnated
    cycle = max(np.diff(own.cycle_starts + [own.iterations]))
    bound = own.iterations + 2 * int(cycle)
    res = of.variational_optical_flow(mv, max_iterations=1000, **gc.solve_kwargs(c, rtol=1e-16))
    st = res["stats"][0]
    level = gc.attainable(c.shape, c.regime, c.quirks)
    true = gr.residuals(A, b, [interior(res)])[0]
    print("rtol 1e-16, %s: GPU %d steps (restatement %d, cycles at %s, bound %d), converged %d, residual %.3e (CPU %.3e), "
          "eps |A| |x| / |b| %.3e, ratio %.2g" % (coarse, st["iterations"], own.iterations, own.cycle_starts, bound, st["converged"],
                                                 st["relative_residual"], true, level, true / level))
    assert not st["converged"]
    assert 0 < st["iterations"] <= bound
    assert true <= 100.0 * level and st["relative_residual"] <= 100.0 * level
