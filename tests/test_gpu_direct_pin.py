"""The direct preconditioner (csrc/vof_direct.hpp; direct_setup / direct_apply_t / direct_solve_list of csrc/vof.hip) pinned through
the public API at its shape edges (tests/direct_cases.py) against a float64 restatement (tests/direct_restatement.py).

The Krylov iteration around the preconditioner repairs whatever is a little wrong in it at the price of extra steps, and the other
tests allow up to 4.  Here the iteration is cut to ONE step: after one BiCGStab half-step with the preconditioner M from the zero
guess the true relative residual is ||(I - A M^-1) b|| / ||b||, so `max_iterations=1` turns the library's own independent
`relative_residual` into a measurement of how exact M^-1 is.  (The multigrid cycle needs at least 3 steps to reach 1e-10, so
`iterations == 1` with `converged` also proves that the direct path ran.)"""
import functools

import numpy as np
import pytest

from oracle import vof_oracle as orc

import direct_cases as dc
import direct_restatement as dr

pytestmark = pytest.mark.gpu

TIGHT = 1e-7          # rel-L2 bar per field against the exact solution of the reference system (tests/test_gpu_parity.py)
# Bounds of the GPU's one-step residual (test (b)); measured ratios per case: profiles/direct_pin_summary.md.
#  * Cases that run the direct preconditioner: one decade over the restatement with the tile inverse.  Library and tile restatement
#    are the same elimination in the same tile order and differ in the summation order inside the products and the tile inverses
#    only; the restatement itself moves by up to 1.25 x between two BLAS builds, the library sits at 0.7 ... 2.1 times it.  (The 17 x
#    between LAPACK and the tile inverse is a difference of method, not of rounding, and does not enter.)
#  * The single-level 5 x 5 image, which the dense coarse inverse solves and not the direct preconditioner: two decades.  The
#    restatement's 2e-14 there is a few ulp of its 27 unknowns; the library's 1.5e-13 (6.4 x) is the level of every other case.
#  * The ill-conditioned case: two decades over the level rounding allows, eps ||A|| ||x|| / ||b|| (3.5e-12).  The two inverses of the
#    restatement are a factor 6 apart there, on other stacks 400 in either direction; the allowance is the one
#    tests/test_direct_restatement_cpu.py makes for the restatement itself.
OVER_TILE = 10.0
OVER_TILE_SINGLE_LEVEL = 100.0
OVER_ATTAINABLE = 100.0
FIELDS = ("v_x", "v_y", "remodelling", "speed")


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def of():
    from opticalflow_amd import optical_flow
    return optical_flow


_runs = {}


def one_step_run(of, i, max_pairs_in_flight=None):
    """Case i through the public entry with the direct preconditioner and the iteration cut to one step; run once per module."""
    key = (i, max_pairs_in_flight)
    if key not in _runs:
        c = dc.CASES[i]
        _runs[key] = of.variational_optical_flow(dc.movie(i), speed_alpha=c.alpha, remodelling_alpha=c.beta, reference_quirks=c.quirks,
                                                 preconditioner="direct", rtol=1e-10, max_iterations=1, return_stats=True,
                                                 max_pairs_in_flight=max_pairs_in_flight)
    return _runs[key]


@functools.lru_cache(maxsize=None)
def exact(i):
    c = dc.CASES[i]
    return orc.variational_optical_flow(dc.movie(i), speed_alpha=c.alpha, remodelling_alpha=c.beta, reference_quirks=c.quirks)


@pytest.mark.parametrize("i", dc.ONE_STEP, ids=dc.case_id)
def test_one_krylov_step_solves_the_admitted_cases(of, i):
    """(a) Where one step of the restated preconditioner reaches 1e-12 with either inverse, one step of the library reaches the tight
    rule: converged, exactly one iteration, residual <= 1e-10, and the fields are the exact solution of the reference system."""
    res = one_step_run(of, i)
    st = res["stats"]
    print(dc.case_id(i), "iterations", st["iterations"].tolist(), "relative_residual", st["relative_residual"].tolist())
    assert st["converged"].all(), st
    assert (st["iterations"] == 1).all(), st
    assert st["relative_residual"].max() <= 1e-10, st
    ref = exact(i)
    for k in ("v_x", "v_y", "remodelling"):
        e = relerr(res[k], ref[k])
        assert e < TIGHT, (k, e)


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.case_id)
def test_one_step_residual_against_the_restatement(of, i):
    """(b) Every case, the ill-conditioned and "residual only" ones included: the library's independent residual after one step
    within a decade of the true one-step residual of the restatement with the tile inverse (the design's own accuracy); the two
    exceptions and the reasons for every bound stand beside OVER_TILE."""
    c = dc.CASES[i]
    st = one_step_run(of, i)["stats"]
    assert (st["iterations"] == 1).all(), st
    single_level = max(c.n_i, c.n_j) - 2 <= 5       # COARSEST_MAX of oracle/mg_prototype.py: no hierarchy, no direct preconditioner
    for k, (_x, _steps, rr) in enumerate(dc.restated(i, "tile")):
        got = float(st["relative_residual"][k])
        print(dc.case_id(i), "pair", k, "GPU %.3e restatement (tile) %.3e (LAPACK %.3e) ratio %.2f"
              % (got, rr, dc.restated(i, "lapack")[k][2], got / rr))
        if c.kind == "ill-conditioned":
            level = dc.attainable(i)[k]
            print(dc.case_id(i), "pair", k, "eps ||A|| ||x|| / ||b|| %.3e ratio %.2f" % (level, got / level))
            bound = OVER_ATTAINABLE * level
        else:
            bound = (OVER_TILE_SINGLE_LEVEL if single_level else OVER_TILE) * rr
        assert np.isfinite(got) and got <= bound, (k, got, rr, bound)


def test_the_ill_conditioned_case_by_the_full_solve(of):
    """The reference's switch on the ill-conditioned case: converged within the step count
    test_hard_regimes_are_rescued_by_the_direct_preconditioner allows."""
    (i,) = [i for i, c in enumerate(dc.CASES) if c.kind == "ill-conditioned"]
    c = dc.CASES[i]
    res = of.variational_optical_flow(dc.movie(i), speed_alpha=c.alpha, remodelling_alpha=c.beta, use_direct_solver=True,
                                      return_stats=True)
    st = res["stats"]
    print(dc.case_id(i), "iterations", st["iterations"].tolist(), "relative_residual", st["relative_residual"].tolist())
    assert st["converged"].all() and st["iterations"].max() <= 4, st


def test_batches_of_the_blocked_path_give_the_same_bits(of):
    """(c) Three pairs whose data differ, as one batch of three, three batches of one, and a batch of two and one: the same bits in
    every returned field, and each pair equal to its own two-frame solve - a pair reading its neighbour's inverse (sT), stencil table
    (sTab) or vectors (sV) cannot pass."""
    i = dc.BATCH_CASE
    c, mv = dc.CASES[i], dc.movie(i)
    runs = {mp: one_step_run(of, i, mp) for mp in (None, 1, 2)}
    for mp, r in runs.items():
        assert r["stats"]["converged"].all() and (r["stats"]["iterations"] == 1).all(), (mp, r["stats"])
    # the premise: one batch of three, three batches of one, a batch of two and a batch of one
    assert [runs[mp]["stats"]["batch_pairs"].tolist() for mp in (None, 1, 2)] == [[3, 3, 3], [1, 1, 1], [2, 2, 1]]
    for mp in (1, 2):
        for k in FIELDS:
            np.testing.assert_array_equal(runs[mp][k], runs[None][k], err_msg=f"max_pairs_in_flight={mp}: {k}")
    for pair in range(c.T - 1):
        own = of.variational_optical_flow(mv[pair:pair + 2], speed_alpha=c.alpha, remodelling_alpha=c.beta, reference_quirks=c.quirks,
                                          preconditioner="direct", rtol=1e-10, max_iterations=1, return_stats=True)
        for k in FIELDS:
            np.testing.assert_array_equal(runs[None][k][pair], own[k][0], err_msg=f"pair {pair}: {k}")
        assert own["stats"]["relative_residual"][0] == runs[None]["stats"]["relative_residual"][pair]
    # the three pairs are three different problems (a batch that solved pair 0 three times would not be noticed otherwise)
    assert relerr(runs[None]["v_x"][1], runs[None]["v_x"][0]) > 1e-3 and relerr(runs[None]["v_x"][2], runs[None]["v_x"][1]) > 1e-3


SUMMARY_TABLES = ("speed_means", "speed_variances", "remodelling_means", "remodelling_variances", "functional")


@functools.lru_cache(maxsize=None)
def sweep_inputs():
    """An 8-bit (3, 14, 70) stack (m = 204: blocked, ld 256) whose first frame is bright and whose other two are dim (1/16 of the
    8-bit range), and the 4 x 3 grid of logspace(-1, 4) values, the speed_alpha values in the order 215, 4.64, 0.1, 1e4.  The system
    matrix of a pair is built from its first frame, so pair 0 (bright: speed_alpha / I^2 256 times smaller) is the harder one for the
    multigrid cycle at every combination.  Within 80 Krylov steps the cycle solves both pairs at speed_alpha 1e4, loses pair 0 alone at
    215 and 4.64 and both pairs at 0.1, whatever remodelling_alpha: in this order the first combination leaves one pair to the direct
    re-solve and the seventh leaves two."""
    tex = orc.make_texture_stack(70, 3, seed=9)[:, :14, :70]
    movie = np.round(tex * np.array([255.0, 16.0, 16.0])[:, None, None]).astype(np.uint8)
    return movie, np.logspace(-1, 4, 4)[[2, 1, 0, 3]], np.logspace(-1, 4, 3)


SWEEP_KW = dict(smoothing_sigma=1, delta_x=0.4, delta_t=10.0)


def test_parameter_table_on_the_blocked_path(of):
    """(d) vary_regularisation with use_direct_solver=True at m = 204: per-pair alpha, beta and frame index from the PairParam table
    on the blocked kernels (the existing sweep test runs at 56 x 56, i.e. on the one-workgroup inverse)."""
    movie, sa, ra = sweep_inputs()
    assert dr.path_rule(movie.shape[2])["blocked"]
    r = of.vary_regularisation(movie, speed_alpha_values=sa, remodelling_alpha_values=ra, use_direct_solver=True, return_stats=True,
                               **SWEEP_KW)
    print("max_relative_residual", r["stats"]["max_relative_residual"].tolist(), "iterations", r["stats"]["max_iterations_used"].tolist())
    assert r["stats"]["converged_all"].all(), r["stats"]["max_relative_residual"]
    ref = orc.vary_regularisation(movie, sa, ra, **SWEEP_KW)
    for k in SUMMARY_TABLES:
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-6, atol=1e-12, err_msg=k)


def test_direct_resolve_with_buffers_sized_by_a_shorter_first_list(of):
    """(d) The automatic re-solve when the direct buffers were sized by a first, shorter list (dir_cap of direct_solve_list is kept
    for the life of the context): the same grid with the default preconditioner and max_iterations=80, one combination per batch
    (max_pairs_in_flight = the two pairs of the stack).  The first combination must leave exactly one pair to the re-solve - the
    buffers are then allocated for one pair - and a later one both, which are then solved in two batches of one.  That the multigrid
    attempt does leave these pairs is checked here with the same attempt on its own.  The context is released first, so the probes
    create one for batches of two; the sweep re-uses it, and its dir_cap is still 0 then, because preconditioner="multigrid"
    allocates no direct buffers."""
    movie, sa, ra = sweep_inputs()
    kw = dict(max_iterations=80, max_pairs_in_flight=movie.shape[0] - 1, return_stats=True, **SWEEP_KW)
    of.release_device_memory()
    left = np.zeros((len(sa), len(ra)), dtype=int)
    for a in range(len(sa)):
        for b in range(len(ra)):
            st = of.variational_optical_flow(movie, speed_alpha=sa[a], remodelling_alpha=ra[b], preconditioner="multigrid", **kw)["stats"]
            left[a, b] = int((st["converged"] == 0).sum())
    print("pairs the multigrid attempt leaves unconverged, per combination:", left.tolist())
    # all the sticky path needs (measured: 1 at speed_alpha 215 and 4.64, 2 at 0.1, 0 at 1e4, for every remodelling_alpha)
    assert left[0, 0] == 1 and (left.ravel()[1:] == 2).any(), left
    r = of.vary_regularisation(movie, speed_alpha_values=sa, remodelling_alpha_values=ra, **kw)
    assert r["stats"]["converged_all"].all(), r["stats"]["max_relative_residual"]
    ref = orc.vary_regularisation(movie, sa, ra, **SWEEP_KW)
    np.testing.assert_allclose(r["speed_means"], ref["speed_means"], rtol=2e-3)


def test_vcycle_precision_is_ignored_under_the_direct_preconditioner(of):
    """(e) The float32 storage modes of the cycle vectors are switched off while the direct preconditioner is on (solve_batch), so
    every vcycle_precision returns the bits of "float64", on a blocked case."""
    i = 1
    c = dc.CASES[i]
    assert dr.path_rule(c.n_j)["blocked"]
    kw = dict(speed_alpha=c.alpha, remodelling_alpha=c.beta, reference_quirks=c.quirks, preconditioner="direct", rtol=1e-10,
              return_stats=True)
    ref = of.variational_optical_flow(dc.movie(i), vcycle_precision="float64", **kw)
    assert ref["stats"]["converged"].all()
    for mode in ("float32", "auto", "coarse_float32"):
        res = of.variational_optical_flow(dc.movie(i), vcycle_precision=mode, **kw)
        for k in FIELDS:
            np.testing.assert_array_equal(res[k], ref[k], err_msg=f"{mode}: {k}")
        np.testing.assert_array_equal(res["stats"]["iterations"], ref["stats"]["iterations"])
        np.testing.assert_array_equal(res["stats"]["relative_residual"], ref["stats"]["relative_residual"])
