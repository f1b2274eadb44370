"""The GMRES restatement (tests/gmres_restatement.py) on the cases of tests/gmres_cases.py, without a GPU: its own figures - the bars
of tests/test_gpu_gmres_pin.py are multiples of them -, the admission of the cases that claim coverage of the chunk edges, and what the
checks see of three deliberately broken variants of the method."""
import numpy as np
import pytest

import gmres_cases as gc
import gmres_restatement as gr

CASE_IDS = [gc.case_id(i) for i in range(len(gc.CASES))]
CLAIMING = [i for i, c in enumerate(gc.CASES) if c.claims]


@pytest.mark.parametrize("i", range(len(gc.CASES)), ids=CASE_IDS)
def test_the_restatement_has_the_properties_it_checks(i):
    """Every case: STEPS iterates, a residual that never grows, and a worst cosine far below anything a wrong method gives (the
    visible variants below start at 0.1).  The figures are printed: they are the reference values of the GPU test."""
    c = gc.CASES[i]
    r = gc.restated(c)
    above = sum(1 for v in r["residuals"][1:] if v >= gr.RESIDUAL_FLOOR)
    print(gc.case_id(i), "worst cosine %.2e over %d steps, steps above the floor %d, largest growth %.3g, residual after %d steps %.2e"
          % (r["cosine"], r["counted"], above, r["growth"], gc.STEPS, r["residuals"][-1]))
    t = r["trace"]
    assert t.converged if t.iterations < gc.STEPS else t.iterations == gc.STEPS       # (the easier cases reach CUT_RTOL)
    assert not t.stagnated
    assert r["counted"] == above and above >= 5
    assert r["growth"] <= 1.0 + gr.MONOTONE_SLACK
    assert r["cosine"] < 1e-3
    # the estimate |g[k]| is the true residual while rounding allows: it is what `iterations` and `converged` go by
    for k in range(1, t.iterations + 1):
        if r["residuals"][k] >= gr.RESIDUAL_FLOOR:
            assert t.estimates[k - 1] == pytest.approx(r["residuals"][k], rel=1e-3)
    # full cycles while the residual is above the floor, as `optimality` assumes
    m = min(c.restart, gc.STEPS + 1)
    assert [s for s in t.cycle_starts if s < above] == list(range(0, above, m))


@pytest.mark.parametrize("i", CLAIMING, ids=[CASE_IDS[i] for i in CLAIMING])
def test_admission_of_the_chunk_edge_cases(i):
    """A case counts as coverage of columns 9, 16 and 17 only if its cuts get there above the floor and its cycle is long enough."""
    c = gc.CASES[i]
    r = gc.restated(c)
    assert c.restart >= 17
    assert sum(1 for v in r["residuals"][1:] if v >= gr.RESIDUAL_FLOOR) >= gc.CLAIM_STEPS
    assert all(v >= gr.RESIDUAL_FLOOR for v in r["residuals"][1:gc.CLAIM_STEPS + 1])


def test_the_cases_cover_what_they_are_for():
    shapes = {c.shape for c in gc.CASES}
    assert {(18, 18), (34, 34)} <= shapes and any(s[0] != s[1] for s in shapes)
    assert {c.restart for c in gc.CASES} == {100, 5, 9, 17, 128}
    assert {c.regime for c in gc.CASES} == {"N", "T", "W"} and gc.CASES[gc.EASY].regime == "N"
    assert any(not c.quirks for c in gc.CASES) and {c.coarse for c in gc.CASES} == {"float64", "float8"}
    assert gc.STEPS >= 2 * 9 + 1 and gc.STEPS > 17            # two restarts of 5 and of 9, and column 17
    for c in gc.CASES:
        assert max(c.shape) <= 70 and gc.movie(c.shape, c.regime).shape == (2,) + c.shape
        if c.regime != "N":
            mv = gc.movie(c.shape, c.regime)
            assert np.array_equal(mv, np.round(mv)) and mv.min() >= 0 and mv.max() <= 255


@pytest.mark.parametrize("i", [i for i in CLAIMING if gc.CASES[i].coarse == "float64" and gc.CASES[i].quirks],
                         ids=lambda i: CASE_IDS[i])
def test_what_the_checks_see_of_the_broken_variants(i):
    """Dropping the coefficient of basis vector 8 and flipping the sign of one rotation both show in the cosine at more than 100
    times the clean value (the bar of the GPU test), and both make the residual grow.  Leaving the second pass's coefficients out
    of h is harmless in exact arithmetic: neither check sees it, and it is not claimed as covered."""
    c = gc.CASES[i]
    clean = gc.restated(c)
    for variant in ("drop_v8", "flip_rotation"):
        bad = gc.restated(c, variant)
        print(gc.case_id(i), variant, "cosine %.2e (clean %.2e), growth %.3g" % (bad["cosine"], clean["cosine"], bad["growth"]))
        assert bad["cosine"] > 100.0 * clean["cosine"]
        assert bad["growth"] > 1.0 + gr.MONOTONE_SLACK
    unseen = gc.restated(c, "no_second_h")
    print(gc.case_id(i), "no_second_h", "cosine %.2e (clean %.2e), growth %.3g" % (unseen["cosine"], clean["cosine"], unseen["growth"]))
    assert unseen["cosine"] < 100.0 * clean["cosine"] and unseen["growth"] <= 1.0 + gr.MONOTONE_SLACK


@pytest.mark.parametrize("shape,regime,quirks", gc.SYSTEMS, ids=["%dx%d-%s%s" % (s[0], s[1], r, "" if q else "-noquirks")
                                                                  for s, r, q in gc.SYSTEMS])
def test_span_of_the_restatement(shape, regime, quirks):
    """Every system of the case table: x_k - x_0 of the restatement lies in M K_k(A M, r_0) for k <= SPAN_STEPS, the basis built
    independently by Arnoldi.  The defects are printed: the bar of the GPU test is a multiple of the same figure on the library's A and M."""
    d = gc.restated_span(shape, regime, quirks)
    print(shape, regime, quirks, "span defects", ["%.1e" % v for v in d], "eps |A| |x| / |b| %.2e" % gc.attainable(shape, regime, quirks))
    assert 1 <= len(d) <= gr.SPAN_STEPS and max(d) < 1e-7


def test_stagnation_rule_ends_a_solve_below_the_attainable_accuracy():
    """rtol below what rounding allows: the restatement's solve ends by the rule of k_gm_init, neither converged nor at the limit."""
    c = gc.CASES[gc.EASY]
    A, M, b = gc.system(c.shape, c.regime, c.quirks)
    t = gr.restarted_gmres(A, M, b, m=c.restart, rtol=1e-16, max_steps=1000)
    print(gc.case_id(gc.EASY), "stagnated after", t.iterations, "steps, cycles at", t.cycle_starts)
    assert t.stagnated and not t.converged and t.iterations < 100
