"""CPU checks of the restatement the direct preconditioner is pinned against (tests/direct_restatement.py) and of the case table
(tests/direct_cases.py): the table hits the edges it claims, the restated elimination is the inverse of the reference system, and
every case marked "one step" really is solved to 1e-12 by one preconditioned Krylov step with either inverse."""
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg

from conftest import ROOT

import direct_cases as dc
import direct_restatement as dr

# N_j -> (m, blocked, ld, nt), written out by hand from  m = 3 (N_j - 2),  blocked iff m > 192,  ld = ceil(m / 64) * 64
EDGES = {5: (9, False, 9, 0), 9: (21, False, 21, 0), 12: (30, False, 30, 0), 40: (114, False, 114, 0),
         66: (192, False, 192, 0),       # the last one-workgroup inverse
         67: (195, True, 256, 4),        # the first blocked size: 61 of 256 columns are padding
         70: (204, True, 256, 4), 99: (291, True, 320, 5),
         130: (384, True, 384, 6),       # exactly 6 tiles
         131: (387, True, 448, 7), 195: (579, True, 640, 10),
         259: (771, True, 832, 13)}
# (N_i, N_j[, quirks]) the table must keep
REQUIRED = [(12, 66), (12, 67), (67, 12), (131, 9), (9, 130), (9, 131), (6, 259), (30, 99), (5, 5)]


def test_the_restated_constants_are_those_of_the_source():
    csrc = os.path.join(ROOT, "opticalflow_amd", "csrc")
    with open(os.path.join(csrc, "vof.hip")) as f:
        hip = f.read()
    with open(os.path.join(csrc, "vof_direct.hpp")) as f:
        hpp = f.read()
    assert int(re.search(r"constexpr int DIRECT_OWN_MAX = (\d+);", hip).group(1)) == dr.OWN_MAX
    assert int(re.search(r"constexpr int DNB = (\d+)", hpp).group(1)) == dr.TILE
    assert "return 3 * c->L[0].nj > DIRECT_OWN_MAX;" in hip
    assert "direct_uses_blocked(c) ? ((m + DNB - 1) / DNB) * DNB : m;" in hip


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.case_id)
def test_every_case_takes_the_path_it_claims(i):
    c = dc.CASES[i]
    m, blocked, ld, nt = EDGES[c.n_j]
    assert dr.path_rule(c.n_j) == dict(m=m, blocked=blocked, ld=ld, nt=nt)
    assert m == 3 * (c.n_j - 2) and blocked == (m > 192) and ld % 64 == (0 if blocked else m % 64) and ld - m < 64
    assert max(c.n_i, c.n_j) <= 260 and c.T >= 2
    assert dc.movie(i).shape == (c.T, c.n_i, c.n_j)
    if c.scale == 255.0:
        assert np.array_equal(dc.movie(i), np.round(dc.movie(i))) and dc.movie(i).max() > 128     # integers on the 8-bit scale


def test_the_table_keeps_its_edges():
    shapes = {(c.n_i, c.n_j) for c in dc.CASES}
    assert not [s for s in REQUIRED if s not in shapes]
    assert any((c.n_i, c.n_j, c.quirks) == (14, 195, False) for c in dc.CASES)
    one_step = [dc.CASES[i] for i in dc.ONE_STEP]
    # both inverse kernels, padded and unpadded tiles, both aspect ratios and the quirk switch among the cases that must take one step
    assert {dr.path_rule(c.n_j)["blocked"] for c in one_step} == {True, False}
    assert {dr.path_rule(c.n_j)["ld"] == dr.path_rule(c.n_j)["m"] for c in one_step if dr.path_rule(c.n_j)["blocked"]} == {True, False}
    assert {c.n_i > c.n_j for c in one_step} == {True, False} and {c.quirks for c in one_step} == {True, False}
    assert {(c.alpha, c.beta, c.scale) for c in one_step} >= {dc.T_, dc.W_, dc.N_} and any(c.alpha == 0.1 for c in one_step)
    assert max(dr.path_rule(c.n_j)["nt"] for c in one_step) == 13
    assert [c.kind for c in dc.CASES].count("ill-conditioned") == 1
    batch = dc.CASES[dc.BATCH_CASE]
    assert batch.T == 4 and batch.kind == "one step" and dr.path_rule(batch.n_j)["blocked"]
    mv = dc.movie(dc.BATCH_CASE)
    assert not any(np.array_equal(mv[a], mv[b]) for a in range(4) for b in range(a))     # three pairs whose data differ


def test_tile_inverse_is_an_inverse_at_padded_and_exact_sizes():
    rng = np.random.default_rng(0)
    for m in (1, 63, 64, 65, 128, 195):
        S = rng.standard_normal((m, m)) + 4.0 * np.sqrt(m) * np.eye(m)
        np.testing.assert_allclose(dr.tile_inverse(S) @ S, np.eye(m), rtol=0, atol=1e-13)


@pytest.mark.parametrize("i", range(len(dc.CASES)), ids=dc.case_id)
def test_the_restated_elimination_solves_the_reference_system(i):
    """M^-1 r against SuperLU on the same matrix, for the right-hand side of the pair and a random one, with both inverses.  The bar
    is the suite's own for "the same solution of the reference system" (TIGHT = 1e-7 of tests/test_gpu_parity.py): a slip in the
    elimination (a block taken from the wrong row, a field out of order) costs O(1)."""
    c, mv = dc.CASES[i], dc.movie(i)
    A, b = dr.system(mv[0], mv[1], c.alpha, c.beta, c.quirks)
    lu_ref = scipy.sparse.linalg.splu(A.tocsc())
    rhs = (b, np.random.default_rng(i).standard_normal(b.size))
    for inverse in ("lapack", "tile"):
        lu = dr.RowBlockLU(A, c.n_i - 2, c.n_j - 2, inverse)
        for r in rhs:
            z, ref = lu.solve(r), lu_ref.solve(r)
            err = np.linalg.norm(z - ref) / np.linalg.norm(ref)
            print(dc.case_id(i), inverse, "relative difference to SuperLU %.2e" % err)
            assert err <= 1e-7, (inverse, err)


@pytest.mark.parametrize("i", dc.ONE_STEP, ids=dc.case_id)
def test_admission_one_step_reaches_1e_minus_12_with_both_inverses(i):
    """The admission condition of a "one step" case: the TRUE residual after one Krylov step is <= 1e-12 with the LAPACK inverse and
    with the tile inverse, for every pair of the case.  A case that misses it is replaced or demoted in the table; the bar stays."""
    for inverse in ("lapack", "tile"):
        for k, (x, steps, rr) in enumerate(dc.restated(i, inverse)):
            print(dc.case_id(i), "pair", k, inverse, "steps", steps, "true residual %.2e" % rr)
            assert np.isfinite(x).all()     # (steps is 1 whatever the step reached: max_it = 1)
            assert rr <= dc.ADMISSION, (inverse, k, rr)


@pytest.mark.parametrize("i", [i for i in range(len(dc.CASES)) if i not in dc.ONE_STEP], ids=dc.case_id)
def test_the_other_cases_are_yardsticks_worth_having(i):
    """"residual only" cases: what one step of the restatement leaves is the yardstick of the GPU test, so it has to meet the tight rule
    (1e-10) at least.  The "ill-conditioned" case must really be one: some inverse of the restatement is left above 1e-12, at the level
    rounding allows - within two decades (growth in an elimination of a few thousand unknowns) of eps ||A|| ||x|| / ||b||."""
    c = dc.CASES[i]
    rr = {inverse: [r[2] for r in dc.restated(i, inverse)] for inverse in ("lapack", "tile")}
    print(dc.case_id(i), rr)
    if c.kind == "ill-conditioned":
        print("eps ||A|| ||x|| / ||b||:", dc.attainable(i))
        assert max(max(v) for v in rr.values()) > 10 * dc.ADMISSION, rr
        for v in rr.values():
            assert all(r <= 100.0 * a for r, a in zip(v, dc.attainable(i))), (rr, dc.attainable(i))
    else:
        assert max(max(v) for v in rr.values()) <= 1e-10, rr
