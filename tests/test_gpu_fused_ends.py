"""GPU tests of the fused ends of a batch (k_stream_apply0, MODE 2 and 3): VOF_FUSED_ENDS on against off in one process.

The switch is read when a context is created, so every comparison creates fresh contexts (``ends``).  Values: 0 = the
stand-alone kernels (k_rhs_norm, k_gather_guess / k_fill, the residual pass, k_finalize_functionals), 1 = fused prologue only,
2 = fused epilogue only, 3 = both ends fused (the default).

Bars.  The pointwise vectors (b, x0, r0, r^, the four outputs) are the same expressions in the fused and the stand-alone
kernels; the block partial sums are partitioned differently, so the Krylov scalars differ in their last bits.  For whole
solves the project's bar holds (profiles/r06_lane_groups_summary.md): iterations and converged flags identical, relative
residual <= 1e-6 (the default rtol) on both sides, fields within 2e-8 of the field's max-abs.  The functionals are sums of
squares of the fields and their differences: twice the fields' relative bar, 4e-8.  With the same solution going into it
(1 against 3: the prologue is the same, only the epilogue differs) the epilogue's outputs are bit-identical and its
functionals and residual norm agree to summation order, 1e-12.

The two-phase warm start (saved guesses, guess source -1) needs 16 Mpixel of phase-1 pairs (solve_range_dev), whatever the
image size: those two tests use 1434 pairs of 130 x 258, the smallest stack of the strip-and-band shape that is above it.
Below that threshold a stack is solved cold, so the small cases reach the prologue through non-zero constant initial fields."""
import contextlib
import os

import numpy as np
import pytest

from oracle import vof_oracle as orc

pytestmark = pytest.mark.gpu

FIELDS = ("v_x", "v_y", "remodelling", "speed")
FUNCTIONALS = ("L1_functional", "speed_functional", "remodelling_functional")
GUESS = dict(initial_v_x=0.3, initial_v_y=-0.2, initial_remodelling=0.01)


@pytest.fixture(scope="module")
def of():
    from opticalflow_amd import optical_flow
    return optical_flow


@contextlib.contextmanager
def ends(of, value):
    """VOF_FUSED_ENDS=value for the contexts created inside (the cached context is dropped on both sides)."""
    old = os.environ.get("VOF_FUSED_ENDS")
    os.environ["VOF_FUSED_ENDS"] = str(value)
    of.release_device_memory()
    try:
        yield
    finally:
        of.release_device_memory()
        if old is None:
            del os.environ["VOF_FUSED_ENDS"]
        else:
            os.environ["VOF_FUSED_ENDS"] = old


def movie_of(shape, eight_bit=False):
    T, ni, nj = shape
    m = np.ascontiguousarray(orc.make_texture_stack(max(ni, nj), T, seed=11)[:, :ni, :nj])
    return np.round(m * 255.0) if eight_bit else m


def solve(of, value, movie, **kw):
    with ends(of, value):
        return of.variational_optical_flow(movie, return_stats=True, **kw)


def assert_whole_solve_agrees(a, b, field_tol=2e-8, relres=1e-6):
    sa, sb = a["stats"], b["stats"]
    print("iterations", sa["iterations"], sb["iterations"], "relres", sa["relative_residual"].max(), sb["relative_residual"].max())
    np.testing.assert_array_equal(sa["iterations"], sb["iterations"])
    np.testing.assert_array_equal(sa["converged"], sb["converged"])
    if relres is not None:
        assert sa["converged"].all() and sa["relative_residual"].max() <= relres and sb["relative_residual"].max() <= relres
    for k in FIELDS:
        d = np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()
        print(k, "max difference / max-abs", d)
        assert d <= field_tol, k
    for k in FUNCTIONALS:
        print(k, sa[k], sb[k])
        np.testing.assert_allclose(sa[k], sb[k], rtol=2 * field_tol, err_msg=k)


@pytest.mark.parametrize("shape", [(4, 66, 70), (4, 130, 258)])
@pytest.mark.parametrize("guess", [{}, GUESS], ids=["zero", "constants"])
def test_strip_and_band_edges(of, shape, guess):
    """Interior 64 x 68 (one strip) and 128 x 256 (two strips, several bands; the width is no multiple of a strip), two
    batches (2 + 1 pairs).  From zero only the epilogue is fused; with constant initial fields the prologue is too."""
    movie = movie_of(shape)
    kw = dict(warm_start_stride=3, max_pairs_in_flight=2, **guess)
    off, pro, epi, on = (solve(of, v, movie, **kw) for v in (0, 1, 2, 3))
    assert_whole_solve_agrees(on, off)
    assert_whole_solve_agrees(pro, off)
    assert_whole_solve_agrees(epi, off)
    # the same solution into either epilogue (2 against 0, 3 against 1): same bits out
    for k in FIELDS:
        np.testing.assert_array_equal(epi[k], off[k], err_msg=k)
        np.testing.assert_array_equal(on[k], pro[k], err_msg=k)
    np.testing.assert_array_equal(on["stats"]["iterations"], pro["stats"]["iterations"])
    np.testing.assert_allclose(on["stats"]["relative_residual"], pro["stats"]["relative_residual"], rtol=1e-12)
    for k in FUNCTIONALS:
        np.testing.assert_allclose(on["stats"][k], pro["stats"][k], rtol=1e-12, err_msg=k)


@pytest.fixture(scope="module")
def two_phase_stack():
    """1434 pairs of 130 x 258 on the device: 478 phase-1 pairs x 33540 pixels = 16.03 Mpixel, the two-phase warm start is on."""
    import torch
    from opticalflow_amd.synthetic import texture_stack_torch
    T = 1435
    dev = torch.device("cuda", 0)
    movie = texture_stack_torch(258, T, 4, dev)[:, :130, :].contiguous()
    torch.cuda.synchronize()
    return movie


def solve_two_phase(of, value, movie, **kw):
    import torch
    from opticalflow_amd import _native
    T = movie.shape[0]
    p = _native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, warm_start_stride=3, **kw)
    f = [torch.empty_like(movie[:-1]) for _ in range(4)]
    torch.cuda.synchronize()
    with ends(of, value), _native.Solver(130, 258, T - 1) as s:
        st = s.solve_dev(movie, T, p, *f)
    res = {k: t.cpu().numpy() for k, t in zip(("v_x", "v_y", "remodelling", "speed"), f)}
    res["stats"] = st
    return res


def test_saved_guess(of, two_phase_stack):
    """Phase 2 of the warm start: x0 is gathered from the saved solutions inside the prologue."""
    on, off = (solve_two_phase(of, v, two_phase_stack) for v in (3, 0))
    assert_whole_solve_agrees(on, off)
    warm = np.arange(on["stats"].size) % 3 != 0
    assert on["stats"]["iterations"][warm].mean() < on["stats"]["iterations"][~warm].mean()   # the guesses were used


def test_guess_source_minus_one(of, two_phase_stack):
    """One iteration leaves every phase-1 pair unconverged, so every phase-2 pair takes the constant fields inside the
    prologue (non-zero, so that they show).  Nothing converges: the residuals are compared instead of held to rtol."""
    kw = dict(max_iterations=1, preconditioner=0, initial_v_x=0.3, initial_v_y=-0.2, initial_remodelling=0.01)
    on, off = (solve_two_phase(of, v, two_phase_stack, **kw) for v in (3, 0))
    assert not on["stats"]["converged"].any()
    assert_whole_solve_agrees(on, off, relres=None)
    np.testing.assert_allclose(on["stats"]["relative_residual"], off["stats"]["relative_residual"], rtol=1e-6)


@pytest.mark.parametrize("guess", [{}, dict(initial_v_x=0.1)], ids=["zero", "constants"])
def test_pair_param_table(of, guess):
    """vary_regularisation: pp[pair].frame is not the pair index, the alphas and the output slot come from the table."""
    movie = movie_of((3, 34, 38), eight_bit=True)
    sa, ra = np.array([0.5, 2.0]), np.array([20.0, 3000.0])
    res = []
    for v in (3, 0):
        with ends(of, v):
            res.append(of.vary_regularisation(movie, sa, ra, return_stats=True, **guess))
    on, off = res
    np.testing.assert_array_equal(on["converged"], off["converged"])
    assert on["stats"]["converged_all"].all() and max(on["stats"]["max_relative_residual"].max(), off["stats"]["max_relative_residual"].max()) <= 1e-6
    for k in ("speed_means", "remodelling_means"):
        print(k, np.abs(on[k] - off[k]).max())
        np.testing.assert_allclose(on[k], off[k], rtol=2e-8, atol=2e-8 * np.abs(off[k]).max(), err_msg=k)
    for k in ("speed_variances", "remodelling_variances", "functional"):
        print(k, np.abs(on[k] / off[k] - 1).max())
        np.testing.assert_allclose(on[k], off[k], rtol=4e-8, err_msg=k)


def test_restart_regime(of):
    """The hard regime of test_native_sweep_resolves_hard_regime_in_both_branches (8-bit data, speed_alpha 1e4, rtol 1e-9):
    BiCGStab's recursive residual drifts from the true one, and pairs are restarted, handed to GMRES or re-solved with the
    direct preconditioner after the fused epilogue has run once: outputs and functionals must be those of the last solution.
    3 against 1 (the solve starts from zero, so 1 runs the stand-alone kernels throughout): the same Krylov trajectory, so the
    same iterations and the same bits in every field - a field left over from the first epilogue would differ.
    On against off, as the issue allows where a restart cannot be forced; bar as reasoned in that test: both results meet rtol
    1e-9, such results are within 1e-5 of the exact fields in this regime, so two of them differ by at most 2e-5 (functionals:
    twice that)."""
    movie = np.round(orc.make_texture_stack(66, 4, seed=5) * 255.0)
    kw = dict(speed_alpha=1e4, remodelling_alpha=1e2, rtol=1e-9, max_iterations=60)
    on, sep, off = (solve(of, v, movie, **kw) for v in (3, 1, 0))
    print("iterations", on["stats"]["iterations"], sep["stats"]["iterations"], off["stats"]["iterations"])
    np.testing.assert_array_equal(on["stats"]["iterations"], sep["stats"]["iterations"])
    np.testing.assert_array_equal(on["stats"]["converged"], sep["stats"]["converged"])
    for k in FIELDS:
        np.testing.assert_array_equal(on[k], sep[k], err_msg=k)
    for k in FUNCTIONALS:
        np.testing.assert_allclose(on["stats"][k], sep["stats"][k], rtol=1e-12, err_msg=k)
    assert on["stats"]["converged"].all() and off["stats"]["converged"].all()
    assert max(on["stats"]["relative_residual"].max(), off["stats"]["relative_residual"].max()) <= 1e-9
    for k in FIELDS:
        d = np.abs(on[k] - off[k]).max() / np.abs(off[k]).max()
        print(k, d)
        assert d <= 2e-5, k
    for k in FUNCTIONALS:
        np.testing.assert_allclose(on["stats"][k], off["stats"][k], rtol=4e-5, err_msg=k)


@pytest.mark.parametrize("krylov", ["gmres", ("auto", 1)], ids=["gmres", "auto-1"])
def test_gmres_takes_every_pair_after_the_epilogue(of, krylov):
    """krylov_method "gmres" / ("auto", 1): BiCGStab runs no / one iteration, the fused epilogue runs on x0 / a one-step x, and
    GMRES then takes every pair: outputs and functionals must be rewritten from GMRES's solution.  Were they not, the fields
    would be those of x0 (the constants) and miss every bar below grossly."""
    movie = movie_of((4, 66, 70))
    kw = dict(krylov_method=krylov, max_pairs_in_flight=3, **GUESS)
    off, sep, on = (solve(of, v, movie, **kw) for v in (0, 1, 3))
    assert on["stats"]["iterations"].min() >= 2          # GMRES did run
    assert np.abs(on["v_x"] - GUESS["initial_v_x"]).max() > 1e-3
    assert_whole_solve_agrees(on, off)
    np.testing.assert_array_equal(on["stats"]["iterations"], sep["stats"]["iterations"])
    for k in FIELDS:
        np.testing.assert_array_equal(on[k], sep[k], err_msg=k)
    for k in FUNCTIONALS:
        np.testing.assert_allclose(on["stats"][k], sep["stats"][k], rtol=1e-12, err_msg=k)


def test_the_fused_kernels_run(of):
    """The profiler's tables show which kernels ran: the fused launches carry their `moved` bytes under "rhs" (prologue: 16 B of
    frames in, 96 B of b, x0, r0, r^ out per pixel with constant initial fields) and "finalize" (epilogue: 64 B in, 32 B out), the
    stand-alone k_rhs_norm and k_finalize_functionals record none; the apply0 class loses the residual pass that each fused end
    replaces.  One batch of 3 pairs."""
    from opticalflow_amd import _native
    movie = movie_of((4, 66, 70))
    npts = 64 * 68
    p = _native.default_params(**GUESS)
    napply = {}
    for value in (0, 1, 2, 3):
        with ends(of, value), _native.Solver(66, 70, 3) as s:
            s.profile_enable(True)
            res = s.solve_host(movie, p)
            got = {k: s.profile_moved(k, 0) for k in ("rhs", "finalize")}
            napply[value] = s.profile_get("apply0", 0)[0]
        print(value, got, napply[value], res[4]["iterations"])
        assert res[4]["converged"].all()
        assert got["rhs"] == (112.0 * npts * 3 if value & 1 else 0.0)
        assert got["finalize"] == (96.0 * npts * 3 if value & 2 else 0.0)
    assert napply[0] - napply[1] == 1 and napply[0] - napply[2] == 1 and napply[0] - napply[3] == 2, napply


def test_without_reference_quirks(of):
    """reference_quirks=False: other level-0 smoother kernels and the true y-derivatives, the same two ends."""
    movie = movie_of((4, 66, 70))
    kw = dict(reference_quirks=False, max_pairs_in_flight=2, **GUESS)
    assert_whole_solve_agrees(solve(of, 3, movie, **kw), solve(of, 0, movie, **kw))
