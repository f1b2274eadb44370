"""vcycle_precision 3: the level-0 hand-off vectors of the cycle - the pre-smoothed iterate and the cycle's result y / z - are
stored as float32 by the register-resident passes (k_sweep0r, XT = float) during the first 8 BiCGStab iterations
(VOF_L0_HANDOFF=0: float64).  The arithmetic stays FP64, so the switch changes the cycle by float32 rounding only, and the
Krylov iteration not at all beyond that."""
import numpy as np
import pytest

from oracle import vof_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture
def native(monkeypatch):
    from opticalflow_amd import _native
    _native.load_library()
    # the small grids of this file run the register-resident pass too (by default it starts at 512 one-wave blocks per launch)
    monkeypatch.setenv("VOF_SWEEP0R_MIN_BLOCKS", "0")
    return _native


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def f32_exact(a):
    return bool(np.array_equal(np.asarray(a, dtype=np.float32).astype(np.float64), a))


def texture(n, pairs, seed, scale=1.0):
    return np.ascontiguousarray(orc.make_texture_stack(n, pairs + 1, seed=seed) * scale)


def cycle(native, monkeypatch, mv, p, r, switch):
    monkeypatch.setenv("VOF_L0_HANDOFF", switch)
    with native.Solver(mv.shape[1], mv.shape[2], mv.shape[0] - 1) as s:
        s.debug_setup(mv, p)
        y = s.debug_vcycle(r)
        ya, v, _, fused = s.debug_vcycle_apply(r)
        v_ref = s.debug_apply(0, ya)
    return y, ya, v, v_ref, fused


def solve(native, monkeypatch, mv, p, switch):
    monkeypatch.setenv("VOF_L0_HANDOFF", switch)
    with native.Solver(mv.shape[1], mv.shape[2], mv.shape[0] - 1) as s:
        return s.solve_host(mv, p)


@pytest.mark.parametrize("shape", [(130, 258), (258, 130)])
def test_cycle_result_in_float32(native, monkeypatch, shape):
    mv = np.ascontiguousarray(texture(max(shape), 2, 7)[:, :shape[0], :shape[1]])
    p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4)
    with native.Solver(shape[0], shape[1], 2) as s:
        s.debug_setup(mv, p)
        r = np.random.default_rng(7).standard_normal((2, 3) + s.level_shape(0))
    on = cycle(native, monkeypatch, mv, p, r, "1")
    off = cycle(native, monkeypatch, mv, p, r, "0")
    assert f32_exact(on[0]) and not f32_exact(off[0])
    np.testing.assert_array_equal(on[1], on[0])             # the fused Krylov product does not change the cycle
    assert on[4] and off[4]
    assert relerr(on[2], on[3]) < 1e-12                     # v = A y of the rounded y
    assert relerr(on[0], off[0]) < 2e-6                     # float32 rounding of the iterate and of the result


# (the fields are compared where the iteration converges in a few steps; T and W are ill-conditioned at this size)
REGIMES = [("bench", 1.0, 1.0, 1e4, dict(coarse_precision=3)),   # bench.py's workload (float8 stencils below level 0)
           ("N", 1.0, 1.0, 1e4, {}), ("8-bit", 255.0, 1e5, 1e3, {}), ("T", 255.0, 1e4, 1e2, {}), ("W", 255.0, 2e3, 1.0, {})]
FAST = ("bench", "N", "8-bit")


@pytest.mark.parametrize("name,scale,alpha,beta,extra", REGIMES, ids=[r[0] for r in REGIMES])
def test_solves_agree_with_and_without_float32_handoff(native, monkeypatch, name, scale, alpha, beta, extra):
    mv = texture(258, 3, 5, scale)
    p = native.default_params(speed_alpha=alpha, remodelling_alpha=beta, **extra)
    on = solve(native, monkeypatch, mv, p, "1")
    off = solve(native, monkeypatch, mv, p, "0")
    st_on, st_off = on[4], off[4]
    np.testing.assert_array_equal(st_on["converged"], st_off["converged"])
    assert abs(st_on["iterations"].mean() - st_off["iterations"].mean()) <= 0.5, (st_on["iterations"], st_off["iterations"])
    for st in (st_on, st_off):
        ok = st["converged"] != 0
        assert (st["relative_residual"][ok] <= p.rtol).all()
    if name in FAST:
        for a, b in zip(on[:3], off[:3]):
            assert np.max(np.abs(a - b)) <= 1e-4 * np.max(np.abs(b))


def test_stragglers_switch_to_float64(native, monkeypatch):
    """More than 8 iterations: the hand-off vectors go back to float64 with the levels below (regime T at 130^2: ~40)."""
    mv = texture(130, 2, 5, 255.0)
    p = native.default_params(speed_alpha=1e4, remodelling_alpha=1e2, preconditioner=0)
    on = solve(native, monkeypatch, mv, p, "1")
    off = solve(native, monkeypatch, mv, p, "0")
    assert (off[4]["iterations"] > 8).all()
    assert on[4]["converged"].all() and off[4]["converged"].all()
    # (in this slowly converging regime the count reacts to any rounding in the first iterations: 44 / 38 against 45 / 43 measured)
    it_on, it_off = int(on[4]["iterations"].sum()), int(off[4]["iterations"].sum())
    assert abs(it_on - it_off) <= 0.15 * it_off, (on[4]["iterations"], off[4]["iterations"])
    assert (on[4]["relative_residual"] <= p.rtol).all()


@pytest.mark.parametrize("shape,quirks", [((130, 131), 1), ((130, 258), 0)])
def test_other_passes_keep_float64(native, monkeypatch, shape, quirks):
    """Odd row length (k_sweep0) and reference_quirks=False (k_sweep0m): float64 hand-off, the switch changes nothing."""
    mv = np.ascontiguousarray(texture(max(shape), 2, 3)[:, :shape[0], :shape[1]])
    p = native.default_params(speed_alpha=1.0, remodelling_alpha=1e4, reference_quirks=quirks)
    on = solve(native, monkeypatch, mv, p, "1")
    off = solve(native, monkeypatch, mv, p, "0")
    for a, b in zip(on[:4], off[:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(on[4]["iterations"], off[4]["iterations"])
    with native.Solver(shape[0], shape[1], 2) as s:
        s.debug_setup(mv, p)
        r = np.random.default_rng(3).standard_normal((2, 3) + s.level_shape(0))
    monkeypatch.setenv("VOF_L0_HANDOFF", "1")
    with native.Solver(shape[0], shape[1], 2) as s:
        s.debug_setup(mv, p)
        y = s.debug_vcycle(r)
    assert not f32_exact(y)
