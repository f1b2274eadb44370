"""The level-0 Galerkin product of the batch set-up (k_galerkin) and VOF_GALERKIN_FAST, a bit mask read
when a context is created (every run here has a context of its own): 0 = one generic kernel for every coarse point, 1 (the
default) = a kernel of their own for the points away from the border, 3 = that kernel evaluates the closed form.

Every stored level of every format against oracle/mg_prototype.py, with the tolerances of
test_gpu_kernels.py::test_galerkin_hierarchy_and_transfers, for the default and for the closed form; the closed form against the
generic kernel (float64: 1e-13 on every level); the per-pair alpha / beta table through vary_regularisation against single
solves, for both.

Frame shapes: 12 x 13 and 13 x 12 (both parities, the orphan weights, deeper levels with no interior point at all), 21 x 134
(level 1 is 66 columns wide: a 64-lane block edge lies between interior points), 37 x 20."""
import functools

import numpy as np
import pytest

from oracle import mg_prototype as mg, vof_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(12, 13), (13, 12), (21, 134), (37, 20)]
PARAMS = [(1.0, 1e4), (0.1, 0.1)]
NPAIRS = 2
TOL = {0: 1e-12, 1: 2e-6, 2: 4e-3, 3: 6e-2}


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture
def native():
    from opticalflow_amd import _native
    _native.load_library()
    return _native


@functools.lru_cache(maxsize=None)
def movie_of(shape):
    mv = np.random.default_rng(shape[0] * 1000 + shape[1]).random((NPAIRS + 1,) + shape) * 2.0
    mv.setflags(write=False)
    return mv


@functools.lru_cache(maxsize=None)
def reference(shape, alpha, beta):
    return [mg.Hierarchy(movie_of(shape)[k], alpha, beta) for k in range(NPAIRS)]


def stored_levels(native, monkeypatch, switch, shape, alpha, beta, fmt):
    """The stencils of levels 1 .. of a fresh context (switch: the value of VOF_GALERKIN_FAST, None = unset)."""
    if switch is None:
        monkeypatch.delenv("VOF_GALERKIN_FAST", raising=False)
    else:
        monkeypatch.setenv("VOF_GALERKIN_FAST", str(switch))
    p = native.default_params(speed_alpha=alpha, remodelling_alpha=beta, coarse_precision=fmt)
    with native.Solver(shape[0], shape[1], NPAIRS) as s:
        s.debug_setup(movie_of(shape), p)
        return [s.debug_stencil(lvl) for lvl in range(1, s.num_levels)]


@pytest.mark.parametrize("alpha,beta", PARAMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_every_stored_level_against_the_prototype(native, monkeypatch, shape, alpha, beta):
    H = reference(shape, alpha, beta)
    for fmt, switch in [(f, sw) for f in (0, 1, 2, 3) for sw in (None, 3)]:   # the default, and the closed form
        levels = stored_levels(native, monkeypatch, switch, shape, alpha, beta, fmt)
        assert len(levels) == len(H[0].levels) - 1 >= 1
        for lvl, Cg in enumerate(levels, start=1):
            for k in range(NPAIRS):
                Cr = H[k].levels[lvl]
                assert Cg[k].shape == Cr.shape
                err = relerr(Cg[k], Cr)
                print(shape, (alpha, beta), "switch", switch, "format", fmt, "level", lvl, "pair", k, "relerr", err)
                assert err < TOL[fmt], (fmt, lvl, k)
                if fmt >= 2:
                    # block row sums are the unrounded ones; the off-diagonal blocks are exactly representable in the format
                    rs_g, rs_r = Cg[k].sum(axis=(0, 1)), Cr.sum(axis=(0, 1))
                    assert np.abs(rs_g - rs_r).max() <= 2e-5 * max(1.0, np.abs(Cr).max()), (fmt, lvl, k)
                    off = np.ones((3, 3), bool); off[1, 1] = False
                    q = Cg[k][off]
                    if fmt == 2:
                        assert np.array_equal(q.astype(np.float32).view(np.uint32) & 0xFFFF, np.zeros(q.shape, np.uint32))
                    else:
                        m, _ = np.frexp(q)
                        assert np.array_equal(m * 16, np.round(m * 16))


@pytest.mark.parametrize("alpha,beta", PARAMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_interior_kernels_against_the_generic_kernel(native, monkeypatch, shape, alpha, beta):
    # float64 stencils: the closed form, and the interior kernel without it, against the generic kernel for every point
    off = stored_levels(native, monkeypatch, 0, shape, alpha, beta, 0)
    for switch in (3, 1):
        on = stored_levels(native, monkeypatch, switch, shape, alpha, beta, 0)
        assert len(on) == len(off)
        for lvl, (a, b) in enumerate(zip(on, off), start=1):
            for k in range(NPAIRS):
                err = relerr(a[k], b[k])
                print(shape, (alpha, beta), "switch", switch, "float64 level", lvl, "pair", k, "relerr to the generic kernel", err)
                assert err <= 1e-13, (switch, lvl, k)
    # the default is bit 0 alone; bit 1 without bit 0 is the generic kernel
    for fmt in (0, 3):
        for x, y in zip(stored_levels(native, monkeypatch, None, shape, alpha, beta, fmt), stored_levels(native, monkeypatch, 1, shape, alpha, beta, fmt)):
            assert np.array_equal(x, y)
        for x, y in zip(stored_levels(native, monkeypatch, 2, shape, alpha, beta, fmt), stored_levels(native, monkeypatch, 0, shape, alpha, beta, fmt)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("switch", [None, 3], ids=["default", "closed_form"])
def test_per_pair_parameters_reach_the_interior_kernel(monkeypatch, switch):
    """vary_regularisation hands alpha and beta to the set-up per pair (the table `pp`; the closed form starts its accumulators
    from them): a 2 x 2 grid on a 34 x 35 x 3 stack against the four single solves, to the tolerances of
    test_gpu_consumers.py::test_native_sweep_equals_per_combination_solves."""
    if switch is None:
        monkeypatch.delenv("VOF_GALERKIN_FAST", raising=False)
    else:
        monkeypatch.setenv("VOF_GALERKIN_FAST", str(switch))
    from opticalflow_amd import optical_flow as of
    of.release_device_memory()   # the module keeps a context between calls; this one has to read the switch
    try:
        movie = orc.make_texture_stack(35, 3, seed=23)[:, :34, :]
        sa, ra = np.array([0.5, 2.0]), np.array([20.0, 3000.0])
        kw = dict(delta_x=0.5, delta_t=2.0, rtol=1e-9, initial_v_x=0.1)
        r = of.vary_regularisation(movie, sa, ra, return_stats=True, **kw)
        for i, a in enumerate(sa):
            for j, b in enumerate(ra):
                one = of.variational_optical_flow(movie, speed_alpha=a, remodelling_alpha=b, **kw)
                np.testing.assert_allclose(r["speed_means"][i, j], np.mean(one["speed"]), rtol=1e-12)
                np.testing.assert_allclose(r["speed_variances"][i, j], np.var(one["speed"]), rtol=1e-12)
                np.testing.assert_allclose(r["remodelling_means"][i, j], np.mean(one["remodelling"]), rtol=1e-12, atol=1e-18)
                np.testing.assert_allclose(r["remodelling_variances"][i, j], np.var(one["remodelling"]), rtol=1e-12)
                np.testing.assert_allclose(r["functional"][i, j], one["L1_functional"] + one["speed_functional"]
                                           + one["remodelling_functional"], rtol=1e-12)
                assert r["converged"][i, j] == one["converged"]
        assert r["stats"]["converged_all"].all() and r["stats"]["max_relative_residual"].max() < 1e-8
    finally:
        of.release_device_memory()   # the next caller gets a context of its own environment
