"""One multigrid cycle on the register-resident level-0 pass k_sweep0r, the kernel the product runs, against the numpy prototype of the
same recursion (oracle/mg_prototype.py) and the oracle's operator: at the widths and heights where a strip or a band of the pass
ends (tests/level0_path_cases.py: SHAPES) and under cycle options other than the default (CYCLES).  By default the pass is chosen from
512 one-wave blocks per launch on, which none of these grids reaches: the module runs with VOF_SWEEP0R_MIN_BLOCKS=0, and one test per
shape witnesses that the forced path is the register pass (only k_sweep0r stores the cycle's result as float32)."""
import functools
import os

import numpy as np
import pytest

from level0_path_cases import CYCLES, SHAPES, cycle_movie, takes_register_pass
from oracle import vof_oracle as orc, mg_prototype as mg

pytestmark = pytest.mark.gpu

PAIRS, ALPHA, BETA = 2, 1.0, 1e4


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def f32_exact(a):
    return bool(np.array_equal(np.asarray(a, dtype=np.float32).astype(np.float64), a))


@pytest.fixture(scope="module")
def native():
    from opticalflow_amd import _native, optical_flow
    _native.load_library()
    old = os.environ.get("VOF_SWEEP0R_MIN_BLOCKS")
    os.environ["VOF_SWEEP0R_MIN_BLOCKS"] = "0"
    optical_flow.release_device_memory()      # a cached context was created under the other setting
    yield _native
    optical_flow.release_device_memory()
    if old is None:
        os.environ.pop("VOF_SWEEP0R_MIN_BLOCKS", None)
    else:
        os.environ["VOF_SWEEP0R_MIN_BLOCKS"] = old


@functools.lru_cache(maxsize=None)
def hierarchies(shape):
    mv = cycle_movie(shape, PAIRS)
    return tuple(mg.Hierarchy(mv[k], ALPHA, BETA) for k in range(PAIRS))


_gpu_runs = {}


def gpu_run(native, shape, cyc):
    """r = debug_rhs(), debug_vcycle(r) and debug_vcycle_apply(r) of one case, computed once for the tests that look at them."""
    if (shape, cyc) not in _gpu_runs:
        mv = cycle_movie(shape, PAIRS)
        p = native.default_params(speed_alpha=ALPHA, remodelling_alpha=BETA, coarse_precision=0, vcycle_precision=0, nu_pre=cyc[0], nu_post=cyc[1],
                                  nu_pre_coarse=cyc[2], nu_post_coarse=cyc[3], w_cycle_level=cyc[4], w_cycle_visits=cyc[5])
        assert takes_register_pass(shape, bool(p.reference_quirks), "float64", min_blocks=0)
        H = hierarchies(shape)
        with native.Solver(shape[0], shape[1], PAIRS) as s:
            s.debug_setup(mv, p)
            # (a shape the library treats as single-level would be a mistake in the table, not a reason to skip)
            assert s.num_levels > 1 and s.num_levels == len(H[0].levels)
            for lvl in range(s.num_levels):
                assert s.level_shape(lvl) == tuple(H[0].shapes()[lvl])
            r = s.debug_rhs()
            e = s.debug_vcycle(r)
            y, v, dots, fused = s.debug_vcycle_apply(r)
        _gpu_runs[(shape, cyc)] = dict(r=r, e=e, y=y, v=v, dots=dots, fused=fused)
    return _gpu_runs[(shape, cyc)]


@pytest.mark.parametrize("cyc", CYCLES, ids=["-".join(str(v) for v in c) for c in CYCLES])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_cycle_matches_prototype(native, shape, cyc):
    """debug_vcycle(r) against the same recursion in numpy: smooth, restrict the residual, recurse (the coarse levels with their
    own sweep counts, level w_cycle_level visiting the next one `visits` times), prolong, smooth in reverse.  Float64 storage
    everywhere: the bar of test_vcycle_matches_prototype / test_w_cycle_matches_prototype."""
    g = gpu_run(native, shape, cyc)
    H = hierarchies(shape)
    errs = [relerr(g["e"][k], H[k].cycle(g["r"][k], cyc[:4], w_cycle_level=cyc[4], visits=cyc[5])) for k in range(PAIRS)]
    print(f"cycle {shape} {cyc}: relerr {errs}")
    assert max(errs) < 1e-9, errs


@pytest.mark.parametrize("cyc", CYCLES, ids=["-".join(str(v) for v in c) for c in CYCLES])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_krylov_product_of_the_last_pass_against_the_oracle_operator(native, shape, cyc):
    """debug_vcycle_apply(r): the cycle's last pass also forms v = A y and the dot products (v, r), (v, v) (TRAIL = 1, strips four
    columns narrower).  y is the cycle's result bit for bit, v is the oracle's operator applied to it, the dot products are numpy's."""
    g = gpu_run(native, shape, cyc)
    mv = cycle_movie(shape, PAIRS)
    assert g["fused"] is True
    np.testing.assert_array_equal(g["y"], g["e"])
    for k in range(PAIRS):
        v_ref = orc.apply_operator_interior(mv[k], g["y"][k], ALPHA, BETA)
        r = g["r"][k]
        err = relerr(g["v"][k], v_ref)
        # the reference's own rounding: a second float64 evaluation of the same product on the CPU (level0_path_cases.cycle_movie)
        own = relerr(mg.apply_stencil(hierarchies(shape)[k].levels[0], g["y"][k]), v_ref)
        print(f"product {shape} {cyc} pair {k}: relerr {err} (two CPU evaluations: {own})")
        assert own < 5e-13
        assert err < 1e-12
        assert g["dots"][k, 0] == pytest.approx(float(np.vdot(v_ref, r)), rel=1e-11, abs=1e-9 * np.linalg.norm(v_ref) * np.linalg.norm(r))
        assert g["dots"][k, 1] == pytest.approx(float(np.vdot(v_ref, v_ref)), rel=1e-12)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_forced_path_is_the_register_pass(native, monkeypatch, shape):
    """Default parameters (vcycle_precision 3, two sweeps before and after): only k_sweep0r stores the cycle's result as float32
    (XT = float), so the result is exactly representable in float32 - and is not with VOF_L0_HANDOFF=0."""
    mv = cycle_movie(shape, PAIRS)
    p = native.default_params(speed_alpha=ALPHA, remodelling_alpha=BETA)
    assert (p.vcycle_precision, p.nu_pre, p.nu_post) == (3, 2, 2)
    r = np.random.default_rng(shape[0] * 1000 + shape[1]).standard_normal((PAIRS, 3, shape[0] - 2, shape[1] - 2))
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("VOF_L0_HANDOFF", switch)
        with native.Solver(shape[0], shape[1], PAIRS) as s:
            s.debug_setup(mv, p)
            out[switch] = s.debug_vcycle(r)
    assert np.isfinite(out["1"]).all() and np.abs(out["1"]).max() > 0
    assert f32_exact(out["1"])
    assert not f32_exact(out["0"])
