"""CPU tests of the Liu-Shen Jacobi flow (liu_shen_optical_flow_jit): the numpy restatement against every fixture the
reference wrote, the check that the fixtures exercise the reference's edge rules, and the boundary of the new entry points
(header, library, binding, Python names, no CPU fallback).

Agreement metric: e = max|x - ref| / max(|ref v_x|, |ref v_y|) over both fields; bound 1e-13 (the restatement inverts the
2 x 2 block in closed form where the reference calls numpy.linalg.inv: 0.8-2.2e-15 measured, the margin covers another
BLAS build)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from liushen_restatement import liu_shen, error  # noqa: E402

BOUND = 1e-13
CASES = ["a", "b", "c", "d", "e"]


def arguments(g):
    """The positional arguments of the reference call a fixture records."""
    def field(a):
        return float(a) if a.ndim == 0 else a
    return (g["movie"], float(g["delta_x"]), float(g["delta_t"]), float(g["alpha"]), 1.0, field(g["initial_v_x"]),
            field(g["initial_v_y"]), field(g["initial_remodelling"]), int(g["max_iterations"]))


def test_fixtures_cover_what_they_should():
    g = {c: load_golden(f"g12{c}_liushen.npz") for c in CASES}
    assert g["a"]["movie"].shape[1:] == (40, 56) and g["b"]["movie"].shape[1:] == (56, 40)
    assert g["a"]["movie"].dtype == np.float64 and g["c"]["movie"].dtype == np.uint8
    assert float(g["a"]["delta_x"]) != 1.0 and float(g["a"]["delta_t"]) != 1.0
    assert float(g["c"]["alpha"]) == 1e4 and float(g["d"]["alpha"]) == 1.0 and g["d"]["movie"].max() > 100
    assert g["d"]["initial_v_x"].shape == g["d"]["movie"].shape[1:]
    assert 100 <= int(g["b"]["max_iterations"]) <= 200
    assert g["e"]["movie"].shape[0] == 2 and g["e"]["v_x_steps"].shape[:2] == (1, int(g["e"]["max_iterations"]) // int(g["e"]["iteration_stepsize"]) + 1)
    for c in CASES:
        for k in g[c]:
            assert np.isfinite(g[c][k]).all(), (c, k)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(case):
    g = load_golden(f"g12{case}_liushen.npz")
    v_x, v_y, speed, remodelling, last = liu_shen(*arguments(g))
    e = error(v_x, v_y, g["v_x"], g["v_y"])
    es = error(speed, speed, g["speed"], g["speed"]) * float(np.abs(g["speed"]).max()) / max(np.abs(g["v_x"]).max(), np.abs(g["v_y"]).max())
    print(f"{case}: e = {e:.3g}, speed {es:.3g}")
    assert e <= BOUND and es <= BOUND
    assert np.array_equal(remodelling, np.broadcast_to(g["initial_remodelling"], g["v_x"].shape))
    assert np.array_equal(remodelling, g["remodelling"])
    assert last == int(g["max_iterations"]) - 1 == int(g["last_iteration"])


def test_restatement_reproduces_the_step_record():
    g = load_golden("g12e_liushen.npz")
    movie, dx, dt, alpha = g["movie"], float(g["delta_x"]), float(g["delta_t"]), float(g["alpha"])
    step = int(g["iteration_stepsize"])
    this = (float(g["initial_v_x"]), float(g["initial_v_y"]), float(g["initial_remodelling"]))
    assert np.all(g["v_x_steps"][:, 0] == this[0]) and np.all(g["remodelling_steps"] == this[2])
    for r in range(1, g["v_x_steps"].shape[1]):
        res = liu_shen(movie, dx, dt, alpha, 1.0, *this, step)
        e = error(res[0], res[1], g["v_x_steps"][:, r], g["v_y_steps"][:, r])
        print(f"record {r}: e = {e:.3g}")
        assert e <= BOUND
        this = (res[0], res[1], res[3])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mutation", ["mirror_bar", "n_eight"])
def test_fixtures_exercise_the_edge_rules(case, mutation):
    """The restatement with one of the reference's edge rules switched off must miss the bound by at least 1e3."""
    g = load_golden(f"g12{case}_liushen.npz")
    v_x, v_y = liu_shen(*arguments(g), **{mutation: True})[:2]
    e = error(v_x, v_y, g["v_x"], g["v_y"])
    print(f"{case} {mutation}: e = {e:.3g}")
    assert e >= 1e3 * BOUND


def test_restatement_argument_checks():
    movie = np.random.default_rng(0).random((2, 8, 8))
    with pytest.raises(ValueError):
        liu_shen(movie, max_iterations=0)
    with pytest.raises(ValueError):
        liu_shen(movie[:, :2], max_iterations=1)


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)
    for name in ("vof_liu_shen_dev", "vof_liu_shen_host"):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert proto, name
        assert hasattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert len(args) == 15 == len(proto.group(1).split(","))
    assert lib.vof_version() == 202
    assert hasattr(_native.Solver, "liu_shen_host") and hasattr(_native.Solver, "liu_shen_dev")
    assert "VOF_LIUSHEN_FUSE" in open(os.path.join(ROOT, "include", "vof.h")).read()
    assert "vof_liushen.hpp" in build.default_deps(build.CSRC, build.SOURCES[0])


def test_python_names_and_signatures():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    for name in ("liu_shen_optical_flow_jit", "conduct_variational_optical_flow_deprecated"):
        assert getattr(shim, name) is getattr(of, name) and name in of.__all__
    empty = inspect.Parameter.empty
    p = inspect.signature(of.liu_shen_optical_flow_jit).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert positional == [("movie", empty), ("delta_x", 1.0), ("delta_t", 1.0), ("alpha", 100), ("remodelling_alpha", 1.0),
                          ("initial_v_x", 0.0), ("initial_v_y", 0.0), ("initial_remodelling", 0.0), ("max_iterations", 10),
                          ("tolerance", 1e-9), ("include_remodelling", True)]
    assert [n for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == ["device", "output"]
    p = inspect.signature(of.conduct_variational_optical_flow_deprecated).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert positional == [("movie", empty), ("delta_x", 1.0), ("delta_t", 1.0), ("speed_alpha", 1.0), ("remodelling_alpha", 1000.0),
                          ("v_x_guess", 0.1), ("v_y_guess", 0.1), ("remodelling_guess", 0.5), ("max_iterations", 10),
                          ("smoothing_sigma", None), ("return_iterations", False), ("iteration_stepsize", 1),
                          ("tolerance", 1e-10), ("include_remodelling", True), ("use_liu_shen", False)]
    assert [n for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == ["device", "output"]


def test_argument_errors_need_no_gpu():
    from opticalflow_amd import optical_flow as of
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(ValueError, match="max_iterations"):
        of.liu_shen_optical_flow_jit(movie, max_iterations=0)
    with pytest.raises(ValueError, match="sides"):
        of.liu_shen_optical_flow_jit(movie[:, :2, :], max_iterations=3)
    with pytest.raises(ValueError, match="sides"):
        of.liu_shen_optical_flow_jit(movie[:, :, :2], max_iterations=3)
    with pytest.raises(ValueError, match="liu shen"):
        of.conduct_variational_optical_flow_deprecated(movie)
    with pytest.raises(ValueError, match="iteration_stepsize"):
        of.conduct_variational_optical_flow_deprecated(movie, use_liu_shen=True, return_iterations=True, max_iterations=4,
                                                       iteration_stepsize=5)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(_native.VofError):
        optical_flow.liu_shen_optical_flow_jit(movie)
    with pytest.raises(_native.VofError):
        optical_flow.conduct_variational_optical_flow_deprecated(movie, use_liu_shen=True)
