"""CPU tests of the box least-squares flow (conduct_optical_flow): the numpy restatement against every fixture the reference
wrote, and the boundary of the new entry points (header, library, binding, Python names, no CPU fallback)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from boxflow_restatement import box_flow, kappa_max  # noqa: E402

EPS = 2.2e-16
CASES = ["a", "b", "c", "d", "e"]


def runs_of(case):
    """(label, analysed movie, box, delta_x, delta_t, remodelling, {field: reference}) of every reference run of a fixture."""
    g = load_golden(f"g11{case}_boxflow.npz")
    box, dx, dt = int(g["box"]), float(g["delta_x"]), float(g["delta_t"])
    out = []
    for prefix, movie in ((("s_", g["s_blurred_data"]), ("b_", g["b_blurred_data"])) if case == "f" else (("", g["movie"]),)):
        out.append((f"{case}{prefix}plain", movie, box, dx, dt, False,
                    {k: g[prefix + k] for k in ("v_x", "v_y", "speed")}))
        out.append((f"{case}{prefix}remodelling", movie, box, dx, dt, True,
                    {"v_x": g[prefix + "r_v_x"], "v_y": g[prefix + "r_v_y"], "net_remodelling": g[prefix + "r_net_remodelling"],
                     "speed": np.zeros_like(g[prefix + "r_v_x"])}))
    return out


def assert_matches(got, ref, kappa, units, label):
    """Non-finite values exactly where the reference has them; elsewhere |got - ref| <= units * eps * kappa_max * max|field|."""
    km = kappa_max(kappa, *ref.values())
    worst = 0.0
    for k, r in ref.items():
        g = np.asarray(got[k])
        assert np.array_equal(np.isfinite(g), np.isfinite(r)), (label, k, "non-finite values at other positions")
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, k)
        fin = np.isfinite(r)
        if not fin.any() or not np.abs(r[fin]).max() > 0:
            assert not np.abs(g[fin]).any() if fin.any() else True, (label, k)
            continue
        unit = EPS * km * np.abs(r[fin]).max()
        err = float(np.abs(g[fin] - r[fin]).max()) / unit
        worst = max(worst, err)
        print(f"{label} {k}: kappa_max {km:.3g}, error {err:.3g} units")
        assert err <= units, (label, k, err)
    return worst


@pytest.mark.parametrize("case", CASES + ["f"])
def test_restatement_matches_the_reference(case):
    for label, movie, box, dx, dt, rem, ref in runs_of(case):
        r = box_flow(movie, box, dx, dt, include_remodelling=rem)
        assert_matches(r, ref, r["kappa"], 64, label)
        assert kappa_max(r["kappa"], *ref.values()) <= 1e5


def test_restatement_is_exact_on_integer_data():
    for label, movie, box, dx, dt, rem, ref in runs_of("d"):
        r = box_flow(movie, box, dx, dt, include_remodelling=rem)
        for k in ("v_x", "v_y", "net_remodelling"):
            if k in ref:
                assert np.array_equal(r[k], ref[k]), (label, k)


def test_quirk_free_restatement_differs_only_where_the_quirks_act():
    g = load_golden("g11a_boxflow.npz")
    q = box_flow(g["movie"], 15, include_remodelling=False)
    f = box_flow(g["movie"], 15, include_remodelling=False, reference_quirks=False)
    h, n_i = 7, g["movie"].shape[1]
    assert np.isfinite(f["v_x"]).all() and np.isnan(q["v_x"][:, :, n_i + h:]).all()
    assert np.array_equal(q["v_x"][:, :, :n_i - h], f["v_x"][:, :, :n_i - h])
    fr = box_flow(g["movie"], 15, include_remodelling=True, reference_quirks=False)
    assert fr["speed"].any()


def test_symbols_are_declared_exported_and_prototyped():
    from opticalflow_amd import build, _native
    build.build_native(verbose=False)
    lib = _native.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vof.h")).read(), flags=re.S)
    for name in ("vof_box_flow_dev", "vof_box_flow_host"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name)
        res, args = _native.SIGNATURES[name]
        assert len(args) == 12
    assert lib.vof_version() == 202
    assert hasattr(_native.Solver, "box_flow_host") and hasattr(_native.Solver, "box_flow_dev")


def test_python_names_and_signatures():
    sys.path.insert(0, os.path.join(ROOT, "source"))
    import optical_flow as shim
    from opticalflow_amd import optical_flow as of
    assert shim.conduct_optical_flow is of.conduct_optical_flow and shim.conduct_optical_flow_jit is of.conduct_optical_flow_jit
    assert "conduct_optical_flow" in of.__all__ and "conduct_optical_flow_jit" in of.__all__
    p = inspect.signature(of.conduct_optical_flow).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert positional == [("movie", inspect.Parameter.empty), ("boxsize", 15), ("delta_x", 1.0), ("delta_t", 1.0),
                          ("smoothing_sigma", None), ("background", None), ("include_remodelling", False)]
    assert [n for n, v in p.items() if v.kind is v.KEYWORD_ONLY] == ["reference_quirks", "device", "output"]
    assert p["reference_quirks"].default is True
    p = inspect.signature(of.conduct_optical_flow_jit).parameters
    positional = [(n, v.default) for n, v in p.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert positional == [("movie", inspect.Parameter.empty), ("box_size", 15), ("delta_x", 1.0), ("delta_t", 1.0),
                          ("include_remodelling", False)]


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from opticalflow_amd import optical_flow, _native
    movie = np.random.default_rng(0).random((3, 16, 16))
    with pytest.raises(_native.VofError):
        optical_flow.conduct_optical_flow(movie)
    with pytest.raises(_native.VofError):
        optical_flow.conduct_optical_flow_jit(movie)
