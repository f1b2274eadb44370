"""GPU tests of the box least-squares flow (conduct_optical_flow / vof_box_flow_*): the fused LDS kernel and the general
three-kernel path against the reference's fixtures and the numpy restatement.

Bound (set from the reference's own error, not from what the GPU gives): non-finite values at exactly the reference's
positions and, on the finite pixels, |gpu - ref| <= 64 * eps * kappa_max * max|field| per field, kappa_max = the largest
conditioning number of the closed form over the finite pixels (tests/boxflow_restatement.py).  Every comparison prints its
error in these units before it asserts."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from boxflow_restatement import box_flow  # noqa: E402
from test_boxflow_cpu import assert_matches, runs_of  # noqa: E402

pytestmark = pytest.mark.gpu
UNITS = 64


@pytest.fixture(params=["fused", "general"])
def path(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("VOF_BOXFLOW_FUSED", "0")
    else:
        monkeypatch.delenv("VOF_BOXFLOW_FUSED", raising=False)
    return request.param


def gpu_fields(movie, box, dx, dt, rem, entry, quirks=True):
    from opticalflow_amd import optical_flow as of
    if entry == "host":
        v_x, v_y, speed, g = of.conduct_optical_flow_jit(movie, box, dx, dt, rem, reference_quirks=quirks)
        return {"v_x": v_x, "v_y": v_y, "speed": speed, "net_remodelling": g}
    res = of.conduct_optical_flow(movie, box, dx, dt, include_remodelling=rem, reference_quirks=quirks, output="torch")
    out = {k: res[k].cpu().numpy() for k in ("v_x", "v_y", "speed")}
    out["net_remodelling"] = res["net_remodelling"].cpu().numpy() if rem else np.zeros_like(out["v_x"])
    return out


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_fixture_cases(case, entry, path):
    """Every run the reference wrote (case f: the flow of the reference's own analysed movie; the wrapper steps that
    produce that movie are checked in test_wrapper_steps)."""
    for label, movie, box, dx, dt, rem, ref in runs_of(case):
        kappa = box_flow(movie, box, dx, dt, include_remodelling=rem)["kappa"]
        got = gpu_fields(movie, box, dx, dt, rem, entry)
        assert_matches(got, ref, kappa, UNITS, f"{label} {path} {entry}")
        if not rem:
            assert not got["net_remodelling"].any()


def test_integer_data_is_bit_identical(path):
    """Case d: every window sum of 8-bit data is exact in any order, so only the closed form is left."""
    for label, movie, box, dx, dt, rem, ref in runs_of("d"):
        got = gpu_fields(movie, box, dx, dt, rem, "host")
        for k in ("v_x", "v_y", "net_remodelling"):
            if k in ref:
                diff = np.abs(got[k] - ref[k]).max()
                print(f"{label} {path} {k}: max difference {diff}")
                assert np.array_equal(got[k], ref[k]), (label, k, diff)
        if not rem:
            ulp = np.spacing(np.abs(ref["speed"]))
            worst = float((np.abs(got["speed"] - ref["speed"]) / ulp).max())
            print(f"{label} {path} speed: {worst} ulp")
            assert worst <= 1.0


def texture(n_i, n_j, frames=2, seed=5):
    from oracle import vof_oracle as orc
    n = max(n_i, n_j)
    return np.ascontiguousarray(orc.make_texture_stack(n, frames, seed=seed)[:, :n_i, :n_j])


@pytest.mark.parametrize("shape,boxes", [((130, 258), (3, 15, 31, 41)), ((258, 130), (15, 40)), ((1024, 1024), (31, 41))])
@pytest.mark.parametrize("rem", [False, True])
def test_sizes_no_fixture_has(shape, boxes, rem, path):
    movie = texture(*shape)
    for box in boxes:
        r = box_flow(movie, box, 0.5, 2.0, include_remodelling=rem)
        got = gpu_fields(movie, box, 0.5, 2.0, rem, "dev")
        assert_matches(got, {k: r[k] for k in ("v_x", "v_y", "speed", "net_remodelling")}, r["kappa"], UNITS,
                       f"{shape} box {box} rem {rem} {path}")


@pytest.mark.parametrize("n_i", [31, 32, 33])
@pytest.mark.parametrize("n_j", [63, 64, 65])
def test_tile_edges(n_i, n_j, path):
    movie = texture(n_i, n_j, seed=n_i + n_j)
    for rem in (False, True):
        for box in (5, 31):
            r = box_flow(movie, box, include_remodelling=rem)
            got = gpu_fields(movie, box, 1.0, 1.0, rem, "host")
            assert_matches(got, {k: r[k] for k in ("v_x", "v_y", "speed", "net_remodelling")}, r["kappa"], UNITS,
                           f"{n_i}x{n_j} box {box} rem {rem} {path}")


@pytest.mark.parametrize("quirks", [True, False])
def test_box_larger_than_the_image_and_quirk_free(quirks, path):
    for shape, box in (((16, 20), 51), ((24, 40), 9), ((40, 24), 6), ((24, 40), 100)):
        movie = texture(*shape, seed=3)
        for rem in (False, True):
            r = box_flow(movie, box, 0.25, 0.5, include_remodelling=rem, reference_quirks=quirks)
            got = gpu_fields(movie, box, 0.25, 0.5, rem, "host", quirks=quirks)
            assert_matches(got, {k: r[k] for k in ("v_x", "v_y", "speed", "net_remodelling")}, r["kappa"], UNITS,
                           f"{shape} box {box} rem {rem} quirks {quirks} {path}")
            if not quirks and rem:
                assert got["speed"].any()


def test_wrapper_steps():
    """Case f: blur and background subtraction as the reference's wrapper does them, the dict, object identity."""
    from opticalflow_amd import optical_flow as of
    g = load_golden("g11f_boxflow.npz")
    movie = g["movie"]
    for prefix, kw in (("s_", dict(smoothing_sigma=float(g["smoothing_sigma"]))), ("b_", dict(background=float(g["background"])))):
        for rem in (False, True):
            res = of.conduct_optical_flow(movie, int(g["box"]), float(g["delta_x"]), float(g["delta_t"]), include_remodelling=rem, **kw)
            keys = ["blurred_data", "delta_t", "delta_x", "original_data", "speed", "v_x", "v_y"] + (["net_remodelling"] if rem else [])
            assert sorted(res) == sorted(keys)
            assert res["original_data"] is movie
            np.testing.assert_allclose(res["blurred_data"], g[prefix + "blurred_data"], rtol=0, atol=1e-12)
            if prefix == "b_":
                assert np.array_equal(res["blurred_data"] == 0.0, g["b_blurred_data"] == 0.0)
            jit = of.conduct_optical_flow_jit(res["blurred_data"], int(g["box"]), float(g["delta_x"]), float(g["delta_t"]), rem)
            for k, f in zip(("v_x", "v_y", "speed"), jit):
                assert np.array_equal(res[k], f, equal_nan=True), (prefix, rem, k)
            if rem:
                assert np.array_equal(res["net_remodelling"], jit[3]) and not res["speed"].any()
    plain = of.conduct_optical_flow(movie)
    assert plain["blurred_data"] is movie and plain["original_data"] is movie and plain["delta_x"] == 1.0


def test_torch_output_equals_numpy_and_stacks_of_any_length(path):
    import torch
    from opticalflow_amd import optical_flow as of
    for frames, shape in ((2, (24, 24)), (40, (24, 36))):
        movie = texture(*shape, frames=frames, seed=8)
        for rem in (False, True):
            host = of.conduct_optical_flow(movie, 7, 0.5, 0.25, smoothing_sigma=1.0, include_remodelling=rem)
            dev = of.conduct_optical_flow(torch.as_tensor(movie).cuda(), 7, 0.5, 0.25, smoothing_sigma=1.0, include_remodelling=rem,
                                          output="torch")
            assert sorted(host) == sorted(dev) and host["v_x"].shape == (frames - 1,) + shape
            for k in ("v_x", "v_y", "speed", "blurred_data") + (("net_remodelling",) if rem else ()):
                assert dev[k].is_cuda and dev[k].dtype == torch.float64
                assert np.array_equal(host[k], dev[k].cpu().numpy(), equal_nan=True), (frames, rem, k)
            jit = of.conduct_optical_flow_jit(host["blurred_data"], 7, 0.5, 0.25, rem)
            assert len(jit) == 4
            for k, f in zip(("v_x", "v_y", "speed"), jit):
                assert np.array_equal(host[k], f, equal_nan=True)
            assert np.array_equal(jit[3], host["net_remodelling"]) if rem else not jit[3].any()
            # every pair depends on its two frames only
            one = of.conduct_optical_flow_jit(host["blurred_data"][-2:], 7, 0.5, 0.25, rem)
            assert np.array_equal(one[0][0], host["v_x"][-1], equal_nan=True)


def test_errors_by_return_code():
    from opticalflow_amd import _native
    movie = texture(16, 16)
    with _native.Solver(16, 16, 1) as s:
        with pytest.raises(_native.VofError, match="box_size"):
            s.box_flow_host(movie, 0)
        with pytest.raises(_native.VofError, match="two frames"):
            s.box_flow_host(movie[:1], 5)
        rc = s.lib.vof_box_flow_host(s.h, _native._ptr(movie), 2, 5, 1.0, 1.0, 0, 1, None, None, None, None)
        assert rc != 0 and b"NULL" in s.lib.vof_last_error(s.h)
