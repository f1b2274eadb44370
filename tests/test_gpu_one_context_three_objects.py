"""One context driven through calls of all three sources of libvof.so (csrc/vof.hip, vof_pairs.hip, vof_frames.hip; DESIGN.md
section 1.1), there and back: what crosses the object boundaries - the scratch arena regrown under another caller, the solver's
staging slots that the box flow on host arrays borrows, the one-time dynamic-LDS attribute flags - leaves every result of the
second round byte for byte that of the first, and no buffer is written outside its bounds.

48 x 40 with 2 pairs in flight and 4 frames: three pairs are two batches of the solver, two chunks of the box flow, of the
box-size sweep and of conduct_piv (two pairs in flight); four frames are two chunks of CLAHE; 48 x 40 is more than one workgroup
of every kernel (blur 64 x 4 threads, box flow and Liu-Shen 32 x 32 tiles, PIV a workgroup per window)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from boxflow_restatement import box_flow  # noqa: E402
from test_boxflow_cpu import assert_matches  # noqa: E402

pytestmark = pytest.mark.gpu

N_I, N_J, SLOTS, FRAMES = 48, 40, 2, 4
SIGMA = 1.5
PIV = dict(window=16, radius=4, step=8)


def movie():
    """The texture of the oracle on the 8-bit scale (CLAHE takes no other), whole numbers."""
    from oracle import vof_oracle as orc
    m = np.ascontiguousarray(np.round(255.0 * orc.make_texture_stack(max(N_I, N_J), FRAMES, seed=7)[:, :N_I, :N_J]))
    assert m.shape == (FRAMES, N_I, N_J) and m.min() >= 0 and m.max() <= 255 and m.max() > 100
    return m


def calls(m):
    """(name, call); a call returns the list of its output arrays."""
    from opticalflow_amd import _native, optical_flow as of
    params = _native.default_params(speed_alpha=2.0 * 255.0 ** 2, remodelling_alpha=100.0)
    taps = of.gaussian_taps(SIGMA)
    grid = ((N_I - PIV["window"] - 2 * PIV["radius"]) // PIV["step"] + 1, (N_J - PIV["window"] - 2 * PIV["radius"]) // PIV["step"] + 1)
    assert grid == (4, 3)

    def piv(s):
        outs = [np.empty((FRAMES - 1,) + grid) for _ in range(3)]
        counts = s.piv_flow(m, FRAMES - 1, [PIV["window"]], [PIV["radius"]], [PIV["step"]], *outs, None, 2)
        return outs + [counts]

    def boxsizes(s):
        stats, _hist, _probes, fields = s.vary_boxsize_host(m, (3, 7), return_fields=True)
        return [np.asarray(stats)] + [f for f in fields if f is not None]

    return [
        ("solve_host", lambda s: list(s.solve_host(m, params)[:4])),
        ("blur_host", lambda s: [s.blur_host(m, taps)]),
        ("box_flow_host", lambda s: list(s.box_flow_host(m, 5))),
        ("vary_boxsize_host", boxsizes),
        ("clahe_host", lambda s: [s.clahe_host(m, 2.0, 2, 2, frames_in_flight=2)]),
        ("liu_shen_host", lambda s: list(s.liu_shen_host(m, max_iterations=3))),
        ("piv_flow", piv),
    ]


def test_there_and_back_on_one_context(monkeypatch):
    from opticalflow_amd import _native
    from oracle import vof_oracle as orc
    monkeypatch.setenv("VOF_DEBUG_CANARY", "1")                     # guard regions around every device buffer of the context
    m = movie()
    todo = calls(m)
    with _native.Solver(N_I, N_J, SLOTS) as s:
        first = {name: call(s) for name, call in todo}
        second = {name: call(s) for name, call in reversed(todo)}
        s.check_canaries()
    assert list(first) == [name for name, _ in todo] and list(second) == list(reversed(list(first)))
    for name, outs in first.items():
        assert outs and len(outs) == len(second[name]), name
        for i, (a, b) in enumerate(zip(outs, second[name])):
            assert isinstance(a, np.ndarray) and a.size and a.dtype == b.dtype and a.shape == b.shape, (name, i)
            assert a.tobytes() == b.tobytes(), (name, i)
    assert all(np.isfinite(f).all() for f in first["solve_host"]) and first["solve_host"][0].any()
    # the two calls whose kernels another source launches or whose staging another source owns, against the oracle: the blur
    # to 4 ulp of the data range (tests/test_gpu_consumers.py), the box flow in the units of tests/test_gpu_boxflow.py
    want = orc.blur_movie(m, SIGMA)
    worst = float(np.abs(first["blur_host"][0] - want).max())
    print("blur: largest difference from scipy", worst, "bound", 4 * np.finfo(np.float64).eps * 255.0)
    np.testing.assert_allclose(first["blur_host"][0], want, rtol=0, atol=4 * np.finfo(np.float64).eps * 255.0)
    r = box_flow(m, 5)
    got = dict(zip(("v_x", "v_y", "speed", "net_remodelling"), first["box_flow_host"]))
    assert_matches(got, {k: r[k] for k in got}, r["kappa"], 64, "box 5 on one context")
