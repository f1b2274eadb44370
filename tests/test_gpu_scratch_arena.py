"""GPU tests of the call-scoped scratch arena: the blur, the box flow's general path, the Liu-Shen flow, the sweeps,
the channel comparison and the frame-wise calls carve one buffer of the context anew in every call.  What a call computes inside
a buffer that another owner filled is compared bit for bit with the same call on a fresh context."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (24, 36)
SLOTS = 2                                  # the _host sweeps run their five pairs as three chunks
PROBES = [(0, 0), (5, 7), (23, 35), (23, 0)]
SPEED_EDGES = np.linspace(0.0, 4.0, 9)


@functools.lru_cache(maxsize=None)
def movies():
    """Two 24 x 36 textures of 6 frames (the texture() input of test_gpu_boxsweep.py), uint8-valued so the threshold accepts them."""
    from oracle import vof_oracle as orc
    out = []
    for seed in (11, 3):
        m = np.ascontiguousarray(np.round(255.0 * orc.make_texture_stack(max(SHAPE), 6, seed=seed)[:, :SHAPE[0], :SHAPE[1]]))
        assert m.min() >= 0 and m.max() <= 255 and m.max() > 100
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


def taps(sigma):
    from opticalflow_amd import optical_flow
    return optical_flow.gaussian_taps(sigma)


def box_flow_dev(solver, movie, box):
    import torch
    d = torch.as_tensor(np.array(movie)).cuda()
    fields = [torch.zeros((movie.shape[0] - 1,) + SHAPE, dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    solver.box_flow_dev(d, movie.shape[0], box, 1.0, 1.0, False, True, *fields)
    return None, tuple(f.cpu().numpy() for f in fields)


def summaries_and_fields(result):
    return result[:-1], result[-1]


def calls():
    """(name, call): small, then large, then small.  A call returns (summaries, fields), either a possibly nested tuple of arrays
    and None."""
    a, b = movies()
    assert taps(0.8).size == 7 and taps(1.6).size == 13                      # two radii
    boxsize = lambda s: summaries_and_fields(s.vary_boxsize_host(                                                  # noqa: E731
        a, (3, 8, 21), include_remodelling=True, weights=taps(1.0), histogram_edges=SPEED_EDGES, probe_locations=PROBES, return_fields=True))
    rng = np.random.default_rng(6)
    initial = [0.2 * rng.standard_normal((a.shape[0] - 1,) + SHAPE) for _ in range(3)]
    return [
        ("blur of one frame", lambda s: (s.blur_host(a[:1], taps(1.0)), None)),
        ("blur sweep", lambda s: summaries_and_fields(s.vary_blursize_host(
            a, [taps(0.8), taps(1.6)], 5, histogram_edges=SPEED_EDGES, angle_bins=8, intensity_edges=np.linspace(0.0, 255.0, 17),
            probe_locations=PROBES, return_fields=True))),
        ("box flow, general path, box wider than the image", lambda s: box_flow_dev(s, a, 33)),
        ("box-size sweep", boxsize),
        ("box flow on host arrays, box 33", lambda s: (None, s.box_flow_host(a, 33))),
        ("threshold", lambda s: (s.adaptive_threshold_host(a, 11, 2.5, frames_in_flight=2), None)),
        ("comparison", lambda s: summaries_and_fields(s.compare_flows_host(
            a, b, 7, weights_a=taps(0.8), weights_b=taps(1.6), histogram_edges=SPEED_EDGES, angle_bins=8, relative_angle_bins=10,
            joint_speed_edges=(np.linspace(0.0, 4.0, 6), np.linspace(0.0, 4.0, 5)), return_fields=True))),
        ("Liu-Shen on host arrays, stack initial fields", lambda s: (None, s.liu_shen_host(a, 0.5, 2.0, 10.0, *initial, 5))),
        ("blur of six frames", lambda s: (s.blur_host(a, taps(1.6)), None)),
        ("box-size sweep again", boxsize),
    ]


def arrays(x):
    if x is None:
        return []
    return [x] if isinstance(x, np.ndarray) else [a for part in x for a in arrays(part)]


def assert_same(got, want, name):
    """Summaries byte for byte; the fields element for element, a NaN equal to a NaN."""
    assert arrays(got), name
    for part, (g_all, w_all) in enumerate(zip(got, want)):
        g_all, w_all = arrays(g_all), arrays(w_all)
        assert len(g_all) == len(w_all), name
        for i, (g, w) in enumerate(zip(g_all, w_all)):
            assert g.dtype == w.dtype and g.shape == w.shape, (name, part, i)
            if part == 0:
                assert g.tobytes() == w.tobytes(), (name, i)
            else:
                assert np.array_equal(g, w, equal_nan=True), (name, i)


def solver():
    from opticalflow_amd import _native
    return _native.Solver(SHAPE[0], SHAPE[1], SLOTS)


def run_sequence(after_each_call=lambda s: None):
    results = []
    with solver() as s:
        for _name, call in calls():
            results.append(call(s))
            after_each_call(s)
    return results


@functools.lru_cache(maxsize=None)
def plain_sequence():
    return run_sequence()


def test_every_owner_in_turn_on_one_context():
    """Every result of the sequence equals the same call on a fresh context of its own: the counters are zeroed and nothing
    stale is read, although each statistics call runs inside a buffer the previous owner filled with other data."""
    for (name, call), got in zip(calls(), plain_sequence()):
        with solver() as fresh:
            assert_same(got, call(fresh), name)
    fields = arrays(plain_sequence()[3][1])
    assert len(fields) == 4 and all(f.shape == (3, 5) + SHAPE for f in fields)                     # the sweep did return its fields
    assert calls()[5][0] == "threshold"
    assert plain_sequence()[5][0].any() and not plain_sequence()[5][0].all()                       # the mask is no constant
    for at, name in ((4, "box flow on host arrays, box 33"), (7, "Liu-Shen on host arrays, stack initial fields")):
        assert calls()[at][0] == name
        v_x = plain_sequence()[at][1][0]
        assert np.isfinite(v_x).any() and np.unique(v_x[np.isfinite(v_x)]).size > 1, name            # the flow is no constant


def test_the_sequence_under_guard_regions_and_poison(monkeypatch):
    """The same sequence with guard regions around every device buffer and poisoned (0xFF: NaN) allocations: no guard region is
    touched by any call, the results are those of the plain run, and every field is finite where the plain run's is."""
    plain = plain_sequence()
    monkeypatch.setenv("VOF_DEBUG_CANARY", "1")
    monkeypatch.setenv("VOF_DEBUG_POISON", "1")
    guarded = run_sequence(lambda s: s.check_canaries())
    for (name, _call), got, want in zip(calls(), guarded, plain):
        assert_same(got, want, name)
        for g, w in zip(arrays(got[1]), arrays(want[1])):
            assert np.array_equal(np.isfinite(g), np.isfinite(w)), name


def test_the_context_holds_one_buffer_not_a_sum():
    """d(X): growth of workspace_bytes over a fresh context after call X alone.  After A, B, A on one context - A the box-size
    sweep on device tensors, statistics only; B the threshold on device tensors, two frames in flight; neither touches the
    solver's host staging - the growth is max(d(A), d(B)) exactly, and the repeat does not change it."""
    import torch
    a, _ = movies()
    d = torch.as_tensor(np.array(a)).cuda()
    mask = torch.zeros(a.shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    A = lambda s: s.vary_boxsize_dev(d, a.shape[0], (3, 8, 21), 1.0, 1.0, False, True, histogram_edges=SPEED_EDGES)     # noqa: E731
    B = lambda s: s.adaptive_threshold_dev(d, mask, a.shape[0], 11, 2.5, frames_in_flight=2)                            # noqa: E731
    growth = {}
    for key, call in (("A", A), ("B", B)):
        with solver() as s:
            before = s.workspace_bytes
            call(s)
            growth[key] = s.workspace_bytes - before
    assert growth["A"] > 0 and growth["B"] > 0 and growth["A"] != growth["B"]
    with solver() as s:
        before = s.workspace_bytes
        A(s)
        assert s.workspace_bytes - before == growth["A"]
        B(s)
        assert s.workspace_bytes - before == max(growth.values())
        A(s)
        assert s.workspace_bytes - before == max(growth.values())


def texture11():
    from oracle import vof_oracle as orc
    return np.ascontiguousarray(orc.make_texture_stack(20, 11, seed=4)[:, :16, :20])


def test_pair_chunks_do_not_depend_on_the_context():
    """The Liu-Shen flow on host arrays stages its own chunks of 8 pairs (here 8 + 2) in the arena, whatever the solver's batch
    capacity: contexts of 1 and of 8 pairs give the same bytes and grow by the same number of bytes.  (The box flow on host
    arrays still chunks by the context's pairs: profiles/pair_chunks_summary.md.)"""
    from opticalflow_amd import _native
    movie = texture11()
    rng = np.random.default_rng(12)
    initial = [0.2 * rng.standard_normal((10, 16, 20)) for _ in range(3)]
    results, growth = {}, {}
    for slots in (1, 8):
        with _native.Solver(16, 20, slots) as s:
            before = s.workspace_bytes
            fields = list(s.liu_shen_host(movie, 0.3, 0.7, 0.2, *initial, 7))
            results[slots], growth[slots] = fields, s.workspace_bytes - before
    assert len(results[1]) == len(results[8]) == 4
    for i, (one, eight) in enumerate(zip(results[1], results[8])):
        assert one.shape == (10, 16, 20) and one.tobytes() == eight.tobytes(), i
    assert all(np.isfinite(pair).all() and pair.any() for pair in results[1][0])                  # every pair holds a flow
    print("growth of workspace_bytes:", growth)
    assert growth[1] == growth[8] > 0


def test_the_liu_shen_flow_on_host_arrays_asks_for_a_context_of_one_pair():
    from opticalflow_amd import optical_flow as of
    of.release_device_memory()
    out = of.liu_shen_optical_flow_jit(texture11()[:10], 1.0, 1.0, 0.5, 1.0, 0.1, 0.1, 0.0, 3)
    assert out[0].shape == (9, 16, 20)
    assert of._cache["solver"].max_pairs == 1
