"""Every entry that takes ``output=`` has one body for host arrays and device tensors (the Python layer).  This file pins
what the two modes share, at 4 frames of 24 x 40 pixels (Farnebaeck needs sides >= 16; box sizes on both sides of the fused / general
switch at 31):

  * the result has the same keys (or tuple length) in both modes, and the documented dtypes and shapes;
  * the identity rules: ``original_data`` is the object passed in; ``blurred_data`` of the box flow and of the channel comparison is
    that object too when nothing was subtracted or blurred (for a device tensor that already is float64: the float64 device stack is
    the tensor itself), and a float64 device stack for a uint8 tensor; ``conduct_opencv_flow`` has no ``blurred_data`` and returns
    the blurred movie as ``original_data`` when it blurs; ``variational_optical_flow`` on host arrays returns its float64 copy of the
    movie as both when nothing is blurred;
  * on a float64 movie every array of the result has the same bits in both modes.  This holds for every entry here, the variational
    solve included (tests/test_gpu_consumers.py pins that one at a larger shape), so no entry is compared at a tolerance.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, N_I, N_J = 4, 24, 40
FARNEBACK = dict(pyr_scale=0.5, levels=2, winsize=9, iterations=2, poly_n=5, poly_sigma=1.1)


def make_movie():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:N_I, 0:N_J]
    return np.stack([100.0 + 60.0 * np.sin(0.31 * (yy + 0.7 * k)) * np.cos(0.23 * (xx - 0.9 * k)) + 5.0 * rng.random((N_I, N_J))
                     for k in range(T)])


MOVIE = make_movie()
OTHER = np.ascontiguousarray(MOVIE[::-1]) * 0.5 + 20.0

# name -> call(of, movie, other, output); movie and other are arrays of the side ``output`` names
ENTRIES = {
    "box_flow_fused": lambda of, m, o, out: of.conduct_optical_flow(m, 31, output=out),
    "box_flow_general": lambda of, m, o, out: of.conduct_optical_flow(m, 33, include_remodelling=True, output=out),
    "box_flow_blur_background": lambda of, m, o, out: of.conduct_optical_flow(m, 7, 0.5, 2.0, 1.5, 90, True, reference_quirks=False, output=out),
    "opencv_flow": lambda of, m, o, out: of.conduct_opencv_flow(m, 0.5, 2.0, output=out, **FARNEBACK),
    "opencv_flow_blur_box": lambda of, m, o, out: of.conduct_opencv_flow(m, smoothing_sigma=1.2, window="box", output=out, **FARNEBACK),
    "farneback_pair_box": lambda of, m, o, out: of.calcOpticalFlowFarneback(m[0], m[1], None, 0.5, 2, 9, 2, 5, 1.1, 0, output=out),
    "farneback_pair_gaussian": lambda of, m, o, out: of.calcOpticalFlowFarneback(m[0], m[1], None, 0.5, 1, 7, 1, 7, 1.5, 256, output=out),
    "liu_shen_scalars": lambda of, m, o, out: of.liu_shen_optical_flow_jit(m, 0.5, 2.0, 50, 1.0, 0.1, -0.2, 0.3, 4, output=out),
    "liu_shen_plane_and_stack": lambda of, m, o, out: of.liu_shen_optical_flow_jit(m, 1.0, 1.0, 100, 1.0, 0.01 * m[:-1], 0.02 * o[1], 0.0, 3,
                                                                                   output=out),
    "compare_channels": lambda of, m, o, out: of.compare_channel_flows(m, o, 7, histogram_range=(0.0, 3.0), joint_speed_bins=(5, 6),
                                                                       joint_speed_ranges=((0, 2), (0, 3)), return_fields=True, output=out),
    "compare_channels_blur_background": lambda of, m, o, out: of.compare_channel_flows(
        m, o, 33, 0.5, 2.0, (1.0, None), (None, 80), True, histogram_range=(0.0, 3.0), return_fields=True, output=out),
    "variational": lambda of, m, o, out: of.variational_optical_flow(m, 0.5, 2.0, 2.0, 500.0, output=out),
    "variational_blur": lambda of, m, o, out: of.variational_optical_flow(m, smoothing_sigma=1.0, reference_quirks=False, output=out),
    "vary_boxsize": lambda of, m, o, out: of.vary_boxsize(m, [9, 35], 0.5, 2.0, 1.0, 90, True, return_fields=True, histogram_bins=6,
                                                           histogram_range=(0.0, 2.0), probe_locations=[[3, 4], [20, 30]], output=out),
    "vary_blursize": lambda of, m, o, out: of.vary_blursize(m, [0.6, 1.4], 33, histogram_bins=8, histogram_range=(0.0, 3.0), angle_bins=6,
                                                             intensity_bins=5, intensity_range=(0.0, 255.0), return_fields=True, output=out),
    "adaptive_threshold": lambda of, m, o, out: of.apply_adaptive_threshold(m, 7, 1.0, output=out),
    "clahe": lambda of, m, o, out: of.apply_clahe(m, 40000, 3, output=out),
    "downsample": lambda of, m, o, out: of.downsample_movie(m, (10, 17), output=out),
}


def on_side(array, output):
    import torch
    return array if output == "numpy" else torch.as_tensor(array).cuda()


def both_modes(name, movie=MOVIE, other=OTHER):
    """(arguments, result) of entry ``name`` per mode."""
    from opticalflow_amd import optical_flow as of
    runs = {}
    for output in ("numpy", "torch"):
        m, o = on_side(movie, output), on_side(other, output)
        runs[output] = (m, o, ENTRIES[name](of, m, o, output))
    return runs


def leaves(value, path=""):
    """(path, leaf) of a result: dicts and tuples are walked, everything else is a leaf."""
    if isinstance(value, dict):
        for k, v in value.items():
            yield from leaves(v, f"{path}.{k}")
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            yield from leaves(v, f"{path}[{i}]")
    else:
        yield path, value


def host(leaf):
    return leaf.cpu().numpy() if hasattr(leaf, "data_ptr") and not isinstance(leaf, np.ndarray) else np.asarray(leaf)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_same_keys_and_same_bits_in_both_modes(name):
    import torch
    runs = both_modes(name)
    numpy_leaves, torch_leaves = dict(leaves(runs["numpy"][2])), dict(leaves(runs["torch"][2]))
    assert list(numpy_leaves) == list(torch_leaves)
    for path, a in numpy_leaves.items():
        b = torch_leaves[path]
        assert not isinstance(a, torch.Tensor), path
        if path.endswith((".v_x", ".v_y", ".speed")):
            assert isinstance(b, torch.Tensor) and b.is_cuda, path                 # a field stack stays on its side
        a, b = host(a), host(b)
        assert a.dtype == b.dtype and a.shape == b.shape, path
        assert a.tobytes() == b.tobytes(), path


@pytest.mark.parametrize("name", ["box_flow_fused", "box_flow_general", "box_flow_blur_background"])
def test_box_flow_identities(name):
    for output, (movie, _, res) in both_modes(name).items():
        assert list(res)[:7] == ["v_x", "v_y", "speed", "original_data", "delta_x", "delta_t", "blurred_data"]
        assert ("net_remodelling" in res) == (name != "box_flow_fused")
        assert res["original_data"] is movie
        assert (res["blurred_data"] is movie) == (name != "box_flow_blur_background"), output
        assert res["v_x"].shape == (T - 1, N_I, N_J) and str(res["blurred_data"].dtype).endswith("float64")


def test_box_flow_of_an_integer_movie_keeps_the_object_on_the_host_only():
    import torch
    movie = np.clip(MOVIE, 0, 255).astype(np.uint8)
    runs = both_modes("box_flow_fused", movie=movie)
    assert runs["numpy"][2]["blurred_data"] is movie
    dev = runs["torch"][2]
    assert dev["original_data"] is runs["torch"][0]
    assert dev["blurred_data"].dtype == torch.float64 and dev["blurred_data"].is_cuda
    assert np.array_equal(dev["blurred_data"].cpu().numpy(), movie.astype(np.float64))


def test_channel_comparison_identities():
    for output, (movie, other, res) in both_modes("compare_channels").items():
        for key, passed in (("a", movie), ("b", other)):
            assert res[key]["original_data"] is passed and res[key]["blurred_data"] is passed, (output, key)
            assert set(res[key]) == {"v_x", "v_y", "speed", "original_data", "delta_x", "delta_t", "blurred_data"}
    for output, (movie, other, res) in both_modes("compare_channels_blur_background").items():
        for key, passed in (("a", movie), ("b", other)):
            assert res[key]["original_data"] is passed and res[key]["blurred_data"] is not passed, (output, key)
            assert "net_remodelling" in res[key]


def test_opencv_flow_identities():
    for output, (movie, _, res) in both_modes("opencv_flow").items():
        assert list(res) == ["v_x", "v_y", "speed", "original_data", "delta_x", "delta_t"]
        assert res["original_data"] is movie
    for output, (movie, _, res) in both_modes("opencv_flow_blur_box").items():
        assert "blurred_data" not in res and res["original_data"] is not movie
        assert tuple(res["original_data"].shape) == (T, N_I, N_J) and str(res["original_data"].dtype).endswith("float64")
        assert not np.array_equal(host(res["original_data"]), MOVIE)


def test_variational_identities():
    runs = both_modes("variational")
    movie, _, res = runs["numpy"]
    assert res["original_data"] is not movie and res["blurred_data"] is res["original_data"]
    assert np.array_equal(res["original_data"], movie)
    movie, _, res = runs["torch"]
    assert res["original_data"] is movie and res["blurred_data"] is movie
    for output, (movie, _, res) in both_modes("variational_blur").items():
        assert res["blurred_data"] is not res["original_data"]


def test_return_shapes_and_dtypes():
    import torch
    from opticalflow_amd import optical_flow as of
    for output, (_, _, res) in both_modes("liu_shen_scalars").items():
        assert len(res) == 5 and res[4] == 3 and all(tuple(f.shape) == (T - 1, N_I, N_J) for f in res[:4])
    for output, (_, _, res) in both_modes("farneback_pair_box").items():
        assert tuple(res.shape) == (N_I, N_J, 2) and str(res.dtype).endswith("float32")
    masks = both_modes("adaptive_threshold")
    assert masks["numpy"][2].dtype == np.bool_ and masks["torch"][2].dtype == torch.bool
    for name, shape in (("clahe", (T, N_I, N_J)), ("downsample", (T, 10, 17))):
        for output, (_, _, res) in both_modes(name).items():
            assert tuple(res.shape) == shape and str(res.dtype).endswith("float64")
    jit = of.conduct_optical_flow_jit(MOVIE, 7)
    assert len(jit) == 4 and all(f.shape == (T - 1, N_I, N_J) and f.dtype == np.float64 for f in jit) and not jit[3].any()
    flow = of.conduct_optical_flow(MOVIE, 7)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(jit[:3], (flow["v_x"], flow["v_y"], flow["speed"])))
