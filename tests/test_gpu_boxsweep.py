"""GPU tests of the box-size sweep (vary_boxsize / vof_vary_boxsize_*).

Bounds, none of them taken from what the GPU gives:
* up to box 41: the bound of the box flow, non-finite values at exactly the reference's positions and
  |gpu - ref| <= 64 * eps * kappa_max * max|field| (tests/test_boxflow_cpu.py assert_matches);
* boxes 75 and 121: kappa counts the determinant only and misses the cancellation n = box^2 brings into the numerators, so
  the yardstick is the error of the direct-sum order every other path uses: with E = max |field - longdouble evaluation|
  over the finite pixels, E_gpu <= 2 * E_direct (the factor: a margin over the 0.93 - 1.23 the recurrence shows on the CPU);
* integer data: bit-identical, every order sums exactly;
* statistics: rtol 1e-12 against numpy (the tolerance of tests/test_gpu_consumers.py for the same reduction), counts exact.
Every comparison prints its figure before it asserts."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from boxflow_restatement import box_flow  # noqa: E402
from boxsweep_restatement import box_flow_extended  # noqa: E402
from test_boxflow_cpu import assert_matches, runs_of  # noqa: E402

pytestmark = pytest.mark.gpu
UNITS = 64
FIELDS = ("v_x", "v_y", "speed", "net_remodelling")


def texture(n_i, n_j, frames=2, seed=5):
    from oracle import vof_oracle as orc
    n = max(n_i, n_j)
    return np.ascontiguousarray(orc.make_texture_stack(n, frames, seed=seed)[:, :n_i, :n_j])


def sweep(movie, boxes, dx=1.0, dt=1.0, rem=False, entry="host", quirks=True, **kw):
    """vary_boxsize with fields; the field stacks as numpy arrays, net_remodelling zeros without remodelling."""
    from opticalflow_amd import optical_flow as of
    if entry == "host":
        res = of.vary_boxsize(movie, boxes, dx, dt, include_remodelling=rem, return_fields=True, reference_quirks=quirks, **kw)
    else:
        import torch
        res = of.vary_boxsize(torch.as_tensor(movie).cuda(), boxes, dx, dt, include_remodelling=rem, return_fields=True,
                              reference_quirks=quirks, output="torch", **kw)
        for k in FIELDS[:3] + (("net_remodelling",) if rem else ()):
            assert res[k].is_cuda and res[k].dtype == torch.float64
            res[k] = res[k].cpu().numpy()
    if not rem:
        res["net_remodelling"] = np.zeros_like(res["v_x"])
    return res


def at(res, b):
    return {k: res[k][b] for k in FIELDS}


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in FIELDS)


@pytest.mark.parametrize("entry", ["host", "torch"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_fixture_cases(case, entry):
    for label, movie, box, dx, dt, rem, ref in runs_of(case):
        kappa = box_flow(movie, box, dx, dt, include_remodelling=rem)["kappa"]
        boxes = (box + 4, 3, box, 2 * (box // 2))
        res = sweep(movie, boxes, dx, dt, rem, entry)
        assert np.array_equal(res["boxsizes"], boxes)
        assert_matches(at(res, 2), ref, kappa, UNITS, f"{label} {entry}")


def test_integer_data_is_bit_identical():
    from opticalflow_amd import optical_flow as of
    boxes = (1, 2, 3, 8, 15, 16, 31, 41)
    for label, movie, _box, dx, dt, rem, _ref in runs_of("d"):
        res = sweep(movie, boxes, dx, dt, rem)
        for b, box in enumerate(boxes):
            jit = dict(zip(FIELDS, of.conduct_optical_flow_jit(movie, box, dx, dt, rem)))
            for k in ("v_x", "v_y", "net_remodelling"):
                with np.errstate(invalid="ignore"):
                    d = np.abs(res[k][b] - jit[k])
                diff = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
                print(f"{label} box {box} {k}: max difference {diff}")
                assert np.array_equal(res[k][b], jit[k], equal_nan=True), (label, box, k)
            with np.errstate(invalid="ignore"):
                ulp = np.spacing(np.abs(jit["speed"]))
                d = np.abs(res["speed"][b] - jit["speed"]) / ulp
            assert np.array_equal(np.isfinite(res["speed"][b]), np.isfinite(jit["speed"]))
            worst = float(np.nanmax(np.where(np.isfinite(jit["speed"]), d, 0.0)))
            print(f"{label} box {box} speed: {worst} ulp")
            assert worst <= 1.0


@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("rem", [False, True])
@pytest.mark.parametrize("shape,boxes", [((24, 40), (41, 3, 16, 15, 9, 9, 1)), ((40, 24), (41, 3, 16, 15, 9, 9, 1)),
                                         ((33, 65), (41, 3, 16, 15, 9, 9, 1)), ((31, 63), (41, 3, 16, 15, 9, 9, 1)),
                                         ((16, 20), (51, 100))])
def test_equivalence_per_box(shape, boxes, rem, quirks):
    movie = texture(*shape, frames=3, seed=3)
    res = sweep(movie, boxes, 0.25, 0.5, rem, "host", quirks)
    for b, box in enumerate(boxes):
        r = box_flow(movie, box, 0.25, 0.5, include_remodelling=rem, reference_quirks=quirks)
        assert_matches(at(res, b), {k: r[k] for k in FIELDS}, r["kappa"], UNITS, f"{shape} box {box} rem {rem} quirks {quirks}")
    if len(boxes) > 2:
        assert same_bits(at(res, 4), at(res, 5))


@pytest.mark.parametrize("rem", [False, True])
@pytest.mark.parametrize("shape", [(258, 130), (130, 258)])
def test_large_boxes_against_extended_precision(shape, rem):
    movie = texture(*shape)
    boxes = (75, 121)
    res = sweep(movie, boxes, 0.5, 2.0, rem, "torch")
    for b, box in enumerate(boxes):
        exact = box_flow_extended(movie, box, 0.5, 2.0, include_remodelling=rem)
        direct = box_flow(movie, box, 0.5, 2.0, include_remodelling=rem)
        for k in ("v_x", "v_y", "net_remodelling") + (() if rem else ("speed",)):
            x, g, d = exact[k], res[k][b], direct[k]
            assert np.array_equal(np.isfinite(g), np.isfinite(d)) and np.array_equal(np.isnan(g), np.isnan(d)), (shape, box, k)
            fin = np.isfinite(d)
            e_gpu = float(np.abs(g[fin] - x[fin]).max()) if fin.any() else 0.0
            e_direct = float(np.abs(d[fin] - x[fin]).max()) if fin.any() else 0.0
            print(f"{shape} box {box} rem {rem} {k}: E_gpu {e_gpu:.3e}, E_direct {e_direct:.3e}, ratio {e_gpu / e_direct if e_direct else 0.0:.3f}")
            assert e_gpu <= 2 * e_direct, (shape, box, rem, k, e_gpu, e_direct)


def test_independence_of_the_list_and_of_chunking():
    from opticalflow_amd import _native
    movie = texture(24, 36, frames=6, seed=11)
    for rem in (False, True):
        alone = at(sweep(movie, (21,), rem=rem), 0)
        assert same_bits(alone, at(sweep(movie, (5, 21, 33), rem=rem), 1))
        pair = sweep(movie, (20, 21), rem=rem)
        assert same_bits(alone, at(pair, 1))
        if not rem:
            assert same_bits(at(pair, 0), at(pair, 1))
        # one pair slot: the five pairs go through in five chunks
        with _native.Solver(24, 36, 1) as s:
            _st, _h, _p, chunked = s.vary_boxsize_host(movie, (5, 21), include_remodelling=rem, return_fields=True)
            for k in range(5):
                _st, _h, _p, single = s.vary_boxsize_host(movie[k:k + 2], (5, 21), include_remodelling=rem, return_fields=True)
                for f in range(4 if rem else 3):
                    assert np.array_equal(chunked[f][:, k], single[f][:, 0], equal_nan=True), (rem, k, f)
                assert rem or (chunked[3] is None and single[3] is None)
        assert np.array_equal(chunked[0][1], alone["v_x"], equal_nan=True)


@pytest.mark.parametrize("entry", ["host", "torch"])
def test_statistics(entry):
    from opticalflow_amd import optical_flow as of
    import torch
    boxes = (7, 4, 21)
    for shape, rem, quirks in (((36, 24), False, True), ((24, 36), True, False), ((24, 40), False, True)):
        movie = texture(*shape, frames=4, seed=2)
        probes = [(0, 0), (5, 7), (shape[0] - 1, shape[1] - 1), (shape[0] - 1, 0)]      # one on the last row and column
        arg = torch.as_tensor(movie).cuda() if entry == "torch" else movie
        kw = dict(include_remodelling=rem, reference_quirks=quirks, output="torch" if entry == "torch" else "numpy",
                  probe_locations=probes)
        full = of.vary_boxsize(arg, boxes, 0.5, 0.25, return_fields=True, **kw)
        speed = full["speed"].cpu().numpy() if entry == "torch" else full["speed"]
        finite = speed[np.isfinite(speed)]
        wide = (0.0, float(finite.max()))
        cut = (float(np.quantile(finite, 0.1)), float(np.quantile(finite, 0.9)))
        if not cut[1] > cut[0]:
            cut = (wide[1] * 0.25, wide[1] * 0.5 + 1.0)
        for rng in (wide, cut):
            with_fields = of.vary_boxsize(arg, boxes, 0.5, 0.25, return_fields=True, histogram_bins=50, histogram_range=rng, **kw)
            stats_only = of.vary_boxsize(arg, boxes, 0.5, 0.25, histogram_bins=50, histogram_range=rng, **kw)
            assert "speed" not in stats_only and "v_x" not in stats_only
            for k in ("speed_means", "speed_stds", "nonfinite_counts", "speed_histograms", "probe_speeds", "histogram_edges") + \
                    (("remodelling_means", "remodelling_stds") if rem else ()):
                assert np.array_equal(with_fields[k], stats_only[k], equal_nan=True), (shape, k)
            assert stats_only["speed_histograms"].dtype == np.int64 and stats_only["speed_histograms"].shape == (3, 50)
            assert np.array_equal(stats_only["histogram_edges"], np.linspace(rng[0], rng[1], 51))
            for b in range(3):
                ref = np.histogram(speed[b].ravel(), bins=50, range=rng)[0]
                assert np.array_equal(stats_only["speed_histograms"][b], ref), (shape, boxes[b], rng)
        assert sorted(set(full) - set(stats_only)) == sorted(["v_x", "v_y", "speed"] + (["net_remodelling"] if rem else []))
        for b in range(3):
            with np.errstate(invalid="ignore"):
                m, s = np.mean(speed[b]), np.std(speed[b])
            print(f"{shape} box {boxes[b]}: mean {full['speed_means'][b]} / {m}, std {full['speed_stds'][b]} / {s}")
            np.testing.assert_allclose(full["speed_means"][b], m, rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(full["speed_stds"][b], s, rtol=1e-12, atol=0, equal_nan=True)
            assert full["nonfinite_counts"][b] == (~np.isfinite(speed[b])).sum()
            if rem:
                g = full["net_remodelling"].cpu().numpy() if entry == "torch" else full["net_remodelling"]
                np.testing.assert_allclose(full["remodelling_means"][b], np.mean(g[b]), rtol=1e-12, atol=0, equal_nan=True)
                np.testing.assert_allclose(full["remodelling_stds"][b], np.std(g[b]), rtol=1e-12, atol=0, equal_nan=True)
            else:
                assert "remodelling_means" not in full
            assert full["probe_speeds"].shape == (3, 3, 4)
            for l, (i, j) in enumerate(probes):
                assert np.array_equal(full["probe_speeds"][b, :, l], speed[b, :, i, j], equal_nan=True)
        if shape == (24, 40):        # the column-clamp quirk leaves columns with empty windows
            assert np.isnan(full["speed_means"]).all() and (full["nonfinite_counts"] > 0).all()
        else:
            assert np.isfinite(full["speed_means"]).all()


@pytest.mark.parametrize("rem", [False, True])
@pytest.mark.parametrize("shape", [(24, 40), (31, 63)])
def test_torch_output_equals_numpy_bitwise(shape, rem):
    """output="torch" (device movie, fields stored straight into device stacks, up to 32 pairs per launch) against
    output="numpy" (host movie, chunks of the wrapper's 8-pair context bounced back): every field stack and every summary
    bit for bit, plain and with the torch wrapper's own background / smoothing_sigma steps.  10 pairs are more than one host
    chunk; (24, 40) with quirks has empty windows, so NaN positions and NaN summaries are compared too."""
    import torch
    from opticalflow_amd import optical_flow as of
    movie = texture(*shape, frames=11, seed=7)
    boxes = (41, 3, 16, 15, 9, 9, 1)
    probes = [(0, 0), (5, 7), (shape[0] - 1, shape[1] - 1)]
    level = float(np.median(movie))
    for kw in (dict(), dict(smoothing_sigma=1.5), dict(background=level), dict(smoothing_sigma=1.5, background=level)):
        kw = dict(kw, include_remodelling=rem, return_fields=True, histogram_bins=50, histogram_range=(0.0, 2.0),
                  probe_locations=probes)
        host = of.vary_boxsize(movie, boxes, 0.5, 0.25, **kw)
        dev = of.vary_boxsize(torch.as_tensor(movie).cuda(), boxes, 0.5, 0.25, output="torch", **kw)
        assert sorted(host) == sorted(dev)
        stacks = ("v_x", "v_y", "speed") + (("net_remodelling",) if rem else ())
        assert "net_remodelling" in host or not rem
        for k in host:
            got = dev[k]
            if k in stacks:
                assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64, k
                assert got.shape == (len(boxes), 10) + shape and host[k].shape == got.shape
                got = got.cpu().numpy()
            else:
                assert not isinstance(got, torch.Tensor), k
            same = np.array_equal(np.asarray(got), np.asarray(host[k]), equal_nan=True)
            print(f"{shape} rem {rem} {sorted(set(kw) & {'smoothing_sigma', 'background'})} {k}: {'same bits' if same else 'DIFFERENT'}")
            assert same, (shape, rem, k)
        assert np.isfinite(host["speed"]).any()


def test_wrapper_steps_and_saved_file(tmp_path):
    """Pre-processing as conduct_optical_flow does it, on a crop of case f.  Two summation orders agree bit for bit only
    where they are the same order, which for the ring-growing sweep and the direct sums of conduct_optical_flow is h = 0: at
    box 1 the whole pipeline (background, blur, flow) must give conduct_optical_flow's bits.  At the larger boxes the
    pre-processing is pinned bit for bit through the sweep of conduct_optical_flow's own analysed movie, and the fields
    against conduct_optical_flow's at the bound of the other float-data comparisons (64 units)."""
    from opticalflow_amd import optical_flow as of
    g = load_golden("g11f_boxflow.npz")
    movie = np.ascontiguousarray(g["movie"][:, :40, :48])
    boxes = (1, 9, 22)
    names = lambda rem: ("v_x", "v_y", "speed") + (("net_remodelling",) if rem else ())     # noqa: E731
    for kw in (dict(smoothing_sigma=float(g["smoothing_sigma"])), dict(background=float(g["background"])),
               dict(smoothing_sigma=1.5, background=float(g["background"]))):
        for rem in (False, True):
            res = of.vary_boxsize(movie, boxes, 0.5, 0.25, include_remodelling=rem, return_fields=True, **kw)
            one = of.conduct_optical_flow(movie, 1, 0.5, 0.25, include_remodelling=rem, **kw)
            for k in names(rem):
                assert np.array_equal(res[k][0], one[k], equal_nan=True), (kw, rem, 1, k)
            plain = of.vary_boxsize(one["blurred_data"], boxes, 0.5, 0.25, include_remodelling=rem, return_fields=True)
            for k in names(rem):
                assert np.array_equal(res[k], plain[k], equal_nan=True), (kw, rem, k)
            assert np.array_equal(res["speed_means"], plain["speed_means"], equal_nan=True)
            for b, box in list(enumerate(boxes))[1:]:
                one = of.conduct_optical_flow(movie, box, 0.5, 0.25, include_remodelling=rem, **kw)
                kappa = box_flow(one["blurred_data"], box, 0.5, 0.25, include_remodelling=rem)["kappa"]
                assert_matches({k: res[k][b] for k in names(rem)}, {k: one[k] for k in names(rem)}, kappa, UNITS,
                               f"{sorted(kw)} box {box} rem {rem}")
    name = str(tmp_path / "sweep.npy")
    res = of.vary_boxsize(movie, np.linspace(3, 21, 4), filename=name, histogram_bins=10, histogram_range=(0.0, 2.0))
    assert np.array_equal(res["boxsizes"], [3, 9, 15, 21])
    back = np.load(name, allow_pickle=True).item()
    assert sorted(back) == sorted(res) == sorted(["boxsizes", "speed_means", "speed_stds", "nonfinite_counts", "speed_histograms",
                                                  "histogram_edges", "delta_x", "delta_t"])
    for k in res:
        assert np.array_equal(back[k], res[k], equal_nan=True), k


def test_errors():
    from opticalflow_amd import _native, optical_flow as of
    movie = texture(16, 16)
    with _native.Solver(16, 16, 1) as s:
        def call(n_frames, boxes, stats=True):
            b = np.asarray(boxes, dtype=np.int32)
            st = np.zeros(max(b.size, 1), dtype=_native.BOXSIZE_DTYPE)
            rc = s.lib.vof_vary_boxsize_host(s.h, _native._ptr(movie), n_frames, _native._ptr(b) if b.size else None, b.size, 1.0, 1.0,
                                             0, 1, None, 0, None, 0, None, None, 0, None, _native._ptr(st) if stats else None,
                                             None, None, None, None)
            return rc, s.lib.vof_last_error(s.h)
        for args, text in (((2, []), b"empty"), ((2, [5, 0]), b">= 1"), ((1, [5]), b"two frames"), ((2, [5], False), b"NULL")):
            rc, msg = call(*args)
            print(args, rc, msg)
            assert rc != 0 and text in msg
        rc, _msg = call(2, [5, 4])
        assert rc == 0
    with pytest.raises(ValueError, match="histogram_range"):
        of.vary_boxsize(movie, [5], histogram_bins=50)
    with pytest.raises(ValueError, match="probe outside"):
        of.vary_boxsize(movie, [5], probe_locations=[(16, 3)])
