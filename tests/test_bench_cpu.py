"""bench.py --dump-outputs on host tensors: whole fields below the limit, the same seeded sample of the flattened field
above it (also when the field is held in several chunks), float64 files only."""
import os

import numpy as np
import pytest
import torch

import bench


def _fields(rng, shapes):
    parts = [torch.from_numpy(rng.standard_normal(s)) for s in shapes]
    return parts, np.concatenate([p.numpy() for p in parts])


@pytest.mark.parametrize("shapes", [[(5, 4, 4)], [(2, 4, 4), (3, 4, 4)]])
def test_dump_whole_and_sampled_fields(tmp_path, shapes):
    rng = np.random.default_rng(3)
    parts, whole = _fields(rng, shapes)
    stats = np.zeros(5, dtype=[(k, np.float64) for k in bench.DUMP_STATS])
    stats["iterations"] = np.arange(5)
    bench.dump_outputs(str(tmp_path / "all"), {"v_x": parts}, stats, limit=whole.size)
    bench.dump_outputs(str(tmp_path / "some"), {"v_x": parts}, stats, limit=17)
    a = np.load(tmp_path / "all" / "v_x.npy")
    np.testing.assert_array_equal(a, whole)
    s = np.load(tmp_path / "some" / "v_x.npy")
    idx = bench.sample_index(whole.size, 17)
    assert s.shape == (17,) and len(np.unique(idx)) == 17
    np.testing.assert_array_equal(s, whole.reshape(-1)[idx])
    np.testing.assert_array_equal(idx, bench.sample_index(whole.size, 17))      # the same sample in every run
    for d in ("all", "some"):
        names = sorted(os.listdir(tmp_path / d))
        assert names == sorted(["v_x.npy"] + [k + ".npy" for k in bench.DUMP_STATS])
        for f in names:
            assert np.load(tmp_path / d / f).dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "iterations.npy"), np.arange(5))


def test_dumped_fields_stay_within_32_mb():
    # four float64 fields of at most DUMP_SAMPLE values; the per-pair statistics add 48 B per pair
    assert 4 * bench.DUMP_SAMPLE * 8 <= 32 * 2 ** 20
