"""tests/summary_launch_cases.py cannot drift from the library unnoticed: every restated constant and block-count rule is read back
from csrc/, every shape is in the regime it is in the table for with its neighbour on the other side of the cap, the input
conditions hold for every combination of lattice inputs, bins and ranges that tests/test_gpu_summary_launch_shapes.py uses, and
plant_edges puts its samples where numpy's histograms put them."""
import os
import re
import time

import numpy as np
import pytest

import summary_launch_cases as sl
from conftest import ROOT
from flow_compare_restatement import compare_restatement, make_result

CSRC = os.path.join(ROOT, "opticalflow_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_restated_constants_are_the_library_s():
    fc, cp, bz = source("vof_flowcompare.hpp"), source("vof_compare.hpp"), source("vof_blursweep.hpp")
    shared, pairs, frames = source("vof_shared.hpp"), source("vof_pairs.hip"), source("vof_frames.hip")
    for text, names in ((fc, ("FC_BLOCK", "FC_PER_LANE", "FC_MAX_BLOCKS", "FC_UNROLL")),
                        (cp, ("CP_PER_LANE", "CP_MAX_BLOCKS")), (shared, ("CP_LDS_JOINT", "CP_MAX_THETA_BINS", "CP_MAX_SPEED_BINS")),
                        (bz, ("BZ_ANGLE_PER_LANE", "BZ_ANGLE_MAX_BLOCKS", "BZ_MAX_ANGLE_BINS")), (shared, ("BS_LDS_BINS",)), (shared, ("RBLK",)),
                        (pairs, ("BS_MAX_CHUNK",)), (frames, ("PRE_MAX_FLIGHT",))):
        for name in names:
            assert constant(text, name) == getattr(sl, name), name


def test_restated_block_rules_are_the_library_s():
    fc, cp, hip = source("vof_flowcompare.hpp"), source("vof_compare.hpp"), source("vof_pairs.hip") + source("vof_frames.hip")
    # fc_blocks, cp_blocks: fs / (lanes * PER_LANE), at least 1, at most MAX_BLOCKS
    assert re.search(r"inline int fc_blocks\(size_t fs\) \{[^}]*fs / \(\(size_t\)FC_BLOCK \* FC_PER_LANE\);\s*"
                     r"return n < 1 \? 1 : \(n > \(size_t\)FC_MAX_BLOCKS \? FC_MAX_BLOCKS : \(int\)n\);", fc)
    assert re.search(r"inline int cp_blocks\(size_t fs\) \{[^}]*fs / \(64 \* CP_PER_LANE\);\s*"
                     r"return n < 1 \? 1 : \(n > \(size_t\)CP_MAX_BLOCKS \? CP_MAX_BLOCKS : \(int\)n\);", cp)
    # the direction histogram's
    assert re.search(r"blk = \(int\)std::min<size_t>\(BZ_ANGLE_MAX_BLOCKS, std::max<size_t>\(1, fs / \(64 \* BZ_ANGLE_PER_LANE\)\)\);", hip)
    m = re.search(r"inline int pair_moments_blocks\(size_t fs\) \{ return \(int\)std::min<size_t>\((\d+), std::max<size_t>\(1, "
                  r"\(fs \+ (\d+) \* RBLK - 1\) / \((\d+) \* RBLK\)\)\); \}", hip)
    assert m and [int(v) for v in m.groups()] == [sl.MOMENTS_MAX_BLOCKS, 4, 4]
    # the two k_bs_counts launches (the speed of a chunk, the blurred stack) and k_fc_mask's
    counts = re.findall(r"const int nb = \(int\)std::min<size_t>\((\d+), \(m \+ (\d+) \* (\d+) - 1\) / \((\d+) \* (\d+)\)\);", hip)
    assert len(counts) == 2 and all([int(v) for v in c] == [sl.COUNTS_MAX_BLOCKS, 4, 256, 4, 256] for c in counts)
    assert len(re.findall(r"k_bs_counts<<<nb, 256, 0, c->stream>>>", hip)) == 2
    m = re.search(r"const int blocks = \(int\)std::min<size_t>\((\d+), \(n \+ (\d+) \* FC_BLOCK - 1\) / \((\d+) \* FC_BLOCK\)\);", hip)
    assert m and [int(v) for v in m.groups()] == [sl.MASK_MAX_BLOCKS, 8, 8]
    # the fold of the extremes is one wave striding by 64 over blk * nf records; the sums of the direction blocks start at block 0
    assert re.search(r"for \(int i = threadIdx\.x; i < n; i \+= 64\) fc_merge\(e, part\[i\]\);", fc)
    assert re.search(r"k_fc_extremes_fold<<<1, 64, 0, c->stream>>>\(part, blk \* nf, acc\);", hip)
    # the values of the rules
    fs = sl.samples(sl.MID)
    assert (sl.fc_blocks(fs), sl.cp_blocks(fs), sl.direction_blocks(fs), sl.pair_moments_blocks(fs)) == (5, 21, 10, 22)
    assert [sl.fc_blocks(n) for n in (1, 4095, 8191, 8192, 256 * 4096, 10 ** 9)] == [1, 1, 1, 2, 256, 256]
    assert [sl.pair_moments_blocks(n) for n in (1, 1024, 1025, 256 * 1024, 256 * 1024 + 1)] == [1, 1, 2, 256, 256]
    assert [sl.counts_blocks(n) for n in (1, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1)] == [1, 1, 2, 1024, 1024]
    assert [sl.mask_blocks(n) for n in (1, 2048, 2049, 2048 * 2048 + 1)] == [1, 1, 2, 2048]


def test_every_shape_is_in_its_regime():
    n = {name: sl.samples(shape) for name, shape in sl.SHAPES.items()}
    assert n["MID"] == 21593 and n["MID"] % 64 != 0 and sl.MID_T == sl.MID[::-1]
    for shape in sl.SHAPES.values():
        assert shape[0] != shape[1]
    # MID: more than one block of every kernel, no cap; 16 pairs in flight are more extremes records than the fold's stride, and a
    # lane of k_fc_extremes / k_cp_joint runs out of samples inside its unrolled group (the tail of fc_for_each)
    assert 1 < sl.fc_blocks(n["MID"]) < sl.FC_MAX_BLOCKS and sl.fc_blocks(n["MID"]) * sl.PRE_MAX_FLIGHT > 64
    assert n["MID"] % (sl.fc_blocks(n["MID"]) * sl.FC_BLOCK * sl.FC_UNROLL) != 0
    assert 1 < sl.direction_blocks(n["MID"]) < sl.BZ_ANGLE_MAX_BLOCKS and 1 < sl.cp_blocks(n["MID"]) < sl.CP_MAX_BLOCKS
    assert 33 > sl.BS_MAX_CHUNK and 17 > sl.PRE_MAX_FLIGHT                      # the frame counts of the tests: 32 + 1 and 16 + 1
    # each cap with the shape one step below it
    for rule, cap, above, below in ((sl.cp_blocks, sl.CP_MAX_BLOCKS, "CP_CAP", "CP_BELOW"),
                                    (sl.pair_moments_blocks, sl.MOMENTS_MAX_BLOCKS, "CP_CAP", "CP_BELOW"),
                                    (sl.direction_blocks, sl.BZ_ANGLE_MAX_BLOCKS, "BZ_CAP", "BZ_BELOW"),
                                    (sl.fc_blocks, sl.FC_MAX_BLOCKS, "FC_CAP", "FC_BELOW")):
        assert sl.uncapped(rule, n[above]) in (cap + 1, cap + 2) and rule(n[above]) == cap, (rule.__name__, above)
        assert cap - 1 <= sl.uncapped(rule, n[below]) <= cap and rule(n[below]) == sl.uncapped(rule, n[below]), (rule.__name__, below)
    # k_bs_counts: two pairs or three frames at BZ_CAP (and at BZ_BELOW) are past 1024 blocks, one pair is not
    for name in ("BZ_CAP", "BZ_BELOW"):
        assert sl.uncapped(sl.counts_blocks, 2 * n[name]) > sl.COUNTS_MAX_BLOCKS and sl.uncapped(sl.counts_blocks, 3 * n[name]) > sl.COUNTS_MAX_BLOCKS
        assert sl.counts_blocks(n[name]) < sl.COUNTS_MAX_BLOCKS
    assert 1 < sl.counts_blocks(33 * n["MID"]) < sl.COUNTS_MAX_BLOCKS
    # k_fc_mask: four frames of FC_CAP are past 2048 blocks, one frame is not; 16 frames of MID are not
    assert sl.uncapped(sl.mask_blocks, 4 * n["FC_CAP"]) > sl.MASK_MAX_BLOCKS > sl.mask_blocks(n["FC_CAP"]) > 1
    assert 1 < sl.mask_blocks(16 * n["MID"]) < sl.MASK_MAX_BLOCKS


LATTICE_COMBOS = [dict(angle_bins=21), dict(joint_speed_bins=(64, 64), angle_bins=63), dict(joint_speed_bins=(64, 65), angle_bins=63),
                  dict(joint_speed_bins=(64, 64), angle_bins=63, joint_speed_ranges=((0, 6), (0, 6)), angle_range=(0, np.pi)),
                  dict(joint_speed_bins=(64, 65), angle_bins=63, joint_speed_ranges=((0, 6), (0, 6)), angle_range=(0, np.pi)),
                  dict(joint_speed_ranges=((0, 6), (0, 6)), angle_range=(0.5, 2.5), angle_edges=np.linspace(0.5, 2.5, 22))]


@pytest.mark.parametrize("name,pairs", [("MID", 17), ("FC_CAP", 2), ("FC_BELOW", 2)])
def test_input_conditions_hold_for_the_lattice_inputs(name, pairs):
    """Every (input, bins, ranges) combination of the GPU file with lattice inputs, at the small and at the large size: the set of
    thetas is the same 132 values, so the gaps are the same, far above 1e-9."""
    a, b = sl.lattice_results((pairs,) + sl.SHAPES[name], 51)
    combos = LATTICE_COMBOS if name == "MID" else LATTICE_COMBOS[:1]
    for quirks in (True, False):
        for kw in combos:
            figures, want = sl.launch_input_conditions(a, b, reference_quirks=quirks, **kw)
            gaps = [v for k, v in figures.items() if k.startswith(("theta", "speed"))]
            print(name, quirks, {k: v for k, v in kw.items() if k != "angle_edges"}, figures)
            assert figures["distinct_thetas"] == 132 and min(gaps) > 1e-6         # measured: 1.2e-5 (the range 0.5 .. 2.5) and up
            assert (figures["above_one"] > 0.002 * figures["m2"]) if quirks else figures["above_one"] == 0
    # an even number of angle bins puts pi / 4 and pi / 2 within an ulp of an edge: the condition rightly fails
    with pytest.raises(AssertionError):
        sl.launch_input_conditions(a, b, angle_bins=20, angle_range=(0, np.pi))
    # the planted stacks: everything but the planted speeds is held to the condition
    if name != "MID":
        pa, pb = sl.copy_of(a), sl.copy_of(b)
        edges = [np.histogram_bin_edges(np.zeros(0), n, range=(0, 6)) for n in sl.PLANTED_BINS]
        planted = sl.plant_edges(pa, pb, *edges)
        kw = dict(joint_speed_bins=sl.PLANTED_BINS, joint_speed_ranges=((0, 6), (0, 6)), angle_range=(0, np.pi), angle_bins=21)
        figures, _ = sl.launch_input_conditions(pa, pb, planted=planted, **kw)
        print(name, "planted", figures)
        with pytest.raises(AssertionError):
            sl.launch_input_conditions(pa, pb, **kw)                      # without the exception the planted speeds are found


def test_the_condition_on_unique_values_is_the_condition_on_all_values():
    """edge_gap against the N x edges matrix of flow_compare_restatement.input_conditions, on values near, on and between edges."""
    rng = np.random.default_rng(5)
    edges = np.linspace(0.0, 3.0, 22)
    values = np.concatenate([rng.uniform(-0.5, 3.5, 500), edges[3:6], edges[7:9] + 3e-10, edges[12:13] - 1e-12, [np.nan, np.inf]])
    finite = values[np.isfinite(values)]
    for outer in (False, True):
        e = edges if outer else edges[1:-1]
        d = np.abs(finite[:, None] - e[None, :])
        assert sl.edge_gap(values, edges, outer) == d[d > 0].min()
    assert sl.edge_gap(edges[1:-1], edges) == np.diff(edges).min() and sl.edge_gap(np.zeros(0), edges) == np.inf


def test_the_planted_bins_need_both_corrections_of_bs_bin_of():
    """bs_bin_of as it stands: the scaled index, then one step down against edges[idx], one step up against edges[idx + 1].  Of
    the planted samples some sit where the scaled index alone is one too low (on an edge) and some where it is one too high (one
    ulp below an edge): a kernel without either correction miscounts them."""
    bs = source("vof_shared.hpp")
    assert re.search(r"int idx = \(int\)\(\(\(x - first\) / \(last - first\)\) \* \(double\)bins\);\s*if \(idx == bins\) --idx;\s*"
                     r"if \(x < edges\[idx\]\) --idx;\s*if \(x >= edges\[idx \+ 1\] && idx != bins - 1\) \+\+idx;", bs)
    a, b = sl.lattice_results((2,) + sl.MID, 51)
    edges = [np.histogram_bin_edges(np.zeros(0), n, range=(0, 6)) for n in sl.PLANTED_BINS]
    planted = sl.plant_edges(a, b, *edges)
    needs_up, needs_down = [0, 0], [0, 0]
    for stack, pair, k, kind, index in planted:
        if kind in ("edge", "below"):
            s = (a, b)[stack]["speed"][pair].flat[k]
            true = int(np.searchsorted(edges[stack], s, side="right")) - 1
            assert true == (index if kind == "edge" else index - 1)
            guess = int(sl.scaled_index(s, edges[stack]))
            assert abs(guess - true) <= 1
            needs_up[stack] += guess < true
            needs_down[stack] += guess > true
    print("planted samples that need the upward correction:", needs_up, "the downward one:", needs_down)
    assert min(needs_up) >= 2 and needs_down[1] >= 2


@pytest.mark.parametrize("bins", [(50, 50), sl.PLANTED_BINS])
def test_plant_edges_puts_each_sample_where_numpy_puts_it(bins):
    a, b = sl.lattice_results((3,) + sl.MID, 51)
    before = (sl.copy_of(a), sl.copy_of(b))
    edges = [np.histogram_bin_edges(np.zeros(0), n, range=(0, 6)) for n in bins]
    planted = sl.plant_edges(a, b, edges[0], edges[1])
    kinds = {(stack, kind) for stack, _, _, kind, _ in planted}
    assert kinds == {(s, k) for s in (0, 1) for k in ("edge", "last", "outside", "below", "nan", "inf")}
    assert len(planted) >= 40 and {pair for _, pair, _, _, _ in planted} == {0, 2}
    fs, blocks = sl.samples(sl.MID), sl.fc_blocks(sl.samples(sl.MID))
    owners = {(k // sl.FC_BLOCK) % blocks for _, _, k, kind, _ in planted if kind not in ("nan", "inf")}
    assert {0, blocks // 2, blocks - 1} <= owners                                   # the first, a middle and the last block
    assert max(k for _, _, k, _, _ in planted) == fs - 1
    changed = np.zeros((3, fs), dtype=bool)
    for stack, pair, k, kind, index in planted:
        assert not changed[pair, k]
        changed[pair, k] = True
        mine, other = (a, b) if stack == 0 else (b, a)
        s, so = mine["speed"][pair].flat[k], other["speed"][pair].flat[k]
        if kind in ("nan", "inf"):
            assert np.isnan(s) if kind == "nan" else s == np.inf
            continue
        assert s == np.sqrt(mine["v_x"][pair].flat[k] ** 2 + mine["v_y"][pair].flat[k] ** 2) and so == 5.0
        pair_of = (np.array([s]), np.array([so])) if stack == 0 else (np.array([so]), np.array([s]))
        counts = np.histogram2d(*pair_of, bins=bins, range=((0, 6), (0, 6)))[0]
        one = np.histogram(np.array([s]), bins[stack], (0, 6))[0]
        n = bins[stack]
        where = {"edge": index, "last": n - 1, "below": index - 1, "outside": None}[kind]
        if where is None:
            assert counts.sum() == 0 and one.sum() == 0 and s > 6.0                # one ulp outside: dropped
        else:
            assert counts.sum() == 1 and one[where] == 1                           # on an edge: the bin it opens; the last edge counts
            assert counts.sum(axis=1 - stack)[where] == 1
    for r, r0 in zip((a, b), before):                                              # nothing else was touched
        for key in r:
            same = (r[key] == r0[key]) | (np.isnan(r[key]) & np.isnan(r0[key]))
            assert same.reshape(3, fs)[~changed].all(), key


def test_the_restatements_at_mid_are_quick():
    a, b = sl.lattice_results((17,) + sl.MID, 51)
    start = time.perf_counter()
    sl.launch_input_conditions(a, b)
    compare_restatement(a, b, angle_bins=21)
    took = time.perf_counter() - start
    print(f"condition and restatement at 17 x 143 x 151: {took:.2f} s")
    assert took < 1.0


@pytest.mark.parametrize("quirks", [True, False])
def test_the_continuous_inputs_meet_the_condition_and_hold_their_extremes_late(quirks):
    a, b, records = sl.continuous_results(17)
    assert len(set(records)) == 3 and min(records) >= 64
    figures, want = sl.launch_input_conditions(a, b, angle_bins=sl.CP_MAX_THETA_BINS, joint_speed_bins=(64, 65), reference_quirks=quirks)
    print(figures)
    low = np.nextafter(0.1, np.inf)
    assert np.array_equal(want["speed_extremes"], [[low, 12.0], [low, 13.0]]) and np.array_equal(want["cos_extremes"], [-1.0, 1.0])
    # each extreme is held by one sample only: without the planted pairs every extreme is another
    fewer = compare_restatement({k: v[:13] for k, v in a.items()}, {k: v[:13] for k, v in b.items()}, reference_quirks=quirks)
    assert not (fewer["speed_extremes"] == want["speed_extremes"]).any() and not (fewer["cos_extremes"] == want["cos_extremes"]).any()
