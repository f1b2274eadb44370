"""The shapes and inputs of tests/test_gpu_summary_launch_shapes.py: the summary kernels (k_fc_*, k_cp_joint, k_bz_angles, k_bs_counts,
k_bs_moments) at launches of more than one block per pair, at their block caps and over more pairs than a launch holds.
tests/test_summary_launch_cases_cpu.py keeps the restated constants and block-count rules the library's, so that a change of one
fails there instead of silently moving the shapes off the edges.  Plain Python, no GPU."""
import numpy as np

from flow_compare_restatement import compare_restatement, make_result, sample_values

# csrc/vof_flowcompare.hpp
FC_BLOCK = 256            # threads of a block of k_fc_mask / k_fc_extremes / k_fc_histograms
FC_PER_LANE = 16          # samples a lane takes at least before a plane gets another block
FC_MAX_BLOCKS = 256       # blocks per pair at most
FC_UNROLL = 4
# csrc/vof_compare.hpp
CP_PER_LANE = 16
CP_MAX_BLOCKS = 256
# csrc/vof_shared.hpp
CP_LDS_JOINT = 4096       # 2-D counters that are counted in LDS first
CP_MAX_THETA_BINS = 64
CP_MAX_SPEED_BINS = 1024
# csrc/vof_blursweep.hpp
BZ_ANGLE_PER_LANE = 32
BZ_ANGLE_MAX_BLOCKS = 256
BZ_MAX_ANGLE_BINS = 128
# csrc/vof_shared.hpp, csrc/vof_pairs.hip, csrc/vof_frames.hip
BS_LDS_BINS = 1024        # k_bs_counts: more bins go to global atomics
RBLK = 256                # threads of a reduction block
BS_MAX_CHUNK = 32         # pairs per launch of a sweep at most
PRE_MAX_FLIGHT = 16       # units in flight of a frame-chunk walk when the caller leaves the number to the library
MOMENTS_MAX_BLOCKS = 256  # pair_moments_blocks
COUNTS_MAX_BLOCKS = 1024  # the two k_bs_counts launches
MASK_MAX_BLOCKS = 2048    # k_fc_mask


def _clamp(n, most):
    return max(1, min(most, n))


def fc_blocks(fs):
    """Blocks per pair of k_fc_extremes / k_fc_histograms (fc_blocks of vof_flowcompare.hpp)."""
    return _clamp(fs // (FC_BLOCK * FC_PER_LANE), FC_MAX_BLOCKS)


def cp_blocks(fs):
    """One-wave blocks per pair of k_cp_joint (cp_blocks of vof_compare.hpp)."""
    return _clamp(fs // (64 * CP_PER_LANE), CP_MAX_BLOCKS)


def direction_blocks(fs):
    """One-wave blocks per pair of k_bz_angles (DirectionHist::regions)."""
    return _clamp(fs // (64 * BZ_ANGLE_PER_LANE), BZ_ANGLE_MAX_BLOCKS)


def pair_moments_blocks(fs):
    """Blocks per pair of k_bs_moments."""
    return _clamp(-(-fs // (4 * RBLK)), MOMENTS_MAX_BLOCKS)


def counts_blocks(m):
    """Blocks of a k_bs_counts launch over m samples (the speed of the pairs of a chunk, or the blurred stack)."""
    return min(COUNTS_MAX_BLOCKS, -(-m // (4 * 256)))


def mask_blocks(n):
    """Blocks of a k_fc_mask launch over the n samples of the frames in flight."""
    return min(MASK_MAX_BLOCKS, -(-n // (8 * FC_BLOCK)))


def uncapped(rule, fs):
    """What a block-count rule would give without its cap."""
    return {fc_blocks: fs // (FC_BLOCK * FC_PER_LANE), cp_blocks: fs // (64 * CP_PER_LANE), direction_blocks: fs // (64 * BZ_ANGLE_PER_LANE),
            pair_moments_blocks: -(-fs // (4 * RBLK)), counts_blocks: -(-fs // 1024), mask_blocks: -(-fs // (8 * FC_BLOCK))}[rule]


# (N_i, N_j): the smallest planes that reach each regime, odd-sized where the regime allows, N_i != N_j, no multiple of 64 samples.
MID = (143, 151)          # 21 593 samples: 5 fc, 21 cp, 10 direction, 22 moment blocks; 16 pairs are 80 extremes records
MID_T = (151, 143)
CP_CAP = (513, 514)       # 263 682: cp_blocks 257 and pair_moments_blocks 258, both capped at 256
CP_BELOW = (511, 513)     # 262 143: 255 cp blocks and 256 moment blocks, neither capped
BZ_CAP = (726, 727)       # 527 802: 257 direction blocks capped at 256; two pairs or three frames are > 1024 k_bs_counts blocks
BZ_BELOW = (723, 727)     # 525 621: 256 direction blocks, not capped
FC_CAP = (1026, 1027)     # 1 053 702: 257 fc blocks capped at 256; four units are > 2048 k_fc_mask blocks
FC_BELOW = (1023, 1025)   # 1 048 575: 255 fc blocks
SHAPES = dict(MID=MID, MID_T=MID_T, CP_CAP=CP_CAP, CP_BELOW=CP_BELOW, BZ_CAP=BZ_CAP, BZ_BELOW=BZ_BELOW, FC_CAP=FC_CAP, FC_BELOW=FC_BELOW)


def samples(shape):
    return shape[-2] * shape[-1]


# ---- inputs of compare_flow_results at any size -------------------------------------------------------------------------------
def lattice_results(shape, seed, hi=4):
    """Two results of shape (P, N_i, N_j) whose velocities are integers of -hi .. hi as float64, speed = sqrt(v_x^2 + v_y^2) as
    flow_compare_restatement.make_result forms it.  theta then takes a finite set of values whatever the plane size (132 with
    hi = 4), so the distance of the thetas and of the speeds to the bin edges does not shrink with the number of samples.  About
    0.4 % of the samples have cos > 1 by rounding: what reference_quirks drops."""
    v = np.random.default_rng(seed).integers(-hi, hi + 1, (4,) + tuple(shape)).astype(np.float64)
    return make_result(v[0], v[1]), make_result(v[2], v[3])


def continuous_results(pairs=17):
    """Two results of normal velocities at MID (inputs (A) of tests/test_gpu_flow_compare.py at this size) whose six extremes -
    the smallest and the largest speed of a and of b among the samples above the thresholds, cos = 1 and cos = -1 exactly - are
    single planted samples in the last block of the pairs 13, 14 and 15: with 5 blocks per pair and 16 pairs in a launch those are
    the records 69, 74 and 79 of k_fc_extremes, past the first stride of the fold.  Returns (a, b, records of the plants)."""
    assert pairs >= 16
    shape = (pairs,) + MID
    va = np.random.default_rng(46).normal(0, 1, (2,) + shape)
    vb = 0.6 * va + 0.8 * np.random.default_rng(47).normal(0, 1, (2,) + shape)
    low = np.nextafter(0.1, np.inf)                          # the smallest speed above the default speed_threshold
    fs, blocks = samples(MID), fc_blocks(samples(MID))
    plants = [(13, 9, (low, 0.0), (0.0, 2.0)), (14, 9, (0.0, 2.0), (low, 0.0)), (15, 9, (12.0, 0.0), (0.0, 3.0)), (15, 11, (0.0, 3.0), (13.0, 0.0)),
              (14, 11, (3.0, 4.0), (6.0, 8.0)), (13, 11, (3.0, 4.0), (-6.0, -8.0))]
    records = []
    for pair, lane, at_a, at_b in plants:
        k = (blocks - 1) * FC_BLOCK + lane
        i, j = divmod(k, MID[1])
        va[0][pair, i, j], va[1][pair, i, j] = at_a
        vb[0][pair, i, j], vb[1][pair, i, j] = at_b
        records.append(pair * blocks + (k // FC_BLOCK) % blocks)
    return make_result(va[0], va[1]), make_result(vb[0], vb[1]), records


def copy_of(result):
    return {k: np.array(v) for k, v in result.items()}


def edge_gap(values, edges, outer=False):
    """The smallest distance > 0 between a value and an interior edge (with `outer`: any edge), found on np.unique(values) with
    searchsorted; inf if there is none.  A value exactly on an edge is allowed: numpy and the device agree on it."""
    u = np.unique(values[np.isfinite(values)])
    e = np.asarray(edges if outer else edges[1:-1], dtype=np.float64)
    if u.size == 0 or e.size == 0:
        return np.inf
    at = np.searchsorted(e, u)
    best = np.inf
    for shift in (-1, 0, 1):
        i = at + shift
        ok = (i >= 0) & (i < e.size)
        d = np.abs(u[ok] - e[i[ok]])
        d = d[d > 0]
        if d.size:
            best = min(best, float(d.min()))
    return best


GAP_BOUND = 1e-9          # the bound of flow_compare_restatement.input_conditions, unchanged


def launch_input_conditions(a, b, speed_threshold=0.1, angle_threshold=0.5, reference_quirks=True, joint_speed_bins=(50, 50),
                            angle_bins=21, joint_speed_ranges=None, angle_range=None, angle_edges=None, planted=()):
    """flow_compare_restatement.input_conditions for stacks of any size: the same condition - no numpy theta and no speed within
    1e-9 of an interior edge unless exactly on it, np.arccos monotone at the extremes - asserted on the unique values.  With
    `angle_edges` (an explicit edge vector whose outer edges drop or clamp samples) the outer angle edges are held to it too.
    `planted`: the records of plant_edges; the speeds of those samples are one ulp from an edge on purpose (the device reads a
    speed, it does not compute it, so its bin is numpy's for every double) and are the one exception from the speed condition -
    their thetas are held to the condition like all others, and every one of them is compared.
    Returns (figures, the restatement's result).  A condition on the inputs, never a reason to drop a sample."""
    sa, sb, cos, theta, m1, m2, _ = sample_values(a, b, speed_threshold, angle_threshold, reference_quirks)
    kept = m2 & ~np.isnan(theta)
    want = compare_restatement(a, b, speed_threshold, angle_threshold, joint_speed_bins, joint_speed_ranges, angle_bins, angle_range, None,
                               reference_quirks)
    drawn = np.ones(sa.shape, dtype=bool)
    for _stack, pair, k, _kind, _index in planted:
        drawn[pair].flat[k] = False
    gaps = dict(theta=edge_gap(theta[kept], want["angle_edges"]), speed_a=edge_gap(sa[m1 & drawn], want["joint_speed_edges_a"]),
                speed_b=edge_gap(sb[m1 & drawn], want["joint_speed_edges_b"]))
    if angle_edges is not None:
        gaps["theta_given"] = edge_gap(theta[kept], angle_edges, outer=True)
    assert min(gaps.values()) > GAP_BOUND, gaps
    assert theta[kept].min() == np.arccos(cos[kept].max()) and theta[kept].max() == np.arccos(cos[kept].min())
    with np.errstate(invalid="ignore"):
        above_one = int((m2 & (np.abs(cos) > 1.0)).sum())
    figures = dict(gaps, m1=int(m1.sum()), m2=int(m2.sum()), above_one=above_one, distinct_thetas=int(np.unique(theta[kept]).size),
                   angle_bins_occupied=int((want["angle_histogram"] > 0).sum()))
    return figures, want


def block_positions(fs, blocks, block=FC_BLOCK, stack=0):
    """Plane indices in the first, a middle and the last block's samples of a launch of `blocks` blocks of `block` lanes (block x
    takes the samples x * block + lane, + blocks * block, ...), and the last samples of the plane (the unroll tail).  The two
    stacks get neighbouring samples, never the same one."""
    first = [0, 2, block - 2]
    mid = [(blocks // 2) * block + 4, (blocks // 2) * block + blocks * block + 6]
    last = [(blocks - 1) * block + 8, (blocks - 1) * block + block - 2]
    tail = [fs - 1 - stack, fs - 3 - stack, fs - block - 1 - stack]
    return [k for k in [e + stack for e in first + mid + last] + tail if 0 <= k < fs]


PLANTED_BINS = (50, 65)   # the joint bins of the planted case over (0, 6): both correction branches of bs_bin_of decide bins


def scaled_index(x, edges):
    """The first guess of bs_bin_of (vof_shared.hpp) for values inside the range: ((x - first) / (last - first)) * bins in
    float64, truncated.  bs_bin_of then corrects it against the two neighbouring edges."""
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.size - 1
    return np.minimum((((np.asarray(x, dtype=np.float64) - edges[0]) / (edges[-1] - edges[0])) * float(bins)).astype(np.int64), bins - 1)


def corrected_edges(edges):
    """(up, down): the interior edges i for which a sample exactly on the edge gets the first guess i - 1 and needs the
    `x >= edges[idx + 1]` correction of bs_bin_of, and those for which a sample one ulp below the edge gets the guess i and needs
    the `x < edges[idx]` correction."""
    edges = np.asarray(edges, dtype=np.float64)
    i = np.arange(1, edges.size - 1)
    up = i[scaled_index(edges[1:-1], edges) < i]
    down = i[scaled_index(np.nextafter(edges[1:-1], -np.inf), edges) >= i]
    return up.tolist(), down.tolist()


def plant_edges(a, b, edges_a, edges_b, partner=(3.0, 4.0)):
    """Overwrites a few dozen samples of the two results (in place) in the first, a middle and the last block's index ranges of
    the first and the last pair with speeds exactly on interior edges of `edges_a` / `edges_b`, on the last edge, one ulp outside
    the last edge and one ulp below an interior edge, and one NaN and one +inf speed per stack.  Among the interior edges are those
    of corrected_edges, where the scaled index alone is off by one and a correction branch of bs_bin_of decides (with 50 bins over
    (0, 6) only the upward one occurs, with 65 both).  A planted speed s has the velocity
    (s, 0), so that sqrt(v_x^2 + v_y^2) is s; the other result holds `partner` there (speed 5 by default, which must lie inside
    its range).  Returns the records (stack, pair, plane index, kind, edge index): kind is "edge" (bin = edge index), "last"
    (bin = bins - 1), "outside" (no bin), "below" (bin = edge index - 1), "nan" or "inf"."""
    P, n_i, n_j = a["speed"].shape
    fs = n_i * n_j
    records, taken = [], set()
    for stack, (mine, other, edges) in enumerate(((a, b, edges_a), (b, a, edges_b))):
        bins = len(edges) - 1
        up, down = corrected_edges(edges)
        values = [("edge", i, edges[i]) for i in sorted({1, bins // 2, bins - 1} | set(up[:2]))]
        values += [("last", bins, edges[bins]), ("outside", bins, np.nextafter(edges[bins], np.inf))]
        values += [("below", i, np.nextafter(edges[i], -np.inf)) for i in sorted({bins // 2} | set(down[:2]))]
        for pair in sorted({0, P - 1}):
            for n, k in enumerate(block_positions(fs, fc_blocks(fs), stack=stack)):
                if (pair, k) in taken:
                    continue
                taken.add((pair, k))
                kind, index, s = values[(n + pair + stack) % len(values)]
                i, j = divmod(k, n_j)
                mine["v_x"][pair, i, j], mine["v_y"][pair, i, j], mine["speed"][pair, i, j] = s, 0.0, s
                other["v_x"][pair, i, j], other["v_y"][pair, i, j] = partner
                other["speed"][pair, i, j] = np.sqrt(partner[0] ** 2 + partner[1] ** 2)
                records.append((stack, pair, k, kind, index))
        # one NaN and one +inf speed per stack, in the middle of the plane of the last pair
        for kind, value, k in (("nan", np.nan, fs // 2 + 11 + 2 * stack), ("inf", np.inf, fs // 3 + 17 + 2 * stack)):
            i, j = divmod(k, n_j)
            mine["speed"][P - 1, i, j] = value
            records.append((stack, P - 1, k, kind, -1))
    return records


# ---- movies of the box-flow sweeps --------------------------------------------------------------------------------------------
def random_movie(shape, frames, seed):
    """`frames` random 8-bit frames (input (B) of tests/test_gpu_blursweep.py at any size): every speed of the box flow is finite
    and the directions fill [-1, 1]."""
    movie = np.random.default_rng(seed).integers(0, 256, (frames,) + tuple(shape)).astype(np.uint8)
    movie.setflags(write=False)
    return movie


def moments_field(n, seed=0):
    """n doubles of mean 1e6 and unit variance (test_field_moments_are_accurate_with_a_large_offset at any size)."""
    return 1e6 + np.random.default_rng(seed).standard_normal(n)
