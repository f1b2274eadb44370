"""numpy restatement of ``filter_PIV_flow_result`` and ``compare_flow_results``, written from their description: whole stacks,
``np.histogram2d``, ``np.histogram`` and ``np.arccos``; the blurred movie is an argument (the blur has its own tests).  Shared
by tests/test_flow_compare_cpu.py and tests/test_gpu_flow_compare.py; it is what a user does on the host today."""
import numpy as np

SHAPE = (3, 40, 52)


def make_result(v_x, v_y):
    with np.errstate(invalid="ignore", over="ignore"):
        return dict(v_x=np.ascontiguousarray(v_x), v_y=np.ascontiguousarray(v_y), speed=np.sqrt(v_x ** 2 + v_y ** 2))


def inputs_a():
    """The pair of results (A) of the issue: b is correlated with a; five NaN speeds in a, one infinite in b, four zero vectors in a."""
    va = np.random.default_rng(46).normal(0, 1, (2,) + SHAPE)
    vb = 0.6 * va + 0.8 * np.random.default_rng(47).normal(0, 1, (2,) + SHAPE)
    a, b = make_result(va[0], va[1]), make_result(vb[0], vb[1])
    a["speed"][0, 0, :5] = a["v_x"][0, 0, :5] = np.nan
    b["speed"][1, 3, 7] = b["v_x"][1, 3, 7] = np.inf
    for key in ("v_x", "v_y", "speed"):
        a[key][2, 5, :4] = 0.0
    return a, b


def negated(result):
    return dict(v_x=-result["v_x"], v_y=-result["v_y"], speed=result["speed"].copy())


def filter_inputs():
    """The filter's movie (uint8, T = 4) and result (T - 1 pairs; one NaN and one +inf speed) of the issue."""
    movie = np.random.default_rng(48).integers(0, 256, (SHAPE[0] + 1,) + SHAPE[1:]).astype(np.uint8)
    v = np.random.default_rng(49).normal(0, 4, (2,) + SHAPE)
    result = make_result(v[0], v[1])
    result["speed"][0, 1, 2] = np.nan
    result["speed"][2, 30, 40] = np.inf
    result["original_data"] = movie
    return result


def filter_restatement(result, blurred, intensity_threshold=10, speed_threshold=7, reference_quirks=True):
    """``(v_x, v_y, speed, low, fast)`` after the filter; ``blurred`` is ``blur_movie(original_data, 3)`` (its first frames are used)."""
    v_x, v_y, speed = (result[k].copy() for k in ("v_x", "v_y", "speed"))
    with np.errstate(invalid="ignore"):
        low = blurred[:speed.shape[0]] < intensity_threshold
        fast = speed > (7 if reference_quirks else speed_threshold)
    v_x[low] = 0.0
    v_y[low] = 0.0
    v_x[fast] = 0.0
    v_y[fast] = 0.0
    speed[fast] = 0.0
    if not reference_quirks:
        speed[low] = 0.0
    return v_x, v_y, speed, low, fast


def sample_values(a, b, speed_threshold=0.1, angle_threshold=0.5, reference_quirks=True):
    """``(sa, sb, cos, theta, m1, m2, infinite)`` of every sample, in the order the description gives."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sa = np.where(np.isnan(a["speed"]), 0.0, a["speed"])
        sb = np.where(np.isnan(b["speed"]), 0.0, b["speed"])
        infinite = np.isinf(sa) | np.isinf(sb)
        m1 = ~infinite & (sa > speed_threshold) & (sb > speed_threshold)
        dot = b["v_x"] * a["v_x"] + b["v_y"] * a["v_y"]
        w = sb * sa
        cos = dot / w
        if not reference_quirks:
            cos = np.where(cos > 1.0, 1.0, np.where(cos < -1.0, -1.0, cos))
        theta = np.arccos(cos)
        m2 = ~infinite & (sa > angle_threshold) & (sb > angle_threshold)
    return sa, sb, cos, theta, m1, m2, infinite


def extremes_of(x):
    return [x.min(), x.max()] if x.size else [np.nan, np.nan]


def compare_restatement(a, b, speed_threshold=0.1, angle_threshold=0.5, joint_speed_bins=(50, 50), joint_speed_ranges=None,
                        angle_bins=20, angle_range=None, ground_truth=None, reference_quirks=True):
    sa, sb, cos, theta, m1, m2, infinite = sample_values(a, b, speed_threshold, angle_threshold, reference_quirks)
    kept = m2 & ~np.isnan(theta)
    ranges = [None, None] if joint_speed_ranges is None else list(joint_speed_ranges)
    joint, edges_a, edges_b = np.histogram2d(sa[m1], sb[m1], bins=joint_speed_bins, range=ranges)
    angles, angle_edges = np.histogram(theta[kept], bins=angle_bins, range=angle_range)
    first_pass = angle_range is None or any(r is None for r in ranges)
    nothing = [np.nan, np.nan]
    out = dict(joint_speed_histogram=joint.astype(np.int64), joint_speed_edges_a=edges_a, joint_speed_edges_b=edges_b,
               angle_histogram=angles.astype(np.int64), angle_edges=angle_edges,
               nan_speed_counts=np.array([np.isnan(a["speed"]).sum(), np.isnan(b["speed"]).sum()], dtype=np.int64),
               infinite_count=int(infinite.sum()), joint_count=int(m1.sum()), angle_count=int(kept.sum()),
               angle_dropped=int((m2 & ~kept).sum()),
               speed_extremes=np.array([extremes_of(sa[m1]), extremes_of(sb[m1])] if first_pass else [nothing, nothing]),
               cos_extremes=np.array(extremes_of(cos[kept]) if first_pass else nothing))
    if ground_truth is not None:
        frame, start, end = ground_truth
        start, end = np.asarray(start), np.asarray(end)
        dx, dy = (end - start)[:, 0], (end - start)[:, 1]
        errors = []
        for r in (a, b):
            v_x, v_y = r["v_x"][frame, start[:, 0], start[:, 1]], r["v_y"][frame, start[:, 0], start[:, 1]]
            errors.append(np.sqrt(np.power(dy - v_y, 2) + np.power(dx - v_x, 2)) / np.sqrt(np.power(dy, 2) + np.power(dx, 2)))
        out["relative_errors"] = np.array(errors)
    return out


def input_conditions(a, b, speed_threshold, angle_threshold, reference_quirks=True, joint_speed_bins=(50, 50), angle_bins=20,
                     joint_speed_ranges=None, angle_range=None):
    """What the exact comparison with the device rests on, for the edges of the given bins and ranges, asserted on the inputs
    alone; returns the figures it found.  No numpy
    theta and no speed lies within 1e-9 of an interior edge unless exactly on it (the device's acos may differ from np.arccos in
    its last bits), and np.arccos is monotone where it matters: the extremes of theta are the arccos of the extremes of cos."""
    sa, sb, cos, theta, m1, m2, _ = sample_values(a, b, speed_threshold, angle_threshold, reference_quirks)
    kept = m2 & ~np.isnan(theta)
    want = compare_restatement(a, b, speed_threshold, angle_threshold, joint_speed_bins, joint_speed_ranges, angle_bins, angle_range, None,
                               reference_quirks)

    def gap(values, edges):
        d = np.abs(values[:, None] - edges[None, 1:-1])
        return d[d > 0].min() if (d > 0).any() else np.inf
    gaps = dict(theta=gap(theta[kept], want["angle_edges"]), speed_a=gap(sa[m1], want["joint_speed_edges_a"]),
                speed_b=gap(sb[m1], want["joint_speed_edges_b"]))
    assert min(gaps.values()) > 1e-9, gaps
    assert theta[kept].min() == np.arccos(cos[kept].max()) and theta[kept].max() == np.arccos(cos[kept].min())
    with np.errstate(invalid="ignore"):
        above_one = int((m2 & (np.abs(cos) > 1.0)).sum())
    return dict(gaps, m1=int(m1.sum()), m2=int(m2.sum()), above_one=above_one,
                angle_bins_occupied=int((want["angle_histogram"] > 0).sum()))
