"""Numpy restatement of the statistics of compare_channel_flows.  Test infrastructure only.

``compare_summaries`` takes the result dicts of two ``conduct_optical_flow`` calls (anything with ``v_x``, ``v_y`` and ``speed``
of one shape) and the bin arguments of ``compare_channel_flows`` and returns every per-channel and joint summary of that
function, computed with ``np.histogram``, ``np.histogram2d`` and ``np.arccos`` on the whole stacks."""
import numpy as np

PER_CHANNEL = ("speed_means", "speed_stds", "nonfinite_counts", "speed_histograms", "angle_histograms", "weighted_angle_histograms")


def direction(flow):
    """The flow direction to the y axis in units of pi, sign(0) = 0; NaN where the speed is 0 or not finite."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.arccos(flow["v_y"] / flow["speed"]) * np.sign(flow["v_x"]) / np.pi


def relative_angle(flow_a, flow_b, reference_quirks=True):
    """``(theta, w)`` of every sample: the angle between the two flows in units of pi and the product of the speeds."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dot = flow_a["v_x"] * flow_b["v_x"] + flow_a["v_y"] * flow_b["v_y"]
        w = flow_a["speed"] * flow_b["speed"]
        cos = dot / w
        if not reference_quirks:
            cos = np.clip(cos, -1.0, 1.0)                    # NaN stays NaN
        return np.arccos(cos) / np.pi, w


def compare_summaries(flow_a, flow_b, histogram_bins=None, histogram_range=None, angle_bins=None, relative_angle_bins=50,
                      joint_speed_bins=None, joint_speed_ranges=None, joint_speed_min_b=None, reference_quirks=True):
    flows = [{k: np.asarray(f[k], dtype=np.float64) for k in ("v_x", "v_y", "speed")} for f in (flow_a, flow_b)]
    out = {k: [] for k in PER_CHANNEL}
    for f in flows:
        speed = f["speed"]
        with np.errstate(invalid="ignore"):
            out["speed_means"].append(np.mean(speed))
            out["speed_stds"].append(np.std(speed))
        out["nonfinite_counts"].append(int((~np.isfinite(speed)).sum()))
        if histogram_bins is not None:
            out["speed_histograms"].append(np.histogram(speed.ravel(), histogram_bins, histogram_range)[0])
        if angle_bins is not None:
            ok = np.isfinite(speed)                          # a sample whose speed is not finite counts nowhere
            a, weight = direction(f)[ok], speed[ok]
            a, weight = a[~np.isnan(a)], weight[~np.isnan(a)]
            out["angle_histograms"].append(np.histogram(a, angle_bins, (-1, 1))[0])
            out["weighted_angle_histograms"].append(np.histogram(a, angle_bins, (-1, 1), weights=weight)[0])
    out = {k: np.asarray(v) for k, v in out.items() if v}
    if angle_bins is not None:
        out["angle_edges"] = np.linspace(-1.0, 1.0, angle_bins + 1)
    if histogram_bins is not None:
        out["histogram_edges"] = np.linspace(histogram_range[0], histogram_range[1], histogram_bins + 1)

    both = np.isfinite(flows[0]["speed"]) & np.isfinite(flows[1]["speed"])
    theta, w = relative_angle(flows[0], flows[1], reference_quirks)
    theta, w = theta[both], w[both]
    kept = ~np.isnan(theta)
    out["joint_nonfinite_count"] = int((~both).sum())
    out["relative_angle_dropped"] = int((~kept).sum())
    out["relative_angle_histogram"], edges = np.histogram(theta[kept], relative_angle_bins, (0, 1))
    out["weighted_relative_angle_histogram"] = np.histogram(theta[kept], relative_angle_bins, (0, 1), weights=w[kept])[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["weighted_relative_angle_density"] = np.histogram(theta[kept], relative_angle_bins, (0, 1), weights=w[kept], density=True)[0]
    out["relative_angle_edges"] = edges
    if joint_speed_bins is not None:
        sa, sb = flows[0]["speed"].ravel(), flows[1]["speed"].ravel()
        with np.errstate(invalid="ignore"):
            m = np.ones(sb.shape, dtype=bool) if joint_speed_min_b is None else sb > joint_speed_min_b
        counts, ea, eb = np.histogram2d(sa[m], sb[m], joint_speed_bins, joint_speed_ranges)
        out["joint_speed_histogram"] = counts.astype(np.int64)
        out["joint_speed_edges_a"], out["joint_speed_edges_b"] = ea, eb
    return out
