"""numpy restatement of ``downsample_movie`` as the GPU has to compute it, bit for bit: OpenCV 4's ``cv2.resize(frame,
dsize=(n_j, n_i), interpolation=cv2.INTER_AREA)`` of one channel when neither axis is enlarged (``resize.cpp``), per frame.

Per axis, in float64, with ``ssize`` the input and ``dsize`` the output size: ``inv = dsize / ssize``, ``scale = 1.0 / inv``,
``iscale = int(scale)``.  ``fast = |scale_x - iscale_x| < DBL_EPSILON and |scale_y - iscale_y| < DBL_EPSILON``.

General path (``resizeArea_``): the table of an axis (``computeResizeAreaTab``) holds, for ``d = 0 .. dsize - 1`` with
``f1 = d * scale``, ``f2 = f1 + scale``, ``cw = min(scale, ssize - f1)``, ``s1 = ceil(f1)``, ``s2 = min(floor(f2), ssize - 1)``,
``s1 = min(s1, s2)``, the entries
    (s1 - 1, float32((s1 - f1) / cw))                      if s1 - f1 > 1e-3
    (s, float32(1.0 / cw))                                 for s = s1 .. s2 - 1
    (s2, float32(min(min(f2 - s2, 1.0), cw) / cw))         if f2 - s2 > 1e-3
in this order.  The working type WT is float32 for uint8 frames and float64 for float64 frames (a weight is promoted).  Output
pixel (dy, dx): for the rows (r, beta) of ytab[dy] in order, ``buf = 0`` and ``buf = buf + S[r][c] * alpha`` for the entries
(c, alpha) of xtab[dx] in order, every product and every sum rounded on its own in WT; the first row sets ``sum = beta * buf``,
every later one ``sum = sum + beta * buf``.  float64: ``sum``; uint8: ``saturate_u8(rint(sum))``, half to even.

Fast path (``resizeAreaFast_``): ``area = iscale_x * iscale_y``, ``scale_f = float32(1) / float32(area)``.
    uint8, 2 x 2:    (S00 + S01 + S10 + S11 + 2) >> 2                                   (half up)
    uint8 otherwise: saturate_u8(rint(float32(integer sum) * scale_f))                  (half to even)
    float64:         the samples in row-major order k = sy * iscale_x + sx; while k <= area - 4:
                     sum += ((S[k] + S[k+1]) + S[k+2]) + S[k+3]; the rest one by one; result sum * float64(scale_f)

The result is float64 in both depths (the reference's scripts store it into a float64 array).  ``exact_area_mean`` is the
overlap-weighted mean written down directly in float64, independent of the tables.
"""
import math

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)


def axis_scale(ssize, dsize):
    """(scale, iscale) of one axis, OpenCV's two roundings kept: inv = dsize / ssize, scale = 1.0 / inv."""
    inv = float(dsize) / float(ssize)
    scale = 1.0 / inv
    return scale, int(scale)


def axis_table(ssize, dsize):
    """The entries of every output index of one axis: a list of (source indices int64, weights float32), and the intermediate
    values (f1, f2, cw, s1, s2, head kept, tail kept) per output index."""
    scale, _ = axis_scale(ssize, dsize)
    entries, detail = [], []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cw = min(scale, ssize - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        idx, w = [], []
        head = s1 - f1 > 1e-3
        if head:
            idx.append(s1 - 1)
            w.append(np.float32((s1 - f1) / cw))
        for s in range(s1, s2):
            idx.append(s)
            w.append(np.float32(1.0 / cw))
        tail = f2 - s2 > 1e-3
        if tail:
            idx.append(s2)
            w.append(np.float32(min(min(f2 - s2, 1.0), cw) / cw))
        entries.append((np.array(idx, dtype=np.int64), np.array(w, dtype=np.float32)))
        detail.append(dict(f1=f1, f2=f2, cw=cw, s1=s1, s2=s2, head=head, tail=tail))
    return entries, detail


def _padded(entries):
    """(index, weight, count) arrays of a table, padded to the longest entry list."""
    K = max(len(i) for i, _ in entries)
    idx = np.zeros((len(entries), K), dtype=np.int64)
    w = np.zeros((len(entries), K), dtype=np.float32)
    cnt = np.array([len(i) for i, _ in entries])
    for d, (i, ww) in enumerate(entries):
        idx[d, :len(i)] = i
        w[d, :len(i)] = ww
    return idx, w, cnt


def _general(S, ytab, xtab, WT):
    """S: (T, N_i, N_j) in WT.  Returns sum (T, n_i, n_j) in WT."""
    xi, xw, xc = _padded(xtab)
    xw = xw.astype(WT)
    out = np.zeros((S.shape[0], len(ytab), len(xtab)), dtype=WT)
    for dy, (rows, betas) in enumerate(ytab):
        total = None
        for r, beta in zip(rows, betas):
            buf = np.zeros((S.shape[0], len(xtab)), dtype=WT)
            for k in range(xi.shape[1]):
                m = xc > k
                prod = S[:, r, xi[m, k]] * xw[m, k]            # rounded in WT
                buf[:, m] = buf[:, m] + prod                    # rounded in WT
            t = WT(beta) * buf
            total = t if total is None else total + t
        out[:, dy] = total
    return out


def _blocks(movie, n_i, n_j, isy, isx):
    """(T, n_i, n_j, area): the samples of every block in row-major order k = sy * isx + sx."""
    T = movie.shape[0]
    b = movie[:, :n_i * isy, :n_j * isx].reshape(T, n_i, isy, n_j, isx)
    return b.transpose(0, 1, 3, 2, 4).reshape(T, n_i, n_j, isy * isx)


def unrolled_sum(samples):
    """OpenCV's float64 block sum over the last axis: groups of four as ((a + b) + c) + d, then the rest one by one."""
    area = samples.shape[-1]
    total = np.zeros(samples.shape[:-1], dtype=np.float64)
    k = 0
    while k <= area - 4:
        total = total + (((samples[..., k] + samples[..., k + 1]) + samples[..., k + 2]) + samples[..., k + 3])
        k += 4
    while k < area:
        total = total + samples[..., k]
        k += 1
    return total


def saturate_u8(x):
    """rint (half to even), then the clamp to 0 .. 255."""
    return np.clip(np.rint(x), 0, 255)


def resize_area(movie, n_i, n_j, record=None):
    """``cv2.resize(frame, (n_j, n_i), interpolation=cv2.INTER_AREA)`` of every frame of a uint8 or float64 ``(T, N_i, N_j)``
    stack, as float64 ``(T, n_i, n_j)``.  ``record`` (a dict) receives the path ("fast" / "general"), the per-axis scales, the
    tables and, on the fast path, what the other roundings would have given."""
    movie = np.asarray(movie)
    if movie.dtype not in (np.uint8, np.float64):
        raise ValueError("uint8 or float64 only")
    if movie.ndim != 3:
        raise ValueError("movie must be (T, N_i, N_j)")
    T, N_i, N_j = movie.shape
    if not (1 <= n_i <= N_i and 1 <= n_j <= N_j):
        raise ValueError("downsampling only")
    u8 = movie.dtype == np.uint8
    scale_y, iscale_y = axis_scale(N_i, n_i)
    scale_x, iscale_x = axis_scale(N_j, n_j)
    fast = abs(scale_x - iscale_x) < DBL_EPSILON and abs(scale_y - iscale_y) < DBL_EPSILON
    rec = record if record is not None else {}
    rec.update(path="fast" if fast else "general", scale_y=scale_y, scale_x=scale_x, iscale_y=iscale_y, iscale_x=iscale_x, u8=u8)
    if not fast:
        ytab, ydetail = axis_table(N_i, n_i)
        xtab, xdetail = axis_table(N_j, n_j)
        rec.update(ytab=ytab, xtab=xtab, ydetail=ydetail, xdetail=xdetail)
        WT = np.float32 if u8 else np.float64
        total = _general(movie.astype(WT), ytab, xtab, WT)
        rec["sum"] = total
        return saturate_u8(total).astype(np.float64) if u8 else total
    area = iscale_x * iscale_y
    scale_f = np.float32(1.0) / np.float32(area)
    rec.update(area=area, scale_f=scale_f)
    blocks = _blocks(movie, n_i, n_j, iscale_y, iscale_x)
    if u8:
        isum = blocks.astype(np.int64).sum(axis=-1)
        rec["block_sum"] = isum
        half_even = saturate_u8(isum.astype(np.float32) * scale_f).astype(np.float64)
        rec["rint"] = half_even
        if iscale_x == 2 and iscale_y == 2:
            rec["path"] = "fast2x2"
            return ((isum + 2) >> 2).astype(np.float64)
        return half_even
    total = unrolled_sum(blocks)
    left_to_right = np.zeros_like(total)
    for k in range(area):
        left_to_right = left_to_right + blocks[..., k]
    rec["left_to_right"] = left_to_right * np.float64(scale_f)
    return total * np.float64(scale_f)


def exact_area_mean(frame, n_i, n_j):
    """The mean of ``frame`` over the cell [d N / n, (d + 1) N / n) of every output pixel, each source pixel weighted by the
    length of its overlap with the cell: two dense float64 weight matrices, no tables, no float32."""
    frame = np.asarray(frame, dtype=np.float64)

    def weights(N, n):
        d = np.arange(n, dtype=np.float64)[:, None]
        s = np.arange(N, dtype=np.float64)[None, :]
        lo, hi = d * N / n, (d + 1) * N / n
        overlap = np.clip(np.minimum(s + 1, hi) - np.maximum(s, lo), 0.0, None)
        return overlap * (n / N)

    return weights(frame.shape[0], n_i) @ frame @ weights(frame.shape[1], n_j).T
