"""numpy restatement of ``apply_adaptive_threshold`` and ``apply_clahe`` as the GPU has to compute them, bit for bit.  It is
the arithmetic of OpenCV 4's ``adaptiveThreshold`` (mean, binary) and ``clahe.cpp`` (16-bit input) spelled out; of the
reference only its two casts (OF.py:330, 364) and its tile formula (OF.py:365-366) are pinned.  No ``cv2`` is used here:
tests/test_preprocess_cv2_cpu.py compares this file with the real one wherever it can be imported.

apply_adaptive_threshold(movie, window_size, threshold) - the input is read as float64:
 1. m = max(movie) over the whole stack.  ValueError if anything is non-finite, the minimum is < 0 or m <= 0 (the reference's
    uint8 cast of such values is platform-dependent: the one deviation).
 2. u = (uint8) trunc((x / m) * 255.0): a float64 division, then a multiplication, then the truncation.
 3. S = sum of u over the window_size x window_size window centred on the pixel, out-of-image indices clamped to the edge
    (BORDER_REPLICATE); the window may be larger than the image.  mean = floor((2 S + w^2) / (2 w^2)): S / w^2 rounded to
    nearest; w is odd, so a tie cannot occur.
 4. result = (u - mean) > -ceil(threshold)   (THRESH_BINARY with ADAPTIVE_THRESH_MEAN_C, maxValue 1, then the reference's == 1.0)
 5. window_size must be odd and > 1: ValueError otherwise.
 6. OpenCV's vectorised box filter scales S by float32(1 / w^2), its scalar tail by the double 1 / w^2, each followed by a
    rounding half to even; ``record`` receives both, so that a test can assert they equal the exact rounding on its input.

apply_clahe(movie, clipLimit, tile_number):
 1. v = (uint16) trunc(x).  ValueError unless every value is finite and in [0, 65536) (the reference wraps).
 2. histSize = 65536, tilesX = tile_number (along N_j: OpenCV's Size(width, height)), tilesY = round(tile_number * N_j / N_i)
    with Python's round, evaluated as the reference does, tile_number * (N_j / N_i).  ValueError unless 1 <= tilesX <= N_j - 1
    and 1 <= tilesY <= N_i - 1.
 3. Padding only if N_j % tilesX != 0 or N_i % tilesY != 0; then the right side grows by tilesX - N_j % tilesX columns and the
    bottom by tilesY - N_i % tilesY rows, BORDER_REFLECT_101 (index c >= N maps to 2 (N - 1) - c).  A dimension that divides
    still receives a full `tiles` of padding when the other does not.  tw, th = padded size / grid; area = tw * th.
 4. clip = max(int(clipLimit * area / 65536), 1) in double if clipLimit > 0; otherwise no clipping.
 5. Per tile: h = histogram of v; clipped = sum max(h - clip, 0); h = min(h, clip); batch = clipped // 65536, residual =
    clipped % 65536; h += batch; if residual > 0: step = max(65536 // residual, 1) and the bins 0, step, 2 step, ... get + 1,
    the first `residual` of them that are < 65536.
 6. lutScale = float32(65535) / float32(area); lut[i] = saturate_u16(rint(float32(sum_{k <= i} h[k]) * lutScale)): one float32
    multiplication, rounded half to even.
 7. Over the original (unpadded) pixels, all float32, every operation rounded on its own: inv_tw = 1.0f / tw;
    txf = float(x) * inv_tw - 0.5f; tx1 = floor(txf); tx2 = tx1 + 1; xa = txf - tx1; xa1 = 1.0f - xa; then tx1 >= 0 and
    tx2 <= tilesX - 1; the same in y with th;
    res = (L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya;
    output saturate_u16(rint(res)) as float64.
 8. The reference's print(np.max(...)) is not reproduced.
"""
import math

import numpy as np

BINS = 65536


# ---- adaptive threshold -------------------------------------------------------------------------------------------------
def scale_to_uint8(movie):
    x = np.asarray(movie, dtype=np.float64)
    if not np.isfinite(x).all():
        raise ValueError("non-finite values")
    m = x.max()
    if x.min() < 0 or not m > 0:
        raise ValueError("negative values or a maximum that is not positive")
    q = x / m
    return np.trunc(q * 255.0).astype(np.uint8)


def window_sums(u, w):
    """S of one uint8 frame: the w x w window sums with replicated borders, int64."""
    r = w // 2
    padded = np.pad(u.astype(np.int64), r, mode="edge")
    integral = np.zeros((padded.shape[0] + 1, padded.shape[1] + 1), dtype=np.int64)
    integral[1:, 1:] = padded.cumsum(0).cumsum(1)
    n_i, n_j = u.shape
    return integral[w:w + n_i, w:w + n_j] - integral[:n_i, w:w + n_j] - integral[w:w + n_i, :n_j] + integral[:n_i, :n_j]


def adaptive_threshold(movie, window_size=51, threshold=0.0, record=None):
    x = np.asarray(movie)
    if x.ndim != 3:
        raise ValueError("movie must be 3-D")
    w = int(window_size)
    if w != window_size or w % 2 == 0 or w <= 1:
        raise ValueError("window_size must be odd and > 1")
    u = scale_to_uint8(x)
    S = np.stack([window_sums(f, w) for f in u])
    mean = (2 * S + w * w) // (2 * w * w)
    idelta = math.ceil(threshold)
    if record is not None:
        record["u"], record["S"], record["mean"] = u, S, mean
        record["mean_float32"] = np.rint(S.astype(np.float32) * np.float32(1.0 / (w * w))).astype(np.int64)
        record["mean_float64"] = np.rint(S.astype(np.float64) * (1.0 / (w * w))).astype(np.int64)
    return (u.astype(np.int64) - mean) > -idelta


# ---- CLAHE --------------------------------------------------------------------------------------------------------------
def reflect101(c, n):
    """Source index of padded index c for a dimension of n: c >= n maps to 2 (n - 1) - c."""
    c = np.asarray(c)
    return np.where(c >= n, 2 * (n - 1) - c, c)


def clahe_geometry(n_i, n_j, tile_number, clipLimit):
    if int(tile_number) != tile_number:
        raise ValueError("tile_number must be an integer")
    tiles_x = int(tile_number)
    tiles_y = round(tile_number * (n_j / n_i))
    if not (1 <= tiles_x <= n_j - 1 and 1 <= tiles_y <= n_i - 1):
        raise ValueError("tile grid does not fit the image")
    pad = n_j % tiles_x != 0 or n_i % tiles_y != 0
    pad_j = tiles_x - n_j % tiles_x if pad else 0
    pad_i = tiles_y - n_i % tiles_y if pad else 0
    tw, th = (n_j + pad_j) // tiles_x, (n_i + pad_i) // tiles_y
    area = tw * th
    clip = max(int(float(clipLimit) * area / BINS), 1) if clipLimit > 0 else 0
    return dict(tilesX=tiles_x, tilesY=tiles_y, pad_i=pad_i, pad_j=pad_j, tw=tw, th=th, area=area, clip=clip)


def tile_table(values, clip, area):
    """The uint16 table of one tile from its (padded) pixels, and (clip, clipped, residual, batch, step)."""
    h = np.bincount(values.ravel(), minlength=BINS).astype(np.int64)
    clipped = residual = batch = step = 0
    if clip > 0:
        clipped = int(np.maximum(h - clip, 0).sum())
        h = np.minimum(h, clip)
        batch, residual = clipped // BINS, clipped % BINS
        h += batch
        if residual > 0:
            step = max(BINS // residual, 1)
            bins = np.arange(residual, dtype=np.int64) * step
            h[bins[bins < BINS]] += 1
    lut_scale = np.float32(BINS - 1) / np.float32(area)
    scaled = np.cumsum(h).astype(np.float32) * lut_scale
    assert scaled.dtype == np.float32
    lut = np.clip(np.rint(scaled), 0, BINS - 1).astype(np.uint16)
    return lut, (clip, clipped, residual, batch, step)


def blend_weights(n, inv_t, tiles):
    """(t1, t2, a, a1) of step 7 for the n pixel positions of one axis."""
    tf = np.arange(n, dtype=np.float32) * inv_t - np.float32(0.5)
    t1 = np.floor(tf).astype(np.int64)
    a = tf - t1.astype(np.float32)
    a1 = np.float32(1.0) - a
    assert tf.dtype == a.dtype == a1.dtype == np.float32
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def clahe(movie, clipLimit=50000, tile_number=10, record=None):
    x = np.asarray(movie)
    if x.ndim != 3:
        raise ValueError("movie must be 3-D")
    x = x.astype(np.float64)
    if not np.isfinite(x).all() or x.min() < 0 or x.max() >= BINS:
        raise ValueError("values outside [0, 65536)")
    v = np.trunc(x).astype(np.uint16)
    T, n_i, n_j = v.shape
    g = clahe_geometry(n_i, n_j, tile_number, clipLimit)
    rows = reflect101(np.arange(n_i + g["pad_i"]), n_i)
    cols = reflect101(np.arange(n_j + g["pad_j"]), n_j)
    ty1, ty2, ya, ya1 = blend_weights(n_i, np.float32(1.0) / np.float32(g["th"]), g["tilesY"])
    tx1, tx2, xa, xa1 = blend_weights(n_j, np.float32(1.0) / np.float32(g["tw"]), g["tilesX"])
    out = np.empty(v.shape, dtype=np.float64)
    tiles = []
    for t in range(T):
        padded = v[t][np.ix_(rows, cols)].astype(np.int64)
        luts = np.empty((g["tilesY"], g["tilesX"], BINS), dtype=np.uint16)
        rec = []
        for a in range(g["tilesY"]):
            for b in range(g["tilesX"]):
                luts[a, b], r = tile_table(padded[a * g["th"]:(a + 1) * g["th"], b * g["tw"]:(b + 1) * g["tw"]], g["clip"], g["area"])
                rec.append(r)
        tiles.append(rec)
        val = v[t].astype(np.int64)

        def L(ty, tx):
            return luts[ty[:, None], tx[None, :], val].astype(np.float32)
        top = L(ty1, tx1) * xa1[None, :] + L(ty1, tx2) * xa[None, :]
        bottom = L(ty2, tx1) * xa1[None, :] + L(ty2, tx2) * xa[None, :]
        res = top * ya1[:, None] + bottom * ya[:, None]
        assert res.dtype == np.float32
        out[t] = np.clip(np.rint(res), 0, BINS - 1).astype(np.float64)
    if record is not None:
        record.update(g)
        record["tiles"] = np.array(tiles, dtype=np.int64)          # (T, tilesY * tilesX, 5): clip, clipped, residual, batch, step
    return out
