// vof_preprocess.hpp - the two per-frame preprocessing steps the reference's scripts run around every estimator, on gfx950:
// apply_adaptive_threshold (OF.py:308-338: cv2.adaptiveThreshold, ADAPTIVE_THRESH_MEAN_C / THRESH_BINARY, of the movie scaled
// to uint8) and apply_clahe (OF.py:340-374: cv2.createCLAHE(...).apply of the movie cast to uint16).  OpenCV 4's arithmetic is
// restated kernel by kernel below (DESIGN.md section 14 has the whole specification); everything up to the CLAHE blend is
// integer, so no result depends on the order of an atomic or of a reduction.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vof_shared.hpp"

namespace vof {

constexpr int PP_BLOCK = 256;
constexpr int PP_RANGE_BLOCKS = 1024;     // partial records of the range reduction at most
constexpr int PP_MAX_ROW = 15360;         // adaptive threshold: n_j up to this (the row's prefix sums live in 60 KiB of LDS)
constexpr int PP_MAX_WINDOW = 4095;       // ... and window_size up to this: 255 * w^2 < 2^32, every window sum fits 32 bits
constexpr int PP_COL_ROWS = 64;           // rows a lane of the column pass slides its window down
constexpr int PP_BINS = 65536;            // CLAHE: histSize of a 16-bit image
constexpr int PP_LUT_STEP = 4 * PP_BLOCK; // bins a workgroup of k_pp_lut takes per iteration (4 per lane)

// profiler stages of VOF_K_PREPROCESS (the `level` of vof_profile_get)
enum { PP_ST_RANGE = 0, PP_ST_ROWSUM, PP_ST_THRESHOLD, PP_ST_HIST, PP_ST_LUT, PP_ST_BLEND, PP_ST_RESIZE };

struct PpRange { double vmax, vmin; unsigned long long bad; };   // of the finite values; bad: NaN / Inf count

__device__ inline unsigned int pp_wave_scan(unsigned int v) {    // inclusive, over the 64 lanes
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// ---- max, min and the non-finite count of n doubles: part[blockIdx.x], then one record -----------------------------
__global__ __launch_bounds__(PP_BLOCK) void k_pp_range(const double* __restrict__ x, size_t n, PpRange* __restrict__ part) {
    __shared__ PpRange ws[PP_BLOCK / 64];
    double mx = -INFINITY, mn = INFINITY;
    unsigned long long bad = 0;
    for (size_t i = (size_t)blockIdx.x * PP_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * PP_BLOCK) {
        const double v = x[i];
        if (isfinite(v)) { mx = fmax(mx, v); mn = fmin(mn, v); }
        else ++bad;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        mx = fmax(mx, __shfl_down(mx, d));
        mn = fmin(mn, __shfl_down(mn, d));
        bad += __shfl_down(bad, d);
    }
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = PpRange{mx, mn, bad};
    __syncthreads();
    if (threadIdx.x == 0) {
        PpRange r = ws[0];
        for (int w = 1; w < PP_BLOCK / 64; ++w) { r.vmax = fmax(r.vmax, ws[w].vmax); r.vmin = fmin(r.vmin, ws[w].vmin); r.bad += ws[w].bad; }
        part[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(64) void k_pp_range_final(const PpRange* __restrict__ part, int nb, PpRange* __restrict__ out) {
    double mx = -INFINITY, mn = INFINITY;
    unsigned long long bad = 0;
    for (int i = threadIdx.x; i < nb; i += 64) { mx = fmax(mx, part[i].vmax); mn = fmin(mn, part[i].vmin); bad += part[i].bad; }
    for (int d = 32; d >= 1; d >>= 1) {
        mx = fmax(mx, __shfl_down(mx, d));
        mn = fmin(mn, __shfl_down(mn, d));
        bad += __shfl_down(bad, d);
    }
    if (threadIdx.x == 0) *out = PpRange{mx, mn, bad};
}

// ---- adaptive threshold ------------------------------------------------------------------------------------------------
// u = (uint8) trunc((x / m) * 255.0): a float64 division, then a multiplication, then the truncation (0 <= x <= m was checked)
__device__ inline unsigned int pp_u8(double x, double m) {
    const double q = x / m;
    return (unsigned int)(q * 255.0);
}

// Row pass: H[row][j] = sum of u over the columns j - r .. j + r, indices clamped to the row (BORDER_REPLICATE).  One workgroup
// per (row, frame): u is recomputed from x, scanned into LDS (inclusive prefix P, a tile of 256 at a time), and
//   H = P[min(j + r, W - 1)] - P[max(j - r, 0) - 1] + (columns left of 0) * u[0] + (columns right of W - 1) * u[W - 1].
// Dynamic LDS: n_j * 4 bytes.
__global__ __launch_bounds__(PP_BLOCK) void k_pp_rowsum(const double* __restrict__ x, int ni, int nj, double m, int r,
                                                        unsigned int* __restrict__ H) {
    extern __shared__ unsigned int pp_P[];
    __shared__ unsigned int wt[PP_BLOCK / 64];
    const size_t row = (size_t)blockIdx.y * ni + blockIdx.x;
    const double* xr = x + row * nj;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int carry = 0;
    for (int base = 0; base < nj; base += PP_BLOCK) {
        const int j = base + threadIdx.x;
        const unsigned int s = pp_wave_scan(j < nj ? pp_u8(xr[j], m) : 0u);
        if (lane == 63) wt[wave] = s;
        __syncthreads();
        unsigned int off = carry, tot = 0;
        for (int w = 0; w < PP_BLOCK / 64; ++w) { if (w < wave) off += wt[w]; tot += wt[w]; }
        if (j < nj) pp_P[j] = s + off;
        carry += tot;
        __syncthreads();
    }
    const unsigned int first = pp_P[0], last = pp_P[nj - 1] - pp_P[nj - 2];
    for (int j = threadIdx.x; j < nj; j += PP_BLOCK) {
        const int lo = j - r, hi = j + r;
        const int clo = lo < 0 ? 0 : lo, chi = hi > nj - 1 ? nj - 1 : hi;
        unsigned int s = pp_P[chi] - (clo > 0 ? pp_P[clo - 1] : 0u);
        s += (unsigned int)(clo - lo) * first + (unsigned int)(hi - chi) * last;
        H[row * nj + j] = s;
    }
}

// Column pass, fused with the mean, the comparison and the 1-byte store.  Grid (ceil(nj / 256), ceil(ni / PP_COL_ROWS), frames),
// no LDS, no barrier.  A lane owns a column and PP_COL_ROWS rows: it sums
// the rows i0 - r .. i0 + r of H (clamped rows by their multiplicity), then slides the window down one row at a time.
//   S = window sum of u (w x w, replicate border);  mean = floor((2 S + w^2) / (2 w^2))  (S / w^2 to nearest; w odd: no tie)
//   mask = (u - mean) > -idelta  <=>  mean <= u + idelta - 1  <=>  2 S + w^2 < (u + idelta) * 2 w^2   (no division)
__global__ __launch_bounds__(PP_BLOCK) void k_pp_threshold(const double* __restrict__ x, const unsigned int* __restrict__ H, int ni, int nj,
                                                     double m, int r, int idelta, uint8_t* __restrict__ mask) {
    const int j = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (j >= nj) return;
    const size_t plane = (size_t)blockIdx.z * ni * nj;
    const unsigned int* Hc = H + plane + j;
    const double* xc = x + plane + j;
    uint8_t* mc = mask + plane + j;
    const int i0 = blockIdx.y * PP_COL_ROWS, i1 = min(i0 + PP_COL_ROWS, ni);
    const int lo = i0 - r, hi = i0 + r;
    const int below = lo < 0 ? min(hi, -1) - lo + 1 : 0;              // rows of the window above the image
    const int above = hi > ni - 1 ? hi - max(lo, ni) + 1 : 0;         // ... and beyond its last row
    unsigned int S = (unsigned int)below * Hc[0] + (unsigned int)above * Hc[(size_t)(ni - 1) * nj];
    for (int k = max(lo, 0); k <= min(hi, ni - 1); ++k) S += Hc[(size_t)k * nj];
    const long long w = 2 * r + 1, w2 = w * w;
    for (int i = i0; i < i1; ++i) {
        const long long u = (long long)pp_u8(xc[(size_t)i * nj], m);
        mc[(size_t)i * nj] = (2 * (long long)S + w2 < (u + idelta) * 2 * w2) ? 1 : 0;
        const int in = min(i + r + 1, ni - 1), out = max(i - r, 0);
        S += Hc[(size_t)in * nj] - Hc[(size_t)out * nj];
    }
}

// ---- CLAHE ---------------------------------------------------------------------------------------------------------------
struct ClaheGeom {
    int ni, nj;               // image
    int tx, ty;               // tile grid: tx along j (OpenCV's tilesX), ty along i
    int pi, pj;               // padded image (reflect-101 at the bottom and the right; == ni, nj without padding)
    int tw, th;               // tile size: pj / tx, pi / ty
    int clip;                 // 0: no clipping
    float lut_scale;          // float32(65535) / float32(tw * th)
    float inv_tw, inv_th;     // 1.0f / tw, 1.0f / th
};

// v = (uint16) trunc(x) of every pixel of the padded image, counted into the histogram of its tile: hist[frame][tile][65536].
// The padding is read by index (c >= N -> 2 (N - 1) - c).  Grid (ceil(pj / 256), pi, frames).
__global__ __launch_bounds__(PP_BLOCK) void k_pp_hist(const double* __restrict__ x, ClaheGeom g, unsigned int* __restrict__ hist) {
    const int pj = blockIdx.x * PP_BLOCK + threadIdx.x, pi = blockIdx.y;
    if (pj >= g.pj) return;
    const int i = pi < g.ni ? pi : 2 * (g.ni - 1) - pi;
    const int j = pj < g.nj ? pj : 2 * (g.nj - 1) - pj;
    const unsigned int v = min((unsigned int)x[((size_t)blockIdx.z * g.ni + i) * g.nj + j], (unsigned int)(PP_BINS - 1));
    const size_t tile = ((size_t)blockIdx.z * g.ty + pi / g.th) * g.tx + pj / g.tw;
    atomicAdd(hist + tile * PP_BINS + v, 1u);
}

// One workgroup per (tile, frame): the clipped excess, the rebuilt bins and their running sum, in two passes over the tile's
// histogram, 4 bins per lane and iteration.
//   clipped = sum max(h - clip, 0);  batch = clipped / 65536;  residual = clipped % 65536;  step = max(65536 / residual, 1)
//   h'[i] = min(h[i], clip) + batch + (residual > 0 and i % step == 0 and i / step < residual)
//   lut[i] = saturate_u16(rint(float32(sum_{k <= i} h'[k]) * lut_scale))      one float32 multiplication, half to even
__global__ __launch_bounds__(PP_BLOCK) void k_pp_lut(const unsigned int* __restrict__ hist, ClaheGeom g, uint16_t* __restrict__ lut) {
    __shared__ unsigned int wt[PP_BLOCK / 64];
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint4* h4 = (const uint4*)(hist + tile * PP_BINS);
    ushort4* l4 = (ushort4*)(lut + tile * PP_BINS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int clip = g.clip > 0 ? (unsigned int)g.clip : 0xFFFFFFFFu;
    unsigned int clipped = 0;
    if (g.clip > 0) {
        unsigned int e = 0;
        for (int q = threadIdx.x; q < PP_BINS / 4; q += PP_BLOCK) {
            const uint4 h = h4[q];
            e += (h.x > clip ? h.x - clip : 0u) + (h.y > clip ? h.y - clip : 0u) + (h.z > clip ? h.z - clip : 0u) + (h.w > clip ? h.w - clip : 0u);
        }
        for (int d = 32; d >= 1; d >>= 1) e += __shfl_down(e, d);
        if (lane == 0) wt[wave] = e;
        __syncthreads();
        for (int w = 0; w < PP_BLOCK / 64; ++w) clipped += wt[w];
        __syncthreads();
    }
    const unsigned int batch = clipped / PP_BINS, residual = clipped % PP_BINS;
    const unsigned int step = residual ? max((unsigned int)PP_BINS / residual, 1u) : 1u;
    unsigned int carry = 0;
    for (int q = threadIdx.x; q < PP_BINS / 4; q += PP_BLOCK) {      // every lane runs every iteration
        const uint4 h = h4[q];
        unsigned int b[4] = {min(h.x, clip) + batch, min(h.y, clip) + batch, min(h.z, clip) + batch, min(h.w, clip) + batch};
        if (residual)
            for (int k = 0; k < 4; ++k) {
                const unsigned int i = 4u * q + k, d = i / step;
                b[k] += (d * step == i && d < residual) ? 1u : 0u;
            }
        b[1] += b[0]; b[2] += b[1]; b[3] += b[2];
        const unsigned int s = pp_wave_scan(b[3]);
        if (lane == 63) wt[wave] = s;
        __syncthreads();
        unsigned int off = carry + s - b[3], tot = 0;
        for (int w = 0; w < PP_BLOCK / 64; ++w) { if (w < wave) off += wt[w]; tot += wt[w]; }
        carry += tot;
        ushort4 o;
        unsigned short* op = (unsigned short*)&o;
        for (int k = 0; k < 4; ++k) {
            const int v = __float2int_rn((float)(off + b[k]) * g.lut_scale);
            op[k] = (unsigned short)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
        }
        l4[q] = o;
        __syncthreads();
    }
}

// The blend over the original pixels, float32, every operation rounded on its own: plain operators under fp contract(off) - the
// __fmul_rn / __fadd_rn wrappers are plain operators compiled where contraction is on, and hipcc fuses them after inlining:
//   txf = float(x) * inv_tw - 0.5f;  tx1 = floor(txf);  tx2 = tx1 + 1;  xa = txf - tx1;  xa1 = 1.0f - xa;  then tx1 >= 0, tx2 <= tx - 1
//   (the same in y);  res = (L11 * xa1 + L12 * xa) * ya1 + (L21 * xa1 + L22 * xa) * ya;  out = saturate_u16(rint(res)) as float64
// Grid (ceil(nj / 256), ni, frames).
__global__ __launch_bounds__(PP_BLOCK) void k_pp_blend(const double* __restrict__ x, ClaheGeom g, const uint16_t* __restrict__ lut,
                                                       double* __restrict__ out) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * PP_BLOCK + threadIdx.x, i = blockIdx.y;
    if (j >= g.nj) return;
    const float ry = (float)i * g.inv_th, tyf = ry - 0.5f;
    int ty1 = (int)floorf(tyf);
    const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
    int ty2 = ty1 + 1;
    ty1 = max(ty1, 0); ty2 = min(ty2, g.ty - 1);
    const float rx = (float)j * g.inv_tw, txf = rx - 0.5f;
    int tx1 = (int)floorf(txf);
    const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
    int tx2 = tx1 + 1;
    tx1 = max(tx1, 0); tx2 = min(tx2, g.tx - 1);
    const size_t p = ((size_t)blockIdx.z * g.ni + i) * g.nj + j;
    const unsigned int v = min((unsigned int)x[p], (unsigned int)(PP_BINS - 1));
    const uint16_t* L = lut + (size_t)blockIdx.z * g.ty * g.tx * PP_BINS + v;
    const float l11 = (float)L[((size_t)ty1 * g.tx + tx1) * PP_BINS], l12 = (float)L[((size_t)ty1 * g.tx + tx2) * PP_BINS];
    const float l21 = (float)L[((size_t)ty2 * g.tx + tx1) * PP_BINS], l22 = (float)L[((size_t)ty2 * g.tx + tx2) * PP_BINS];
    const float top = l11 * xa1 + l12 * xa;
    const float bot = l21 * xa1 + l22 * xa;
    const float res = top * ya1 + bot * ya;
    const int o = __float2int_rn(res);
    out[p] = (double)(o < 0 ? 0 : (o > 65535 ? 65535 : o));
}

}  // namespace vof
