// vof_farneback.hpp - cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
// OPTFLOW_FARNEBACK_GAUSSIAN) of every frame pair of a stack on gfx950 (conduct_opencv_flow; DESIGN.md section 16 has the
// specification).  OpenCV 4's optflowgf.cpp is restated operation by operation; every table that needs an exp comes from the host
// (farneback_plan), so no transcendental is evaluated here.  All float32 arithmetic is written as plain operators under
// fp contract(off): a product and the sum that takes it round separately, in the order the specification gives, whatever the tiling.
//
// Per pair and level the planes are float32 and planar, h x w each, the pair on the grid's z axis:
//   level image -> R (5 planes per role: the polynomial expansion) -> M (5 planes) <-> V (5 planes: M after the window's vertical pass)
// An iteration is two launches: k_fb_vblur (M -> V, an LDS tile of 32 + 2 m rows by 64 columns per workgroup and plane) and
// k_fb_update (V -> window sum along the row out of LDS, the 2 x 2 solve, the flow, and M rebuilt from the pixel's own new flow).
// With V between them M needs no second copy: the first launch only reads M, the second only writes it.
// The box window (OpenCV's default, flags = 0) has the same two launches, k_fb_box_rows and k_fb_box_update, with V in double.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vof_preprocess.hpp"

namespace vof {

constexpr int FB_BLOCK = 256;            // lanes of a row workgroup (one output pixel each)
constexpr int FB_MAX_POLY_N = 10;
constexpr int FB_MAX_WINSIZE = 129;      // m = winsize / 2 <= 64
constexpr int FB_VB_COLS = 64;           // k_fb_vblur: columns of a tile, two per lane
constexpr int FB_VB_ROWS = 32;           // ... and its output rows
constexpr int FB_VB_PER = FB_VB_ROWS / (FB_BLOCK / (FB_VB_COLS / 2));   // output rows of a lane: 4
constexpr int FB_PLANES = 27;            // float32 planes of scratch per pair in flight (FbPair), Gaussian window
constexpr int FB_BOX_PLANES = 32;        // ... box window: V is five double planes
constexpr int FB_BR_BLOCK = 64;          // k_fb_box_rows: lanes of a workgroup (a column of a plane each)
constexpr int FB_BR_LOOK = 16;           // ... steps whose rows of M a lane loads ahead (DESIGN.md section 16.4 has the ones dropped)
constexpr int FB_BU_ROWS = 8;            // k_fb_box_update: rows of a workgroup's band
constexpr int FB_BU_COLS = 32;           // ... columns of a tile
constexpr int FB_BU_PITCH = FB_BU_COLS + 1;   // ... doubles from one (row, plane) line in LDS to the next: odd

// profiler stages of VOF_K_PREPROCESS, after those of vof_preprocess.hpp
enum { PP_ST_FB_LEVEL = PP_ST_RESIZE + 1, PP_ST_FB_POLY, PP_ST_FB_FLOW, PP_ST_FB_MATRICES, PP_ST_FB_VBLUR, PP_ST_FB_UPDATE, PP_ST_FB_OUT,
       PP_ST_FB_BOX_ROWS, PP_ST_FB_BOX_UPDATE };

__device__ inline int fb_reflect101(int i, int n) {
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
    }
    return i;
}

// One pass of the pre-smoothing, BORDER_REFLECT_101: s = w[r] * S[0], then s = s + w[r + i] * (S[-i] + S[+i]) for i = 1 .. r.
// ALONG_ROW: the taps run along the columns (the first pass, which also converts the frame to float32).  Grid (ceil(nj / FB_BLOCK), ni, frames).
template <typename T, bool ALONG_ROW>
__global__ __launch_bounds__(FB_BLOCK) void k_fb_smooth(const T* __restrict__ in, size_t in_stride, int ni, int nj, const float* __restrict__ w, int r,
                                                        float* __restrict__ out, size_t out_stride) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * FB_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= nj) return;
    const T* f = in + (size_t)blockIdx.z * in_stride;
    float s = w[r] * (float)f[(size_t)y * nj + x];
    for (int i = 1; i <= r; ++i) {
        float a, b;
        if (ALONG_ROW) {
            a = (float)f[(size_t)y * nj + fb_reflect101(x - i, nj)];
            b = (float)f[(size_t)y * nj + fb_reflect101(x + i, nj)];
        } else {
            a = (float)f[(size_t)fb_reflect101(y - i, ni) * nj + x];
            b = (float)f[(size_t)fb_reflect101(y + i, ni) * nj + x];
        }
        const float p = w[r + i] * (a + b);
        s = s + p;
    }
    out[(size_t)blockIdx.z * out_stride + (size_t)y * nj + x] = s;
}

// One axis of cv2.resize's INTER_LINEAR: f = float32((d + 0.5) * sc - 0.5), s = floor(f), f -= s; s < 0 -> (0, 0); s >= ssize - 1 ->
// (ssize - 1, 0) and a single term.
struct FbTap { int s; float f; bool two; };
__device__ inline FbTap fb_linear_tap(int d, double sc, int ssize) {
#pragma clang fp contract(off)
    const double pos = (d + 0.5) * sc;
    float f = (float)(pos - 0.5);
    const float fl = floorf(f);
    int s = (int)fl;
    f = f - fl;
    if (s < 0) { s = 0; f = 0.0f; }
    const bool two = s < ssize - 1;
    if (!two) { s = ssize - 1; f = 0.0f; }
    return FbTap{s, f, two};
}

// Bilinear resize of `planes` planes per pair, the horizontal pass S[s] * (1 - f) + S[s + 1] * f first, then the vertical one in the
// same form on its results; SCALE: every value is then multiplied by mul (the flow carried to the next finer level).
// Grid (ceil(dw / FB_BLOCK), dh, pairs * planes).
template <bool SCALE>
__global__ __launch_bounds__(FB_BLOCK) void k_fb_resize(const float* __restrict__ in, size_t in_stride, int sh, int sw, float* __restrict__ out,
                                                        size_t out_stride, int dh, int dw, double scy, double scx, int planes, float mul) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * FB_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const int pair = blockIdx.z / planes, plane = blockIdx.z % planes;
    const float* S = in + (size_t)pair * in_stride + (size_t)plane * sh * sw;
    const FbTap tx = fb_linear_tap(x, scx, sw), ty = fb_linear_tap(y, scy, sh);
    const float wx = 1.0f - tx.f, wy = 1.0f - ty.f;
    float h[2] = {0.0f, 0.0f};
    for (int e = 0; e < (ty.two ? 2 : 1); ++e) {
        const float* row = S + (size_t)(ty.s + e) * sw;
        float v = row[tx.s] * wx;
        if (tx.two) { const float q = row[tx.s + 1] * tx.f; v = v + q; }
        h[e] = v;
    }
    float v = h[0] * wy;
    if (ty.two) { const float q = h[1] * ty.f; v = v + q; }
    if (SCALE) v = v * mul;
    out[(size_t)pair * out_stride + (size_t)plane * dh * dw + (size_t)y * dw + x] = v;
}

// Polynomial expansion of a level image, FarnebackPolyExp.  tab: g | xg | xxg, 2 n + 1 floats each (index n + k for offset k).
// Vertical pass (float32, rows clamped) of the workgroup's columns and n more on either side (columns clamped) into LDS:
//   t0 = S[y] * g[0], t1 = t2 = 0; for k = 1 .. n: a = S[y - k], b = S[y + k], p = a + b; t0 += g[k] * p; t1 += xg[k] * (b - a); t2 += xxg[k] * p
// Horizontal pass in double: the sum or difference of two t values is a float32 promoted, every product and running sum double.
// Grid (ceil(w / FB_BLOCK), h, frames).
struct FbInvG { double ig11, ig03, ig33, ig55; };
__global__ __launch_bounds__(FB_BLOCK) void k_fb_polyexp(const float* __restrict__ img, size_t img_stride, int h, int w, int n, const float* __restrict__ tab,
                                                         FbInvG ig, float* __restrict__ R, size_t R_stride) {
#pragma clang fp contract(off)
    __shared__ float t[3][FB_BLOCK + 2 * FB_MAX_POLY_N];
    const int x0 = blockIdx.x * FB_BLOCK, y = blockIdx.y;
    const float* S = img + (size_t)blockIdx.z * img_stride;
    const float *g = tab + n, *xg = tab + (2 * n + 1) + n, *xxg = tab + 2 * (2 * n + 1) + n;
    for (int e = threadIdx.x; e < FB_BLOCK + 2 * n; e += FB_BLOCK) {
        const int col = min(max(x0 - n + e, 0), w - 1);
        float t0 = S[(size_t)y * w + col] * g[0], t1 = 0.0f, t2 = 0.0f;
        for (int k = 1; k <= n; ++k) {
            const float a = S[(size_t)max(y - k, 0) * w + col], b = S[(size_t)min(y + k, h - 1) * w + col];
            const float p = a + b, d = b - a;
            const float q0 = g[k] * p, q1 = xg[k] * d, q2 = xxg[k] * p;
            t0 = t0 + q0; t1 = t1 + q1; t2 = t2 + q2;
        }
        t[0][e] = t0; t[1][e] = t1; t[2][e] = t2;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    // the column x + k clamped to the image is the LDS entry of that clamped column
    const int c = threadIdx.x + n;
    const double g0 = (double)g[0];
    double b1 = (double)t[0][c] * g0, b3 = (double)t[1][c] * g0, b5 = (double)t[2][c] * g0, b2 = 0.0, b4 = 0.0, b6 = 0.0;
    for (int k = 1; k <= n; ++k) {
        const int hi = min(x + k, w - 1) - x0 + n, lo = max(x - k, 0) - x0 + n;
        const double gk = (double)g[k], xgk = (double)xg[k], xxgk = (double)xxg[k];
        const float s0 = t[0][hi] + t[0][lo], d0 = t[0][hi] - t[0][lo];
        const float s1 = t[1][hi] + t[1][lo], d1 = t[1][hi] - t[1][lo];
        const float s2 = t[2][hi] + t[2][lo];
        const double tg = (double)s0;
        const double p1 = tg * gk, p4 = tg * xxgk, p2 = (double)d0 * xgk, p3 = (double)s1 * gk, p6 = (double)d1 * xgk, p5 = (double)s2 * gk;
        b1 = b1 + p1; b4 = b4 + p4; b2 = b2 + p2; b3 = b3 + p3; b6 = b6 + p6; b5 = b5 + p5;
    }
    const size_t hw = (size_t)h * w;
    float* o = R + (size_t)blockIdx.z * R_stride + (size_t)y * w + x;
    const double q13 = b1 * ig.ig03, q5 = b5 * ig.ig33, q4 = b4 * ig.ig33;
    o[0] = (float)(b3 * ig.ig11);
    o[hw] = (float)(b2 * ig.ig11);
    o[2 * hw] = (float)(q13 + q5);
    o[3 * hw] = (float)(q13 + q4);
    o[4 * hw] = (float)(b6 * ig.ig55);
}

// FarnebackUpdateMatrices at one pixel: M[0 .. 4] from R0 at the pixel, R1 gathered bilinearly at (x + dx, y + dy) and the pixel's flow.
// A position whose floor is not inside [0, w - 1) x [0, h - 1) - NaN and what fits no int included - takes the outside branch.
__device__ inline void fb_matrix_values(const float* __restrict__ R0, const float* __restrict__ R1, int h, int w, int x, int y, float dx, float dy,
                                        float* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t hw = (size_t)h * w, at = (size_t)y * w + x;
    float fx = (float)x + dx, fy = (float)y + dy;
    const float flx = floorf(fx), fly = floorf(fy);
    float r2, r3, r4, r5, r6;
    const float c2 = R0[at + 2 * hw], c3 = R0[at + 3 * hw], c4 = R0[at + 4 * hw];
    if (flx >= 0.0f && flx < (float)(w - 1) && fly >= 0.0f && fly < (float)(h - 1)) {
        const int x1 = (int)flx, y1 = (int)fly;
        fx = fx - flx; fy = fy - fly;
        const float ux = 1.0f - fx, uy = 1.0f - fy;
        const float a00 = ux * uy, a01 = fx * uy, a10 = ux * fy, a11 = fx * fy;
        const float* p = R1 + (size_t)y1 * w + x1;
        float r[5];
        for (int c = 0; c < 5; ++c, p += hw) {
            const float q0 = a00 * p[0], q1 = a01 * p[1], q2 = a10 * p[w], q3 = a11 * p[w + 1];
            r[c] = ((q0 + q1) + q2) + q3;
        }
        r2 = r[0]; r3 = r[1];
        r4 = (c2 + r[2]) * 0.5f;
        r5 = (c3 + r[3]) * 0.5f;
        r6 = (c4 + r[4]) * 0.25f;
    } else {
        r2 = 0.0f; r3 = 0.0f;
        r4 = c2; r5 = c3;
        r6 = c4 * 0.5f;
    }
    r2 = (R0[at] - r2) * 0.5f;
    r3 = (R0[at + hw] - r3) * 0.5f;
    {
        const float p0 = r4 * dy, p1 = r6 * dx, p2 = r6 * dy, p3 = r5 * dx;
        r2 = r2 + (p0 + p1);
        r3 = r3 + (p2 + p3);
    }
    if (x < 5 || x >= w - 5 || y < 5 || y >= h - 5) {
        const float bd[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
        float s = (x < 5 ? bd[x] : 1.0f) * (x >= w - 5 ? bd[w - x - 1] : 1.0f);
        s = s * (y < 5 ? bd[y] : 1.0f);
        s = s * (y >= h - 5 ? bd[h - y - 1] : 1.0f);
        r2 = r2 * s; r3 = r3 * s; r4 = r4 * s; r5 = r5 * s; r6 = r6 * s;
    }
    const float r44 = r4 * r4, r66 = r6 * r6, r55 = r5 * r5;
    const float r42 = r4 * r2, r63 = r6 * r3, r62 = r6 * r2, r53 = r5 * r3;
    out[0] = r44 + r66;
    out[1] = (r4 + r5) * r6;
    out[2] = r55 + r66;
    out[3] = r42 + r63;
    out[4] = r62 + r53;
}

__device__ inline void fb_matrix(const float* __restrict__ R0, const float* __restrict__ R1, int h, int w, int x, int y, float dx, float dy,
                                 float* __restrict__ M) {
    float v[5];
    fb_matrix_values(R0, R1, h, w, x, y, dx, dy, v);
    const size_t hw = (size_t)h * w, at = (size_t)y * w + x;
    for (int c = 0; c < 5; ++c) M[at + c * hw] = v[c];
}

// M of a whole level from its start flow.  Grid (ceil(w / FB_BLOCK), h, pairs); every array with its stride per pair.
__global__ __launch_bounds__(FB_BLOCK) void k_fb_matrices(const float* __restrict__ R0, const float* __restrict__ R1, const float* __restrict__ flow,
                                                          float* __restrict__ M, size_t stride, int h, int w) {
    const int x = blockIdx.x * FB_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const size_t o = (size_t)blockIdx.z * stride, hw = (size_t)h * w, at = (size_t)y * w + x;
    fb_matrix(R0 + o, R1 + o, h, w, x, y, flow[o + at], flow[o + hw + at], M + o);
}

// The window's vertical pass, rows clamped: V[y] = M[y] * k[0], then V[y] += (M[y + i] + M[y - i]) * k[i] for i = 1 .. m.
// A workgroup stages the rows y0 - m .. y0 + FB_VB_ROWS - 1 + m of FB_VB_COLS columns of one plane in LDS as float2: a lane owns
// two neighbouring columns and FB_VB_PER output rows, so every LDS read is 8 bytes wide (a 32-lane half of a wave reads one
// 256-byte bank row) and feeds two sums.  Grid (ceil(w / 64), ceil(h / 32), pairs * 5); dynamic LDS (FB_VB_ROWS + 2 m) *
// FB_VB_COLS floats.
__global__ __launch_bounds__(FB_BLOCK) void k_fb_vblur(const float* __restrict__ M, float* __restrict__ V, size_t stride, int h, int w, int m,
                                                       const float* __restrict__ k) {
#pragma clang fp contract(off)
    extern __shared__ float2 fb_tile[];
    constexpr int PAIRS = FB_VB_COLS / 2, GROUPS = FB_BLOCK / PAIRS;      // 32 column pairs by 8 row groups
    const int pair = blockIdx.z / 5, plane = blockIdx.z % 5;
    const size_t o = (size_t)pair * stride + (size_t)plane * h * w;
    const int cp = threadIdx.x % PAIRS, q = threadIdx.x / PAIRS;
    const int x = blockIdx.x * FB_VB_COLS + 2 * cp, y0 = blockIdx.y * FB_VB_ROWS;
    const int xa = min(x, w - 1), xb = min(x + 1, w - 1);
    const int rows = FB_VB_ROWS + 2 * m;
    for (int r = q; r < rows; r += GROUPS) {
        const float* row = M + o + (size_t)min(max(y0 - m + r, 0), h - 1) * w;
        fb_tile[r * PAIRS + cp] = make_float2(row[xa], row[xb]);
    }
    __syncthreads();
    const float2* col = fb_tile + (q * FB_VB_PER + m) * PAIRS + cp;      // the lane's first output row
    float2 v[FB_VB_PER];
    const float k0 = k[0];
    for (int j = 0; j < FB_VB_PER; ++j) {
        const float2 c = col[j * PAIRS];
        v[j].x = c.x * k0;
        v[j].y = c.y * k0;
    }
    for (int i = 1; i <= m; ++i) {
        const float ki = k[i];
        for (int j = 0; j < FB_VB_PER; ++j) {
            const float2 a = col[(j + i) * PAIRS], b = col[(j - i) * PAIRS];
            const float px = (a.x + b.x) * ki, py = (a.y + b.y) * ki;
            v[j].x = v[j].x + px;
            v[j].y = v[j].y + py;
        }
    }
    for (int j = 0; j < FB_VB_PER; ++j) {
        const int y = y0 + q * FB_VB_PER + j;
        if (y >= h) break;
        if (x < w) V[o + (size_t)y * w + x] = v[j].x;
        if (x + 1 < w) V[o + (size_t)y * w + x + 1] = v[j].y;
    }
}

// The rest of an iteration at one pixel: the window's horizontal pass over V (columns clamped; h = V[x] * k[0], then
// h += k[i] * (V[x - i] + V[x + i])) out of the row segments staged in LDS, the solve in double
//   idet = 1 / (g11 * g22 - g12 * g12 + 1e-3); flow = ((g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet)
// the flow, and - unless this is the level's last iteration - M rebuilt from that flow.  Grid (ceil(w / FB_BLOCK), h, pairs).
__global__ __launch_bounds__(FB_BLOCK) void k_fb_update(const float* __restrict__ V, const float* __restrict__ R0, const float* __restrict__ R1,
                                                        float* __restrict__ flow, float* __restrict__ M, size_t stride, int h, int w, int m,
                                                        const float* __restrict__ k, int rebuild) {
#pragma clang fp contract(off)
    __shared__ float seg[5][FB_BLOCK + FB_MAX_WINSIZE - 1];
    const int x0 = blockIdx.x * FB_BLOCK, y = blockIdx.y;
    const size_t o = (size_t)blockIdx.z * stride, hw = (size_t)h * w;
    for (int e = threadIdx.x; e < FB_BLOCK + 2 * m; e += FB_BLOCK) {
        const int col = min(max(x0 - m + e, 0), w - 1);
        for (int c = 0; c < 5; ++c) seg[c][e] = V[o + c * hw + (size_t)y * w + col];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const int at = threadIdx.x + m;
    float b[5];
    const float k0 = k[0];
    for (int c = 0; c < 5; ++c) b[c] = seg[c][at] * k0;
    for (int i = 1; i <= m; ++i) {
        const float ki = k[i];
        for (int c = 0; c < 5; ++c) {
            const float p = ki * (seg[c][at - i] + seg[c][at + i]);
            b[c] = b[c] + p;
        }
    }
    const double g11 = b[0], g12 = b[1], g22 = b[2], h1 = b[3], h2 = b[4];
    const double p0 = g11 * g22, p1 = g12 * g12;
    const double idet = 1.0 / ((p0 - p1) + 1e-3);
    const double a0 = g11 * h2, a1 = g12 * h1, c0 = g22 * h1, c1 = g12 * h2;
    const float dx = (float)((a0 - a1) * idet), dy = (float)((c0 - c1) * idet);
    const size_t px = (size_t)y * w + x;
    flow[o + px] = dx;
    flow[o + hw + px] = dy;
    if (rebuild) fb_matrix(R0 + o, R1 + o, h, w, x, y, dx, dy, M + o);
}

// ---- the box window (flags without OPTFLOW_FARNEBACK_GAUSSIAN; DESIGN.md section 16.1, "Iteration, box window") ------------------
// OpenCV keeps the window as two running sums in double, so every value depends on the order of the additions: both kernels add
// in that order, one double addition per element; everything else (the differences, the solve, fb_matrix) is pixel-parallel.
//
// The vertical running sum of one column of one plane per lane, lanes along x (coalesced without staging):
//   v = double(float32(M[0] * float32(m + 2))); v += double(M[min(y, h - 1)]) for y = 1 .. m - 1; then for y = 0 .. h - 1
//   v += double(float32(M[min(y + m, h - 1)] - M[max(y - m - 1, 0)])), V[y] = v (double planes).
// A lane's addresses are known ahead, so it holds the two rows of M of the next FB_BR_LOOK steps in registers while it adds the
// current ones: at 1024^2 x 16 pairs there are 1.25 waves per SIMD and only loads in flight hide the memory latency.  Row indices
// past the last step are clamped, loaded and not used.  Grid (ceil(w / FB_BR_BLOCK), 1, pairs * 5).
template <int LOOK>
__global__ __launch_bounds__(FB_BR_BLOCK) void k_fb_box_rows(const float* __restrict__ M, size_t stride, double* __restrict__ V, size_t v_stride, int h, int w,
                                                             int m) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * FB_BR_BLOCK + threadIdx.x;
    if (x >= w) return;
    const int pair = blockIdx.z / 5, plane = blockIdx.z % 5;
    const size_t hw = (size_t)h * w;
    const float* Mc = M + (size_t)pair * stride + (size_t)plane * hw + x;
    double* Vc = V + (size_t)pair * v_stride + (size_t)plane * hw + x;
    double v = (double)(Mc[0] * (float)(m + 2));
    for (int y0 = 1; y0 < m; y0 += LOOK) {
        float a[LOOK];
#pragma unroll
        for (int j = 0; j < LOOK; ++j) a[j] = Mc[(size_t)min(y0 + j, h - 1) * w];
#pragma unroll
        for (int j = 0; j < LOOK; ++j) if (y0 + j < m) v = v + (double)a[j];
    }
    float a[LOOK], b[LOOK];
#pragma unroll
    for (int j = 0; j < LOOK; ++j) {
        a[j] = Mc[(size_t)min(j + m, h - 1) * w];
        b[j] = Mc[(size_t)max(min(j, h - 1) - m - 1, 0) * w];
    }
    for (int y0 = 0; y0 < h; y0 += LOOK) {
        float na[LOOK], nb[LOOK];
#pragma unroll
        for (int j = 0; j < LOOK; ++j) {
            const int y = min(y0 + LOOK + j, h - 1);
            na[j] = Mc[(size_t)min(y + m, h - 1) * w];
            nb[j] = Mc[(size_t)max(y - m - 1, 0) * w];
        }
#pragma unroll
        for (int j = 0; j < LOOK; ++j) {
            if (y0 + j < h) {
                const float d = a[j] - b[j];
                v = v + (double)d;
                Vc[(size_t)(y0 + j) * w] = v;
            }
            a[j] = na[j]; b[j] = nb[j];
        }
    }
}

// The rest of a box iteration.  The horizontal running sum of a row and plane, columns clamped, in double:
//   a = V[0] * double(m + 2); a += V[x] for x = 1 .. m - 1; then for x = 0 .. w - 1: a += (V[x + m] - V[x - m - 1]), g[x] = a
// then g * scale (1 / winsize^2), the solve of k_fb_update, the flow, and M rebuilt from it.  The chains run along x, so a workgroup
// owns a band of FB_BU_ROWS rows and sweeps x in tiles of FB_BU_COLS columns, three steps per tile:
//   (a) all lanes read V[x + m] and V[x - m - 1] (coalesced, 32 columns of a row and plane per half wave), form the difference in
//       double and store it in LDS, one line of FB_BU_PITCH doubles per (row, plane);
//   (b) one lane per (row, plane), 5 FB_BU_ROWS of the 256, adds its line in order into the running sum it keeps in a register and
//       overwrites the line with the sums;
//   (c) all lanes: FB_BU_ROWS / 8 pixels each (lanes along x), the solve, the flow and fb_matrix.
// A tile costs a workgroup two dependent trips to memory, (a)'s reads and (c)'s gather at the new flow, so (a)'s reads are requested
// a tile ahead, before (c), and only the gather's latency is left on the path.
// FB_BU_PITCH is odd: in (b) the 32 lanes of a half wave read 8 bytes at 66 L + 2 t dwords, 32 different bank pairs of the 64; (a)
// and (c) touch consecutive doubles.  Rows past the band's end inside the last band are clamped, computed and not written.
// Grid (ceil(h / FB_BU_ROWS), 1, pairs); 5 FB_BU_ROWS FB_BU_PITCH doubles of LDS.
__global__ __launch_bounds__(FB_BLOCK) void k_fb_box_update(const double* __restrict__ V, size_t v_stride, const float* __restrict__ R0,
                                                            const float* __restrict__ R1, float* __restrict__ flow, float* __restrict__ M, size_t stride,
                                                            int h, int w, int m, double scale, int rebuild) {
#pragma clang fp contract(off)
    constexpr int LINES = FB_BU_ROWS * 5, LOOK = 8;
    __shared__ double line[LINES * FB_BU_PITCH];
    const int y0 = blockIdx.x * FB_BU_ROWS, tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.z * stride, hw = (size_t)h * w;
    const double* Vp = V + (size_t)blockIdx.z * v_stride;
    double a = 0.0;                                                      // (b): the running sum of line tid = row * 5 + plane
    if (tid < LINES) {
        const double* row = Vp + (size_t)(tid % 5) * hw + (size_t)min(y0 + tid / 5, h - 1) * w;
        a = row[0] * (double)(m + 2);
        for (int x0 = 1; x0 < m; x0 += LOOK) {
            double s[LOOK];
#pragma unroll
            for (int j = 0; j < LOOK; ++j) s[j] = row[min(x0 + j, w - 1)];
#pragma unroll
            for (int j = 0; j < LOOK; ++j) if (x0 + j < m) a = a + s[j];
        }
    }
    static_assert(LINES * FB_BU_COLS % FB_BLOCK == 0 && FB_BU_ROWS * FB_BU_COLS % FB_BLOCK == 0, "whole rounds of the workgroup");
    constexpr int ROUNDS = LINES * FB_BU_COLS / FB_BLOCK;
    double enter[ROUNDS], leave[ROUNDS];                                 // (a): V[x + m] and V[x - m - 1] of the tile at x0, requested a tile ahead
    const auto request = [&](int x0) {
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
            const int e = i * FB_BLOCK + tid, t = e % FB_BU_COLS, l = e / FB_BU_COLS;
            const double* row = Vp + (size_t)(l % 5) * hw + (size_t)min(y0 + l / 5, h - 1) * w;
            enter[i] = row[min(x0 + t + m, w - 1)];
            leave[i] = row[max(min(x0 + t, w - 1) - m - 1, 0)];
        }
    };
    request(0);
    for (int x0 = 0; x0 < w; x0 += FB_BU_COLS) {
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
            const int e = i * FB_BLOCK + tid;
            line[e / FB_BU_COLS * FB_BU_PITCH + e % FB_BU_COLS] = enter[i] - leave[i];
        }
        __syncthreads();
        if (tid < LINES) {
            double* d = line + tid * FB_BU_PITCH;
#pragma unroll
            for (int t = 0; t < FB_BU_COLS; ++t) {
                a = a + d[t];
                d[t] = a;
            }
        }
        __syncthreads();
        request(x0 + FB_BU_COLS);                                        // in flight during (c); past the last tile: the last column again, unused
        // a lane's pixels are computed side by side - the loads of all of them in flight together - at coordinates clamped into the
        // image; only the stores ask whether the pixel exists
#pragma unroll
        for (int i = 0; i < FB_BU_ROWS * FB_BU_COLS / FB_BLOCK; ++i) {
            const int e = i * FB_BLOCK + tid;
            const bool inside = x0 + e % FB_BU_COLS < w && y0 + e / FB_BU_COLS < h;
            const int x = min(x0 + e % FB_BU_COLS, w - 1), y = min(y0 + e / FB_BU_COLS, h - 1);
            const double* g = line + (e / FB_BU_COLS) * 5 * FB_BU_PITCH + e % FB_BU_COLS;
            const double g11 = g[0] * scale, g12 = g[FB_BU_PITCH] * scale, g22 = g[2 * FB_BU_PITCH] * scale, h1 = g[3 * FB_BU_PITCH] * scale,
                         h2 = g[4 * FB_BU_PITCH] * scale;
            const double p0 = g11 * g22, p1 = g12 * g12;
            const double idet = 1.0 / ((p0 - p1) + 1e-3);
            const double a0 = g11 * h2, a1 = g12 * h1, c0 = g22 * h1, c1 = g12 * h2;
            const float dx = (float)((a0 - a1) * idet), dy = (float)((c0 - c1) * idet);
            const size_t px = (size_t)y * w + x;
            float v[5];
            if (rebuild) fb_matrix_values(R0 + o, R1 + o, h, w, x, y, dx, dy, v);
            if (inside) {
                flow[o + px] = dx;
                flow[o + hw + px] = dy;
                if (rebuild) for (int c = 0; c < 5; ++c) M[o + c * hw + px] = v[c];
            }
        }
        __syncthreads();                                                 // the next tile's (a) overwrites the lines
    }
}

// The results: the float32 flow promoted to double and multiplied by delta_x / delta_t; speed = sqrt(v_x * v_x + v_y * v_y) in double.
// Grid (ceil(n / FB_BLOCK), 1, pairs), n = n_i * n_j.
__global__ __launch_bounds__(FB_BLOCK) void k_fb_output(const float* __restrict__ flow, size_t stride, size_t n, double scale, double* __restrict__ vx,
                                                        double* __restrict__ vy, double* __restrict__ speed) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * FB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* f = flow + (size_t)blockIdx.z * stride;
    const double a = (double)f[i] * scale, b = (double)f[n + i] * scale;
    const double aa = a * a, bb = b * b;
    const size_t at = (size_t)blockIdx.z * n + i;
    vx[at] = a;
    vy[at] = b;
    speed[at] = __dsqrt_rn(aa + bb);
}

}  // namespace vof
