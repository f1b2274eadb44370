// vof_piv.hpp - the dense part of the reference's convert_PIV_result (OF.py:2141-2230) on gfx950: the piecewise cubic of
// scipy.interpolate.griddata(..., method='cubic') - a Clough-Tocher element per Delaunay triangle - evaluated at every pixel of
// the frames in flight.  The triangulation and the gradients at the points are made by scipy on the host and arrive as tables;
// here are the control values per triangle, the triangle of every pixel and the value.  DESIGN.md section 19; the arithmetic is
// that of tests/piv_restatement.py, every operation single and uncontracted, and the kernels are held to it bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "vof_flowcompare.hpp"

namespace vof {

constexpr int PIV_BLOCK = 256;
constexpr int PIV_WAVE = 64;
constexpr int PIV_TRI_PER_BLOCK = PIV_BLOCK / PIV_WAVE;   // k_piv_locate: one wave per triangle
constexpr int PIV_COEF = 44;              // doubles per triangle: the transform (T00 T01 T10 T11 rx ry), 19 control values of v_x, 19 of v_y
constexpr int PIV_NONE = 0x7f7f7f7f;      // the map's "no triangle": one byte repeated, so a memset fills the map
constexpr double PIV_EPS = 100.0 * 2.220446049250313e-16;   // scipy's find_simplex tolerance on a barycentric coordinate
constexpr double PIV_BOX_MARGIN = 1e-6;   // pixels a bounding box is widened by: the tolerance reaches PIV_EPS * the triangle's extent past its vertices

// profiler stages of VOF_K_REDUCE, after those of vof_flowcompare.hpp
enum { PIV_ST_COEFFS = FC_ST_HISTOGRAMS + 1, PIV_ST_LOCATE, PIV_ST_EVAL };

// The tables of the frames of one chunk, frame after frame; a frame's rows start at pt_off[f] - pt_off[0] (points, values,
// gradients) and tri_off[f] - tri_off[0] (simplices, neighbours, transforms, coefficients): the offsets are those of the whole call.
struct PivTables {
    const double* points;      // 2 per point: x, y
    const double* values;      // 2 per point: v_x, v_y
    const double* grads;       // 4 per point: d v_x / dx, d v_x / dy, d v_y / dx, d v_y / dy
    const double* transforms;  // 6 per triangle
    const int* simplices;      // 3 per triangle, frame-local point indices
    const int* neighbours;     // 3 per triangle, frame-local triangle indices, -1: none
    const int* pt_off;         // [frame] and one more, of the chunk's first frame on
    const int* tri_off;
};

struct PivBary { double c0, c1, c2; };

__device__ __forceinline__ PivBary piv_barycentric(const double* __restrict__ T, double qx, double qy) {
#pragma clang fp contract(off)
    const double dx = qx - T[4], dy = qy - T[5];
    PivBary b;
    b.c0 = T[0] * dx + T[1] * dy;
    b.c1 = T[2] * dx + T[3] * dy;
    b.c2 = 1.0 - b.c0 - b.c1;
    return b;
}

__device__ __forceinline__ bool piv_inside(const PivBary& b) {
    return b.c0 >= -PIV_EPS && b.c0 <= 1.0 + PIV_EPS && b.c1 >= -PIV_EPS && b.c1 <= 1.0 + PIV_EPS && b.c2 >= -PIV_EPS && b.c2 <= 1.0 + PIV_EPS;
}

// ---- the control values: one thread per triangle, the frame is blockIdx.y --------------------------------------------------------
// coef[triangle][PIV_COEF]: the transform as it came, then per component the 19 control values in the order of the sum of k_piv_eval.
__global__ __launch_bounds__(PIV_BLOCK) void k_piv_coeffs(PivTables tb, double* __restrict__ coef) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const int t0 = tb.tri_off[f] - tb.tri_off[0], nt = tb.tri_off[f + 1] - tb.tri_off[f];
    const int p0 = tb.pt_off[f] - tb.pt_off[0];
    const int t = blockIdx.x * PIV_BLOCK + threadIdx.x;
    if (t >= nt) return;
    const double* P = tb.points + (size_t)2 * p0;
    const double* V = tb.values + (size_t)2 * p0;
    const double* G = tb.grads + (size_t)4 * p0;
    const int* S = tb.simplices + (size_t)3 * t0;
    const double* T = tb.transforms + (size_t)6 * (t0 + t);
    double* out = coef + (size_t)PIV_COEF * (t0 + t);
    for (int k = 0; k < 6; ++k) out[k] = T[k];
    const int v0 = S[3 * t], v1 = S[3 * t + 1], v2 = S[3 * t + 2];
    const double e12x = P[2 * v1] - P[2 * v0], e12y = P[2 * v1 + 1] - P[2 * v0 + 1];
    const double e23x = P[2 * v2] - P[2 * v1], e23y = P[2 * v2 + 1] - P[2 * v1 + 1];
    const double e31x = P[2 * v0] - P[2 * v2], e31y = P[2 * v0 + 1] - P[2 * v2 + 1];
    double g[3];
    for (int k = 0; k < 3; ++k) {                                  // the neighbour opposite vertex k
        const int nb = tb.neighbours[(size_t)3 * (t0 + t) + k];
        if (nb < 0) { g[k] = -0.5; continue; }
        const int a = S[3 * nb], b = S[3 * nb + 1], c = S[3 * nb + 2];
        const double yx = (P[2 * a] + P[2 * b] + P[2 * c]) / 3.0, yy = (P[2 * a + 1] + P[2 * b + 1] + P[2 * c + 1]) / 3.0;
        const PivBary y = piv_barycentric(T, yx, yy);
        const double ya = k == 0 ? y.c2 : (k == 1 ? y.c0 : y.c1), yb = k == 0 ? y.c1 : (k == 1 ? y.c2 : y.c0);
        g[k] = (2.0 * ya + yb - 1.0) / (2.0 - 3.0 * ya - 3.0 * yb);
    }
    for (int comp = 0; comp < 2; ++comp) {
        const double f1 = V[2 * v0 + comp], f2 = V[2 * v1 + comp], f3 = V[2 * v2 + comp];
        const double g0x = G[4 * v0 + 2 * comp], g0y = G[4 * v0 + 2 * comp + 1];
        const double g1x = G[4 * v1 + 2 * comp], g1y = G[4 * v1 + 2 * comp + 1];
        const double g2x = G[4 * v2 + 2 * comp], g2y = G[4 * v2 + 2 * comp + 1];
        const double df12 = +(g0x * e12x + g0y * e12y), df21 = -(g1x * e12x + g1y * e12y);
        const double df23 = +(g1x * e23x + g1y * e23y), df32 = -(g2x * e23x + g2y * e23y);
        const double df31 = +(g2x * e31x + g2y * e31y), df13 = -(g0x * e31x + g0y * e31y);
        const double c3000 = f1;
        const double c2100 = (df12 + 3.0 * c3000) / 3.0;
        const double c2010 = (df13 + 3.0 * c3000) / 3.0;
        const double c0300 = f2;
        const double c1200 = (df21 + 3.0 * c0300) / 3.0;
        const double c0210 = (df23 + 3.0 * c0300) / 3.0;
        const double c0030 = f3;
        const double c1020 = (df31 + 3.0 * c0030) / 3.0;
        const double c0120 = (df32 + 3.0 * c0030) / 3.0;
        const double c2001 = (c2100 + c2010 + c3000) / 3.0;
        const double c0201 = (c1200 + c0300 + c0210) / 3.0;
        const double c0021 = (c1020 + c0120 + c0030) / 3.0;
        const double c0111 = (g[0] * (-c0300 + 3.0 * c0210 - 3.0 * c0120 + c0030) + (-c0300 + 2.0 * c0210 - c0120 + c0021 + c0201)) / 2.0;
        const double c1011 = (g[1] * (-c0030 + 3.0 * c1020 - 3.0 * c2010 + c3000) + (-c0030 + 2.0 * c1020 - c2010 + c2001 + c0021)) / 2.0;
        const double c1101 = (g[2] * (-c3000 + 3.0 * c2100 - 3.0 * c1200 + c0300) + (-c3000 + 2.0 * c2100 - c1200 + c2001 + c0201)) / 2.0;
        const double c1002 = (c1101 + c1011 + c2001) / 3.0;
        const double c0102 = (c1101 + c0111 + c0201) / 3.0;
        const double c0012 = (c1011 + c0111 + c0021) / 3.0;
        const double c0003 = (c1002 + c0102 + c0012) / 3.0;
        double* o = out + 6 + 19 * comp;
        o[0] = c3000; o[1] = c2100; o[2] = c2010; o[3] = c2001; o[4] = c1200; o[5] = c1101; o[6] = c1020; o[7] = c1011; o[8] = c1002;
        o[9] = c0300; o[10] = c0210; o[11] = c0201; o[12] = c0120; o[13] = c0111; o[14] = c0102; o[15] = c0030; o[16] = c0021;
        o[17] = c0012; o[18] = c0003;
    }
}

// ---- the triangle of every pixel: one wave per triangle, the frame is blockIdx.y ---------------------------------------------------
// map[frame][Ni][Nj] was set to PIV_NONE.  The lanes stride over the pixels of the triangle's bounding box, widened by
// PIV_BOX_MARGIN and clipped to the image; a pixel the triangle includes takes the minimum of its entry and the triangle's index:
// integer atomics only, so the map is that of the lowest-index rule whatever the order of the waves.
__global__ __launch_bounds__(PIV_BLOCK) void k_piv_locate(PivTables tb, const double* __restrict__ coef, int* __restrict__ map, int Ni, int Nj) {
    const int f = blockIdx.y;
    const int t0 = tb.tri_off[f] - tb.tri_off[0], nt = tb.tri_off[f + 1] - tb.tri_off[f];
    const int t = blockIdx.x * PIV_TRI_PER_BLOCK + (int)(threadIdx.x / PIV_WAVE), lane = threadIdx.x % PIV_WAVE;
    if (t >= nt) return;
    const double* P = tb.points + (size_t)2 * (tb.pt_off[f] - tb.pt_off[0]);
    const int* S = tb.simplices + (size_t)3 * (t0 + t);
    const double* T = coef + (size_t)PIV_COEF * (t0 + t);
    const double x0 = P[2 * S[0]], x1 = P[2 * S[1]], x2 = P[2 * S[2]], y0 = P[2 * S[0] + 1], y1 = P[2 * S[1] + 1], y2 = P[2 * S[2] + 1];
    // the box in doubles first: clipped to the image before anything becomes an int
    const double jlo = fmax(ceil(fmin(x0, fmin(x1, x2)) - PIV_BOX_MARGIN), 0.0), jhi = fmin(floor(fmax(x0, fmax(x1, x2)) + PIV_BOX_MARGIN), (double)(Nj - 1));
    const double ilo = fmax(ceil(fmin(y0, fmin(y1, y2)) - PIV_BOX_MARGIN), 0.0), ihi = fmin(floor(fmax(y0, fmax(y1, y2)) + PIV_BOX_MARGIN), (double)(Ni - 1));
    if (!(jlo <= jhi && ilo <= ihi)) return;                        // outside the image (or not a number)
    const int j0 = (int)jlo, i0 = (int)ilo, w = (int)jhi - j0 + 1, h = (int)ihi - i0 + 1;
    int* m = map + (size_t)f * Ni * Nj;
    for (int k = lane; k < w * h; k += PIV_WAVE) {                  // w * h <= Ni * Nj < 2^31
        const int i = i0 + k / w, j = j0 + k % w;
        if (piv_inside(piv_barycentric(T, (double)j, (double)i))) atomicMin(&m[(size_t)i * Nj + j], t);
    }
}

// ---- the value: one thread per pixel, the frame is blockIdx.y -----------------------------------------------------------------------
__device__ __forceinline__ double piv_cubic(const double* __restrict__ k, double b1, double b2, double b3, double b4) {
#pragma clang fp contract(off)
    double w = ((b1 * b1) * b1) * k[0];
    w = w + ((3.0 * (b1 * b1)) * b2) * k[1];
    w = w + ((3.0 * (b1 * b1)) * b3) * k[2];
    w = w + ((3.0 * (b1 * b1)) * b4) * k[3];
    w = w + ((3.0 * b1) * (b2 * b2)) * k[4];
    w = w + (((6.0 * b1) * b2) * b4) * k[5];
    w = w + ((3.0 * b1) * (b3 * b3)) * k[6];
    w = w + (((6.0 * b1) * b3) * b4) * k[7];
    w = w + ((3.0 * b1) * (b4 * b4)) * k[8];
    w = w + ((b2 * b2) * b2) * k[9];
    w = w + ((3.0 * (b2 * b2)) * b3) * k[10];
    w = w + ((3.0 * (b2 * b2)) * b4) * k[11];
    w = w + ((3.0 * b2) * (b3 * b3)) * k[12];
    w = w + (((6.0 * b2) * b3) * b4) * k[13];
    w = w + ((3.0 * b2) * (b4 * b4)) * k[14];
    w = w + ((b3 * b3) * b3) * k[15];
    w = w + ((3.0 * (b3 * b3)) * b4) * k[16];
    w = w + ((3.0 * b3) * (b4 * b4)) * k[17];
    w = w + ((b4 * b4) * b4) * k[18];
    return w;
}

// A pixel without a triangle is NaN in all three outputs and counted in *outside - unless its frame has no triangle at all: that
// frame is the caller's (the host fallback) and only filled.  4 bytes read and 24 written per pixel; the coefficients of a pixel's
// triangle are shared by its neighbours and come from the caches.
__global__ __launch_bounds__(PIV_BLOCK) void k_piv_eval(PivTables tb, const double* __restrict__ coef, const int* __restrict__ map, int Ni, int Nj,
                                                        double* __restrict__ vx, double* __restrict__ vy, double* __restrict__ sp,
                                                        unsigned long long* __restrict__ outside) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const size_t fs = (size_t)Ni * Nj, p = (size_t)blockIdx.x * PIV_BLOCK + threadIdx.x;
    const int nt = tb.tri_off[f + 1] - tb.tri_off[f];
    bool none = false;
    if (p < fs) {
        const size_t o = (size_t)f * fs + p;
        const int t = map[o];
        none = t >= nt;                                             // PIV_NONE; an index past the frame's triangles cannot be in the map
        double a = __longlong_as_double(0x7ff8000000000000LL), b = a, s = a;
        if (!none) {
            const double* T = coef + (size_t)PIV_COEF * (tb.tri_off[f] - tb.tri_off[0] + t);
            const PivBary c = piv_barycentric(T, (double)(p % Nj), (double)(p / Nj));
            double m = c.c0;
            if (c.c1 < m) m = c.c1;
            if (c.c2 < m) m = c.c2;
            const double b1 = c.c0 - m, b2 = c.c1 - m, b3 = c.c2 - m, b4 = 3.0 * m;
            a = piv_cubic(T + 6, b1, b2, b3, b4);
            b = piv_cubic(T + 25, b1, b2, b3, b4);
            s = sqrt(a * a + b * b);
        }
        vx[o] = a; vy[o] = b; sp[o] = s;
    }
    const int n_none = __syncthreads_count(none && nt > 0);
    if (threadIdx.x == 0 && n_none) atomicAdd(outside, (unsigned long long)n_none);
}

}  // namespace vof
