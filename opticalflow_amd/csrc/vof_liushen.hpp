// vof_liushen.hpp - Liu-Shen physics-based flow without remodelling as a fixed number of Jacobi iterations
// (liu_shen_optical_flow_jit, OF.py:426-673) on gfx950, float64.
//
// Per frame pair (p = frame k, c = frame k + 1) every pixel is updated from the OLD iterate only:
//   v_new = A^-1 F,  A = [[I Ixx - 2 I^2 - n alpha, I Ixy], [I Ixy, I Iyy - 2 I^2 - n alpha]]  (n = 8 / 5 / 3: interior / edge line / corner)
// with F of OF.py:621-630, a 9-point stencil of p, v_x, v_y and a 5-point one of c.  The reference pads frames and fields by
// one pixel and mirrors the border (row -1 = row 1, row N = row N - 2, then the columns); here a pixel on an image edge reads
// its inner neighbour in place of the missing outer one, which is the same value and never leaves the image.  The
// 8-neighbour sums Vx_bar, Vy_bar take neighbours outside the image as zero (OF.py:531-548).
//
// ls_update is the only place the update is written: the reference's operation order, every operation explicit,
// contraction off, IEEE division.  Both kernels call it on the same values, so a pixel's new iterate has the same bits
// whichever kernel, tile or fusion depth computes it.
//   k_ls_step    one iteration per launch from and to device memory (VOF_LIUSHEN_FUSE=1)
//   k_ls_fused   k <= LS_KMAX iterations per launch: a LS_TI x LS_TJ tile of p, c and both fields with a halo of k pixels
//                lives in LDS (fields double-buffered), the updated region shrinks by one ring per iteration, the last
//                iteration stores the tile itself
//   k_ls_init / k_ls_finish   initial fields * delta_t / delta_x; fields * (delta_x / delta_t), speed, remodelling
#pragma once
#include <hip/hip_runtime.h>
#include "vof_shared.hpp"

namespace vof {

constexpr int LS_TI = 32, LS_TJ = 32;     // output tile of the fused kernel
constexpr int LS_THREADS = 256;
constexpr int LS_KMAX = 8;                // largest fusion depth (LDS: 6 planes of (32 + 16)^2 doubles = 108 KiB)
constexpr int LS_KDEF = 4;                // default fusion depth (6 planes of 40^2 doubles = 75 KiB: two blocks per CU)

struct LsArgs {
    const double* movie;       // frame 0 of the first pair of the launch; pair z is (frame z, frame z + 1)
    size_t fs;                 // doubles per frame
    int Ni, Nj;
    int k;                     // iterations of this launch (fused kernel)
    double alpha;
    const double *sx, *sy;     // old iterate (pairs, Ni, Nj)
    double *dx, *dy;           // new iterate
};

inline size_t ls_fused_lds(int k) { return (size_t)6 * (LS_TI + 2 * k) * (LS_TJ + 2 * k) * sizeof(double); }

// One pixel.  p, c, x, y point at the pixel in planes of one pitch; up / dn / lf / rt are the element offsets of the
// neighbours i - 1, i + 1, j - 1, j + 1, already mirrored on an image edge; top / bot / left / right say which edges the
// pixel lies on.
__device__ __forceinline__ void ls_update(const double* p, const double* c, const double* x, const double* y, int up, int dn, int lf,
                                          int rt, bool top, bool bot, bool left, bool right, double alpha, double& nx, double& ny) {
#pragma clang fp contract(off)
    const double I = p[0];
    const double pU = p[up], pD = p[dn], pL = p[lf], pR = p[rt];
    const double Ix = (pD - pU) / 2.0, Iy = (pR - pL) / 2.0;
    const double Ixt = (((c[dn] - c[up]) - pD) + pU) / 2.0;
    const double Iyt = (((c[rt] - c[lf]) - pR) + pL) / 2.0;
    const double Ixx = (pD + pU) - 2.0 * I, Iyy = (pR + pL) - 2.0 * I;
    const double Ixy = (((p[dn + rt] - p[dn + lf]) - p[up + rt]) + p[up + lf]) / 4.0;

    const double xU = x[up], xD = x[dn], xL = x[lf], xR = x[rt];
    const double xUL = x[up + lf], xUR = x[up + rt], xDL = x[dn + lf], xDR = x[dn + rt];
    const double yU = y[up], yD = y[dn], yL = y[lf], yR = y[rt];
    const double yUL = y[up + lf], yUR = y[up + rt], yDL = y[dn + lf], yDR = y[dn + rt];
    const double dxVx = (xD - xU) / 2.0, dyVx = (xR - xL) / 2.0;
    const double dxyVx = (((xDR - xDL) - xUR) + xUL) / 4.0;
    const double dxVy = (yD - yU) / 2.0, dyVy = (yR - yL) / 2.0;
    const double dxyVy = (((yDR - yDL) - yUR) + yUL) / 4.0;
    const double Vx_barx = xD + xU, Vy_bary = yR + yL;
    // OF.py:541-548: [0,1] + [2,1] + [1,2] + [1,0] + [0,0] + [0,2] + [2,0] + [2,2], rows / columns outside the image zeroed
    const double Vx_bar = (((((((top ? 0.0 : xU) + (bot ? 0.0 : xD)) + (right ? 0.0 : xR)) + (left ? 0.0 : xL)) +
                             ((top || left) ? 0.0 : xUL)) + ((top || right) ? 0.0 : xUR)) + ((bot || left) ? 0.0 : xDL)) +
                          ((bot || right) ? 0.0 : xDR);
    const double Vy_bar = (((((((top ? 0.0 : yU) + (bot ? 0.0 : yD)) + (right ? 0.0 : yR)) + (left ? 0.0 : yL)) +
                             ((top || left) ? 0.0 : yUL)) + ((top || right) ? 0.0 : yUR)) + ((bot || left) ? 0.0 : yDL)) +
                          ((bot || right) ? 0.0 : yDR);

    const double II = I * I;
    const double F0 = ((((-I) * Ixt) - I * ((((2.0 * Ix) * dxVx) + Iy * dxVy) + Ix * dyVy)) - II * (Vx_barx + dxyVy)) - alpha * Vx_bar;
    const double F1 = ((((-I) * Iyt) - I * ((((2.0 * Iy) * dyVy) + Ix * dyVx) + Iy * dxVx)) - II * (Vy_bary + dxyVx)) - alpha * Vy_bar;

    const bool ei = top || bot, ej = left || right;
    const double n = (ei && ej) ? 3.0 : ((ei || ej) ? 5.0 : 8.0);
    const double na = n * alpha;
    const double a = ((I * Ixx) - 2.0 * II) - na;
    const double b = I * Ixy;
    const double d = ((I * Iyy) - 2.0 * II) - na;
    const double det = a * d - b * b;
    nx = (d * F0 - b * F1) / det;
    ny = (a * F1 - b * F0) / det;
}

// ---- one iteration per launch ---------------------------------------------------------------------------------------
__global__ void k_ls_step(LsArgs a) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= a.Ni || j >= a.Nj) return;
    const size_t po = (size_t)blockIdx.z * a.fs, o = (size_t)i * a.Nj + j;
    const double* p = a.movie + po + o;
    const bool top = i == 0, bot = i == a.Ni - 1, left = j == 0, right = j == a.Nj - 1;
    double nx, ny;
    ls_update(p, p + a.fs, a.sx + po + o, a.sy + po + o, top ? a.Nj : -a.Nj, bot ? -a.Nj : a.Nj, left ? 1 : -1, right ? -1 : 1, top, bot,
              left, right, a.alpha, nx, ny);
    a.dx[po + o] = nx;
    a.dy[po + o] = ny;
}

// ---- a.k iterations per launch ----------------------------------------------------------------------------------------
// LDS planes of RI x RJ = (LS_TI + 2k) x (LS_TJ + 2k) doubles, pitch RJ: consecutive lanes read consecutive doubles for
// every one of the nine offsets.  Positions outside the image are neither loaded, computed nor read.
__global__ __launch_bounds__(LS_THREADS) void k_ls_fused(LsArgs a) {
    extern __shared__ double ls_lds[];
    const int k = a.k, RI = LS_TI + 2 * k, RJ = LS_TJ + 2 * k, plane = RI * RJ;
    double* sp = ls_lds;
    double* sc = sp + plane;
    double* bx[2] = {sc + plane, sc + 3 * plane};
    double* by[2] = {sc + 2 * plane, sc + 4 * plane};
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * LS_TI - k, j0 = blockIdx.x * LS_TJ - k;     // image position of the LDS origin
    const size_t po = (size_t)blockIdx.z * a.fs;
    {
        const double* p = a.movie + po;
        const double* c = p + a.fs;
        const double* x = a.sx + po;
        const double* y = a.sy + po;
        const int rlo = max(0, -i0), rhi = min(RI, a.Ni - i0), clo = max(0, -j0), chi = min(RJ, a.Nj - j0);
        const int w = chi - clo, count = (rhi - rlo) * w;
        for (int idx = tid; idx < count; idx += LS_THREADS) {
            const int q = idx / w, r = rlo + q, t = clo + (idx - q * w);
            const size_t g = (size_t)(i0 + r) * a.Nj + (j0 + t);
            const int o = r * RJ + t;
            sp[o] = p[g]; sc[o] = c[g]; bx[0][o] = x[g]; by[0][o] = y[g];
        }
    }
    __syncthreads();
    int cur = 0;
    for (int s = 1; s <= k; ++s) {
        // the tile widened by k - s rings, clipped to the image
        const int rlo = max(s, -i0), rhi = min(RI - s, a.Ni - i0), clo = max(s, -j0), chi = min(RJ - s, a.Nj - j0);
        const int w = chi - clo, count = (rhi - rlo) * w;
        const double* x = bx[cur];
        const double* y = by[cur];
        for (int idx = tid; idx < count; idx += LS_THREADS) {
            const int q = idx / w, r = rlo + q, t = clo + (idx - q * w);
            const int i = i0 + r, j = j0 + t, o = r * RJ + t;
            const bool top = i == 0, bot = i == a.Ni - 1, left = j == 0, right = j == a.Nj - 1;
            double nx, ny;
            ls_update(sp + o, sc + o, x + o, y + o, top ? RJ : -RJ, bot ? -RJ : RJ, left ? 1 : -1, right ? -1 : 1, top, bot, left, right,
                      a.alpha, nx, ny);
            if (s == k) {
                const size_t g = po + (size_t)i * a.Nj + j;
                a.dx[g] = nx;
                a.dy[g] = ny;
            } else {
                bx[cur ^ 1][o] = nx;
                by[cur ^ 1][o] = ny;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

// ---- first and last step ------------------------------------------------------------------------------------------------
// kind 0: the scalars; 1: one (Ni, Nj) plane for every pair; 2: a (pairs, Ni, Nj) stack.  Element-wise, so a source may be
// the destination itself.
__device__ __forceinline__ double ls_initial(const double* src, double scalar, int kind, size_t idx, size_t fs) {
    return kind == 0 ? scalar : (kind == 1 ? src[idx % fs] : src[idx]);
}

__global__ void k_ls_init(double* dx, double* dy, const double* ix, const double* iy, double sx, double sy, int kind, size_t fs, size_t n,
                          double delta_t, double delta_x) {
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const double x = ls_initial(ix, sx, kind, idx, fs), y = ls_initial(iy, sy, kind, idx, fs);
    dx[idx] = (x * delta_t) / delta_x;          // OF.py:505-506
    dy[idx] = (y * delta_t) / delta_x;
}

// OF.py:670-672; rem == nullptr: the remodelling plane is not written
__global__ void k_ls_finish(const double* sx, const double* sy, double* vx, double* vy, double* speed, double* rem, const double* irem,
                            double srem, int kind, size_t fs, size_t n, double scale) {
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const double x = sx[idx] * scale, y = sy[idx] * scale;
    const double r = rem ? ls_initial(irem, srem, kind, idx, fs) : 0.0;
    vx[idx] = x;
    vy[idx] = y;
    speed[idx] = __dsqrt_rn(x * x + y * y);
    if (rem) rem[idx] = r;
}

}  // namespace vof
