// vof_boxflow.hpp - box least-squares flow (conduct_optical_flow, OF.py:24-218; Vig et al. 2016) on gfx950.
//
// Per frame pair (p = frame k, c = frame k + 1) three derived planes
//   dIdx = (c[i+1] + p[i+1] - c[i-1] - p[i-1]) / 4, dIdy likewise along j (both zero on the border lines), dI = c - p,
// five (eight with the net-remodelling term) products of them summed over the (2h+1) x (2h+1) window of every pixel, the
// window clipped at the image edge, and a closed-form 2 x 2 / 3 x 3 solve per pixel.  A window clipped at row / column
// bounds is the full window over planes that are ZERO outside the bounds, so the derived planes are written with zeros
// outside [0, N_i) x [0, cend) (cend = min(N_i, N_j) with the reference's column clamp OF.py:108, N_j without) and every
// sum runs over all (2h+1)^2 offsets.  Sums are direct sums (rows first, then columns of row sums), never running windows.
//
// Two paths:
//   k_boxflow_fused   h <= 15: one launch, derived planes and row sums live in LDS only; per pixel and pair it has to move
//                     one frame in and 3 (4) planes out
//   k_bf_derived / k_bf_hsum / k_bf_vsum   any h: the same three stages through device scratch planes
// Arithmetic of the closed forms: the reference's operation order, every operation explicit, contraction off, IEEE
// division and square root (integer-valued movies reproduce the reference's v_x, v_y, net_remodelling bit for bit).
#pragma once
#include <hip/hip_runtime.h>
#include "vof_shared.hpp"

namespace vof {

constexpr int BF_TI = 32, BF_TJ = 32;        // output tile of the fused kernel; BF_TI * BF_TJ threads, one pixel each
constexpr int BF_THREADS = BF_TI * BF_TJ;
constexpr int BF_HMAX = 15;                  // largest half box of the fused kernel (box sizes up to 31)

struct BoxArgs {
    const double* movie;   // frame 0 of the first pair of the launch; pair z is (frame z, frame z + 1)
    size_t fs;             // doubles per frame
    int Ni, Nj, h;
    int cend;              // columns >= cend belong to no window
    int quirks;            // 1: n = box_size^2, remodelling mode leaves speed and singular pixels zero
    double n_box;          // box_size^2
    double scale;          // delta_x / delta_t
    double *vx, *vy, *speed, *gamma;   // (pairs, Ni, Nj); gamma may be nullptr without remodelling
};

// dynamic LDS of the fused kernel: three derived planes of the tile + halo (odd pitch) and one plane of row sums
inline size_t bf_fused_lds(int h) {
    const size_t RI = BF_TI + 2 * h, RJ = BF_TJ + 2 * h, pitch = RJ | 1;
    return (3 * RI * pitch + RI * BF_TJ) * sizeof(double);
}

__device__ __forceinline__ void bf_derived_at(const double* __restrict__ c, const double* __restrict__ p, int Ni, int Nj, int cend,
                                              int i, int j, double& dx, double& dy, double& dI) {
#pragma clang fp contract(off)
    dx = 0.0; dy = 0.0; dI = 0.0;
    if (i < 0 || i >= Ni || j < 0 || j >= cend) return;
    const size_t o = (size_t)i * Nj + j;
    dI = c[o] - p[o];
    if (i >= 1 && i < Ni - 1 && j >= 1 && j < Nj - 1) {
        dx = (((c[o + Nj] + p[o + Nj]) - c[o - Nj]) - p[o - Nj]) / 4.0;
        dy = (((c[o + 1] + p[o + 1]) - c[o - 1]) - p[o - 1]) / 4.0;
    }
}

// quantity Q of one pixel: 0 dx^2, 1 dx dy, 2 dy^2, 3 dI dx, 4 dI dy, 5 dx, 6 dy, 7 dI
template <int Q>
__device__ __forceinline__ double bf_term(const double* dx, const double* dy, const double* dI, size_t o) {
#pragma clang fp contract(off)
    if (Q == 0) { const double a = dx[o]; return a * a; }
    if (Q == 1) return dx[o] * dy[o];
    if (Q == 2) { const double a = dy[o]; return a * a; }
    if (Q == 3) return dI[o] * dx[o];
    if (Q == 4) return dI[o] * dy[o];
    if (Q == 5) return dx[o];
    if (Q == 6) return dy[o];
    return dI[o];
}

// pixels of the clipped window of (i, j) without the reference's quirks
__device__ __forceinline__ double bf_window_count(int i, int j, int h, int Ni, int Nj) {
    const int ri = min(i + h + 1, Ni) - max(i - h, 0), rj = min(j + h + 1, Nj) - max(j - h, 0);
    return (double)ri * (double)rj;
}

// S: the window sums in the order of bf_term.  The pixel's unscaled results (OF.py:119-155 in the reference's operation order).
template <bool REMODEL>
__device__ __forceinline__ void bf_solve(const double* S, int quirks, double n, double& Vx, double& Vy, double& sp, double& g) {
#pragma clang fp contract(off)
    if (!REMODEL) {
        const double A = S[0], B = S[1], C = S[2], s1 = S[3], s2 = S[4];
        const double det = A * C - B * B;
        Vx = ((-C) * s1 + B * s2) / det;
        Vy = ((-A) * s2 + B * s1) / det;
        sp = __dsqrt_rn(Vx * Vx + Vy * Vy);
        g = 0.0;
    } else {
        const double A = S[0], B = S[1], D = S[2], s1 = S[3], s2 = S[4], C = S[5], E = S[6], s3 = S[7];
        const double de = ((((n * A) * D - A * (E * E)) - n * (B * B)) - (C * C) * D) + ((2.0 * B) * C) * E;
        Vx = 0.0; Vy = 0.0; g = 0.0; sp = 0.0;
        if (de == 0.0) {
            if (!quirks) { Vx = Vy = g = sp = __builtin_nan(""); }
        } else {
            const double nBCE = n * B - C * E;
            Vx = (((E * E - n * D) * s1 + nBCE * s2) + (C * D - B * E) * s3) / de;
            Vy = ((nBCE * s1 + (C * C - n * A) * s2) + (A * E - B * C) * s3) / de;
            g = -((((B * E - C * D) * s1 + (B * C - A * E) * s2) + (A * D - B * B) * s3) / de);
            if (!quirks) sp = __dsqrt_rn(Vx * Vx + Vy * Vy);
        }
    }
}

// Writes the pixel's results: v_x, v_y, speed in delta_x / delta_t units, net_remodelling unscaled.
template <bool REMODEL>
__device__ __forceinline__ void bf_solve_store(const double* S, const BoxArgs& a, double n, size_t o) {
#pragma clang fp contract(off)
    double Vx, Vy, sp, g;
    bf_solve<REMODEL>(S, a.quirks, n, Vx, Vy, sp, g);
    a.vx[o] = Vx * a.scale;
    a.vy[o] = Vy * a.scale;
    a.speed[o] = sp * a.scale;
    if (REMODEL || a.gamma) a.gamma[o] = g;
}

// ---- fused kernel ---------------------------------------------------------------------------------------------
// One quantity: row sums of the tile's RI rows into hs (barrier), then the column sum of this thread's pixel.
template <int Q>
__device__ __forceinline__ double bf_fused_quantity(const double* sdx, const double* sdy, const double* sdI, double* hs, int h, int RI,
                                                    int pitch, int tid) {
#pragma clang fp contract(off)
    const int w = 2 * h + 1;
    for (int idx = tid; idx < RI * BF_TJ; idx += BF_THREADS) {
        const int r = idx / BF_TJ, t = idx - r * BF_TJ;
        const size_t o = (size_t)r * pitch + t;
        double s = 0.0;
        for (int d = 0; d < w; ++d) s += bf_term<Q>(sdx, sdy, sdI, o + d);
        hs[idx] = s;
    }
    __syncthreads();
    const int ti = tid / BF_TJ, tj = tid - ti * BF_TJ;
    double s = 0.0;
    for (int d = 0; d < w; ++d) s += hs[(ti + d) * BF_TJ + tj];
    __syncthreads();     // hs is overwritten by the next quantity
    return s;
}

template <bool REMODEL>
__global__ __launch_bounds__(BF_THREADS) void k_boxflow_fused(BoxArgs a) {
    extern __shared__ double bf_lds[];
    const int h = a.h, RI = BF_TI + 2 * h, RJ = BF_TJ + 2 * h, pitch = RJ | 1;
    double* sdx = bf_lds;
    double* sdy = sdx + (size_t)RI * pitch;
    double* sdI = sdy + (size_t)RI * pitch;
    double* hs = sdI + (size_t)RI * pitch;
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * BF_TI, j0 = blockIdx.x * BF_TJ;
    const double* p = a.movie + (size_t)blockIdx.z * a.fs;
    const double* c = p + a.fs;
    for (int idx = tid; idx < RI * RJ; idx += BF_THREADS) {
        const int r = idx / RJ, t = idx - r * RJ;
        double dx, dy, dI;
        bf_derived_at(c, p, a.Ni, a.Nj, a.cend, i0 - h + r, j0 - h + t, dx, dy, dI);
        const size_t o = (size_t)r * pitch + t;
        sdx[o] = dx; sdy[o] = dy; sdI[o] = dI;
    }
    __syncthreads();
    double S[REMODEL ? 8 : 5];
    S[0] = bf_fused_quantity<0>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
    S[1] = bf_fused_quantity<1>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
    S[2] = bf_fused_quantity<2>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
    S[3] = bf_fused_quantity<3>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
    S[4] = bf_fused_quantity<4>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
    if (REMODEL) {
        S[5] = bf_fused_quantity<5>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
        S[6] = bf_fused_quantity<6>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
        S[7] = bf_fused_quantity<7>(sdx, sdy, sdI, hs, h, RI, pitch, tid);
    }
    const int ti = tid / BF_TJ, tj = tid - ti * BF_TJ;
    const int i = i0 + ti, j = j0 + tj;
    if (i >= a.Ni || j >= a.Nj) return;
    BoxArgs out = a;
    const size_t po = (size_t)blockIdx.z * a.fs;
    out.vx += po; out.vy += po; out.speed += po;
    if (out.gamma) out.gamma += po;
    const double n = a.quirks ? a.n_box : bf_window_count(i, j, h, a.Ni, a.Nj);
    bf_solve_store<REMODEL>(S, out, n, (size_t)i * a.Nj + j);
}

// ---- general path: the same stages through device scratch planes (any h) -----------------------------------------
// der: [pair][3][Ni][Nj] (dx, dy, dI)
__global__ void k_bf_derived(BoxArgs a, double* __restrict__ der) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= a.Ni || j >= a.Nj) return;
    const double* p = a.movie + (size_t)blockIdx.z * a.fs;
    double dx, dy, dI;
    bf_derived_at(p + a.fs, p, a.Ni, a.Nj, a.cend, i, j, dx, dy, dI);
    double* d = der + (size_t)blockIdx.z * 3 * a.fs + (size_t)i * a.Nj + j;
    d[0] = dx; d[a.fs] = dy; d[2 * a.fs] = dI;
}

template <int Q>
__device__ __forceinline__ double bf_row_sum(const double* dx, const double* dy, const double* dI, size_t row, int jl, int ju) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int jj = jl; jj <= ju; ++jj) s += bf_term<Q>(dx, dy, dI, row + jj);
    return s;
}

// rows: [pair][NQ][Ni][Nj], row sums over the columns max(j - h, 0) .. min(j + h, Nj - 1)
template <bool REMODEL>
__global__ void k_bf_hsum(BoxArgs a, const double* __restrict__ der, double* __restrict__ rows) {
    constexpr int NQ = REMODEL ? 8 : 5;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= a.Ni || j >= a.Nj) return;
    const double* dx = der + (size_t)blockIdx.z * 3 * a.fs;
    const double* dy = dx + a.fs;
    const double* dI = dy + a.fs;
    const int jl = max(j - a.h, 0), ju = (int)min((long long)j + a.h, (long long)a.Nj - 1);
    const size_t row = (size_t)i * a.Nj;
    double* out = rows + (size_t)blockIdx.z * NQ * a.fs + row + j;
    out[0] = bf_row_sum<0>(dx, dy, dI, row, jl, ju);
    out[a.fs] = bf_row_sum<1>(dx, dy, dI, row, jl, ju);
    out[2 * a.fs] = bf_row_sum<2>(dx, dy, dI, row, jl, ju);
    out[3 * a.fs] = bf_row_sum<3>(dx, dy, dI, row, jl, ju);
    out[4 * a.fs] = bf_row_sum<4>(dx, dy, dI, row, jl, ju);
    if (REMODEL) {
        out[5 * a.fs] = bf_row_sum<5>(dx, dy, dI, row, jl, ju);
        out[6 * a.fs] = bf_row_sum<6>(dx, dy, dI, row, jl, ju);
        out[7 * a.fs] = bf_row_sum<7>(dx, dy, dI, row, jl, ju);
    }
}

// column sums of the row sums over the rows max(i - h, 0) .. min(i + h, Ni - 1), closed form, store
template <bool REMODEL>
__global__ void k_bf_vsum(BoxArgs a, const double* __restrict__ rows) {
#pragma clang fp contract(off)
    constexpr int NQ = REMODEL ? 8 : 5;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= a.Ni || j >= a.Nj) return;
    const int il = max(i - a.h, 0), iu = (int)min((long long)i + a.h, (long long)a.Ni - 1);
    const double* r = rows + (size_t)blockIdx.z * NQ * a.fs + j;
    double S[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double s = 0.0;
        for (int ii = il; ii <= iu; ++ii) s += r[(size_t)q * a.fs + (size_t)ii * a.Nj];
        S[q] = s;
    }
    BoxArgs out = a;
    const size_t po = (size_t)blockIdx.z * a.fs;
    out.vx += po; out.vy += po; out.speed += po;
    if (out.gamma) out.gamma += po;
    const double n = a.quirks ? a.n_box : bf_window_count(i, j, a.h, a.Ni, a.Nj);
    bf_solve_store<REMODEL>(S, out, n, (size_t)i * a.Nj + j);
}

}  // namespace vof
