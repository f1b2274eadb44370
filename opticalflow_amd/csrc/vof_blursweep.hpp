// vof_blursweep.hpp - the blur sweep of the box least-squares flow (vary_blursize; the reference's scripts loop
// conduct_optical_flow over 145 values of smoothing_sigma, compare_rho_and_actin.py:485-614) on gfx950: the LDS-tiled form of
// the separable blur and the flow-direction statistics.  The flow itself is the one of vof_boxflow.hpp, the speed statistics
// those of vof_boxsweep.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "vof_boxsweep.hpp"

namespace vof {

// ---- k_blur1d out of LDS ----------------------------------------------------------------------------------------------
// k_blur1d reads its 2 r + 1 taps per pixel from global memory; radius = int(4 sigma + 0.5) reaches 60 in the sweep.  Here a
// workgroup of BX x BY threads loads its output tile and `radius` halo rows (AXIS 0) or columns (AXIS 1) on either side once,
// edge indices clamped as in k_blur1d, and accumulates every output out of LDS in k_blur1d's order: centre tap first, then
// k = -radius .. -1 as acc += (a + b) * w[k + radius], no FMA.  Same values in the same order: same bits.
//   AXIS 0: tile[BL_TI + 2 r][BX]; lane = column, so a wave reads 64 consecutive doubles of one LDS row per tap: each 32-lane
//           half of a ds_read_b64 covers the 64 banks once, conflict-free.
//   AXIS 1: tile[BL_TR][BX + 2 r]; lane = column again, the taps shift the whole wave along the row: conflict-free for any pitch.
// Dynamic LDS: blur_tiled_lds(axis, radius), at most 80 KiB (AXIS 0 at BL_RMAX), so that two workgroups still share the
// 160 KiB of a CU; the limit of the AXIS 0 kernel is raised once per context.  The sweep's largest radius is 60 (sigma 15);
// above BL_RMAX k_blur1d stays the path.

// ==========================================================================================
// Gaussian blur of the frames (OF.py:282-306: skimage.filters.gaussian == scipy.ndimage.gaussian_filter with
// mode='nearest', truncate=4): two 1-D correlations, axis 0 then axis 1, with edge clamping.  The summation order
// is the one of scipy's symmetric-kernel branch (NI_Correlate1D): centre tap first, then the mirrored pairs
// from the outside in, so results agree with the host filter to the last bit or two.
// ==========================================================================================
template <int AXIS>
__global__ __launch_bounds__(NT) void k_blur1d(const double* __restrict__ in, double* __restrict__ out, int Ni, int Nj,
                                               const double* __restrict__ w, int radius) {
#pragma clang fp contract(off)   // no FMA: the host filter rounds the product and the sum separately
    int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y, f = blockIdx.z;
    if (i >= Ni || j >= Nj) return;
    const double* src = in + (size_t)f * Ni * Nj;
    double acc = src[(size_t)i * Nj + j] * w[radius];
    for (int k = -radius; k < 0; ++k) {
        double a, b;
        if (AXIS == 0) {
            int ia = min(max(i + k, 0), Ni - 1), ib = min(max(i - k, 0), Ni - 1);
            a = src[(size_t)ia * Nj + j];
            b = src[(size_t)ib * Nj + j];
        } else {
            int ja = min(max(j + k, 0), Nj - 1), jb = min(max(j - k, 0), Nj - 1);
            a = src[(size_t)i * Nj + ja];
            b = src[(size_t)i * Nj + jb];
        }
        acc += (a + b) * w[k + radius];
    }
    out[(size_t)f * Ni * Nj + (size_t)i * Nj + j] = acc;
}

template <int AXIS>
__global__ __launch_bounds__(NT) void k_blur1d_tiled(const double* __restrict__ in, double* __restrict__ out, int Ni, int Nj,
                                                     const double* __restrict__ w, int radius) {
#pragma clang fp contract(off)   // as k_blur1d
    extern __shared__ double tile[];
    const double* src = in + (size_t)blockIdx.z * Ni * Nj;
    double* dst = out + (size_t)blockIdx.z * Ni * Nj;
    const int j0 = blockIdx.x * BX, j = j0 + threadIdx.x;
    if (AXIS == 0) {
        const int i0 = blockIdx.y * BL_TI, nout = min(BL_TI, Ni - i0);
        const int jc = min(j, Nj - 1);                 // lanes past the image load the last column and store nothing
        for (int r = threadIdx.y; r < nout + 2 * radius; r += BY)
            tile[r * BX + threadIdx.x] = src[(size_t)min(max(i0 - radius + r, 0), Ni - 1) * Nj + jc];
        __syncthreads();
        if (j >= Nj) return;
        for (int t = threadIdx.y; t < nout; t += BY) {
            const double* p = tile + (t + radius) * BX + threadIdx.x;
            double acc = p[0] * w[radius];
            for (int k = -radius; k < 0; ++k) acc += (p[k * BX] + p[-k * BX]) * w[k + radius];
            dst[(size_t)(i0 + t) * Nj + j] = acc;
        }
    } else {
        const int i0 = blockIdx.y * BL_TR, nrow = min(BL_TR, Ni - i0);
        const int pitch = BX + 2 * radius, ncol = min(BX, Nj - j0) + 2 * radius;
        for (int t = threadIdx.y; t < nrow; t += BY) {
            const double* row = src + (size_t)(i0 + t) * Nj;
            for (int cc = threadIdx.x; cc < ncol; cc += BX) tile[t * pitch + cc] = row[min(max(j0 - radius + cc, 0), Nj - 1)];
        }
        __syncthreads();
        if (j >= Nj) return;
        for (int t = threadIdx.y; t < nrow; t += BY) {
            const double* p = tile + t * pitch + radius + threadIdx.x;
            double acc = p[0] * w[radius];
            for (int k = -radius; k < 0; ++k) acc += (p[k] + p[-k]) * w[k + radius];
            dst[(size_t)(i0 + t) * Nj + j] = acc;
        }
    }
}

// ---- flow-direction statistics of one sigma over the pairs in flight ------------------------------------------------------
// a = acos(v_y / speed) * sign(v_x) / pi in float64, sign(0) = 0 (compare_rho_and_actin.py:560-563); a sample whose speed is
// not finite counts nowhere, NaN and values outside the edges are dropped as np.histogram drops them.
//   hist[b]  += number of samples in bin b (bs_bin_of against the np.linspace(-1, 1, bins + 1) edges): integer atomics.
//   partials[pair][block][b] = sum of speed over the block's samples in bin b, in a fixed shape: a workgroup is one wave, lane l
//     of block q adds the samples q * 64 + l, + gridDim.x * 64, ... of its pair in that order into a column of its own,
//     lw[b][l]; the 64 columns are then added by wave_sum's fixed tree.  gridDim.x depends on the plane size only, and
//     k_bz_angle_sum adds the blocks of a pair in block order, so a pair's sums do not depend on the launch that held it.
// No floating-point atomics.  Dynamic LDS: bins * 64 doubles, exactly 64 KiB at bins = BZ_MAX_ANGLE_BINS, next to the 512 B of
// static counters (lc): 66 048 B per workgroup, more than 64 KiB in all.  Observed on gfx950: the launch is accepted as it is, with
// no hipFuncSetAttribute for this kernel (the dynamic part alone does not exceed 64 KiB, and a CU has 160 KiB), and the counts and
// sums of 128 bins are those of numpy (tests/test_gpu_summary_launch_shapes.py).  A larger BZ_MAX_ANGLE_BINS needs the attribute.
constexpr int BZ_MAX_ANGLE_BINS = 128;
constexpr int BZ_ANGLE_PER_LANE = 32;    // samples a lane adds at least before a plane gets another block ...
constexpr int BZ_ANGLE_MAX_BLOCKS = 256; // ... up to this many blocks per pair

__global__ __launch_bounds__(64) void k_bz_angles(const double* __restrict__ vx, const double* __restrict__ vy,
                                                  const double* __restrict__ speed, size_t fs, const double* __restrict__ edges,
                                                  int bins, unsigned long long* __restrict__ hist, double* __restrict__ partials) {
#pragma clang fp contract(off)
    extern __shared__ double lw[];                      // [bins][64]
    __shared__ unsigned int lc[BZ_MAX_ANGLE_BINS];
    const int lane = threadIdx.x;
    for (int b = 0; b < bins; ++b) lw[b * 64 + lane] = 0.0;
    for (int b = lane; b < bins; b += 64) lc[b] = 0u;
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * fs;
    for (size_t k = (size_t)blockIdx.x * 64 + lane; k < fs; k += (size_t)gridDim.x * 64) {
        const double sp = speed[base + k], x = vx[base + k];
        if (!(fabs(sp) <= 1.7976931348623157e308) || x != x) continue;
        const double sgn = (double)(x > 0.0) - (double)(x < 0.0);
        const double a = acos(vy[base + k] / sp) * sgn / 3.141592653589793;
        const int b = bs_bin_of(a, edges, bins);
        if (b >= 0) {
            atomicAdd(&lc[b], 1u);
            lw[b * 64 + lane] += sp;
        }
    }
    __syncthreads();
    double* pp = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * bins;
    for (int b = 0; b < bins; ++b) {
        const double s = wave_sum(lw[b * 64 + lane]);
        if (lane == 0) pp[b] = s;
    }
    for (int b = lane; b < bins; b += 64)
        if (lc[b]) atomicAdd(&hist[b], (unsigned long long)lc[b]);
}

// out[pair][b] = ((partials[pair][0][b] + partials[pair][1][b]) + ...) in block order
__global__ void k_bz_angle_sum(const double* __restrict__ partials, int nblk, int bins, int pairs, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pairs * bins) return;
    const int pair = t / bins, b = t - pair * bins;
    double s = 0.0;
    for (int q = 0; q < nblk; ++q) s += partials[((size_t)pair * nblk + q) * bins + b];
    out[t] = s;
}

}  // namespace vof
