// vof_intensity.hpp - the illumination correction of the reference's real-data scripts (correct_intensity_change,
// analyse_short_timeinterval_data.py:241-301 and 128-145) and the per-frame intensity histograms they judge it by
// (investigate_intensities, compare_rho_and_actin.py:98-118) on gfx950.  DESIGN.md section 18.
//
// The correction of frame k against the reference frame, B the (optionally) blurred movie, G the blur of vof_blur_stack_*:
//   D = B[k] - B[ref];  E = G(D, filter_size);  out = Tg[k] - E,  Tg = B or the movie.
// Made of the existing passes that is blur (4 planes), difference (3), blur (4), subtraction (3).  Here the difference is formed
// by the loader of the second blur's axis-0 pass and the subtraction by the store of its axis-1 pass: 4 + 3 + 3 planes, and
// neither D nor E exists as a stack.  The subtractions are single IEEE operations and the accumulation is k_blur1d's - centre
// tap first, then k = -radius .. -1 as acc += (a + b) * w[k + radius], no FMA - so the bits are those of the unfused chain.
#pragma once
#include <hip/hip_runtime.h>
#include "vof_shared.hpp"
#include "vof_farneback.hpp"

namespace vof {

// profiler stages of VOF_K_PREPROCESS, after those of vof_farneback.hpp.  The profiler keeps 16 slots per class and the class had
// used them all: a launch scope carries its own number (VOF_DEBUG_SYNC names it), the recorder sums what lies above 15 in slot 15.
enum { PP_ST_IC_AXIS0 = PP_ST_FB_BOX_UPDATE + 1, PP_ST_IC_AXIS1, PP_ST_IH_COUNTS };

// ---- axis 0: blur along the rows of b[frame] - ref, the difference formed while the tile is filled ---------------------------
// The tile of k_blur1d_tiled<0>, tile[BL_TI + 2 r][BX] (blur_tiled_lds(0, radius), 80 KiB at BL_RMAX: the limit is raised for this
// kernel by every call that takes it), the same clamped halo rows; an element costs two global reads.  Lanes past N_j load the last column and store
// nothing; an image of fewer rows than the radius clamps on both sides inside the one tile.
__global__ __launch_bounds__(NT) void k_ic_axis0_tiled(const double* __restrict__ b, const double* __restrict__ ref, double* __restrict__ out,
                                                       int Ni, int Nj, const double* __restrict__ w, int radius) {
#pragma clang fp contract(off)
    extern __shared__ double tile[];
    const double* src = b + (size_t)blockIdx.z * Ni * Nj;
    double* dst = out + (size_t)blockIdx.z * Ni * Nj;
    const int j0 = blockIdx.x * BX, j = j0 + threadIdx.x;
    const int i0 = blockIdx.y * BL_TI, nout = min(BL_TI, Ni - i0);
    const int jc = min(j, Nj - 1);
    for (int r = threadIdx.y; r < nout + 2 * radius; r += BY) {
        const size_t o = (size_t)min(max(i0 - radius + r, 0), Ni - 1) * Nj + jc;
        tile[r * BX + threadIdx.x] = src[o] - ref[o];
    }
    __syncthreads();
    if (j >= Nj) return;
    for (int t = threadIdx.y; t < nout; t += BY) {
        const double* p = tile + (t + radius) * BX + threadIdx.x;
        double acc = p[0] * w[radius];
        for (int k = -radius; k < 0; ++k) acc += (p[k * BX] + p[-k * BX]) * w[k + radius];
        dst[(size_t)(i0 + t) * Nj + j] = acc;
    }
}

// the same out of global memory, for the radii the tile does not serve (k_blur1d<0> with the difference in its loads)
__global__ __launch_bounds__(NT) void k_ic_axis0(const double* __restrict__ b, const double* __restrict__ ref, double* __restrict__ out,
                                                 int Ni, int Nj, const double* __restrict__ w, int radius) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (i >= Ni || j >= Nj) return;
    const double* src = b + (size_t)blockIdx.z * Ni * Nj;
    const size_t o = (size_t)i * Nj + j;
    double acc = (src[o] - ref[o]) * w[radius];
    for (int k = -radius; k < 0; ++k) {
        const size_t oa = (size_t)min(max(i + k, 0), Ni - 1) * Nj + j, ob = (size_t)min(max(i - k, 0), Ni - 1) * Nj + j;
        const double a = src[oa] - ref[oa], bb = src[ob] - ref[ob];
        acc += (a + bb) * w[k + radius];
    }
    out[(size_t)blockIdx.z * Ni * Nj + o] = acc;
}

// ---- axis 1: blur along the columns of `mid`; the store is target - acc, and acc itself where the drift is asked for ---------
// The tile of k_blur1d_tiled<1>, tile[BL_TR][BX + 2 r].  `out` and `drift` alias neither `mid` nor `target`.
template <bool DRIFT>
__global__ __launch_bounds__(NT) void k_ic_axis1_tiled(const double* __restrict__ mid, const double* __restrict__ target, double* __restrict__ out,
                                                       double* __restrict__ drift, int Ni, int Nj, const double* __restrict__ w, int radius) {
#pragma clang fp contract(off)
    extern __shared__ double tile[];
    const size_t f = (size_t)blockIdx.z * Ni * Nj;
    const int j0 = blockIdx.x * BX, j = j0 + threadIdx.x;
    const int i0 = blockIdx.y * BL_TR, nrow = min(BL_TR, Ni - i0);
    const int pitch = BX + 2 * radius, ncol = min(BX, Nj - j0) + 2 * radius;
    for (int t = threadIdx.y; t < nrow; t += BY) {
        const double* row = mid + f + (size_t)(i0 + t) * Nj;
        for (int cc = threadIdx.x; cc < ncol; cc += BX) tile[t * pitch + cc] = row[min(max(j0 - radius + cc, 0), Nj - 1)];
    }
    __syncthreads();
    if (j >= Nj) return;
    for (int t = threadIdx.y; t < nrow; t += BY) {
        const double* p = tile + t * pitch + radius + threadIdx.x;
        double acc = p[0] * w[radius];
        for (int k = -radius; k < 0; ++k) acc += (p[k] + p[-k]) * w[k + radius];
        const size_t o = f + (size_t)(i0 + t) * Nj + j;
        out[o] = target[o] - acc;
        if (DRIFT) drift[o] = acc;
    }
}

template <bool DRIFT>
__global__ __launch_bounds__(NT) void k_ic_axis1(const double* __restrict__ mid, const double* __restrict__ target, double* __restrict__ out,
                                                 double* __restrict__ drift, int Ni, int Nj, const double* __restrict__ w, int radius) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (i >= Ni || j >= Nj) return;
    const size_t f = (size_t)blockIdx.z * Ni * Nj;
    const double* row = mid + f + (size_t)i * Nj;
    double acc = row[j] * w[radius];
    for (int k = -radius; k < 0; ++k) acc += (row[min(max(j + k, 0), Nj - 1)] + row[min(max(j - k, 0), Nj - 1)]) * w[k + radius];
    const size_t o = f + (size_t)i * Nj + j;
    out[o] = target[o] - acc;
    if (DRIFT) drift[o] = acc;
}

// ---- np.histogram of every frame in flight -------------------------------------------------------------------------------------
// k_bs_counts per frame: the frame is blockIdx.y, its fs doubles are shared by the gridDim.x blocks of that row.  hist[frame][bins]
// += counts (bs_bin_of against the np.linspace edges passed in: last bin closed on the right, NaN and values outside dropped),
// nonfinite[frame] += NaN / Inf values.  Counters live in LDS up to BS_LDS_BINS bins and go straight to global memory above;
// integer atomics only, so no count depends on the order of the blocks.
constexpr int IH_BLOCK = 256;
constexpr int IH_PER_THREAD = 8;         // values a thread counts at least before a frame gets another block ...
constexpr int IH_MAX_BLOCKS = 128;       // ... up to this many blocks per frame
constexpr int IH_MAX_BINS = 1 << 20;     // 8 MiB of counters per frame in flight

__global__ __launch_bounds__(IH_BLOCK) void k_ih_counts(const double* __restrict__ x, size_t fs, const double* __restrict__ edges, int bins,
                                                        unsigned long long* __restrict__ hist, unsigned long long* __restrict__ nonfinite) {
    __shared__ unsigned int lh[BS_LDS_BINS];
    __shared__ unsigned int lbad;
    const bool lds = bins <= BS_LDS_BINS;
    if (lds) for (int b = threadIdx.x; b < bins; b += IH_BLOCK) lh[b] = 0u;
    if (threadIdx.x == 0) lbad = 0u;
    __syncthreads();
    const double* xf = x + (size_t)blockIdx.y * fs;
    unsigned long long* hf = hist + (size_t)blockIdx.y * bins;
    unsigned int bad = 0u;
    for (size_t k = (size_t)blockIdx.x * IH_BLOCK + threadIdx.x; k < fs; k += (size_t)gridDim.x * IH_BLOCK) {
        const double v = xf[k];
        if (!(fabs(v) <= 1.7976931348623157e308)) ++bad;
        const int b = bs_bin_of(v, edges, bins);
        if (b >= 0) {
            if (lds) atomicAdd(&lh[b], 1u);
            else atomicAdd(&hf[b], 1ull);
        }
    }
    if (bad) atomicAdd(&lbad, bad);
    __syncthreads();
    if (lds)
        for (int b = threadIdx.x; b < bins; b += IH_BLOCK)
            if (lh[b]) atomicAdd(&hf[b], (unsigned long long)lh[b]);
    if (threadIdx.x == 0 && lbad) atomicAdd(&nonfinite[blockIdx.y], (unsigned long long)lbad);
}

}  // namespace vof
