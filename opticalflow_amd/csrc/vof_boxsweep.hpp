// vof_boxsweep.hpp - the box-size sweep of the box least-squares flow (vary_boxsize; the reference's scripts loop
// conduct_optical_flow over 50 - 73 box sizes) on gfx950.
//
// Per pair the three derived planes of vof_boxflow.hpp are computed once and the window of every pixel grows by one ring
// per step, so a box size costs O(1) per pixel instead of O(box).  With t the per-pixel term of a quantity (bf_term over
// the zero-extended derived planes) three accumulator planes per quantity, all 0.0 + t at h = 0:
//   R_h(i, j) = (R_{h-1} + t(i, j-h)) + t(i, j+h)          row sums
//   C_h(i, j) = (C_{h-1} + t(i-h, j)) + t(i+h, j)          column sums
//   W_h       = (((W_{h-1} + R_h(i-h, j)) + R_h(i+h, j)) + C_{h-1}(i, j-h)) + C_{h-1}(i, j+h)
// reads outside the image being 0.  Terms are only ever added to float64 accumulators: no running windows, no summed-area
// tables, nothing is subtracted.  The chain always starts at h = 0, so a box's fields do not depend on the other boxes.
//
// Two launches per h, so that no launch reads a plane one of its own threads writes:
//   k_bs_grow    R -> R_h, C -> C_{h-1}: pointwise, reads the derived planes only
//   k_bs_window  W -> W_h in place from R and C; on a requested h the closed form of vof_boxflow.hpp (bf_solve) and the stores
// Both are pure streaming: contiguous reads shifted by +-h rows or +-h columns.
#pragma once
#include <hip/hip_runtime.h>
#include "vof_boxflow.hpp"

namespace vof {

struct SweepArgs {
    const double* der;     // [pair][3][fs]: dx, dy, dI (k_bf_derived)
    double *R, *C, *W;     // [pair][NQ][fs] each
    size_t fs;
    int Ni, Nj, h;
};

template <int Q>
__device__ __forceinline__ void bs_init_q(const SweepArgs& s, const double* dx, const double* dy, const double* dI, size_t acc, size_t o) {
#pragma clang fp contract(off)
    const double v = 0.0 + bf_term<Q>(dx, dy, dI, o);     // as the first step of a direct sum
    const size_t a = acc + (size_t)Q * s.fs + o;
    s.R[a] = v; s.C[a] = v; s.W[a] = v;
}

// h = 0: every accumulator is the pixel's own term
template <bool REMODEL>
__global__ void k_bs_init(SweepArgs s) {
    constexpr int NQ = REMODEL ? 8 : 5;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= s.Ni || j >= s.Nj) return;
    const double* dx = s.der + (size_t)blockIdx.z * 3 * s.fs;
    const double* dy = dx + s.fs;
    const double* dI = dy + s.fs;
    const size_t o = (size_t)i * s.Nj + j, acc = (size_t)blockIdx.z * NQ * s.fs;
    bs_init_q<0>(s, dx, dy, dI, acc, o);
    bs_init_q<1>(s, dx, dy, dI, acc, o);
    bs_init_q<2>(s, dx, dy, dI, acc, o);
    bs_init_q<3>(s, dx, dy, dI, acc, o);
    bs_init_q<4>(s, dx, dy, dI, acc, o);
    if (REMODEL) {
        bs_init_q<5>(s, dx, dy, dI, acc, o);
        bs_init_q<6>(s, dx, dy, dI, acc, o);
        bs_init_q<7>(s, dx, dy, dI, acc, o);
    }
}

// lf / rt / up / dn: the pixel h columns to the left / right, g = h - 1 rows up / down lies inside the image
template <int Q>
__device__ __forceinline__ void bs_grow_q(const SweepArgs& s, const double* dx, const double* dy, const double* dI, size_t acc, size_t o,
                                          bool lf, bool rt, bool up, bool dn, size_t gr) {
#pragma clang fp contract(off)
    const size_t a = acc + (size_t)Q * s.fs + o;
    double r = s.R[a];
    r = r + (lf ? bf_term<Q>(dx, dy, dI, o - s.h) : 0.0);
    r = r + (rt ? bf_term<Q>(dx, dy, dI, o + s.h) : 0.0);
    s.R[a] = r;
    if (s.h >= 2) {
        double c = s.C[a];
        c = c + (up ? bf_term<Q>(dx, dy, dI, o - gr) : 0.0);
        c = c + (dn ? bf_term<Q>(dx, dy, dI, o + gr) : 0.0);
        s.C[a] = c;
    }
}

// step h >= 1, first launch: R_{h-1} -> R_h and C_{h-2} -> C_{h-1}
template <bool REMODEL>
__global__ void k_bs_grow(SweepArgs s) {
    constexpr int NQ = REMODEL ? 8 : 5;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= s.Ni || j >= s.Nj) return;
    const double* dx = s.der + (size_t)blockIdx.z * 3 * s.fs;
    const double* dy = dx + s.fs;
    const double* dI = dy + s.fs;
    const size_t o = (size_t)i * s.Nj + j, acc = (size_t)blockIdx.z * NQ * s.fs;
    const int g = s.h - 1;
    const bool lf = j - s.h >= 0, rt = j + s.h < s.Nj, up = i - g >= 0, dn = i + g < s.Ni;
    const size_t gr = (size_t)g * s.Nj;
    bs_grow_q<0>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
    bs_grow_q<1>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
    bs_grow_q<2>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
    bs_grow_q<3>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
    bs_grow_q<4>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
    if (REMODEL) {
        bs_grow_q<5>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
        bs_grow_q<6>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
        bs_grow_q<7>(s, dx, dy, dI, acc, o, lf, rt, up, dn, gr);
    }
}

// step h >= 1, second launch (STEP): W_{h-1} -> W_h in place from R_h and C_{h-1}, which this launch only reads.
// SOLVE: the closed form with the window sums W_h and the stores; a.h is the half box, a.vx / a.vy / a.gamma may be nullptr
// (stats-only sweeps keep speed, and net_remodelling with REMODEL, of the pairs in flight only).
template <bool REMODEL, bool STEP, bool SOLVE>
__global__ void k_bs_window(SweepArgs s, BoxArgs a) {
#pragma clang fp contract(off)
    constexpr int NQ = REMODEL ? 8 : 5;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= s.Ni || j >= s.Nj) return;
    const size_t o = (size_t)i * s.Nj + j, acc = (size_t)blockIdx.z * NQ * s.fs + o;
    const int h = s.h;
    const bool up = i - h >= 0, dn = i + h < s.Ni, lf = j - h >= 0, rt = j + h < s.Nj;
    const size_t hr = (size_t)h * s.Nj;
    double S[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const size_t p = acc + (size_t)q * s.fs;
        double w = s.W[p];
        if (STEP) {
            w = w + (up ? s.R[p - hr] : 0.0);
            w = w + (dn ? s.R[p + hr] : 0.0);
            w = w + (lf ? s.C[p - h] : 0.0);
            w = w + (rt ? s.C[p + h] : 0.0);
            s.W[p] = w;
        }
        S[q] = w;
    }
    if (SOLVE) {
        const double n = a.quirks ? a.n_box : bf_window_count(i, j, a.h, a.Ni, a.Nj);
        double Vx, Vy, sp, g;
        bf_solve<REMODEL>(S, a.quirks, n, Vx, Vy, sp, g);
        const size_t po = (size_t)blockIdx.z * s.fs + o;
        if (a.vx) a.vx[po] = Vx * a.scale;
        if (a.vy) a.vy[po] = Vy * a.scale;
        a.speed[po] = sp * a.scale;
        if (a.gamma) a.gamma[po] = g;
    }
}

// ---- statistics of one box over the pairs in flight -----------------------------------------------------------------
// hist (bins counters, or nullptr) += counts of x[0 .. n); *nonfinite += number of NaN / Inf values.  Integer atomics only:
// the result does not depend on the order of the blocks.
__global__ __launch_bounds__(256) void k_bs_counts(const double* __restrict__ x, size_t n, const double* __restrict__ edges, int bins,
                                                   unsigned long long* __restrict__ hist, unsigned long long* __restrict__ nonfinite) {
    __shared__ unsigned int lh[BS_LDS_BINS];
    __shared__ unsigned int lbad;
    const bool lds = hist && bins <= BS_LDS_BINS;
    if (lds) for (int b = threadIdx.x; b < bins; b += blockDim.x) lh[b] = 0u;
    if (threadIdx.x == 0) lbad = 0u;
    __syncthreads();
    unsigned int bad = 0u;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        const double v = x[k];
        if (!(fabs(v) <= 1.7976931348623157e308)) ++bad;
        if (hist) {
            const int b = bs_bin_of(v, edges, bins);
            if (b >= 0) {
                if (lds) atomicAdd(&lh[b], 1u);
                else atomicAdd(&hist[b], 1ull);
            }
        }
    }
    if (bad) atomicAdd(&lbad, bad);
    __syncthreads();
    if (lds)
        for (int b = threadIdx.x; b < bins; b += blockDim.x)
            if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
    if (threadIdx.x == 0 && lbad) atomicAdd(nonfinite, (unsigned long long)lbad);
}

// out[pair][l] = speed[pair][probe_ij[2 l]][probe_ij[2 l + 1]]
__global__ void k_bs_probe(const double* __restrict__ speed, size_t fs, int Nj, int pairs, const int* __restrict__ probe_ij, int n_probes,
                           double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pairs * n_probes) return;
    const int k = t / n_probes, l = t - k * n_probes;
    out[t] = speed[(size_t)k * fs + (size_t)probe_ij[2 * l] * Nj + probe_ij[2 * l + 1]];
}

}  // namespace vof
