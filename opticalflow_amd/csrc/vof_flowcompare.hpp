// vof_flowcompare.hpp - what the reference does with two finished flow results (compare_flow_results, filter_PIV_flow_result;
// analyse_short_timeinterval_data.py:604-745 and OF.py:2232-2250) on gfx950: the mask of the result filter, and the two passes
// of the comparison over the six planes (v_x, v_y, speed of a and of b) of the pairs in flight.  DESIGN.md section 17.
#pragma once
#include <hip/hip_runtime.h>
#include "vof_shared.hpp"

namespace vof {

constexpr int FC_BLOCK = 256;
constexpr int FC_PER_LANE = 16;           // samples a lane takes at least before a plane gets another block ...
constexpr int FC_MAX_BLOCKS = 256;        // ... up to this many blocks per pair
constexpr int FC_UNROLL = 4;

// profiler stages of VOF_K_REDUCE (the `level` of vof_profile_get; 0 is every other reduction)
enum { FC_ST_MASK = 1, FC_ST_EXTREMES, FC_ST_HISTOGRAMS };

inline int fc_blocks(size_t fs) {          // by the plane size only
    const size_t n = fs / ((size_t)FC_BLOCK * FC_PER_LANE);
    return n < 1 ? 1 : (n > (size_t)FC_MAX_BLOCKS ? FC_MAX_BLOCKS : (int)n);
}

// ---- the result filter -------------------------------------------------------------------------------------------------
// Per sample of the frames in flight: low = blurred < intensity (NaN: false), fast = speed > limit on the incoming speed
// (NaN: false, +inf: true); v_x and v_y become 0.0 where low or fast, speed where fast - and where low too with zero_low (the
// reference leaves it).  Every other value is written back as it was read, NaN included.  The outputs may be the inputs: a
// lane reads its sample of every plane before it writes it, and no other lane touches that sample.  counts[0] += low samples,
// counts[1] += fast samples.  32 bytes read and 24 written per sample.
__global__ __launch_bounds__(FC_BLOCK) void k_fc_mask(const double* blurred, const double* vx, const double* vy, const double* sp, size_t n,
                                                      double intensity, double limit, int zero_low, double* ovx, double* ovy, double* osp,
                                                      unsigned long long* counts) {
    __shared__ unsigned int lcount[2];
    if (threadIdx.x < 2) lcount[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int n_low = 0u, n_fast = 0u;
    for (size_t k = (size_t)blockIdx.x * FC_BLOCK + threadIdx.x; k < n; k += (size_t)gridDim.x * FC_BLOCK) {
        const double b = blurred[k], x = vx[k], y = vy[k], s = sp[k];
        const bool low = b < intensity, fast = s > limit;
        n_low += low; n_fast += fast;
        ovx[k] = (low || fast) ? 0.0 : x;
        ovy[k] = (low || fast) ? 0.0 : y;
        osp[k] = (fast || (zero_low && low)) ? 0.0 : s;
    }
    if (n_low) atomicAdd(&lcount[0], n_low);
    if (n_fast) atomicAdd(&lcount[1], n_fast);
    __syncthreads();
    if (threadIdx.x < 2 && lcount[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)lcount[threadIdx.x]);
}

// ---- the comparison of two results ---------------------------------------------------------------------------------------
// Per sample, every operation explicit and uncontracted, in this order:
//   sa, sb = the two speeds with NaN replaced by 0 (nan_a, nan_b: which were);
//   infinite = sa or sb is +-inf: the sample takes no part below;
//   m1 = sa > speed_min and sb > speed_min      (the 2-D histogram of (sa, sb));
//   dot = v_x_b * v_x_a + v_y_b * v_y_a;  w = sb * sa;  cos = dot / w;  clipped to [-1, 1] with `clip` (NaN stays NaN);
//   theta = acos(cos), radians;
//   m2 = sa > angle_min and sb > angle_min      (the histogram of theta; a NaN theta under m2 is dropped and counted).
struct FcSample { double sa, sb, cs, theta; bool nan_a, nan_b, infinite, m1, m2; };

__device__ __forceinline__ FcSample fc_sample(double xa, double ya, double pa, double xb, double yb, double pb, double speed_min,
                                              double angle_min, int clip) {
#pragma clang fp contract(off)
    FcSample s;
    s.nan_a = pa != pa; s.nan_b = pb != pb;
    s.sa = s.nan_a ? 0.0 : pa; s.sb = s.nan_b ? 0.0 : pb;
    s.infinite = fabs(s.sa) > 1.7976931348623157e308 || fabs(s.sb) > 1.7976931348623157e308;
    s.m1 = !s.infinite && s.sa > speed_min && s.sb > speed_min;
    s.m2 = !s.infinite && s.sa > angle_min && s.sb > angle_min;
    const double dot = xb * xa + yb * ya;
    const double w = s.sb * s.sa;
    double cs = dot / w;
    if (clip) cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
    s.cs = cs;
    s.theta = acos(cs);
    return s;
}

struct FlowPlanes { const double *vxa, *vya, *spa, *vxb, *vyb, *spb; size_t fs; };   // [pair][fs] each

// The loads of FC_UNROLL samples of a lane are issued before the first of them is used (as in k_cp_joint); fn(sample) is then
// called for each in ascending order.  Block (x, pair) takes the samples x * FC_BLOCK + lane, + gridDim.x * FC_BLOCK, ... of its pair.
template <class F>
__device__ __forceinline__ void fc_for_each(const FlowPlanes& p, double speed_min, double angle_min, int clip, F&& fn) {
    const size_t base = (size_t)blockIdx.y * p.fs, stride = (size_t)gridDim.x * FC_BLOCK;
    for (size_t k0 = (size_t)blockIdx.x * FC_BLOCK + threadIdx.x; k0 < p.fs; k0 += FC_UNROLL * stride) {
        double xa[FC_UNROLL], ya[FC_UNROLL], pa[FC_UNROLL], xb[FC_UNROLL], yb[FC_UNROLL], pb[FC_UNROLL];
#pragma unroll
        for (int u = 0; u < FC_UNROLL; ++u) {
            const size_t k = k0 + u * stride, o = base + (k < p.fs ? k : k0);      // past the plane: the first sample again, unused
            xa[u] = p.vxa[o]; ya[u] = p.vya[o]; pa[u] = p.spa[o];
            xb[u] = p.vxb[o]; yb[u] = p.vyb[o]; pb[u] = p.spb[o];
        }
#pragma unroll
        for (int u = 0; u < FC_UNROLL; ++u) {
            if (k0 + u * stride >= p.fs) break;
            fn(fc_sample(xa[u], ya[u], pa[u], xb[u], yb[u], pb[u], speed_min, angle_min, clip));
        }
    }
}

// First pass.  One record per block: the exact extremes of sa and sb over the m1 samples and of cos over the m2 samples whose
// theta is not NaN; +inf / -inf where a block has none.  min and max do not depend on the order, so block partials and one
// final reduction give the same bits for every launch shape; no floating-point atomics.
struct FcExtremes { double sa_min, sa_max, sb_min, sb_max, cos_min, cos_max; };

__device__ __forceinline__ void fc_merge(FcExtremes& a, const FcExtremes& b) {
    a.sa_min = fmin(a.sa_min, b.sa_min); a.sa_max = fmax(a.sa_max, b.sa_max);
    a.sb_min = fmin(a.sb_min, b.sb_min); a.sb_max = fmax(a.sb_max, b.sb_max);
    a.cos_min = fmin(a.cos_min, b.cos_min); a.cos_max = fmax(a.cos_max, b.cos_max);
}
__device__ __forceinline__ FcExtremes fc_wave_extremes(FcExtremes e) {          // lane 0 holds the wave's
    for (int d = 32; d >= 1; d >>= 1) {
        FcExtremes o;
        o.sa_min = __shfl_down(e.sa_min, d); o.sa_max = __shfl_down(e.sa_max, d);
        o.sb_min = __shfl_down(e.sb_min, d); o.sb_max = __shfl_down(e.sb_max, d);
        o.cos_min = __shfl_down(e.cos_min, d); o.cos_max = __shfl_down(e.cos_max, d);
        fc_merge(e, o);
    }
    return e;
}
__device__ __forceinline__ FcExtremes fc_no_extremes() { return FcExtremes{INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY}; }

__global__ __launch_bounds__(FC_BLOCK) void k_fc_extremes(FlowPlanes p, double speed_min, double angle_min, int clip, FcExtremes* part) {
    __shared__ FcExtremes ws[FC_BLOCK / 64];
    FcExtremes e = fc_no_extremes();
    fc_for_each(p, speed_min, angle_min, clip, [&](const FcSample& s) {
        if (s.m1) {
            e.sa_min = fmin(e.sa_min, s.sa); e.sa_max = fmax(e.sa_max, s.sa);
            e.sb_min = fmin(e.sb_min, s.sb); e.sb_max = fmax(e.sb_max, s.sb);
        }
        if (s.m2 && s.theta == s.theta) { e.cos_min = fmin(e.cos_min, s.cs); e.cos_max = fmax(e.cos_max, s.cs); }
    });
    e = fc_wave_extremes(e);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FC_BLOCK / 64; ++w) fc_merge(e, ws[w]);
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = e;
    }
}

// *acc = the extremes of *acc and of the n records of part (one wave; the chunks of a call fold into one record in turn)
__global__ __launch_bounds__(64) void k_fc_extremes_fold(const FcExtremes* part, int n, FcExtremes* acc) {
    FcExtremes e = fc_no_extremes();
    for (int i = threadIdx.x; i < n; i += 64) fc_merge(e, part[i]);
    e = fc_wave_extremes(e);
    if (threadIdx.x == 0) { fc_merge(e, *acc); *acc = e; }
}

// Second pass.  jhist[ia][ib] += the m1 samples with sa in bin ia of ea and sb in bin ib of eb: bs_bin_of once per axis, as
// np.histogram2d bins every axis on its own - the last edge inclusive, a sample outside a range dropped.  thist[b] += the m2
// samples with theta in bin b of tedges; with clamp_theta - the range was chosen from the extremes of this very stack, so every
// kept sample lies inside it and only the last bits of acos could say otherwise - a theta below the first edge is in bin 0 and
// one above the last in bin tbins - 1; without it (an explicit range) a theta outside is dropped as numpy drops it.
// counters: 0, 1 NaN speeds of a and of b; 2 infinite; 3 m1 samples; 4 m2 samples whose theta is not NaN; 5 m2 samples whose
// theta is NaN.  The edges are staged in LDS (bs_bin_of reads two or three of them per sample and axis).  ba * bb <= CP_LDS_JOINT
// 2-D counters and the theta counters (one set per wave) live in LDS first; larger 2-D histograms go to global integer atomics
// (as k_cp_joint).  Static LDS: 16 KiB + 1 KiB + 16.5 KiB of edges.  Integer atomics only: nothing depends on the order of the blocks.
enum { FC_N_NAN_A = 0, FC_N_NAN_B, FC_N_INFINITE, FC_N_JOINT, FC_N_ANGLE, FC_N_DROPPED, FC_COUNTERS };

struct FcHistArgs {
    FlowPlanes p;
    double speed_min, angle_min; int clip, clamp_theta;
    const double *ea, *eb; int ba, bb;
    const double* tedges; int tbins;
    unsigned long long *jhist, *thist, *counters;
};

__global__ __launch_bounds__(FC_BLOCK) void k_fc_histograms(FcHistArgs a) {
    __shared__ unsigned int lj[CP_LDS_JOINT];
    __shared__ unsigned int lt[FC_BLOCK / 64][CP_MAX_THETA_BINS];
    __shared__ unsigned int lcount[FC_COUNTERS];
    __shared__ double le[2 * (CP_MAX_SPEED_BINS + 1) + CP_MAX_THETA_BINS + 1];      // the three edge vectors: bs_bin_of reads them per sample
    const int nj = a.ba * a.bb, wave = threadIdx.x >> 6;
    const bool jlds = nj <= CP_LDS_JOINT;
    double* const lea = le; double* const leb = lea + a.ba + 1; double* const let = leb + a.bb + 1;
    for (int b = threadIdx.x; b <= a.ba; b += FC_BLOCK) lea[b] = a.ea[b];
    for (int b = threadIdx.x; b <= a.bb; b += FC_BLOCK) leb[b] = a.eb[b];
    for (int b = threadIdx.x; b <= a.tbins; b += FC_BLOCK) let[b] = a.tedges[b];
    if (jlds) for (int b = threadIdx.x; b < nj; b += FC_BLOCK) lj[b] = 0u;
    for (int b = threadIdx.x; b < (FC_BLOCK / 64) * CP_MAX_THETA_BINS; b += FC_BLOCK) (&lt[0][0])[b] = 0u;
    if (threadIdx.x < FC_COUNTERS) lcount[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int n[FC_COUNTERS] = {};
    const double t_first = let[0], t_last = let[a.tbins];
    fc_for_each(a.p, a.speed_min, a.angle_min, a.clip, [&](const FcSample& s) {
        n[FC_N_NAN_A] += s.nan_a; n[FC_N_NAN_B] += s.nan_b; n[FC_N_INFINITE] += s.infinite;
        if (s.m1) {
            ++n[FC_N_JOINT];
            const int ia = bs_bin_of(s.sa, lea, a.ba);
            const int ib = ia >= 0 ? bs_bin_of(s.sb, leb, a.bb) : -1;
            if (ib >= 0) {
                if (jlds) atomicAdd(&lj[ia * a.bb + ib], 1u);
                else atomicAdd(&a.jhist[(size_t)ia * a.bb + ib], 1ull);
            }
        }
        if (s.m2) {
            if (s.theta == s.theta) {
                ++n[FC_N_ANGLE];
                int b;
                if (a.clamp_theta && s.theta < t_first) b = 0;
                else if (a.clamp_theta && s.theta > t_last) b = a.tbins - 1;
                else b = bs_bin_of(s.theta, let, a.tbins);
                if (b >= 0) atomicAdd(&lt[wave][b], 1u);
            } else {
                ++n[FC_N_DROPPED];
            }
        }
    });
#pragma unroll
    for (int i = 0; i < FC_COUNTERS; ++i)
        if (n[i]) atomicAdd(&lcount[i], n[i]);
    __syncthreads();
    if (jlds)
        for (int b = threadIdx.x; b < nj; b += FC_BLOCK)
            if (lj[b]) atomicAdd(&a.jhist[b], (unsigned long long)lj[b]);
    for (int b = threadIdx.x; b < a.tbins; b += FC_BLOCK) {
        unsigned int t = 0u;
        for (int w = 0; w < FC_BLOCK / 64; ++w) t += lt[w][b];
        if (t) atomicAdd(&a.thist[b], (unsigned long long)t);
    }
    if (threadIdx.x < FC_COUNTERS && lcount[threadIdx.x]) atomicAdd(&a.counters[threadIdx.x], (unsigned long long)lcount[threadIdx.x]);
}

}  // namespace vof
