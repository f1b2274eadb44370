// vof_compare.hpp - the joint statistics of the box least-squares flows of two channels of one movie (compare_channel_flows;
// the reference's compare_rho_and_actin.py:616-767 runs conduct_optical_flow on the Rho and the actin channel and compares the
// two velocity fields) on gfx950.  The flows themselves are those of vof_boxflow.hpp, the per-channel statistics those of
// vof_boxsweep.hpp and vof_blursweep.hpp; this header adds the one pass over the six planes of the pairs in flight.
#pragma once
#include <hip/hip_runtime.h>
#include "vof_blursweep.hpp"

namespace vof {

// Per sample, every operation explicit and uncontracted, in this order:
//   dot = v_x_a * v_x_b + v_y_a * v_y_b;  w = speed_a * speed_b;  cos = dot / w;  theta = acos(cos) / pi
// A sample whose speed is not finite in either channel takes no part (counters[0]).  cos is not clipped with the reference's
// quirks, so a rounding excess over 1 is a NaN theta; clipped to [-1, 1] without them (NaN stays NaN: a zero speed).  A NaN
// theta is in no bin (counters[1]).
//   thist[b]  += number of samples with theta in bin b (bs_bin_of against the np.linspace(0, 1, bins + 1) edges), counted in
//               LDS first, then integer atomics.
//   partials[pair][block][b] = sum of w over the block's samples in bin b, in the fixed shape of k_bz_angles: a workgroup is
//     one wave, lane l of block q adds the samples q * 64 + l, + gridDim.x * 64, ... of its pair in that order into a column
//     of its own, lw[b][l] (a lane's column is one LDS bank pair: conflict-free); wave_sum's fixed tree adds the 64 columns and
//     k_bz_angle_sum the blocks of a pair in block order.  gridDim.x depends on the plane size only (cp_blocks), so a pair's
//     sums do not depend on the launch that held it.  No floating-point atomics.
//   jhist[ia][ib] += samples with speed_a in bin ia of ea and speed_b in bin ib of eb (bs_bin_of once per axis, as
//     np.histogram2d bins every axis on its own: NaN and values outside a range are dropped) and, with has_min,
//     speed_b > min_b; ba * bb <= CP_LDS_JOINT counters live in LDS first, more go to global integer atomics (k_bs_counts).
// The loads of CP_UNROLL samples of a lane are issued before the first of them is used; a lane still adds its samples in
// ascending order.  48 bytes are read per sample, nothing of field size is written.
// Dynamic LDS: cp_lds(), (tbins * 64) doubles + (tbins + ba * bb) counters: 49408 B at the limits, 35800 B for the reference's
// 50 and 50 x 50 bins - inside the default 64 KiB, no limit to raise.
constexpr int CP_PER_LANE = 16;           // samples a lane adds at least before a plane gets another block ...
constexpr int CP_MAX_BLOCKS = 256;        // ... up to this many blocks per pair
constexpr int CP_UNROLL = 4;

struct CompareArgs {
    const double *vxa, *vya, *spa, *vxb, *vyb, *spb;   // [pair][fs] each
    size_t fs;
    const double* tedges; int tbins;
    const double *ea, *eb; int ba, bb;                 // ba == 0: no 2-D histogram
    int has_min; double min_b;
    int clip;                                          // reference_quirks == 0
    unsigned long long *thist, *jhist, *counters;      // counters: joint non-finite, theta dropped
    double* partials;                                  // [pair][gridDim.x][tbins]
};

inline int cp_blocks(size_t fs) {          // by the plane size only
    const size_t n = fs / (64 * CP_PER_LANE);
    return n < 1 ? 1 : (n > (size_t)CP_MAX_BLOCKS ? CP_MAX_BLOCKS : (int)n);
}
inline int cp_lds_joint(int ba, int bb) { return (size_t)ba * bb <= (size_t)CP_LDS_JOINT ? ba * bb : 0; }
inline size_t cp_lds(int tbins, int ba, int bb) {
    return (size_t)tbins * 64 * sizeof(double) + ((size_t)tbins + cp_lds_joint(ba, bb)) * sizeof(unsigned int);
}

__global__ __launch_bounds__(64) void k_cp_joint(CompareArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double lw[];                                  // [tbins][64]
    unsigned int* const lc = (unsigned int*)(lw + a.tbins * 64);    // [tbins]
    unsigned int* const lj = lc + a.tbins;                          // [ba * bb] if that fits
    __shared__ unsigned int lbad, ldrop;
    const int lane = threadIdx.x;
    const int nj = a.ba * a.bb;
    const bool jlds = nj > 0 && nj <= CP_LDS_JOINT;
    for (int b = 0; b < a.tbins; ++b) lw[b * 64 + lane] = 0.0;
    for (int b = lane; b < a.tbins; b += 64) lc[b] = 0u;
    if (jlds) for (int b = lane; b < nj; b += 64) lj[b] = 0u;
    if (lane == 0) { lbad = 0u; ldrop = 0u; }
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * a.fs, stride = (size_t)gridDim.x * 64;
    unsigned int bad = 0u, drop = 0u;
    for (size_t k0 = (size_t)blockIdx.x * 64 + lane; k0 < a.fs; k0 += CP_UNROLL * stride) {
        double xa[CP_UNROLL], ya[CP_UNROLL], sa[CP_UNROLL], xb[CP_UNROLL], yb[CP_UNROLL], sb[CP_UNROLL];
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u) {
            const size_t k = k0 + u * stride, o = base + (k < a.fs ? k : k0);      // past the plane: the first sample again, unused
            xa[u] = a.vxa[o]; ya[u] = a.vya[o]; sa[u] = a.spa[o];
            xb[u] = a.vxb[o]; yb[u] = a.vyb[o]; sb[u] = a.spb[o];
        }
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u) {
            if (k0 + u * stride >= a.fs) break;
            if (nj) {
                const int ia = bs_bin_of(sa[u], a.ea, a.ba);
                const int ib = ia >= 0 ? bs_bin_of(sb[u], a.eb, a.bb) : -1;
                if (ib >= 0 && (!a.has_min || sb[u] > a.min_b)) {
                    if (jlds) atomicAdd(&lj[ia * a.bb + ib], 1u);
                    else atomicAdd(&a.jhist[(size_t)ia * a.bb + ib], 1ull);
                }
            }
            if (!(fabs(sa[u]) <= 1.7976931348623157e308) || !(fabs(sb[u]) <= 1.7976931348623157e308)) { ++bad; continue; }
            const double dot = xa[u] * xb[u] + ya[u] * yb[u];
            const double w = sa[u] * sb[u];
            double cs = dot / w;
            if (a.clip) cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
            const double theta = acos(cs) / 3.141592653589793;
            const int b = bs_bin_of(theta, a.tedges, a.tbins);
            if (b >= 0) {
                atomicAdd(&lc[b], 1u);
                lw[b * 64 + lane] += w;
            } else {
                ++drop;
            }
        }
    }
    if (bad) atomicAdd(&lbad, bad);
    if (drop) atomicAdd(&ldrop, drop);
    __syncthreads();
    double* pp = a.partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.tbins;
    for (int b = 0; b < a.tbins; ++b) {
        const double s = wave_sum(lw[b * 64 + lane]);
        if (lane == 0) pp[b] = s;
    }
    for (int b = lane; b < a.tbins; b += 64)
        if (lc[b]) atomicAdd(&a.thist[b], (unsigned long long)lc[b]);
    if (jlds)
        for (int b = lane; b < nj; b += 64)
            if (lj[b]) atomicAdd(&a.jhist[b], (unsigned long long)lj[b]);
    if (lane == 0) {
        if (lbad) atomicAdd(&a.counters[0], (unsigned long long)lbad);
        if (ldrop) atomicAdd(&a.counters[1], (unsigned long long)ldrop);
    }
}

}  // namespace vof
