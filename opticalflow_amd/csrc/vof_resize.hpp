// vof_resize.hpp - cv2.resize(frame, (n_j, n_i), interpolation=cv2.INTER_AREA) of every frame of a stack when neither axis is
// enlarged, on gfx950: the loop the reference's small-grid experiments run before the estimator (DESIGN.md section 15 has the
// specification).  OpenCV 4's arithmetic is restated operation by operation: resizeArea_ with the two axis tables of
// computeResizeAreaTab (built on the host, vof_frames.hip) where a scale is fractional, resizeAreaFast_ where both are integers.
//
// Both kernels share one skeleton.  A workgroup owns one output row and RS_BLOCK output columns, a lane one output pixel.  For
// every source row the output row reads, the workgroup stages the contiguous piece of that row its columns need in LDS (16-byte
// loads from the first 16-byte aligned element on, RS_SEG doubles at a time) and every lane consumes its own columns from there
// in table order; the sums over the rows stay in registers, in row order.  A source pixel is read once per output row that uses
// it: once, except for the one row two neighbouring output rows can share on a fractional scale.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "vof_preprocess.hpp"

namespace vof {

constexpr int RS_BLOCK = 256;                   // output columns (lanes) of a workgroup
constexpr int RS_SEG = 2048;                    // doubles of a source row staged at a time
constexpr int RS_LDS = RS_SEG + RS_SEG / 32;    // one pad per 32: lanes a whole number of columns apart spread over the banks

// One axis table: output index d reads the sources start[d] .. start[d] + count[d] - 1 with the weights w[d * kmax + k].
struct RsAxis {
    const int* start;
    const int* count;
    const float* w;
    int kmax;
};

__device__ inline int rs_pos(int i) { return i + (i >> 5); }

// row[c0 .. c0 + len) -> seg (len <= RS_SEG), by the whole workgroup
__device__ inline void rs_stage(const double* __restrict__ row, int c0, int len, double* seg) {
    const double* p = row + c0;
    const int head = min((int)(((uintptr_t)p >> 3) & 1), len);         // one element up to the 16-byte boundary
    if (threadIdx.x == 0 && head) seg[0] = p[0];
    const int pairs = (len - head) >> 1;
    const double2* p2 = (const double2*)(p + head);
    for (int q = threadIdx.x; q < pairs; q += RS_BLOCK) {
        const double2 v = p2[q];
        const int i = head + 2 * q;
        seg[rs_pos(i)] = v.x;
        seg[rs_pos(i + 1)] = v.y;
    }
    const int done = head + 2 * pairs;
    if (threadIdx.x == RS_BLOCK - 1 && done < len) seg[rs_pos(done)] = p[done];
}

// General path, resizeArea_<uchar, float> (U8) / <double, double>.  For the rows (r, beta) of ytab[dy] in order: buf = 0, then
// buf = buf + S[r][c] * alpha for the entries (c, alpha) of xtab[dx] in order; the first row sets sum = beta * buf, a later one
// sum = sum + beta * buf.  Every product and every sum is rounded on its own in WT (float32 for U8, float64 otherwise; a weight
// is a float32 promoted to WT): plain operators under fp contract(off), as in k_pp_blend.  U8: saturate_u8(rint(sum)), half to even.
// Grid (ceil(oj / RS_BLOCK), oi, frames).
template <bool U8>
__global__ __launch_bounds__(RS_BLOCK) void k_rs_area(const double* __restrict__ x, int ni, int nj, int oi, int oj, RsAxis yt, RsAxis xt,
                                                      double* __restrict__ out) {
#pragma clang fp contract(off)
    using WT = typename std::conditional<U8, float, double>::type;
    __shared__ double seg[RS_LDS];
    const int dy = blockIdx.y, dx0 = blockIdx.x * RS_BLOCK, dx = dx0 + threadIdx.x;
    const int dx1 = min(dx0 + RS_BLOCK, oj) - 1;
    const bool live = dx <= dx1;
    const int s0 = xt.start[dx0], s1 = xt.start[dx1] + xt.count[dx1];   // the columns this workgroup reads: [s0, s1)
    const int xs = live ? xt.start[dx] : 0, xc = live ? xt.count[dx] : 0;
    const float* xw = xt.w + (size_t)(live ? dx : dx0) * xt.kmax;
    const double* frame = x + (size_t)blockIdx.z * ni * nj;
    const int ys = yt.start[dy], yc = yt.count[dy];
    const float* yw = yt.w + (size_t)dy * yt.kmax;
    WT sum = 0;
    for (int e = 0; e < yc; ++e) {
        const double* row = frame + (size_t)(ys + e) * nj;
        WT buf = 0;
        int k = 0;
        for (int c0 = s0; c0 < s1; c0 += RS_SEG) {
            const int len = min(RS_SEG, s1 - c0);
            __syncthreads();                                            // the previous piece has been consumed
            rs_stage(row, c0, len, seg);
            __syncthreads();
            for (; k < xc && xs + k < c0 + len; ++k) {
                const WT p = (WT)seg[rs_pos(xs + k - c0)] * (WT)xw[k];
                buf = buf + p;
            }
        }
        const WT t = (WT)yw[e] * buf;
        sum = e == 0 ? t : sum + t;
    }
    if (!live) return;
    double r = (double)sum;
    if (U8) {
        const int v = __float2int_rn((float)sum);
        r = (double)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
    out[((size_t)blockIdx.z * oi + dy) * oj + dx] = r;
}

// Fast path, resizeAreaFast_: both scales are integers (isy x isx source pixels per output pixel, area = isx * isy) and
// scale_f = 1.0f / area is a float32 in both depths.
//   U8, half_up_2x2:  (S00 + S01 + S10 + S11 + 2) >> 2                                         (ResizeAreaFastVec)
//   U8 otherwise:     saturate_u8(rint(float32(integer sum) * scale_f))                        one float32 product, half to even
//   float64:          the samples in row-major order k = sy * isx + sx, summed as OpenCV's unrolled loop does: while k <= area - 4
//                     sum += ((S[k] + S[k+1]) + S[k+2]) + S[k+3], the rest one by one; result sum * (double) scale_f
// A group of four may run over the end of a block row, so the open group (g) travels with the lane from row to row.
// Grid (ceil(oj / RS_BLOCK), oi, frames).
template <bool U8>
__global__ __launch_bounds__(RS_BLOCK) void k_rs_fast(const double* __restrict__ x, int ni, int nj, int oi, int oj, int isy, int isx,
                                                      float scale_f, int half_up_2x2, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double seg[RS_LDS];
    const int dy = blockIdx.y, dx0 = blockIdx.x * RS_BLOCK, dx = dx0 + threadIdx.x;
    const int dx1 = min(dx0 + RS_BLOCK, oj) - 1;
    const bool live = dx <= dx1;
    const long long s0 = (long long)dx0 * isx, s1 = (long long)(dx1 + 1) * isx;   // <= nj
    const long long xs = live ? (long long)dx * isx : 0;
    const int xc = live ? isx : 0;
    const double* frame = x + (size_t)blockIdx.z * ni * nj;
    const int grouped = (isx * isy) & ~3;                               // samples that are summed in groups of four
    int isum = 0, n = 0;
    double sum = 0.0, g = 0.0;
    for (int sy = 0; sy < isy; ++sy) {
        const double* row = frame + ((size_t)dy * isy + sy) * nj;
        int k = 0;
        for (long long c0 = s0; c0 < s1; c0 += RS_SEG) {
            const int len = (int)min((long long)RS_SEG, s1 - c0);
            __syncthreads();
            rs_stage(row, (int)c0, len, seg);
            __syncthreads();
            for (; k < xc && xs + k < c0 + len; ++k, ++n) {
                const double v = seg[rs_pos((int)(xs + k - c0))];
                if (U8) {
                    isum += (int)v;
                } else if (n < grouped) {
                    g = (n & 3) ? g + v : v;
                    if ((n & 3) == 3) sum = sum + g;
                } else {
                    sum = sum + v;
                }
            }
        }
    }
    if (!live) return;
    double r;
    if (U8) {
        const int v = half_up_2x2 ? (isum + 2) >> 2 : __float2int_rn((float)isum * scale_f);
        r = (double)(v < 0 ? 0 : (v > 255 ? 255 : v));
    } else {
        r = sum * (double)scale_f;
    }
    out[((size_t)blockIdx.z * oi + dy) * oj + dx] = r;
}

}  // namespace vof
