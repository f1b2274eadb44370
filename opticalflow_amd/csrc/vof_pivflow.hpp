// vof_pivflow.hpp - conduct_piv on gfx950: direct (spatial-domain) zero-normalised cross-correlation PIV of every frame pair of a
// stack, multi-pass with integer window offsets from the pass before.  DESIGN.md section 20; the arithmetic is that of
// tests/piv_flow_restatement.py - float64, every operation single and uncontracted, every window sum two-level (a window row left
// to right from 0.0, the row sums top to bottom from 0.0, products rounded before they are added) - and the kernels are held to it
// bit for bit.  Integer atomics only (the counts): results are the same from call to call and for every frames_in_flight.
// Two options (DESIGN.md sections 20.7 to 20.9, tests/piv_deform_restatement.py): the normalised median test on the vectors of a pass
// before the next one uses them (k_pivflow_validate), and window deformation, where the search region of a later pass is frame k + 1
// resampled by the interpolated vectors of the pass before (the DEFORM staging of k_pivflow_correlate).
#pragma once
#include <hip/hip_runtime.h>
#include "vof_piv.hpp"

namespace vof {

constexpr int PF_BLOCK = 256;             // threads of k_pivflow_correlate: 4 waves, one per SIMD
constexpr int PF_WAVE = 64;
constexpr int PF_MIN_W = 4, PF_MAX_W = 64, PF_MAX_R = 16, PF_MAX_PASSES = 8;
constexpr int PF_LONG_RUN = 5, PF_SHORT_RUN = 3;   // displacements d_j a lane owns: PF_LONG_RUN from radius PF_LONG_FROM_R on
constexpr int PF_LONG_FROM_R = 10;
constexpr size_t PF_LDS_LIMIT = 160 * 1024 - 2048;  // dynamic LDS of a workgroup: the CU's 160 KiB less the kernel's static arrays

// profiler stages of VOF_K_REDUCE, after those of vof_piv.hpp: the offsets, then the correlation of pass p at PF_ST_PASS0 + p
enum { PF_ST_OFFSETS = PIV_ST_EVAL + 1, PF_ST_PASS0 };
static_assert(PF_ST_PASS0 + PF_MAX_PASSES - 1 <= 15, "the profiler keeps 16 stages per class");

// One pass as the kernels see it.  m: the margin r_0 + ... + r_p; (R, C): the grid of windows, window (a, b) at (m + a s, m + b s).
struct PfPass { int w, r, s, m, R, C; };

__host__ __device__ inline int pf_run(int r) { return r >= PF_LONG_FROM_R ? PF_LONG_RUN : PF_SHORT_RUN; }
// Row strides in LDS are odd: lanes that differ in their row then read different banks.
__host__ __device__ inline int pf_odd(int n) { return n | 1; }
// Dynamic LDS of the correlation kernel, doubles: the window of frame k, the search region of frame k + 1, and the row sums of the
// region and of its squares per (d_j, row) - where the correlation values lie once the sums are used up (D * D <= 2 * S * D).
__host__ __device__ inline size_t pf_lds_doubles(int w, int r) {
    const size_t S = (size_t)w + 2 * r, D = 2 * (size_t)r + 1;
    return (size_t)w * pf_odd(w) + S * pf_odd((int)S) + 2 * S * D;
}
// The work items of a window: (run of d_j, d_i).  At most PF_BLOCK for every accepted radius (231 at r = 16, 133 at r = 9).
__host__ __device__ inline int pf_items(int r) { const int D = 2 * r + 1, K = pf_run(r); return D * ((D + K - 1) / K); }

__device__ __forceinline__ double pf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool pf_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }

// floor((2 (i0 - m') + w - w' + s') / (2 s')) clamped to [0, n' - 1]: the window of the pass before whose centre is nearest
__device__ __forceinline__ int pf_previous(int at, int w, const PfPass& q, int n) {
    const int num = 2 * (at - q.m) + w - q.w + q.s, den = 2 * q.s;
    int a = num >= 0 ? num / den : -((-num + den - 1) / den);     // floor division
    return a < 0 ? 0 : (a > n - 1 ? n - 1 : a);
}

// ---- the predictor of a deformed pass ------------------------------------------------------------------------------------------------
// A real position on an axis of n nodes at c + s * index: g = clamp((pos - c) / s, 0, n - 1), lo = floor(g) but n - 2 at the last node
// (0 where there is one node), t = g - lo, hi = min(lo + 1, n - 1).  Whatever comes in, NaN included, lo and hi lie in [0, n - 1].
struct PfSplit { int lo, hi; double t; };
__device__ __forceinline__ PfSplit pf_split(double pos, double c, double s, int n) {
#pragma clang fp contract(off)
    double g = (pos - c) / s;
    g = fmin(fmax(g, 0.0), (double)(n - 1));
    int lo = (int)floor(g);
    if (lo > n - 2) lo = max(n - 2, 0);
    return PfSplit{lo, min(lo + 1, n - 1), g - (double)lo};
}
__device__ __forceinline__ double pf_lerp2(double f00, double f01, double f10, double f11, double ta, double tb) {
#pragma clang fp contract(off)
    const double top = f00 + tb * (f01 - f00), bot = f10 + tb * (f11 - f10);
    return top + ta * (bot - top);
}
// What a deformed pass reads of the pass before: its geometry and its vectors [pair][R][C], validated where validation is on.
struct PfDeform { PfPass q; const double* u; const double* v; int Ni; };
// (U, V) of pass q's vectors of one pair between the rows a.lo, a.hi and the columns b.lo, b.hi; a vector with a NaN reads as (0, 0).
__device__ __forceinline__ void pf_predict(const double* __restrict__ u, const double* __restrict__ v, int C, const PfSplit& a, const PfSplit& b,
                                           double& U, double& V) {
    const int at[4] = {a.lo * C + b.lo, a.lo * C + b.hi, a.hi * C + b.lo, a.hi * C + b.hi};
    double fu[4], fv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        fu[k] = u[at[k]]; fv[k] = v[at[k]];
        if (fu[k] != fu[k] || fv[k] != fv[k]) { fu[k] = 0.0; fv[k] = 0.0; }
    }
    U = pf_lerp2(fu[0], fu[1], fu[2], fu[3], a.t, b.t);
    V = pf_lerp2(fv[0], fv[1], fv[2], fv[3], a.t, b.t);
}
__device__ __forceinline__ double pf_centre(const PfPass& q) {
#pragma clang fp contract(off)
    return (double)q.m + (double)(q.w - 1) / 2.0;
}

// ---- the normalised median test (Westerweel & Scarano 2005) on the vectors of a pass: one thread per window, the pair is blockIdx.y ----
// Compare and exchange where y < x: the 19 comparators of the 8-input network, absent neighbours +inf, so k values sort to s[0 .. k).
__device__ __forceinline__ void pf_sort8(double (&s)[8]) {
#define PF_CX(x, y) { const double lo_ = s[y] < s[x] ? s[y] : s[x], hi_ = s[y] < s[x] ? s[x] : s[y]; s[x] = lo_; s[y] = hi_; }
    PF_CX(0, 1) PF_CX(2, 3) PF_CX(4, 5) PF_CX(6, 7) PF_CX(0, 2) PF_CX(1, 3) PF_CX(4, 6) PF_CX(5, 7) PF_CX(1, 2) PF_CX(5, 6) PF_CX(0, 4) PF_CX(3, 7)
    PF_CX(1, 5) PF_CX(2, 6) PF_CX(1, 4) PF_CX(3, 6) PF_CX(2, 4) PF_CX(3, 5) PF_CX(3, 4)
#undef PF_CX
}
// the median of the k finite values among the eight: the middle one, or (lo + hi) * 0.5
__device__ __forceinline__ double pf_median8(double (&s)[8], int k) {
#pragma clang fp contract(off)
    pf_sort8(s);
    const int i_lo = (k - 1) / 2, i_hi = k / 2;
    double lo = s[0], hi = s[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) { if (i == i_lo) lo = s[i]; if (i == i_hi) hi = s[i]; }
    return (k & 1) ? lo : (lo + hi) * 0.5;
}
// r = |x - med| / (med |x_n - med| + eps) of a centre x among its neighbours xn (absent: +inf)
__device__ __forceinline__ double pf_residual(double x, double med, const double (&xn)[8], int k, double eps) {
#pragma clang fp contract(off)
    double dev[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dev[i] = xn[i] < INFINITY ? fabs(xn[i] - med) : INFINITY;
    return fabs(x - med) / (pf_median8(dev, k) + eps);
}
// Jacobi style: reads (u, v), writes (u_out, v_out), [pair][R][C] each.  A window with fewer than three valid neighbours is copied; an
// invalid centre becomes the medians (counts[1], filled); a valid one whose r_u or r_v exceeds the threshold too (counts[0], outliers).
__global__ __launch_bounds__(PF_BLOCK) void k_pivflow_validate(int R, int C, const double* __restrict__ u, const double* __restrict__ v,
                                                              double threshold, double eps, double* __restrict__ u_out,
                                                              double* __restrict__ v_out, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PF_BLOCK + threadIdx.x, pair = blockIdx.y;
    if (t >= R * C) return;
    const int a = t / C, b = t % C;
    const double* pu = u + (size_t)pair * R * C;
    const double* pv = v + (size_t)pair * R * C;
    double un[8], vn[8];
    int k = 0, slot = 0;
#pragma unroll
    for (int da = -1; da <= 1; ++da) {
#pragma unroll
        for (int db = -1; db <= 1; ++db) {
            if (da == 0 && db == 0) continue;
            const int aa = a + da, bb = b + db;
            double x = INFINITY, y = INFINITY;
            if (aa >= 0 && aa < R && bb >= 0 && bb < C) {
                const double nu = pu[aa * C + bb], nv = pv[aa * C + bb];
                if (!(nu != nu) && !(nv != nv)) { x = nu; y = nv; ++k; }
            }
            un[slot] = x; vn[slot] = y; ++slot;
        }
    }
    double cu = pu[t], cv = pv[t];
    if (k >= 3) {
        double su[8], sv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { su[i] = un[i]; sv[i] = vn[i]; }
        const double um = pf_median8(su, k), vm = pf_median8(sv, k);
        if (cu != cu || cv != cv) {
            cu = um; cv = vm;
            atomicAdd(&counts[1], 1ULL);
        } else {
            const double ru = pf_residual(cu, um, un, k, eps), rv = pf_residual(cv, vm, vn, k, eps);
            if (ru > threshold || rv > threshold) { cu = um; cv = vm; atomicAdd(&counts[0], 1ULL); }
        }
    }
    u_out[(size_t)pair * R * C + t] = cu; v_out[(size_t)pair * R * C + t] = cv;
}

// ---- the offsets of a pass from the vectors of the pass before: one thread per window, the pair is blockIdx.y ----------------------
// off[pair][R][C][2] = (o_i, o_j) = floor(v' + 0.5), floor(u' + 0.5), or (0, 0) where the vector is NaN.  |o| <= m' by the
// arithmetic; the clamp never acts and only keeps a search region inside the frame whatever comes in.
__global__ __launch_bounds__(PF_BLOCK) void k_pivflow_offsets(PfPass p, PfPass q, const double* __restrict__ u_prev,
                                                             const double* __restrict__ v_prev, int* __restrict__ off) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PF_BLOCK + threadIdx.x, pair = blockIdx.y;
    if (t >= p.R * p.C) return;
    const int a = t / p.C, b = t % p.C;
    const int ap = pf_previous(p.m + a * p.s, p.w, q, q.R), bp = pf_previous(p.m + b * p.s, p.w, q, q.C);
    const size_t at = ((size_t)pair * q.R + ap) * q.C + bp;
    const double u = u_prev[at], v = v_prev[at];
    int oi = 0, oj = 0;
    if (!(u != u) && !(v != v)) {
        const double fi = fmin(fmax(floor(v + 0.5), (double)-q.m), (double)q.m), fj = fmin(fmax(floor(u + 0.5), (double)-q.m), (double)q.m);
        oi = (int)fi; oj = (int)fj;
    }
    int* o = off + 2 * ((size_t)pair * p.R * p.C + t);
    o[0] = oi; o[1] = oj;
}

// The window values and the new values of B of the K steps from column j of a window row: arow[j + s] and brow[j + s + K - 1]
// (brow starts at the lane's first d_j).  CLAMP: a column past the window is not used, and one past the region (`last`, from brow)
// belongs to a d_j past D, whose result is dropped: the last column is read instead.  Without CLAMP the caller knows that every
// column lies inside, and the 2 K reads are one address each plus constant offsets.
template <int K, bool CLAMP>
__device__ __forceinline__ void pf_read(const double* arow, const double* brow, int j, int w, int last, double (&xa)[K], double (&nb)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        xa[s] = arow[CLAMP ? min(j + s, w - 1) : j + s];
        nb[s] = brow[CLAMP ? min(j + s + K - 1, last) : j + s + K - 1];
    }
}

// K steps from column jb, a multiple of K (TAIL: those of them inside the row): ring[(s + k) % K] holds B[.][d_j0 + jb + s + k],
// the newest value replacing the one that step jb + s - 1 used first.  acc[k] = acc[k] + x * b: the product is rounded, then added.
template <int K, bool TAIL>
__device__ __forceinline__ void pf_steps(int jb, int w, const double (&xa)[K], const double (&nb)[K], double (&ring)[K], double (&acc)[K]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (!TAIL || jb + s < w) {
            ring[(s + K - 1) % K] = nb[s];
            const double x = xa[s];
            double prod[K];                                         // the K products, then the K additions: no instruction waits for the one before it
#pragma unroll
            for (int k = 0; k < K; ++k) prod[k] = x * ring[(s + k) % K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = acc[k] + prod[k];
        }
    }
}

// ---- the correlation: one window per workgroup, grid (C, R, pairs) -------------------------------------------------------------
// frames: the chunk's frames, pair k reads frames k and k + 1.  off: the offsets of this pass (NULL: none, pass 0).  u, v, corr:
// [pair][R][C] (corr may be NULL: an intermediate pass).  counts[3]: flat, border, below the threshold.
//
// LDS, doubles: A[w][w|1], B[S][S|1] (S = w + 2 r), then rb[D][S] and rbb[D][S] (D = 2 r + 1): the sums of B[y][d_j .. d_j + w)
// and of their squares, formed once per (row, d_j) and shared by the D displacements d_i that read row y.
// The hot loop: a lane owns (d_i, K consecutive d_j) and walks the window row by row; B[i + d_i][j + d_j .. + K) lives in a ring
// of K registers, so a step of j costs one read of B and one (broadcast) read of A for K multiplications and K additions.
// K = 5 from r = 10 on, 3 below (pf_run); runs of 3 in six waves for every radius were measured and are slower
// (profiles/piv_flow_summary.md).
//
// DEFORM (a pass after the first, off NULL): the region is rows [i0 - r, ... + S) of frame k + 1 resampled.  Pixel (i, j) holds the frame
// at (i + V(i, j), j + U(i, j)), bilinear and clamped to the frame, (U, V) the bilinear predictor from the vectors of pass df.q.  The
// splits of the S rows and S columns between the nodes of that pass are formed once, in the LDS of the row sums, which are not yet
// in use; a pixel then costs four gathers of each vector grid, four of the frame and the two interpolations.  At the end thread 0
// adds the predictor at the window's centre instead of the offset.  Everything between - sums, hot loop, peak - is the same code.
template <int K, bool DEFORM>
__global__ __launch_bounds__(PF_BLOCK) void k_pivflow_correlate(PfPass p, const double* __restrict__ frames, size_t fs, int Nj,
                                                               const int* __restrict__ off, double min_correlation,
                                                               double* __restrict__ u, double* __restrict__ v, double* __restrict__ corr,
                                                               unsigned long long* __restrict__ counts, PfDeform df) {
#pragma clang fp contract(off)
    extern __shared__ double pf_lds[];
    __shared__ double rows_a[2 * PF_MAX_W];
    __shared__ double sums_a[2];
    __shared__ double best_v[PF_WAVE];
    __shared__ int best_at[PF_WAVE];
    const int w = p.w, r = p.r, S = w + 2 * r, D = 2 * r + 1, wP = pf_odd(w), SP = pf_odd(S);
    double* const A = pf_lds;
    double* const B = A + (size_t)w * wP;
    double* const rb = B + (size_t)S * SP;
    double* const rbb = rb + (size_t)D * S;
    double* const Cv = rb;                                          // the correlation values, after the row sums
    const int b = blockIdx.x, a = blockIdx.y, pair = blockIdx.z, tid = threadIdx.x;
    const size_t win = ((size_t)pair * p.R + a) * p.C + b;
    const int i0 = p.m + a * p.s, j0 = p.m + b * p.s;
    const int oi = off ? off[2 * win] : 0, oj = off ? off[2 * win + 1] : 0;

    // the two windows: rows [i0, i0 + w) of frame k, rows [i0 + oi - r, ... + S) of frame k + 1 (inside the frame: |o| <= m - r)
    const double* fa = frames + (size_t)pair * fs + (size_t)i0 * Nj + j0;
    const double* fb = frames + (size_t)(pair + 1) * fs + (size_t)(i0 + oi - r) * Nj + (j0 + oj - r);
#pragma unroll 4
    for (int k = tid; k < w * w; k += PF_BLOCK) A[(k / w) * wP + k % w] = fa[(size_t)(k / w) * Nj + k % w];
    if (!DEFORM) {
#pragma unroll 4
        for (int k = tid; k < S * S; k += PF_BLOCK) B[(k / S) * SP + k % S] = fb[(size_t)(k / S) * Nj + k % S];
    } else {
        double* const split_t = rb;                                 // [2 S]: rows, then columns
        int* const split_lo = (int*)(rb + 2 * S);
        const double cq = pf_centre(df.q), sq = (double)df.q.s;
        for (int k = tid; k < 2 * S; k += PF_BLOCK) {
            const PfSplit sp = k < S ? pf_split((double)(i0 - r + k), cq, sq, df.q.R) : pf_split((double)(j0 - r + k - S), cq, sq, df.q.C);
            split_t[k] = sp.t; split_lo[k] = sp.lo;
        }
        __syncthreads();
        const double* pu = df.u + (size_t)pair * df.q.R * df.q.C;
        const double* pv = df.v + (size_t)pair * df.q.R * df.q.C;
        const double* second = frames + (size_t)(pair + 1) * fs;
        for (int k = tid; k < S * S; k += PF_BLOCK) {
            const int y = k / S, x = k % S;
            const PfSplit ga{split_lo[y], min(split_lo[y] + 1, df.q.R - 1), split_t[y]};
            const PfSplit gb{split_lo[S + x], min(split_lo[S + x] + 1, df.q.C - 1), split_t[S + x]};
            double U, V;
            pf_predict(pu, pv, df.q.C, ga, gb, U, V);
            const PfSplit fa2 = pf_split((double)(i0 - r + y) + V, 0.0, 1.0, df.Ni), fb2 = pf_split((double)(j0 - r + x) + U, 0.0, 1.0, Nj);
            const double* r0 = second + (size_t)fa2.lo * Nj;
            const double* r1 = second + (size_t)fa2.hi * Nj;
            B[y * SP + x] = pf_lerp2(r0[fb2.lo], r0[fb2.hi], r1[fb2.lo], r1[fb2.hi], fa2.t, fb2.t);
        }
    }
    __syncthreads();

    // S_a and S_aa: a thread per row, then thread 0 adds the rows top to bottom
    if (tid < w) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
        for (int j = 0; j < w; ++j) { const double x = A[tid * wP + j]; s1 = s1 + x; s2 = s2 + x * x; }
        rows_a[tid] = s1; rows_a[PF_MAX_W + tid] = s2;
    }
    // the row sums of B: item (d_j, y), lanes along y
    for (int k = tid; k < D * S; k += PF_BLOCK) {
        const int dj = k / S, y = k % S;
        const double* row = B + (size_t)y * SP + dj;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
        for (int j = 0; j < w; ++j) { const double x = row[j]; s1 = s1 + x; s2 = s2 + x * x; }
        rb[k] = s1; rbb[k] = s2;
    }
    __syncthreads();
    if (tid == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < w; ++i) { s1 = s1 + rows_a[i]; s2 = s2 + rows_a[PF_MAX_W + i]; }
        sums_a[0] = s1; sums_a[1] = s2;
    }
    __syncthreads();
    const double n = (double)(w * w);
    const double Sa = sums_a[0], Saa = sums_a[1];
    const double Da = n * Saa - Sa * Sa;
    if (!(Da > 0.0)) {                                              // a flat window (the whole workgroup takes this branch)
        if (tid == 0) {
            u[win] = pf_nan(); v[win] = pf_nan();
            if (corr) corr[win] = pf_nan();
            atomicAdd(&counts[0], 1ULL);
        }
        return;
    }

    // S_ab, S_b, S_bb and C(d) of the lane's K displacements
    const int runs = (D + K - 1) / K;
    const int run = tid / D, di = tid % D, dj0 = run * K;           // lanes along d_i: rows of B one odd stride apart
    const bool active = tid < D * runs;
    const int last = S - 1 - dj0;                                   // the last column of the region, from the lane's first
    double cval[K];
    if (active) {
        double tot[K];
#pragma unroll
        for (int k = 0; k < K; ++k) tot[k] = 0.0;
        for (int i = 0; i < w; ++i) {
            const double* arow = A + (size_t)i * wP;
            const double* brow = B + (size_t)(i + di) * SP + dj0;
            double acc[K], ring[K], xa[K], nb[K], xa2[K], nb2[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll
            for (int k = 0; k < K - 1; ++k) ring[k] = brow[min(k, last)];
            ring[K - 1] = 0.0;
            // K steps at a time, and the reads of the next K steps are issued before the arithmetic of these: a workgroup has one
            // wave per SIMD, so nothing else hides the latency of LDS.  The loop over whole double blocks has no branch in it (a
            // read past the row is clamped and unused); the last steps of the row, fewer than 2 K, are guarded and read nothing.
            const int whole = w - w % (2 * K);
            pf_read<K, true>(arow, brow, 0, w, last, xa, nb);
            int jb = 0;
            for (; jb + 4 * K - 2 < w; jb += 2 * K) {               // the last column read, jb + 4 K - 2 of brow, is inside the window
                pf_read<K, false>(arow, brow, jb + K, w, last, xa2, nb2);
                pf_steps<K, false>(jb, w, xa, nb, ring, acc);
                pf_read<K, false>(arow, brow, jb + 2 * K, w, last, xa, nb);
                pf_steps<K, false>(jb + K, w, xa2, nb2, ring, acc);
            }
            for (; jb < whole; jb += 2 * K) {
                pf_read<K, true>(arow, brow, jb + K, w, last, xa2, nb2);
                pf_steps<K, false>(jb, w, xa, nb, ring, acc);
                pf_read<K, true>(arow, brow, jb + 2 * K, w, last, xa, nb);
                pf_steps<K, false>(jb + K, w, xa2, nb2, ring, acc);
            }
            pf_read<K, true>(arow, brow, whole + K, w, last, xa2, nb2);
            pf_steps<K, true>(whole, w, xa, nb, ring, acc);
            pf_steps<K, true>(whole + K, w, xa2, nb2, ring, acc);
#pragma unroll
            for (int k = 0; k < K; ++k) tot[k] = tot[k] + acc[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int dj = dj0 + k;
            cval[k] = 0.0;
            if (dj < D) {
                const double* c1 = rb + (size_t)dj * S + di;
                const double* c2 = rbb + (size_t)dj * S + di;
                double Sb = 0.0, Sbb = 0.0;
#pragma unroll 8
                for (int i = 0; i < w; ++i) { Sb = Sb + c1[i]; Sbb = Sbb + c2[i]; }
                const double Db = n * Sbb - Sb * Sb;
                cval[k] = Db > 0.0 ? (n * tot[k] - Sa * Sb) / sqrt(Da * Db) : -INFINITY;
            }
        }
    }
    __syncthreads();                                                // every row sum is read: the values take their place
    if (active) {
#pragma unroll
        for (int k = 0; k < K; ++k) if (dj0 + k < D) Cv[di * D + dj0 + k] = cval[k];
    }
    __syncthreads();

    // the first maximum in raster order: wave 0, a lane per contiguous stretch, then thread 0 over the lanes in order
    const int DD = D * D;
    if (tid < PF_WAVE) {
        const int per = (DD + PF_WAVE - 1) / PF_WAVE, lo = tid * per, hi = min(lo + per, DD);
        double bv = -INFINITY; int at = lo < DD ? lo : 0;
        for (int k = lo; k < hi; ++k) if (Cv[k] > bv) { bv = Cv[k]; at = k; }
        best_v[tid] = bv; best_at[tid] = at;
    }
    __syncthreads();
    if (tid != 0) return;
    double c0 = best_v[0]; int at = best_at[0];
    for (int l = 1; l < PF_WAVE; ++l) if (best_v[l] > c0) { c0 = best_v[l]; at = best_at[l]; }
    if (!(c0 > -INFINITY)) {                                        // no displacement with a texture under it: counted with the flat windows
        u[win] = pf_nan(); v[win] = pf_nan();
        if (corr) corr[win] = c0;
        atomicAdd(&counts[0], 1ULL);
        return;
    }
    const int pi = at / D, pj = at % D;                             // d = (pi - r, pj - r)
    double delta_i = 0.0, delta_j = 0.0;
    if (pi > 0 && pi < D - 1) {
        const double cm = Cv[at - D], cp = Cv[at + D];
        if (pf_finite(cm) && pf_finite(cp)) {
            const double den = 2.0 * ((cm - 2.0 * c0) + cp);
            if (den < 0.0) delta_i = (cm - cp) / den;
        }
    }
    if (pj > 0 && pj < D - 1) {
        const double cm = Cv[at - 1], cp = Cv[at + 1];
        if (pf_finite(cm) && pf_finite(cp)) {
            const double den = 2.0 * ((cm - 2.0 * c0) + cp);
            if (den < 0.0) delta_j = (cm - cp) / den;
        }
    }
    if (pi == 0 || pi == D - 1 || pj == 0 || pj == D - 1) atomicAdd(&counts[1], 1ULL);
    double vv, uu;
    if (!DEFORM) {
        vv = (double)(oi + pi - r) + delta_i; uu = (double)(oj + pj - r) + delta_j;
    } else {                                                        // the predictor at the window's centre, then d + delta
        const double half = (double)(w - 1) / 2.0, cq = pf_centre(df.q), sq = (double)df.q.s;
        double Uc, Vc;
        pf_predict(df.u + (size_t)pair * df.q.R * df.q.C, df.v + (size_t)pair * df.q.R * df.q.C, df.q.C,
                   pf_split((double)i0 + half, cq, sq, df.q.R), pf_split((double)j0 + half, cq, sq, df.q.C), Uc, Vc);
        vv = Vc + ((double)(pi - r) + delta_i); uu = Uc + ((double)(pj - r) + delta_j);
    }
    if (c0 < min_correlation) { uu = pf_nan(); vv = pf_nan(); atomicAdd(&counts[2], 1ULL); }
    u[win] = uu; v[win] = vv;
    if (corr) corr[win] = c0;
}

}  // namespace vof
