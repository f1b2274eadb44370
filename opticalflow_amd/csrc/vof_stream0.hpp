// vof_stream0.hpp - the two row-streaming kernels of the matrix-free level 0 and the LDS ring they share.
//
//   k_stream_apply0<MODE>   y = A x (0), y = b - A x (1), the batch prologue (2) and the batch epilogue (3)
//   k_stream_resrestrict0   b_c = R (b - A x), the stand-alone coarse right-hand side
//
// Both march down a band of rows with a six-row ring of x (three fields) and of the image in LDS.  What one thread loads
// for a ring row (ApRow, ap_load_x, ap_load_im), how the row is put into the ring (ap_store_row) and how (A x)(p, q) is
// formed from the ring (ap_point) exist once, below; the kernels hold only what is their own.
#pragma once
#include "vof_device.hpp"

namespace vof {

// A block owns a 128-column strip (+1 halo column each side) and a band of TI rows; per step the two wave pairs compute two
// rows.
constexpr int AP_OUT = 128, AP_W = 132, AP_THREADS = 256;
// Ring depth: a step loads rows r + 3, r + 4 while rows r - 1 .. r + 2 are read, i.e. six live rows (the fused
// residual + restriction kernel likewise keeps residual rows 2s - 4 .. 2s + 1).  Six slots instead of the next power of
// two keep that kernel at 43.8 KB of LDS = 3 workgroups per CU (8 slots: 58 KB = 2 per CU, 2.9 TB/s).
constexpr int AP_RING = 6;
__device__ __forceinline__ int ap_slot(int row) { return (row + 64 * AP_RING) % AP_RING; }   // row >= -64 * AP_RING
static_assert(AP_THREADS == RBLK, "block_store_partials sums the waves of an RBLK-thread block");

// What every launch of the two kernels is given (the host builds it in one place, ap_args): the frames, the level-0 grid
// (ni x nj interior points of an image with Nj columns), the band height, the model parameters and the per-pair tables.
struct ApArgs {
    const double* frames; size_t frame_stride; int Nj, ni, nj, TI; double alpha, beta; int quirks;
    ActiveSet act; const PairParam* pp;
};

// ------------------------------------------------------------------------------------------ the ring
// What one thread loads for one ring row of a strip whose first fine column is q0: x at column q0 + col (l0..l2, three
// fields), x at this thread's halo column (h0..h2, lanes 0 and 127: columns q0 - 1 and q0 + 128) and the image at
// full-image columns q0 + col (li0) and q0 + 128 + col (li1, lanes 0 and 1).  Zero where the grid ends.
template <typename XT>
struct ApRow {
    XT l0 = (XT)0, l1 = (XT)0, l2 = (XT)0, h0 = (XT)0, h1 = (XT)0, h2 = (XT)0;
    double li0 = 0.0, li1 = 0.0;
};

// this thread's halo column qh, and whether it has one inside the grid
__device__ __forceinline__ bool ap_halo(int q0, int col, int nj, int& qh) {
    qh = (col == 0) ? q0 - 1 : q0 + AP_OUT;
    return (col == 0 || col == 127) && qh >= 0 && qh < nj;
}

// x of one row (xr: the row's first point of field 0); col_ok: column q0 + col is inside the grid
template <typename XT>
__device__ __forceinline__ void ap_load_x(ApRow<XT>& ld, const XT* xr, size_t npts, int nj, int q0, int col, bool col_ok) {
    const int q = q0 + col;
    int qh;
    const bool halo = ap_halo(q0, col, nj, qh);
    if (col_ok) { ld.l0 = xr[q]; ld.l1 = xr[npts + q]; ld.l2 = xr[2 * npts + q]; }
    if (halo) { ld.h0 = xr[qh]; ld.h1 = xr[npts + qh]; ld.h2 = xr[2 * npts + qh]; }
}

// one full-image row `ir` (nj + 2 columns).  LOW: the strip may start left of the image (q0 = -1, k_stream_resrestrict0),
// so the columns are checked against 0 as well; a strip of k_stream_apply0 never does and is spared the comparison
template <bool LOW>
__device__ __forceinline__ void ap_load_im(const double* ir, int nj, int q0, int col, double& v0, double& v1) {
    const int fc0 = q0 + col, fc1 = q0 + 128 + col;
    if ((!LOW || fc0 >= 0) && fc0 <= nj + 1) v0 = ir[fc0];
    if (col < 2 && (!LOW || fc1 >= 0) && fc1 <= nj + 1) v1 = ir[fc1];
}

// ... and into slot sl of an image ring: local column li <-> full-image column q0 + li
__device__ __forceinline__ void ap_store_im(double* ring, int sl, int col, double v0, double v1) {
    double* ir = ring + sl * AP_W;
    ir[col] = v0;
    if (col < 2) ir[128 + col] = v1;
}

// a loaded row into slot sl of the rings: x ring local column of q0 + col is col + 1 (local 0 <-> q0 - 1)
template <typename XT>
__device__ __forceinline__ void ap_store_row(XT* xs, double* im, int sl, int col, const ApRow<XT>& ld) {
    XT* xr = xs + sl * 3 * AP_W;
    xr[col + 1] = ld.l0; xr[AP_W + col + 1] = ld.l1; xr[2 * AP_W + col + 1] = ld.l2;
    if (col == 0 || col == 127) {
        const int ch = (col == 0) ? 0 : AP_OUT + 1;
        xr[ch] = ld.h0; xr[AP_W + ch] = ld.h1; xr[2 * AP_W + ch] = ld.h2;
    }
    ap_store_im(im, sl, col, ld.li0, ld.li1);
}

// (A x)(p, q) from the rings: relative row rc of the band, local column col; oU / oD / oL / oR: the row above / below and
// the column left / right of the point lie outside the grid (ghosts fold onto their mirror, corner ghosts count twice).
// Hands back the image coefficients k and the neighbourhood n it formed.  offdiag0 plus the three diagonal lines: not the
// association of apply0_point, whose last bits differ.
template <typename XT>
__device__ __forceinline__ void ap_point(const XT* xs, const double* im, int rc, int col, bool oU, bool oD, bool oL, bool oR,
                                         double alpha, double beta, int quirks, PixCoef& k, Nbr& n, double& y0, double& y1,
                                         double& y2) {
    const int cC = col + 1, cL = oL ? col + 2 : col, cR = oR ? col : col + 2;
    const int sU = ap_slot(rc - 1), sC = ap_slot(rc), sD = ap_slot(rc + 1);
    // point q uses image ring columns col, col + 1, col + 2
    const double* i0 = im + sU * AP_W;
    const double* i1 = im + sC * AP_W;
    const double* i2 = im + sD * AP_W;
    double imm = i0[col], im0 = i0[col + 1], imp = i0[col + 2];
    double i0m = i1[col], i00 = i1[col + 1], i0p = i1[col + 2];
    double ipm = i2[col], ip0 = i2[col + 1], ipp = i2[col + 2];
    k.P = i00;
    k.Dx = (ip0 - im0) / 2;
    k.Dy = quirks ? k.Dx : (i0p - i0m) / 2;
    k.Dxx = ip0 + im0 - 2 * i00;
    k.Dyy = i0p + i0m - 2 * i00;
    k.Dxy = (ipp - ipm - imp + imm) / 4;
    const XT* ru = xs + (oU ? sD : sU) * 3 * AP_W;   // ghost row -1 mirrors row 1, ghost row n mirrors n-2
    const XT* rcn = xs + sC * 3 * AP_W;
    const XT* rd = xs + (oD ? sU : sD) * 3 * AP_W;
    const double sUL = (oU && oL) ? 2.0 : 1.0, sUR = (oU && oR) ? 2.0 : 1.0;
    const double sDL = (oD && oL) ? 2.0 : 1.0, sDR = (oD && oR) ? 2.0 : 1.0;
    n.u[0] = sUL * (double)ru[cL]; n.w[0] = sUL * (double)ru[AP_W + cL];
    n.u[1] = (double)ru[cC];       n.w[1] = (double)ru[AP_W + cC];       n.g[1] = (double)ru[2 * AP_W + cC];
    n.u[2] = sUR * (double)ru[cR]; n.w[2] = sUR * (double)ru[AP_W + cR];
    n.u[3] = (double)rcn[cL];      n.w[3] = (double)rcn[AP_W + cL];      n.g[3] = (double)rcn[2 * AP_W + cL];
    n.u[4] = (double)rcn[cC];      n.w[4] = (double)rcn[AP_W + cC];      n.g[4] = (double)rcn[2 * AP_W + cC];
    n.u[5] = (double)rcn[cR];      n.w[5] = (double)rcn[AP_W + cR];      n.g[5] = (double)rcn[2 * AP_W + cR];
    n.u[6] = sDL * (double)rd[cL]; n.w[6] = sDL * (double)rd[AP_W + cL];
    n.u[7] = (double)rd[cC];       n.w[7] = (double)rd[AP_W + cC];       n.g[7] = (double)rd[2 * AP_W + cC];
    n.u[8] = sDR * (double)rd[cR]; n.w[8] = sDR * (double)rd[AP_W + cR];
    offdiag0(k, alpha, beta, n, y0, y1, y2);
    const double P = k.P;
    y0 += (P * (k.Dxx - 2 * P) - 4 * alpha) * n.u[4] + P * k.Dxy * n.w[4];
    y1 += (P * (k.Dyy - 2 * P) - 4 * alpha) * n.w[4] + P * k.Dxy * n.u[4];
    y2 += (-1 - 4 * beta) * n.g[4] + k.Dx * n.u[4] + k.Dy * n.w[4];
}

// ==========================================================================================
// k_stream_apply0: level-0 operator application y = A x (MODE 0) or y = b - A x (MODE 1), matrix-free,
// streaming over rows through an LDS ring (every array is read once, coalesced; the 9-point neighbourhood and
// the 3x3 image neighbourhood come from LDS).  A block owns a 128-column aligned strip (+1 halo column each
// side) and a band of TI rows; per step the two wave pairs compute two rows.  Optional fused reductions:
// slot 0 = sum y * dotvec (or y * y if dotvec == nullptr and want_yy), slot 1 = sum y * y (dotvec && want_yy);
// per-block partials are written at index blockIdx.y * gridDim.x + blockIdx.x (deterministic two-stage sum).
//
// The two ends of a batch run the same ring (MODE 2 and 3, float64 vectors; their extra arguments travel in ApEnds):
//   MODE 2, prologue of a batch that does not start from zero: the right-hand side b (the expressions of k_rhs_norm, the second
//     frame through a ring of its own), the initial guess x0 (the saved solution src[pair] of `saved`, or the constants where
//     src[pair] < 0 or src == nullptr, as k_gather_guess / k_fill write it), r0 = b - A x0 and its copy, with the block partials of
//     (b, b) in slot 0 and of (r0, r0) in slot 1: frames and guess in, b, x0, r0, r^ out (136 B per pixel instead of 192).
//   MODE 3, epilogue: the norm of b - A x (slot 0, no residual vector) and, from the same rows of x, what k_finalize_functionals
//     computes: the four outputs on the full grid with the mirror fix-up (the owner of interior row / column 1 and n - 2 also
//     writes the border that mirrors it) and the block partials of the three functionals in `fpartials` (96 B instead of 128).
// ==========================================================================================
struct ApEnds {
    const double* saved; const int* src; double c0, c1, c2;   // MODE 2: the guess
    double* xo; double* bo;                                   // MODE 2: x0 and b (written)
    double vscale; double *vx, *vy, *gm, *speed;              // MODE 3: outputs (speed may be nullptr)
    double* fpartials;                                        // MODE 3: [pair][3][nblk] for k_sum3
};

// (MODE 3 carries the outputs and the functionals' sums on top of MODE 1: held to the three waves per SIMD of MODE 1.  For the
// other modes the attribute says 1, which is the default lower bound of a 256-thread kernel: their code is what it was without it)
template <int MODE, typename XT, typename BT, typename YT>
__global__ __launch_bounds__(AP_THREADS) __attribute__((amdgpu_waves_per_eu(MODE == 3 ? 3 : 1))) void k_stream_apply0(
    ApArgs a, const XT* __restrict__ x, const BT* __restrict__ b, YT* __restrict__ y, const double* __restrict__ dotvec,
    int want_yy, double* __restrict__ partials, int nblk, YT* __restrict__ ycopy, ApEnds e) {
    // ycopy (or nullptr): a second copy of the result (the shadow residual of a warm-started solve)
    __shared__ XT xs[AP_RING * 3 * AP_W];
    __shared__ double im[AP_RING * AP_W];
    __shared__ double jm[MODE == 2 ? AP_RING * AP_W : 1];   // MODE 2: the pair's second frame, as im
    // what a mode never takes is known when it is compiled (MODE 2 / 3: no dot partner; MODE 3: the norm alone, no vector)
    const double* const dotv = MODE >= 2 ? nullptr : dotvec;
    const int wyy = MODE == 3 ? 1 : want_yy;
    YT* const yo = MODE == 3 ? nullptr : y;
    YT* const yc = MODE == 3 ? nullptr : ycopy;
    const int pair = a.act.pair(blockIdx.z);
    if (!a.act.on(pair)) return;
    const size_t frame_stride = a.frame_stride;
    const int Nj = a.Nj, ni = a.ni, nj = a.nj, TI = a.TI, quirks = a.quirks;
    double alpha = a.alpha, beta = a.beta;
    int fidx = pair;
    if (a.pp) { alpha = a.pp[pair].alpha; beta = a.pp[pair].beta; fidx = a.pp[pair].frame; }
    const int tid = threadIdx.x;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);   // which of the two rows of a step
    const int col = tid & 127;
    const int q0 = blockIdx.x * AP_OUT, p0 = blockIdx.y * TI;
    const int q = q0 + col;
    const bool col_ok = q < nj;
    const size_t npts = (size_t)ni * nj, off = (size_t)pair * 3 * npts;
    const XT* xp = x + off;
    const double* img = a.frames + (size_t)fidx * frame_stride;
    if (MODE == 2) {   // the guess: a saved solution, or (xp == nullptr) the constants
        const int sp = e.src ? e.src[pair] : -1;
        xp = sp >= 0 ? (const XT*)(e.saved + (size_t)sp * 3 * npts) : nullptr;
    }
    const size_t obase = MODE == 3 ? (size_t)(a.pp ? a.pp[pair].out : pair) * (size_t)(ni + 2) * Nj : 0;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;   // MODE 3: the functionals' sums
    double jn = 0.0;                        // MODE 3: second frame at this thread's point of the next step
    const bool oL = q - 1 < 0, oR = q + 1 >= nj;
    double s0 = 0.0, s1 = 0.0;
    const int nsteps = TI / 2;
    BT bn0 = (BT)0, bn1 = (BT)0, bn2 = (BT)0;   // b and the dot partner of this thread's point of the NEXT step (loaded a step ahead)
    double dn0 = 0.0, dn1 = 0.0, dn2 = 0.0;
    for (int s = -2; s < nsteps; ++s) {
        const int r = 2 * s;
        BT bc0 = bn0, bc1 = bn1, bc2 = bn2;
        const double jc = jn;
        const double dc0 = dn0, dc1 = dn1, dc2 = dn2;
        // ---- global loads of relative row r + 3 + half into registers
        const int rl = r + 3 + half, pl = p0 + rl;
        const bool row_ld = rl <= TI && pl >= 0 && pl < ni;
        const bool irow_ld = rl <= TI && pl + 1 >= 0 && pl + 1 <= ni + 1;
        ApRow<XT> ld;
        double lj0 = 0.0, lj1 = 0.0;
        if (row_ld) {
            if (MODE == 2 && !xp) {
                int qh;
                if (col_ok) { ld.l0 = (XT)e.c0; ld.l1 = (XT)e.c1; ld.l2 = (XT)e.c2; }
                if (ap_halo(q0, col, nj, qh)) { ld.h0 = (XT)e.c0; ld.h1 = (XT)e.c1; ld.h2 = (XT)e.c2; }
            } else {
                ap_load_x(ld, xp + (size_t)pl * nj, npts, nj, q0, col, col_ok);
            }
            if (MODE == 2 && rl >= 0 && rl < TI && col_ok) {   // x0: the rows and columns this block owns
                const size_t idl = off + (size_t)pl * nj + q;
                e.xo[idl] = (double)ld.l0; e.xo[npts + idl] = (double)ld.l1; e.xo[2 * npts + idl] = (double)ld.l2;
            }
        }
        if (irow_ld) {
            const double* ir = img + (size_t)(pl + 1) * Nj;
            ap_load_im<false>(ir, nj, q0, col, ld.li0, ld.li1);
            if (MODE == 2) ap_load_im<false>(ir + frame_stride, nj, q0, col, lj0, lj1);
        }
        {   // b / dot partner of the row this thread computes in the next step
            const int rcn = r + 2 + half, pn = p0 + rcn;
            if (s + 1 >= 0 && rcn < TI && pn < ni && col_ok) {
                const size_t idn = (size_t)pn * nj + q;
                if (MODE == 1) { bn0 = b[off + idn]; bn1 = b[off + npts + idn]; bn2 = b[off + 2 * npts + idn]; }
                if (dotv) { dn0 = dotv[off + idn]; dn1 = dotv[off + npts + idn]; dn2 = dotv[off + 2 * npts + idn]; }
                if (MODE == 3) jn = img[frame_stride + (size_t)(pn + 1) * Nj + q + 1];
            }
        }
        // ---- compute relative row r + half
        const int rc = r + half, p = p0 + rc;
        if (s >= 0 && rc < TI && p < ni && col_ok) {
            PixCoef k;
            Nbr n;
            double y0, y1, y2;
            ap_point(xs, im, rc, col, p - 1 < 0, p + 1 >= ni, oL, oR, alpha, beta, quirks, k, n, y0, y1, y2);
            const size_t idx = (size_t)p * nj + q;
            if (MODE == 2) {   // b as k_rhs_norm forms it (rounded products: no contraction into the residual below)
                const int tU = ap_slot(rc - 1) * AP_W + col, tC = ap_slot(rc) * AP_W + col, tD = ap_slot(rc + 1) * AP_W + col;
                const double dxt = (jm[tD + 1] - jm[tU + 1] - im[tD + 1] + im[tU + 1]) / 2;
                const double dyt = (jm[tC + 2] - jm[tC] - im[tC + 2] + im[tC]) / 2;
                const double dt = jm[tC + 1] - k.P;
                {
#pragma clang fp contract(off)
                    bc0 = -k.P * dxt; bc1 = -k.P * dyt; bc2 = -dt;
                }
                e.bo[off + idx] = bc0; e.bo[off + npts + idx] = bc1; e.bo[off + 2 * npts + idx] = bc2;
                s0 += (double)bc0 * bc0 + (double)bc1 * bc1 + (double)bc2 * bc2;
            }
            if (MODE == 3) {   // functional terms of this pixel, as in k_finalize_functionals
                const double u0 = n.u[4], w0 = n.w[4], g0 = n.g[4];
                const double dt = jc - k.P;
                const double dux = (n.u[7] - n.u[1]) / 2, dwx = (n.w[7] - n.w[1]) / 2, dgx = (n.g[7] - n.g[1]) / 2;
                const double duy = quirks ? dux : (n.u[5] - n.u[3]) / 2;
                const double dwy = quirks ? dwx : (n.w[5] - n.w[3]) / 2;
                const double dgy = quirks ? dgx : (n.g[5] - n.g[3]) / 2;
                const double ee = dt + u0 * k.Dx + w0 * k.Dy + k.P * dux + k.P * dwy - g0;
                f0 += ee * ee;
                f1 += dux * dux + duy * duy + dwx * dwx + dwy * dwy;
                f2 += dgx * dgx + dgy * dgy;
            }
            if (MODE == 3) { bc0 = b[off + idx]; bc1 = b[off + npts + idx]; bc2 = b[off + 2 * npts + idx]; }
            if (MODE >= 1) {
                y0 = (double)bc0 - y0;
                y1 = (double)bc1 - y1;
                y2 = (double)bc2 - y2;
            }
            if (yo) {   // (nullptr: only the reductions are wanted)
                yo[off + idx] = (YT)y0;
                yo[off + npts + idx] = (YT)y1;
                yo[off + 2 * npts + idx] = (YT)y2;
            }
            if (yc) {
                yc[off + idx] = (YT)y0;
                yc[off + npts + idx] = (YT)y1;
                yc[off + 2 * npts + idx] = (YT)y2;
            }
            if (MODE == 2) {
                s1 += y0 * y0 + y1 * y1 + y2 * y2;
            } else if (dotv) {
                s0 += y0 * dc0 + y1 * dc1 + y2 * dc2;
                if (wyy) s1 += y0 * y0 + y1 * y1 + y2 * y2;
            } else if (wyy) {
                s0 += y0 * y0 + y1 * y1 + y2 * y2;
            }
            if (MODE == 3) {   // outputs of this pixel, as in k_finalize_functionals (last: only x of the pixel is still live)
                const double u0 = n.u[4], w0 = n.w[4], g0 = n.g[4];
                const double u = u0 * e.vscale, w = w0 * e.vscale;
                const double sp = e.speed ? sqrt(u * u + w * w) : 0.0;
                auto put = [&](int i, int j) {
                    const size_t t = obase + (size_t)i * Nj + j;
                    e.vx[t] = u; e.vy[t] = w; e.gm[t] = g0;
                    if (e.speed) e.speed[t] = sp;
                };
                // border rows / columns mirror interior row / column 1 and n - 2 (fold): their owner writes them along
                const int iA = p == 1 ? 0 : -1, iB = p == ni - 2 ? ni + 1 : -1;
                const int jA = q == 1 ? 0 : -1, jB = q == nj - 2 ? nj + 1 : -1;
                put(p + 1, q + 1);
                if ((iA & iB & jA & jB) >= 0) {
                    const int ri[3] = {p + 1, iA, iB}, cj[3] = {q + 1, jA, jB};
#pragma unroll
                    for (int a2 = 0; a2 < 3; ++a2)
#pragma unroll
                        for (int c2 = 0; c2 < 3; ++c2)
                            if (a2 + c2 > 0 && ri[a2] >= 0 && cj[c2] >= 0) put(ri[a2], cj[c2]);
                }
            }
        }
        // ---- loaded row -> LDS ring
        if (rl <= TI) {
            const int sl = ap_slot(rl);
            ap_store_row(xs, im, sl, col, ld);
            if (MODE == 2) ap_store_im(jm, sl, col, lj0, lj1);
        }
        __syncthreads();
    }
    if (partials && (dotv || wyy || MODE == 2)) {
        const int blk = blockIdx.y * gridDim.x + blockIdx.x;
        block_store_partials(s0, s1, 0.0, partials, ((dotv && wyy) || MODE == 2) ? 2 : 1, nblk, pair, blk);
        if (MODE == 3) {   // the functionals: alpha and beta scale the block's sums
            __syncthreads();   // thread 0 has read the scratch of the call above
            block_store_partials(f0, f1, f2, e.fpartials, 3, nblk, pair, blk, alpha, beta);
        }
    }
}

// ==========================================================================================
// k_stream_resrestrict0: coarse right-hand side  b_c = R (b - A x)  of level 0 in one pass: the fine residual
// rows come from the ring helpers and ap_point above, i.e. from the very code of k_stream_apply0<1>, but are kept in a
// small LDS ring and immediately restricted (full weighting, R = P^T / 4), so the fine residual is never written to /
// re-read from HBM (I + x(3) + b(3) in, 3/4 out per fine pixel = 62 B instead of 80 + 30).
// A block owns 63 coarse columns x TI/2 coarse rows: fine columns [126 bx - 1, 126 bx + 127), fine rows
// [p0 - 1, p0 + TI) with p0 = by * TI (even).  Its strip can start at fine column -1: the one difference in the loads.
// ==========================================================================================
constexpr int RR_CO = 63;   // coarse columns per strip (fine stride 126)

template <typename XT, typename BT, typename CT2>
__global__ __launch_bounds__(AP_THREADS) void k_stream_resrestrict0(ApArgs a, const XT* __restrict__ x, const BT* __restrict__ b,
                                                                    CT2* __restrict__ bc, int nci, int ncj) {
    __shared__ XT xs[AP_RING * 3 * AP_W];
    __shared__ double im[AP_RING * AP_W];
    __shared__ double rs[AP_RING * 3 * 128];     // residual ring [row][field][fine column of the strip]
    const int pair = a.act.pair(blockIdx.z);
    if (!a.act.on(pair)) return;
    const int Nj = a.Nj, ni = a.ni, nj = a.nj, TI = a.TI;
    double alpha = a.alpha, beta = a.beta;
    int fidx = pair;
    if (a.pp) { alpha = a.pp[pair].alpha; beta = a.pp[pair].beta; fidx = a.pp[pair].frame; }
    const int tid = threadIdx.x;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int col = tid & 127;
    const int q0 = blockIdx.x * (2 * RR_CO) - 1;        // first fine column whose residual the strip computes
    const int p0 = blockIdx.y * TI - 1;                 // first fine row
    const int q = q0 + col;
    const bool col_ok = q >= 0 && q < nj;
    const size_t npts = (size_t)ni * nj, off = (size_t)pair * 3 * npts;
    const XT* xp = x + off;
    const double* img = a.frames + (size_t)fidx * a.frame_stride;
    const bool oL = q - 1 < 0, oR = q + 1 >= nj;
    // restriction phase: thread <-> (field, coarse column of the strip)
    const int ef = tid / RR_CO, em = tid % RR_CO;
    const int ecq = blockIdx.x * RR_CO + em;
    const bool e_on = tid < 3 * RR_CO && ecq < ncj;
    const size_t ncpts = (size_t)nci * ncj;
    const int nsteps = TI / 2 + 1;                      // fine rows p0 .. p0 + TI (relative 0 .. TI)
    BT bn0 = (BT)0, bn1 = (BT)0, bn2 = (BT)0;           // b of this thread's point of the NEXT step (loaded a step ahead: used
                                                        // at the point of use, its latency was exposed in every step)
    for (int s = -2; s <= nsteps + 1; ++s) {
        const int r = 2 * s;
        const BT bc0 = bn0, bc1 = bn1, bc2 = bn2;
        // ---- restriction of coarse row k = s - 2 (fine relative rows 2k, 2k+1, 2k+2), computed in earlier steps
        {
            const int k = s - 2;
            const int cp = blockIdx.y * (TI / 2) + k;
            if (k >= 0 && k < TI / 2 && cp < nci && e_on) {
                double acc = 0.0;
#pragma unroll
                for (int di = -1; di <= 1; ++di) {
                    const int fp = 2 * cp + di;
                    if (fp < 0 || fp >= ni) continue;
                    const double wi = pweight(fp, cp, nci);
                    const double* row = rs + (ap_slot(2 * k + 1 + di) * 3 + ef) * 128;
#pragma unroll
                    for (int dj = -1; dj <= 1; ++dj) {
                        const int fq = 2 * ecq + dj;
                        if (fq < 0 || fq >= nj) continue;
                        acc += wi * pweight(fq, ecq, ncj) * row[2 * em + 1 + dj];
                    }
                }
                bc[(size_t)pair * 3 * ncpts + (size_t)ef * ncpts + (size_t)cp * ncj + ecq] = (CT2)(0.25 * acc);
            }
        }
        // ---- global loads of relative row r + 3 + half into registers
        const int rl = r + 3 + half, pl = p0 + rl;
        const bool need = rl <= TI + 1;
        const bool row_ld = need && pl >= 0 && pl < ni;
        const bool irow_ld = need && pl + 1 >= 0 && pl + 1 <= ni + 1;
        ApRow<XT> ld;
        if (row_ld) ap_load_x(ld, xp + (size_t)pl * nj, npts, nj, q0, col, col_ok);
        if (irow_ld) ap_load_im<true>(img + (size_t)(pl + 1) * Nj, nj, q0, col, ld.li0, ld.li1);
        {   // b of the row this thread computes in the next step
            const int rcn = r + 2 + half, pn = p0 + rcn;
            if (s + 1 >= 0 && rcn <= TI && pn >= 0 && pn < ni && col_ok) {
                const size_t idn = (size_t)pn * nj + q;
                bn0 = b[off + idn]; bn1 = b[off + npts + idn]; bn2 = b[off + 2 * npts + idn];
            }
        }
        // ---- fine residual of relative row r + half -> LDS residual ring
        const int rc = r + half, p = p0 + rc;
        if (s >= 0 && rc <= TI) {
            double y0 = 0.0, y1 = 0.0, y2 = 0.0;
            if (p >= 0 && p < ni && col_ok) {
                PixCoef k;
                Nbr n;
                ap_point(xs, im, rc, col, p - 1 < 0, p + 1 >= ni, oL, oR, alpha, beta, a.quirks, k, n, y0, y1, y2);
                y0 = (double)bc0 - y0;
                y1 = (double)bc1 - y1;
                y2 = (double)bc2 - y2;
            }
            double* rr = rs + (ap_slot(rc) * 3) * 128 + col;
            rr[0] = y0; rr[128] = y1; rr[256] = y2;
        }
        // ---- loaded row -> LDS ring
        if (need) ap_store_row(xs, im, ap_slot(rl), col, ld);
        __syncthreads();
    }
}

}  // namespace vof
