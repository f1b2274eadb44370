// vof_sweepst.hpp - the fused sweeps of the stored levels: k_sweep (float32 / float64 stencils), k_sweep_st (packed stencil
// formats) and k_sweep_st2 (two sweeps of a packed format in one pass).  Included by vof.hip after vof_device.hpp, which holds what
// the level-0 passes share with them (SW_HALO, SW_RING, sw_slot, sw_wrap, sw_strip).
#pragma once
#include "vof_device.hpp"

namespace vof {

// ==========================================================================================
// Fused 4-colour block-GS sweep, streaming over rows (the north-star kernel).
//
// One launch = one full sweep (colours 0,1,2,3 in that order; po = 1 gives the order 3,2,1,0).
// A block owns a strip of SW_OUT output columns (+4 halo columns each side, recomputed) and a band of
// TI rows, and marches down the band keeping a ring of SW_RING rows of x (and of the image) in LDS.
// The four colours are software-pipelined over rows so that every update sees exactly the neighbour
// states of the global colour-by-colour order:
//     step s (e = 2s):  wave 0: colour 0 on row e      wave 1: colour 1 on row e-2
//                       wave 2: colour 2 on row e-5    wave 3: colour 3 on row e-7      (rows relative
// to the band start, "even" = colour-0/1 rows).  Even rows only need OLD odd rows, odd rows need the
// finished even rows above and below, so no halo rows are recomputed except the one even row below the
// band.  Each array is read once and written once per sweep: x(3) + b(3) + I(1) in, x(3) out = 80 B/pixel
// (x_in == nullptr means a zero initial guess: 56 B/pixel).  Out of place (x_in -> x_out) because
// neighbouring blocks read each other's halo.
// LDS: columns are stored parity-split (even columns first) so the stride-2 accesses of a colour are
// contiguous (no bank conflicts).
// ==========================================================================================

// The strip geometry of the stored levels (the matrix-free level 0 has kernels of its own, k_sweep0*, with 120 owned columns
// of 128 in LDS):
//  GeoB: 128 owned columns, 128-column aligned, so the coefficient rows of the colour-split stencil planes are
//        read in whole aligned cache lines; four colour waves, and a 5th wave that recomputes the six halo points.
//  GeoR: the two sweeps of k_sweep_st2 (see there): seven stage waves and a wave of 21 halo points, 8 halo columns, 22 ring rows.
struct GeoB {
    static constexpr int OUT = 128, HALO = SW_HALO, W = 136, THREADS = 320, RING = SW_RING;
};
struct GeoR {
    static constexpr int OUT = 128, HALO = 8, W = 144, THREADS = 512, RING = 22;
};
template <class G> __device__ __forceinline__ int sw_cs(int lc) { return (lc & 1) * (G::W / 2) + (lc >> 1); }

// k_sweep: the sweep with the stencil of a point in one coefficient set (81 float32 or float64 words).
// 32-bit format: the coefficient words of the NEXT step's point are loaded into registers before the step barrier (the registers
// of the current step are dead by then), so their latency overlaps the barrier and the next step's row traffic.  double
// stencils (162 registers) are loaded at use.
// Register budget (launch bound): 2 waves per SIMD, i.e. no limit that forces spills.  Measured: forcing 128 VGPRs (4 waves
// per SIMD, 3 workgroups per CU) spills ~110 bytes per thread and halves the kernel's speed; the compiler's own choice
// (~154 registers for the packed bfloat16 format, 2 workgroups of 5 waves per CU) runs at 4.1 TB/s.
template <typename CT, typename VT>
__global__ __launch_bounds__(GeoB::THREADS, 2) void k_sweep(const typename CoefFmt<CT>::word_t* C, int ni, int nj, int TI, int po,
                                                            int nx, int ny, int nz, const VT* __restrict__ x_in, VT* __restrict__ x_out,
                                                            const VT* __restrict__ b, const ActiveSet act) {
    typedef GeoB G;
    typedef typename CoefFmt<CT>::word_t word_t;
    constexpr int W = G::W, OUT = G::OUT, THREADS = G::THREADS, PLANES = CoefFmt<CT>::PLANES;
    constexpr bool kPrefetch = sizeof(word_t) == 4;
    extern __shared__ double sw_lds[];
    VT* xs = reinterpret_cast<VT*>(sw_lds);                                                     // [SW_RING][3][W]
    int bx, by, pair;
    if (!sw_strip(act, nx, ny, nz, bx, by, pair)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keeps the stage's row arithmetic scalar
    const int p0 = by * TI - po;
    // strips are always 128-aligned, po only swaps the column parity of the stages
    const int qs = bx * OUT - SW_HALO;
    const size_t npts = (size_t)ni * nj, off = (size_t)pair * 3 * npts;
    const VT* xin = x_in ? x_in + off : nullptr;
    VT* xout = x_out + off;
    const VT* bp = b + off;
    const CLay L(ni, nj);
    const word_t* Cp = C + (size_t)pair * PLANES * L.plane;   // [pair][PLANES][colour-split plane]

    // ---- stage of this lane.  Waves 0-3: colour = wave.  Wave 4 recomputes the six halo points.
    // column parity of stage c is (c & 1) ^ po; for po = 1 the halo pattern is the mirror image
    int stage = wave, lc = SW_HALO + 2 * lane + ((wave & 1) ^ po);
    bool lane_on = true;
    if (wave == 4) {
        const int hs[6] = {0, 0, 0, 1, 1, 2};
        const int hl[6] = {2, SW_HALO + OUT, SW_HALO + OUT + 2, 3, SW_HALO + OUT + 1, SW_HALO + OUT};
        lane_on = lane < 6;
        stage = hs[lane_on ? lane : 0];
        lc = hl[lane_on ? lane : 0];
        if (po) lc = W - 1 - lc;
    }
    // per-lane constants of the stage point: x-ring column slots of q-1, q, q+1, column parts of the colour-split stencil index
    // and of the index into b
    const int q = qs + lc;
    const bool col_ok = lane_on && (q >= 0) && (q < nj);
    const int qc = col_ok ? q : 0, lcc = col_ok ? lc : 2;      // keep the index math of masked lanes in range
    const int cC = sw_cs<G>(lcc), uL = sw_cs<G>(lcc - 1), uR = sw_cs<G>(lcc + 1);
    const size_t cq = (size_t)(qc & 1) * L.sub + (size_t)(qc >> 1);
    const size_t bcol = col_ok ? (size_t)q : 0;

    // ---- cooperative load-in / write-out of 2 rows x 3 fields x W columns per step (W = 136, 320 threads): generic
    // element mapping, up to three elements per thread
    int m_lds[3], m_rs[3];
    size_t m_g[3];
    bool m_ld[3], m_st[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int idx = tid + THREADS * k;
        bool on = idx < 2 * 3 * W;
        idx = on ? idx : 0;
        int f = (idx % (3 * W)) / W, mlc = idx % W, qq = qs + mlc;
        bool cv = on && qq >= 0 && qq < nj;
        m_rs[k] = idx / (3 * W);
        m_lds[k] = f * W + sw_cs<G>(mlc);
        m_g[k] = (size_t)f * npts + (size_t)(cv ? qq : 0);
        m_ld[k] = cv;
        m_st[k] = cv && mlc >= SW_HALO && mlc < SW_HALO + OUT;
        if (!on) m_lds[k] = -1;
    }

    const int sro = (stage == 0) ? 0 : (stage == 1) ? -2 : (stage == 2) ? -5 : -7;   // row of the stage relative to e
    const int rr_lo = (stage < 2) ? 0 : 1, rr_hi = (stage < 2) ? TI : TI - 1;
    // row part of the colour-split coefficient index
    auto crow = [&](const int p) { return (size_t)((p & 1) << 1) * L.sub + (size_t)(p >> 1) * L.hj; };
    double bn0 = 0, bn1 = 0, bn2 = 0;  // b of the stage's point for the NEXT step (prefetched)
    CoefSet<CT> cf;            // coefficients of the next step's point
    if (kPrefetch) cf.clear();
    const int s_end = TI / 2 + 4;
    int slotA = sw_slot(-2);   // ring slot of relative row e + 2, advanced by 2 per step
    for (int s = -2; s <= s_end; ++s, slotA = sw_wrap(slotA + 2)) {
        const int e = 2 * s;
        // the two rows that leave (e-10, e-9) / enter (e+2, e+3) the ring share the slots slotA, slotA + 1
        const int slotB = slotA + 1;
        VT lx[3];
        const bool do_load = (e + 2 <= TI + 1);
        // (1) write-out of the rows that became final: relative rows e-10, e-9
        {
            const int rrA = e - 10, rrB = e - 9, pA = p0 + rrA, pB = p0 + rrB;
            const bool okA = rrA >= 0 && rrA < TI && pA >= 0 && pA < ni;
            const bool okB = rrB >= 0 && rrB < TI && pB >= 0 && pB < ni;
            if (okA || okB) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const bool rowok = m_rs[k] ? okB : okA;
                    if (m_st[k] && rowok) {
                        const int slot = m_rs[k] ? slotB : slotA;
                        const size_t prow = (size_t)(m_rs[k] ? pB : pA) * nj;
                        xout[prow + m_g[k]] = xs[slot * 3 * W + m_lds[k]];
                    }
                }
            }
        }
        // (2) global loads of relative rows e+2, e+3 into registers
        {
            const int pA = p0 + e + 2, pB = pA + 1;
            const bool okA = do_load && xin && pA >= 0 && pA < ni, okB = do_load && xin && pB >= 0 && pB < ni;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lx[k] = (VT)0;
                const bool rowok = m_rs[k] ? okB : okA;
                if (m_ld[k] && rowok) lx[k] = xin[(size_t)(m_rs[k] ? pB : pA) * nj + m_g[k]];
            }
        }
        // (3) this step's b (prefetched during the previous step) and the prefetch for the next step
        double b0 = bn0, b1 = bn1, b2 = bn2;
        const int rrn = e + 2 + sro, pn = p0 + rrn;
        const bool next_ok = col_ok && rrn >= rr_lo && rrn <= rr_hi && pn >= 0 && pn < ni;
        if (next_ok) {
            const VT* brow = bp + (size_t)pn * nj;
            bn0 = (double)brow[bcol]; bn1 = (double)brow[npts + bcol]; bn2 = (double)brow[2 * npts + bcol];
        }
        // (4) the stage of this wave: block Gauss-Seidel update of its point
        {
            const int rr = e + sro, p = p0 + rr;
            if (col_ok && rr >= rr_lo && rr <= rr_hi && p >= 0 && p < ni) {
                // rows rr-1, rr, rr+1 are (e+2) + (sro - 3), (sro - 2), (sro - 1); sro - 3 >= -10 > -SW_RING
                const int sU = sw_wrap(slotA + SW_RING + sro - 3), sC = sw_wrap(slotA + SW_RING + sro - 2),
                          sD = sw_wrap(slotA + SW_RING + sro - 1);
                const int rowo[3] = {sU * 3 * W, sC * 3 * W, sD * 3 * W};
                const int colo[3] = {uL, cC, uR};
                CoefSet<CT> cl;
                if (!kPrefetch) cl.load(Cp + crow(p) + cq, L.plane);
                const CoefSet<CT>& cu = kPrefetch ? cf : cl;
                double y0 = 0, y1 = 0, y2 = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const VT* row = xs + rowo[a];
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        if (a == 1 && bb == 1) continue;
                        double xu = (double)row[colo[bb]], xw = (double)row[W + colo[bb]], xg = (double)row[2 * W + colo[bb]];
                        const int t0 = (a * 3 + bb) * 9;
                        y0 += cu.get(t0 + 0) * xu + cu.get(t0 + 1) * xw + cu.get(t0 + 2) * xg;
                        y1 += cu.get(t0 + 3) * xu + cu.get(t0 + 4) * xw + cu.get(t0 + 5) * xg;
                        y2 += cu.get(t0 + 6) * xu + cu.get(t0 + 7) * xw + cu.get(t0 + 8) * xg;
                    }
                }
                double D[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) D[t] = cu.get(36 + t);
                double u, w, gm;
                solve3(D, b0 - y0, b1 - y1, b2 - y2, u, w, gm);
                VT* row = xs + rowo[1] + cC;
                row[0] = (VT)u; row[W] = (VT)w; row[2 * W] = (VT)gm;
            }
        }
        // (5) loaded rows -> LDS ring (the slots freed by (1), same thread <-> element mapping)
        if (do_load) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (m_lds[k] >= 0) xs[(m_rs[k] ? slotB : slotA) * 3 * W + m_lds[k]] = lx[k];
        }
        // (6) coefficient prefetch for the next step's point (float stencils).  (wave-uniform base pointer) + (32-bit lane index):
        // the plane offsets stay in scalar registers, see CoefSet::load_u
        if (kPrefetch) {
            if (wave < 4) {   // colour waves: the row is wave-uniform -> scalar row / plane offsets
                const int pnu = __builtin_amdgcn_readfirstlane(pn);
                if (next_ok) cf.load_u(Cp + crow(pnu), L.plane, (unsigned)cq);
            } else if (next_ok) {   // halo wave: a row per lane
                cf.load_u(Cp, L.plane, (unsigned)(crow(pn) + cq));
            }
        }
        __syncthreads();
    }
}

// ==========================================================================================
// k_sweep_st: the fused 4-colour sweep of a STORED level (32-bit stencil formats, GeoB geometry) with the coefficient stream
// decoupled from the step barrier.  Same schedule, ring and results as k_sweep; what changes is when the memory operations are
// issued and how they are waited for:
//  * two coefficient sets in registers: the 45 words of the point of step s + 1 are requested at the START of step s (k_sweep
//    requests them at its end, i.e. just before the barrier after which they are needed - the "prefetch" hid a barrier, not a
//    memory latency), after the row loads of the step, so that waiting for the rows never waits for the coefficients
//    (vector-memory results return in order);
//  * the steps in which every row touched exists run a body whose loads are all unconditional (clamped addresses): with
//    loads inside branches the compiler cannot count the operations in flight and emits s_waitcnt vmcnt(0), which drains
//    the whole stream at every wait.  These steps have their own loop (two steps per iteration, static register sets), entered
//    after a full wait, so the counts on its back edge are exact;
//  * the point update reads its neighbours row by row, so that two coefficient sets fit the register budget of 10 waves
//    per CU.
// k_sweep_st2 (below) runs two such sweeps in one march and must give the same bits.  Its lane set-up, coefficient requests, point
// update, row traffic and step walk repeat this kernel's, statement for statement: a change to one is made in both.
// ==========================================================================================
constexpr unsigned SWST_NO_UPDATE = 0x8000u;   // block mask value of a colour wave that leaves its colour alone
template <typename CT> struct SweepStBudget {
    // waves per SIMD the register allocation aims at: 3 (170 registers; two workgroups of five waves per CU) with the two sets of 36
    // bfloat16 words, 4 (128 registers; three workgroups) with the two sets of 18 words of the 8-bit format
    static constexpr int kF8Waves = 4;
    static constexpr int kMinWaves = std::is_same<CT, CoefF8>::value ? kF8Waves : 3;
};

// OT: storage type of x_out (double for the float32 level whose result the float64 level above interpolates)
// EC: the sweep starts from x_in + P ecoarse (bilinear interpolation of the coarse-grid correction, as k_prolong_add computes it):
// the coarse rows go through a 3-row LDS ring, one new row per step requested a step ahead, and are added to the fine rows on
// their way into the x ring - the separate prolongation pass (read + write of x) disappears
template <typename CT, typename VT, typename OT = VT, bool EC = false>
__global__ __launch_bounds__(GeoB::THREADS, SweepStBudget<CT>::kMinWaves) void k_sweep_st(const typename CoefFmt<CT>::word_t* __restrict__ C, int ni, int nj, int TI,
                                                               int po, int nx, int ny, int nz, const VT* __restrict__ x_in,
                                                               OT* __restrict__ x_out, const VT* __restrict__ b,
                                                               const ActiveSet act, const VT* __restrict__ ecoarse, int nci,
                                                               int ncj, int skip0) {
    // skip0: x_in comes straight from a sweep in REVERSE colour order with the same b (the post-smoothing of the previous
    // visit of a W-cycle): colour 0 was updated last there and none of its neighbours has changed since - updating it again
    // would reproduce its value, so this forward sweep leaves colour 0 alone (no stencil words, no arithmetic; same bits)
    typedef GeoB G;
    typedef typename CoefFmt<CT>::word_t word_t;
    constexpr int W = G::W, OUT = G::OUT, THREADS = G::THREADS, PLANES = CoefFmt<CT>::PLANES;
    extern __shared__ double sw_lds[];
    VT* xs = reinterpret_cast<VT*>(sw_lds);                                                     // [SW_RING][3][W]
    constexpr int CRW = W / 2 + 2;                                                              // coarse ring width
    VT* cr = xs + SW_RING * 3 * W;                                                              // [3][3][CRW] (EC)
    int bx, by, pair;
    if (!sw_strip(act, nx, ny, nz, bx, by, pair)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p0 = by * TI - po;
    const int qs = bx * OUT - SW_HALO;
    const size_t npts = (size_t)ni * nj, off = (size_t)pair * 3 * npts;
    const VT* xin = x_in ? x_in + off : nullptr;
    OT* xout = x_out + off;
    const VT* bp = b + off;
    const CLay L(ni, nj);
    const word_t* Cp = C + (size_t)pair * PLANES * L.plane;

    // ---- stage of this lane.  Waves 0-3: colour = wave; wave 4 recomputes the six halo points (see k_sweep).
    int stage = wave, lc;
    bool lane_on = true;
    lc = SW_HALO + 2 * lane + ((wave & 1) ^ po);
    if (wave == 4) {
        const int hs[6] = {0, 0, 0, 1, 1, 2};
        const int hl[6] = {2, SW_HALO + OUT, SW_HALO + OUT + 2, 3, SW_HALO + OUT + 1, SW_HALO + OUT};
        lane_on = lane < 6;
        stage = hs[lane_on ? lane : 0];
        lc = hl[lane_on ? lane : 0];
        if (po) lc = W - 1 - lc;
    }
    const int q = qs + lc;
    const bool col_ok = lane_on && (q >= 0) && (q < nj);
    const int qc = col_ok ? q : 0, lcc = col_ok ? lc : 2;
    const int cC = sw_cs<G>(lcc), uL = sw_cs<G>(lcc - 1), uR = sw_cs<G>(lcc + 1);
    const unsigned ccq = (unsigned)((size_t)(qc & 1) * L.sub + (size_t)(qc >> 1));   // column part of the stencil index
    const unsigned bcol = (unsigned)qc;
    // ---- cooperative load-in / write-out of 2 rows x 3 fields x W columns per step: thread <-> (row, column) of the two
    // rows (2 x 136 of the 320 threads), the three fields are the unrolled index.  The mapping is RECOMPUTED where it is used,
    // from a thread index the compiler cannot see through: as loop invariants these values sat in registers across the point
    // update, where the two coefficient sets leave no room (a spill reload is a scratch load, and waiting for one drains the
    // whole coefficient stream).
    auto opaque_tid = [&]() { int t = tid; asm volatile("" : "+v"(t)); return t; };
    struct XMap { int row, col, q, lds; unsigned g; bool on, ld, st; };
    auto xmap = [&](const int t) {
        XMap m;
        m.row = t >= W ? 1 : 0; m.col = t - m.row * W;
        m.on = t < 2 * W;
        m.q = qs + m.col;
        m.ld = m.on && m.q >= 0 && m.q < nj;
        m.st = m.ld && m.col >= SW_HALO && m.col < SW_HALO + OUT;
        m.g = m.ld ? (unsigned)m.q : 0u;
        m.lds = sw_cs<G>(m.on ? m.col : 0);
        return m;
    };
    // coarse-correction ring: thread <-> (field, coarse column) of the row requested in a step; fine column q interpolates
    // from the coarse columns (q >> 1) and (q >> 1) + 1
    const size_t ncpts = (size_t)nci * ncj;
    const VT* ec = EC ? ecoarse + (size_t)pair * 3 * ncpts : nullptr;
    const int cqs = qs >> 1;                                   // coarse column of ring column 0 (qs is even)
    struct CMap { int f, c; unsigned g; bool on, cv; };
    auto cmap = [&](const int t) {
        CMap m;
        const int f = t / CRW;
        m.c = t - f * CRW;
        m.on = EC && t < 3 * CRW;
        m.f = m.on ? f : 0;
        const int crq = cqs + m.c;
        m.cv = m.on && crq >= 0 && crq < ncj;
        m.g = m.cv ? (unsigned)crq : 0u;
        return m;
    };
    auto cr_slot = [](int k) { return ((k % 3) + 3) % 3; };
    if (EC) {   // prologue: the two coarse rows the first step's fine rows need
        const CMap cm = cmap(tid);
        const int k0 = (p0 - 2) >> 1;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int k = k0 + d;
            VT v = (VT)0;
            if (cm.cv && k >= 0 && k < nci) v = ec[(size_t)cm.f * ncpts + (size_t)k * ncj + cm.g];
            if (cm.on) cr[(cr_slot(k) * 3 + cm.f) * CRW + cm.c] = v;
        }
        __syncthreads();
    }
    const int sro = (stage == 0) ? 0 : (stage == 1) ? -2 : (stage == 2) ? -5 : -7;
    const int rr_lo = (stage < 2) ? 0 : 1, rr_hi = (stage < 2) ? TI : TI - 1;
    const bool uni = wave < 4;                           // colour waves: the stage's row is wave-uniform
    const bool upd_ok = !(skip0 && po == 0 && stage == 0);   // (halo lanes of colour 0 under skip0)
    const int sro_u = __builtin_amdgcn_readfirstlane(sro);

    // coefficients of the stage's point, this step's / the next step's: two sets of the off-diagonal words (planes 0 .. ND - 1),
    // one set of the diagonal block (planes ND ..), which is requested when the update that used the previous one is done
    constexpr int ND = CoefFmt<CT>::ND;   // (bfloat16: 36 words + 9 floats; 8-bit floats: 18 words + 9 floats + the row units)
    constexpr bool F8 = std::is_same<CT, CoefF8>::value;
    constexpr int PW = F8 ? 4 : 2;         // off-diagonal coefficients per word
    static_assert(CoefPacked<CT>::value, "k_sweep_st is written for the packed stencil formats");
    word_t cw[2][ND], dg[PLANES - ND];
    VT bq[3];                                            // b of the stage's point: requested with the diagonal block
#pragma unroll
    for (int k = 0; k < ND; ++k) cw[0][k] = cw[1][k] = 0;
#pragma unroll
    for (int k = 0; k < PLANES - ND; ++k) dg[k] = 0;
    bq[0] = bq[1] = bq[2] = (VT)0;
    auto offd = [](const word_t* w, int j) {   // off-diagonal coefficient j (0..71) of a set (CoefF8: in the units of its row)
        if constexpr (F8) {
            return (double)f8_decode(w[j >> 2], j & 3);
        } else {
            const uint32_t v = w[j >> 1];
            return (double)__uint_as_float((j & 1) ? (v & 0xFFFF0000u) : (v << 16));
        }
    };

    // base pointer (wave-uniform part) and lane index of the stencil words of the stage's point in row pn
    auto point_base = [&](const int pn, const word_t*& base, unsigned& idx, const bool fast) {
        if (fast && uni) {
            const int pnu = __builtin_amdgcn_readfirstlane(pn);
            base = Cp + (size_t)((pnu & 1) << 1) * L.sub + (size_t)(pnu >> 1) * L.hj;
            idx = ccq;
        } else {
            base = Cp;
            idx = (unsigned)((size_t)((pn & 1) << 1) * L.sub + (size_t)(pn >> 1) * L.hj) + ccq;
        }
    };
    // off-diagonal stencil words of the stage's point of the step with e = eN -> set J
    // (mask_tag: bit d set = the neighbour block d can meet a non-zero neighbour - all eight blocks, except in a sweep from
    // zero, see below; word k of the packed format holds the coefficients 2k, 2k + 1 of the off-diagonal list)
    auto fetch_point = [&](auto fast_tag, auto jtag, auto mask_tag, const int eN) {
        constexpr bool FAST = decltype(fast_tag)::value;
        constexpr int J = decltype(jtag)::value;
        constexpr unsigned MASK = decltype(mask_tag)::value;
        const int rrn = eN + sro, pn = p0 + rrn;
        if (MASK != 0u && MASK != SWST_NO_UPDATE && (FAST || (col_ok && rrn >= rr_lo && rrn <= rr_hi && pn >= 0 && pn < ni))) {
            const word_t* base; unsigned idx;
            point_base(pn, base, idx, FAST);
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                bool need = false;
#pragma unroll
                for (int u = 0; u < PW; ++u) {
                    const int dd = (PW * k + u) / 9, d = dd < 4 ? dd : dd + 1;
                    need = need || ((MASK >> d) & 1u);
                }
                if (need) cw[J][k] = (base + (size_t)k * L.plane)[idx];
            }
        }
    };
    // diagonal block and b of the stage's point of the step with e = eN
    auto fetch_diag = [&](auto fast_tag, auto mask_tag, const int eN) {
        constexpr bool FAST = decltype(fast_tag)::value;
        constexpr bool NOUP = decltype(mask_tag)::value == SWST_NO_UPDATE;
        const int rrn = eN + sro, pn = p0 + rrn;
        if (!NOUP && (FAST || (col_ok && rrn >= rr_lo && rrn <= rr_hi && pn >= 0 && pn < ni))) {
            const word_t* base; unsigned idx;
            point_base(pn, base, idx, FAST);
#pragma unroll
            for (int k = 0; k < PLANES - ND; ++k) dg[k] = (base + (size_t)(ND + k) * L.plane)[idx];
            const VT* brow = bp + (size_t)pn * nj + bcol;
            bq[0] = brow[0]; bq[1] = brow[npts]; bq[2] = brow[2 * npts];
        }
    };

    int slotA = sw_slot(-2);   // ring slot of relative row e + 2, advanced by 2 per step
    // JC: set of this step's point, 1 - JC: set requested for the next step
    auto step = [&](auto fast_tag, auto jtag, auto mask_tag, const int e) {
        constexpr bool FAST = decltype(fast_tag)::value;
        constexpr int JC = decltype(jtag)::value;
        constexpr unsigned MASK = decltype(mask_tag)::value;
        const int slotB = slotA + 1;
        const bool do_load = FAST ? true : (e + 2 <= TI + 1);
        const XMap m1 = xmap(opaque_tid());
        // (1) write-out of the rows that became final: relative rows e - 10, e - 9
        {
            const int rrA = e - 10, rrB = e - 9, pA = p0 + rrA, pB = p0 + rrB;
            const bool okA = FAST ? true : (rrA >= 0 && rrA < TI && pA >= 0 && pA < ni);
            const bool okB = FAST ? true : (rrB >= 0 && rrB < TI && pB >= 0 && pB < ni);
            const bool rowok = m1.row ? okB : okA;
            if (m1.st && rowok) {
                const int slot = m1.row ? slotB : slotA;
                OT* orow = xout + (size_t)(m1.row ? pB : pA) * nj + m1.g;
                const VT* lrow = xs + slot * 3 * W + m1.lds;
                orow[0] = (OT)lrow[0]; orow[npts] = (OT)lrow[W]; orow[2 * npts] = (OT)lrow[2 * W];
            }
        }
        // (2) rows e + 2, e + 3 -> registers (moved into the ring in (5)), then the next step's point
        VT lx[3] = {(VT)0, (VT)0, (VT)0};
        if (xin) {
            const int pR = p0 + e + 2 + m1.row;
            if (FAST) {
                const VT* irow = xin + (size_t)pR * nj + m1.g;
                // (columns outside the grid take the value of a clamped address instead of 0: they only ever meet the zero
                // coefficients of out-of-grid neighbours, and a select here would be a wait for the load just issued)
                lx[0] = irow[0]; lx[1] = irow[npts]; lx[2] = irow[2 * npts];
            } else if (m1.ld && do_load && pR >= 0 && pR < ni) {
                const VT* irow = xin + (size_t)pR * nj + m1.g;
                lx[0] = irow[0]; lx[1] = irow[npts]; lx[2] = irow[2 * npts];
            }
        }
        VT crv = (VT)0;                                   // element of the coarse row the NEXT step needs
        const int knew = ((p0 + e + 4) >> 1) + 1;
        const bool kok = knew >= 0 && knew < nci;
        if (EC) {
            const CMap cm = cmap(opaque_tid());
            if (FAST) crv = ec[(size_t)cm.f * ncpts + (size_t)(kok ? knew : 0) * ncj + cm.g];
            else if (cm.cv && kok) crv = ec[(size_t)cm.f * ncpts + (size_t)knew * ncj + cm.g];
        }
        fetch_point(fast_tag, std::integral_constant<int, 1 - JC>{}, mask_tag, e + 2);
        // (4) the stage of this lane: block Gauss-Seidel update of its point, neighbours read row by row
        {
            const int rr = e + sro, p = p0 + rr;
            if (MASK != SWST_NO_UPDATE && col_ok && upd_ok && (FAST || (rr >= rr_lo && rr <= rr_hi && p >= 0 && p < ni))) {
                const int sU = sw_wrap(slotA + SW_RING + sro - 3), sC = sw_wrap(slotA + SW_RING + sro - 2),
                          sD = sw_wrap(slotA + SW_RING + sro - 1);
                const int rowo[3] = {sU * 3 * W, sC * 3 * W, sD * 3 * W};
                const int colo[3] = {uL, cC, uR};
                const word_t* c_ = cw[JC];
                double y0 = 0, y1 = 0, y2 = 0;
                // CoefF8: one sum per block position, in the units of that position (float32 sums for float32 vectors: measured, no
                // faster and no fewer registers)
                typedef double AT;
                AT yp[F8 ? 9 : 1];
                if constexpr (F8) {
#pragma unroll
                    for (int t = 0; t < 9; ++t) yp[t] = 0;
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const VT* row = xs + rowo[a];
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        if (a == 1 && bb == 1) continue;
                        if (!((MASK >> (a * 3 + bb)) & 1u)) continue;   // (a sweep from zero: this neighbour is still zero)
                        double xu = (double)row[colo[bb]], xw = (double)row[W + colo[bb]], xg = (double)row[2 * W + colo[bb]];
                        const int d = a * 3 + bb, t0 = (d < 4 ? d : d - 1) * 9;
                        if constexpr (F8) {
                            const AT au = (AT)row[colo[bb]], aw = (AT)row[W + colo[bb]], ag = (AT)row[2 * W + colo[bb]];
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
                                yp[3 * r + 0] += (AT)f8_decode(c_[(t0 + 3 * r + 0) >> 2], (t0 + 3 * r + 0) & 3) * au;
                                yp[3 * r + 1] += (AT)f8_decode(c_[(t0 + 3 * r + 1) >> 2], (t0 + 3 * r + 1) & 3) * aw;
                                yp[3 * r + 2] += (AT)f8_decode(c_[(t0 + 3 * r + 2) >> 2], (t0 + 3 * r + 2) & 3) * ag;
                            }
                        } else {
                            y0 += offd(c_, t0 + 0) * xu + offd(c_, t0 + 1) * xw + offd(c_, t0 + 2) * xg;
                            y1 += offd(c_, t0 + 3) * xu + offd(c_, t0 + 4) * xw + offd(c_, t0 + 5) * xg;
                            y2 += offd(c_, t0 + 6) * xu + offd(c_, t0 + 7) * xw + offd(c_, t0 + 8) * xg;
                        }
                    }
                    asm volatile("" ::: "memory");   // keep the LDS reads of the next row behind this row's arithmetic
                }
                double Dm[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) Dm[t] = (double)__uint_as_float(dg[t]);
                if constexpr (F8) {
                    y0 = (double)yp[0] * (double)f8_unit(dg[9], 0) + (double)yp[1] * (double)f8_unit(dg[9], 1) + (double)yp[2] * (double)f8_unit(dg[9], 2);
                    y1 = (double)yp[3] * (double)f8_unit(dg[10], 0) + (double)yp[4] * (double)f8_unit(dg[10], 1) + (double)yp[5] * (double)f8_unit(dg[10], 2);
                    y2 = (double)yp[6] * (double)f8_unit(dg[11], 0) + (double)yp[7] * (double)f8_unit(dg[11], 1) + (double)yp[8] * (double)f8_unit(dg[11], 2);
                }
                double u, w, gm;
                solve3(Dm, (double)bq[0] - y0, (double)bq[1] - y1, (double)bq[2] - y2, u, w, gm);
                VT* row = xs + rowo[1] + cC;
                row[0] = (VT)u; row[W] = (VT)w; row[2 * W] = (VT)gm;
            }
        }
        fetch_diag(fast_tag, mask_tag, e + 2);   // the diagonal block of the next step's point (the registers are free now)
        // (5) loaded rows -> LDS ring (the slots freed by (1), same thread <-> element mapping)
        const XMap m5 = xmap(opaque_tid());
        if (do_load && m5.on) {
            if (EC) {   // + (P e)(pR, q) from the coarse ring; same terms in the same order as k_prolong_add
                const int pR = p0 + e + 2 + m5.row;
                if (m5.ld && (FAST || (pR >= 0 && pR < ni))) {
                    const int cp = pR >> 1;
                    const bool ipi = (pR & 1) && (cp + 1 < nci);
                    const bool ipj = (m5.q & 1) && ((m5.q >> 1) + 1 < ncj);
                    const double wi0 = ipi ? 0.5 : 1.0, wj0 = ipj ? 0.5 : 1.0;
                    const int ilcq = (m5.q >> 1) - cqs;                    // ring column of (q >> 1)
                    const VT* c0 = cr + cr_slot(cp) * 3 * CRW + ilcq;
                    const VT* c1 = cr + cr_slot(cp + 1) * 3 * CRW + ilcq;
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        double v = wi0 * wj0 * (double)c0[f * CRW];
                        if (ipj) v += wi0 * 0.5 * (double)c0[f * CRW + 1];
                        if (ipi) {
                            v += 0.5 * wj0 * (double)c1[f * CRW];
                            if (ipj) v += 0.25 * (double)c1[f * CRW + 1];
                        }
                        lx[f] = (VT)((double)lx[f] + v);
                    }
                }
            }
            VT* lrow = xs + (m5.row ? slotB : slotA) * 3 * W + m5.lds;
            lrow[0] = lx[0]; lrow[W] = lx[1]; lrow[2 * W] = lx[2];
        }
        if (EC && do_load) {
            const CMap cm = cmap(opaque_tid());
            if (cm.on) cr[(cr_slot(knew) * 3 + cm.f) * CRW + cm.c] = (cm.cv && kok) ? crv : (VT)0;
        }
        slotA = sw_wrap(slotA + 2);
        __syncthreads();
    };

    // Steps s = -2 .. TI / 2 + 4 (e = 2 s); step n = s + 2 uses set n & 1.  A step is FAST when every row it touches - written
    // out (e - 10, e - 9), loaded (e + 2, e + 3), updated (e, e - 2, e - 5, e - 7, all inside their colour's row range) - and
    // every row the NEXT step updates exists.
    const int s_end = TI / 2 + 4;
    // lower bounds: write-out row e - 10 >= 0 and inside the grid (the updated rows e - 7 .. e follow); upper bounds: loaded
    // row e + 3 <= TI + 1 and inside the grid, the next step's updated row e + 2 <= TI
    const int e_lo = max(10, 10 - p0);
    const int e_hi = min(TI - 2, ni - 4 - p0);
    auto pair_fast = [&](const int s) { return 2 * s >= e_lo && 2 * (s + 1) <= e_hi; };
    auto run = [&](auto mask_tag) {
        int s = -2;
        for (int part = 0; part < 2; ++part) {
            while (s <= s_end && (part == 1 || !pair_fast(s))) {
                step(std::false_type{}, std::integral_constant<int, 0>{}, mask_tag, 2 * s);
                if (s + 1 <= s_end) step(std::false_type{}, std::integral_constant<int, 1>{}, mask_tag, 2 * (s + 1));
                s += 2;
            }
            if (part == 0 && s <= s_end) {
                __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): nothing requested by the predicated steps is still in flight
                while (pair_fast(s)) {
                    step(std::true_type{}, std::integral_constant<int, 0>{}, mask_tag, 2 * s);
                    step(std::true_type{}, std::integral_constant<int, 1>{}, mask_tag, 2 * (s + 1));
                    s += 2;
                }
            }
        }
    };
    // A sweep from zero in the forward colour order meets non-zero neighbours only where an earlier colour of the same sweep
    // has been: colour 0 none (x = D^-1 b), colour 1 its left / right neighbours (blocks 3, 5), colour 2 the rows above and
    // below (blocks 0-2, 6-8), colour 3 all eight.  The colour waves then request only the words of those blocks: 0 / 10 /
    // 28 / 36 of the 36 off-diagonal words - the mirror image of k_resrestrict_u.  Skipping a block drops products with
    // exact zeros: the result is the same, bit for bit.  (The wave of the halo points keeps all blocks: its lanes differ.)
    if (skip0 && po == 0 && wave == 0) {
        run(std::integral_constant<unsigned, SWST_NO_UPDATE>{});
    } else if (!x_in && po == 0 && wave < 4) {
        if (wave == 0) run(std::integral_constant<unsigned, 0x000u>{});
        else if (wave == 1) run(std::integral_constant<unsigned, 0x028u>{});
        else if (wave == 2) run(std::integral_constant<unsigned, 0x1C7u>{});
        else run(std::integral_constant<unsigned, 0x1EFu>{});
    } else {
        run(std::integral_constant<unsigned, 0x1EFu>{});
    }
}

// ==========================================================================================
// k_sweep_st2: TWO sweeps of a stored level in one march down the band - a sweep in reverse colour order (3,2,1,0) followed by a
// forward sweep that leaves colour 0 alone (k_sweep_st's skip0) - for the revisits of a W-cycle, where the post-smoothing of
// one visit and the pre-smoothing of the next run back to back with the same b.  x_mid receives the result of the reverse
// sweep (the x_old of k_resrestrict_u), x_out the final one.  Same point update, same order per point, same bits as the two
// k_sweep_st launches; the x rows are read once and the stencil words of a row are requested a second time 9 - 11 rows after
// their first use, while they are still on the die.
//  * Rows are counted in the frame of the reverse sweep: relative row 0 is the row ABOVE the forward band of TI rows, and
//    the reverse sweep covers TI + 4 rows, so that its result is final on every row the forward sweep reads (relative rows
//    0 .. TI + 2).  Seven stage waves: 0-3 the reverse sweep's colours on rows e, e-2, e-5, e-7 as in k_sweep_st; 4-6 the
//    forward colours 1, 2, 3 on rows e-11, e-14, e-16.  Row e-9 of the reverse sweep is final after step e-2 and written
//    to x_mid at the start of step e, so the first forward stage may touch it from step e+2 on; the later forward stages
//    trail by the three / two rows the colour order asks for.  Rows e-20, e-19 leave the ring (22 rows) for x_out.
//  * Columns: the forward sweep reads the reverse sweep's result two columns to the left and three to the right of the
//    owned 128, so the reverse sweep owns those five columns too and its own halo triangle moves out by as much: 8 halo
//    columns each side, and an eighth wave that updates the 21 halo points of a step (18 reverse, 3 forward).
//  * Every stage wave keeps its two sets of off-diagonal words and requests b with the diagonal block, as in k_sweep_st.
// ==========================================================================================
template <typename CT, typename VT>
__global__ __launch_bounds__(GeoR::THREADS, SweepStBudget<CT>::kMinWaves) void k_sweep_st2(const typename CoefFmt<CT>::word_t* __restrict__ C, int ni, int nj, int TI,
                                                               int nx, int ny, int nz, const VT* __restrict__ x_in,
                                                               VT* __restrict__ x_mid, VT* __restrict__ x_out,
                                                               const VT* __restrict__ b, const ActiveSet act) {
    typedef GeoR G;
    typedef typename CoefFmt<CT>::word_t word_t;
    constexpr int W = G::W, OUT = G::OUT, HALO = G::HALO, RING = G::RING, PLANES = CoefFmt<CT>::PLANES;
    extern __shared__ double sw_lds[];
    VT* xs = reinterpret_cast<VT*>(sw_lds);                                                     // [RING][3][W]
    int bx, by, pair;
    if (!sw_strip(act, nx, ny, nz, bx, by, pair)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = TI + 4;                 // rows of the reverse sweep
    const int p0 = by * TI - 1;           // true row of relative row 0
    const int qs = bx * OUT - HALO;
    const size_t npts = (size_t)ni * nj, off = (size_t)pair * 3 * npts;
    const VT* xin = x_in + off;
    VT* xmid = x_mid + off;
    VT* xout = x_out + off;
    const VT* bp = b + off;
    const CLay L(ni, nj);
    const word_t* Cp = C + (size_t)pair * PLANES * L.plane;

    // ---- stage of this lane.  Waves 0-6: stage = wave; wave 7 updates the halo points.  Stages 0-3 have the column parities
    // of a sweep with po = 1, stages 4-6 those of the colours 1-3 of a sweep with po = 0: (stage & 1) ^ 1 in both cases.
    int stage = wave, lc;
    bool lane_on = true;
    lc = HALO + 2 * lane + ((wave & 1) ^ 1);
    if (wave == 7) {
        constexpr int NH = 21;
        const int hs[NH] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
        const int hl[NH] = {3, 5, 7, HALO + OUT + 1, HALO + OUT + 3, HALO + OUT + 5, 4, 6, HALO + OUT, HALO + OUT + 2, HALO + OUT + 4,
                            5, 7, HALO + OUT + 1, HALO + OUT + 3, 6, HALO + OUT, HALO + OUT + 2, 7, HALO + OUT + 1, HALO + OUT};
        lane_on = lane < NH;
        stage = hs[lane_on ? lane : 0];
        lc = hl[lane_on ? lane : 0];
    }
    const int q = qs + lc;
    const bool col_ok = lane_on && (q >= 0) && (q < nj);
    const int qc = col_ok ? q : 0, lcc = col_ok ? lc : 2;
    const int cC = sw_cs<G>(lcc), uL = sw_cs<G>(lcc - 1), uR = sw_cs<G>(lcc + 1);
    const unsigned ccq = (unsigned)((size_t)(qc & 1) * L.sub + (size_t)(qc >> 1));   // column part of the stencil index
    const unsigned bcol = (unsigned)qc;
    // cooperative load-in / write-out of 2 rows x 3 fields x W columns per step; recomputed where used, see k_sweep_st
    auto opaque_tid = [&]() { int t = tid; asm volatile("" : "+v"(t)); return t; };
    struct XMap { int row, col, q, lds; unsigned g; bool on, ld, st; };
    auto xmap = [&](const int t) {
        XMap m;
        m.row = t >= W ? 1 : 0; m.col = t - m.row * W;
        m.on = t < 2 * W;
        m.q = qs + m.col;
        m.ld = m.on && m.q >= 0 && m.q < nj;
        m.st = m.ld && m.col >= HALO && m.col < HALO + OUT;
        m.g = m.ld ? (unsigned)m.q : 0u;
        m.lds = sw_cs<G>(m.on ? m.col : 0);
        return m;
    };
    auto wrap = [](int t) { return t >= RING ? t - RING : t; };   // t in [0, 2 RING)
    const int sro = (stage == 0) ? 0 : (stage == 1) ? -2 : (stage == 2) ? -5 : (stage == 3) ? -7 : (stage == 4) ? -11 : (stage == 5) ? -14 : -16;
    const int rr_lo = (stage < 2) ? 0 : (stage < 5) ? 1 : 2;
    const int rr_hi = (stage < 2) ? H : (stage < 4) ? H - 1 : (stage == 4) ? TI + 1 : TI;
    const bool uni = wave < 7;                           // stage waves: the stage's row is wave-uniform

    constexpr int ND = CoefFmt<CT>::ND;
    constexpr bool F8 = std::is_same<CT, CoefF8>::value;
    static_assert(CoefPacked<CT>::value, "k_sweep_st2 is written for the packed stencil formats");
    word_t cw[2][ND], dg[PLANES - ND];
    VT bq[3];                                            // b of the stage's point: requested with the diagonal block
#pragma unroll
    for (int k = 0; k < ND; ++k) cw[0][k] = cw[1][k] = 0;
#pragma unroll
    for (int k = 0; k < PLANES - ND; ++k) dg[k] = 0;
    bq[0] = bq[1] = bq[2] = (VT)0;
    auto offd = [](const word_t* w, int j) {   // off-diagonal coefficient j (0..71) of a set (CoefF8: in the units of its row)
        if constexpr (F8) {
            return (double)f8_decode(w[j >> 2], j & 3);
        } else {
            const uint32_t v = w[j >> 1];
            return (double)__uint_as_float((j & 1) ? (v & 0xFFFF0000u) : (v << 16));
        }
    };
    auto point_base = [&](const int pn, const word_t*& base, unsigned& idx, const bool fast) {
        if (fast && uni) {
            const int pnu = __builtin_amdgcn_readfirstlane(pn);
            base = Cp + (size_t)((pnu & 1) << 1) * L.sub + (size_t)(pnu >> 1) * L.hj;
            idx = ccq;
        } else {
            base = Cp;
            idx = (unsigned)((size_t)((pn & 1) << 1) * L.sub + (size_t)(pn >> 1) * L.hj) + ccq;
        }
    };
    auto fetch_point = [&](auto fast_tag, auto jtag, const int eN) {
        constexpr bool FAST = decltype(fast_tag)::value;
        constexpr int J = decltype(jtag)::value;
        const int rrn = eN + sro, pn = p0 + rrn;
        if (FAST || (col_ok && rrn >= rr_lo && rrn <= rr_hi && pn >= 0 && pn < ni)) {
            const word_t* base; unsigned idx;
            point_base(pn, base, idx, FAST);
#pragma unroll
            for (int k = 0; k < ND; ++k) cw[J][k] = (base + (size_t)k * L.plane)[idx];
        }
    };
    auto fetch_diag = [&](auto fast_tag, const int eN) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const int rrn = eN + sro, pn = p0 + rrn;
        if (FAST || (col_ok && rrn >= rr_lo && rrn <= rr_hi && pn >= 0 && pn < ni)) {
            const word_t* base; unsigned idx;
            point_base(pn, base, idx, FAST);
#pragma unroll
            for (int k = 0; k < PLANES - ND; ++k) dg[k] = (base + (size_t)(ND + k) * L.plane)[idx];
            const VT* brow = bp + (size_t)pn * nj + bcol;
            bq[0] = brow[0]; bq[1] = brow[npts]; bq[2] = brow[2 * npts];
        }
    };

    int slotA = (2 * RING - 2) % RING;   // ring slot of relative row e + 2 (even), advanced by 2 per step
    auto step = [&](auto fast_tag, auto jtag, const int e) {
        constexpr bool FAST = decltype(fast_tag)::value;
        constexpr int JC = decltype(jtag)::value;
        const bool do_load = FAST ? true : (e + 2 <= H + 1);
        const XMap m1 = xmap(opaque_tid());
        // (1) write-out: rows e - 10, e - 9 of the reverse sweep's result, rows e - 20, e - 19 of the final one (the slots the rows
        // loaded in this step take over).  Both only for the TI rows of the forward band, relative rows 1 .. TI.
        {
            const int rr = e - 10 + m1.row, p = p0 + rr;
            if (m1.st && (FAST || (rr >= 1 && rr <= TI && p >= 0 && p < ni))) {
                VT* orow = xmid + (size_t)p * nj + m1.g;
                const VT* lrow = xs + (wrap(slotA + RING - 12) + m1.row) * 3 * W + m1.lds;
                orow[0] = lrow[0]; orow[npts] = lrow[W]; orow[2 * npts] = lrow[2 * W];
            }
        }
        {
            const int rr = e - 20 + m1.row, p = p0 + rr;
            if (m1.st && (FAST || (rr >= 1 && rr <= TI && p >= 0 && p < ni))) {
                VT* orow = xout + (size_t)p * nj + m1.g;
                const VT* lrow = xs + (slotA + m1.row) * 3 * W + m1.lds;
                orow[0] = lrow[0]; orow[npts] = lrow[W]; orow[2 * npts] = lrow[2 * W];
            }
        }
        // (2) rows e + 2, e + 3 -> registers (moved into the ring in (5)), then the next step's point
        VT lx[3] = {(VT)0, (VT)0, (VT)0};
        {
            const int pR = p0 + e + 2 + m1.row;
            if (FAST) {   // (columns outside the grid: a clamped address, see k_sweep_st)
                const VT* irow = xin + (size_t)pR * nj + m1.g;
                lx[0] = irow[0]; lx[1] = irow[npts]; lx[2] = irow[2 * npts];
            } else if (m1.ld && do_load && pR >= 0 && pR < ni) {
                const VT* irow = xin + (size_t)pR * nj + m1.g;
                lx[0] = irow[0]; lx[1] = irow[npts]; lx[2] = irow[2 * npts];
            }
        }
        fetch_point(fast_tag, std::integral_constant<int, 1 - JC>{}, e + 2);
        // (4) the stage of this lane: block Gauss-Seidel update of its point, neighbours read row by row (as in k_sweep_st)
        {
            const int rr = e + sro, p = p0 + rr;
            if (col_ok && (FAST || (rr >= rr_lo && rr <= rr_hi && p >= 0 && p < ni))) {
                // rows rr - 1, rr, rr + 1 are (e + 2) + (sro - 3), (sro - 2), (sro - 1); sro - 3 >= -19 > -RING
                const int sU = wrap(slotA + RING + sro - 3), sC = wrap(slotA + RING + sro - 2), sD = wrap(slotA + RING + sro - 1);
                const int rowo[3] = {sU * 3 * W, sC * 3 * W, sD * 3 * W};
                const int colo[3] = {uL, cC, uR};
                const word_t* c_ = cw[JC];
                double y0 = 0, y1 = 0, y2 = 0;
                typedef double AT;
                AT yp[F8 ? 9 : 1];
                if constexpr (F8) {
#pragma unroll
                    for (int t = 0; t < 9; ++t) yp[t] = 0;
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const VT* row = xs + rowo[a];
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        if (a == 1 && bb == 1) continue;
                        double xu = (double)row[colo[bb]], xw = (double)row[W + colo[bb]], xg = (double)row[2 * W + colo[bb]];
                        const int d = a * 3 + bb, t0 = (d < 4 ? d : d - 1) * 9;
                        if constexpr (F8) {
                            const AT au = (AT)row[colo[bb]], aw = (AT)row[W + colo[bb]], ag = (AT)row[2 * W + colo[bb]];
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
                                yp[3 * r + 0] += (AT)f8_decode(c_[(t0 + 3 * r + 0) >> 2], (t0 + 3 * r + 0) & 3) * au;
                                yp[3 * r + 1] += (AT)f8_decode(c_[(t0 + 3 * r + 1) >> 2], (t0 + 3 * r + 1) & 3) * aw;
                                yp[3 * r + 2] += (AT)f8_decode(c_[(t0 + 3 * r + 2) >> 2], (t0 + 3 * r + 2) & 3) * ag;
                            }
                        } else {
                            y0 += offd(c_, t0 + 0) * xu + offd(c_, t0 + 1) * xw + offd(c_, t0 + 2) * xg;
                            y1 += offd(c_, t0 + 3) * xu + offd(c_, t0 + 4) * xw + offd(c_, t0 + 5) * xg;
                            y2 += offd(c_, t0 + 6) * xu + offd(c_, t0 + 7) * xw + offd(c_, t0 + 8) * xg;
                        }
                    }
                    asm volatile("" ::: "memory");   // keep the LDS reads of the next row behind this row's arithmetic
                }
                double Dm[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) Dm[t] = (double)__uint_as_float(dg[t]);
                if constexpr (F8) {
                    y0 = (double)yp[0] * (double)f8_unit(dg[9], 0) + (double)yp[1] * (double)f8_unit(dg[9], 1) + (double)yp[2] * (double)f8_unit(dg[9], 2);
                    y1 = (double)yp[3] * (double)f8_unit(dg[10], 0) + (double)yp[4] * (double)f8_unit(dg[10], 1) + (double)yp[5] * (double)f8_unit(dg[10], 2);
                    y2 = (double)yp[6] * (double)f8_unit(dg[11], 0) + (double)yp[7] * (double)f8_unit(dg[11], 1) + (double)yp[8] * (double)f8_unit(dg[11], 2);
                }
                double u, w, gm;
                solve3(Dm, (double)bq[0] - y0, (double)bq[1] - y1, (double)bq[2] - y2, u, w, gm);
                VT* row = xs + rowo[1] + cC;
                row[0] = (VT)u; row[W] = (VT)w; row[2 * W] = (VT)gm;
            }
        }
        fetch_diag(fast_tag, e + 2);   // the diagonal block and b of the next step's point (the registers are free now)
        // (5) loaded rows -> LDS ring (the slots freed by the second write-out, same thread <-> element mapping)
        const XMap m5 = xmap(opaque_tid());
        if (do_load && m5.on) {
            VT* lrow = xs + (slotA + m5.row) * 3 * W + m5.lds;
            lrow[0] = lx[0]; lrow[W] = lx[1]; lrow[2 * W] = lx[2];
        }
        slotA = wrap(slotA + 2);
        __syncthreads();
    };

    // Steps s = -2 .. TI / 2 + 10 (e = 2 s); step n = s + 2 uses set n & 1.  A step is FAST when every row it touches - written out
    // (e - 20 .. e - 9, inside 1 .. TI), loaded (e + 2, e + 3), updated (e .. e - 16, inside their stage's range) - and every row the
    // NEXT step updates exists.
    const int s_end = TI / 2 + 10;
    const int e_lo = max(22, 20 - p0);                 // row e - 20 >= 2 and inside the grid
    const int e_hi = min(TI + 2, ni - 4 - p0);         // loaded row e + 3 <= H + 1 and inside the grid, next step's row e + 2 <= H
    auto pair_fast = [&](const int s) { return 2 * s >= e_lo && 2 * (s + 1) <= e_hi; };
    int s = -2;
    for (int part = 0; part < 2; ++part) {
        while (s <= s_end && (part == 1 || !pair_fast(s))) {
            step(std::false_type{}, std::integral_constant<int, 0>{}, 2 * s);
            if (s + 1 <= s_end) step(std::false_type{}, std::integral_constant<int, 1>{}, 2 * (s + 1));
            s += 2;
        }
        if (part == 0 && s <= s_end) {
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): nothing requested by the predicated steps is still in flight
            while (pair_fast(s)) {
                step(std::true_type{}, std::integral_constant<int, 0>{}, 2 * s);
                step(std::true_type{}, std::integral_constant<int, 1>{}, 2 * (s + 1));
                s += 2;
            }
        }
    }
}

}  // namespace vof
