// vof_shared.hpp - what the three sources of libvof.so share on the device side: launch constants, the types a kernel argument or
// the context names, and __device__ __forceinline__ helpers.  No __global__ function lives here: every
// source includes this header, and a kernel belongs to exactly one code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vof {

constexpr int BX = 64;  // lanes along j
constexpr int BY = 4;   // rows per block
constexpr int NT = BX * BY;

struct PairScalars {
    double rho, alpha, omega, beta;
    double bnorm2, rnorm2;
    double tol2;      // rtol^2 * bnorm2
    int iterations;
    int converged;
    int breakdown;
    int halfstep;     // 1: converged at the half step, x += alpha y still pending; 2: done
};

// Per-pair overrides for "virtual pairs" (vary_regularisation batches several (speed_alpha, remodelling_alpha)
// combinations of the same movie into one launch): regularisation parameters and the index of the pair's first frame.
// Kernels take a `const PairParam* pp`; nullptr (the normal case) = kernel arguments / frame index = pair index.
struct PairParam {
    double alpha, beta;
    int frame;   // index of the pair's first frame in the movie
    int out;     // index of the pair's slot in the output stacks
};

// The pairs a launch serves.  flags[pair] != 0: the pair is still being solved (nullptr: every pair is).  list: the slots of the
// pairs that were active when the host last counted them, ascending; the grid dimension that runs over the pairs then holds one
// entry per listed pair instead of one per slot of the batch (nullptr: one per slot).  A block takes its pair from the list and
// still checks the flag: pairs are switched off on the device between two counts (k_scalar), and those blocks leave as before.
struct ActiveSet {
    const int* flags;
    const int* list;
    __device__ __forceinline__ int pair(int slot) const { return list ? list[slot] : slot; }
    __device__ __forceinline__ bool on(int pair) const { return !flags || flags[pair]; }
};

// ---- reductions: threads of a reduction block and the sum over a wave (the kernels and block_store_partials: vof_device.hpp)
constexpr int RBLK = 256;  // threads per reduction block

// The shuffle takes HIP's default width (the wave, 64 lanes here), not a literal 64: where every call of a code object passes the
// same literal the compiler builds it into __shfl_down before inlining and the lane arithmetic of every reduction comes out
// differently, so the code of a kernel would depend on which other kernels share its source (profiles/split_build_summary.md).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// ---- restarted GMRES: the per-pair state the context holds (the kernels: vof_device.hpp)
constexpr int GM_MAXM = 128;   // largest restart length
constexpr int GM_NV = 8;       // basis vectors per multi-dot / multi-axpy launch

struct GmresState {
    double R[GM_MAXM * GM_MAXM];   // rotated Hessenberg matrix, column j at R + j * GM_MAXM (upper triangular)
    double cs[GM_MAXM], sn[GM_MAXM];
    double g[GM_MAXM + 1];         // rotated right-hand side; |g[k]| = residual norm after k steps
    double y[GM_MAXM];             // solution of the k x k triangular system
    double h[GM_MAXM + 2];         // current Hessenberg column (before the rotations)
    double c[GM_MAXM + 2];         // coefficients of the current Gram-Schmidt pass
    double scale;                  // 1 / norm of the vector to normalise next
    int k;                         // columns built in this cycle
    int est_converged;             // the cycle ended because the residual estimate met the tolerance
};

// ---- k_tail_cycle: the arguments the context keeps (the kernel: vof_device.hpp)
constexpr int TAIL_THREADS = 256;
constexpr int TAIL_MAX_LEVELS = 8;
constexpr int TAIL_MAX_OPS = 160;
constexpr int TAIL_MAX_PTS = 1024;    // points of the largest tail level
constexpr int TAIL_MAX_SUB = 256;     // points per colour class of the largest tail level (= threads)
enum TailOpCode { T_SMOOTH = 0, T_RESTRICT = 1, T_COARSE = 2, T_PROLONG = 3 };

struct TailLevel {
    int ni, nj;
    int hj;                      // (nj + 1) / 2: row length of a colour sub-plane
    int sub;                     // elements of a colour sub-plane ((ni + 1) / 2 * hj)
    unsigned long long plane;    // CLay(ni, nj).plane
    const void* C;               // stencil [pair][81][plane]; nullptr on the dense coarsest level
    int xo, bo;                  // LDS offsets (in doubles) of x (3 x (ni + 2) x (nj + 2), zero halo) and b (3 x ni x nj)
};
struct TailArgs {
    int nl;                      // tail levels; level nl - 1 is the coarsest (dense inverse)
    int n_ops;
    int ro;                      // LDS offset of the residual scratch (3 x points of tail level 0)
    int nd;                      // unknowns of the coarsest level
    const double* invT;          // [pair][nd][nd] transposed inverse
    TailLevel L[TAIL_MAX_LEVELS];
    // op_arg of T_SMOOTH: bit 0 = start from zero, bit 1 = reverse colour order, bits 2.. = number of sweeps
    unsigned char op[TAIL_MAX_OPS], op_level[TAIL_MAX_OPS], op_arg[TAIL_MAX_OPS];
};

// ---- histograms of the summary kernels (vof_boxsweep.hpp, vof_blursweep.hpp, vof_compare.hpp, vof_flowcompare.hpp, vof_intensity.hpp)
constexpr int BS_LDS_BINS = 1024;    // histograms up to this many bins are counted per block in LDS first

// np.histogram(x, bins, range)[0] for equal bins: scaled index, corrected against the two neighbouring edges (the bins+1
// values of np.linspace, passed in); last bin closed on the right; values outside [first, last] and NaN dropped.
__device__ __forceinline__ int bs_bin_of(double x, const double* __restrict__ edges, int bins) {
#pragma clang fp contract(off)
    const double first = edges[0], last = edges[bins];
    if (!(x >= first && x <= last)) return -1;
    int idx = (int)(((x - first) / (last - first)) * (double)bins);
    if (idx == bins) --idx;
    if (x < edges[idx]) --idx;
    if (x >= edges[idx + 1] && idx != bins - 1) ++idx;
    return idx;
}

// limits of k_cp_joint (vof_compare.hpp) that k_fc_histograms (vof_flowcompare.hpp) shares
constexpr int CP_MAX_THETA_BINS = 64;
constexpr int CP_MAX_SPEED_BINS = 1024;   // per axis of the 2-D histogram
constexpr int CP_LDS_JOINT = 4096;        // ba * bb up to this are counted per block in LDS first

// ---- tile geometry of k_blur1d_tiled (vof_blursweep.hpp), shared by the tiled passes of vof_intensity.hpp
constexpr int BL_TI = 32;      // AXIS 0: output rows of a tile (8 per thread)
constexpr int BL_TR = 16;      // AXIS 1: rows of a tile (4 per thread)
constexpr int BL_RMAX = 64;    // (BL_TI + 2 * 64) * BX * 8 B = 81920 B
constexpr int BL_RMIN = 1;     // radius 0 is a copy scaled by w[0]: nothing to share

inline size_t blur_tiled_lds(int axis, int radius) {
    return (axis == 0 ? (size_t)(BL_TI + 2 * radius) * BX : (size_t)BL_TR * (BX + 2 * radius)) * sizeof(double);
}

}  // namespace vof
