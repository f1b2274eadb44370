/* vof.h - C ABI of the MI355X-native variational optical-flow solver (libvof.so).
 *
 * The reference has no FFI layer: its boundary is the Python function
 *   source/optical_flow.py:715-724  variational_optical_flow(movie, delta_x, delta_t, speed_alpha,
 *                                    remodelling_alpha, smoothing_sigma, initial_v_x, initial_v_y,
 *                                    initial_remodelling, use_direct_solver)
 * The entry points below are what a binding for that function calls (see INTEGRATION.md for the
 * ctypes stub); each one names the reference lines it replaces.  Plain pointers and sizes only,
 * no exceptions cross the ABI, no global state (contrast PETSc.Options(), OF.py:1081-1092).
 *
 * Conventions: images are row-major (N_i, N_j) float64, axis 0 = "x" = i, axis 1 = "y" = j
 * (OF.py:730-733).  Pair k is (frame k, frame k+1) (OF.py:794-795).  Return value 0 = success,
 * negative = error (message via vof_last_error).  Non-convergence is NOT an error: it is reported
 * per pair in vof_pair_stats, like the reference which only prints a warning (OF.py:1135-1138).
 */
#ifndef VOF_H
#define VOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOF_VERSION 202 /* 0.2.2: vof_pair_stats carries the batch time (0.2.1: vof_params carries its own size and the ABI version) */

typedef struct vof_ctx vof_ctx;

/* Solver parameters.  Defaults (vof_default_params) reproduce the reference's settings.
 * ABI guard: the first two fields are filled in by vof_default_params and checked by every entry point that takes a
 * vof_params (a binding compiled against another layout is rejected with an error instead of being read past its end). */
typedef struct vof_params {
    uint32_t struct_size;      /* sizeof(vof_params) of the header the caller was built with */
    uint32_t abi_version;      /* VOF_VERSION of that header */
    double speed_alpha;        /* OF.py:718  */
    double remodelling_alpha;  /* OF.py:719  */
    double delta_x;            /* OF.py:716; velocities are returned in delta_x/delta_t units (OF.py:1189-1190) */
    double delta_t;            /* OF.py:717  */
    double initial_v_x;        /* OF.py:721,800: initial guess in delta_x/delta_t units */
    double initial_v_y;        /* OF.py:722,801 */
    double initial_remodelling;/* OF.py:723,802 */
    double rtol;               /* OF.py:1120: 1e-6, ||b - A x||_2 <= rtol ||b||_2 (unpreconditioned, OF.py:1126) */
    int32_t max_iterations;    /* OF.py:1120: 1000 BiCGStab iterations */
    int32_t nu_pre;            /* block-GS sweeps before the coarse-grid correction on level 0 (default 2) */
    int32_t nu_post;           /* ... and after (default 2) */
    int32_t reference_quirks;  /* 1 (default): OF.py:698-699 'dy' == 'dx'; OF.py:1205 speed_functional bug */
    int32_t coarse_precision;  /* storage of the Galerkin stencils (preconditioner only): 3 (default) 8-bit float off-diagonal
                                  blocks (units of a power of two per block position) + float32 diagonal block that absorbs their
                                  rounding errors (block row sums kept; 120 bytes per coarse point, +1 % iterations); 2: the same
                                  with bfloat16 off-diagonal blocks (180 bytes, iteration counts of float32); 1: float32 (324
                                  bytes); 0: float64 */
    int32_t vcycle_precision;  /* storage of the V-cycle vectors: 0 float64; 1 float32; 2 auto = float32 for the first 8
                                  iterations, float64 afterwards; 3 (default) = float64 on level 0, float32 on the levels below
                                  for the first 8 iterations - and there also float32 for the vectors that only pass between
                                  level-0 passes (the pre-smoothed iterate, the cycle's result) where the register-resident
                                  passes run the whole level-0 part of the cycle.  Krylov vectors, operator products, residuals and the stopping rule are
                                  always FP64; so is the arithmetic of every cycle kernel, except the level-0 smoother of the
                                  float32-vector modes 1 / 2 (k_sweep0p: packed float32 - part of the preconditioner only) */
    int32_t nu_pre_coarse;     /* sweeps on the levels >= 1 (default 1); 0 = same as nu_pre / nu_post */
    int32_t nu_post_coarse;
    int32_t w_cycle_level;     /* l >= 0 (default 1): level l visits level l+1 w_cycle_visits times per cycle (a one-level W-cycle); -1: V-cycle */
    int32_t w_cycle_visits;    /* visits of level w_cycle_level + 1 per cycle (default 3); 0 = 2 */
    int32_t krylov_method;     /* 0: BiCGStab only (the reference's KSP type 'bcgs', OF.py:1081); 1: restarted GMRES only;
                                  2 (default): BiCGStab, then GMRES(gmres_restart) for the pairs that have not met the
                                  stopping rule after fallback_after iterations or broke down.  Same preconditioner,
                                  same stopping rule; `iterations` counts the Krylov steps of both phases */
    int32_t gmres_restart;     /* restart length (default 100, at most 128); the basis takes (restart + 1) float64 vectors per pair in
                                  flight and is capped at half of the free device memory when the fallback first runs */
    int32_t fallback_after;    /* BiCGStab iterations before the fallback (default 25) */
    int32_t warm_start_stride; /* vof_solve_stack_dev / _host (per batch), stacks whose first phase is >= 16 Mpixel of pairs: every stride-th pair is solved first from the
                                  constant initial fields, the others start from the solution of their nearest solved neighbour
                                  (the reference warm-starts pair k from pair k-1, OF.py:803-806).  Default 3; 0 or 1: every pair
                                  starts from the constant initial fields.  Same stopping rule either way */
    int32_t preconditioner;    /* 0: multigrid cycle only; 1: direct - block-tridiagonal LU of the level-0 operator by image rows
                                  (dense 3 n_j x 3 n_j Schur blocks inverted in-house; n_i (3 n_j)^2 doubles per pair in flight), the
                                  reference's SuperLU branch (OF.py:1146-1147) as the preconditioner of the same Krylov iteration;
                                  2 (default): the multigrid cycle (at most 150 Krylov steps where the direct re-solve takes
                                  seconds: images up to ~530 pixels wide), and the pairs it leaves unconverged once more with the
                                  direct preconditioner when its buffers fit into the free device memory */
    int32_t reserved0;         /* keeps the size a multiple of 8; must be 0 */
} vof_params;

/* Per-pair solver report (the reference prints these: OF.py:1131-1154). */
typedef struct vof_pair_stats {
    int32_t iterations;        /* BiCGStab iterations used */
    int32_t converged;         /* 1 iff the INDEPENDENT residual below meets the stopping rule, ||b - A x||^2 <= rtol^2 ||b||^2
                                  (OF.py:1135 solver.is_converged, OF.py:1120,1126), evaluated on the residual recomputed
                                  from x after the solve - never on the solver's recursively updated residual */
    double relative_residual;  /* independent ||A x - b|| / ||b|| after the solve (OF.py:1151) */
    double L1_functional;      /* OF.py:1178-1180 */
    double speed_functional;   /* OF.py:1181-1182 (the true one; the dict-level bug is applied by the caller) */
    double remodelling_functional; /* OF.py:1183 */
    double batch_ms;           /* GPU time (HIP events on the stream of the lane that solved it, see VOF_LANES) of the batch this
                                  pair was solved in: hierarchy set-up + Krylov iteration + epilogue of batch_pairs pairs advancing
                                  together, i.e. this pair's share is batch_ms / batch_pairs (the reference prints per-pair wall
                                  times, OF.py:1073-1076, 1156-1157); a pair re-solved by a fallback carries the sum of its shares.
                                  The batches of concurrent lanes overlap in time: their shares add up to more than the wall time */
    int32_t batch_pairs;       /* pairs in that batch (a per-lane batch when the solve ran in lanes) */
    int32_t reserved;          /* 0 */
} vof_pair_stats;

/* Kernel classes for the built-in HIP-event profiler (vof_profile_*). */
enum vof_kernel_id {
    VOF_K_RHS = 0, VOF_K_APPLY0, VOF_K_GS0, VOF_K_GS, VOF_K_RESIDUAL, VOF_K_RESTRICT, VOF_K_PROLONG,
    VOF_K_GALERKIN0, VOF_K_GALERKIN, VOF_K_COARSE_SETUP, VOF_K_COARSE_SOLVE, VOF_K_VECTOR, VOF_K_REDUCE,
    VOF_K_FINALIZE, VOF_K_FUNCTIONALS, VOF_K_COARSE_TAIL, VOF_K_PREPROCESS, VOF_K_COUNT
};

int vof_version(void);
/* sizeof(vof_params) of the library (a binding asserts that its own struct has this size). */
size_t vof_params_size(void);
/* Fills *p with the defaults.  struct_size = sizeof(vof_params) as the CALLER declares it: if it differs from the
 * library's, nothing is written and -1 is returned (a stale binding can neither be overrun nor half-initialised). */
int vof_default_params(vof_params* p, size_t struct_size);

/* Environment variables read once by vof_create (A/B experiment switches; results are identical, only speed changes):
 *   VOF_SWEEP0R_MIN_BLOCKS=n   level 0, float64 vectors: the register-resident pass k_sweep0r from n one-wave blocks per launch on
 *                              (default 512; smaller launches use the LDS-ring pass k_sweep0m)
 *   VOF_L0_HANDOFF=0           vcycle_precision 3: the level-0 hand-off vectors of the cycle stay float64 (default: float32 where
 *                              the first 8 iterations run their level-0 passes in k_sweep0r)
 *   VOF_FUSE_B=0               the BiCGStab updates s = r - alpha v and p = r + beta (p - omega v) by their stand-alone kernels instead
 *                              of inside the first pre-smoothing pass of the cycle that consumes them (same bits)
 *   VOF_FUSE_RR=0              level 0: the coarse right-hand side R (b - A x) by the stand-alone residual + restriction kernel instead
 *                              of as the trailing stage of the pre-smoothing pass
 *   VOF_ACTIVE_LIST=0          every launch of a Krylov round covers all pair slots of the batch, and the blocks of finished pairs
 *                              read their flag and leave (default: after each count of the active pairs the launches take the
 *                              list of their slots and cover those alone; same bits, tests/test_gpu_active_list.py)
 *   VOF_FUSE_REVISIT=0         W-cycle: between two visits of the revisited stored level, the post-smoothing sweep of one visit and the
 *                              pre-smoothing sweep of the next as two launches (default: one pass over the level, k_sweep_st2; same bits,
 *                              tests/test_gpu_revisit_fusion.py)
 *   VOF_GALERKIN_FAST=n        batch set-up, level-0 Galerkin product (k_galerkin); a bit mask, default 1.  0: one generic kernel (existence
 *                              tests, ghost folds and weights at run time) for every coarse point.  bit 0: the coarse points away
 *                              from the border by a kernel of their own (compile-time weights, raw blocks: the arithmetic these
 *                              points had before) and the border frame by the generic kernel on a compact grid.  bit 1 (with
 *                              bit 0, i.e. 3): that kernel evaluates the product in closed form (the image fields times
 *                              compile-time coefficients).  Off by default: it takes a tenth off that kernel (0.4 ms of a 173 ms
 *                              step) and moves the last bits of the level-1 stencils, with which an ill-conditioned regime's
 *                              iteration counts shift by one (profiles/r20_galerkin_setup_summary.md section 5;
 *                              tests/test_gpu_galerkin_setup.py checks both settings)
 *   VOF_FOLD_STORED=1          stored levels: coarse-grid correction interpolated inside the first post-sweep
 *   VOF_TRACE=1                direct preconditioner: progress lines on stderr
 * Read at every vof_solve_stack_dev call (speed only; per pair the same arithmetic, partial sums may add in another order):
 *   VOF_LANES=1|2|3            the multigrid solve of the stack as this many concurrent pair groups ("lanes"), each on a stream
 *                              and host thread of its own with an equal share of the context's pair slots (default 3).  In
 *                              the two-phase warm start a lane runs phase 1 then phase 2 of its own groups of pairs and waits
 *                              only for the phase 1 of the group that holds the guess of its group's last pairs; the lanes
 *                              join once, before the direct re-solve, which runs on the context's stream.  One lane while
 *                              vof_profile_enable is on or with VOF_DEBUG_SYNC; vof_solve_stack_host and
 *                              vof_vary_regularisation_host always run one
 *   VOF_LANE_GROUPS=1|2        groups of pairs per lane in the two-phase warm start (default 1: equal shares, one group per
 *                              lane).  2: a lane's share is cut in two at a place that differs from lane to lane, so that the
 *                              lanes reach the under-filled last Krylov iterations of a batch at different times (measured
 *                              slower on 1024^2 x 256: every extra batch ends in such iterations of its own)
 *   VOF_LANES_MIN_MPIX=x       fewer lanes while a lane's share of a phase would be below x Mpixel of frame pairs (default 16);
 *                              one group per lane where two would leave a group with fewer phase-1 pairs than that
 * Read at every vof_box_flow_dev / _host call:
 *   VOF_BOXFLOW_FUSED=0        box flow: the general three-kernel path through device scratch planes also for box sizes up to 31
 *                              (default: the fused LDS kernel k_boxflow_fused there); same window sums in another order
 * Read at every blur (vof_blur_stack_dev / _host, and the blurs inside vof_vary_boxsize_* and vof_vary_blursize_*):
 *   VOF_BLUR_TILED=0           the blur by k_blur1d, every tap from device memory, also for radii 1 .. 64 (default: the LDS-tiled
 *                              k_blur1d_tiled there; larger radii always take k_blur1d); same bits
 * Read at every vof_liu_shen_dev / _host call:
 *   VOF_LIUSHEN_FUSE=k         Liu-Shen flow: k = 1 .. 8 Jacobi iterations per launch (default 4: the LDS kernel k_ls_fused);
 *                              1: one iteration per launch from and to device memory (k_ls_step).  Same bits for every k
 * Debug switches (fault attribution; they change timing, never results):
 *   VOF_DEBUG_SYNC=1           the context's stream is synchronised and asked for its error after every launch scope; the
 *                              first failure is reported on stderr and appended to every later error text as
 *                              "scope #n, kernel class 'name', level l, pairs, image size: error"
 *   VOF_DEBUG_SYNC_FILE=path   (with VOF_DEBUG_SYNC) the scope about to be waited for is written to this file first, so that
 *                              a process the driver aborts leaves the name of the launch that was in flight
 *   VOF_DEBUG_CANARY=1         every device buffer of the context is allocated between two 4-KiB guard regions of a known byte
 *                              pattern, checked by vof_debug_check_canaries and vof_destroy (out-of-bounds WRITES are named
 *                              by buffer and offset)
 *   VOF_DEBUG_POISON=1         every device buffer is filled with 0xFF bytes (NaN as floating point) when it is allocated: a read of
 *                              workspace nothing has written shows up as a non-finite result
 *   VOF_DEBUG_ALLOC_LOG=1      base, end, size and name of every device buffer on stderr (maps a faulting address to a buffer)
 *   VOF_FUSED_ENDS=0|1|2|3     (read once by vof_create) the two ends of a batch on the matrix-free level 0.  Bit 0: the prologue of a
 *                              batch that does not start from zero (right-hand side, initial guess, initial residual and its copy)
 *                              in one pass of k_stream_apply0; bit 1: the epilogue (independent residual norm, the four outputs, the
 *                              functionals) in one pass.  Default 3; 0: the stand-alone kernels k_rhs_norm, k_gather_guess /
 *                              k_fill, the residual pass and k_finalize_functionals.  The four outputs are the same bits for the
 *                              same solution (tested); the vectors are the same expressions in the same order (not compared
 *                              bit by bit); the block partial sums add in another order
 *   VOF_TRACE_HOST=1           vof_solve_stack_host: timeline of the host pipeline (page touching, pinning, copies, batches) on stderr */

/* One context = one device = one host thread at a time.  Owns device workspaces for images of
 * (n_i, n_j) and up to max_pairs_in_flight frame pairs solved concurrently (batch dimension).
 * stream: a hipStream_t to launch on, or NULL for a context-owned stream. */
int vof_create(vof_ctx** out, int device_id, int n_i, int n_j, int max_pairs_in_flight, void* stream);
void vof_destroy(vof_ctx* ctx);
const char* vof_last_error(const vof_ctx* ctx); /* ctx may be NULL: error of the last failed vof_create */
size_t vof_workspace_bytes(const vof_ctx* ctx);
/* Device bytes a context for (n_i, n_j, max_pairs_in_flight) allocates (without host-API staging) when it is used with the
 * default storage formats; _for: with the given vof_params.coarse_precision / vcycle_precision (the stencil storage of the
 * stored levels is sized by the format in use: 120 / 180 / 324 / 648 bytes per coarse point; a context re-allocates it,
 * never shrinking, when a call asks for a wider format than any call before). */
size_t vof_query_workspace(int n_i, int n_j, int max_pairs_in_flight);
size_t vof_query_workspace_for(int n_i, int n_j, int max_pairs_in_flight, int coarse_precision, int vcycle_precision);
/* Free / total device memory in bytes; returns 0 on success. */
int vof_device_memory(int device_id, size_t* free_bytes, size_t* total_bytes);
int vof_num_levels(const vof_ctx* ctx);

/* Replaces the frame-pair loop OF.py:791-1186 + epilogue OF.py:1189-1191 for a whole stack.
 * movie: (n_frames, n_i, n_j) float64 (already blurred if blurring is wanted, OF.py:770-773).
 * v_x, v_y, remodelling, speed: (n_frames-1, n_i, n_j) float64, caller allocated; speed may be NULL.
 * stats: n_frames-1 entries, host memory, may be NULL.
 * _host: all array pointers are host memory (copies are staged by the library).
 * _dev : all array pointers are device memory on the context's device (no PCIe traffic). */
int vof_solve_stack_host(vof_ctx* ctx, const double* movie, int n_frames, const vof_params* p,
                         double* v_x, double* v_y, double* remodelling, double* speed,
                         vof_pair_stats* stats);
int vof_solve_stack_dev(vof_ctx* ctx, const double* movie, int n_frames, const vof_params* p,
                        double* v_x, double* v_y, double* remodelling, double* speed,
                        vof_pair_stats* stats);

/* Replaces blur_movie (OF.py:282-306): per-frame Gaussian blur, scipy.ndimage.gaussian_filter semantics
 * (mode='nearest'); weights = the 2*radius+1 normalised taps in host memory (radius = int(4*sigma + 0.5) for the
 * reference's skimage call).  The context fixes the frame size; any number of frames.
 * Scratch: the blur, the general path of the box flow, the sweeps, the channel comparison and the frame-wise calls below take
 * their device scratch from one buffer of the context, allocated on first use, grown on demand to the largest request served
 * (not their sum), kept, and freed by vof_destroy; every call lays it out anew and nothing in it survives the call. */
int vof_blur_stack_dev(vof_ctx* ctx, const double* in_dev, double* out_dev, int n_frames, const double* weights, int radius);
int vof_blur_stack_host(vof_ctx* ctx, const double* in_host, double* out_host, int n_frames, const double* weights, int radius);

/* Replaces conduct_optical_flow_jit (OF.py:24-157), the reference's windowed least-squares flow (Vig et al. 2016): per pair
 * (frame k, frame k + 1) the sums of dIdx^2, dIdx dIdy, dIdy^2, dI dIdx, dI dIdy (and, with include_remodelling, of dIdx, dIdy, dI)
 * over the box_size x box_size window of every pixel (half width int(box_size / 2), clipped at the image edge) and the closed-form
 * 2 x 2 / 3 x 3 solve.  v_x, v_y, speed come in delta_x / delta_t units, net_remodelling unscaled; a singular pixel holds what
 * IEEE division gives.  reference_quirks != 0 keeps OF.py:108 (column window clamped with N_i: for N_j > N_i the columns
 * j >= N_i + h have empty windows), n = box_size^2 for clipped windows and even box sizes, and - with include_remodelling - speed
 * all zero and zeros at the pixels whose determinant is 0.0; 0: n = pixels in the window, speed filled, such pixels NaN.
 * movie: (n_frames, n_i, n_j) float64; outputs (n_frames - 1, n_i, n_j) float64, caller allocated, every element written;
 * net_remodelling may be NULL without include_remodelling (zeros are written otherwise).  Box sizes up to 31 run in one fused
 * kernel, larger ones through scratch planes (the context's scratch buffer, above).  _dev: device pointers; _host: host
 * pointers, staged by the library. */
int vof_box_flow_dev(vof_ctx* ctx, const double* movie, int n_frames, int box_size, double delta_x, double delta_t,
                     int include_remodelling, int reference_quirks,
                     double* v_x, double* v_y, double* speed, double* net_remodelling);
int vof_box_flow_host(vof_ctx* ctx, const double* movie, int n_frames, int box_size, double delta_x, double delta_t,
                      int include_remodelling, int reference_quirks,
                      double* v_x, double* v_y, double* speed, double* net_remodelling);

/* Replaces liu_shen_optical_flow_jit (OF.py:426-673), the physics-based flow of Liu and Shen without remodelling as exactly
 * max_iterations Jacobi iterations per pair (frame k, frame k + 1): every pixel is updated from the old iterate by a 9-point
 * stencil and the closed-form solve of its constant 2 x 2 block [[I Ixx - 2 I^2 - n alpha, I Ixy], [I Ixy, I Iyy - 2 I^2 - n alpha]]
 * (n = 8 / 5 / 3 in the interior / on an edge line / in a corner).  Frames and fields are mirrored over the image edge
 * (row -1 = row 1), except in the 8-neighbour sums, which take outside neighbours as zero.  Every pair starts from
 * initial_v_x * delta_t / delta_x (no warm start between pairs); v_x, v_y come back times delta_x / delta_t, speed is their
 * norm, remodelling the initial one.  A singular block stores what IEEE division gives.
 * initial_kind 0: initial_v_x, initial_v_y, initial_remodelling each point to ONE double in host memory (both variants);
 * 1: to an (n_i, n_j) plane used for every pair; 2: to an (n_frames - 1, n_i, n_j) stack.  With 1 and 2 they are device
 * arrays for _dev and host arrays for _host; initial_remodelling must not be one of the outputs of _dev.
 * movie: (n_frames, n_i, n_j) float64 (n_i, n_j >= 3); outputs (n_frames - 1, n_i, n_j) float64, caller allocated, every element
 * written (speed and remodelling hold iterates on the way).  max_iterations >= 1. */
int vof_liu_shen_dev(vof_ctx* ctx, const double* movie, int n_frames, double delta_x, double delta_t, double alpha,
                     const double* initial_v_x, const double* initial_v_y, const double* initial_remodelling, int initial_kind,
                     int max_iterations, double* v_x, double* v_y, double* speed, double* remodelling);
int vof_liu_shen_host(vof_ctx* ctx, const double* movie, int n_frames, double delta_x, double delta_t, double alpha,
                      const double* initial_v_x, const double* initial_v_y, const double* initial_remodelling, int initial_kind,
                      int max_iterations, double* v_x, double* v_y, double* speed, double* remodelling);

/* Summary of one (speed_alpha, remodelling_alpha) combination of vary_regularisation (OF.py:1978-1983). */
typedef struct vof_variation_stats {
    double speed_mean, speed_variance;             /* np.mean / np.var of result['speed'] (OF.py:1978-1979) */
    double remodelling_mean, remodelling_variance; /* ... of result['remodelling'] (OF.py:1980-1981) */
    double L1_functional, speed_functional, remodelling_functional; /* sums over the pairs; speed_functional is the true
                                                      alpha * sum |grad u|^2 (the caller applies the OF.py:1205 quirk) */
    double max_relative_residual;                  /* worst pair */
    int32_t converged_last;                        /* flag of the last pair = result['converged'] (OF.py:1202, 1982) */
    int32_t converged_all;                         /* 1 if every pair met the stopping rule */
    int32_t max_iterations_used;                   /* worst pair */
    int32_t reserved;
} vof_variation_stats;

/* Replaces vary_regularisation (OF.py:1918-1998): every (speed_alphas[i], remodelling_alphas[j]) combination is an
 * independent solve of the same movie.  The movie is uploaded (and blurred, if blur_weights != NULL; taps as for
 * vof_blur_stack_*) once, all solves and the mean / variance reductions run on the device, and only the summaries
 * cross PCIe.  base: all other parameters.  out: n_speed_alphas * n_remodelling_alphas entries, row-major [i][j]. */
int vof_vary_regularisation_host(vof_ctx* ctx, const double* movie, int n_frames, const vof_params* base,
                                 const double* speed_alphas, int n_speed_alphas,
                                 const double* remodelling_alphas, int n_remodelling_alphas,
                                 const double* blur_weights, int blur_radius, vof_variation_stats* out);

/* Summary of one box size of vary_boxsize. */
typedef struct vof_boxsize_stats {
    double speed_mean, speed_variance;             /* np.mean / np.var of the box's speed stack; NaN propagates as in numpy */
    double remodelling_mean, remodelling_variance; /* ... of net_remodelling; 0 without include_remodelling */
    int64_t nonfinite_count;                       /* NaN / Inf values in the speed stack */
    int32_t box_size;                              /* box_sizes[b], echoed */
    int32_t reserved;
} vof_boxsize_stats;

/* The box-size sweep the reference's scripts run around conduct_optical_flow (compare_rho_and_actin.py:387-419, 853-894):
 * what vof_box_flow_* computes for every box_sizes[b] (n_boxes >= 1 entries, any order, duplicates allowed, each >= 1) of the
 * same movie in one call.  The derived planes of a pair are computed once and the window grows by one ring per step from
 * half width 0 to max int(box / 2), only ever adding terms to float64 accumulators, so a box costs O(1) per pixel; the fields
 * of a box do not depend on the other boxes of the list.  The frames are blurred first if blur_weights != NULL (taps as for
 * vof_blur_stack_*).  Pairs are processed in chunks sized by the free device memory (_host: at most the context's
 * max_pairs_in_flight at a time); the scratch planes are the context's one scratch buffer (vof_blur_stack_*).
 * stats: n_boxes records, host memory, required.  Mean / variance are two-pass reductions on the device.
 * histogram_edges: NULL, or the histogram_bins + 1 edges of np.linspace(lo, hi, bins + 1) in host memory; histograms (host,
 *   n_boxes x histogram_bins int64) then receives np.histogram(speed, bins, (lo, hi))[0] of every box exactly.
 * probe_ij: NULL, or n_probes (i, j) index pairs in host memory; probe_speeds (host, n_boxes x (n_frames - 1) x n_probes)
 *   then receives speed[k][i][j].
 * v_x, v_y, speed, net_remodelling: NULL (stats only: no full-size stack exists anywhere), or (n_boxes, n_frames - 1, n_i, n_j)
 *   float64, all of v_x, v_y, speed together; net_remodelling may be NULL also then (required with include_remodelling).
 * _dev: movie and the four field stacks are device pointers; _host: host pointers, staged through the context's pinned
 * bounce buffer.  Everything else is host memory in both. */
int vof_vary_boxsize_dev(vof_ctx* ctx, const double* movie, int n_frames, const int32_t* box_sizes, int n_boxes,
                         double delta_x, double delta_t, int include_remodelling, int reference_quirks,
                         const double* blur_weights, int blur_radius,
                         const double* histogram_edges, int histogram_bins, int64_t* histograms,
                         const int32_t* probe_ij, int n_probes, double* probe_speeds, vof_boxsize_stats* stats,
                         double* v_x, double* v_y, double* speed, double* net_remodelling);
int vof_vary_boxsize_host(vof_ctx* ctx, const double* movie, int n_frames, const int32_t* box_sizes, int n_boxes,
                          double delta_x, double delta_t, int include_remodelling, int reference_quirks,
                          const double* blur_weights, int blur_radius,
                          const double* histogram_edges, int histogram_bins, int64_t* histograms,
                          const int32_t* probe_ij, int n_probes, double* probe_speeds, vof_boxsize_stats* stats,
                          double* v_x, double* v_y, double* speed, double* net_remodelling);

/* Summary of one blur size of vary_blursize. */
typedef struct vof_blursize_stats {
    double speed_mean, speed_variance;             /* np.mean / np.var of the sigma's speed stack; NaN propagates as in numpy */
    double remodelling_mean, remodelling_variance; /* ... of net_remodelling; 0 without include_remodelling */
    int64_t nonfinite_count;                       /* NaN / Inf values in the speed stack */
    int32_t sigma_index;                           /* s, the position in the list, echoed */
    int32_t reserved;
} vof_blursize_stats;

/* The blur sweep the reference's scripts run around conduct_optical_flow (compare_rho_and_actin.py:485-614, and 120-196 for the
 * intensity histogram): for each of the n_sigmas >= 1 tap vectors (blur_weights: 2 * blur_radii[s] + 1 taps as for
 * vof_blur_stack_*, concatenated in list order; any order, duplicates allowed) the movie is blurred and what vof_box_flow_*
 * computes for box_size from the blurred frames is reduced, in one call.  The movie is uploaded once; per entry all frames are
 * blurred into a scratch stack (the context's scratch buffer), the box flow runs with the kernels and the fused / general
 * choice of vof_box_flow_dev (same bits), for pairs in chunks sized as in vof_vary_boxsize_*.  The results of an entry do not
 * depend on the other entries of the list.
 * stats: n_sigmas records, host memory, required.  Mean / variance are two-pass reductions on the device.
 * histogram_edges / histogram_bins / histograms: as for vof_vary_boxsize_* (n_sigmas x histogram_bins int64).
 * angle_bins: 0, or 1 .. 128 bins of the flow direction a = acos(v_y / speed) * sign(v_x) / pi (float64, sign(0) = 0) on (-1, 1):
 *   angle_histograms (host, n_sigmas x angle_bins int64) receives np.histogram(a, angle_bins, (-1, 1))[0] and
 *   weighted_angle_histograms (host, n_sigmas x angle_bins float64) np.histogram(a, angle_bins, (-1, 1), weights=speed)[0].
 *   A sample whose speed is not finite counts in neither; NaN directions are dropped.  The weighted sums are deterministic:
 *   a fixed-shape reduction per pair, the pairs added in pair order on the host; no floating-point atomics.
 * intensity_edges: NULL, or the intensity_bins + 1 edges of np.linspace in host memory; intensity_histograms (host, n_sigmas x
 *   intensity_bins int64) then receives np.histogram of the whole blurred stack (n_frames frames) of every entry.
 * probe_ij / probe_speeds, v_x .. net_remodelling ((n_sigmas, n_frames - 1, n_i, n_j), or NULL: no full-size field stack exists
 *   anywhere), _dev / _host: as for vof_vary_boxsize_*. */
int vof_vary_blursize_dev(vof_ctx* ctx, const double* movie, int n_frames, const double* blur_weights, const int32_t* blur_radii,
                          int n_sigmas, int box_size, double delta_x, double delta_t, int include_remodelling, int reference_quirks,
                          const double* histogram_edges, int histogram_bins, int64_t* histograms,
                          int angle_bins, int64_t* angle_histograms, double* weighted_angle_histograms,
                          const double* intensity_edges, int intensity_bins, int64_t* intensity_histograms,
                          const int32_t* probe_ij, int n_probes, double* probe_speeds, vof_blursize_stats* stats,
                          double* v_x, double* v_y, double* speed, double* net_remodelling);
int vof_vary_blursize_host(vof_ctx* ctx, const double* movie, int n_frames, const double* blur_weights, const int32_t* blur_radii,
                           int n_sigmas, int box_size, double delta_x, double delta_t, int include_remodelling, int reference_quirks,
                           const double* histogram_edges, int histogram_bins, int64_t* histograms,
                           int angle_bins, int64_t* angle_histograms, double* weighted_angle_histograms,
                           const double* intensity_edges, int intensity_bins, int64_t* intensity_histograms,
                           const int32_t* probe_ij, int n_probes, double* probe_speeds, vof_blursize_stats* stats,
                           double* v_x, double* v_y, double* speed, double* net_remodelling);

/* Summary of one channel of compare_channel_flows. */
typedef struct vof_compare_stats {
    double speed_mean, speed_variance;             /* np.mean / np.var of the channel's speed stack; NaN propagates as in numpy */
    double remodelling_mean, remodelling_variance; /* ... of net_remodelling; 0 without include_remodelling */
    int64_t nonfinite_count;                       /* NaN / Inf values in the speed stack */
    int32_t channel;                               /* 0 = a, 1 = b, echoed */
    int32_t reserved;
} vof_compare_stats;

/* The comparison of two channels of one movie the reference's scripts run around conduct_optical_flow
 * (compare_rho_and_actin.py:616-767): what vof_box_flow_* computes for box_size from movie_a and from movie_b (the same
 * n_frames and image size; the kernels and the fused / general choice of vof_box_flow_dev, same bits), the per-channel
 * statistics of vof_vary_blursize_* and the joint statistics of the two velocity fields, in one call.  A channel's frames are
 * blurred first if its blur_weights != NULL (taps as for vof_blur_stack_*).  Pairs are processed in chunks sized as in
 * vof_vary_boxsize_*; per chunk the box flow runs once per channel, then one pass reads v_x, v_y and speed of both channels
 * (48 bytes per pixel and pair) and writes nothing of field size.
 * stats: 2 records (a, b), host memory, required.  Every per-channel array below has a leading axis of length 2, a first.
 * histogram_edges / histogram_bins / histograms (2 x histogram_bins int64), angle_bins (0, or 1 .. 64) / angle_histograms /
 *   weighted_angle_histograms (2 x angle_bins): as for vof_vary_blursize_*.
 * Joint, per sample of all n_frames - 1 pairs, float64, every operation explicit and in this order:
 *   dot = v_x_a * v_x_b + v_y_a * v_y_b;  w = speed_a * speed_b;  cos = dot / w;  theta = acos(cos) / pi.
 *   A sample takes part only if both speeds are finite; the others are counted in joint_counts[0].  With reference_quirks cos is
 *   not clipped, as in the script: a rounding excess over 1 gives a NaN theta; without, cos is clipped to [-1, 1] first (a NaN
 *   stays one).  Samples whose theta is NaN are in no bin and counted in joint_counts[1].
 * relative_angle_bins: 1 .. 64.  relative_angle_histogram (host, int64) receives np.histogram(theta, bins, (0, 1))[0] and
 *   weighted_relative_angle_histogram (host, float64) np.histogram(theta, bins, (0, 1), weights=w)[0]: a fixed-shape reduction
 *   per pair whose shape depends on the image size only, the pairs added in pair order on the host; no floating-point atomics,
 *   so the sums are bit-identical from call to call and for every number of pairs in flight.
 * joint_speed_edges_a / _b: both NULL, or the joint_speed_bins_a + 1 and joint_speed_bins_b + 1 edges of np.linspace in host
 *   memory (1 .. 1024 bins per axis); joint_speed_histogram (host, bins_a x bins_b int64) then receives
 *   np.histogram2d(speed_a[m], speed_b[m], (bins_a, bins_b), ranges)[0] with m = speed_b > *joint_speed_min_b (all samples
 *   with joint_speed_min_b == NULL).
 * joint_counts: host, 2 x int64, required.
 * v_x_a .. net_remodelling_b: NULL (stats only: no full-size stack exists anywhere beyond the pairs in flight), or
 *   (n_frames - 1, n_i, n_j) float64, v_x, v_y and speed of both channels together; the two net_remodelling may be NULL also
 *   then (required with include_remodelling).
 * _dev: the movies and the eight field stacks are device pointers; _host: host pointers, staged through the context's pinned
 * bounce buffer.  Everything else is host memory in both. */
int vof_compare_flows_dev(vof_ctx* ctx, const double* movie_a, const double* movie_b, int n_frames,
                          const double* blur_weights_a, int blur_radius_a, const double* blur_weights_b, int blur_radius_b,
                          int box_size, double delta_x, double delta_t, int include_remodelling, int reference_quirks,
                          const double* histogram_edges, int histogram_bins, int64_t* histograms,
                          int angle_bins, int64_t* angle_histograms, double* weighted_angle_histograms,
                          int relative_angle_bins, int64_t* relative_angle_histogram, double* weighted_relative_angle_histogram,
                          const double* joint_speed_edges_a, int joint_speed_bins_a,
                          const double* joint_speed_edges_b, int joint_speed_bins_b,
                          const double* joint_speed_min_b, int64_t* joint_speed_histogram,
                          int64_t* joint_counts, vof_compare_stats* stats,
                          double* v_x_a, double* v_y_a, double* speed_a, double* net_remodelling_a,
                          double* v_x_b, double* v_y_b, double* speed_b, double* net_remodelling_b);
int vof_compare_flows_host(vof_ctx* ctx, const double* movie_a, const double* movie_b, int n_frames,
                           const double* blur_weights_a, int blur_radius_a, const double* blur_weights_b, int blur_radius_b,
                           int box_size, double delta_x, double delta_t, int include_remodelling, int reference_quirks,
                           const double* histogram_edges, int histogram_bins, int64_t* histograms,
                           int angle_bins, int64_t* angle_histograms, double* weighted_angle_histograms,
                           int relative_angle_bins, int64_t* relative_angle_histogram, double* weighted_relative_angle_histogram,
                           const double* joint_speed_edges_a, int joint_speed_bins_a,
                           const double* joint_speed_edges_b, int joint_speed_bins_b,
                           const double* joint_speed_min_b, int64_t* joint_speed_histogram,
                           int64_t* joint_counts, vof_compare_stats* stats,
                           double* v_x_a, double* v_y_a, double* speed_a, double* net_remodelling_a,
                           double* v_x_b, double* v_y_b, double* speed_b, double* net_remodelling_b);

/* The two per-frame preprocessing steps the reference's scripts run around every estimator (OF.py:308-374), OpenCV 4's
 * arithmetic restated in integer / float32 operations (DESIGN.md section 14 has the specification; parity with the real cv2 is
 * not tested in this repository).  Both first reduce the whole stack to (max, min of the finite values, non-finite count),
 * written to range[3] (host, may be NULL), and return 1 - nothing else computed, vof_last_error says why - where the
 * reference's integer cast would be platform-dependent or wrap:
 *   threshold: a non-finite value, min < 0 or max <= 0;   CLAHE: a non-finite value, min < 0 or max >= 65536.
 * Frames are processed in chunks of frames_in_flight (0: sized from the free device memory, 16 at most).  The scratch memory,
 * the context's one scratch buffer (vof_blur_stack_*), holds per frame in flight: threshold 4 bytes per pixel, CLAHE
 * 65536 x 6 bytes per tile, _host the staged frame and its result; once per call: the records of the range reduction (and the
 * tables of the calls below).  It is allocated on first use, grown on demand, kept, and freed by
 * vof_destroy; nothing in it is kept from one call to the next.  Results do not depend on frames_in_flight.
 * Profiler: class VOF_K_PREPROCESS, the `level` is the stage: 0 range, 1 row sums, 2 threshold, 3 histograms, 4 tables, 5 blend.
 *
 * vof_adaptive_threshold_*: cv2.adaptiveThreshold(u, 1, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY, window_size, threshold) == 1 of
 *   u = (uint8) trunc((x / max) * 255.0) per frame: mask = (u - mean) > -ceil(threshold), mean = the sum of u over the
 *   window_size x window_size window (indices clamped to the image) divided by window_size^2, rounded to nearest.
 *   window_size: odd, 3 .. 4095 (every window sum then fits 32 bits); n_j <= 15360.  mask: n_frames x n_i x n_j bytes, 0 / 1.
 * vof_clahe_*: cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply of v = (uint16) trunc(x) per frame, as float64.
 *   tiles_x runs along n_j (1 .. n_j - 1), tiles_y along n_i (1 .. n_i - 1); clip_limit <= 0: no clipping.
 * _dev: movie and the result are device pointers; _host: host pointers, staged through the context's pinned bounce buffer. */
int vof_adaptive_threshold_dev(vof_ctx* ctx, const double* movie, int n_frames, int window_size, double threshold,
                               int frames_in_flight, uint8_t* mask, double* range);
int vof_adaptive_threshold_host(vof_ctx* ctx, const double* movie, int n_frames, int window_size, double threshold,
                                int frames_in_flight, uint8_t* mask, double* range);
int vof_clahe_dev(vof_ctx* ctx, const double* movie, int n_frames, double clip_limit, int tiles_x, int tiles_y,
                  int frames_in_flight, double* out, double* range);
int vof_clahe_host(vof_ctx* ctx, const double* movie, int n_frames, double clip_limit, int tiles_x, int tiles_y,
                   int frames_in_flight, double* out, double* range);

/* The resize of the reference's small-grid experiments, cv2.resize(frame, dsize=(out_j, out_i), interpolation=cv2.INTER_AREA)
 * of every frame of a one-channel stack when neither axis is enlarged (1 <= out_i <= n_i, 1 <= out_j <= n_j), OpenCV 4's
 * arithmetic restated operation by operation (DESIGN.md section 15 has the specification; parity with the real cv2 is not
 * tested in this repository).  Frames arrive as float64 whatever the arithmetic; the result is float64, n_frames x out_i x out_j.
 *   VOF_RESIZE_U8:  the arithmetic OpenCV applies to uint8 frames - float32 sums where a scale is fractional, integer block
 *     sums where both are integers, the result rounded to 0 .. 255 (half to even; half up on the 2 x 2 path).  The stack is
 *     first reduced as in the calls above: a non-finite value, min < 0 or max > 255 returns 1, nothing else computed,
 *     vof_last_error says why.  That every value is an integer is the caller's contract and is not checked.
 *   VOF_RESIZE_F64: the arithmetic of float64 frames - float64 sums with float32 weights; NaN and Inf propagate.
 * Frames are processed in chunks of frames_in_flight (0: sized from the free device memory, 16 at most).  In the scratch
 * buffer of the calls above: once per call the two axis tables, built on the host; per frame in flight, _host only, the staged
 * frame and its result.  Results do not depend on frames_in_flight.  Profiler: class VOF_K_PREPROCESS, `level` 6.
 * _dev: movie and out are device pointers (out must not alias movie); _host: host pointers, staged through the context's
 * pinned bounce buffer. */
enum vof_resize_arithmetic { VOF_RESIZE_U8 = 0, VOF_RESIZE_F64 = 1 };
int vof_resize_area_dev(vof_ctx* ctx, const double* movie, int n_frames, int out_i, int out_j, int arithmetic,
                        int frames_in_flight, double* out);
int vof_resize_area_host(vof_ctx* ctx, const double* movie, int n_frames, int out_i, int out_j, int arithmetic,
                         int frames_in_flight, double* out);

/* Farnebaeck's dense flow of n_pairs frame pairs, cv2.calcOpticalFlowFarneback(first[k], second[k], None, pyr_scale, levels,
 * winsize, iterations, poly_n, poly_sigma, OPTFLOW_FARNEBACK_GAUSSIAN) without an initial flow, OpenCV 4's arithmetic restated
 * operation by operation in float32 and, where OpenCV uses it, double (DESIGN.md section 16 has the specification; parity
 * with the real cv2 is not tested in this repository).  first and second are two stacks of n_pairs frames of n_i x n_j
 * float64 each and may be two views of one movie (second = first + n_i * n_j).  Everything that needs an exp is planned by the
 * caller (farneback_plan of the Python package) and arrives as host arrays:
 *   n_levels, level_sizes[2 * n_levels]   (height, width) of the pyramid's images, finest first; level 0 is (n_i, n_j)
 *   ksizes[n_levels], presmooth_taps      the odd tap counts of the blur that precedes the resize to a level, and the taps of
 *                                         all levels one after the other (float32)
 *   poly_n, poly_tables, poly_ig          1 .. 10; g | xg | xxg, 2 poly_n + 1 float32 each (offsets -poly_n .. poly_n); the
 *                                         four entries (1,1), (0,3), (3,3), (5,5) of the inverse moment matrix
 *   winsize, window_taps                  1 .. 129; the winsize / 2 + 1 float32 taps k[0 ..] of the Gaussian window
 *   iterations, flow_scale                >= 0; float32(1 / pyr_scale), applied to the flow carried to the next finer level
 *   velocity_scale                        delta_x / delta_t
 * Results: v_x = channel 0 of OpenCV's flow (along n_j), v_y = channel 1 (along n_i), promoted to float64 and multiplied by
 * velocity_scale, and speed = sqrt(v_x^2 + v_y^2); n_pairs x n_i x n_j each.  Both stacks are first reduced as in the
 * preprocessing calls above: a non-finite value returns 1, nothing else computed, vof_last_error says why.
 * Pairs are processed in chunks of frames_in_flight (0: sized from the free device memory, 16 at most).  In the scratch buffer
 * of the calls above: once per call the tap tables; per pair in flight 108 bytes per pixel of planes and, _host only, the two
 * staged frames and the three results.  Results do not depend on frames_in_flight.
 * Frames of at least 16 x 16.  Profiler: class VOF_K_PREPROCESS, `level` 7 level images, 8 polynomial expansion, 9 flow carried
 * to a level, 10 matrices, 11 window rows (vertical pass), 12 window columns + solve + update, 13 results.
 * _dev: the stacks and the results are device pointers; _host: host pointers, staged through the pinned bounce buffer. */
int vof_farneback_dev(vof_ctx* ctx, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes,
                      const int* ksizes, const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig,
                      int winsize, const float* window_taps, int iterations, float flow_scale, double velocity_scale,
                      int frames_in_flight, double* v_x, double* v_y, double* speed);
int vof_farneback_host(vof_ctx* ctx, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes,
                       const int* ksizes, const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig,
                       int winsize, const float* window_taps, int iterations, float flow_scale, double velocity_scale,
                       int frames_in_flight, double* v_x, double* v_y, double* speed);

/* The same with OpenCV's default window (flags without OPTFLOW_FARNEBACK_GAUSSIAN): the box window of 2 (winsize / 2) + 1 rows and
 * columns, which OpenCV keeps as two running sums in double - down the columns, then along the rows - and divides by winsize^2;
 * the sums are formed in OpenCV's order of additions ("Iteration, box window").  The arguments are those
 * of vof_farneback_* without window_taps; everything else - levels, level images, expansion, matrices, results, the range
 * reduction and its return code 1, chunking - is shared with them.  winsize: 2 .. 129; at winsize 1 OpenCV's start values count
 * row 0 and column 0 once too often, which is not restated: -1.
 * Scratch per pair in flight: 128 bytes per pixel of planes instead of 108 - 32 float32 planes, of which the window's vertical
 * running sums take ten as five double planes - and, _host only, the staged frames and results; the same buffer, re-carved by
 * either variant.  Profiler: class VOF_K_PREPROCESS, `level` 7 - 10 and 13 as above, 14 window rows (the vertical running sum),
 * 15 window columns (the horizontal running sum) + solve + update; 11 and 12 stay the Gaussian window's. */
int vof_farneback_box_dev(vof_ctx* ctx, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes,
                          const int* ksizes, const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig,
                          int winsize, int iterations, float flow_scale, double velocity_scale, int frames_in_flight, double* v_x,
                          double* v_y, double* speed);
int vof_farneback_box_host(vof_ctx* ctx, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes,
                           const int* ksizes, const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig,
                           int winsize, int iterations, float flow_scale, double velocity_scale, int frames_in_flight, double* v_x,
                           double* v_y, double* speed);

/* The reference's filter of a finished flow result, optical_flow.filter_PIV_flow_result (OF.py:2232-2250), in place on the
 * n_pairs x n_i x n_j float64 stacks v_x, v_y and speed.  movie: the first n_pairs frames of the result's original data, float64.
 * Per chunk of frames_in_flight frames (0: sized from the free device memory, 16 at most) the frames are blurred into the
 * scratch buffer with the kernels of vof_blur_stack_* (blur_weights: 2 * blur_radius + 1 taps; same bits) and one kernel
 * applies, per sample: low = blurred < intensity_threshold; fast = speed > speed_threshold on the incoming speed; v_x and v_y
 * become 0.0 where low or fast; speed becomes 0.0 where fast, and where low too with zero_speed_under_low != 0 (the reference
 * leaves it).  NaN compares false and is kept; +inf > speed_threshold is true.  The blurred movie never exists at stack size.
 * counts (host, 2 x int64): the samples with low, the samples with fast.  A NaN threshold returns -1.
 * Profiler: class VOF_K_REDUCE, `level` 1 (the mask kernel; the blur is VOF_K_RHS).
 * _dev: movie and the three stacks are device pointers; _host: host pointers, staged through the pinned bounce buffer. */
int vof_flow_filter_dev(vof_ctx* ctx, const double* movie, int n_pairs, const double* blur_weights, int blur_radius,
                        double intensity_threshold, double speed_threshold, int zero_speed_under_low, int frames_in_flight,
                        double* v_x, double* v_y, double* speed, int64_t* counts);
int vof_flow_filter_host(vof_ctx* ctx, const double* movie, int n_pairs, const double* blur_weights, int blur_radius,
                         double intensity_threshold, double speed_threshold, int zero_speed_under_low, int frames_in_flight,
                         double* v_x, double* v_y, double* speed, int64_t* counts);

/* The comparison of two finished flow results the reference's scripts make (analyse_short_timeinterval_data.py:697-745): six
 * n_pairs x n_i x n_j float64 stacks, v_x, v_y and speed of result a and of result b, read in chunks of frames_in_flight pairs
 * (as above); 48 bytes per sample and pass, nothing of field size is written and the stacks are never modified.
 * Per sample, float64, every operation explicit and in this order:
 *   sa, sb = the speeds with NaN replaced by 0;  a sample whose sa or sb is +-inf takes no part below;
 *   m1 = sa > speed_threshold and sb > speed_threshold;
 *   dot = v_x_b * v_x_a + v_y_b * v_y_a;  w = sb * sa;  cos = dot / w;  theta = acos(cos), radians;
 *   m2 = sa > angle_threshold and sb > angle_threshold.
 * With reference_quirks cos is not clipped (a rounding excess over 1 is a NaN theta); without, it is clipped to [-1, 1] first
 * (NaN stays NaN).
 * vof_flow_extremes_*: the first pass.  extremes (host, 6 doubles): min and max of sa over the m1 samples, of sb over the m1
 *   samples, and of cos over the m2 samples whose theta is not NaN; +inf and -inf where there is no such sample.  Exact and
 *   order independent: block partials and a final reduction, no floating-point atomics.
 * vof_flow_compare_*: the second pass.  joint_speed_histogram (host, bins_a x bins_b int64) receives
 *   np.histogram2d(sa[m1], sb[m1], bins, ranges)[0] for the np.linspace edges given (joint_speed_bins: 1 .. 1024 bins per axis),
 *   angle_histogram (host, angle_bins int64; angle_bins: 1 .. 64) np.histogram(theta[m2], angle_bins, range)[0] without the NaN.
 *   clamp_angle != 0 (a range chosen from the extremes of these stacks): a theta outside the edges is counted in the first or
 *   the last bin; 0 (an explicit range): it is dropped, as numpy drops it.  Edges are host memory and must increase.
 *   counts (host, 6 x int64): NaN speeds of a, of b; samples with an infinite speed; m1 samples; m2 samples whose theta is not
 *   NaN; m2 samples whose theta is NaN (in no bin).  Counters live in LDS first (2-D histograms of more than 4096 bins in global
 *   memory); integer atomics only, so every result is bit-identical from call to call and for every frames_in_flight.
 * Profiler: class VOF_K_REDUCE, `level` 2 (extremes) and 3 (histograms).
 * _dev: the six stacks are device pointers; _host: host pointers, staged through the pinned bounce buffer. */
int vof_flow_extremes_dev(vof_ctx* ctx, const double* v_x_a, const double* v_y_a, const double* speed_a, const double* v_x_b,
                          const double* v_y_b, const double* speed_b, int n_pairs, double speed_threshold, double angle_threshold,
                          int reference_quirks, int frames_in_flight, double* extremes);
int vof_flow_extremes_host(vof_ctx* ctx, const double* v_x_a, const double* v_y_a, const double* speed_a, const double* v_x_b,
                           const double* v_y_b, const double* speed_b, int n_pairs, double speed_threshold, double angle_threshold,
                           int reference_quirks, int frames_in_flight, double* extremes);
int vof_flow_compare_dev(vof_ctx* ctx, const double* v_x_a, const double* v_y_a, const double* speed_a, const double* v_x_b,
                         const double* v_y_b, const double* speed_b, int n_pairs, double speed_threshold, double angle_threshold,
                         int reference_quirks, const double* joint_speed_edges_a, int joint_speed_bins_a,
                         const double* joint_speed_edges_b, int joint_speed_bins_b, const double* angle_edges, int angle_bins,
                         int clamp_angle, int frames_in_flight, int64_t* joint_speed_histogram, int64_t* angle_histogram,
                         int64_t* counts);
int vof_flow_compare_host(vof_ctx* ctx, const double* v_x_a, const double* v_y_a, const double* speed_a, const double* v_x_b,
                          const double* v_y_b, const double* speed_b, int n_pairs, double speed_threshold, double angle_threshold,
                          int reference_quirks, const double* joint_speed_edges_a, int joint_speed_bins_a,
                          const double* joint_speed_edges_b, int joint_speed_bins_b, const double* angle_edges, int angle_bins,
                          int clamp_angle, int frames_in_flight, int64_t* joint_speed_histogram, int64_t* angle_histogram,
                          int64_t* counts);

/* The illumination correction of the reference's real-data scripts, optical_flow.correct_intensity_change
 * (analyse_short_timeinterval_data.py:241-301, 128-145), of n_frames float64 frames.  With G(f, taps) the blur of vof_blur_stack_*
 * (same kernels or the same arithmetic in the same order: same bits), per frame k, in this order and nothing else:
 *   B[k] = G(movie[k], smoothing_weights)      (smoothing_weights NULL: B = movie, no first blur; smoothing_radius is then ignored)
 *   D    = B[k] - B[reference_frame]           (one float64 subtraction per pixel)
 *   E    = G(D, filter_weights)                (the drift)
 *   out[k] = Tg[k] - E,  Tg = B for target VOF_INTENSITY_TARGET_BLURRED, the movie for VOF_INTENSITY_TARGET_ORIGINAL.
 * drift (n_frames frames, may be NULL) receives E.  Weights are host memory, 2 * radius + 1 taps each.  reference_frame:
 * 0 .. n_frames - 1; its D is +0.0, its drift 0 and its output Tg[reference_frame] bit for bit.  NaN and Inf propagate through
 * the taps.  out and drift alias neither each other nor movie.
 * Frames are walked in chunks of frames_in_flight (0: sized from the free device memory, 16 at most).  Scratch: once per call the
 * blurred reference frame and the taps; per frame in flight the blurred frame (with a first blur) and the row-filtered frame -
 * D and E never exist as stacks - and, _host only, the staged frames and results.  The difference is formed by the loader of the
 * second blur's axis-0 pass and the subtraction by the store of its axis-1 pass, so a frame moves 10 planes (4 + 3 + 3), not the 14
 * of blur, difference, blur, subtraction.  Results do not depend on frames_in_flight nor on the chunk that holds the reference.
 * Profiler: class VOF_K_PREPROCESS, stage 16 axis-0 pass, 17 axis-1 pass (the first blur is VOF_K_RHS).  The profiler keeps 16
 * `level` slots per class, so both are summed in slot 15, with stage 15 of vof_farneback_box_* if that ran since the last reset;
 * VOF_DEBUG_SYNC names the stages apart.
 * _dev: movie, out and drift are device pointers; _host: host pointers, staged through the pinned bounce buffer. */
#define VOF_INTENSITY_TARGET_BLURRED 0
#define VOF_INTENSITY_TARGET_ORIGINAL 1
int vof_intensity_correct_dev(vof_ctx* ctx, const double* movie, int n_frames, const double* smoothing_weights, int smoothing_radius,
                              const double* filter_weights, int filter_radius, int reference_frame, int target, int frames_in_flight,
                              double* out, double* drift);
int vof_intensity_correct_host(vof_ctx* ctx, const double* movie, int n_frames, const double* smoothing_weights, int smoothing_radius,
                               const double* filter_weights, int filter_radius, int reference_frame, int target, int frames_in_flight,
                               double* out, double* drift);

/* np.histogram(F[k].ravel(), bins, range)[0] of every frame, optical_flow.intensity_histograms: F the movie, or with blur_weights
 * (host, 2 * blur_radius + 1 taps; NULL: none) its blur, taken a chunk of frames_in_flight frames at a time and never a stack.
 * edges: host, the bins + 1 values of np.linspace(lo, hi, bins + 1), increasing; bins: 1 .. 2^20.  The bin index is corrected
 * against the edges, the last bin is closed on the right, NaN and values outside [lo, hi] are dropped.
 * counts (host, n_frames x bins int64) and nonfinite (host, n_frames int64: the NaN / Inf values of F[k]) are overwritten.
 * Counters live in LDS up to 1024 bins, in global memory above; integer atomics only, so every count is the same from call to
 * call and for every frames_in_flight.  Profiler: class VOF_K_PREPROCESS, stage 18 (slot 15, as above).
 * _dev: movie is a device pointer; _host: a host pointer, staged through the pinned bounce buffer. */
int vof_intensity_hist_dev(vof_ctx* ctx, const double* movie, int n_frames, const double* blur_weights, int blur_radius,
                           const double* edges, int bins, int frames_in_flight, int64_t* counts, int64_t* nonfinite);
int vof_intensity_hist_host(vof_ctx* ctx, const double* movie, int n_frames, const double* blur_weights, int blur_radius,
                            const double* edges, int bins, int frames_in_flight, int64_t* counts, int64_t* nonfinite);

/* The dense part of optical_flow.convert_PIV_result (OF.py:2141-2230), optical_flow.upsample_PIV_vectors: the piecewise cubic
 * of scipy.interpolate.griddata(points, values, targets, method='cubic') - a Clough-Tocher element on every triangle of a
 * Delaunay triangulation - of the two vector components at every pixel of n_frames frames of n_i x n_j, and its speed.
 * out[k][i][j] is the value at the target (x = j, y = i).  The triangulation and the gradients are the caller's (scipy's
 * Delaunay and CloughTocher2DInterpolator(tri, values).grad): host tables of all frames, frame after frame, with
 * point_offsets and triangle_offsets (n_frames + 1 int32 each, starting at 0) saying where a frame's rows lie:
 *   points, values: 2 doubles per point (x, y; v_x, v_y);  gradients: 4 (d v_x/dx, d v_x/dy, d v_y/dx, d v_y/dy);
 *   simplices, neighbours: 3 int32 per triangle, indices local to the frame, neighbour k opposite vertex k, -1 for none;
 *   transforms: 6 doubles per triangle, tri.transform - the 2 x 2 inverse, row-major, then the offset r.
 * Every table is checked before anything is uploaded: indices inside their frame, every number finite (-1 otherwise).
 * Per target q, float64, every operation single and uncontracted, in the order of tests/piv_restatement.py:
 *   c0 = T00 (qx - rx) + T01 (qy - ry), c1 = T10 (qx - rx) + T11 (qy - ry), c2 = 1 - c0 - c1 in triangle t; t includes q when
 *   all three lie in [-eps, 1 + eps], eps = 100 DBL_EPSILON; of the triangles that include q the lowest index is taken; the
 *   19 control values of scipy's element from the three vertices and the centroids of the neighbours; m = min(c),
 *   b = c - m, b4 = 3 m and the 19 terms summed left to right with powers as products; speed = sqrt(v_x v_x + v_y v_y).
 * A pixel no triangle includes is NaN in v_x, v_y and speed.  A frame without triangles is the caller's to fill (a frame with a
 * degenerate simplex, whose transform holds NaN, is refused with triangles): it is written as NaN and counted.
 * counts (host, 2 x int64): the pixels outside every triangle of the frames that have triangles; the frames without.
 * Frames are walked in chunks of frames_in_flight (0: sized from the free device memory, 16 at most); scratch per frame in
 * flight: the tables at the size of the largest frame, 44 doubles per triangle and an int32 map of the frame.  Integer atomics
 * only: results are the same from call to call and for every frames_in_flight.
 * Profiler: class VOF_K_REDUCE, `level` 4 control values, 5 the map, 6 evaluation.
 * _dev: v_x, v_y and speed are device pointers; _host: host pointers, staged through the pinned bounce buffer. */
int vof_piv_upsample_dev(vof_ctx* ctx, int n_frames, const double* points, const double* values, const double* gradients,
                         const int32_t* simplices, const int32_t* neighbours, const double* transforms, const int32_t* point_offsets,
                         const int32_t* triangle_offsets, int frames_in_flight, double* v_x, double* v_y, double* speed,
                         int64_t* counts);
int vof_piv_upsample_host(vof_ctx* ctx, int n_frames, const double* points, const double* values, const double* gradients,
                          const int32_t* simplices, const int32_t* neighbours, const double* transforms, const int32_t* point_offsets,
                          const int32_t* triangle_offsets, int frames_in_flight, double* v_x, double* v_y, double* speed,
                          int64_t* counts);

/* optical_flow.conduct_piv: direct (spatial-domain) zero-normalised cross-correlation PIV of the n_pairs frame pairs of
 * movie (n_pairs + 1 float64 frames of n_i x n_j), in n_passes passes (1 to 8) with integer window offsets from the pass
 * before.  Pass p has the window size w_p = window_sizes[p], the search radius r_p = search_radii[p] and the step
 * s_p = steps[p] (int32 each); its margin is m_p = r_0 + ... + r_p and its grid R_p = (n_i - w_p - 2 m_p) / s_p + 1,
 * C_p likewise from n_j (integer division); window (a, b) has its top-left pixel at i0 = m_p + a s_p, j0 = m_p + b s_p.
 * Refused with -1 and a message, before anything is uploaded: w outside [4, 64], r outside [1, 16], s < 1, a w that grows
 * from one pass to the next, an empty grid (n_i or n_j < w_p + 2 m_p), R_p > 65535, a window whose LDS need
 * 8 (w (w|1) + S (S|1) + 2 S D) bytes, S = w + 2 r, D = 2 r + 1, exceeds 160 KiB - 2 KiB (no accepted w and r does).
 * float64, every operation single and uncontracted, in the order of tests/piv_flow_restatement.py:
 *   offset: (0, 0) in pass 0; later the vector (u', v') of the pass before at a' = clamp(floor((2 (i0 - m_{p-1}) + w_p -
 *     w_{p-1} + s_{p-1}) / (2 s_{p-1})), 0, R_{p-1} - 1), b' likewise: o_i = (int) floor(v' + 0.5), o_j = (int) floor(u' + 0.5),
 *     (0, 0) if the vector is NaN.  |o| <= m_{p-1}, so no search region leaves the frame.  Computed on the device.
 *   sums: A the w x w window of frame k at (i0, j0), B_d that of frame k + 1 at (i0 + o_i + d_i, j0 + o_j + d_j), d in
 *     [-r, r]^2.  S_a, S_aa, S_b, S_bb, S_ab: each window row summed left to right from 0.0, the row sums added top to bottom
 *     from 0.0, every product rounded before it is added.
 *   correlation: n = w w, D_a = n S_aa - S_a S_a, D_b = n S_bb - S_b S_b, C(d) = (n S_ab - S_a S_b) / sqrt(D_a D_b);
 *     !(D_a > 0): a flat window, u, v and correlation NaN; !(D_b > 0): C(d) = -inf.
 *   peak: the first maximum of C in raster order over (d_i, d_j), c0; c0 = -inf: u and v NaN (counted as flat).
 *   subpixel, per axis, where the peak is not on the border of the search range on that axis and both neighbours c-, c+ are
 *     finite: den = 2.0 * ((c- - 2.0 * c0) + c+); den < 0: delta = (c- - c+) / den; otherwise delta = 0.
 *   v = (double)(o_i + d_i) + delta_i (along rows), u = (double)(o_j + d_j) + delta_j (along columns), pixels per frame.
 *   c0 < min_correlation (NaN: no threshold): u and v NaN, the correlation is kept; in every pass.
 * u, v, correlation: the last pass, n_pairs x R x C doubles each.  counts (host, n_passes x 3 int64): windows that are flat
 * (or have no valid displacement), whose peak lies on the border of the search range, that fell under the threshold.
 * The movie must be finite.  Pairs are walked in chunks of frames_in_flight (0: sized from the free device memory, 16 at most);
 * scratch per pair in flight: the vectors of the earlier passes and two int32 per window.  Integer atomics only: results
 * are the same from call to call and for every frames_in_flight.
 * Profiler: class VOF_K_REDUCE, `level` 7 the offsets, 8 + p the correlation of pass p.
 * _dev: movie, u, v and correlation are device pointers; _host: host pointers, staged through the pinned bounce buffer. */
int vof_piv_flow_dev(vof_ctx* ctx, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes,
                     const int32_t* search_radii, const int32_t* steps, double min_correlation, int frames_in_flight, double* u,
                     double* v, double* correlation, int64_t* counts);
int vof_piv_flow_host(vof_ctx* ctx, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes,
                      const int32_t* search_radii, const int32_t* steps, double min_correlation, int frames_in_flight, double* u,
                      double* v, double* correlation, int64_t* counts);

/* vof_piv_flow_* with two options, independent of each other; with deformation 0 and outlier_threshold NaN it is that call,
 * bit for bit (vof_piv_flow_* is this call with everything off).  Grids, margins, limits and LDS need are unchanged.
 * Refused with -1 and a message, besides what vof_piv_flow_* refuses: deformation or validate_last other than 0 or 1; an
 * outlier_threshold that is neither NaN nor positive and finite; an outlier_epsilon that is not >= 0 and finite; validate_last
 * with outlier_threshold NaN; validation_counts NULL with outlier_threshold given.
 * float64, every operation single and uncontracted, only + - * / sqrt floor fabs fmin fmax, in the order of
 * tests/piv_deform_restatement.py:
 *   validation (outlier_threshold given) of the vectors of pass p before pass p + 1 uses them, and with validate_last of the
 *     returned vectors of the last pass - the normalised median test (Westerweel & Scarano 2005), reading the unvalidated field
 *     and writing a second one: a vector is valid when neither component is NaN; the neighbours of window (a, b) are the valid
 *     ones among the up to eight others of its 3 x 3 neighbourhood inside the grid; fewer than 3: the window is left as it is
 *     and not counted.  med of k values: sorted ascending (a fixed 8-input network that exchanges where y < x, absent values
 *     +inf), the middle one for odd k, (lo + hi) * 0.5 for even k.  u_m = med(u_n), v_m = med(v_n).  Centre not valid: it becomes
 *     (u_m, v_m), counted as filled.  Centre valid: r_u = fabs(u - u_m) / (med(fabs(u_n - u_m)) + outlier_epsilon), r_v likewise;
 *     r_u > outlier_threshold || r_v > outlier_threshold: it becomes (u_m, v_m), counted as an outlier.  The correlation values are
 *     never changed; counts keeps its meaning (what the correlation of the pass found).  On the integer path the offsets are then
 *     taken from the validated vectors (a median of values bounded by m is bounded by m).
 *   predictor from pass q = p - 1 at a real position (y, x): c = (double)m_q + (double)(w_q - 1) / 2.0; g = (y - c) / (double)s_q;
 *     g = fmin(fmax(g, 0.0), (double)(R_q - 1)); lo = (int)floor(g), but max(R_q - 2, 0) if lo > R_q - 2; t = g - (double)lo;
 *     hi = min(lo + 1, R_q - 1); likewise along the columns with C_q.  A vector that is not valid reads as (0, 0).  Bilinear:
 *     top = F[lo][b] + t_b * (F[lo][b_hi] - F[lo][b]), bot likewise on row hi, value = top + t_a * (bot - top); U and V separately.
 *   deformation, pass p >= 1: pixel (i, j) of the search region holds frame k + 1 at y = (double)i + V(i, j), x = (double)j +
 *     U(i, j), (U, V) the predictor at ((double)i, (double)j); the region is rows i0 - r .. i0 + w + r - 1 and columns likewise -
 *     no offset, always inside the frame; the sample by the split rule and the bilinear formula above with c = 0, s = 1 and
 *     n = n_i resp. n_j (the clamp is part of the arithmetic).  Sums, C(d), peak, subpixel fit, threshold and counts as in
 *     vof_piv_flow_* on that region; v = V_c + ((double)d_i + delta_i), u = U_c + ((double)d_j + delta_j), (U_c, V_c) the
 *     predictor at the window centre (i0 + (w - 1) / 2.0, j0 + (w - 1) / 2.0).  Pass 0 is unchanged; one pass: no effect.
 * validation_counts (host, n_passes x 2 int64, may be NULL when outlier_threshold is NaN): outliers and filled vectors per
 * pass; the last row is zero unless validate_last.
 * Scratch per pair in flight, besides that of vof_piv_flow_*: two doubles per window for the validated vectors (and the
 * unvalidated ones of the last pass with validate_last); no offsets with deformation.
 * Profiler: the validation shares `level` 7 with the offsets; a deformed pass keeps 8 + p. */
int vof_piv_flow_ex_dev(vof_ctx* ctx, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes,
                        const int32_t* search_radii, const int32_t* steps, double min_correlation, int frames_in_flight, double* u,
                        double* v, double* correlation, int64_t* counts, int deformation, double outlier_threshold,
                        double outlier_epsilon, int validate_last, int64_t* validation_counts);
int vof_piv_flow_ex_host(vof_ctx* ctx, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes,
                         const int32_t* search_radii, const int32_t* steps, double min_correlation, int frames_in_flight, double* u,
                         double* v, double* correlation, int64_t* counts, int deformation, double outlier_threshold,
                         double outlier_epsilon, int validate_last, int64_t* validation_counts);

/* Mean and (population) variance of n device-resident doubles, deterministic two-pass reduction. */
int vof_field_moments_dev(vof_ctx* ctx, const double* field_dev, size_t n, double* mean, double* variance);

/* Replaces the sampling loop of subsample_velocities_for_visualisation (OF.py:1614-1632) for a device-resident
 * field stack (n_fields, n_i, n_j): out[k][a][b] = field[k][a*box + offset][b*box + offset], a < n_i / box,
 * b < n_j / box (the reference uses offset = round(box / 2)).  out_dev: (n_fields, n_i/box, n_j/box) doubles. */
int vof_subsample_dev(vof_ctx* ctx, const double* field_dev, int n_fields, int box, int offset, double* out_dev);

/* Benchmark harness (no counterpart in the reference; SURVEY.md section 8(d) fixes the recipe): n_frames frames of the
 * exactly translating synthetic texture, written to device memory,
 *   I_t(i, j) = clip(0.5 + scale * sum_k a_k cos(2 pi (f_k (i - ox_t) + g_k (j - oy_t)) / period + phi_k), 0, 1).
 * mode_params: host, 4 * n_modes doubles (f, g, a, phi); frame_offsets: host, (ox_t, oy_t) per frame. */
int vof_texture_stack_dev(vof_ctx* ctx, double* out_dev, int n_frames, const double* mode_params, int n_modes,
                          const double* frame_offsets, double period, double scale);

/* Smoother implementation: 1 (default) = fused streaming 4-colour sweep (one launch per sweep),
 * 0 = one launch per colour (the simple reference kernels, kept for A/B tests). */
int vof_set_fused_sweeps(vof_ctx* ctx, int on);

/* Fixed-work kernel benchmark (SURVEY 8(d) "fixed sweep count"): n_sweeps full 4-colour block-GS
 * sweeps of the fine level on n_pairs pairs of a device-resident movie.  Used by scripts/gpu_sweep_micro.py and
 * scripts/gpu_sweep_shape.py (bench.py times the whole solve and reads the per-class profiler instead). */
int vof_bench_sweeps_dev(vof_ctx* ctx, const double* movie, int n_pairs, const vof_params* p, int n_sweeps);

/* Built-in profiler: when enabled, every kernel launch is bracketed by HIP events on the
 * context's stream; totals are accumulated per kernel class and multigrid level. */
int vof_profile_enable(vof_ctx* ctx, int on);
int vof_profile_reset(vof_ctx* ctx);
/* Restrict event recording to one kernel class / level (-1 = any); keeps the timed region light. */
int vof_profile_filter(vof_ctx* ctx, int kernel_id, int level);
/* level < 0: sum over levels.  Outputs: number of launches, total milliseconds. */
int vof_profile_get(vof_ctx* ctx, int kernel_id, int level, int64_t* launches, double* total_ms);
/* Sum over the recorded launches of the number of frame pairs each launch actually processed
 * (converged pairs are skipped by later launches), i.e. the "units" of the roofline figure. */
int vof_profile_get_units(vof_ctx* ctx, int kernel_id, int level, int64_t* pair_launches);
/* Sum over the recorded launches of their algorithmic bytes (bytes per pixel of DESIGN.md section 3 x
 * level pixels x pairs processed); 0 for kernel classes that do not report it. */
int vof_profile_get_bytes(vof_ctx* ctx, int kernel_id, int level, double* algorithmic_bytes);
/* Same sum with the bytes a launch minimally has to MOVE.  Equal to the algorithmic bytes except for the level-0 smoother
 * k_sweep0m, where one pass over the data performs two sweeps (algorithmic: 80 bytes per pixel and sweep performed; moved:
 * 80 per pixel and pass). */
int vof_profile_get_moved(vof_ctx* ctx, int kernel_id, int level, double* moved_bytes);
const char* vof_kernel_name(int kernel_id);

/* ---- debug / test entry points: single building blocks on device memory of the context -------
 * All vectors are interior-grid vectors of level `level`, layout [pair][3][n_i(level)][n_j(level)].
 * vof_debug_setup must be called first (uploads frames, builds the Galerkin hierarchy). */
int vof_debug_setup(vof_ctx* ctx, const double* movie_host, int n_pairs, const vof_params* p);
/* 0: all guard regions intact (or VOF_DEBUG_CANARY off); -5: damaged, vof_last_error names buffer and offset */
int vof_debug_check_canaries(vof_ctx* ctx);
int vof_debug_level_shape(vof_ctx* ctx, int level, int* n_i, int* n_j);
int vof_debug_rhs(vof_ctx* ctx, double* b_host);                                   /* level 0 */
int vof_debug_apply(vof_ctx* ctx, int level, const double* x_host, double* y_host); /* y = A_l x */
int vof_debug_gs(vof_ctx* ctx, int level, double* x_host, const double* b_host, int colour);
/* one full fused 4-colour sweep (reverse: colour order 3,2,1,0; from_zero: ignore x, start from 0) */
int vof_debug_sweep(vof_ctx* ctx, int level, double* x_host, const double* b_host, int reverse, int from_zero);
/* nu full sweeps as the multigrid cycle runs them (on level 0: the passes of k_sweep0m, two sweeps each) */
int vof_debug_smooth(vof_ctx* ctx, int level, double* x_host, const double* b_host, int nu, int reverse, int from_zero);
int vof_debug_restrict(vof_ctx* ctx, int level, const double* fine_host, double* coarse_host);
int vof_debug_prolong_add(vof_ctx* ctx, int level, double* fine_host, const double* coarse_host);
/* stored level >= 1: coarse right-hand side R (b - A x_new) straight after ONE forward sweep x_old -> x_new with right-hand
 * side b (x_old_host NULL: the sweep started from zero), computed from the sweep's update alone (k_resrestrict_u) */
int vof_debug_resrestrict_u(vof_ctx* ctx, int level, const double* x_new_host, const double* x_old_host, double* coarse_host);
int vof_debug_stencil(vof_ctx* ctx, int level, double* c_host); /* [pair][81][n_i][n_j], level >= 1 */
int vof_debug_vcycle(vof_ctx* ctx, const double* r_host, double* e_host);
int vof_debug_coarse_solve(vof_ctx* ctx, const double* r_host, double* e_host);
/* y = M r (one cycle), v = A y, dots[2 k] = (v, r), dots[2 k + 1] = (v, v) of pair k - the Krylov step as the solver runs it;
 * *fused = 1 if the product came out of the cycle's last smoothing pass (k_sweep0m's trailing stage) */
int vof_debug_vcycle_apply(vof_ctx* ctx, const double* r_host, double* y_host, double* v_host, double* dots_host, int* fused);

#ifdef __cplusplus
}
#endif
#endif /* VOF_H */
