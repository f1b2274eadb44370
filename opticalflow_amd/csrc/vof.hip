// vof.hip - host side of libvof.so: context, workspace, multigrid hierarchy, BiCGStab driver, C ABI.
//
// Replaces the per-pair body of source/optical_flow.py::variational_optical_flow (OF.py:791-1186:
// scipy.sparse assembly + PETSc KSP bcgs / composite PC) with a batched, matrix-free solve on one
// MI355X: right-preconditioned BiCGStab (the reference's KSP type, OF.py:1081) whose preconditioner is
// one geometric-multigrid V-cycle with a 4-colour 3x3-block Gauss-Seidel smoother and Galerkin coarse
// operators; stopping rule ||b - A x|| <= rtol ||b|| (OF.py:1120,1126).  All frame pairs of a batch
// advance together; per-pair scalars stay on the device.
#include "vof_device.hpp"
#include "vof_sweep0r.hpp"
#include "vof_sweep0p.hpp"
#include "vof_stream0.hpp"
#include "vof_direct.hpp"
#include "vof_boxflow.hpp"
#include "vof_boxsweep.hpp"
#include "vof_blursweep.hpp"
#include "vof_compare.hpp"
#include "vof_flowcompare.hpp"
#include "vof_liushen.hpp"
#include "vof_preprocess.hpp"
#include "vof_resize.hpp"
#include "vof_farneback.hpp"
#include "vof_intensity.hpp"
#include "vof_piv.hpp"
#include "vof_pivflow.hpp"
#include "../../include/vof.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace vof;

namespace {

constexpr int COARSEST_MAX = 5;      // coarsen until max(n_i, n_j) <= COARSEST_MAX (5: dense inverse of <= 75 unknowns; was 9 = 243 unknowns, whose
                                     // Gauss-Jordan inversion took 4.4 ms per batch - the fused coarse-tail kernel makes the extra level free)
constexpr int MAX_PROF_RECS = 32768;
constexpr int MAX_LANES = 3;        // concurrent pair groups of one device solve (solve_range_dev, VOF_LANES)
constexpr int MAX_LANE_GROUPS = 2;  // groups of pairs a lane runs one after the other in the two-phase solve (VOF_LANE_GROUPS)
constexpr int AUTO_F64_AFTER = 8;   // vcycle_precision == 2: switch the V-cycle vectors to float64 after this many iterations

struct Level {
    int ni = 0, nj = 0;
    size_t npts = 0;
    void* C = nullptr;   // stored stencil [B][81][npts] (double or float); level 0: only for 1-level grids
    // V-cycle vectors; element type is float or double (ctx->vfloat), allocations are sized for double
    void* x = nullptr;  // levels >= 1
    void* b = nullptr;  // levels >= 1
    void* r = nullptr;  // residual scratch (all levels but the last)
    void* x2 = nullptr; // ping-pong partner of x for the out-of-place fused sweeps
};

struct ProfRec {
    hipEvent_t e0, e1;
    int kid, level, units;
    double bytes;  // algorithmic bytes of this launch (units x bytes per pair; SURVEY 8(d): per sweep / operator application performed)
    double moved;  // minimal bytes the launch has to move (differs when one pass performs two sweeps)
};

}  // namespace

struct vof_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int Ni = 0, Nj = 0, B = 0;
    std::vector<Level> L;
    double *kx = nullptr, *kb = nullptr, *kr = nullptr, *krh = nullptr, *kp = nullptr, *kv = nullptr, *kt = nullptr;
    double* ky = nullptr;   // V-cycle outputs y = M p and z = M s (V-typed: float when vfloat)
    double* kz = nullptr;
    double* b32 = nullptr;  // V-typed copy of the V-cycle right-hand side (p or s) when vfloat
    bool vfloat = false;    // V-cycle vectors stored as float32 (arithmetic stays FP64)
    bool vcoarse32 = false; // vcycle_precision 3: float64 vectors on level 0, float32 on the levels below (the two meet in the fused
                            // residual + restriction kernel and in the post-smoothing pass that interpolates the correction)
    bool l0_handoff = true; // VOF_L0_HANDOFF=0: the level-0 hand-off vectors stay float64 in vcycle_precision 3 (see h32)
    bool h32 = false;       // the cycles run now store their level-0 hand-off vectors as float32: the pre-smoothed iterate x and the
                            // cycle's result (y, z).  Set per BiCGStab iteration where handoff32_ok holds, and by vof_debug_vcycle*
    const PairParam* pp = nullptr;   // per-pair (alpha, beta, frame) overrides of the batch in solve_batch ("virtual pairs") or nullptr;
                                     // written by solve_batch alone (BatchReq), nullptr outside it - the debug entry points rely on that
    PairParam* pp_buf = nullptr;     // device storage for them (B entries, lazy)
    // warm start (two-phase solve of a stack): interior solutions of the phase-1 pairs, and device storage for a batch's
    // table of the saved solutions its pairs start from (BatchReq::guess; B entries, lazy)
    double* warm_x = nullptr;
    size_t warm_cap = 0;
    int* warm_src = nullptr;
    double* partials = nullptr;
    int nblk = 0;
    PairScalars* sc = nullptr;
    int* active = nullptr;
    int* alist = nullptr;        // slots of the pairs that were active at the host's last count, ascending (post_active_list)
    int alist_n = 0;             // ... and how many: the pair dimension of a launch that takes the list
    bool use_alist = true;       // VOF_ACTIVE_LIST=0: every launch covers all slots of the batch (no list)
    double* func3 = nullptr;
    double *W = nullptr, *invT = nullptr;
    int nd = 0;
    // host mirrors (pinned)
    int* h_active = nullptr;
    int* h_alist = nullptr;
    PairScalars* h_sc = nullptr;
    double* h_func3 = nullptr;
    char* h_bounce = nullptr;        // pinned bounce buffer of the debug / test entry points (lazy)
    hipEvent_t ev_batch[2] = {nullptr, nullptr};   // start / end of the batch in flight (vof_pair_stats.batch_ms)
    // staging for the host-pointer API (allocated lazily)
    double* st_movie = nullptr;
    double* st_out[4] = {nullptr, nullptr, nullptr, nullptr};
    double* st_out2[4] = {nullptr, nullptr, nullptr, nullptr};   // second output set (copy / solve overlap of the host API)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_solved[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr}, ev_uploaded[2] = {nullptr, nullptr};
    double* st_movie2 = nullptr;                                 // second frame buffer (upload of the next batch under the solve)
    char* scratch = nullptr;                                             // the one scratch buffer of the blur, the box flow's general path, the sweeps, the comparison and the frame-wise calls (lazy, grown on demand; the Scratch of the call in progress carves it anew)
    size_t scratch_bytes = 0;
    bool bf_lds_set = false;                                             // box flow, fused kernel: dynamic LDS limit raised
    bool bl_lds_set = false;                                             // tiled blur: dynamic LDS limit raised
    bool ls_lds_set = false;                                             // Liu-Shen flow, fused kernel: dynamic LDS limit raised
    double* tex_tab = nullptr;                                           // synthetic-texture tables (lazy)
    size_t tex_cap = 0;
    // GMRES fallback (allocated on first use): basis vectors V_0..V_m (each B * len0), per-pair state, partials, flags
    double* gm_V = nullptr;
    GmresState* gm_state = nullptr;
    double* gm_partials = nullptr;
    int* gm_cycle = nullptr;
    int gm_m = 0;                // restart length the basis holds
    int gm_want = 0;             // restart length it was asked for (> gm_m where the free memory cut it)
    long long gmres_pairs = 0;   // pairs handed to the fallback since the context was created
    struct Alloc { void* raw; char* user; size_t bytes; const char* name; int line; };
    std::vector<Alloc> allocs;     // every device buffer of the context (raw != user only with guard regions)
    int c_bytes_per_point = 0;     // stencil storage allocated per point of a stored level (120 float8 .. 648 float64)
    size_t bytes = 0;
    std::string err;
    // state of the last setup
    const double* frames = nullptr;  // device pointer to frame 0 of the current batch
    int npairs = 0;
    vof_params prm;
    int cfmt = 0;   // storage format of the stored stencils of the current hierarchy: 0 double, 1 float, 2 CoefB16 (levels >= 1;
                    // the stored level 0 of a one-level grid is always double)
    bool fused = true;   // fused streaming 4-colour sweeps (false: one launch per colour)
    bool fold_stored = false;   // stored levels, packed stencils (k_sweep_st): the coarse-grid correction interpolated inside the first
                                // post-sweep (VOF_FOLD_STORED=1; measured: the sweep gets slower by what the stand-alone prolongation
                                // kernel costs, so that one stays)
    bool fuse_revisit = true;   // VOF_FUSE_REVISIT=0: between two visits of the W-cycle's revisited level, the post-smoothing sweep of one
                                // visit and the pre-smoothing sweep of the next as two k_sweep_st launches instead of one k_sweep_st2 pass
    int galerkin_fast = 1;      // VOF_GALERKIN_FAST, level-0 Galerkin product.  bit 0: a kernel of its own for the coarse points away from
                                // the border; bit 1 (with bit 0): that kernel evaluates the closed form (last bits differ; off by
                                // default).  0: the generic kernel for every point
    // direct preconditioner (block-tridiagonal LU by image rows, vof_direct.hpp); buffers allocated on first use
    bool direct_on = false;          // the batch in solve_batch is preconditioned by the direct solver instead of the multigrid cycle
                                     // (BatchReq::direct; written by solve_batch alone)
    int dir_cap = 0;                 // pairs the direct buffers hold
    double *dir_T = nullptr, *dir_tabs = nullptr, *dir_W = nullptr, *dir_r = nullptr, *dir_y = nullptr, *dir_x = nullptr, *dir_t = nullptr;
    int *dir_ipiv = nullptr, *dir_info = nullptr;
    double *dir_R = nullptr, *dir_C = nullptr, *dir_D = nullptr;   // blocked inverse: row panel, column panel, inverted diagonal tile
    int dir_ld = 0;                  // leading dimension of the dense blocks (m, or m rounded up to the tile size of the blocked inverse)
    long long direct_pairs = 0;      // pairs solved with the direct preconditioner since the context was created
    size_t pivflow_lds[4] = {0, 0, 0, 0};  // dynamic LDS k_pivflow_correlate<PF_SHORT_RUN / PF_LONG_RUN>, then their DEFORM variants, may ask for (raised on first need)
    // what a level-0 pass may take on besides its sweeps (plan_l0_pass decides; the requests travel in CycleIO / SmoothArgs)
    bool fuse_rr = true;        // VOF_FUSE_RR=0: the stand-alone kernel k_stream_resrestrict0 instead of the trailing stage of the
                                // pre-smoothing pass (k_sweep0r, TRAIL = 2)
    bool fuse_b = true;         // VOF_FUSE_B=0: the stand-alone kernels k_update_s / k_update_p instead of the vector update folded
                                // into the cycle's first pre-smoothing pass (k_sweep0r, BF = 1 / 2)
    int fused_ends = 3;         // VOF_FUSED_ENDS: bit 0 the batch prologue (b, x0, r0, r^), bit 1 the epilogue (residual norm, outputs,
                                // functionals) in one pass of k_stream_apply0 each; 0: the stand-alone kernels
    long sweep0r_min_blocks = 512;   // level 0, float64 vectors, even n_j: the register-resident pass k_sweep0r for launches of at least
                                     // this many one-wave blocks, the LDS-ring pass k_sweep0m below (VOF_SWEEP0R_MIN_BLOCKS; the tests set 0)
    int tail_first = -1;        // first level of the tail (-1: no tail for this grid)
    size_t tail_lds = 0;        // dynamic LDS bytes of k_tail_cycle
    TailArgs tail;              // levels / LDS layout; the operation list is rebuilt when the cycle parameters change
    int tail_key[6] = {-9, -9, -9, -9, -9, -9};   // cycle parameters the operation list was built for
    // profiler
    bool prof = false;
    int prof_kid = -1, prof_level = -1;  // filter (-1 = any)
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> free_events;
    long long prof_dropped = 0;
    double prof_ms[VOF_K_COUNT][16];
    long long prof_n[VOF_K_COUNT][16];
    long long prof_units[VOF_K_COUNT][16];
    double prof_bytes[VOF_K_COUNT][16];
    double prof_moved[VOF_K_COUNT][16];
    int cur_units = 0;  // frame pairs the next launches process (active pairs of the batch)
    // fault attribution (see the "debug switches" paragraph of include/vof.h)
    int dbg_sync = 0;            // VOF_DEBUG_SYNC=1: synchronise + check after every launch scope; the first failure names its kernel class
    long long dbg_seq = 0;       // launch scopes checked so far
    std::string dbg_fault;       // the first failure
    int dbg_fd = -1;             // VOF_DEBUG_SYNC_FILE: the scope in flight is written here before it is waited for (survives an abort)
    bool dbg_canary = false;     // VOF_DEBUG_CANARY=1: every device buffer sits between two guard pages of a known pattern
    bool dbg_alloc_log = false;  // VOF_DEBUG_ALLOC_LOG=1: base / size / name of every device buffer on stderr
    bool dbg_poison = false;     // VOF_DEBUG_POISON=1: every new device buffer is filled with 0xFF bytes (NaN as float / double, -1 as int)
    size_t part_per_pair = 0;    // doubles of `partials` per batch slot
    // lanes (solve_range_dev): a lane is a copy of the context whose per-pair buffers are views of the slots [lane_lo, lane_lo +
    // lane_slots) of the parent's, with a stream and batch events of its own (make_lane); it allocates nothing itself
    vof_ctx* lane_parent = nullptr;
    int lane_lo = 0, lane_slots = 0;
    int dir_ok = -1;             // lane: the parent's direct_ok_for_fallback, decided before the lanes start (-1: ask)
    hipStream_t lane_stream[MAX_LANES] = {};
    hipEvent_t lane_ev[MAX_LANES][2] = {};
    hipEvent_t ev_fork = nullptr;
    hipEvent_t group_ev[MAX_LANES * MAX_LANE_GROUPS] = {};   // two-phase solve: a group's phase-1 solutions are in warm_x
};

static std::string g_create_error;

namespace {

// VOF_DEBUG_SYNC: wait for the launches of the scope that has just ended and ask for their error, so that a fault is
// reported against the kernel class and level that caused it instead of at some later synchronising call.
void dbg_sync_check(vof_ctx* c, const char* what, int level) {
    if (!c->dbg_sync) return;
    ++c->dbg_seq;
    char line[256];
    if (c->dbg_fd >= 0) {
        int n = snprintf(line, sizeof line, "in flight: scope #%lld '%s' level %d, %d pairs, grid %dx%d (%d levels)%-40s\n", c->dbg_seq, what, level,
                         c->cur_units, c->Ni, c->Nj, (int)c->L.size(), "");
        if (pwrite(c->dbg_fd, line, (size_t)n, 0) < 0) { /* diagnostics only */ }
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    hipError_t e2 = hipGetLastError();
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess && c->dbg_fault.empty()) {
        snprintf(line, sizeof line, "VOF_DEBUG_SYNC: scope #%lld, kernel class '%s', level %d, %d pairs, image %dx%d: %s", c->dbg_seq, what, level,
                 c->cur_units, c->Ni, c->Nj, hipGetErrorString(e));
        c->dbg_fault = line;
        fprintf(stderr, "%s\n", line);
        fflush(stderr);
    }
}

struct Prof {
    vof_ctx* c;
    bool on;
    int dkid, dlevel;
    ProfRec rec;
    Prof(vof_ctx* c_, int kid, int level, double bytes_per_pair = 0.0, double moved_per_pair = -1.0) : c(c_), on(false), dkid(kid), dlevel(level) {
        if (!c->prof) return;
        if (c->prof_kid >= 0 && kid != c->prof_kid) return;
        if (c->prof_level >= 0 && level != c->prof_level) return;
        if ((int)c->recs.size() >= MAX_PROF_RECS) { c->prof_dropped++; return; }
        if (c->free_events.size() >= 2) {
            rec.e0 = c->free_events.back(); c->free_events.pop_back();
            rec.e1 = c->free_events.back(); c->free_events.pop_back();
        } else {
            if (hipEventCreate(&rec.e0) != hipSuccess || hipEventCreate(&rec.e1) != hipSuccess) return;
        }
        rec.kid = kid; rec.level = level < 0 ? 0 : (level > 15 ? 15 : level);
        rec.units = c->cur_units;
        rec.bytes = bytes_per_pair * c->cur_units;
        rec.moved = (moved_per_pair < 0.0 ? bytes_per_pair : moved_per_pair) * c->cur_units;
        on = true;
        hipEventRecord(rec.e0, c->stream);
    }
    ~Prof() {
        if (on) {
            hipEventRecord(rec.e1, c->stream);
            c->recs.push_back(rec);
        }
        if (c->dbg_sync) dbg_sync_check(c, vof_kernel_name(dkid), dlevel);
    }
};

void prof_collect(vof_ctx* c) {
    if (c->recs.empty()) return;
    hipStreamSynchronize(c->stream);
    for (auto& r : c->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            c->prof_ms[r.kid][r.level] += ms;
            c->prof_n[r.kid][r.level] += 1;
            c->prof_units[r.kid][r.level] += r.units;
            c->prof_bytes[r.kid][r.level] += r.bytes;
            c->prof_moved[r.kid][r.level] += r.moved;
        }
        c->free_events.push_back(r.e0);
        c->free_events.push_back(r.e1);
    }
    c->recs.clear();
}

#define HIPCHK(call)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            char buf_[512];                                                                        \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            c->err = buf_;                                                                         \
            if (!c->dbg_fault.empty()) c->err += " [" + c->dbg_fault + "]";                        \
            return -2;                                                                             \
        }                                                                                          \
    } while (0)

// Caller host memory (pageable) <-> device through a pinned bounce buffer on the context's stream: no null stream, and nothing
// for the runtime to pin on the fly.  Every copy of the debug entry points, the box flow and Liu-Shen host
// variants, the sweeps, the comparison, the frame-wise calls and the blur's taps - not the frames of vof_blur_stack_host (blur_stack).
constexpr size_t BOUNCE_BYTES = (size_t)8 << 20;
int d2h_bounced(vof_ctx* c, void* host, const void* dev, size_t bytes) {
    if (!c->h_bounce) HIPCHK(hipHostMalloc((void**)&c->h_bounce, BOUNCE_BYTES));
    for (size_t off = 0; off < bytes; off += BOUNCE_BYTES) {
        const size_t n = std::min(BOUNCE_BYTES, bytes - off);
        HIPCHK(hipMemcpyAsync(c->h_bounce, (const char*)dev + off, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        memcpy((char*)host + off, c->h_bounce, n);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
int h2d_bounced(vof_ctx* c, void* dev, const void* host, size_t bytes) {
    if (!c->h_bounce) HIPCHK(hipHostMalloc((void**)&c->h_bounce, BOUNCE_BYTES));
    for (size_t off = 0; off < bytes; off += BOUNCE_BYTES) {
        const size_t n = std::min(BOUNCE_BYTES, bytes - off);
        memcpy(c->h_bounce, (const char*)host + off, n);
        HIPCHK(hipMemcpyAsync((char*)dev + off, c->h_bounce, n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// A range of caller host memory registered (pinned in place) while the object lives; move-only.  Where the registration does
// not hold, copies from / to the range run as pageable ones.
class HostPin {
    void* p_ = nullptr;
public:
    HostPin() = default;
    HostPin(const void* p, size_t bytes) {
        if (hipHostRegister((void*)p, bytes, hipHostRegisterDefault) == hipSuccess) p_ = (void*)p;
        else (void)hipGetLastError();
    }
    HostPin(HostPin&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    HostPin& operator=(HostPin&& o) noexcept { std::swap(p_, o.p_); return *this; }
    ~HostPin() { release(); }
    bool ok() const { return p_ != nullptr; }
    void release() { if (p_) (void)hipHostUnregister(p_); p_ = nullptr; }   // (the return code is discarded, as it always was)
};

constexpr size_t DBG_GUARD = 4096;       // bytes of guard pattern on either side of a buffer (VOF_DEBUG_CANARY=1)
constexpr int DBG_GUARD_BYTE = 0xC5;

template <typename T>
int dev_alloc_named(vof_ctx* c, T** p, size_t n, const char* name, int line) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(n * sizeof(T), 256);
    if (c->dbg_canary) {
        HIPCHK(hipMalloc(&q, bytes + 2 * DBG_GUARD));
        HIPCHK(hipMemset(q, DBG_GUARD_BYTE, DBG_GUARD));
        HIPCHK(hipMemset((char*)q + DBG_GUARD + bytes, DBG_GUARD_BYTE, DBG_GUARD));
        c->allocs.push_back({q, (char*)q + DBG_GUARD, bytes, name, line});
        *p = (T*)((char*)q + DBG_GUARD);
    } else {
        HIPCHK(hipMalloc(&q, bytes));
        c->allocs.push_back({q, (char*)q, bytes, name, line});
        *p = (T*)q;
    }
    c->bytes += bytes;
    if (c->dbg_poison) HIPCHK(hipMemset(*p, 0xFF, bytes));
    if (c->dbg_alloc_log)
        fprintf(stderr, "vof alloc ctx=%p %s (vof.hip:%d) base=%p end=%p bytes=%zu\n", (void*)c, name, line, (void*)*p, (void*)((char*)*p + bytes), bytes);
    return 0;
}
#define dev_alloc(c, p, n) dev_alloc_named(c, p, n, #p, __LINE__)

// Releases one buffer of the context (a buffer that is re-allocated larger); nullptr is fine.
int dev_free(vof_ctx* c, void* user) {
    if (!user) return 0;
    for (size_t i = 0; i < c->allocs.size(); ++i)
        if ((void*)c->allocs[i].user == user) {
            HIPCHK(hipFree(c->allocs[i].raw));
            c->bytes -= c->allocs[i].bytes;
            c->allocs.erase(c->allocs.begin() + (long)i);
            return 0;
        }
    c->err = "internal: dev_free of a pointer the context does not own";
    return -1;
}

constexpr int DEFAULT_COARSE_PRECISION = 3;
inline int vof_params_default_coarse_precision() { return DEFAULT_COARSE_PRECISION; }
// bytes of stencil storage per point of a stored level in format `fmt` (vof_params.coarse_precision)
inline int coef_bytes_per_point(int fmt) { return fmt == 3 ? 30 * 4 : (fmt == 2 ? 45 * 4 : (fmt == 1 ? 81 * 4 : 81 * 8)); }

// Stencil storage of the levels >= 1 for format `fmt`: allocated for the default format by vof_create, re-allocated
// (never shrunk) when a call asks for a wider one.  Round 2 sized it for float64 whatever the format: 648 instead of 120
// bytes per coarse point, 45 % of the workspace never touched.
int ensure_stencil_storage(vof_ctx* c, int fmt) {
    const int need = coef_bytes_per_point(fmt);
    if (need <= c->c_bytes_per_point || c->L.size() < 2) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t l = 1; l < c->L.size(); ++l) {
        Level& lv = c->L[l];
        if (int rc = dev_free(c, lv.C)) return rc;
        lv.C = nullptr;
    }
    for (size_t l = 1; l < c->L.size(); ++l) {
        Level& lv = c->L[l];
        uint32_t* C = nullptr;
        if (int rc = dev_alloc(c, &C, (size_t)c->B * (need / 4) * CLay(lv.ni, lv.nj).plane)) return rc;
        lv.C = C;
    }
    c->c_bytes_per_point = need;
    c->frames = nullptr;   // a hierarchy built earlier is gone: the debug entry points ask for a new vof_debug_setup
    return 0;
}

// Buffers that depend on the parameters of the call (every entry point runs this through check_params).
int ensure_storage(vof_ctx* c) {
    if (int rc = ensure_stencil_storage(c, c->prm.coarse_precision)) return rc;
    if (c->vfloat && !c->b32)   // float32 copy of the cycle's right-hand side (vcycle_precision 1 / 2 only)
        if (int rc = dev_alloc(c, &c->b32, (size_t)c->B * 3 * c->L[0].npts)) return rc;
    return 0;
}

// Guard pages of every buffer of the context against their pattern; the number of damaged buffers, each named in `report`.
int dbg_check_canaries(vof_ctx* c, std::string* report) {
    int bad = 0;
    std::vector<unsigned char> h(2 * DBG_GUARD);
    if (!c->dbg_canary) return 0;
    for (const auto& a : c->allocs) {
        if (hipMemcpy(h.data(), a.raw, DBG_GUARD, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h.data() + DBG_GUARD, a.user + a.bytes, DBG_GUARD, hipMemcpyDeviceToHost) != hipSuccess) {
            if (report) *report += "guard pages unreadable; ";
            return -1;
        }
        long first_lo = -1, first_hi = -1;
        for (size_t i = 0; i < DBG_GUARD; ++i) if (h[DBG_GUARD - 1 - i] != DBG_GUARD_BYTE) { first_lo = (long)i + 1; break; }   // bytes BELOW the buffer
        for (size_t i = 0; i < DBG_GUARD; ++i) if (h[DBG_GUARD + i] != DBG_GUARD_BYTE) { first_hi = (long)i; break; }            // bytes PAST its end
        if (first_lo >= 0 || first_hi >= 0) {
            ++bad;
            char line[256];
            snprintf(line, sizeof line, "buffer %s (vof.hip:%d, %zu bytes at %p): written %s%ld bytes %s; ", a.name, a.line, a.bytes, (void*)a.user,
                     first_hi >= 0 ? "" : "-", first_hi >= 0 ? first_hi : first_lo, first_hi >= 0 ? "past its end" : "before its start");
            if (report) *report += line;
        }
    }
    return bad;
}

// ---- which pairs a launch covers (ActiveSet, vof_device.hpp)
const ActiveSet ALL_PAIRS{nullptr, nullptr};   // every slot of the batch, no flags: set-up, epilogue, debug entry points
// `flags` with the context's list.  Only for flags that are on for no pair outside the list: c->active after post_active_list,
// and the GMRES cycle flags between two of its restarts (gmres_phase)
inline ActiveSet listed(const vof_ctx* c, const int* flags) { return ActiveSet{flags, c->use_alist ? c->alist : nullptr}; }
// entries of the pair dimension of a launch that is given `a`
inline int pair_slots(const vof_ctx* c, const ActiveSet& a, int np) { return a.list ? c->alist_n : np; }

inline dim3 grid2d(int ni, int nj, int z) { return dim3((nj + BX - 1) / BX, (ni + BY - 1) / BY, z); }
inline dim3 grid2d_colour(int ni, int nj, int colour, int z) {
    int cp = colour >> 1, cq = colour & 1;
    int mi = (ni - cp + 1) / 2, mj = (nj - cq + 1) / 2;
    return dim3(std::max(1, (mj + BX - 1) / BX), std::max(1, (mi + BY - 1) / BY), z);
}
const dim3 blk2d(BX, BY, 1);

inline size_t frame_stride(const vof_ctx* c) { return (size_t)c->Ni * c->Nj; }

// ---------------------------------------------------------------- level kernels
// VT = storage type of the V-cycle vectors (float when ctx->vfloat, else double).
#define VDISPATCH(c, ...)                                   \
    do {                                                    \
        if ((c)->vfloat) { using VT = float; __VA_ARGS__; } \
        else { using VT = double; __VA_ARGS__; }            \
    } while (0)

// ... for the kernels that read the cycle's results y, z (float32 also under h32)
#define YDISPATCH(c, ...)                                                  \
    do {                                                                   \
        if ((c)->vfloat || (c)->h32) { using VT = float; __VA_ARGS__; }    \
        else { using VT = double; __VA_ARGS__; }                           \
    } while (0)

template <typename T> struct TypeTag { typedef T type; };
// CT = storage format of the stored stencil of level l (word type CW)
#define CDISPATCH(c, l, ...)                                                                        \
    do {                                                                                            \
        const int cf_ = ((l) > 0) ? (c)->cfmt : 0;                                                  \
        if (cf_ == 2) { using CT = CoefB16; using CW = uint32_t; __VA_ARGS__; }                     \
        else if (cf_ == 3) { using CT = CoefF8; using CW = uint32_t; __VA_ARGS__; }                 \
        else if (cf_ == 1) { using CT = float; using CW = float; __VA_ARGS__; }                     \
        else { using CT = double; using CW = double; __VA_ARGS__; }                                 \
    } while (0)
inline double coef_bytes(const vof_ctx* c, int l) { const int f = l > 0 ? c->cfmt : 0; return f == 3 ? 30.0 * 4 : (f == 2 ? 45.0 * 4 : (f == 1 ? 81.0 * 4 : 81.0 * 8)); }

// one colour, in place, one launch per colour: the simple reference smoother (double vectors only)
void gs_colour(vof_ctx* c, int l, double* x, const double* b, int colour, int np, ActiveSet active) {
    Level& lv = c->L[l];
    dim3 g = grid2d_colour(lv.ni, lv.nj, colour, pair_slots(c, active, np));
    if (l == 0 && c->L.size() > 1) {
        Prof p(c, VOF_K_GS0, 0, 20.0 * lv.npts);
        k_gs0<<<g, blk2d, 0, c->stream>>>(c->frames, frame_stride(c), c->Nj, lv.ni, lv.nj, c->prm.speed_alpha,
                                          c->prm.remodelling_alpha, c->prm.reference_quirks, x, b, colour, active, c->pp);
    } else {
        Prof p(c, VOF_K_GS, l, (coef_bytes(c, l) + 72.0) / 4.0 * lv.npts);
        CDISPATCH(c, l, (k_gs<CT><<<g, blk2d, 0, c->stream>>>((const CW*)lv.C, lv.ni, lv.nj, x, b, colour, active)));
    }
}

// y = A_l x (mode 0) or y = b - A_l x (mode 1); XT/BT/YT storage types (level 0 matrix-free),
// stored levels use one type for all three.
// Band height of the row-streaming kernels: bands of <= 128 rows (balanced, even).  A block marches through its band
// sequentially, so a launch lasts at least (band height / 2 + pipeline depth) steps; when only a few pairs are still
// active (the tail iterations of a batch, or a small stack) the grid does not fill the 256 CUs and shorter bands
// (more, shorter blocks) cut that latency floor.
int pick_band_height(int rows, int nx, int units) {
    const long blocks128 = (long)nx * ((rows + 127) / 128) * std::max(1, units);
    const int cap = blocks128 < 768 ? 32 : (blocks128 < 1536 ? 64 : 128);   // 768 = 3 blocks per CU
    const int nb = (rows + cap - 1) / cap;
    return std::max(2, (((rows + nb - 1) / nb + 1) / 2) * 2);
}

// Geometry of the streaming level-0 operator kernel: 128-column strips, bands of <= 128 rows (even height).
struct ApplyGrid { int TI, nblk; dim3 grid; };
ApplyGrid apply_grid(const vof_ctx* c, int np) {
    const Level& lv = c->L[0];
    int TI = pick_band_height(lv.ni, (lv.nj + AP_OUT - 1) / AP_OUT, c->cur_units);
    ApplyGrid g;
    g.TI = TI;
    g.grid = dim3((lv.nj + AP_OUT - 1) / AP_OUT, (lv.ni + TI - 1) / TI, np);
    g.nblk = g.grid.x * g.grid.y;
    return g;
}
// What both streaming level-0 kernels are given first: frames, level-0 grid, band height TI, model parameters, pair tables.
ApArgs ap_args(const vof_ctx* c, int TI, ActiveSet active) {
    const Level& lv = c->L[0];
    return ApArgs{c->frames, frame_stride(c), c->Nj, lv.ni, lv.nj, TI, c->prm.speed_alpha, c->prm.remodelling_alpha,
                  c->prm.reference_quirks, active, c->pp};
}

// y = A x (mode 0) or y = b - A x (mode 1) on the matrix-free level 0.  Optional fused reductions into
// c->partials (slot 0: y.dotvec, or y.y when dotvec == nullptr; slot 1: y.y when both are asked for); the
// number of per-pair partials is apply_grid().nblk.
template <typename XT, typename BT, typename YT>
void apply_fine_t(vof_ctx* c, const XT* x, const BT* b, YT* y, int mode, int np, ActiveSet active,
                  const double* dotvec = nullptr, int want_yy = 0, YT* ycopy = nullptr) {
    Level& lv = c->L[0];
    const double bytes = (8.0 + 3.0 * sizeof(XT) + ((y ? 3.0 : 0.0) + (ycopy ? 3.0 : 0.0)) * sizeof(YT) + (mode ? 3.0 * sizeof(BT) : 0.0) +
                          (dotvec ? 24.0 : 0.0)) * lv.npts;
    Prof p(c, VOF_K_APPLY0, 0, bytes);
    ApplyGrid ag = apply_grid(c, pair_slots(c, active, np));
    double* part = (dotvec || want_yy) ? c->partials : nullptr;
    const ApArgs a = ap_args(c, ag.TI, active);
    if (mode)
        k_stream_apply0<1, XT, BT, YT><<<ag.grid, AP_THREADS, 0, c->stream>>>(a, x, b, y, dotvec, want_yy, part, ag.nblk, ycopy, ApEnds{});
    else
        k_stream_apply0<0, XT, BT, YT><<<ag.grid, AP_THREADS, 0, c->stream>>>(a, x, b, y, dotvec, want_yy, part, ag.nblk, ycopy, ApEnds{});
}

template <typename VT>
void apply_stored_t(vof_ctx* c, int l, const VT* x, const VT* b, VT* y, int mode, int np, ActiveSet active) {
    Level& lv = c->L[l];
    dim3 g = grid2d(lv.ni, lv.nj, pair_slots(c, active, np));
    Prof p(c, VOF_K_RESIDUAL, l, (coef_bytes(c, l) + (mode ? 9.0 : 6.0) * sizeof(VT)) * lv.npts);
    if (mode) CDISPATCH(c, l, (k_apply<CT, 1, VT><<<g, blk2d, 0, c->stream>>>((const CW*)lv.C, lv.ni, lv.nj, x, b, y, active)));
    else CDISPATCH(c, l, (k_apply<CT, 0, VT><<<g, blk2d, 0, c->stream>>>((const CW*)lv.C, lv.ni, lv.nj, x, b, y, active)));
}

// V-cycle internal operator application on level l (all vectors VT)
template <typename VT>
void apply_level_t(vof_ctx* c, int l, const VT* x, const VT* b, VT* y, int mode, int np, ActiveSet active) {
    if (l == 0 && c->L[0].C == nullptr) apply_fine_t<VT, VT, VT>(c, x, b, y, mode, np, active);
    else apply_stored_t<VT>(c, l, x, b, y, mode, np, active);
}

// Krylov-level products on level 0 with FP64 results: out = A y (y V-typed) and out = b - A x (all double).
// On the matrix-free level 0 the reductions asked for (out.dotvec and/or out.out) are fused into the operator kernel
// and the function returns the number of per-pair partials it wrote; otherwise 0 (the caller then launches k_dot2).
int krylov_apply(vof_ctx* c, const void* y, double* out, int np, ActiveSet active, const double* dotvec = nullptr,
                 int want_yy = 0) {
    if (c->L[0].C) { apply_stored_t<double>(c, 0, (const double*)y, nullptr, out, 0, np, active); return 0; }
    if (c->vfloat || c->h32) apply_fine_t<float, double, double>(c, (const float*)y, nullptr, out, 0, np, active, dotvec, want_yy);
    else apply_fine_t<double, double, double>(c, (const double*)y, nullptr, out, 0, np, active, dotvec, want_yy);
    return (dotvec || want_yy) ? apply_grid(c, np).nblk : 0;
}
// (out == nullptr with want_norm: only the norm is wanted - the streaming kernel then writes nothing; returns 0 if that is
// not possible, and the caller falls back to a residual vector)
// out2 (streaming kernel only, see residual_copy_ok): a second copy of the residual
inline bool residual_copy_ok(const vof_ctx* c) { return !c->L[0].C; }
int residual_d(vof_ctx* c, const double* x, const double* b, double* out, int np, ActiveSet active, int want_norm = 0,
               double* out2 = nullptr) {
    if (!out && !(want_norm && !c->L[0].C)) return 0;
    if (c->L[0].C) { apply_stored_t<double>(c, 0, x, b, out, 1, np, active); return 0; }
    apply_fine_t<double, double, double>(c, x, b, out, 1, np, active, nullptr, want_norm ? 1 : 0, out2);
    return want_norm ? apply_grid(c, np).nblk : 0;
}

// The two ends of a batch on the matrix-free level 0, one pass each (k_stream_apply0, MODE 2 and 3; VOF_FUSED_ENDS).  Both
// return the number of per-pair block partials they wrote.
// Prologue of a batch that does not start from zero: b, x0 (the saved solution src[pair], or the constants where src[pair] < 0 or
// src == nullptr), r0 = b - A x0 and r^ = r0, with the partials of (b, b) in slot 0 and of (r0, r0) in slot 1 of c->partials.
int fused_prologue(vof_ctx* c, const int* src, double c0, double c1, double c2, int np) {
    Level& lv = c->L[0];
    // algorithmic: k_rhs_norm (16 + 24), k_gather_guess (24 + 24; k_fill 24) and the residual pass (8 + 24 + 24 + 24 + 24)
    Prof p(c, VOF_K_RHS, 0, (src ? 192.0 : 168.0) * lv.npts, (src ? 136.0 : 112.0) * lv.npts);
    ApplyGrid ag = apply_grid(c, np);
    ApEnds e{};
    e.saved = c->warm_x; e.src = src; e.c0 = c0; e.c1 = c1; e.c2 = c2; e.xo = c->kx; e.bo = c->kb;
    k_stream_apply0<2, double, double, double><<<ag.grid, AP_THREADS, 0, c->stream>>>(
        ap_args(c, ag.TI, ALL_PAIRS), nullptr, nullptr, c->kr, nullptr, 0, c->partials, ag.nblk, c->krh, e);
    return ag.nblk;
}
// Epilogue: the norm of the independent residual b - A x (slot 0 of c->partials) and, from the same rows of x, the outputs and
// the partials of the three functionals (`fpart`, [pair][3][nblk]).
int fused_epilogue(vof_ctx* c, double* vx, double* vy, double* gm, double* speed, double* fpart, int np) {
    Level& lv = c->L[0];
    const double out = speed ? 32.0 : 24.0;
    // algorithmic: the norm-only residual pass (8 + 24 + 24) and k_finalize_functionals (24 + 16 + outputs)
    Prof p(c, VOF_K_FINALIZE, 0, (96.0 + out) * lv.npts, (64.0 + out) * lv.npts);
    ApplyGrid ag = apply_grid(c, np);
    ApEnds e{};
    e.vscale = c->prm.delta_x / c->prm.delta_t; e.vx = vx; e.vy = vy; e.gm = gm; e.speed = speed; e.fpartials = fpart;
    k_stream_apply0<3, double, double, double><<<ag.grid, AP_THREADS, 0, c->stream>>>(
        ap_args(c, ag.TI, ALL_PAIRS), c->kx, c->kb, nullptr, nullptr, 1, c->partials, ag.nblk, nullptr, e);
    return ag.nblk;
}

template <typename VT>
void restrict_level_t(vof_ctx* c, int l, const VT* fine, VT* coarse, int np, ActiveSet active) {
    Level &f = c->L[l], &k = c->L[l + 1];
    Prof p(c, VOF_K_RESTRICT, l, 3.0 * sizeof(VT) * (f.npts + k.npts));
    k_restrict<VT><<<grid2d(k.ni, k.nj, pair_slots(c, active, np)), blk2d, 0, c->stream>>>(fine, f.ni, f.nj, coarse, k.ni, k.nj, active);
}

// level 0, matrix-free: coarse right-hand side b_1 = R (b - A x) in one pass (no fine residual in HBM)
template <typename VT, typename CVT = VT>
void resrestrict_fine_t(vof_ctx* c, const VT* x, const VT* b, CVT* bc, int np, ActiveSet active) {
    Level &f = c->L[0], &k = c->L[1];
    int TI = pick_band_height(f.ni, (k.nj + RR_CO - 1) / RR_CO, c->cur_units);
    dim3 g((k.nj + RR_CO - 1) / RR_CO, (k.ni + TI / 2 - 1) / (TI / 2), pair_slots(c, active, np));
    Prof p(c, VOF_K_APPLY0, 0, (8.0 + 6.0 * sizeof(VT)) * f.npts + 3.0 * sizeof(CVT) * k.npts);
    k_stream_resrestrict0<VT, VT, CVT><<<g, AP_THREADS, 0, c->stream>>>(ap_args(c, TI, active), x, b, bc, k.ni, k.nj);
}

// stored level l >= 1, straight after ONE forward Gauss-Seidel sweep x_old -> x_new (x_old == nullptr: from zero): the coarse
// right-hand side b_{l+1} = R (b - A x_new) from the sweep's update alone (k_resrestrict_u) - no b, no diagonal blocks, half
// of the off-diagonal coefficients, no residual vector in HBM
inline double resu_coef_bytes(const vof_ctx* c) {   // average per fine point: 8 + 6 + 2 + 0 neighbour blocks over the four colours
    return c->cfmt == 3 ? 12.0 * 4 : (c->cfmt == 2 ? 18.5 * 4 : (c->cfmt == 1 ? 36.0 * 4 : 36.0 * 8));
}
template <typename VT>
void resrestrict_u_t(vof_ctx* c, int l, const VT* x_new, const VT* x_old, VT* bc, int np, ActiveSet active) {
    Level &f = c->L[l], &k = c->L[l + 1];
    const double vs = sizeof(VT);
    // algorithmic: the residual and the restriction it performs (as apply_stored_t + restrict_level_t count them)
    const double algo = (coef_bytes(c, l) + 9.0 * vs) * f.npts + 3.0 * vs * (f.npts + k.npts);
    const double moved = (resu_coef_bytes(c) + (x_old ? 6.0 : 3.0) * vs) * f.npts + 3.0 * vs * k.npts;
    Prof p(c, VOF_K_RESIDUAL, l, algo, moved);
    dim3 g(1, (k.ni + BY - 1) / BY, pair_slots(c, active, np));
    CDISPATCH(c, l, {
        if (x_old) k_resrestrict_u<CT, VT, true><<<g, blk2d, 0, c->stream>>>((const CW*)f.C, f.ni, f.nj, x_new, x_old, bc, k.ni, k.nj, active);
        else k_resrestrict_u<CT, VT, false><<<g, blk2d, 0, c->stream>>>((const CW*)f.C, f.ni, f.nj, x_new, x_old, bc, k.ni, k.nj, active);
    });
}

template <typename VT>
void prolong_add_level_t(vof_ctx* c, int l, VT* fine, const VT* coarse, int np, ActiveSet active) {
    Level &f = c->L[l], &k = c->L[l + 1];
    Prof p(c, VOF_K_PROLONG, l, 3.0 * sizeof(VT) * (2 * f.npts + k.npts));
    k_prolong_add<VT><<<grid2d(f.ni, f.nj, pair_slots(c, active, np)), blk2d, 0, c->stream>>>(fine, f.ni, f.nj, coarse, k.ni, k.nj, active);
}

template <typename VT>
void coarse_solve_t(vof_ctx* c, const VT* r, VT* e, int np, ActiveSet active) {
    Prof p(c, VOF_K_COARSE_SOLVE, (int)c->L.size() - 1);
    k_coarse_solve<VT><<<pair_slots(c, active, np), 256, c->nd * sizeof(double), c->stream>>>(c->invT, c->nd, r, e, active);
}

// k_sweep0m (merged colours, 16-byte accesses, up to two sweeps per pass) needs float64 vectors and an even row length
inline bool sweep0m_usable(const vof_ctx* c) {
    return c->fused && !c->vfloat && (c->L[0].nj % 2 == 0) && c->L[0].C == nullptr;
}

// k_sweep0p (float32 cycle vectors: packed float32 arithmetic, two strips per wave, up to two sweeps per pass)
inline bool sweep0p_usable(const vof_ctx* c) {
    return c->fused && c->vfloat && (c->L[0].nj % 2 == 0) && c->L[0].C == nullptr && c->prm.reference_quirks;
}

// k_sweep_st: stored levels with packed bfloat16 stencils and the 128-column strip geometry
inline bool sweep_st_usable(const vof_ctx* c, int l) {
    return l > 0 && c->L[l].C != nullptr && c->cfmt >= 2;
}

// k_sweep_st2: the post-smoothing of one visit of level l and the pre-smoothing of the next in one pass.  A regular stored level
// (packed stencils, neither the coarsest level nor the top of the coarse tail) that smooths once before and once after its
// coarse-grid correction.  (With VOF_FOLD_STORED the first post-sweep interpolates the correction, which k_sweep_st2 does not.)
bool tail_prepare(vof_ctx* c);
inline bool revisit_fusable(vof_ctx* c, int l) {
    if (!c->fused || !c->fuse_revisit || c->fold_stored || !sweep_st_usable(c, l) || l >= (int)c->L.size() - 1) return false;
    if (l == c->tail_first && tail_prepare(c)) return false;
    const int nu1 = c->prm.nu_pre_coarse > 0 ? c->prm.nu_pre_coarse : c->prm.nu_pre;
    const int nu2 = c->prm.nu_post_coarse > 0 ? c->prm.nu_post_coarse : c->prm.nu_post;
    return nu1 == 1 && nu2 == 1;
}

// vcycle_precision 3 applies when level 0 runs the kernels in which the two storage types meet: the residual + restriction
// (float64 in, float32 out) and the k_sweep0m / k_sweep0r pass with the interpolated correction (float32 in); anything else
// keeps float64 everywhere
inline bool coarse32_ok(const vof_ctx* c, int nu_post) {
    return c->vcoarse32 && c->L.size() > 1 && sweep0m_usable(c) && nu_post > 0;
}

// ---- level-0 smoothing passes: what a caller wants (L0Req), what is launched for it (L0Pass), decided in plan_l0_pass

// Requests to and results of one multigrid cycle that concern its level-0 passes.  The Krylov loop (or a debug entry point)
// fills in the inputs, hands the struct down vcycle -> vcycle_t -> smooth_level_t -> sweep_level_t and reads the outputs.
struct CycleIO {
    // in: the Krylov product v = A y of the cycle's result, wanted from its last smoothing pass (trail.v == nullptr: not wanted)
    S0Trail trail{nullptr, nullptr, 0, nullptr};
    // in: the BiCGStab vector update that forms the cycle's right-hand side, to be folded into the first pre-smoothing pass.
    // bf_mode 0: none; 1: s = r - alpha v (+ (s, s), half-step test); 2: p = r + beta (p_old - omega v)
    S0BSrc bf{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int bf_mode = 0;
    // out
    int trail_nblk = 0;      // per-pair partial sums the fused product wrote (0: not fused, the caller launches the operator)
    bool rr_done = false;    // the last pre-smoothing pass of level 0 wrote the coarse right-hand side (read by vcycle_t)
    bool bf_done = false;    // the folded vector update was performed
    bool failed = false;     // c->err says why; nothing the cycle wrote may be used
};

struct L0Req {
    bool from_zero = false;                    // start from a zero guess instead of x_in
    int po = 0;                                // direction: 1 = reverse (colours 3,2,1,0)
    int nsweeps = 1;                           // sweeps wanted from the pass (1 or 2)
    bool ec = false, ec32 = false;             // start from x_in + P ecoarse; ecoarse is float32 data
    bool trail = false, trail_dot = false;     // the Krylov product of the result is wanted; it has a dot partner
    bool rr = false, rr_f32 = false;           // the coarse right-hand side R (b - A x_out) is wanted; as float32
    int bf = 0;                                // folded vector update wanted (CycleIO::bf_mode)
    bool x32 = false;                          // x_in / x_out are float32 hand-off vectors (c->h32)
};

enum L0Family { L0_SWEEP0R, L0_SWEEP0M, L0_SWEEP0P, L0_SWEEP0 };

struct L0Pass {
    L0Family fam = L0_SWEEP0;
    // the family's template arguments (those it has)
    int NS = 1;                  // sweeps per pass
    bool EC = false, FROM_ZERO = false;
    int TRAIL = 0;               // 1: Krylov product, 2: residual + restriction
    bool ET32 = false;           // ET: float32 coarse data (the correction read, or the coarse right-hand side written)
    int PO = 0;
    int BF = 0;                  // 1 / 2: folded vector update; 3: b read once and carried in registers
    bool XT32 = false;           // XT: float32 x_in / x_out
    // launch
    int nx = 0, nxp = 0, ny = 0, TI = 0, nci = 0, ncj = 0;
    unsigned blocks = 0, block = 0;   // blocks per pair (the grid is blocks x pairs), threads per block
    size_t lds = 0;
    double algo = 0.0, moved = 0.0;   // profiler: algorithmic / minimal bytes per pair
    // requests honoured
    bool trail() const { return TRAIL == 1; }
    bool rr() const { return TRAIL == 2; }
    int bf() const { return BF == 3 ? 0 : BF; }
};

// Strips and bands of a level-0 pass of k_sweep0m / k_sweep0r (NSW sweeps per pass) and whether the register-resident kernel takes it
struct S0Geo { int nx, ny, TI; bool s0r; };
inline S0Geo s0_geometry(const vof_ctx* c, int rows, int NSW, bool trail) {
    const Level& lv = c->L[0];
    S0Geo g;
    const int out = S0_W - 8 * NSW - (trail ? 4 : 0);
    g.nx = (lv.nj + out - 1) / out;
    g.TI = pick_band_height(rows, g.nx, c->cur_units);
    g.ny = (rows + g.TI - 1) / g.TI;
    // (the register-resident pass is compiled with the reference's derivative quirk built in; one wave per block needs a few
    // waves per SIMD-slot to fill the chip: tiny stacks - 128 x 128 x 8: 14 blocks - stay with the 4-wave LDS pass)
    g.s0r = c->prm.reference_quirks && (long)g.nx * g.ny * std::max(1, c->cur_units) >= c->sweep0r_min_blocks;
    return g;
}

// k_sweep0r from zero: the two-sweep pass reads b once and hands it on in registers (vof_sweep0r.hpp)
constexpr int s0r_bf_from_zero(int ns) { return (VOF_S0R_BCARRY && ns == 2) ? 3 : 0; }
inline size_t s0r_lds(int ns, int trail) {
    if (ns == 2) return trail == 2 ? S0R<2, 2>::LDS_TOTAL : (trail == 1 ? S0R<2, 1>::LDS_TOTAL : S0R<2, 0>::LDS_TOTAL);
    return trail == 1 ? S0R<1, 1>::LDS_TOTAL : S0R<1, 0>::LDS_TOTAL;
}

// The pass the matrix-free level 0 runs for `rq` with cycle vectors of type VT.  Reads the context, launches and writes nothing.
template <typename VT>
L0Pass plan_l0_pass(const vof_ctx* c, const L0Req& rq) {
    const Level& lv = c->L[0];
    const double npts = (double)lv.npts, npc = c->L.size() > 1 ? (double)c->L[1].npts : 0.0;
    const int rows = lv.ni + rq.po;
    L0Pass p;
    p.NS = rq.nsweeps >= 2 ? 2 : 1;
    p.EC = rq.ec;
    p.FROM_ZERO = rq.from_zero && !rq.ec;
    p.PO = rq.po;
    if (rq.ec) { p.nci = c->L[1].ni; p.ncj = c->L[1].nj; }
    if (std::is_same<VT, double>::value && sweep0m_usable(c)) {
        // merged colours, 16-byte accesses, one or two sweeps per pass; strips are not shifted by po.  k_sweep0r: registers;
        // k_sweep0m: LDS ring
        const bool trail = rq.trail && !rq.from_zero;
        // the coarse right-hand side as the trailing stage of the two-sweep pass from zero (k_sweep0r only)
        const bool rr = rq.rr && c->fuse_rr && rq.from_zero && p.NS == 2 && !rq.po && !rq.ec && VOF_S0R_BCARRY &&
                        s0_geometry(c, rows, 2, true).s0r;
        const S0Geo geo = s0_geometry(c, rows, p.NS, trail || rr);
        // the vector update that forms b: the same pass, whether or not it also forms the coarse right-hand side
        const int bf = (rq.bf && c->fuse_b && geo.s0r && rq.from_zero && p.NS == 2 && !rq.po && !rq.ec) ? rq.bf : 0;
        p.fam = geo.s0r ? L0_SWEEP0R : L0_SWEEP0M;
        p.nx = p.nxp = geo.nx; p.ny = geo.ny; p.TI = geo.TI;
        p.TRAIL = rr ? 2 : (trail ? 1 : 0);
        p.ET32 = rr ? rq.rr_f32 : (rq.ec && rq.ec32);
        p.BF = bf ? bf : ((geo.s0r && p.FROM_ZERO) ? s0r_bf_from_zero(p.NS) : 0);
        // float32 hand-off: the pass from zero that writes the float32 coarse right-hand side, and the post-smoothing pass
        p.XT32 = rq.x32 && geo.s0r && p.NS == 2 && (rr ? rq.rr_f32 : (rq.po && !rq.from_zero && rq.ec));
        if (rr || bf) { p.nci = c->L[1].ni; p.ncj = c->L[1].nj; }
        const double xs = p.XT32 ? 4.0 : 8.0;
        const double cb = rr ? (rq.rr_f32 ? 12.0 : 24.0) * npc : 0.0;
        if (bf) {   // I + r(3) + v(3) (+ p_old(3)) in, x(3) + b(3) out (+ the coarse right-hand side)
            p.moved = (8.0 + (bf == 2 ? 12.0 : 9.0) * 8.0 + 3.0 * xs) * npts + cb;
            p.algo = p.moved + 80.0 * npts + (rr ? 56.0 * npts : 0.0);
        } else {
            // bytes the pass moves: I + b(3) + x(3) in, x(3) out (+ coarse e), whatever the number of fused sweeps; algorithmic
            // bytes (80 per sweep performed): the second sweep of a double pass counts as a full sweep
            p.moved = (8.0 + 24.0 + (rq.from_zero ? 3.0 : 6.0) * xs) * npts + (rq.ec ? (rq.ec32 ? 12.0 : 24.0) * npc : 0.0);
            p.algo = p.moved + (p.NS - 1) * 80.0 * npts;
            if (trail) {   // + the operator product v = A x_out with its dot products: algorithmic 56 (+24 for the dot partner)
                const double dv = rq.trail_dot ? 24.0 : 0.0;
                p.algo += (56.0 + dv) * npts;
                p.moved += (24.0 + dv) * npts;     // only v out and the dot partner in: x_out and the image are in LDS
            }
            if (rr) {   // + the coarse right-hand side out (x_out, b and the image are in registers / LDS); algorithmic: the 56 B
                        // per pixel the stand-alone residual + restriction kernel reads
                p.algo += 56.0 * npts + cb;
                p.moved += cb;
            }
        }
        if (geo.s0r) { p.block = 64; p.lds = s0r_lds(p.NS, p.TRAIL); }
        else { p.block = 128 * p.NS; p.lds = (size_t)(6 * p.NS + 2 + (trail ? 4 : 0)) * s0_row_bytes(8) + (rq.ec ? (size_t)9 * (S0_W / 2 + 2) * 8 : 0); }
    } else if (std::is_same<VT, float>::value && sweep0p_usable(c)) {
        // k_sweep0p: packed float32 arithmetic, two strips per wave, one or two sweeps per pass
        const int out = S0_W - 8 * p.NS;
        p.fam = L0_SWEEP0P;
        p.nx = (lv.nj + out - 1) / out; p.nxp = (p.nx + 1) / 2;
        p.TI = pick_band_height(rows, p.nxp, c->cur_units);
        p.ny = (rows + p.TI - 1) / p.TI;
        p.moved = (8.0 + (rq.from_zero ? 6.0 : 9.0) * 4.0) * npts + (rq.ec ? 12.0 * npc : 0.0);   // I + b(3) + x(3) in, x(3) out, float32 vectors
        p.algo = p.moved + (p.NS - 1) * 44.0 * npts;
        p.block = 64; p.lds = p.NS == 2 ? S0R<2, 0>::LDS_BYTES : S0R<1, 0>::LDS_BYTES;
    } else {
        // k_sweep0: one sweep per pass, strips of 120 owned columns, shifted by the pass's direction
        const double vs = sizeof(VT);
        p.fam = L0_SWEEP0;
        p.NS = 1;
        p.nx = p.nxp = (lv.nj + rq.po + S0_OUT - 1) / S0_OUT;
        p.TI = pick_band_height(rows, p.nx, c->cur_units);
        p.ny = (rows + p.TI - 1) / p.TI;
        p.algo = p.moved = (8.0 + (rq.from_zero ? 6.0 : 9.0) * vs) * npts + (rq.ec ? 3.0 * vs * npc : 0.0);   // I + b(3) + x(3) in, x(3) out (+ coarse e)
        p.block = S0_THREADS;
        p.lds = (size_t)(SW_RING * 3 * S0_W) * sizeof(VT) + (size_t)(SW_RING * S0_IW) * sizeof(double) +
                (rq.ec ? (size_t)(3 * 3 * (S0_W / 2 + 2)) * sizeof(VT) : 0);
    }
    p.blocks = (unsigned)p.nxp * p.ny;
    return p;
}

// The level-0 passes of the cycle the current parameters describe, as vcycle_t -> smooth_level_t will request them
inline L0Req l0_pre_request(const vof_ctx* c, int bf) {    // first pre-smoothing pass
    L0Req rq;
    rq.from_zero = true;
    rq.nsweeps = std::min(2, c->prm.nu_pre);
    rq.rr = c->prm.nu_pre <= 2;   // (it is also the last one)
    rq.rr_f32 = coarse32_ok(c, c->prm.nu_post);
    rq.bf = bf;
    return rq;
}
inline L0Req l0_post_request(const vof_ctx* c, bool trail) {   // post-smoothing in one pass (nu_post 2)
    L0Req rq;
    rq.po = 1; rq.nsweeps = 2; rq.ec = true;   // (the correction's storage type does not change the choice)
    rq.trail = rq.trail_dot = trail;
    return rq;
}

// Will the next cycle start with a level-0 pass that takes the vector update forming its right-hand side?
inline bool fold_b_usable(const vof_ctx* c) {
    return !c->direct_on && c->L.size() > 1 && c->tail_first != 0 && c->prm.nu_pre >= 2 &&
           plan_l0_pass<double>(c, l0_pre_request(c, 1)).bf() == 1;
}

// vcycle_precision 3: the level-0 hand-off vectors - the pre-smoothed iterate x and the cycle's result y / z - are stored as
// float32 (h32) when every level-0 pass of the cycle can store them: one pre-smoothing pass from zero that forms the float32
// coarse right-hand side (nu_pre 2) and one post-smoothing pass that interpolates the correction (nu_post 2)
inline bool handoff32_ok(const vof_ctx* c) {
    const vof_params& P = c->prm;
    if (!(c->l0_handoff && P.nu_pre == 2 && P.nu_post == 2 && coarse32_ok(c, P.nu_post))) return false;
    L0Req pre = l0_pre_request(c, 0), post = l0_post_request(c, false), post_trail = l0_post_request(c, true);
    pre.x32 = post.x32 = post_trail.x32 = true;
    return plan_l0_pass<double>(c, pre).XT32 && plan_l0_pass<double>(c, post).XT32 && plan_l0_pass<double>(c, post_trail).XT32;
}

// ---- one launcher per kernel family.  A row names one instantiation and launches it if the plan asks for exactly that one;
// the rows are the kernels the library contains (a plan that matches no row is an error, not a reason to instantiate more):
//
//   family     rows  template arguments
//   k_sweep0r   28   <NS 1|2, EC, FROM_ZERO, TRAIL, ET, PO 0|1, 1, BF, double>, for each NS x PO the seven shapes
//                      (EC, FROM_ZERO, TRAIL, ET) = (1,0,1,float) (1,0,0,float) (1,0,1,double) (0,0,1,double) (1,0,0,double)
//                      (0,1,0,double; BF = 3 for NS 2, else 0) (0,0,0,double)
//                3   <2, 0, 1, 2, ET, 0, 1, 3, XT>       (ET, XT) = (float,float) (float,double) (double,double): + coarse rhs
//                8   <2, 0, 1, TRAIL, ET, 0, 1, BF 1|2, XT>  (TRAIL, ET, XT) = the three above with TRAIL 2, and (0,double,double)
//                4   <2, 1, 0, TRAIL 0|1, ET float|double, 1, 1, 0, float>   float32 hand-off, post-smoothing
//   k_sweep0m   14   <NS 1|2, EC, FROM_ZERO, TRAIL, ET>, the same seven shapes
//   k_sweep0p   12   <NS 1|2, EC, FROM_ZERO, PO 0|1>, (EC, FROM_ZERO) = (1,0) (0,1) (0,0)
//   k_sweep0     6   <VT double|float, EC, FROM_ZERO>, (EC, FROM_ZERO) = (1,0) (0,1) (0,0)
struct L0Ptrs {
    const void* x_in; void* x_out; const void* b; ActiveSet active; const void* ecoarse;
    S0Trail tr; S0BSrc bsrc;
};
template <int V> using IntTag = std::integral_constant<int, V>;
template <typename T> constexpr bool is_f32() { return std::is_same<T, float>::value; }

template <int NS, bool EC, bool FZ, int TR, typename ET, int PO, int BF = 0, typename XT = double>
bool s0r_row(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    if (p.NS != NS || p.EC != EC || p.FROM_ZERO != FZ || p.TRAIL != TR || p.ET32 != is_f32<ET>() || p.PO != PO || p.BF != BF || p.XT32 != is_f32<XT>()) return false;
    k_sweep0r<NS, EC, FZ, TR, ET, PO, 1, BF, XT><<<dim3(p.blocks * nslots), p.block, p.lds, c->stream>>>(
        f0, c->L[0].ni, c->L[0].nj, p.TI, p.PO, p.nx, p.ny, nslots, (const XT*)a.x_in, (XT*)a.x_out, (const double*)a.b, a.active,
        (const ET*)a.ecoarse, p.nci, p.ncj, a.tr, 0, 0, a.bsrc);
    return true;
}
bool launch_s0r(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    auto shapes = [&](auto ns, auto po) {
        constexpr int NS = decltype(ns)::value, PO = decltype(po)::value;
        return s0r_row<NS, true, false, 1, float, PO>(c, p, f0, nslots, a) || s0r_row<NS, true, false, 0, float, PO>(c, p, f0, nslots, a) ||
               s0r_row<NS, true, false, 1, double, PO>(c, p, f0, nslots, a) || s0r_row<NS, false, false, 1, double, PO>(c, p, f0, nslots, a) ||
               s0r_row<NS, true, false, 0, double, PO>(c, p, f0, nslots, a) ||
               s0r_row<NS, false, true, 0, double, PO, s0r_bf_from_zero(NS)>(c, p, f0, nslots, a) ||
               s0r_row<NS, false, false, 0, double, PO>(c, p, f0, nslots, a);
    };
    auto from_zero = [&](auto bf) {   // the two-sweep pass from zero with the coarse right-hand side and / or the vector update
        constexpr int BF = decltype(bf)::value;
        return s0r_row<2, false, true, 2, float, 0, BF, float>(c, p, f0, nslots, a) || s0r_row<2, false, true, 2, float, 0, BF, double>(c, p, f0, nslots, a) ||
               s0r_row<2, false, true, 2, double, 0, BF, double>(c, p, f0, nslots, a);
    };
    return from_zero(IntTag<3>{}) || from_zero(IntTag<1>{}) || from_zero(IntTag<2>{}) ||
           s0r_row<2, false, true, 0, double, 0, 1, double>(c, p, f0, nslots, a) || s0r_row<2, false, true, 0, double, 0, 2, double>(c, p, f0, nslots, a) ||
           s0r_row<2, true, false, 1, float, 1, 0, float>(c, p, f0, nslots, a) || s0r_row<2, true, false, 1, double, 1, 0, float>(c, p, f0, nslots, a) ||
           s0r_row<2, true, false, 0, float, 1, 0, float>(c, p, f0, nslots, a) || s0r_row<2, true, false, 0, double, 1, 0, float>(c, p, f0, nslots, a) ||
           shapes(IntTag<2>{}, IntTag<0>{}) || shapes(IntTag<2>{}, IntTag<1>{}) || shapes(IntTag<1>{}, IntTag<0>{}) || shapes(IntTag<1>{}, IntTag<1>{});
}

template <int NS, bool EC, bool FZ, int TR, typename ET = double>
bool s0m_row(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    if (p.NS != NS || p.EC != EC || p.FROM_ZERO != FZ || p.TRAIL != TR || p.ET32 != is_f32<ET>()) return false;
    k_sweep0m<NS, EC, FZ, TR, ET><<<dim3(p.blocks * nslots), p.block, p.lds, c->stream>>>(
        f0, c->L[0].ni, c->L[0].nj, p.TI, p.PO, p.nx, p.ny, nslots, (const double*)a.x_in, (double*)a.x_out, (const double*)a.b, a.active,
        (const ET*)a.ecoarse, p.nci, p.ncj, a.tr);
    return true;
}
bool launch_s0m(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    auto shapes = [&](auto ns) {
        constexpr int NS = decltype(ns)::value;
        return s0m_row<NS, true, false, 1, float>(c, p, f0, nslots, a) || s0m_row<NS, true, false, 0, float>(c, p, f0, nslots, a) ||
               s0m_row<NS, true, false, 1>(c, p, f0, nslots, a) || s0m_row<NS, false, false, 1>(c, p, f0, nslots, a) ||
               s0m_row<NS, true, false, 0>(c, p, f0, nslots, a) || s0m_row<NS, false, true, 0>(c, p, f0, nslots, a) ||
               s0m_row<NS, false, false, 0>(c, p, f0, nslots, a);
    };
    return shapes(IntTag<2>{}) || shapes(IntTag<1>{});
}

template <int NS, bool EC, bool FZ, int PO>
bool s0p_row(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    if (p.NS != NS || p.EC != EC || p.FROM_ZERO != FZ || p.PO != PO) return false;
    k_sweep0p<NS, EC, FZ, PO><<<dim3(p.blocks * nslots), p.block, p.lds, c->stream>>>(
        f0, c->L[0].ni, c->L[0].nj, p.TI, p.nx, p.nxp, p.ny, nslots, (const float*)a.x_in, (float*)a.x_out, (const float*)a.b, a.active,
        (const float*)a.ecoarse, p.nci, p.ncj);
    return true;
}
bool launch_s0p(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    auto shapes = [&](auto ns, auto po) {
        constexpr int NS = decltype(ns)::value, PO = decltype(po)::value;
        return s0p_row<NS, true, false, PO>(c, p, f0, nslots, a) || s0p_row<NS, false, true, PO>(c, p, f0, nslots, a) ||
               s0p_row<NS, false, false, PO>(c, p, f0, nslots, a);
    };
    return shapes(IntTag<2>{}, IntTag<0>{}) || shapes(IntTag<2>{}, IntTag<1>{}) || shapes(IntTag<1>{}, IntTag<0>{}) || shapes(IntTag<1>{}, IntTag<1>{});
}

template <typename VT, bool EC, bool FZ>
bool s0_row(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    if (p.EC != EC || p.FROM_ZERO != FZ) return false;
    k_sweep0<VT, EC, FZ><<<dim3(p.blocks * nslots), p.block, p.lds, c->stream>>>(
        f0, c->L[0].ni, c->L[0].nj, p.TI, p.PO, p.nx, p.ny, nslots, (const VT*)a.x_in, (VT*)a.x_out, (const VT*)a.b, a.active,
        (const VT*)a.ecoarse, p.nci, p.ncj);
    return true;
}
template <typename VT>
bool launch_s0(vof_ctx* c, const L0Pass& p, const Fine0& f0, int nslots, const L0Ptrs& a) {
    return s0_row<VT, true, false>(c, p, f0, nslots, a) || s0_row<VT, false, true>(c, p, f0, nslots, a) || s0_row<VT, false, false>(c, p, f0, nslots, a);
}

// The folded s update (BF = 1) is followed, in stream order, by what follows the stand-alone k_update_s: (s, s) and the stopping
// rule at the half step; pairs done there get their x += alpha y and leave the cycle
void fold_s_epilogue(vof_ctx* c, int np, const L0Pass& p) {
    const size_t len = 3 * c->L[0].npts;
    { Prof pr(c, VOF_K_VECTOR, 0); k_scalar<S_S><<<np, 64, 0, c->stream>>>(c->sc, c->partials, (int)p.blocks, c->active, c->prm.rtol, c->prm.max_iterations); }
    { Prof pr(c, VOF_K_VECTOR, 0);
      if (p.XT32) k_fix_half<float><<<dim3(64, np), RBLK, 0, c->stream>>>(c->kx, (const float*)c->ky, len, c->sc);
      else k_fix_half<double><<<dim3(64, np), RBLK, 0, c->stream>>>(c->kx, (const double*)c->ky, len, c->sc);
      k_clear_half<<<(np + 255) / 256, 256, 0, c->stream>>>(c->sc, np); }
}

// Options of smooth_level_t, and of the passes it issues through sweep_level_t
template <typename VT>
struct SmoothArgs {
    bool from_zero = false;        // smooth_level_t: start from a zero guess instead of the contents of x
    bool reverse = false;          // colours 3,2,1,0
    const VT* ecoarse = nullptr;   // coarse-grid correction still to be added (x += P ecoarse)
    bool ec32 = false;             // ... which really is float32 data (float64 level 0 above float32 coarse levels)
    bool allow_swap = false;       // smooth_level_t: the result may be left in `tmp`
    bool final_smooth = false;     // smooth_level_t: the last pass is the cycle's last (it takes the Krylov product, if one is wanted)
    bool out64 = false;            // the result is written as float64 although VT is float (k_sweep_st; the caller has checked that it applies)
    bool skip0 = false;            // x comes straight from a reverse sweep with the same b: colour 0 needs no update (k_sweep_st)
    void* rr_out = nullptr;        // level 0: the coarse right-hand side is wanted from the last pass, written here ...
    bool rr_f32 = false;           // ... as float32
    int nsweeps = 1;               // sweep_level_t: sweeps of this pass (2: level 0 only)
    bool trail = false;            // sweep_level_t: this pass is the cycle's last
};

// One pass x_in -> x_out (x_in == nullptr: zero initial guess): a.nsweeps full 4-colour sweeps.
template <typename VT>
void sweep_level_t(vof_ctx* c, int l, const VT* x_in, VT* x_out, const VT* b, int np, ActiveSet active, const SmoothArgs<VT>& a,
                   CycleIO& io) {
    Level& lv = c->L[l];
    const VT* ecoarse = a.ecoarse;
    const int po = a.reverse ? 1 : 0;
    if (l == 0 && lv.C == nullptr) {   // matrix-free level 0
        L0Req rq;
        rq.from_zero = x_in == nullptr; rq.po = po; rq.nsweeps = a.nsweeps;
        rq.ec = ecoarse != nullptr; rq.ec32 = a.ec32;
        rq.trail = a.trail && io.trail.v != nullptr; rq.trail_dot = io.trail.dotvec != nullptr;
        rq.rr = a.rr_out != nullptr; rq.rr_f32 = a.rr_f32;
        rq.bf = io.bf_done ? 0 : io.bf_mode;
        rq.x32 = c->h32;
        const L0Pass p = plan_l0_pass<VT>(c, rq);
        // handoff32_ok asked the same planner, so this holds unless a caller set h32 for a cycle it was not asked about
        if (p.XT32 != c->h32) { c->err = "float32 level-0 hand-off: the planned pass does not store float32"; io.failed = true; return; }
        const S0Trail no_trail{nullptr, nullptr, 0, nullptr};
        const L0Ptrs ptrs{x_in, x_out, b, active, ecoarse,
                          p.rr() ? S0Trail{(double*)a.rr_out, nullptr, 0, nullptr} : (p.trail() ? io.trail : no_trail),
                          p.bf() ? io.bf : S0BSrc{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
        const Fine0 f0{c->frames, frame_stride(c), c->Nj, c->prm.speed_alpha, c->prm.remodelling_alpha, c->prm.reference_quirks, c->pp};
        bool launched = false;
        {
            Prof pr(c, VOF_K_GS0, 0, p.algo, p.moved);
            const int nslots = pair_slots(c, active, np);
            switch (p.fam) {
                case L0_SWEEP0R: launched = launch_s0r(c, p, f0, nslots, ptrs); break;
                case L0_SWEEP0M: launched = launch_s0m(c, p, f0, nslots, ptrs); break;
                case L0_SWEEP0P: launched = launch_s0p(c, p, f0, nslots, ptrs); break;
                case L0_SWEEP0: launched = launch_s0<VT>(c, p, f0, nslots, ptrs); break;
            }
        }
        if (!launched) { c->err = "internal: the library holds no kernel for the planned level-0 pass"; io.failed = true; return; }
        if (p.trail()) io.trail_nblk = (int)p.blocks;
        if (p.rr()) io.rr_done = true;
        if (p.bf()) { io.bf_done = true; if (p.bf() == 1) fold_s_epilogue(c, np, p); }
        return;
    }
    // the stored levels: 128-column aligned strips
    const int rows = lv.ni + po;
    const int W = GeoB::W;
    const int nx = (lv.nj + GeoB::OUT - 1) / GeoB::OUT;
    const int TI = pick_band_height(rows, nx, c->cur_units);
    const int ny = (rows + TI - 1) / TI;
    const int nslots = pair_slots(c, active, np);
    dim3 g((unsigned)nx * ny * nslots, 1, 1);
    const double vs = sizeof(VT);
    int nci = 0, ncj = 0;
    double ebytes = 0.0;
    if (ecoarse) { nci = c->L[l + 1].ni; ncj = c->L[l + 1].nj; ebytes = 3.0 * vs * c->L[l + 1].npts; }
    Prof p(c, VOF_K_GS, l, (coef_bytes(c, l) + (x_in ? 9.0 : 6.0) * vs) * lv.npts + ebytes);   // C + b(3) + x(3) in, x(3) out (+ coarse e)
    size_t lds = (size_t)(SW_RING * 3 * W) * sizeof(VT);
    if (sweep_st_usable(c, l)) {   // packed stencil formats: the kernel with the decoupled coefficient stream
        const uint32_t* Cw = (const uint32_t*)lv.C;
        auto launch = [&](auto ct_tag) {
        using PCT = typename decltype(ct_tag)::type;
        if (ecoarse) {   // the sweep starts from x_in + P ecoarse (coarse rows through a 3-row LDS ring)
            const size_t lds_e = lds + (size_t)9 * (W / 2 + 2) * sizeof(VT);
            if (a.out64) k_sweep_st<PCT, VT, double, true><<<g, GeoB::THREADS, lds_e, c->stream>>>(Cw, lv.ni, lv.nj, TI, po, nx, ny, nslots, x_in, (double*)x_out, b, active, ecoarse, nci, ncj, 0);
            else k_sweep_st<PCT, VT, VT, true><<<g, GeoB::THREADS, lds_e, c->stream>>>(Cw, lv.ni, lv.nj, TI, po, nx, ny, nslots, x_in, x_out, b, active, ecoarse, nci, ncj, 0);
        } else {
            const int sk = (a.skip0 && x_in && !a.reverse) ? 1 : 0;
            if (a.out64) k_sweep_st<PCT, VT, double><<<g, GeoB::THREADS, lds, c->stream>>>(Cw, lv.ni, lv.nj, TI, po, nx, ny, nslots, x_in, (double*)x_out, b, active, nullptr, 0, 0, sk);
            else k_sweep_st<PCT, VT><<<g, GeoB::THREADS, lds, c->stream>>>(Cw, lv.ni, lv.nj, TI, po, nx, ny, nslots, x_in, x_out, b, active, nullptr, 0, 0, sk);
        }
        };
        if (c->cfmt == 3) launch(TypeTag<CoefF8>{}); else launch(TypeTag<CoefB16>{});
        return;
    }
    CDISPATCH(c, l, {
        SweepStored<CT> pol; pol.C = (const CW*)lv.C; pol.plane = CLay(lv.ni, lv.nj).plane;
        k_sweep<SweepStored<CT>, GeoB, VT><<<g, GeoB::THREADS, lds, c->stream>>>(pol, lv.ni, lv.nj, TI, po, nx, ny, nslots, x_in, x_out, b, active, ecoarse, nci, ncj);
    });
}

// Stored level l between two visits (revisit_fusable): a reverse sweep x_in -> x_mid and a forward sweep x_mid -> x_out, which
// leaves colour 0 alone, in one pass (k_sweep_st2).  The bands are those of the forward sweep.
template <typename VT>
void sweep2_level_t(vof_ctx* c, int l, const VT* x_in, VT* x_mid, VT* x_out, const VT* b, int np, ActiveSet active) {
    Level& lv = c->L[l];
    const int nx = (lv.nj + GeoR::OUT - 1) / GeoR::OUT;
    const int TI = pick_band_height(lv.ni, nx, c->cur_units);
    const int ny = (lv.ni + TI - 1) / TI;
    const int nslots = pair_slots(c, active, np);
    dim3 g((unsigned)nx * ny * nslots, 1, 1);
    const double vs = sizeof(VT);
    // algorithmic: the two sweeps as sweep_level_t counts them; moved: C once + b(3) + x(3) in, x(6) out
    Prof p(c, VOF_K_GS, l, 2.0 * (coef_bytes(c, l) + 9.0 * vs) * lv.npts, (coef_bytes(c, l) + 12.0 * vs) * lv.npts);
    const size_t lds = (size_t)(GeoR::RING * 3 * GeoR::W) * sizeof(VT);
    const uint32_t* Cw = (const uint32_t*)lv.C;
    if (c->cfmt == 3) k_sweep_st2<CoefF8, VT><<<g, GeoR::THREADS, lds, c->stream>>>(Cw, lv.ni, lv.nj, TI, nx, ny, nslots, x_in, x_mid, x_out, b, active);
    else k_sweep_st2<CoefB16, VT><<<g, GeoR::THREADS, lds, c->stream>>>(Cw, lv.ni, lv.nj, TI, nx, ny, nslots, x_in, x_mid, x_out, b, active);
}

// nu sweeps (from a zero guess if a.from_zero, else from x); the result is guaranteed to end in `x`, or - with a.allow_swap - in
// the buffer returned: `x`, or `tmp` when the last out-of-place sweep ended there (saves a device-to-device copy on the coarse levels).
// a.ecoarse: on the matrix-free level 0 it is folded into the first sweep (coarse rows streamed through LDS); otherwise the
// prolongation kernel runs first.
template <typename VT>
VT* smooth_level_t(vof_ctx* c, int l, VT* x, VT* tmp, const VT* b, int nu, int np, ActiveSet active, SmoothArgs<VT> a, CycleIO& io) {
    const size_t bytes = (size_t)np * 3 * c->L[l].npts * sizeof(VT);
    const bool fine0 = l == 0 && c->L[0].C == nullptr;
    const bool fold = a.ecoarse && nu > 0 && c->fused && !a.from_zero && (fine0 || (sweep_st_usable(c, l) && c->fold_stored));
    if (a.ecoarse && !fold) {
        prolong_add_level_t<VT>(c, l, x, a.ecoarse, np, active);
        a.ecoarse = nullptr;
    }
    if (nu <= 0) {
        if (a.from_zero) hipMemsetAsync(x, 0, bytes, c->stream);
        return x;
    }
    if (!c->fused) {   // reference path: one launch per colour, in place (double vectors only)
        if (a.from_zero) hipMemsetAsync(x, 0, bytes, c->stream);
        for (int s = 0; s < nu; ++s)
            for (int k = 0; k < 4; ++k)
                gs_colour(c, l, (double*)x, (const double*)b, a.reverse ? 3 - k : k, np, active);
        return x;
    }
    // out-of-place fused sweeps: choose the first destination so that the last pass writes into x.  On level 0 a pass may
    // perform two sweeps (temporal blocking): nu sweeps = ceil(nu / 2) passes over the data.
    L0Req two_rq;
    two_rq.nsweeps = 2;
    const bool two = fine0 && plan_l0_pass<VT>(c, two_rq).NS == 2;
    const int npass = two ? (nu + 1) / 2 : nu;
    const VT* src = a.from_zero ? nullptr : x;
    VT* dst = (a.from_zero && (npass % 2 == 1)) ? x : tmp;
    int left = nu;
    for (int s = 0; s < npass && !io.failed; ++s) {
        const bool first = s == 0, last = s == npass - 1;
        SmoothArgs<VT> pa = a;
        pa.nsweeps = two ? std::min(2, left) : 1;
        pa.trail = a.final_smooth && last && l == 0;
        if (!first) { pa.ecoarse = nullptr; pa.skip0 = false; }
        if (!last) { pa.out64 = false; pa.rr_out = nullptr; }
        sweep_level_t<VT>(c, l, src, dst, b, np, active, pa, io);
        left -= pa.nsweeps;
        src = dst;
        dst = (dst == x) ? tmp : x;
    }
    if (src != x) {
        if (a.allow_swap) return tmp;
        hipMemcpyAsync(x, src, bytes, hipMemcpyDeviceToDevice, c->stream);
    }
    return x;
}

// ---- coarse tail (k_tail_cycle): levels tail_first .. last in one launch, one workgroup per pair
void tail_emit(const vof_ctx* c, std::vector<unsigned char>* ops, int l, bool from_zero) {
    const vof_params& P = c->prm;
    const int last = (int)c->L.size() - 1, tl = l - c->tail_first;
    auto emit = [&](int code, int arg) { ops[0].push_back((unsigned char)code); ops[1].push_back((unsigned char)tl); ops[2].push_back((unsigned char)arg); };
    if (l == last) { emit(T_COARSE, 0); return; }
    const int nu1 = P.nu_pre_coarse > 0 ? P.nu_pre_coarse : P.nu_pre;
    const int nu2 = P.nu_post_coarse > 0 ? P.nu_post_coarse : P.nu_post;
    emit(T_SMOOTH, (nu1 << 2) | (from_zero ? 1 : 0));
    emit(T_RESTRICT, 0);
    tail_emit(c, ops, l + 1, true);
    if (P.w_cycle_level == l && l + 1 < last) {
        const int visits = P.w_cycle_visits > 0 ? P.w_cycle_visits : 2;
        for (int v = 1; v < visits; ++v) tail_emit(c, ops, l + 1, false);
    }
    emit(T_PROLONG, 0);
    emit(T_SMOOTH, (nu2 << 2) | 2);
}

// (Re)build the operation list for the current cycle parameters; false: the tail cannot be used (too many operations)
bool tail_prepare(vof_ctx* c) {
    if (c->tail_first < 0 || !c->fused) return false;
    const vof_params& P = c->prm;
    const int key[6] = {P.nu_pre, P.nu_post, P.nu_pre_coarse, P.nu_post_coarse, P.w_cycle_level, P.w_cycle_visits};
    if (memcmp(key, c->tail_key, sizeof key) != 0) {
        std::vector<unsigned char> ops[3];
        tail_emit(c, ops, c->tail_first, true);
        memcpy(c->tail_key, key, sizeof key);
        if (ops[0].size() > (size_t)TAIL_MAX_OPS - 1 || std::max({P.nu_pre, P.nu_post, P.nu_pre_coarse, P.nu_post_coarse}) > 63) { c->tail.n_ops = -1; return false; }
        c->tail.n_ops = (int)ops[0].size();
        for (int i = 0; i < c->tail.n_ops; ++i) { c->tail.op[i] = ops[0][i]; c->tail.op_level[i] = ops[1][i]; c->tail.op_arg[i] = ops[2][i]; }
    }
    return c->tail.n_ops > 0;
}

template <typename VT>
void tail_cycle_t(vof_ctx* c, VT* x, const VT* b, int np, ActiveSet active, bool from_zero) {
    TailArgs A = c->tail;
    const int l0 = c->tail_first, last = (int)c->L.size() - 1;
    for (int l = l0; l <= last; ++l) A.L[l - l0].C = c->L[l].C;
    A.invT = c->invT;
    if (!from_zero) A.op_arg[0] &= ~1;   // the first operation is the pre-smoothing of the top tail level
    const Level& top = c->L[l0];
    Prof p(c, VOF_K_COARSE_TAIL, l0, (from_zero ? 6.0 : 9.0) * sizeof(VT) * top.npts);   // b in, x (in and) out; stencils stay in cache
    CDISPATCH(c, l0, (k_tail_cycle<CT, VT><<<pair_slots(c, active, np), TAIL_THREADS, c->tail_lds, c->stream>>>(A, b, x, from_zero ? 1 : 0, active)));
}

// One multigrid cycle on level l for A_l x = b, starting from a zero guess (from_zero) or from the contents of x.
// (x, tmp) are the level's ping-pong buffers.  Returns the buffer holding the result: `x`, or - on the levels >= 1,
// where the caller only reads it - `tmp`.  With prm.w_cycle_level == l the next coarser level is visited twice
// (the second visit continues from the first one's result): a W-cycle restricted to one level.
template <typename VT>
// after_post: x holds the result of a previous visit of this level with the same b, i.e. of its reverse post-smoothing sweep
// emit64 (level 1 under a float64 level 0, vcycle_precision 3): the last post-smoothing sweep writes the result as float64
// defer_post (revisit_fusable(c, l), another visit follows): the visit ends with x + P e and leaves its post-smoothing sweep to the
// next visit, which is told so by post_pending and performs it together with its own pre-smoothing sweep (k_sweep_st2).  That
// pass writes two vectors, so the level's third buffer (r) joins the ping-pong pair; the caller only reads what is returned.
VT* vcycle_t(vof_ctx* c, int l, VT* x, VT* tmp, const VT* b, int np, ActiveSet active, CycleIO& io, bool from_zero = true,
             bool after_post = false, bool emit64 = false, bool defer_post = false, bool post_pending = false) {
    int last = (int)c->L.size() - 1;
    if (l == last) { coarse_solve_t<VT>(c, b, x, np, active); return x; }
    if (l == c->tail_first && l > 0 && tail_prepare(c)) { tail_cycle_t<VT>(c, x, b, np, active, from_zero); return x; }
    Level& lv = c->L[l];
    Level& nx = c->L[l + 1];
    const int nu1 = (l > 0 && c->prm.nu_pre_coarse > 0) ? c->prm.nu_pre_coarse : c->prm.nu_pre;
    const int nu2 = (l > 0 && c->prm.nu_post_coarse > 0) ? c->prm.nu_post_coarse : c->prm.nu_post;
    // pre-smoothing.  Level 0: result forced into x (the Krylov loop owns that buffer).  Stored levels: the result may end in
    // the ping-pong partner (the caller only reads the buffer this function returns), so the two just trade names - and the
    // partner then still holds the input of the last sweep, which is all k_resrestrict_u needs besides the result.
    const bool resu = l > 0 && lv.C != nullptr && c->fused && nu1 >= 1;
    SmoothArgs<VT> pre;
    pre.from_zero = from_zero;
    if (l == 0) {   // the coarse right-hand side is wanted from the last pre-smoothing pass (plan_l0_pass says whether it can)
        pre.rr_out = nx.b;
        pre.rr_f32 = coarse32_ok(c, nu2);
        io.rr_done = false;
    } else if (c->fused) {
        pre.allow_swap = true;
        pre.skip0 = after_post && !from_zero && nu2 >= 1;
    }
    if (post_pending) {   // x -> tmp (the previous visit's result, x_old of k_resrestrict_u) -> the third buffer
        VT* third = (VT*)lv.x;
        if (third == x || third == tmp) third = (VT*)lv.x2;
        if (third == x || third == tmp) third = (VT*)lv.r;
        sweep2_level_t<VT>(c, l, x, tmp, third, b, np, active);
        x = third;
    } else if (smooth_level_t<VT>(c, l, x, tmp, b, nu1, np, active, pre, io) != x) std::swap(x, tmp);
    if (io.failed) return x;
    const bool rr_fused = l == 0 && io.rr_done;   // ... and it did (k_sweep0r, TRAIL = 2)
    if constexpr (std::is_same<VT, double>::value) {
        if (l == 0 && coarse32_ok(c, nu2)) {
            // float64 vectors on level 0, float32 below: the fused residual + restriction writes the coarse right-hand side as
            // float32, the levels below run in float32, and the post-smoothing pass interpolates the float32 correction
            if (!rr_fused) resrestrict_fine_t<double, float>(c, x, b, (float*)nx.b, np, active);
            float* fx = (float*)nx.x;
            float* ft = (float*)nx.x2;
            // The last visit of level 1 hands its result up as float64 when its last operation is a k_sweep_st sweep (a regular
            // stored level with post-smoothing): 12 more bytes per level-1 point written there, but the pass above then reads
            // the correction as it does in the all-float64 cycle - measured: interpolating from float32 rows costs that pass
            // 6 % (5 ms per step at 255 pairs), widening the stores of the level-1 sweep costs 1 ms
            const int nu2c = c->prm.nu_post_coarse > 0 ? c->prm.nu_post_coarse : c->prm.nu_post;
            const bool can64 = 1 < last && !(c->tail_first == 1 && tail_prepare(c)) && sweep_st_usable(c, 1) && nu2c > 0;
            const int visits = (c->prm.w_cycle_level == 0 && 1 < last) ? (c->prm.w_cycle_visits > 0 ? c->prm.w_cycle_visits : 2) : 1;
            const bool fr = visits > 1 && revisit_fusable(c, 1);
            float* fe = vcycle_t<float>(c, 1, fx, ft, (const float*)nx.b, np, active, io, true, false, /*emit64=*/can64 && visits == 1, /*defer_post=*/fr);
            for (int v = 1; v < visits; ++v) {
                float* other = (fe == fx) ? ft : fx;
                fe = vcycle_t<float>(c, 1, fe, other, (const float*)nx.b, np, active, io, false, false, /*emit64=*/can64 && v == visits - 1,
                                     /*defer_post=*/fr && v < visits - 1, /*post_pending=*/fr);
            }
            SmoothArgs<double> post;
            post.reverse = post.allow_swap = post.final_smooth = true;
            post.ecoarse = (const double*)fe;
            post.ec32 = !can64;
            return smooth_level_t<double>(c, 0, x, tmp, b, nu2, np, active, post, io);
        }
    }
    if (resu) {
        const VT* x_old = (from_zero && nu1 == 1) ? nullptr : tmp;
        resrestrict_u_t<VT>(c, l, x, x_old, (VT*)nx.b, np, active);
    } else if (l == 0 && lv.C == nullptr) {   // matrix-free level 0: residual + restriction in one streaming pass
        if (!rr_fused) resrestrict_fine_t<VT>(c, x, b, (VT*)nx.b, np, active);
    } else {
        apply_level_t<VT>(c, l, x, b, (VT*)lv.r, 1, np, active);
        restrict_level_t<VT>(c, l, (const VT*)lv.r, (VT*)nx.b, np, active);
    }
    VT* cx = (VT*)nx.x;
    VT* ct = (VT*)nx.x2;
    const int visits = (c->prm.w_cycle_level == l && l + 1 < last) ? (c->prm.w_cycle_visits > 0 ? c->prm.w_cycle_visits : 2) : 1;
    const bool fr = visits > 1 && revisit_fusable(c, l + 1);
    VT* ec = vcycle_t<VT>(c, l + 1, cx, ct, (const VT*)nx.b, np, active, io, true, false, false, /*defer_post=*/fr);
    for (int v = 1; v < visits; ++v) {
        VT* other = (ec == cx) ? ct : cx;
        ec = vcycle_t<VT>(c, l + 1, ec, other, (const VT*)nx.b, np, active, io, false, /*after_post=*/true, false,
                          /*defer_post=*/fr && v < visits - 1, /*post_pending=*/fr);
    }
    SmoothArgs<VT> post;
    post.reverse = post.allow_swap = true;
    post.final_smooth = l == 0;
    post.ecoarse = ec;
    post.out64 = emit64 && l == 1 && std::is_same<VT, float>::value && nu2 > 0;
    if (defer_post) {
        prolong_add_level_t<VT>(c, l, x, ec, np, active);
        return x;
    }
    return smooth_level_t<VT>(c, l, x, tmp, b, nu2, np, active, post, io);
}

template <typename VT> int direct_apply_t(vof_ctx* c, VT* z, const VT* r, int np);   // direct preconditioner, below

// One cycle M b -> *xslot (c->ky or c->kz).  The out-of-place sweeps may leave the result in the level-0 ping-pong partner
// instead (an odd number of passes); the two buffers then trade places - a pointer swap instead of a copy of the vector.
void vcycle(vof_ctx* c, double** xslot, const void* b, int np, ActiveSet active, CycleIO& io) {
    if (c->direct_on) {   // the direct preconditioner takes the place of the cycle (every pair of the batch, active or not)
        VDISPATCH(c, direct_apply_t<VT>(c, (VT*)*xslot, (const VT*)b, np));
        return;
    }
    void* res = nullptr;
    VDISPATCH(c, res = (void*)vcycle_t<VT>(c, 0, (VT*)*xslot, (VT*)c->L[0].x2, (const VT*)b, np, active, io));
    if (res != (void*)*xslot) {
        c->L[0].x2 = (void*)*xslot;
        *xslot = (double*)res;
    }
}

// Build the Galerkin hierarchy and the coarsest-level dense inverse for the current batch.
int build_hierarchy(vof_ctx* c, int np) {
    const vof_params& P = c->prm;
    c->cfmt = P.coarse_precision;
    int nl = (int)c->L.size();
    for (int l = 0; l + 1 < nl; ++l) {
        Level &f = c->L[l], &k = c->L[l + 1];
        const dim3 g = grid2d(k.ni, k.nj, np);
        if (l == 0) {
            Prof p(c, VOF_K_GALERKIN0, 0);
            // the points away from the border by the interior kernel and the border frame by the generic one on a compact grid,
            // or every point by the generic kernel (switched off, or no such point)
            const GalerkinFrame frame(f.ni, f.nj, k.ni, k.nj);
            const bool split = frame.any_interior() && (c->galerkin_fast & 1);
            const dim3 gb = split ? dim3((frame.border_points(k.ni, k.nj) + NT - 1) / NT, 1, np) : g;
            if (split && (c->galerkin_fast & 2))
                CDISPATCH(c, 1, (k_galerkin<double, CT, true, true, true><<<g, blk2d, 0, c->stream>>>(
                                     c->frames, frame_stride(c), c->Nj, P.speed_alpha, P.remodelling_alpha, P.reference_quirks,
                                     nullptr, f.ni, f.nj, (CW*)k.C, k.ni, k.nj, c->pp, 0)));
            else if (split)
                CDISPATCH(c, 1, (k_galerkin<double, CT, true, true><<<g, blk2d, 0, c->stream>>>(
                                     c->frames, frame_stride(c), c->Nj, P.speed_alpha, P.remodelling_alpha, P.reference_quirks,
                                     nullptr, f.ni, f.nj, (CW*)k.C, k.ni, k.nj, c->pp, 0)));
            CDISPATCH(c, 1, (k_galerkin<double, CT, true, false><<<gb, blk2d, 0, c->stream>>>(
                                 c->frames, frame_stride(c), c->Nj, P.speed_alpha, P.remodelling_alpha, P.reference_quirks,
                                 nullptr, f.ni, f.nj, (CW*)k.C, k.ni, k.nj, c->pp, split ? 1 : 0)));
        } else {
            Prof p(c, VOF_K_GALERKIN, l);
            CDISPATCH(c, 1, (k_galerkin<CT, CT, false, false><<<g, blk2d, 0, c->stream>>>(
                                 nullptr, 0, 0, 0.0, 0.0, 0, (const CW*)f.C, f.ni, f.nj, (CW*)k.C, k.ni, k.nj, nullptr, 0)));
        }
    }
    return 0;
}

}  // namespace

// The 1-level case needs the fine stencil in stored form.
namespace vof {
__global__ __launch_bounds__(NT) void k_store_fine_stencil(const double* __restrict__ frames, size_t frame_stride,
                                                           int Nj, double alpha, double beta, int quirks, int ni,
                                                           int nj, double* __restrict__ C,
                                                           const PairParam* __restrict__ pp) {
    int q = blockIdx.x * BX + threadIdx.x, p = blockIdx.y * BY + threadIdx.y, pair = blockIdx.z;
    if (p >= ni || q >= nj) return;
    size_t npts = (size_t)ni * nj, idx = (size_t)p * nj + q;
    int fidx = pair;
    if (pp) { alpha = pp[pair].alpha; beta = pp[pair].beta; fidx = pp[pair].frame; }
    PixCoef k = pix_coef(frames + (size_t)fidx * frame_stride, Nj, p, q, quirks);
    const CLay L(ni, nj);
    double* out = C + (size_t)pair * 81 * L.plane + L.idx(p, q);
    (void)idx;
    npts = L.plane;
    for (int oi = -1; oi <= 1; ++oi)
        for (int oj = -1; oj <= 1; ++oj) {
            double blk[9];
            int tp = p + oi, tq = q + oj;
            if (tp < 0 || tp >= ni || tq < 0 || tq >= nj) {
                for (int t = 0; t < 9; ++t) blk[t] = 0.0;
            } else {
                folded_block(k, alpha, beta, p, q, ni, nj, oi, oj, blk);
            }
            for (int t = 0; t < 9; ++t) out[(size_t)(((oi + 1) * 3 + (oj + 1)) * 9 + t) * npts] = blk[t];
        }
}
}  // namespace vof

namespace {

int setup_batch(vof_ctx* c, const double* frames_dev, int np) {
    c->frames = frames_dev;
    c->npairs = np;
    c->cur_units = np;
    int nl = (int)c->L.size();
    if (nl == 1) {
        Level& f = c->L[0];
        Prof p(c, VOF_K_GALERKIN0, 0);
        k_store_fine_stencil<<<grid2d(f.ni, f.nj, np), blk2d, 0, c->stream>>>(
            c->frames, frame_stride(c), c->Nj, c->prm.speed_alpha, c->prm.remodelling_alpha,
            c->prm.reference_quirks, f.ni, f.nj, (double*)f.C, c->pp);
        c->cfmt = 0;
    } else {
        build_hierarchy(c, np);
    }
    Level& last = c->L[nl - 1];
    {
        Prof p(c, VOF_K_COARSE_SETUP, nl - 1);
        CDISPATCH(c, nl - 1, (k_coarse_build<CT><<<np, 256, 0, c->stream>>>((const CW*)last.C, last.ni, last.nj, c->W)));
        dbg_sync_check(c, "coarse_build", nl - 1);
        k_coarse_invert<<<np, 1024, 0, c->stream>>>(c->W, c->nd, c->invT);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

inline dim3 rgrid(const vof_ctx* c, int np) { return dim3(c->nblk, np, 1); }
inline dim3 rgrid(const vof_ctx* c, int np, const ActiveSet& a) { return rgrid(c, pair_slots(c, a, np)); }

// The active list from the flags in c->h_active, which the caller has just copied and waited for: the slots that are on, in
// ascending order, into the pinned mirror, and its copy queued on the context's stream.  The wait that precedes the next call
// (the next count) also ends that copy, so the one mirror is never rewritten under a copy in flight.
int post_active_list(vof_ctx* c, int np) {
    if (!c->use_alist) return 0;
    int n = 0;
    for (int k = 0; k < np; ++k) if (c->h_active[k]) c->h_alist[n++] = k;
    c->alist_n = n;
    if (n) HIPCHK(hipMemcpyAsync(c->alist, c->h_alist, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// Number of active pairs (copies the flags to the host; synchronises the stream); the active list is renewed along unless the
// caller still launches over the pairs of the list in place (renew_list == false).
int count_active(vof_ctx* c, int np, bool renew_list = true) {
    if (hipMemcpyAsync(c->h_active, c->active, np * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    int n = 0;
    for (int k = 0; k < np; ++k) n += c->h_active[k] != 0;
    if (renew_list && post_active_list(c, np)) return -1;
    return n;
}

// Restart length a call asks for (0: the default).
inline int gmres_restart_wanted(const vof_params& P) { return std::min(P.gmres_restart > 0 ? P.gmres_restart : 100, GM_MAXM); }

// A context outlives a call (the Python layer keeps one per image size), and the basis is sized by the first call that reaches
// the fallback.  A call that asks for a longer restart length than the basis was sized for gives it up here, at the start of the
// call (check_params) and so before any lane holds a view of it; gmres_phase then allocates one for this call on first use.  A
// basis the free memory cut below its request is kept: the same request would be cut again.  So is any basis under a call that
// cannot reach the fallback (krylov_method 0, BiCGStab alone): its restart length asks for nothing.
int gmres_release_short_basis(vof_ctx* c) {
    if (!c->gm_V || c->prm.krylov_method == 0 || gmres_restart_wanted(c->prm) <= c->gm_want) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int rc = dev_free(c, c->gm_V)) return rc;
    c->gm_V = nullptr;
    c->gm_m = c->gm_want = 0;
    return 0;
}

// Buffers of the GMRES fallback: restart length = min(requested, what fits in half of the free device memory).
int gmres_buffers(vof_ctx* c, int want_m) {
    want_m = std::min(want_m, GM_MAXM);
    if (c->gm_V) return 0;   // kept between calls (gmres_release_short_basis)
    const size_t vec = (size_t)c->B * 3 * c->L[0].npts * sizeof(double);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t fixed = (size_t)c->B * (sizeof(GmresState) + (GM_NV + 1) * c->nblk * sizeof(double) + sizeof(int));
    const double budget = 0.5 * (double)free_b - (double)fixed;
    int fit = budget > 0 ? (int)std::min<double>(budget / (double)vec, 1e6) - 1 : 0;
    int m = std::min(want_m, fit);
    if (m < 4) { c->err = "not enough device memory for the GMRES fallback (lower max_pairs_in_flight)"; return -3; }
    if (int rc = dev_alloc(c, &c->gm_V, (size_t)(m + 1) * c->B * 3 * c->L[0].npts)) return rc;
    if (!c->gm_state) if (int rc = dev_alloc(c, &c->gm_state, (size_t)c->B)) return rc;   // (do not depend on the restart length)
    if (!c->gm_partials) if (int rc = dev_alloc(c, &c->gm_partials, (size_t)c->B * (GM_NV + 1) * c->nblk)) return rc;
    c->gm_m = m;
    c->gm_want = want_m;
    return 0;
}

// Restarted, right-preconditioned GMRES on the pairs that are not converged yet: x = x_0 + M (V_k y), M = one
// multigrid cycle (float64 vectors), restart from the true residual b - A x.  `iterations` keeps counting Krylov steps
// (one cycle application each) on top of the BiCGStab iterations already spent.
// A lane's GMRES buffers are the parent's (allocated on first use, under a lock: two lanes may ask at once), viewed at the
// lane's slots; the basis keeps the parent's stride of B pairs per vector.  0, or -3 when the basis does not fit.
std::mutex g_lane_alloc;
int lane_gmres_attach(vof_ctx* c, bool basis, int want_m) {
    vof_ctx* p = c->lane_parent;
    std::lock_guard<std::mutex> lock(g_lane_alloc);
    int rc = 0;
    if (!p->gm_cycle) rc = dev_alloc(p, &p->gm_cycle, (size_t)p->B);
    if (!rc && basis && !p->gm_V) rc = gmres_buffers(p, want_m);
    if (rc) { c->err = p->err; p->err.clear(); return rc; }
    const size_t lo = (size_t)c->lane_lo;
    c->gm_cycle = p->gm_cycle + lo;
    if (p->gm_V) {
        c->gm_V = p->gm_V + lo * 3 * c->L[0].npts;
        c->gm_state = p->gm_state + lo;
        c->gm_partials = p->gm_partials + lo * (GM_NV + 1) * c->nblk;
        c->gm_m = p->gm_m;
    }
    return 0;
}

int gmres_phase(vof_ctx* c, int np, int* handed_over) {
    const vof_params& P = c->prm;
    hipStream_t s = c->stream;
    const size_t len = 3 * c->L[0].npts;
    const size_t vstride = (size_t)c->B * len;
    if (!c->gm_cycle) {   // flags are needed before the (large) basis is
        if (c->lane_parent) { if (int rc = lane_gmres_attach(c, false, 0)) return rc; }
        else if (int rc = dev_alloc(c, &c->gm_cycle, (size_t)c->B)) return rc;
    }
    k_gm_begin<<<(np + 63) / 64, 64, 0, s>>>(c->sc, c->active, c->gm_cycle, np, P.max_iterations);
    dbg_sync_check(c, "gm_begin", 0);
    int nact = count_active(c, np);
    if (nact < 0) { c->err = "stream synchronize failed"; return -2; }
    if (nact == 0) return 0;
    *handed_over = nact;
    if (!c->gm_V) {
        const int want = gmres_restart_wanted(P);
        int rc = c->lane_parent ? lane_gmres_attach(c, true, want) : gmres_buffers(c, want);
        if (rc == -3) { c->err.clear(); return 0; }   // no room: leave the pairs unconverged (reported per pair)
        if (rc) return rc;
    }
    c->gmres_pairs += nact;
    const int m = std::min(c->gm_m, gmres_restart_wanted(P));
    c->vfloat = false;   // float64 cycle vectors: the basis vectors are the cycle's right-hand sides
    c->vcoarse32 = false;
    double* V = c->gm_V;
    double* w = c->kt;
    const int coef_c = (int)(offsetof(GmresState, c) / sizeof(double)), coef_y = (int)(offsetof(GmresState, y) / sizeof(double));
    for (;;) {
        c->cur_units = nact;
        // The active list holds the pairs of the cycle from one k_gm_init to the next: k_gm_begin and k_gm_init leave active ==
        // cycle, and the list is taken at the count that follows them.  The counts inside a cycle do not renew it - the cycle's
        // last launches go by the cycle flags again -, so a pair that drops out in between keeps its blocks, which leave at once.
        const ActiveSet cyc = listed(c, c->gm_cycle);
        int nb = residual_d(c, c->kx, c->kb, V, np, cyc, 1);      // V_0 = b - A x and its norm
        if (!nb) { Prof p(c, VOF_K_REDUCE, 0); k_dot2<<<rgrid(c, np, cyc), RBLK, 0, s>>>(V, V, nullptr, nullptr, len, c->partials, cyc); nb = c->nblk; }
        { Prof p(c, VOF_K_VECTOR, 0);
          k_gm_init<<<np, 64, 0, s>>>(c->gm_state, c->sc, c->partials, nb, c->active, c->gm_cycle, P.max_iterations); }
        nact = count_active(c, np);
        if (nact < 0) { c->err = "stream synchronize failed"; return -2; }
        if (nact == 0) break;
        c->cur_units = nact;
        const ActiveSet act = listed(c, c->active);
        const dim3 rg = rgrid(c, np, act);   // (the same for the cycle flags: one list)
        { Prof p(c, VOF_K_VECTOR, 0, 16.0 * len); k_gm_scale<<<rg, RBLK, 0, s>>>(V, V, len, c->gm_state, act); }
        int jdone = 0;
        for (int j = 0; j < m; ++j) {
            CycleIO io;
            vcycle(c, &c->ky, V + (size_t)j * vstride, np, act, io);         // z = M v_j
            if (io.failed) return -1;
            krylov_apply(c, c->ky, w, np, act);                              // w = A z
            for (int pass = 0; pass < 2; ++pass) {                           // classical Gram-Schmidt, twice
                for (int i0 = 0; i0 <= j; i0 += GM_NV) {
                    int cnt = std::min(GM_NV, j + 1 - i0);
                    Prof p(c, VOF_K_REDUCE, 0, 8.0 * len * (cnt + 1));
                    k_gm_multidot<<<rg, RBLK, 0, s>>>(V + (size_t)i0 * vstride, vstride, cnt, w, len, c->gm_partials, act);
                    k_gm_hcoef<<<np, 64, 0, s>>>(c->gm_state, c->gm_partials, c->nblk, i0, cnt, pass, c->active);
                }
                for (int i0 = 0; i0 <= j; i0 += GM_NV) {
                    int cnt = std::min(GM_NV, j + 1 - i0);
                    bool last = pass == 1 && i0 + GM_NV > j;                 // last chunk: write v_{j+1} (unnormalised) + norm
                    Prof p(c, VOF_K_VECTOR, 0, 8.0 * len * (cnt + 2));
                    k_gm_axpy<<<rg, RBLK, 0, s>>>(V + (size_t)i0 * vstride, vstride, i0, cnt, c->gm_state, coef_c, -1.0, w,
                                                  last ? V + (size_t)(j + 1) * vstride : w, len, act, 0,
                                                  last ? c->gm_partials : nullptr);
                }
            }
            { Prof p(c, VOF_K_VECTOR, 0, 16.0 * len);
              k_gm_givens<<<np, 64, 0, s>>>(c->gm_state, c->sc, c->gm_partials, c->nblk, j, c->active, P.max_iterations);
              k_gm_scale<<<rg, RBLK, 0, s>>>(V + (size_t)(j + 1) * vstride, V + (size_t)(j + 1) * vstride, len, c->gm_state, act); }
            jdone = j + 1;
            nact = count_active(c, np, /*renew_list=*/false);
            if (nact < 0) { c->err = "stream synchronize failed"; return -2; }
            if (nact == 0) break;
            c->cur_units = nact;
        }
        // x += M (V_k y) for every pair of this cycle
        { Prof p(c, VOF_K_VECTOR, 0); k_gm_solve_y<<<(np + 63) / 64, 64, 0, s>>>(c->gm_state, c->gm_cycle, np); }
        for (int i0 = 0; i0 < jdone; i0 += GM_NV) {
            int cnt = std::min(GM_NV, jdone - i0);
            Prof p(c, VOF_K_VECTOR, 0, 8.0 * len * (cnt + 2));
            k_gm_axpy<<<rg, RBLK, 0, s>>>(V + (size_t)i0 * vstride, vstride, i0, cnt, c->gm_state, coef_y, 1.0,
                                          i0 ? c->kp : nullptr, c->kp, len, cyc, 1, nullptr);
        }
        CycleIO io;
        vcycle(c, &c->ky, c->kp, np, cyc, io);
        if (io.failed) return -1;
        { Prof p(c, VOF_K_VECTOR, 0, 24.0 * len); k_gm_xpy<<<rg, RBLK, 0, s>>>(c->kx, c->ky, len, cyc); }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------- direct preconditioner
// Dense inverse of the Schur blocks, all in-house: the one-workgroup Gauss-Jordan kernel with partial pivoting up to
// DIRECT_OWN_MAX unknowns per image row (images up to 66 pixels wide), the blocked Gauss-Jordan on the FP64 matrix cores
// beyond (vof_direct.hpp).  (Round 2 used rocSOLVER's getrf + getri for wide images.)
constexpr int DIRECT_OWN_MAX = 192;   // (round 2: 640; the blocked inverse is 6.6 x faster on the reference's 400-combination sweep at 128 x 128: 29.6 -> 4.5 s)
bool direct_uses_blocked(const vof_ctx* c) { return 3 * c->L[0].nj > DIRECT_OWN_MAX; }
int direct_ld(const vof_ctx* c) {
    const int m = 3 * c->L[0].nj;
    return direct_uses_blocked(c) ? ((m + DNB - 1) / DNB) * DNB : m;
}

// The automatic re-solve (preconditioner 2) needs nothing but room for the buffers.
int direct_capacity(vof_ctx* c, int want);
bool direct_ok_for_fallback(vof_ctx* c) { return c->dir_ok >= 0 ? c->dir_ok != 0 : direct_capacity(c, 1) >= 1; }
// preconditioner 1: every pair with the direct preconditioner (a one-level grid is solved by its dense inverse anyway)
inline bool direct_only(const vof_ctx* c) { return c->prm.preconditioner == 1 && c->L.size() > 1; }

// device bytes the direct preconditioner needs per pair in flight
size_t direct_bytes_per_pair(const vof_ctx* c) {
    const size_t ni = c->L[0].ni, nj = c->L[0].nj, m = 3 * nj, ld = (size_t)direct_ld(c);
    const size_t panels = direct_uses_blocked(c) ? (2 * ld + DNB) * DNB : 0;
    return (ni * ld * ld + ld * ld + panels + ni * nj * DIR_TAB + (3 * ni + 1) * m) * sizeof(double) + (m + 1) * sizeof(int);
}

// how many pairs the direct preconditioner can hold (0: it does not fit / is not available)
int direct_capacity(vof_ctx* c, int want) {
    if (c->dir_cap > 0) return c->dir_cap;
    if (c->L.size() < 2 || c->L[0].C != nullptr) return 0;                      // one-level grids are solved directly anyway
    if ((size_t)3 * c->L[0].nj > 8192) return 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
    const double per = (double)direct_bytes_per_pair(c);
    int fit = (int)std::min<double>(0.6 * (double)free_b / per, 1e6);
    return std::max(0, std::min(fit, want));
}

int direct_alloc(vof_ctx* c, int pairs) {
    if (c->dir_cap >= pairs) return 0;
    if (c->dir_cap > 0) { c->err = "direct preconditioner buffers already allocated for a smaller batch"; return -3; }
    const size_t ni = c->L[0].ni, nj = c->L[0].nj, m = 3 * nj, P = (size_t)pairs, ld = (size_t)direct_ld(c);
    c->dir_ld = (int)ld;
    if (int rc = dev_alloc(c, &c->dir_T, P * ni * ld * ld)) return rc;
    if (int rc = dev_alloc(c, &c->dir_W, P * ld * ld)) return rc;
    if (direct_uses_blocked(c)) {
        if (int rc = dev_alloc(c, &c->dir_R, P * ld * DNB)) return rc;
        if (int rc = dev_alloc(c, &c->dir_C, P * ld * DNB)) return rc;
        if (int rc = dev_alloc(c, &c->dir_D, P * DNB * DNB)) return rc;
        const int lds = (DNB * DNB + DNB * DNB_LDB) * (int)sizeof(double);
        HIPCHK(hipFuncSetAttribute((const void*)k_dir_bgj_panel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute((const void*)k_dir_bgj_update, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    if (int rc = dev_alloc(c, &c->dir_tabs, P * ni * nj * DIR_TAB)) return rc;
    if (int rc = dev_alloc(c, &c->dir_r, P * ni * m)) return rc;
    if (int rc = dev_alloc(c, &c->dir_y, P * ni * m)) return rc;
    if (int rc = dev_alloc(c, &c->dir_x, P * ni * m)) return rc;
    if (int rc = dev_alloc(c, &c->dir_t, P * m)) return rc;
    if (int rc = dev_alloc(c, &c->dir_ipiv, P * m)) return rc;
    if (int rc = dev_alloc(c, &c->dir_info, P)) return rc;
    c->dir_cap = pairs;
    return 0;
}

// factorisation for the current batch (frames / PairParam table as set up by solve_batch)
int direct_setup(vof_ctx* c, int np) {
    const vof_params& P = c->prm;
    const int ni = c->L[0].ni, nj = c->L[0].nj, m = 3 * nj, ld = c->dir_ld;
    const size_t sT = (size_t)ni * ld * ld, sW = (size_t)ld * ld, sTab = (size_t)ni * nj * DIR_TAB, rowTab = (size_t)nj * DIR_TAB;
    hipStream_t s = c->stream;
    Prof pr(c, VOF_K_COARSE_SETUP, 0);
    HIPCHK(hipMemsetAsync(c->dir_info, 0, (size_t)np * sizeof(int), s));
    k_dir_tables<<<dim3((nj + 255) / 256, ni, np), 256, 0, s>>>(c->frames, frame_stride(c), c->Nj, P.speed_alpha, P.remodelling_alpha,
                                                               P.reference_quirks, ni, nj, c->dir_tabs, c->pp);
    const dim3 gm((m + 255) / 256, m, np), gs((ld + 255) / 256, ld, np);
    const bool trace = getenv("VOF_TRACE") != nullptr;
    const bool blocked = direct_uses_blocked(c);
    const int nt = ld / DNB;
    const size_t bgj_lds = (size_t)(DNB * DNB + DNB * DNB_LDB) * sizeof(double);
    for (int p = 0; p < ni; ++p) {
        if (trace && (p < 2 || p == ni - 1)) { HIPCHK(hipStreamSynchronize(s)); fprintf(stderr, "[vof] direct_setup: row %d of %d (m = %d, %d pairs)\n", p, ni, m, np); fflush(stderr); }
        double* Tp = c->dir_T + (size_t)p * ld * ld;
        if (p > 0) k_dir_W<<<gm, 256, 0, s>>>(Tp - (size_t)ld * ld, sT, c->dir_tabs + (size_t)(p - 1) * rowTab, sTab, nj, c->dir_W, sW, ld);
        k_dir_schur<<<gs, 256, 0, s>>>(c->dir_tabs + (size_t)p * rowTab, sTab, nj, p > 0 ? c->dir_W : nullptr, sW, Tp, sT, ld);
        if (blocked) {
            for (int kt = 0; kt < nt; ++kt) {
                k_dir_bgj_panel<<<dim3(nt, 2, np), 256, bgj_lds, s>>>(Tp, sT, ld, kt, c->dir_R, c->dir_C, c->dir_D, c->dir_info);
                k_dir_bgj_update<<<dim3(nt, nt, np), 256, bgj_lds, s>>>(Tp, sT, ld, kt, c->dir_R, c->dir_C, c->dir_D);
            }
        } else {
            k_dir_invert<<<np, 1024, 2 * (size_t)m * sizeof(double), s>>>(Tp, sT, m, c->dir_ipiv, c->dir_info);
        }
    }
    HIPCHK(hipGetLastError());
    // a singular pivot anywhere makes the preconditioner useless for that pair: report it instead of iterating on garbage
    std::vector<int> info((size_t)np);
    HIPCHK(hipMemcpyAsync(info.data(), c->dir_info, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < np; ++k)
        if (info[k] != 0) { c->err = "direct preconditioner: a Schur block of pair " + std::to_string(k) + " of the batch is singular"; return -2; }
    return 0;
}

// z = A^{-1} r by block forward / backward substitution (r, z: level-0 vectors of the V-cycle type)
template <typename VT>
int direct_apply_t(vof_ctx* c, VT* z, const VT* r, int np) {
    const int ni = c->L[0].ni, nj = c->L[0].nj, m = 3 * nj, ld = c->dir_ld;
    const size_t sT = (size_t)ni * ld * ld, sTab = (size_t)ni * nj * DIR_TAB, rowTab = (size_t)nj * DIR_TAB, sV = (size_t)ni * m;
    hipStream_t s = c->stream;
    Prof pr(c, VOF_K_COARSE_SOLVE, 0);
    const dim3 gp(64, np), gv((m + 255) / 256, np), gg((m + 63) / 64, np);
    k_dir_permute<const VT, true><<<gp, 256, 0, s>>>(r, c->dir_r, ni, nj);
    for (int p = 0; p < ni; ++p) {      // forward: y_p = r_p - L_p T_{p-1} y_{p-1}
        if (p > 0) k_dir_gemv<<<gg, 256, 0, s>>>(c->dir_T + (size_t)(p - 1) * ld * ld, sT, m, c->dir_y + (size_t)(p - 1) * m, sV, c->dir_t, (size_t)m, ld);
        k_dir_rowupdate<<<gv, 256, 0, s>>>(c->dir_tabs + (size_t)p * rowTab, sTab, nj, -1, c->dir_r + (size_t)p * m, sV,
                                          p > 0 ? c->dir_t : nullptr, (size_t)m, c->dir_y + (size_t)p * m, sV);
    }
    for (int p = ni - 1; p >= 0; --p) {  // backward: x_p = T_p (y_p - U_p x_{p+1})
        k_dir_rowupdate<<<gv, 256, 0, s>>>(c->dir_tabs + (size_t)p * rowTab, sTab, nj, +1, c->dir_y + (size_t)p * m, sV,
                                          p + 1 < ni ? c->dir_x + (size_t)(p + 1) * m : nullptr, sV, c->dir_t, (size_t)m);
        k_dir_gemv<<<gg, 256, 0, s>>>(c->dir_T + (size_t)p * ld * ld, sT, m, c->dir_t, (size_t)m, c->dir_x + (size_t)p * m, sV, ld);
    }
    k_dir_permute<VT, false><<<gp, 256, 0, s>>>(z, c->dir_x, ni, nj);
    return 0;
}

// What one call of solve_batch is to do.  The tables are host arrays of np entries; solve_batch uploads them (after the work
// queued on the stream has ended, so the caller may re-use them between calls).
struct BatchReq {
    const double* frames;     // device pointer to frame 0 of the batch
    int np;
    const PairParam* table;   // per pair (alpha, beta, frame, output slot), or nullptr: pair k = frame k, the context's alphas
    const int* guess;         // per pair the saved solution in warm_x to start from (-1: constant initial fields), or nullptr: no warm start
    bool direct;              // precondition with the direct solver instead of the multigrid cycle (np <= dir_cap)
    double *vx, *vy, *gm, *speed;
    vof_pair_stats* stats;    // per pair, or nullptr
};

int solve_batch(vof_ctx* c, const BatchReq& rq) {
    const vof_params& P = c->prm;
    const double* const frames_dev = rq.frames;
    const int np = rq.np;
    vof_pair_stats* const stats = rq.stats;
    // the request as the kernels' launchers read it: c->pp / c->direct_on for the duration of this call, whatever way it ends
    struct ReqGuard { vof_ctx* c; ~ReqGuard() { c->pp = nullptr; c->direct_on = false; } } req_guard{c};
    const int* guess_src = nullptr;
    if (rq.table || rq.guess) {
        if (rq.table && !c->pp_buf) { if (int rc = dev_alloc(c, &c->pp_buf, (size_t)c->B)) return rc; }
        if (rq.guess && !c->warm_src) { if (int rc = dev_alloc(c, &c->warm_src, (size_t)c->B)) return rc; }
        HIPCHK(hipStreamSynchronize(c->stream));   // the host tables are re-used
        if (rq.table) {
            HIPCHK(hipMemcpyAsync(c->pp_buf, rq.table, (size_t)np * sizeof(PairParam), hipMemcpyHostToDevice, c->stream));
            c->pp = c->pp_buf;
        }
        if (rq.guess) {
            HIPCHK(hipMemcpyAsync(c->warm_src, rq.guess, (size_t)np * sizeof(int), hipMemcpyHostToDevice, c->stream));
            guess_src = c->warm_src;
        }
    }
    c->direct_on = rq.direct;
    // preconditioner 2 ("auto"): when the direct re-solve is available, the multigrid attempt is not run to the reference's
    // 1000 iterations (OF.py:1120) - where the cycle works it needs 3 .. 100 Krylov steps, and a pair that
    // has not converged after MG_ATTEMPT_CAP of them is handed to the direct preconditioner, which settles it in one or two
    struct MaxItGuard { vof_params& p; int saved; ~MaxItGuard() { p.max_iterations = saved; } } max_it_guard{c->prm, c->prm.max_iterations};
    constexpr int MG_ATTEMPT_CAP = 150;
    // (images up to 1026 pixels wide - the reference's real-data sizes -: the direct re-solve takes 3.3 s per pair at 514^2, 18 s and
    // 79 GB at 1026^2, the multigrid attempt to 1000 iterations as long again)
    if (P.preconditioner == 2 && !c->direct_on && c->L.size() > 1 && P.max_iterations > MG_ATTEMPT_CAP && 3 * c->L[0].nj <= 3100 &&
        direct_ok_for_fallback(c))
        c->prm.max_iterations = MG_ATTEMPT_CAP;
    if (stats) HIPCHK(hipEventRecord(c->ev_batch[0], c->stream));
    // storage type of the cycle vectors for this batch (an earlier batch may have switched to float64: "auto"
    // precision after 8 iterations, GMRES fallback)
    c->vfloat = (P.vcycle_precision == 1 || P.vcycle_precision == 2) && c->fused && c->L.size() > 1 && !c->direct_on;
    c->vcoarse32 = P.vcycle_precision == 3 && !c->direct_on;
    c->h32 = false;
    if (c->direct_on) {   // direct preconditioner: block-tridiagonal LU instead of the Galerkin hierarchy
        if (np > c->dir_cap) { c->err = "batch larger than the direct preconditioner's buffers"; return -1; }
        c->frames = frames_dev;
        c->npairs = np;
        c->cur_units = np;
        if (int rc = direct_setup(c, np)) return rc;
        c->direct_pairs += np;
    } else if (int rc = setup_batch(c, frames_dev, np)) return rc;
    Level& f = c->L[0];
    const size_t len = 3 * f.npts;
    hipStream_t s = c->stream;
    // right-hand side and its norm
    // initial guess (OF.py:799-802: constants, in pixels/frame), right-hand side, initial residual r0 and shadow residual r^ = r0
    double sx = P.delta_t / P.delta_x;
    const bool zero_guess = !guess_src && (P.initial_v_x == 0.0 && P.initial_v_y == 0.0 && P.initial_remodelling == 0.0);
    double* rh = c->krh;   // r^: from the zero guess it IS b (read-only from here on) - no copy; a restart switches to the real buffer
    // the fused prologue (k_stream_apply0<2>): b, x0, r0 = b - A x0 and r^ = r0 in one pass over level 0, with (b, b) and
    // (r0, r0) in slots 0 and 1 of the partials
    const bool fuse_pro = (c->fused_ends & 1) && !zero_guess && residual_copy_ok(c) && !c->direct_on;
    int nbb = c->nblk;                          // per-pair partial sums of (b, b) ...
    int nb0 = c->nblk;                          // ... and of (r0, r0): from the zero guess those of (b, b), still in place
    const double* part_r0 = c->partials;
    if (fuse_pro) {
        c->cur_units = np;
        nbb = nb0 = fused_prologue(c, guess_src, P.initial_v_x * sx, P.initial_v_y * sx, P.initial_remodelling, np);
        part_r0 = c->partials + nb0;
    } else {   // b and the block partial sums of (b, b) in one pass; from the zero guess r0 = b is written along
        Prof p(c, VOF_K_RHS, 0);
        k_rhs_norm<<<rgrid(c, np), RBLK, 0, s>>>(frames_dev, frame_stride(c), c->Nj, f.ni, f.nj, c->kb, zero_guess ? c->kr : nullptr,
                                                c->partials, c->pp);
    }
    { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_BNORM><<<np, 64, 0, s>>>(c->sc, c->partials, nbb, c->active, P.rtol, P.max_iterations); }
    if (zero_guess) {
        HIPCHK(hipMemsetAsync(c->kx, 0, (size_t)np * len * sizeof(double), s));
        rh = c->kb;
    } else if (!fuse_pro) {
        if (guess_src) {   // warm start from the solution of a neighbouring, already solved pair (cf. OF.py:803-806)
            Prof p(c, VOF_K_VECTOR, 0, 16.0 * len);
            k_gather_guess<<<rgrid(c, np), RBLK, 0, s>>>(c->kx, c->warm_x, guess_src, len, f.npts, P.initial_v_x * sx, P.initial_v_y * sx,
                                                        P.initial_remodelling);
        } else {
            Prof p(c, VOF_K_VECTOR, 0); k_fill<<<dim3(c->nblk, np), 256, 0, s>>>(c->kx, f.npts, P.initial_v_x * sx, P.initial_v_y * sx, P.initial_remodelling);
        }
        // r0 = b - A x0 with the partial sums of (r0, r0) and, where the streaming kernel runs, the copy r^ from the same pass
        const bool two = residual_copy_ok(c);
        nb0 = residual_d(c, c->kx, c->kb, c->kr, np, ALL_PAIRS, 1, two ? c->krh : nullptr);
        if (!two) HIPCHK(hipMemcpyAsync(c->krh, c->kr, (size_t)np * len * sizeof(double), hipMemcpyDeviceToDevice, s));
        // (p and v need no initialisation: the first iteration after a (re)start sets p = r without reading either)
        if (!nb0) {   // the operator kernel in use does not fuse the norm
            Prof p(c, VOF_K_REDUCE, 0); k_dot2<<<rgrid(c, np), RBLK, 0, s>>>(c->kr, c->kr, nullptr, nullptr, len, c->partials, ALL_PAIRS);
            nb0 = c->nblk;
        }
    }
    { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_R0><<<np, 64, 0, s>>>(c->sc, part_r0, nb0, c->active, P.rtol, P.max_iterations); }

    // krylov_method: 0 = BiCGStab only (the reference's 'bcgs'); 1 = GMRES only; 2 = BiCGStab, and restarted GMRES for
    // the pairs that have not met the tolerance after `fallback_after` iterations (or broke down)
    const int bicg_limit = P.krylov_method == 1 ? 0 : (P.krylov_method == 2 ? std::min(P.max_iterations, P.fallback_after) : P.max_iterations);
    int it_total = 0;   // BiCGStab iterations of this batch (all rounds)
    auto bicg_loop = [&](int limit) -> int {
    bool ran_on_r = false;   // this round's first iteration ran the cycle on r instead of writing p = r
    for (int it = 0; it < limit; ++it, ++it_total) {
        HIPCHK(hipMemcpyAsync(c->h_active, c->active, np * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        int nact = 0;
        for (int k = 0; k < np; ++k) nact += c->h_active[k] != 0;
        if (nact == 0) break;
        if (int rc = post_active_list(c, np)) return rc;
        // vcycle_precision 2 ("auto"): float32 V-cycle vectors for the first iterations, float64 for stragglers
        // (in the slowly converging regimes float32 storage costs iterations)
        if (it_total == AUTO_F64_AFTER) { if (P.vcycle_precision == 2) c->vfloat = false; c->vcoarse32 = false; }
        c->cur_units = nact;
        // float32 level-0 hand-off vectors under the same rule (y and z of one iteration have the same type)
        c->h32 = handoff32_ok(c);
        const ActiveSet act = listed(c, c->active);   // the launches of this iteration cover the nact listed pairs
        void* vrhs_p = c->vfloat ? (void*)c->b32 : (void*)c->kp;   // V-cycle right-hand sides (V-typed)
        void* vrhs_s = c->vfloat ? (void*)c->b32 : (void*)c->kr;
        const double vsz = (c->vfloat || c->h32) ? 4.0 : 8.0;
        // p = r + beta (p - omega v).  The iteration after a (re)start has p = r: the cycle then runs straight on r (unless it
        // needs a float32 copy of its right-hand side) and no p is written - the next iteration finds that p in r^ = r0.
        const bool on_r = it == 0 && !c->vfloat;
        const bool fold_b = fold_b_usable(c);
        // a cycle's requests were met or the iteration ends here (the folded update is only requested where fold_b_usable holds)
        auto cycle_ok = [c](const CycleIO& io, const char* which) {
            if (io.failed) c->h32 = false;
            else if (io.bf_mode && !io.bf_done) c->err = std::string("folded vector update (") + which + "): not consumed by the cycle";
            else return true;
            return false;
        };
        CycleIO io_p, io_s;
        if (on_r) vrhs_p = (void*)c->kr;
        else if (fold_b && it > 0) {
            // folded into the cycle's first pass (k_sweep0r, BF = 2).  The new p goes to the buffer of t, which is dead here,
            // and the two trade names (the bands of the pass overlap: no update in place)
            const double* p_old = (it == 1 && ran_on_r) ? rh : c->kp;
            io_p.bf = S0BSrc{c->kr, c->kv, p_old, c->kt, c->sc, nullptr};
            io_p.bf_mode = 2;
            std::swap(c->kp, c->kt);
            vrhs_p = (void*)c->kp;
        } else {
            Prof p(c, VOF_K_VECTOR, 0, 8.0 * len * (it == 0 ? 2 : 4) + (c->vfloat ? 4.0 * len : 0.0));
            const double* p_old = (it == 1 && ran_on_r) ? rh : c->kp;
            VDISPATCH(c, (k_update_p<VT><<<rgrid(c, np, act), RBLK, 0, s>>>(c->kp, p_old, c->kr, c->kv, len, c->sc, act,
                                                                     c->vfloat ? (VT*)c->b32 : (VT*)nullptr, it == 0 ? 1 : 0)));
        }
        if (it == 0) ran_on_r = on_r;
        // y = M p and v = A y with (r^, v): the product comes out of the cycle's last smoothing pass when that path applies
        io_p.trail = S0Trail{c->kv, rh, 0, c->partials};
        vcycle(c, &c->ky, vrhs_p, np, act, io_p);
        if (!cycle_ok(io_p, "p")) return -1;
        int nb1 = io_p.trail_nblk ? io_p.trail_nblk : krylov_apply(c, c->ky, c->kv, np, act, rh, 0);
        if (!nb1) { Prof p(c, VOF_K_REDUCE, 0, 16.0 * len); k_dot2<<<rgrid(c, np, act), RBLK, 0, s>>>(rh, c->kv, nullptr, nullptr, len, c->partials, act); nb1 = c->nblk; }
        { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_ALPHA><<<np, 64, 0, s>>>(c->sc, c->partials, nb1, c->active, P.rtol, P.max_iterations); }
        if (fold_b) {
            // s = r - alpha v, (s, s), the half-step test and its x += alpha y: in / right after the first pass of the cycle on s
            // (k_sweep0r, BF = 1).  s goes to the buffer of t (dead until the end of this cycle); r's buffer becomes t's
            io_s.bf = S0BSrc{c->kr, c->kv, nullptr, c->kt, c->sc, c->partials};
            io_s.bf_mode = 1;
            std::swap(c->kr, c->kt);
            vrhs_s = (void*)c->kr;
        } else {
        { Prof p(c, VOF_K_VECTOR, 0, 8.0 * len * 3 + (c->vfloat ? 4.0 * len : 0.0));   // s = r - alpha v, (s, s)
          VDISPATCH(c, (k_update_s<VT><<<rgrid(c, np, act), RBLK, 0, s>>>(c->kr, c->kv, len, c->sc, c->partials, act, c->vfloat ? (VT*)c->b32 : (VT*)nullptr))); }
        { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_S><<<np, 64, 0, s>>>(c->sc, c->partials, c->nblk, c->active, P.rtol, P.max_iterations); }
        { Prof p(c, VOF_K_VECTOR, 0);                                  // pairs done at the half step: x += alpha y
          YDISPATCH(c, (k_fix_half<VT><<<dim3(64, np), RBLK, 0, s>>>(c->kx, (const VT*)c->ky, len, c->sc)));
          k_clear_half<<<(np + 255) / 256, 256, 0, s>>>(c->sc, np); }
        }
        // z = M s and t = A z with (t, s) and (t, t)
        io_s.trail = S0Trail{c->kt, c->kr, 1, c->partials};
        vcycle(c, &c->kz, vrhs_s, np, act, io_s);
        if (!cycle_ok(io_s, "s")) return -1;
        int nb2 = io_s.trail_nblk ? io_s.trail_nblk : krylov_apply(c, c->kz, c->kt, np, act, c->kr, 1);
        if (!nb2) { Prof p(c, VOF_K_REDUCE, 0, 16.0 * len); k_dot2<<<rgrid(c, np, act), RBLK, 0, s>>>(c->kt, c->kr, c->kt, c->kt, len, c->partials, act); nb2 = c->nblk; }
        { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_OMEGA><<<np, 64, 0, s>>>(c->sc, c->partials, nb2, c->active, P.rtol, P.max_iterations); }
        { Prof p(c, VOF_K_VECTOR, 0, 8.0 * len * 6 + 2.0 * vsz * len);   // x += alpha y + omega z; r = s - omega t; (r,r), (r^,r)
          YDISPATCH(c, (k_update_xr<VT><<<rgrid(c, np, act), RBLK, 0, s>>>(c->kx, (const VT*)c->ky, (const VT*)c->kz, c->kr, c->kt, rh, len, c->sc, c->partials, act))); }
        { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_R><<<np, 64, 0, s>>>(c->sc, c->partials, c->nblk, c->active, P.rtol, P.max_iterations); }
    }
    c->h32 = false;   // (the other users of the cycle - GMRES, the debug entry points - decide for themselves)
    return 0;
    };
    if (int rc = bicg_loop(bicg_limit)) return rc;
    // independent residual (OF.py:1150-1151): ||b - A x|| recomputed from x for every pair
    // (keep == false: only the norm, no residual vector - it is needed again only if a pair has to be restarted)
    auto independent_residual = [&](bool keep) -> int {
        c->cur_units = np;
        int nb3 = keep ? 0 : residual_d(c, c->kx, c->kb, nullptr, np, ALL_PAIRS, 1);
        if (!nb3) nb3 = residual_d(c, c->kx, c->kb, c->kt, np, ALL_PAIRS, 1);
        if (!nb3) { Prof p(c, VOF_K_REDUCE, 0); k_dot2<<<rgrid(c, np), RBLK, 0, s>>>(c->kt, c->kt, nullptr, nullptr, len, c->partials, ALL_PAIRS); nb3 = c->nblk; }
        { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_FINAL><<<np, 64, 0, s>>>(c->sc, c->partials, nb3, c->active, P.rtol, P.max_iterations); }
        HIPCHK(hipGetLastError());
        return 0;
    };
    // ... and on the matrix-free level 0 the outputs and functionals from the same pass over x: they stand unless a pair is
    // restarted or handed to GMRES below
    bool finalized = false;
    if ((c->fused_ends & 2) && residual_copy_ok(c)) {
        c->cur_units = np;
        double* fpart = c->partials + (size_t)np * 3 * apply_grid(c, np).nblk;   // (part_per_pair holds both)
        const int nb3 = fused_epilogue(c, rq.vx, rq.vy, rq.gm, rq.speed, fpart, np);
        { Prof p(c, VOF_K_VECTOR, 0); k_scalar<S_FINAL><<<np, 64, 0, s>>>(c->sc, c->partials, nb3, c->active, P.rtol, P.max_iterations); }
        { Prof p(c, VOF_K_FINALIZE, 0); k_sum3<<<np, 64, 0, s>>>(fpart, nb3, c->func3); }
        HIPCHK(hipGetLastError());
        finalized = true;
    } else if (int rc = independent_residual(false)) return rc;
    // The stopping rule is evaluated on the independent residual.  BiCGStab tests its recursively updated residual, which
    // drifts from the true one (by rounding; visibly so near the attainable accuracy): pairs it declared converged whose
    // recomputed residual misses the tolerance are restarted from that residual (r = r^ = b - A x, p = v = 0), which a
    // further iteration or two settles.  What is still open afterwards goes to GMRES (krylov_method 2).
    if (bicg_limit > 0) {
        for (int round = 0; round < 3; ++round) {
            { Prof p(c, VOF_K_VECTOR, 0); k_bicg_restart<<<(np + 63) / 64, 64, 0, s>>>(c->sc, c->active, np, P.max_iterations); }
            int nact = count_active(c, np);
            if (nact < 0) { c->err = "stream synchronize failed"; return -2; }
            if (nact == 0) break;
            finalized = false;
            if (int rc = independent_residual(true)) return rc;   // the restart needs the residual vector itself (rare)
            c->cur_units = nact;
            rh = c->krh;   // (the restarting pairs get their new r^ written; the others are done and no longer read theirs)
            { Prof p(c, VOF_K_VECTOR, 0, 8.0 * len * 3);
              const ActiveSet act = listed(c, c->active);
              k_restart_vectors<<<rgrid(c, np, act), RBLK, 0, s>>>(c->kr, rh, c->kt, len, act); }
            if (int rc = bicg_loop(std::min(bicg_limit, 8))) return rc;
            if (int rc = independent_residual(false)) return rc;
        }
    }
    if (P.krylov_method != 0) {
        // GMRES takes the pairs BiCGStab left unconverged, and those whose recursively updated residual met the
        // tolerance while the true one does not (the usual drift of BiCGStab at tight tolerances)
        int handed_over = 0;
        if (int rc = gmres_phase(c, np, &handed_over)) return rc;
        if (handed_over) {
            finalized = false;
            if (int rc = independent_residual(false)) return rc;
        }
    }
    // functionals (OF.py:1167-1183) and epilogue (OF.py:1159-1166, 1189-1191)
    if (!finalized) {   // one pass over the solution: outputs + functionals
        Prof p(c, VOF_K_FINALIZE, 0);
        k_finalize_functionals<<<rgrid(c, np), RBLK, 0, s>>>(frames_dev, frame_stride(c), f.ni, f.nj, P.speed_alpha, P.remodelling_alpha,
                                                             P.reference_quirks, c->kx, P.delta_x / P.delta_t, rq.vx, rq.vy, rq.gm, rq.speed,
                                                             c->partials, c->pp);
        k_sum3<<<np, 64, 0, s>>>(c->partials, c->nblk, c->func3);
    }
    HIPCHK(hipGetLastError());
    if (stats) {
        HIPCHK(hipMemcpyAsync(c->h_sc, c->sc, np * sizeof(PairScalars), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(c->h_func3, c->func3, np * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(c->ev_batch[1], s));
        HIPCHK(hipStreamSynchronize(s));
        float batch_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&batch_ms, c->ev_batch[0], c->ev_batch[1]));
        for (int k = 0; k < np; ++k) {
            const PairScalars& q = c->h_sc[k];
            stats[k].iterations = q.iterations;
            stats[k].relative_residual = q.bnorm2 > 0 ? std::sqrt(q.rnorm2 / q.bnorm2) : 0.0;
            stats[k].converged = (q.rnorm2 <= q.tol2) ? 1 : 0;   // the rule on the independent residual (NaN: 0)
            stats[k].L1_functional = c->h_func3[3 * k];
            stats[k].speed_functional = c->h_func3[3 * k + 1];
            stats[k].remodelling_functional = c->h_func3[3 * k + 2];
            stats[k].batch_ms = batch_ms;
            stats[k].batch_pairs = np;
            stats[k].reserved = 0;
        }
    }
    return 0;
}

int check_params(vof_ctx* c, const vof_params* p) {
    if (!p) { c->err = "params is NULL"; return -1; }
    if (p->struct_size != sizeof(vof_params) || p->abi_version != VOF_VERSION) {
        char buf[256];
        snprintf(buf, sizeof buf, "vof_params ABI mismatch: caller has struct_size %u / version %u, library has %zu / %d "
                 "(fill the struct with vof_default_params(p, sizeof *p) of the matching include/vof.h)",
                 p->struct_size, p->abi_version, sizeof(vof_params), VOF_VERSION);
        c->err = buf;
        return -4;
    }
    if (!(p->delta_x != 0.0) || !(p->delta_t != 0.0)) { c->err = "delta_x and delta_t must be non-zero"; return -1; }
    if (p->nu_pre < 0 || p->nu_post < 0 || p->nu_pre + p->nu_post == 0) { c->err = "nu_pre + nu_post must be > 0"; return -1; }
    if (p->nu_pre_coarse < 0 || p->nu_post_coarse < 0) { c->err = "nu_*_coarse must be >= 0"; return -1; }
    if (p->w_cycle_level < -1 || p->w_cycle_level > 15) { c->err = "w_cycle_level must be -1 or a level index"; return -1; }
    if (p->w_cycle_visits < 0 || p->w_cycle_visits > 8) { c->err = "w_cycle_visits must be in [0, 8]"; return -1; }
    if (!(p->rtol > 0.0)) { c->err = "rtol must be > 0"; return -1; }
    if (p->coarse_precision < 0 || p->coarse_precision > 3) { c->err = "coarse_precision must be 0, 1, 2 or 3"; return -1; }
    if (p->vcycle_precision < 0 || p->vcycle_precision > 3) { c->err = "vcycle_precision must be 0, 1, 2 or 3"; return -1; }
    if (p->krylov_method < 0 || p->krylov_method > 2) { c->err = "krylov_method must be 0, 1 or 2"; return -1; }
    if (p->gmres_restart < 0 || p->gmres_restart > GM_MAXM) { c->err = "gmres_restart must be in [0, 128]"; return -1; }
    if (p->fallback_after < 0) { c->err = "fallback_after must be >= 0"; return -1; }
    if (p->warm_start_stride < 0) { c->err = "warm_start_stride must be >= 0"; return -1; }
    if (p->preconditioner < 0 || p->preconditioner > 2) { c->err = "preconditioner must be 0, 1 or 2"; return -1; }
    c->prm = *p;
    // float32 V-cycle vectors need the fused sweeps and a multi-level hierarchy
    c->vfloat = (p->vcycle_precision == 1 || p->vcycle_precision == 2) && c->fused && c->L.size() > 1;
    c->vcoarse32 = false;   // set per batch (solve_batch); the debug entry points run every level in one storage type
    if (int rc = gmres_release_short_basis(c)) return rc;
    return ensure_storage(c);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" {

int vof_version(void) { return VOF_VERSION; }

size_t vof_params_size(void) { return sizeof(vof_params); }

int vof_default_params(vof_params* p, size_t struct_size) {
    if (!p || struct_size != sizeof(vof_params)) return -1;   // a binding built against another layout: write nothing
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof(vof_params);
    p->abi_version = VOF_VERSION;
    p->speed_alpha = 1.0;          // OF.py:718
    p->remodelling_alpha = 1000.0; // OF.py:719
    p->delta_x = 1.0;
    p->delta_t = 1.0;
    p->rtol = 1e-6;                // OF.py:1120
    p->max_iterations = 1000;      // OF.py:1120
    p->nu_pre = 2;                 // (2,2) sweeps on level 0 ...
    p->nu_post = 2;
    p->nu_pre_coarse = 1;          // ... (1,1) on the stored-stencil levels (measured best time to solution)
    p->nu_post_coarse = 1;
    p->w_cycle_level = 1;          // level 1 visits level 2 several times per cycle (one-level W-cycle) ...
    p->w_cycle_visits = 3;         // ... three times: 5.35 -> 3.4 BiCGStab iterations on the benchmark workload
    p->reference_quirks = 1;
    p->coarse_precision = 3;       // Galerkin stencils (preconditioner only): 8-bit float off-diagonal blocks in units of a power
                                   // of two per block position, float32 diagonal block that keeps the block row sums: 120 B per
                                   // point, +1 % iterations against float32 / bfloat16 (2) on the benchmark, same counts in the
                                   // other regimes (scripts/gpu_regimes3.py)
    p->vcycle_precision = 3;       // float64 V-cycle vectors on level 0, float32 below (0: float64 everywhere, 1: float32 everywhere)
    p->krylov_method = 2;          // BiCGStab (the reference's 'bcgs'); stragglers are finished by restarted GMRES
    p->gmres_restart = 100;        // capped by the free device memory: (restart + 1) vectors per pair in flight
    p->warm_start_stride = 3;      // vof_solve_stack_dev: every 3rd pair first, the others start from their solved neighbour
    p->fallback_after = 25;        // BiCGStab iterations before the fallback (the benchmark regimes need 3-17)
    p->preconditioner = 2;         // multigrid cycle; pairs it leaves unconverged are re-solved with the direct preconditioner if it fits
    return 0;
}

const char* vof_last_error(const vof_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
size_t vof_workspace_bytes(const vof_ctx* ctx) { return ctx ? ctx->bytes : 0; }
int vof_num_levels(const vof_ctx* ctx) { return ctx ? (int)ctx->L.size() : 0; }

size_t vof_query_workspace(int n_i, int n_j, int B) { return vof_query_workspace_for(n_i, n_j, B, DEFAULT_COARSE_PRECISION, 3); }

size_t vof_query_workspace_for(int n_i, int n_j, int B, int coarse_precision, int vcycle_precision) {
    if (n_i < 4 || n_j < 4 || B < 1 || coarse_precision < 0 || coarse_precision > 3) return 0;
    size_t ni = n_i - 2, nj = n_j - 2, total = 0, b = (size_t)B;
    std::vector<std::pair<size_t, size_t>> lv{{ni, nj}};
    while (std::max(lv.back().first, lv.back().second) > (size_t)COARSEST_MAX)
        lv.push_back({(lv.back().first + 1) / 2, (lv.back().second + 1) / 2});
    size_t words = 0;   // 32-bit words of stencil storage
    total += (9 + ((vcycle_precision == 1 || vcycle_precision == 2) && lv.size() > 1 ? 1 : 0)) * b * 3 * ni * nj;
    for (size_t l = 0; l < lv.size(); ++l) {
        size_t npts = lv[l].first * lv[l].second;
        if (l + 1 < lv.size()) total += (l > 0 ? 2 : 1) * b * 3 * npts;
        if (l > 0) total += 2 * b * 3 * npts;
        const size_t plane = CLay((int)lv[l].first, (int)lv[l].second).plane;
        if (lv.size() == 1) total += b * 81 * plane;
        else if (l > 0) words += b * (size_t)(coef_bytes_per_point(coarse_precision) / 4) * plane;
    }
    size_t nd = 3 * lv.back().first * lv.back().second;
    total += b * nd * 2 * nd + b * nd * nd;
    return total * sizeof(double) + words * 4 + (size_t)B * 3 * 256 * sizeof(double) + 4096;
}

int vof_device_memory(int device_id, size_t* free_bytes, size_t* total_bytes) {
    size_t f = 0, t = 0;
    if (hipSetDevice(device_id) != hipSuccess) return -1;
    if (hipMemGetInfo(&f, &t) != hipSuccess) return -2;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

const char* vof_kernel_name(int k) {
    static const char* names[VOF_K_COUNT] = {"rhs", "apply0", "gs0", "gs", "residual", "restrict", "prolong",
                                             "galerkin0", "galerkin", "coarse_setup", "coarse_solve", "vector",
                                             "reduce", "finalize", "functionals", "coarse_tail", "preprocess"};
    return (k >= 0 && k < VOF_K_COUNT) ? names[k] : "?";
}

void vof_destroy(vof_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess && (c->dbg_sync || c->dbg_canary))
            fprintf(stderr, "vof_destroy: the context's stream ends with an error: %s\n", hipGetErrorString(e));
    }
    if (c->dbg_canary) {
        std::string rep;
        if (dbg_check_canaries(c, &rep) != 0) { fprintf(stderr, "vof_destroy: VOF_DEBUG_CANARY: %s\n", rep.c_str()); fflush(stderr); }
    }
    if (c->dbg_fd >= 0) close(c->dbg_fd);
    prof_collect(c);
    for (auto e : c->free_events) hipEventDestroy(e);
    for (const auto& a : c->allocs) hipFree(a.raw);
    if (c->h_active) hipHostFree(c->h_active);
    if (c->h_alist) hipHostFree(c->h_alist);
    if (c->h_sc) hipHostFree(c->h_sc);
    if (c->h_func3) hipHostFree(c->h_func3);
    if (c->h_bounce) hipHostFree(c->h_bounce);
    for (int i = 0; i < 2; ++i) if (c->ev_batch[i]) hipEventDestroy(c->ev_batch[i]);
    for (int i = 0; i < 2; ++i) {
        if (c->ev_solved[i]) hipEventDestroy(c->ev_solved[i]);
        if (c->ev_copied[i]) hipEventDestroy(c->ev_copied[i]);
        if (c->ev_uploaded[i]) hipEventDestroy(c->ev_uploaded[i]);
    }
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    for (int i = 0; i < MAX_LANES; ++i) {
        if (c->lane_stream[i]) hipStreamDestroy(c->lane_stream[i]);
        for (int j = 0; j < 2; ++j) if (c->lane_ev[i][j]) hipEventDestroy(c->lane_ev[i][j]);
    }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    for (hipEvent_t e : c->group_ev) if (e) hipEventDestroy(e);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
}

static int create_impl(vof_ctx* c, int device_id, int n_i, int n_j, int B, void* stream) {
    if (n_i < 4 || n_j < 4) { c->err = "image must be at least 4x4 (the mirror boundary rows need N >= 4)"; return -1; }
    if (B < 1) { c->err = "max_pairs_in_flight must be >= 1"; return -1; }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) { c->err = "no such HIP device"; return -1; }
    HIPCHK(hipSetDevice(device_id));
    c->device = device_id;
    c->Ni = n_i; c->Nj = n_j; c->B = B;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else { HIPCHK(hipStreamCreate(&c->stream)); c->own_stream = true; }
    memset(c->prof_ms, 0, sizeof c->prof_ms);
    memset(c->prof_n, 0, sizeof c->prof_n);
    memset(c->prof_units, 0, sizeof c->prof_units);
    memset(c->prof_bytes, 0, sizeof c->prof_bytes);
    memset(c->prof_moved, 0, sizeof c->prof_moved);
    vof_default_params(&c->prm, sizeof c->prm);
    if (const char* e = getenv("VOF_DEBUG_SYNC")) c->dbg_sync = atoi(e);
    if (const char* e = getenv("VOF_DEBUG_CANARY")) c->dbg_canary = e[0] != '0';
    if (const char* e = getenv("VOF_DEBUG_ALLOC_LOG")) c->dbg_alloc_log = e[0] != '0';
    if (const char* e = getenv("VOF_DEBUG_POISON")) c->dbg_poison = e[0] != '0';
    if (c->dbg_sync)
        if (const char* e = getenv("VOF_DEBUG_SYNC_FILE")) c->dbg_fd = open(e, O_WRONLY | O_CREAT, 0644);
    if (const char* e = getenv("VOF_FOLD_STORED")) c->fold_stored = e[0] != '0';
    if (const char* e = getenv("VOF_FUSE_REVISIT")) c->fuse_revisit = e[0] != '0';
    if (const char* e = getenv("VOF_GALERKIN_FAST")) c->galerkin_fast = atoi(e) & 3;
    if (const char* e = getenv("VOF_L0_HANDOFF")) c->l0_handoff = e[0] != '0';
    if (const char* e = getenv("VOF_SWEEP0R_MIN_BLOCKS")) c->sweep0r_min_blocks = atol(e);
    if (const char* e = getenv("VOF_ACTIVE_LIST")) c->use_alist = e[0] != '0';
    if (const char* e = getenv("VOF_FUSE_B")) c->fuse_b = e[0] != '0';
    if (const char* e = getenv("VOF_FUSE_RR")) c->fuse_rr = e[0] != '0';
    if (const char* e = getenv("VOF_FUSED_ENDS")) { const int v = atoi(e); if (v >= 0 && v <= 3) c->fused_ends = v; }
    // level shapes
    Level l0; l0.ni = n_i - 2; l0.nj = n_j - 2; l0.npts = (size_t)l0.ni * l0.nj;
    c->L.push_back(l0);
    while (std::max(c->L.back().ni, c->L.back().nj) > COARSEST_MAX) {
        Level k; k.ni = (c->L.back().ni + 1) / 2; k.nj = (c->L.back().nj + 1) / 2; k.npts = (size_t)k.ni * k.nj;
        c->L.push_back(k);
    }
    int nl = (int)c->L.size();
    if (nl > 16) { c->err = "too many levels"; return -1; }
    size_t len0 = 3 * l0.npts;
    // (b32, the float32 copy of the cycle's right-hand side, exists only while vcycle_precision 1 / 2 is in use: ensure_storage)
    for (double** v : {&c->kx, &c->kb, &c->kr, &c->krh, &c->kp, &c->kv, &c->kt, &c->ky, &c->kz})
        if (int rc = dev_alloc(c, v, (size_t)B * len0)) return rc;
    for (int l = 0; l < nl; ++l) {
        Level& lv = c->L[l];
        auto valloc = [&](void** q) { double* t = nullptr; int rc = dev_alloc(c, &t, (size_t)B * 3 * lv.npts); *q = t; return rc; };
        // residual scratch (level 0 forms its coarse right-hand side without a residual vector)
        if (l + 1 < nl && l > 0) if (int rc = valloc(&lv.r)) return rc;
        if (l + 1 < nl) if (int rc = valloc(&lv.x2)) return rc;
        if (l > 0) {
            if (int rc = valloc(&lv.x)) return rc;
            if (int rc = valloc(&lv.b)) return rc;
        }
        if (nl == 1) {   // a one-level grid keeps its fine stencil as float64
            double* C = nullptr;
            if (int rc = dev_alloc(c, &C, (size_t)B * 81 * CLay(lv.ni, lv.nj).plane)) return rc;
            lv.C = C;
        }
    }
    // stored stencils of the levels >= 1: sized for the default format; a call that asks for a wider one re-allocates them
    if (int rc = ensure_stencil_storage(c, vof_params_default_coarse_precision())) return rc;
    c->nd = 3 * (int)c->L.back().npts;
    {   // coarse tail: the deepest run of levels that fit one workgroup (and its LDS)
        int first = -1;
        for (int l = 1; l < nl; ++l) {
            const CLay lay(c->L[l].ni, c->L[l].nj);
            if (c->L[l].npts <= (size_t)TAIL_MAX_PTS && lay.sub <= (size_t)TAIL_MAX_SUB) { first = l; break; }
        }
        if (first >= 0) first = std::max(first, nl - TAIL_MAX_LEVELS);
        if (first >= 1 && first < nl - 1) {
            memset(&c->tail, 0, sizeof c->tail);
            int off = 0;
            for (int l = first; l < nl; ++l) {
                TailLevel& t = c->tail.L[l - first];
                const CLay lay(c->L[l].ni, c->L[l].nj);
                t.ni = c->L[l].ni; t.nj = c->L[l].nj; t.hj = lay.hj; t.sub = (int)lay.sub; t.plane = lay.plane;
                t.xo = off; off += 3 * (t.ni + 2) * (t.nj + 2);
                t.bo = off; off += 3 * t.ni * t.nj;
            }
            c->tail.ro = off; off += 3 * (int)c->L[first].npts;
            c->tail.nl = nl - first;
            c->tail.nd = c->nd;
            c->tail.n_ops = 0;
            c->tail_lds = (size_t)off * sizeof(double);
            if (c->tail_lds <= (size_t)150 * 1024) {
                c->tail_first = first;
                const int lds = (int)c->tail_lds;
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<CoefB16, double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<CoefB16, float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<CoefF8, double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<CoefF8, float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<float, double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<float, float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<double, double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                HIPCHK(hipFuncSetAttribute((const void*)k_tail_cycle<double, float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            }
        }
    }
    if (int rc = dev_alloc(c, &c->W, (size_t)B * c->nd * 2 * c->nd)) return rc;
    if (int rc = dev_alloc(c, &c->invT, (size_t)B * c->nd * c->nd)) return rc;
    {   // the level-0 smoother passes with the trailing stage need more than the default 64 KB of dynamic LDS
        const int lds = 18 * s0_row_bytes(8) + 9 * (S0_W / 2 + 2) * 8;
        HIPCHK(hipFuncSetAttribute((const void*)k_sweep0m<2, true, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute((const void*)k_sweep0m<2, false, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute((const void*)k_sweep0m<1, true, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute((const void*)k_sweep0m<1, false, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    {   // ... and so does the 22-row ring of the two-sweep pass of the stored levels with float64 vectors (74 KB; float32: 37 KB)
        const int lds = GeoR::RING * 3 * GeoR::W * (int)sizeof(double);
        HIPCHK(hipFuncSetAttribute((const void*)k_sweep_st2<CoefB16, double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute((const void*)k_sweep_st2<CoefF8, double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    c->nblk = (int)std::min<size_t>(256, std::max<size_t>(1, (len0 + 4 * RBLK - 1) / (4 * RBLK)));
    {
        int nblk_apply = ((l0.nj + AP_OUT - 1) / AP_OUT) * ((l0.ni + 31) / 32 + 1);   // smallest band height: 32 rows
        nblk_apply = std::max(nblk_apply, ((l0.nj + 99) / 100) * ((l0.ni + 1 + 31) / 32 + 1));   // k_sweep0m's trailing stage (strips >= 108 columns)
        // twice three slots: the fused epilogue keeps the functionals' partials behind those of the residual norm
        c->part_per_pair = (size_t)6 * std::max(c->nblk, nblk_apply);
        if (int rc = dev_alloc(c, &c->partials, (size_t)B * c->part_per_pair)) return rc;
    }
    if (int rc = dev_alloc(c, &c->sc, (size_t)B)) return rc;
    if (int rc = dev_alloc(c, &c->active, (size_t)B)) return rc;
    if (int rc = dev_alloc(c, &c->alist, (size_t)B)) return rc;
    if (int rc = dev_alloc(c, &c->func3, (size_t)B * 3)) return rc;
    HIPCHK(hipHostMalloc((void**)&c->h_active, B * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&c->h_alist, B * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&c->h_sc, B * sizeof(PairScalars)));
    HIPCHK(hipHostMalloc((void**)&c->h_func3, B * 3 * sizeof(double)));
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreate(&c->ev_batch[i]));
    return 0;
}

int vof_create(vof_ctx** out, int device_id, int n_i, int n_j, int max_pairs_in_flight, void* stream) {
    if (!out) { g_create_error = "out is NULL"; return -1; }
    *out = nullptr;
    vof_ctx* c = new (std::nothrow) vof_ctx();
    if (!c) { g_create_error = "out of host memory"; return -1; }
    int rc = create_impl(c, device_id, n_i, n_j, max_pairs_in_flight, stream);
    if (rc) {
        g_create_error = c->err;
        vof_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

}  // extern "C"

namespace {

// ---- lanes: the pairs of one device solve as concurrent groups, each on a stream of its own
//
// One stream runs a solve as a chain of dependent launches: each one ends with a tail in which the chip drains, many are
// under-filled by design (the coarse levels; k_tail_cycle runs one workgroup per pair), and the Krylov loop waits on the host
// once per iteration.  Two groups of pairs on two streams fill each other's gaps.  A lane is driven by
// a host thread of its own because its Krylov loop blocks on the host; one thread polling the events of all lanes instead
// would have to turn solve_batch inside out into a resumable state machine.
//
// Lanes of this solve: VOF_LANES (1 .. MAX_LANES, default 3), fewer while a lane's share of a phase would drop below
// VOF_LANES_MIN_MPIX (default 16) Mpixel of pairs - the same kind of rule as the two-phase one; one lane while profiling
// (per-launch times mean something only when launches do not overlap) or with VOF_DEBUG_SYNC.
double lanes_min_pixels() {
    double mpix = 16.0;
    if (const char* e = getenv("VOF_LANES_MIN_MPIX")) { const double v = atof(e); if (v >= 0.0) mpix = v; }
    return mpix * 1e6;
}

int lanes_for(const vof_ctx* c, int pairs_per_phase) {
    if (c->prof || c->dbg_sync) return 1;
    int n = 3;
    if (const char* e = getenv("VOF_LANES")) { const int v = atoi(e); if (v >= 1 && v <= MAX_LANES) n = v; }
    const double minpix = lanes_min_pixels();
    n = std::min(n, c->B);
    while (n > 1 && (pairs_per_phase < n || (double)pairs_per_phase / n * c->Ni * c->Nj < minpix)) --n;
    return n;
}

// ---- groups: what a lane runs in the two-phase solve
//
// The phase-1 pairs of a stack (every stride-th one) are cut into contiguous groups; a group is those phase-1 pairs and the
// warm pairs between them, and a lane runs phase 1 then phase 2 of each of its groups without meeting the other lanes.  The
// last warm pairs of a group take their guess from the first phase-1 pair of the NEXT group, so a group's phase 2 waits for
// the next group's phase 1 and for nothing else (GroupSync).  The order that keeps every such wait short and free of cycles:
// with G groups per lane, lane i owns the groups i, i + L, ... and runs them from the highest down - then the group a lane
// waits for is either one that the next lane started at the same moment or one of an earlier turn.
// The lanes get equal shares; with two groups per lane the cut inside a share differs from lane to lane ((L - i) / (L + 1) of
// the share first, so that the next lane's phase 1 is the shorter one and ends first), which keeps the lanes' under-filled last
// Krylov iterations of a batch apart: one lane's stragglers run beside the other lanes' full launches instead of beside their
// stragglers.  No group below the lanes' size rule (VOF_LANES_MIN_MPIX of phase-1 pairs): the cut is clamped to it, and a share
// too small for two such groups stays one group.
struct LaneGroup { int lo, hi, lane; };   // phase-1 positions [lo, hi) of the stack, run by `lane`

int lane_groups_wanted() {
    int g = 1;   // two groups per lane measured slower on the flagship stack: every extra batch ends in under-filled iterations of its own
    if (const char* e = getenv("VOF_LANE_GROUPS")) { const int v = atoi(e); if (v >= 1 && v <= MAX_LANE_GROUPS) g = v; }
    return g;
}

// n1 phase-1 pairs on L lanes, G groups per lane where the size rule allows it (else one).  Groups in the order of the pairs.
std::vector<LaneGroup> plan_groups(const vof_ctx* c, int n1, int L, int G) {
    const int min_pairs = std::max(1, (int)std::ceil(lanes_min_pixels() / ((double)c->Ni * c->Nj)));
    std::vector<int> share((size_t)L), head((size_t)L);
    for (int i = 0; i < L; ++i) {
        share[i] = (int)((long)n1 * (i + 1) / L - (long)n1 * i / L);
        if (G < 2 || share[i] < 2 * min_pairs) G = 1;
    }
    std::vector<LaneGroup> g;
    int at = 0;
    if (G == 2) {
        for (int i = 0; i < L; ++i)   // head: the group lane i runs first, the upper one in pair order
            head[i] = std::min(std::max((int)std::lround((double)share[i] * (L - i) / (L + 1)), min_pairs), share[i] - min_pairs);
        for (int i = 0; i < L; ++i) { g.push_back({at, at + share[i] - head[i], i}); at += share[i] - head[i]; }
        for (int i = 0; i < L; ++i) { g.push_back({at, at + head[i], i}); at += head[i]; }
    } else {
        for (int i = 0; i < L; ++i) { g.push_back({at, at + share[i], i}); at += share[i]; }
    }
    return g;
}

// Publication of the groups' phase-1 results between the lane threads.  `usable` (phase-1 solutions that may seed a neighbour:
// converged and finite) and `state` are read and written under the mutex only.  A group is published once the copy of its
// solutions into warm_x is queued on its lane's stream and the event behind it recorded - or once its lane has failed, with
// none of its pairs usable, so that nobody waits for it for ever.
struct GroupSync {
    std::mutex m;
    std::condition_variable cv;
    std::vector<char> usable;
    std::vector<int> state;   // per group: 0 not yet, 1 published with its event recorded, -1 published by a lane that failed
};

// Pairs a context runs in one batch: its own B, or a lane's share of the parent's slots.
inline int batch_slots(const vof_ctx* c) { return c->lane_parent ? c->lane_slots : c->B; }

// Lane i of n of context c: a copy of c whose per-pair buffers view the slots [B i / n, B (i + 1) / n).  Every kernel addresses
// a pair's data as base + pair * (per-pair size), with a per-pair size no larger than what the buffer holds per slot (B of
// them), so offset bases keep the lanes apart.  Shared and read-only: the level geometry, the parameters, the tail operation
// list, the frames and outputs (PairParam tables and pointers of the range), warm_x (indexed by the phase-1 position of a pair).
int make_lane(vof_ctx* c, int i, int n, vof_ctx* L) {
    if (!c->lane_stream[i]) {
        HIPCHK(hipStreamCreate(&c->lane_stream[i]));
        for (int j = 0; j < 2; ++j) HIPCHK(hipEventCreate(&c->lane_ev[i][j]));
    }
    *L = *c;
    const size_t lo = (size_t)c->B * i / n;
    L->lane_parent = c;
    L->lane_lo = (int)lo;
    L->lane_slots = (int)((size_t)c->B * (i + 1) / n - lo);
    for (int j = 0; j < MAX_LANES; ++j) { L->lane_stream[j] = nullptr; L->lane_ev[j][0] = L->lane_ev[j][1] = nullptr; }
    L->ev_fork = nullptr;
    L->stream = c->lane_stream[i];
    L->own_stream = false;
    L->ev_batch[0] = c->lane_ev[i][0];
    L->ev_batch[1] = c->lane_ev[i][1];
    L->allocs.clear();
    L->recs.clear();
    L->free_events.clear();
    L->prof = false;
    L->err.clear();
    L->h_bounce = nullptr;
    L->gmres_pairs = 0;
    L->dir_ok = direct_ok_for_fallback(c) ? 1 : 0;
    const size_t len0 = 3 * c->L[0].npts;
    for (double** v : {&L->kx, &L->kb, &L->kr, &L->krh, &L->kp, &L->kv, &L->kt, &L->ky, &L->kz, &L->b32, &L->gm_V})
        if (*v) *v += lo * len0;
    const int nl = (int)c->L.size();
    for (int l = 0; l < nl; ++l) {   // vectors: sized for float64 (a float32 view of a slot uses its first half)
        Level& lv = L->L[l];
        const size_t vb = 3 * lv.npts * sizeof(double);
        const size_t cb = (size_t)(nl == 1 ? 81 * 8 : c->c_bytes_per_point) * CLay(lv.ni, lv.nj).plane;
        for (void** q : {&lv.x, &lv.b, &lv.r, &lv.x2}) if (*q) *q = (char*)*q + lo * vb;
        if (lv.C) lv.C = (char*)lv.C + lo * cb;
    }
    L->W += lo * c->nd * 2 * c->nd;
    L->invT += lo * c->nd * c->nd;
    L->partials += lo * c->part_per_pair;
    L->sc += lo; L->h_sc += lo;
    L->active += lo; L->h_active += lo;
    L->alist += lo; L->h_alist += lo;
    L->func3 += 3 * lo; L->h_func3 += 3 * lo;
    if (L->pp_buf) L->pp_buf += lo;
    if (L->warm_src) L->warm_src += lo;
    if (L->gm_cycle) L->gm_cycle += lo;
    if (L->gm_state) L->gm_state += lo;
    if (L->gm_partials) L->gm_partials += lo * (GM_NV + 1) * c->nblk;
    return 0;
}

// Runs fn(lane, i) for the n lanes of c, each on a host thread of its own and after the work queued so far on c's stream, and
// joins them all (a lane's stream is drained before its thread ends).  The first failing lane's message goes to c->err.
// concurrent_only: the lanes wait for each other (the groups of the two-phase solve), so where not even one thread can be
// started nothing is run and LANES_NO_THREAD returned; otherwise lanes without a thread run here one after the other.
constexpr int LANES_NO_THREAD = -100;
template <typename F>
int run_lanes(vof_ctx* c, int n, F&& fn, bool concurrent_only = false) {
    std::vector<vof_ctx> lanes((size_t)n);
    for (int i = 0; i < n; ++i)
        if (int rc = make_lane(c, i, n, &lanes[i])) return rc;
    if (!c->ev_fork) HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_fork, c->stream));
    for (int i = 0; i < n; ++i) HIPCHK(hipStreamWaitEvent(lanes[i].stream, c->ev_fork, 0));
    std::vector<int> rc((size_t)n, 0);
    std::vector<std::thread> th;
    auto body = [&](int i) {
        vof_ctx* L = &lanes[i];
        if (hipSetDevice(c->device) != hipSuccess) { L->err = "hipSetDevice failed"; rc[i] = -2; return; }
        rc[i] = fn(L, i);
        const hipError_t e = hipStreamSynchronize(L->stream);
        if (!rc[i] && e != hipSuccess) { L->err = std::string("stream synchronize failed: ") + hipGetErrorString(e); rc[i] = -2; }
    };
    // from the last lane down: a group of the two-phase solve waits for one of the next lane, or for the first group of lane 0
    // (plan_groups) - with the last lane on a thread, lanes that run here one after the other find what they wait for
    try {
        for (int i = n - 1; i >= 0; --i) th.emplace_back(body, i);
    } catch (...) {   // no thread: the remaining lanes run here, one after the other
        if (th.empty() && concurrent_only) return LANES_NO_THREAD;
        for (int i = n - 1 - (int)th.size(); i >= 0; --i) body(i);
    }
    for (auto& t : th) t.join();
    for (int i = 0; i < n; ++i) c->gmres_pairs += lanes[i].gmres_pairs;
    for (int i = 0; i < n; ++i)
        if (rc[i]) { c->err = "lane " + std::to_string(i) + ": " + lanes[i].err; return rc[i]; }
    return 0;
}

// ---- plans of vof_solve_stack_host (no runtime call in them)

// Batch schedule: full batches, and the remainder split so that the LAST batch is small - its device-to-host copies are the
// only ones that cannot hide under a solve.
struct HostBatch { int k0, np; };
std::vector<HostBatch> plan_host_batches(int P, int B) {
    std::vector<HostBatch> batches;
    for (int k0 = 0; k0 < P;) {
        const int rest = P - k0;
        int np = std::min(B, rest);
        if (P > B && rest <= B && rest > 48) np = rest - std::max(16, rest / 4);   // e.g. 127 -> 96 + 31
        batches.push_back({k0, np});
        k0 += np;
    }
    return batches;
}

inline size_t next_page(uintptr_t base, size_t offset) { return (size_t)(((base + offset + 4095) & ~(uintptr_t)4095) - base); }

// Bytes of the movie (at address `base`) that are pinned right away; the rest is pinned by a helper thread while the first batch
// is solved.  The split lies behind the first batch's frames, on a page boundary so that the two registrations share no page.
size_t plan_movie_split(uintptr_t base, size_t movie_bytes, size_t first_batch_bytes, bool one_batch) {
    return one_batch ? movie_bytes : std::min(movie_bytes, next_page(base, first_batch_bytes));
}

// Output regions: array i is cut at the batch boundaries, each moved up to the next page so that no two registrations share a
// page; region (bi, i) - entry bi * 4 + i - is what batch bi's copy of array i writes, apart from the < 4 KB before its first
// page, which belong to region bi - 1.  Arrays not asked for have empty regions.
struct HostRegion { char* ptr; size_t bytes; };
std::vector<HostRegion> plan_output_regions(double* const* outs, const std::vector<HostBatch>& batches, size_t frame_bytes, size_t out_bytes) {
    const size_t nb = batches.size();
    std::vector<HostRegion> regions(nb * 4, HostRegion{nullptr, 0});
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        size_t prev = 0;
        for (size_t bi = 0; bi < nb; ++bi) {
            const size_t end = bi + 1 < nb ? std::min(out_bytes, next_page((uintptr_t)outs[i], (size_t)batches[bi + 1].k0 * frame_bytes)) : out_bytes;
            regions[bi * 4 + i] = HostRegion{(char*)outs[i] + prev, end - prev};
            prev = end;
        }
    }
    return regions;
}

// ---- the scratch arena of one ABI call -----------------------------------------------------------
// The blur, the box flow's general path, the sweeps, the channel comparison and the frame-wise calls take their device scratch
// from the context's one buffer through a Scratch on the stack of the call: the call declares typed regions, plan() picks the
// units in flight, grows the buffer and stores the addresses.  One walk measures and carves, so size and layout cannot disagree.
// The rule: an arena is planned exactly once per ABI call, and every address taken from it is dead when the call returns.  A
// helper that needs scratch declares it into its caller's arena (blur_regions, box_flow_regions, sweep_tail_regions) and never
// plans one; no entry point that plans an arena calls another that does.
struct Scratch {
    struct Region { void* ptr; size_t fixed, unit; };              // ptr: where the carve stores the region's address; bytes: fixed + units * unit
    vof_ctx* const c;
    std::vector<Region> regions;
    int units = 0; size_t bytes = 0;                               // what plan() settled on
    explicit Scratch(vof_ctx* c_) : c(c_) {}
    Scratch(const Scratch&) = delete;                              // the regions point at the caller's pointers
    // The request.  *p is the region's address after plan(): `count` elements once per call, per unit in flight (align_units:
    // each at a multiple of 256 bytes; returns the stride in elements), or per unit and once more (the frames of n pairs: n + 1).
    static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
    template <class T> void once(T** p, size_t count) { regions.push_back({p, count * sizeof(T), 0}); }
    template <class T> size_t per_unit(T** p, size_t count, bool align_units = false) {
        regions.push_back({p, 0, align_units ? up256(count * sizeof(T)) : count * sizeof(T)});
        return regions.back().unit / sizeof(T);
    }
    template <class T> void per_unit_plus_one(T** p, size_t count) { regions.push_back({p, count * sizeof(T), count * sizeof(T)}); }

    // The layout, stated once: region after region, each at a multiple of 256 bytes.  Returns the bytes `n` units in flight
    // take; a null base only measures.
    size_t carve(char* base, int n) const {
        size_t at = 0;
        for (const Region& r : regions) {
            if (base) { char* q = base + at; memcpy(r.ptr, &q, sizeof q); }
            at += up256(r.fixed + (size_t)n * r.unit);
        }
        return at;
    }

    // The units in flight - min(want, at_most), or the largest count (one at least) that needs no more than the buffer or `share`
    // of the memory that is free or the arena's - and the buffer.  Returns the count, or < 0 (out_of_memory(): the allocation failed).
    int plan(int want, int at_most, double share) {
        HIPCHK(hipSetDevice(c->device));
        size_t budget = c->scratch_bytes, fr = 0, tot = 0;
        units = std::max(1, std::min(want, at_most));
        if (carve(nullptr, units) > budget) {
            HIPCHK(hipMemGetInfo(&fr, &tot));
            budget = std::max(budget, (size_t)(share * (double)(fr + budget)));
        }
        while (units > 1 && carve(nullptr, units) > budget) --units;
        bytes = carve(nullptr, units);
        if (bytes > c->scratch_bytes) {
            HIPCHK(hipStreamSynchronize(c->stream));
            if (int rc = dev_free(c, c->scratch)) return rc;
            c->scratch = nullptr; c->scratch_bytes = 0;
            if (int rc = dev_alloc(c, &c->scratch, bytes)) { (void)hipGetLastError(); return rc; }
            c->scratch_bytes = bytes;
        }
        carve(c->scratch, units);
        return units;
    }
    bool out_of_memory() const { return bytes > c->scratch_bytes; }   // the buffer does not hold the planned layout
};

// ---- stack chunks: the walk of the frame-wise and pair-wise calls through the scratch arena --------
constexpr int PRE_MAX_FLIGHT = 16;        // units in flight when the caller leaves the number to the library
constexpr int PRE_MAX_WANT = 4096;        // ... and at most when it does not (grid z)

// One call of the adaptive threshold, CLAHE, the resize, Farnebaeck's flow, the result filter, the comparison of two results
// or the Liu-Shen flow over a stack of `n` units (frames or pairs), on the stack of that call: the call declares
// its regions into the arena sc, plan() sizes the chunk and carves the buffer, range() reduces a stack, run() walks the chunks.
// An input holds one frame per unit, or - a pair stack - one more: pair k reads frames k and k + 1, so a chunk of nf pairs reads
// nf + 1.  What a staged input holds is recorded here alone: nothing staged outlives the call.
struct FrameChunks {
    struct In { const double* stack; double* slot; int extra, k0, nf; };   // _host: slot holds frames [k0, k0 + nf + extra) of stack (nf 0: nothing)
    struct Out { char* caller; size_t bytes; char* slot; };        // bytes per unit
    vof_ctx* const c; const char* const what;                      // what: the call, for messages
    const int n, want; const bool host;                            // units; the caller's frames_in_flight
    const size_t fs;                                               // doubles per unit of an input stack
    Scratch sc;
    int cap = 0;                                                   // units in flight (plan)
    PpRange* part = nullptr;                                       // the range reduction's partial records, then its result
    double rg[3] = {};                                             // ... and what range() found
    static constexpr int MAX_IN = 6, MAX_OUT = 3;                  // the comparison of two results reads six stacks
    In in[MAX_IN] = {}; Out out[MAX_OUT] = {}; int n_in = 0, n_out = 0;

    FrameChunks(vof_ctx* c_, const char* what_, int n_, int want_, bool host_) : c(c_), what(what_), n(n_), want(want_), host(host_), fs(frame_stride(c_)), sc(c_) {
        sc.once(&part, (size_t)PP_RANGE_BLOCKS + 1);
    }

    // what every frame-wise entry point checks first
    static int check(vof_ctx* c, std::initializer_list<const void*> pointers, int n, const char* n_name) {
        if (!c) return -1;
        for (const void* p : pointers) if (!p) { c->err = "NULL pointer"; return -1; }
        if (n < 1) { c->err = std::string(n_name) + " must be >= 1"; return -1; }
        return 0;
    }

    void input(const double* stack, bool pairs = false) {          // fs doubles per frame; pairs: a pair stack; _host: staged
        if (host && pairs) sc.per_unit_plus_one(&in[n_in].slot, fs);
        else if (host) sc.per_unit(&in[n_in].slot, fs);
        in[n_in].extra = pairs ? 1 : 0;
        in[n_in++].stack = stack;
    }
    void output(void* caller, size_t unit_bytes) {                 // _host: staged, then copied to `caller`
        if (host) sc.per_unit(&out[n_out].slot, unit_bytes);
        out[n_out].caller = (char*)caller; out[n_out++].bytes = unit_bytes;
    }

    // the chunk size - `want`, or 16 where that is left to the library, within a quarter of the free device memory - and the arena
    int plan() {
        const int rc = sc.plan(want > 0 ? want : PRE_MAX_FLIGHT, std::min(PRE_MAX_WANT, n), 0.25);
        if (rc < 0 && sc.out_of_memory())
            c->err = std::string(what) + ": no device memory for " + std::to_string(sc.bytes >> 20) + " MiB of scratch (" +
                     std::to_string(sc.units) + " frame(s) in flight): " + c->err;
        cap = rc;
        return rc < 0 ? rc : 0;
    }

    // Units [k0, k0 + nf) of input s on the device: the caller's own memory, or the slot - uploaded unless it holds exactly these
    int staged(int s, int k0, int nf, const double** p) {
        In& i = in[s];
        *p = host ? i.slot : i.stack + (size_t)k0 * fs;
        if (!host || (i.nf == nf && i.k0 == k0)) return 0;
        if (int rc = h2d_bounced(c, i.slot, i.stack + (size_t)k0 * fs, (size_t)(nf + i.extra) * fs * sizeof(double))) return rc;
        i.k0 = k0; i.nf = nf;
        return 0;
    }

    // rg = (max, min of the finite values, non-finite count) of the whole of input s (_host: chunk by chunk through its slot), to
    // `report` too if there is one; then return code 1 and the message if anything is non-finite or outside the permitted [lo, hi]
    int range(int s, double lo, double hi, const char* outside, const char* note = "", double* report = nullptr) {
        PpRange* const rng = part + PP_RANGE_BLOCKS;
        PpRange acc{-INFINITY, INFINITY, 0};
        const int chunk = host ? cap : n;
        for (int k0 = 0; k0 < n; k0 += chunk) {
            const int nf = std::min(chunk, n - k0);
            const double* src;
            if (int rc = staged(s, k0, nf, &src)) return rc;
            const size_t m = (size_t)nf * fs;
            const int nb = (int)std::min<size_t>(PP_RANGE_BLOCKS, (m + 8 * PP_BLOCK - 1) / (8 * PP_BLOCK));
            c->cur_units = nf;
            {
                Prof prof(c, VOF_K_PREPROCESS, PP_ST_RANGE, 8.0 * fs);
                k_pp_range<<<nb, PP_BLOCK, 0, c->stream>>>(src, m, part);
                k_pp_range_final<<<1, 64, 0, c->stream>>>(part, nb, rng);
            }
            HIPCHK(hipGetLastError());
            PpRange r;
            if (int rc = d2h_bounced(c, &r, rng, sizeof r)) return rc;
            acc.vmax = std::max(acc.vmax, r.vmax); acc.vmin = std::min(acc.vmin, r.vmin); acc.bad += r.bad;
        }
        rg[0] = acc.vmax; rg[1] = acc.vmin; rg[2] = (double)acc.bad;
        if (report) memcpy(report, rg, sizeof rg);
        const char* found = rg[2] > 0 ? "non-finite values" : (rg[1] < lo || rg[0] > hi ? outside : nullptr);
        if (!found) return 0;
        c->err = std::string(what) + ": the movie holds " + found + note;
        return 1;
    }

    // The chunks in turn: body(k0, nf, inputs, outputs) enqueues the kernels of units [k0, k0 + nf) - device pointers, one per
    // declared input and output - and returns 0; _host: the outputs are then copied to the caller's arrays.
    template <class Body>
    int run(Body&& body) {
        for (int k0 = 0; k0 < n; k0 += cap) {
            const int nf = std::min(cap, n - k0);
            const double* src[MAX_IN] = {}; void* dst[MAX_OUT] = {};
            for (int s = 0; s < n_in; ++s) if (int rc = staged(s, k0, nf, &src[s])) return rc;
            for (int a = 0; a < n_out; ++a) dst[a] = host ? out[a].slot : out[a].caller + (size_t)k0 * out[a].bytes;
            c->cur_units = nf;
            if (int rc = body(k0, nf, src, dst)) return rc;
            HIPCHK(hipGetLastError());
            for (int a = 0; host && a < n_out; ++a)
                if (int rc = d2h_bounced(c, out[a].caller + (size_t)k0 * out[a].bytes, dst[a], (size_t)nf * out[a].bytes)) return rc;
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
};

// (count, mean, M2 = sum (x - mean)^2) of one chunk, exact two-pass; chunks are merged with Chan's formula
struct Moments {
    double n = 0, mean = 0, m2 = 0;
    void merge(double nb, double meanb, double m2b) {
        if (nb == 0) return;
        double nt = n + nb, d = meanb - mean;
        m2 += m2b + d * d * n * nb / nt;
        mean += d * nb / nt;
        n = nt;
    }
};

// ---- sweeps of the box flow: what vary_boxsize and vary_blursize share --------------------------------------------
constexpr int BS_MAX_CHUNK = 32;          // pairs per launch (grid z) at most; more adds nothing once the chip is full

// Mean and variance of a field per list entry, shared by the box-size and the blur sweep: the two-pass reduction of
// vof_field_moments_dev per pair on the device, sums [field][pass][entry][pair][3]; a pair is the unit the host merges.
struct PairMoments {
    double* d_mom; double* d_part;        // device: the sums; the partials of one chunk
    size_t n_mom;                         // n_entries * P * 3
    int n_entries, P, mom_blk;
};

inline int pair_moments_blocks(size_t fs) { return (int)std::min<size_t>(256, std::max<size_t>(1, (fs + 4 * RBLK - 1) / (4 * RBLK))); }

// pairs k0 .. k0 + np of entry b, enqueued behind the kernels that wrote x: no host round trip in a sweep
static void pair_moments_enqueue(vof_ctx* c, const PairMoments& m, const double* x, size_t fs, int field, int b, int k0, int np) {
    const dim3 gm(m.mom_blk, np);
    double* first = m.d_mom + ((size_t)(2 * field) * m.n_entries * m.P + (size_t)b * m.P + k0) * 3;
    double* second = first + m.n_mom;
    Prof prof(c, VOF_K_REDUCE, 0, 16.0 * fs);
    k_bs_moments<<<gm, RBLK, 0, c->stream>>>(x, fs, nullptr, m.d_part);
    k_sum3<<<np, 64, 0, c->stream>>>(m.d_part, m.mom_blk, first);
    k_bs_moments<<<gm, RBLK, 0, c->stream>>>(x, fs, first, m.d_part);
    k_sum3<<<np, 64, 0, c->stream>>>(m.d_part, m.mom_blk, second);
}

// mom: the host copy of d_mom.  Pairs merged in order with Chan's formula; per pair the arithmetic of chunk_moments
static Moments pair_moments_merged(const PairMoments& m, const double* mom, size_t fs, int field, int b) {
    Moments acc;
    const double* first = mom + ((size_t)(2 * field) * m.n_entries * m.P + (size_t)b * m.P) * 3;
    const double* second = first + m.n_mom;
    const double n = (double)fs;
    for (int k = 0; k < m.P; ++k) {
        double mean = first[3 * k] / n;
        const double s0 = second[3 * k], s1 = second[3 * k + 1];
        mean += s0 / n;                                         // first-order correction of the rounded mean
        acc.merge(n, mean, s1 - s0 * s0 / n);
    }
    return acc;
}

// what every sweep is asked for besides its list
struct SweepBase {
    const double* movie; int n_frames;
    double delta_x, delta_t; int remodel, quirks;
    const double* edges; int bins; int64_t* hist;               // speed
    const int32_t* probe_ij; int n_probes; double* probe_out;
    double* outs[4];                      // v_x, v_y, speed, net_remodelling: all NULL = stats only
    bool host;                            // movie and outs are host memory
};

static int sweep_check(vof_ctx* c, const SweepBase& r, const void* stats) {
    if (!r.movie) { c->err = "movie is NULL"; return -1; }
    if (!stats) { c->err = "stats is NULL"; return -1; }
    if (r.n_frames < 2) { c->err = "need at least two frames"; return -1; }
    if (r.delta_t == 0.0) { c->err = "delta_t must not be 0"; return -1; }
    if (r.edges && (r.bins < 1 || !r.hist)) { c->err = "histogram_edges needs histogram_bins >= 1 and histograms"; return -1; }
    if (r.edges && !(r.edges[r.bins] > r.edges[0])) { c->err = "histogram_edges must increase"; return -1; }
    if (r.probe_ij) {
        if (r.n_probes < 1 || !r.probe_out) { c->err = "probe_ij needs n_probes >= 1 and probe_speeds"; return -1; }
        for (int l = 0; l < r.n_probes; ++l)
            if (r.probe_ij[2 * l] < 0 || r.probe_ij[2 * l] >= c->Ni || r.probe_ij[2 * l + 1] < 0 || r.probe_ij[2 * l + 1] >= c->Nj) {
                c->err = "probe outside the image"; return -1;
            }
    }
    const bool any = r.outs[0] || r.outs[1] || r.outs[2] || r.outs[3];
    if (any && (!r.outs[0] || !r.outs[1] || !r.outs[2])) { c->err = "v_x, v_y and speed must be given together (or all NULL)"; return -1; }
    if (any && r.remodel && !r.outs[3]) { c->err = "net_remodelling is NULL with include_remodelling"; return -1; }
    return 0;
}

// pairs a sweep keeps in flight at most: a _host sweep stages no more than the context's slots
inline int sweep_want(const vof_ctx* c, const SweepBase& r) {
    return std::min(std::min(r.n_frames - 1, BS_MAX_CHUNK), r.host ? c->B : BS_MAX_CHUNK);
}

// where the fields of pairs k0 .. of entry b go on the device: the caller's stacks (_dev with fields) or the chunk planes
struct SweepDst {
    double* f[4];
    size_t oo;                            // offset of the chunk in the caller's stacks
    bool keep_v, keep_g;                  // v_x / v_y and net_remodelling are wanted (speed always is)
};

static SweepDst sweep_dst(const SweepBase& r, double* const chunk_out[4], size_t fs, int b, int k0) {
    SweepDst d;
    const bool fields = r.outs[0] != nullptr;
    d.oo = ((size_t)b * (r.n_frames - 1) + k0) * fs;
    for (int f = 0; f < 4; ++f) d.f[f] = (fields && !r.host && r.outs[f]) ? r.outs[f] + d.oo : chunk_out[f];
    d.keep_v = fields;
    d.keep_g = r.remodel || (fields && !r.host && r.outs[3]);      // _host zero-fills on the host
    return d;
}

// _host with fields: np pairs from the chunk planes into the caller's stacks; net_remodelling is zero where it was not computed
static int sweep_copy_out(vof_ctx* c, const SweepBase& r, const SweepDst& d, size_t fs, int np) {
    if (!r.host) return 0;
    const size_t bytes = (size_t)np * fs * sizeof(double);
    for (int f = 0; f < 4; ++f) {
        if (!r.outs[f]) continue;
        if (f == 3 && !r.remodel) memset(r.outs[f] + d.oo, 0, bytes);
        else if (int rc = d2h_bounced(c, r.outs[f] + d.oo, d.f[f], bytes)) return rc;
    }
    return 0;
}

// The statistics every sweep keeps per list entry: histogram and non-finite count of the speed, the speed at the probes, mean
// and variance of speed and net_remodelling.  What the kernels read and write are regions of the sweep's arena.  The counters
// - the tail's, then the sweep's own - are the last regions the sweep declares: one span from d_bad to the arena's end, zeroed
// by one memset and brought back by one copy.
struct SweepTail {
    const SweepBase* r; const char* name;
    int n; size_t fs;
    PairMoments pm;
    size_t n_hist, n_probe, n_mom_all;
    double *d_edges, *d_probe;
    unsigned long long *d_bad, *d_hist;
    int32_t* d_pij;
    std::vector<unsigned long long> counters;     // host copy of the span (sweep_tail_finish)
    const unsigned long long* host(const unsigned long long* dev) const { return counters.data() + (dev - d_bad); }
};

// declares the tail's regions, the counters last: the sweep's own counters follow, everything else of the sweep comes before
static void sweep_tail_regions(Scratch& sc, SweepTail& t, const SweepBase& r, const char* name, int n) {
    const int P = r.n_frames - 1;
    t.r = &r; t.name = name; t.n = n; t.fs = frame_stride(sc.c);
    t.n_hist = r.edges ? (size_t)n * r.bins : 0;
    t.n_probe = r.probe_ij ? (size_t)n * P * r.n_probes : 0;
    // moments: per field (speed, net_remodelling), pass, entry and pair the three sums of k_sum3; then the partials of a chunk
    const size_t n_mom = (size_t)n * P * 3;
    t.n_mom_all = 2 * (r.remodel ? 2 : 1) * n_mom;
    t.pm = PairMoments{nullptr, nullptr, n_mom, n, P, pair_moments_blocks(t.fs)};
    sc.once(&t.d_edges, r.edges ? (size_t)r.bins + 1 : 0);
    sc.once(&t.d_probe, t.n_probe);
    sc.once(&t.pm.d_mom, t.n_mom_all);
    sc.per_unit(&t.pm.d_part, (size_t)3 * t.pm.mom_blk);
    sc.once(&t.d_pij, r.probe_ij ? (size_t)2 * r.n_probes : 0);
    sc.once(&t.d_bad, (size_t)n);
    sc.once(&t.d_hist, t.n_hist);
}

// Plans the sweep's arena, zeroes the counters and uploads edges and probes.  Returns the pairs in flight (1 .. sweep_want) or
// an error code (< 0); `unit`: what the planes of the message are counted for.
static int sweep_tail_begin(Scratch& sc, SweepTail& t, const char* unit) {
    vof_ctx* const c = sc.c;
    const SweepBase& r = *t.r;
    const int cap = sc.plan(sweep_want(c, r), r.n_frames - 1, 0.8);
    if (cap < 0 && sc.units == 1 && sc.out_of_memory()) {       // not even one pair fits; a failed allocation of more stays what it is
        c->err = std::string("the ") + t.name + " does not fit into the free device memory (" +
                 std::to_string(sc.bytes / (t.fs * sizeof(double))) + " planes of n_i x n_j doubles" + unit + ")";
        return -3;
    }
    if (cap < 0) return cap;
    t.counters.resize((size_t)(c->scratch + sc.bytes - (char*)t.d_bad) / 8);
    if (hipMemsetAsync(t.d_bad, 0, t.counters.size() * 8, c->stream) != hipSuccess) { c->err = "memset failed"; return -2; }
    if (r.edges) if (int rc = h2d_bounced(c, t.d_edges, r.edges, (size_t)(r.bins + 1) * 8)) return rc;
    if (r.probe_ij) if (int rc = h2d_bounced(c, t.d_pij, r.probe_ij, (size_t)2 * r.n_probes * sizeof(int32_t))) return rc;
    return cap;
}

// pairs k0 .. k0 + np of entry b, enqueued behind the kernels that wrote them: first the counts and the probes of the speed ...
static void sweep_tail_speed(vof_ctx* c, const SweepTail& t, int b, int k0, int np, const double* speed) {
    const SweepBase& r = *t.r;
    Prof prof(c, VOF_K_REDUCE, 0);
    const size_t m = (size_t)np * t.fs;
    const int nb = (int)std::min<size_t>(1024, (m + 4 * 256 - 1) / (4 * 256));
    k_bs_counts<<<nb, 256, 0, c->stream>>>(speed, m, t.d_edges, r.edges ? r.bins : 0, r.edges ? t.d_hist + (size_t)b * r.bins : nullptr,
                                           t.d_bad + b);
    if (r.probe_ij) {
        const int nt = np * r.n_probes;
        k_bs_probe<<<(nt + 255) / 256, 256, 0, c->stream>>>(speed, t.fs, c->Nj, np, t.d_pij, r.n_probes,
                                                            t.d_probe + ((size_t)b * t.pm.P + k0) * r.n_probes);
    }
}

// ... then, behind whatever the sweep adds on the same fields, the moments; asks for the error of the chunk's launches
static int sweep_tail_moments(vof_ctx* c, const SweepTail& t, int b, int k0, int np, const double* speed, const double* gamma) {
    const SweepBase& r = *t.r;
    pair_moments_enqueue(c, t.pm, speed, t.fs, 0, b, k0, np);
    if (r.remodel) pair_moments_enqueue(c, t.pm, gamma, t.fs, 1, b, k0, np);
    if (hipGetLastError() != hipSuccess) { c->err = std::string(t.name) + ": launch failed"; return -2; }
    return 0;
}

// waits for the sweep, brings the statistics back and fills the fields the two stats records share
template <class Stats>
static int sweep_tail_finish(vof_ctx* c, SweepTail& t, Stats* stats) {
    const SweepBase& r = *t.r;
    if (int rc = d2h_bounced(c, t.counters.data(), t.d_bad, t.counters.size() * 8)) return rc;
    if (r.probe_ij) if (int rc = d2h_bounced(c, r.probe_out, t.d_probe, t.n_probe * 8)) return rc;
    std::vector<double> mom(t.n_mom_all);
    if (int rc = d2h_bounced(c, mom.data(), t.pm.d_mom, mom.size() * 8)) return rc;
    if (hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "stream synchronize failed"; return -2; }
    for (size_t i = 0; i < t.n_hist; ++i) r.hist[i] = (int64_t)t.host(t.d_hist)[i];
    for (int b = 0; b < t.n; ++b) {
        Stats& o = stats[b];
        memset(&o, 0, sizeof o);
        const Moments ms = pair_moments_merged(t.pm, mom.data(), t.fs, 0, b);
        o.speed_mean = ms.mean; o.speed_variance = ms.m2 / ms.n;
        if (r.remodel) {
            const Moments mr = pair_moments_merged(t.pm, mom.data(), t.fs, 1, b);
            o.remodelling_mean = mr.mean; o.remodelling_variance = mr.m2 / mr.n;
        }
        o.nonfinite_count = (int64_t)t.host(t.d_bad)[b];
    }
    return 0;
}

}  // namespace

extern "C" {

// Entries [a, b) of `list` (pairs of the stack) as one phase of the two-phase solve on context or lane c, in batches of its
// slots.  Phase 1 saves each solution in warm_x at the pair's position in the list and marks it in sync.usable; phase 2 starts
// every pair from the saved solution of its nearest phase-1 neighbour (whose phase 1 the caller has waited for).
static int two_phase_part(vof_ctx* c, const double* movie, const std::vector<int>& list, size_t a, size_t b, bool phase2, int stride,
                          GroupSync& sync, double* v_x, double* v_y, double* remodelling, double* speed, vof_pair_stats* stats) {
    const vof_params prm = c->prm;
    const size_t len = 3 * c->L[0].npts;
    const int cap = batch_slots(c);
    const int n1 = (int)sync.usable.size();
    std::vector<PairParam> hp((size_t)cap);
    std::vector<int> hsrc((size_t)cap);
    std::vector<vof_pair_stats> st((size_t)cap);
    for (size_t o = a; o < b; o += (size_t)cap) {
        const int np = (int)std::min<size_t>((size_t)cap, b - o);
        {
            std::lock_guard<std::mutex> lk(sync.m);
            for (int i = 0; i < np; ++i) {
                const int k = list[o + i];
                hp[i] = PairParam{prm.speed_alpha, prm.remodelling_alpha, k, k};
                const int src = std::min((k + stride / 2) / stride, n1 - 1);
                hsrc[i] = phase2 && sync.usable[src] ? src : -1;   // -1: constant initial fields (a failed pair must not poison its neighbours)
            }
        }
        if (int rc = solve_batch(c, BatchReq{movie, np, hp.data(), phase2 ? hsrc.data() : nullptr, false, v_x, v_y, remodelling, speed, st.data()}))
            return rc;
        if (!phase2) {
            HIPCHK(hipMemcpyAsync(c->warm_x + o * len, c->kx, (size_t)np * len * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            std::lock_guard<std::mutex> lk(sync.m);
            for (int i = 0; i < np; ++i) sync.usable[o + i] = st[i].converged && std::isfinite(st[i].relative_residual);
        }
        if (stats)
            for (int i = 0; i < np; ++i) stats[list[o + i]] = st[i];
    }
    return 0;
}

// The groups of one lane (plan_groups), from the highest down: phase 1, publication, the wait for the next group's phase 1,
// phase 2.  `ev`: the parent's event per group.  Whatever happens, every group of the lane is published before this returns.
static int two_phase_lane(vof_ctx* c, int lane, const std::vector<LaneGroup>& groups, hipEvent_t* ev, GroupSync& sync, const double* movie,
                          const std::vector<int>& first, const std::vector<int>& rest, int stride, double* v_x, double* v_y,
                          double* remodelling, double* speed, vof_pair_stats* stats) {
    const int ng = (int)groups.size();
    auto publish = [&](int g, bool ok) {
        {
            std::lock_guard<std::mutex> lk(sync.m);
            if (sync.state[g]) return;
            if (!ok) for (int o = groups[g].lo; o < groups[g].hi; ++o) sync.usable[o] = 0;
            sync.state[g] = ok ? 1 : -1;
        }
        sync.cv.notify_all();
    };
    auto run_group = [&](int g) -> int {
        const LaneGroup& G = groups[g];
        if (int rc = two_phase_part(c, movie, first, (size_t)G.lo, (size_t)G.hi, false, stride, sync, v_x, v_y, remodelling, speed, stats)) return rc;
        HIPCHK(hipEventRecord(ev[g], c->stream));   // behind the last copy into warm_x
        publish(g, true);
        if (g + 1 < ng) {   // the source of this group's last warm pairs: the first phase-1 pair of the next group
            int state;
            {
                std::unique_lock<std::mutex> lk(sync.m);
                if (!sync.cv.wait_for(lk, std::chrono::seconds(60), [&] { return sync.state[g + 1] != 0; })) {
                    c->err = "timed out waiting for the phase-1 solutions of the next pair group";
                    return -2;
                }
                state = sync.state[g + 1];
            }
            if (state > 0) HIPCHK(hipStreamWaitEvent(c->stream, ev[g + 1], 0));
        }
        // the group's warm pairs: those of `rest` between its first phase-1 pair and the next group's
        const size_t ra = (size_t)(std::lower_bound(rest.begin(), rest.end(), G.lo * stride) - rest.begin());
        const size_t rb = g + 1 < ng ? (size_t)(std::lower_bound(rest.begin(), rest.end(), G.hi * stride) - rest.begin()) : rest.size();
        return two_phase_part(c, movie, rest, ra, rb, true, stride, sync, v_x, v_y, remodelling, speed, stats);
    };
    int rc = 0;
    for (int g = ng - 1; g >= 0 && !rc; --g)
        if (groups[g].lane == lane) rc = run_group(g);
    for (int g = 0; g < ng; ++g)
        if (groups[g].lane == lane) publish(g, false);   // (what is published already stays as it is)
    return rc;
}

// Two-phase solve of a stack with warm starts (the reference warm-starts pair k from pair k-1, OF.py:803-806, which
// serialises the pairs; here every stride-th pair is solved first from the constant initial fields, then all the others
// start from the solution of their nearest solved neighbour).  Pairs are addressed through the PairParam table
// (frame / output slot), so both phases are ordinary batches.  With several lanes the stack is cut into groups of pairs and a
// lane runs both phases of its groups without meeting the others (plan_groups, GroupSync); the lanes join once, at the end.
static int solve_stack_two_phase(vof_ctx* c, const double* movie, int P, double* v_x, double* v_y, double* remodelling,
                                 double* speed, vof_pair_stats* stats, int stride, int lanes) {
    const size_t len = 3 * c->L[0].npts;
    const int B = c->B;
    std::vector<int> first, rest;
    for (int k = 0; k < P; ++k) (k % stride == 0 ? first : rest).push_back(k);
    const int n1 = (int)first.size();
    // (the lanes are copies of the context that allocate nothing: the tables' device storage has to exist before they are made)
    if (!c->pp_buf) { if (int rc = dev_alloc(c, &c->pp_buf, (size_t)B)) return rc; }
    if (!c->warm_src) { if (int rc = dev_alloc(c, &c->warm_src, (size_t)B)) return rc; }
    if (c->warm_cap < (size_t)n1 * len) {
        if (int rc = dev_free(c, c->warm_x)) return rc;   // (round 2 kept every outgrown buffer until vof_destroy)
        c->warm_x = nullptr; c->warm_cap = 0;
        if (int rc = dev_alloc(c, &c->warm_x, (size_t)n1 * len)) return rc;
        c->warm_cap = (size_t)n1 * len;
    }
    GroupSync sync;
    sync.usable.assign((size_t)n1, 0);
    int rc = LANES_NO_THREAD;
    if (lanes > 1) {
        const std::vector<LaneGroup> groups = plan_groups(c, n1, lanes, lane_groups_wanted());
        sync.state.assign(groups.size(), 0);
        for (size_t g = 0; g < groups.size(); ++g)
            if (!c->group_ev[g]) HIPCHK(hipEventCreateWithFlags(&c->group_ev[g], hipEventDisableTiming));
        rc = run_lanes(c, lanes, [&](vof_ctx* L, int i) {
            return two_phase_lane(L, i, groups, c->group_ev, sync, movie, first, rest, stride, v_x, v_y, remodelling, speed, stats);
        }, true);
    }
    if (rc == LANES_NO_THREAD) {   // one lane: all of phase 1, then all of phase 2, on the context's stream
        for (int phase = 0; phase < 2; ++phase) {
            const std::vector<int>& list = phase ? rest : first;
            if ((rc = two_phase_part(c, movie, list, 0, list.size(), phase == 1, stride, sync, v_x, v_y, remodelling, speed, stats))) return rc;
        }
    }
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Solve the listed pairs (frame index / output slot relative to `frames`, v_x ...) with the direct preconditioner, in batches
// of what its buffers hold.  stats: per list entry.
static int direct_solve_list(vof_ctx* c, const double* frames, const std::vector<PairParam>& items, double* v_x, double* v_y,
                             double* remodelling, double* speed, vof_pair_stats* stats) {
    if (items.empty()) return 0;
    const int cap = direct_capacity(c, std::min<int>(c->B, (int)items.size()));
    if (cap < 1) { c->err = "the direct preconditioner does not fit into the free device memory (3 n_j x 3 n_j doubles per image row and pair)"; return -3; }
    if (int rc = direct_alloc(c, cap)) return rc;
    std::vector<vof_pair_stats> st((size_t)c->dir_cap);
    for (size_t o = 0; o < items.size(); o += (size_t)c->dir_cap) {
        const int np = (int)std::min<size_t>((size_t)c->dir_cap, items.size() - o);
        if (int rc = solve_batch(c, BatchReq{frames, np, items.data() + o, nullptr, true, v_x, v_y, remodelling, speed, st.data()})) return rc;
        if (stats)
            for (int i = 0; i < np; ++i) stats[o + i] = st[i];
    }
    return 0;
}

// Preconditioner 2 ("auto"), after the multigrid attempt on the n pairs of `table` (nullptr: pair k = frame k, the context's
// alphas) whose records are in stats: those it left unconverged once more with the direct preconditioner, if that fits.
static int resolve_unconverged(vof_ctx* c, const double* frames, const PairParam* table, int n, double* const* outs, vof_pair_stats* stats) {
    if (c->prm.preconditioner != 2 || !stats) return 0;   // (without the first attempt's records there is nothing to select by)
    std::vector<PairParam> items;
    std::vector<int> which;
    for (int k = 0; k < n; ++k)
        if (!stats[k].converged && std::isfinite(stats[k].relative_residual)) {   // a NaN frame stays a reported failure
            items.push_back(table ? table[k] : PairParam{c->prm.speed_alpha, c->prm.remodelling_alpha, k, k});
            which.push_back(k);
        }
    if (items.empty() || !direct_ok_for_fallback(c)) return 0;
    std::vector<vof_pair_stats> st(items.size());
    if (int rc = direct_solve_list(c, frames, items, outs[0], outs[1], outs[2], outs[3], st.data())) {
        if (rc != -3) return rc;     // -3: no room: keep the reported non-convergence
        c->err.clear();
        return 0;
    }
    for (size_t i = 0; i < which.size(); ++i) {
        const vof_pair_stats& first = stats[which[i]];
        st[i].iterations += first.iterations;                                                   // Krylov steps of both attempts
        st[i].batch_ms += first.batch_ms / std::max(1, first.batch_pairs) * st[i].batch_pairs;   // and their time (per-pair share kept)
        stats[which[i]] = st[i];
    }
    return 0;
}

// Solve pairs 0 .. P-1 of a device-resident range of frames (P <= any size): two-phase warm start when it pays, plain
// batches otherwise.  Outputs are indexed by the pair's position in the range.
// preconditioner 1: every pair with the direct preconditioner; 2 (default): the multigrid cycle, and the pairs it leaves
// unconverged (the grad-div dominated regimes) once more with the direct preconditioner if that fits.
// allow_lanes: the multigrid solve may run as concurrent lanes (lanes_for); the direct solves always run on c's stream.
static int solve_range_dev(vof_ctx* c, const double* frames, int P, double* v_x, double* v_y, double* remodelling,
                           double* speed, vof_pair_stats* stats, bool allow_lanes) {
    const vof_params prm = c->prm;
    const int stride = prm.warm_start_stride;
    const size_t fs = frame_stride(c);
    if (direct_only(c)) {
        std::vector<PairParam> items((size_t)P);
        for (int k = 0; k < P; ++k) items[k] = PairParam{prm.speed_alpha, prm.remodelling_alpha, k, k};
        return direct_solve_list(c, frames, items, v_x, v_y, remodelling, speed, stats);
    }
    std::vector<vof_pair_stats> local;
    if (!stats && prm.preconditioner == 2) { local.resize((size_t)P); stats = local.data(); }   // the fallback needs the flags
    // two phases double the latency-bound part of a solve (set-up, small coarse levels): worth it once the first phase
    // alone keeps the chip busy (>= 16 Mpixel of frame pairs; measured: 128^2 x 8 loses 45 %, 512^2 x 64 is neutral,
    // 1024^2 x 129 gains 22 %)
    if (stride > 1 && P >= 2 * stride && (double)(P / stride) * (double)c->Ni * (double)c->Nj >= 16e6) {
        const int lanes = allow_lanes ? lanes_for(c, (P + stride - 1) / stride) : 1;
        if (int rc = solve_stack_two_phase(c, frames, P, v_x, v_y, remodelling, speed, stats, stride, lanes)) return rc;
    } else {
        auto plain = [&](vof_ctx* L, int a, int b) -> int {   // pairs [a, b) in batches of L's slots
            for (int k0 = a; k0 < b; k0 += batch_slots(L)) {
                int np = std::min(batch_slots(L), b - k0);
                const size_t o = (size_t)k0 * fs;
                if (int rc = solve_batch(L, BatchReq{frames + o, np, nullptr, nullptr, false, v_x + o, v_y + o, remodelling + o,
                                                     speed ? speed + o : nullptr, stats ? stats + k0 : nullptr})) return rc;
            }
            return 0;
        };
        const int lanes = allow_lanes ? lanes_for(c, P) : 1;
        if (lanes <= 1) {
            if (int rc = plain(c, 0, P)) return rc;
        } else if (int rc = run_lanes(c, lanes, [&](vof_ctx* L, int i) { return plain(L, (int)((long)P * i / lanes), (int)((long)P * (i + 1) / lanes)); })) {
            return rc;
        }
    }
    double* const outs[4] = {v_x, v_y, remodelling, speed};
    return resolve_unconverged(c, frames, nullptr, P, outs, stats);
}

int vof_solve_stack_dev(vof_ctx* c, const double* movie, int n_frames, const vof_params* p, double* v_x, double* v_y,
                        double* remodelling, double* speed, vof_pair_stats* stats) {
    if (!c) return -1;
    if (!movie || !v_x || !v_y || !remodelling) { c->err = "NULL array pointer"; return -1; }
    if (n_frames < 2) { c->err = "need at least two frames"; return -1; }
    if (int rc = check_params(c, p)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = solve_range_dev(c, movie, n_frames - 1, v_x, v_y, remodelling, speed, stats, true)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Device staging of the host API: frames of one batch (+1) and TWO sets of output buffers, so that the device-to-host
// copies of batch k (copy stream) overlap the solve of batch k+1 (main stream).  st_* serve vof_solve_stack_host,
// vof_vary_regularisation_host, vof_debug_setup and - its chunks are the context's pairs - vof_box_flow_host; every other call
// stages through its arena.
static int ensure_staging(vof_ctx* c, bool double_buffer) {
    const size_t fs = frame_stride(c);
    if (!c->st_movie) {
        if (int rc = dev_alloc(c, &c->st_movie, (size_t)(c->B + 1) * fs)) return rc;
        for (int i = 0; i < 4; ++i)
            if (int rc = dev_alloc(c, &c->st_out[i], (size_t)c->B * fs)) return rc;
    }
    if (double_buffer && !c->st_out2[0]) {
        for (int i = 0; i < 4; ++i)
            if (int rc = dev_alloc(c, &c->st_out2[i], (size_t)c->B * fs)) return rc;
        if (int rc = dev_alloc(c, &c->st_movie2, (size_t)(c->B + 1) * fs)) return rc;
        HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIPCHK(hipEventCreateWithFlags(&c->ev_solved[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->ev_copied[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->ev_uploaded[i], hipEventDisableTiming));
        }
    }
    return 0;
}

int vof_solve_stack_host(vof_ctx* c, const double* movie, int n_frames, const vof_params* p, double* v_x,
                         double* v_y, double* remodelling, double* speed, vof_pair_stats* stats) {
    if (!c) return -1;
    if (!movie || !v_x || !v_y || !remodelling) { c->err = "NULL array pointer"; return -1; }
    if (n_frames < 2) { c->err = "need at least two frames"; return -1; }
    if (int rc = check_params(c, p)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t fs = frame_stride(c);
    const int P = n_frames - 1;
    const bool multi = P > c->B;                       // more than one batch: overlap the copies with the solves
    if (int rc = ensure_staging(c, multi)) return rc;
    const std::vector<HostBatch> batches = plan_host_batches(P, c->B);
    const int nb = (int)batches.size();
    // Pageable host-to-device copies run at ~2 GB/s on this platform, pinned ones at ~55 GB/s: the caller's movie is
    // pinned in place for the duration of the call (0.04 s/GB) - the frames of the first batch right away, the rest by a
    // helper thread while the first batch is solved (plan_movie_split).  Unpinned parts fall back to pageable copies.
    const char* mbase = (const char*)movie;
    const size_t movie_bytes = (size_t)n_frames * fs * sizeof(double);
    const size_t split = plan_movie_split((uintptr_t)mbase, movie_bytes, (size_t)(batches[0].np + 1) * fs * sizeof(double), nb == 1);
    const bool htrace = getenv("VOF_TRACE_HOST") != nullptr;
    const auto ht0 = std::chrono::steady_clock::now();
    auto hmark = [&](const char* what) {
        if (htrace) fprintf(stderr, "[vof host] %8.1f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ht0).count(), what);
    };
    HostPin pin_a(mbase, split), pin_b;
    hmark(pin_a.ok() ? "first movie part pinned" : "first movie part not pinned: pageable copies");
    double* outs[4] = {v_x, v_y, remodelling, speed};
    const size_t out_bytes = (size_t)P * fs * sizeof(double);
    std::vector<std::thread> helpers;
    std::thread movie_helper;
    if (split < movie_bytes)
        movie_helper = std::thread([&pin_b, mbase, split, movie_bytes, dev = c->device]() {
            if (hipSetDevice(dev) == hipSuccess) pin_b = HostPin(mbase + split, movie_bytes - split);
        });
    // Freshly allocated output arrays (np.empty) are not resident yet: first-touch page faults would serialise with the
    // device-to-host copies (8.6 GB of fresh pages cost ~0.4 s).  The arrays are outputs - every byte is overwritten below -,
    // so a pool of helper threads touches their regions (plan_output_regions) IN BATCH ORDER while the GPU solves, and the
    // calling thread pins a batch's regions in place just before its copies (round 2 pinned each array whole and the first
    // batch's copies waited for all of it); arrays below 1 MB are only touched.  The copies of batch bi wait for batch bi's
    // regions alone.
    const bool pin_outputs = out_bytes >= ((size_t)1 << 20);   // pageable device-to-host copies can drop to ~2 GB/s
    const std::vector<HostRegion> regions = plan_output_regions(outs, batches, fs * sizeof(double), out_bytes);
    std::vector<HostPin> region_pins(regions.size());
    std::vector<std::atomic<int>> batch_ready((size_t)nb);
    for (auto& a : batch_ready) a.store(0);
    std::atomic<int> next_task{0};
    const int n_tasks = nb * 4;
    // The helpers only TOUCH the pages (plain stores: no runtime call, no lock shared with the launching thread - eight
    // threads inside hipHostRegister slowed the solver's kernel launches threefold); registering resident pages afterwards
    // takes ~2 ms per GB and is done by the calling thread just before the batch's copies.
    auto helper_body = [&regions, &batch_ready, &next_task, n_tasks]() {
        for (;;) {
            const int t = next_task.fetch_add(1);
            if (t >= n_tasks) return;
            const HostRegion& r = regions[(size_t)t];
            if (r.ptr && r.bytes) {
                volatile char* q = (volatile char*)r.ptr;
                for (size_t o = 0; o < r.bytes; o += 4096) q[o] = 0;
                q[r.bytes - 1] = 0;
            }
            batch_ready[(size_t)(t / 4)].fetch_add(1);
        }
    };
    {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const int n_helpers = (int)std::min<unsigned>(std::min<unsigned>(8u, hw), (unsigned)n_tasks);
        for (int t = 0; t < n_helpers; ++t) helpers.emplace_back(helper_body);
    }
    int regions_pinned_upto = 0;
    auto wait_batch_regions = [&](int bi) {   // every region of batch bi (and of the batches before it) is resident and pinned
        for (int b = 0; b <= bi; ++b)
            while (batch_ready[(size_t)b].load() < 4) std::this_thread::yield();
        for (; regions_pinned_upto <= bi; ++regions_pinned_upto)
            for (int i = 0; i < 4 && pin_outputs; ++i) {
                const size_t t = (size_t)regions_pinned_upto * 4 + i;
                if (regions[t].ptr && regions[t].bytes) region_pins[t] = HostPin(regions[t].ptr, regions[t].bytes);
            }
    };
    auto join_helpers = [&]() { for (auto& t : helpers) if (t.joinable()) t.join(); };
    auto fail_msg = [&](const char* what, hipError_t e) { c->err = std::string(what) + ": " + hipGetErrorString(e); return -2; };
    int rc_all = 0;
    double* frames_buf[2] = {c->st_movie, multi ? c->st_movie2 : c->st_movie};
    auto upload = [&](int bi, hipStream_t st) {   // frames k0 .. k0 + np of batch bi; a copy never straddles the two pinned regions
        const HostBatch& bt = batches[bi];
        const size_t o0 = (size_t)bt.k0 * fs * sizeof(double), o1 = o0 + (size_t)(bt.np + 1) * fs * sizeof(double);
        char* dst = (char*)frames_buf[bi & 1];
        hipError_t e = hipSuccess;
        if (o0 < split) e = hipMemcpyAsync(dst, mbase + o0, std::min(o1, split) - o0, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && o1 > split) {
            const size_t a = std::max(o0, split);
            e = hipMemcpyAsync(dst + (a - o0), mbase + a, o1 - a, hipMemcpyHostToDevice, st);
        }
        return e;
    };
    {
        hipError_t e = upload(0, c->stream);
        if (e != hipSuccess) rc_all = fail_msg("H2D copy failed", e);
    }
    for (int bi = 0; bi < nb && !rc_all; ++bi) {
        const HostBatch& bt = batches[bi];
        const int set = bi & 1;
        double** so = (multi && set) ? c->st_out2 : c->st_out;
        hipError_t e;
        if (bi + 1 < nb) {   // frames of the next batch: uploaded on the copy stream while this batch is solved
            if (movie_helper.joinable()) movie_helper.join();
            // its buffer was last read by batch bi - 1
            if (bi >= 1 && (e = hipStreamWaitEvent(c->copy_stream, c->ev_solved[(bi + 1) & 1], 0)) != hipSuccess) { rc_all = fail_msg("stream wait failed", e); break; }
            if ((e = upload(bi + 1, c->copy_stream)) != hipSuccess ||
                (e = hipEventRecord(c->ev_uploaded[(bi + 1) & 1], c->copy_stream)) != hipSuccess) { rc_all = fail_msg("H2D copy failed", e); break; }
        }
        if (bi > 0 && (e = hipStreamWaitEvent(c->stream, c->ev_uploaded[set], 0)) != hipSuccess) { rc_all = fail_msg("stream wait failed", e); break; }
        if (multi && bi >= 2 && (e = hipStreamWaitEvent(c->stream, c->ev_copied[set], 0)) != hipSuccess) {   // output set free again
            rc_all = fail_msg("stream wait failed", e);
            break;
        }
        int rc = solve_range_dev(c, frames_buf[set], bt.np, so[0], so[1], so[2], so[3], stats ? stats + bt.k0 : nullptr, false);
        if (rc) { rc_all = rc; break; }
        hmark("batch solved");
        wait_batch_regions(bi);
        hmark("output regions of the batch ready");
        hipStream_t cs = multi ? c->copy_stream : c->stream;
        if (multi) {
            if ((e = hipEventRecord(c->ev_solved[set], c->stream)) != hipSuccess ||
                (e = hipStreamWaitEvent(cs, c->ev_solved[set], 0)) != hipSuccess) { rc_all = fail_msg("event record failed", e); break; }
        }
        for (int i = 0; i < 4 && !rc_all; ++i)
            if (outs[i]) {
                // the batch's bytes [o0, o1) of array i: the part before region bi's first page lies in region bi - 1
                const size_t o0 = (size_t)bt.k0 * fs * sizeof(double), o1 = o0 + (size_t)bt.np * fs * sizeof(double);
                const size_t r0 = (size_t)(regions[(size_t)bi * 4 + i].ptr - (char*)outs[i]);
                const size_t cut = std::min(std::max(r0, o0), o1);
                if (cut > o0) {
                    e = hipMemcpyAsync((char*)outs[i] + o0, (const char*)so[i], cut - o0, hipMemcpyDeviceToHost, cs);
                    if (e != hipSuccess) { rc_all = fail_msg("D2H copy failed", e); break; }
                }
                if (o1 > cut) {
                    e = hipMemcpyAsync((char*)outs[i] + cut, (const char*)so[i] + (cut - o0), o1 - cut, hipMemcpyDeviceToHost, cs);
                    if (e != hipSuccess) rc_all = fail_msg("D2H copy failed", e);
                }
            }
        if (multi) {
            if (!rc_all && (e = hipEventRecord(c->ev_copied[set], cs)) != hipSuccess) rc_all = fail_msg("event record failed", e);
        } else if ((e = hipStreamSynchronize(c->stream)) != hipSuccess && !rc_all) rc_all = fail_msg("stream synchronize failed", e);
    }
    join_helpers();
    if (movie_helper.joinable()) movie_helper.join();
    hmark("all batches enqueued");
    if (multi && hipStreamSynchronize(c->copy_stream) != hipSuccess && !rc_all) { c->err = "copy stream synchronize failed"; rc_all = -2; }
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc_all) { c->err = "stream synchronize failed"; rc_all = -2; }
    hmark("copies done");
    for (auto& r : region_pins) r.release();   // in the order they always had: regions, first movie part, second
    pin_a.release();
    pin_b.release();
    hmark("unpinned");
    return rc_all;
}

// workspace of the blur of up to `frames` frames per blur_frames call, declared into the caller's arena: one chunk of
// row-filtered frames, and room for the taps of `radius` where the caller does not bring its own (w null)
constexpr int BLUR_CHUNK = 16;
static void blur_regions(Scratch& sc, int frames, double** tmp, double** w = nullptr, int radius = 0) {
    sc.once(tmp, (size_t)std::min(frames, BLUR_CHUNK) * frame_stride(sc.c));
    if (w) sc.once(w, (size_t)2 * radius + 1);
}

// n_frames device-resident frames with the taps already on the device at w and the row-filtered chunk at tmp (blur_regions),
// enqueued on the context's stream (out may alias in).  Radii BL_RMIN .. BL_RMAX take the LDS-tiled kernels, same bits as k_blur1d.
static int blur_frames(vof_ctx* c, const double* in, double* out, int n_frames, int radius, double* tmp, const double* w) {
    size_t fs = frame_stride(c);
    const int chunk = std::min(n_frames, BLUR_CHUNK);
    bool tiled = radius >= BL_RMIN && radius <= BL_RMAX;
    if (const char* e = getenv("VOF_BLUR_TILED")) tiled = tiled && e[0] != '0';
    if (tiled && !c->bl_lds_set) {
        HIPCHK(hipFuncSetAttribute((const void*)k_blur1d_tiled<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)blur_tiled_lds(0, BL_RMAX)));
        c->bl_lds_set = true;
    }
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        int nf = std::min(chunk, n_frames - f0);
        Prof p(c, VOF_K_RHS, 0);
        if (tiled) {
            const dim3 g0((c->Nj + BX - 1) / BX, (c->Ni + BL_TI - 1) / BL_TI, nf), g1(g0.x, (c->Ni + BL_TR - 1) / BL_TR, nf);
            k_blur1d_tiled<0><<<g0, blk2d, blur_tiled_lds(0, radius), c->stream>>>(in + (size_t)f0 * fs, tmp, c->Ni, c->Nj, w, radius);
            k_blur1d_tiled<1><<<g1, blk2d, blur_tiled_lds(1, radius), c->stream>>>(tmp, out + (size_t)f0 * fs, c->Ni, c->Nj, w, radius);
        } else {
            dim3 g = grid2d(c->Ni, c->Nj, nf);
            k_blur1d<0><<<g, blk2d, 0, c->stream>>>(in + (size_t)f0 * fs, tmp, c->Ni, c->Nj, w, radius);
            k_blur1d<1><<<g, blk2d, 0, c->stream>>>(tmp, out + (size_t)f0 * fs, c->Ni, c->Nj, w, radius);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// The body of both blur entry points.  _dev: the frames where they lie.  _host: a chunk at a time up into a region of the arena,
// blurred in place, down - as pageable asynchronous copies, as they always were: through the bounce buffer the call measured half
// as slow again (profiles/r22_scratch_arena_summary.md).  The taps take the bounce buffer.
static int blur_stack(vof_ctx* c, const double* in, double* out, int n_frames, const double* weights, int radius, bool host) {
    if (!c) return -1;
    if (!in || !out || !weights) { c->err = "NULL pointer"; return -1; }
    if (host && n_frames < 1) return 0;
    if (n_frames < 1 || radius < 0 || radius > 4096) { c->err = "bad n_frames / radius"; return -1; }
    const size_t fs = frame_stride(c);
    Scratch sc(c);
    double *io = nullptr, *tmp, *w;
    if (host) sc.once(&io, (size_t)std::min(n_frames, BLUR_CHUNK) * fs);
    blur_regions(sc, n_frames, &tmp, &w, radius);
    if (int rc = sc.plan(1, 1, 0.8); rc < 0) return rc;
    if (int rc = h2d_bounced(c, w, weights, (size_t)(2 * radius + 1) * sizeof(double))) return rc;
    if (host) {
        for (int f0 = 0; f0 < n_frames; f0 += BLUR_CHUNK) {
            const int nf = std::min(BLUR_CHUNK, n_frames - f0);
            HIPCHK(hipMemcpyAsync(io, in + (size_t)f0 * fs, (size_t)nf * fs * sizeof(double), hipMemcpyHostToDevice, c->stream));
            if (int rc = blur_frames(c, io, io, nf, radius, tmp, w)) return rc;
            HIPCHK(hipMemcpyAsync(out + (size_t)f0 * fs, io, (size_t)nf * fs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    } else if (int rc = blur_frames(c, in, out, n_frames, radius, tmp, w)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int vof_blur_stack_dev(vof_ctx* c, const double* in, double* out, int n_frames, const double* weights, int radius) {
    return blur_stack(c, in, out, n_frames, weights, radius, false);
}
int vof_blur_stack_host(vof_ctx* c, const double* in, double* out, int n_frames, const double* weights, int radius) {
    return blur_stack(c, in, out, n_frames, weights, radius, true);
}

// sum (x - shift), sum (x - shift)^2 over n device doubles -> out2 (host); uses ctx->partials / func3 as scratch
static int moments_pass(vof_ctx* c, const double* x, size_t n, double shift, double* out2) {
    const int nb = c->nblk;
    Prof p(c, VOF_K_REDUCE, 0, 8.0 * n);
    k_moments<<<nb, RBLK, 0, c->stream>>>(x, n, shift, c->partials);
    k_sum3<<<1, 64, 0, c->stream>>>(c->partials, nb, c->func3);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_func3, c->func3, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out2[0] = c->h_func3[0];
    out2[1] = c->h_func3[1];
    return 0;
}

static int chunk_moments(vof_ctx* c, const double* x, size_t n, Moments* acc) {
    double s[2];
    if (int rc = moments_pass(c, x, n, 0.0, s)) return rc;
    double mean = s[0] / (double)n;
    if (int rc = moments_pass(c, x, n, mean, s)) return rc;
    mean += s[0] / (double)n;                                      // first-order correction of the rounded mean
    acc->merge((double)n, mean, s[1] - s[0] * s[0] / (double)n);
    return 0;
}

int vof_field_moments_dev(vof_ctx* c, const double* field, size_t n, double* mean, double* variance) {
    if (!c) return -1;
    if (!field || n == 0) { c->err = "empty field"; return -1; }
    HIPCHK(hipSetDevice(c->device));
    Moments m;
    if (int rc = chunk_moments(c, field, n, &m)) return rc;
    if (mean) *mean = m.mean;
    if (variance) *variance = m.m2 / m.n;
    return 0;
}

int vof_subsample_dev(vof_ctx* c, const double* field, int n_fields, int box, int offset, double* out) {
    if (!c) return -1;
    if (!field || !out) { c->err = "NULL pointer"; return -1; }
    if (n_fields < 1 || box < 1 || offset < 0 || offset >= box) { c->err = "bad n_fields / box / offset"; return -1; }
    HIPCHK(hipSetDevice(c->device));
    int nbx = c->Ni / box, nby = c->Nj / box;
    if (nbx < 1 || nby < 1) return 0;
    k_subsample<<<grid2d(nbx, nby, n_fields), blk2d, 0, c->stream>>>(field, c->Ni, c->Nj, box, offset, nbx, nby, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// One batch of "virtual pairs" (own alpha / beta / frame / output slot each) of a device-resident movie, with the
// preconditioner policy of solve_range_dev: direct only, or multigrid with the direct re-solve of what it leaves unconverged.
static int solve_virtual_pairs(vof_ctx* c, const double* dmovie, const std::vector<PairParam>& hp, int np, double* const* outs,
                               vof_pair_stats* st) {
    if (direct_only(c)) {
        std::vector<PairParam> items(hp.begin(), hp.begin() + np);
        return direct_solve_list(c, dmovie, items, outs[0], outs[1], outs[2], outs[3], st);
    }
    if (int rc = solve_batch(c, BatchReq{dmovie, np, hp.data(), nullptr, false, outs[0], outs[1], outs[2], outs[3], st})) return rc;
    return resolve_unconverged(c, dmovie, hp.data(), np, outs, st);
}

int vof_vary_regularisation_host(vof_ctx* c, const double* movie, int n_frames, const vof_params* base,
                                 const double* speed_alphas, int n_sa, const double* remodelling_alphas, int n_ra,
                                 const double* blur_weights, int blur_radius, vof_variation_stats* out) {
    if (!c) return -1;
    if (!movie || !base || !out || !speed_alphas || !remodelling_alphas) { c->err = "NULL pointer"; return -1; }
    if (n_frames < 2) { c->err = "need at least two frames"; return -1; }
    if (n_sa < 0 || n_ra < 0) { c->err = "negative grid size"; return -1; }
    if (int rc = check_params(c, base)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t fs = frame_stride(c);
    const int P = n_frames - 1;
    if (int rc = ensure_staging(c, false)) return rc;   // per-batch output staging shared with the host API
    // the whole movie stays resident for the sweep (freed on return)
    double* dmovie = nullptr;
    HIPCHK(hipMalloc((void**)&dmovie, (size_t)n_frames * fs * sizeof(double)));
    auto fail = [&](int rc) { (void)hipFree(dmovie); return rc; };
    {   // pinned in place for the upload (pageable copies run at ~2 GB/s here, see vof_solve_stack_host)
        const size_t movie_bytes = (size_t)n_frames * fs * sizeof(double);
        HostPin pin(movie, movie_bytes);
        hipError_t e = hipMemcpyAsync(dmovie, movie, movie_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        pin.release();
        if (e != hipSuccess) { c->err = std::string("H2D copy failed: ") + hipGetErrorString(e); return fail(-2); }
    }
    if (blur_weights)
        if (int rc = vof_blur_stack_dev(c, dmovie, dmovie, n_frames, blur_weights, blur_radius)) return fail(rc);
    auto summarise = [&](vof_variation_stats& o, const vof_pair_stats* st, const Moments& ms, const Moments& mr) {
        memset(&o, 0, sizeof o);
        o.speed_mean = ms.mean; o.speed_variance = ms.m2 / ms.n;
        o.remodelling_mean = mr.mean; o.remodelling_variance = mr.m2 / mr.n;
        o.converged_all = 1;
        for (int k = 0; k < P; ++k) {
            o.L1_functional += st[k].L1_functional;
            o.speed_functional += st[k].speed_functional;
            o.remodelling_functional += st[k].remodelling_functional;
            o.max_relative_residual = std::max(o.max_relative_residual, st[k].relative_residual);
            o.max_iterations_used = std::max(o.max_iterations_used, st[k].iterations);
            o.converged_all &= st[k].converged;
        }
        o.converged_last = st[P - 1].converged;
    };
    const int n_comb = n_sa * n_ra;
    for (int t = 0; t < n_comb; ++t) {   // validate every combination before any work
        vof_params q = *base;
        q.speed_alpha = speed_alphas[t / n_ra];
        q.remodelling_alpha = remodelling_alphas[t % n_ra];
        if (int rc = check_params(c, &q)) return fail(rc);
    }
    if (int rc = check_params(c, base)) return fail(rc);
    if (P <= c->B) {
        // Short movies leave the chip idle (16 pairs of 512^2 fill a third of it): solve G combinations at once as
        // G * P "virtual pairs" of one batch - pair v = (combination v / P, frame pair v % P) reads its own
        // (alpha, beta) and frame index from the PairParam table.
        const int G = std::max(1, c->B / P);
        std::vector<PairParam> hp((size_t)G * P);
        std::vector<vof_pair_stats> st((size_t)G * P);
        for (int t0 = 0; t0 < n_comb; t0 += G) {
            const int g = std::min(G, n_comb - t0), np = g * P;
            for (int u = 0; u < g; ++u)
                for (int k = 0; k < P; ++k)
                    hp[(size_t)u * P + k] = PairParam{speed_alphas[(t0 + u) / n_ra], remodelling_alphas[(t0 + u) % n_ra], k, u * P + k};
            if (int rc = solve_virtual_pairs(c, dmovie, hp, np, c->st_out, st.data())) return fail(rc);
            for (int u = 0; u < g; ++u) {
                Moments ms, mr;
                if (int rc2 = chunk_moments(c, c->st_out[3] + (size_t)u * P * fs, (size_t)P * fs, &ms)) return fail(rc2);
                if (int rc2 = chunk_moments(c, c->st_out[2] + (size_t)u * P * fs, (size_t)P * fs, &mr)) return fail(rc2);
                summarise(out[t0 + u], st.data() + (size_t)u * P, ms, mr);
            }
        }
    } else {
        std::vector<vof_pair_stats> st((size_t)P);
        for (int t = 0; t < n_comb; ++t) {
            vof_params q = *base;
            q.speed_alpha = speed_alphas[t / n_ra];
            q.remodelling_alpha = remodelling_alphas[t % n_ra];
            if (int rc = check_params(c, &q)) return fail(rc);
            Moments ms, mr;
            std::vector<PairParam> hp2((size_t)c->B);
            for (int k0 = 0; k0 < P; k0 += c->B) {
                int np = std::min(c->B, P - k0);
                for (int i = 0; i < np; ++i) hp2[i] = PairParam{q.speed_alpha, q.remodelling_alpha, k0 + i, i};
                if (int rc = solve_virtual_pairs(c, dmovie, hp2, np, c->st_out, st.data() + k0)) return fail(rc);
                if (int rc = chunk_moments(c, c->st_out[3], (size_t)np * fs, &ms)) return fail(rc);
                if (int rc = chunk_moments(c, c->st_out[2], (size_t)np * fs, &mr)) return fail(rc);
            }
            summarise(out[t], st.data(), ms, mr);
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "stream synchronize failed"; return fail(-2); }
    return fail(0);
}

int vof_texture_stack_dev(vof_ctx* c, double* out, int n_frames, const double* mode_params, int n_modes,
                          const double* frame_offsets, double period, double scale) {
    if (!c) return -1;
    if (!out || !mode_params || !frame_offsets) { c->err = "NULL pointer"; return -1; }
    if (n_frames < 1 || n_modes < 1 || n_modes > 4096 || !(period > 0.0)) { c->err = "bad n_frames / n_modes / period"; return -1; }
    HIPCHK(hipSetDevice(c->device));
    const int width = std::max(c->Ni, c->Nj);
    const int chunk = std::max(1, std::min(n_frames, (int)(((size_t)64 << 20) / ((size_t)4 * n_modes * width * sizeof(double)))));
    const size_t need = (size_t)chunk * 4 * n_modes * width + (size_t)4 * n_modes + (size_t)2 * chunk;
    if (c->tex_cap < need) {
        if (int rc = dev_alloc(c, &c->tex_tab, need)) return rc;
        c->tex_cap = need;
    }
    double* prm = c->tex_tab + (size_t)chunk * 4 * n_modes * width;
    double* offs = prm + (size_t)4 * n_modes;
    HIPCHK(hipMemcpyAsync(prm, mode_params, (size_t)4 * n_modes * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int t0 = 0; t0 < n_frames; t0 += chunk) {
        const int nf = std::min(chunk, n_frames - t0);
        HIPCHK(hipMemcpyAsync(offs, frame_offsets + (size_t)2 * t0, (size_t)2 * nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
        k_texture_tables<<<dim3((width + 255) / 256, n_modes, nf), 256, 0, c->stream>>>(c->tex_tab, width, c->Ni, c->Nj, n_modes, prm,
                                                                                       offs, period);
        k_texture_sum<<<dim3((c->Nj + BX - 1) / BX, (c->Ni + BY * TEX_ROWS - 1) / (BY * TEX_ROWS), nf), blk2d, 0, c->stream>>>(
            c->tex_tab, width, c->Ni, c->Nj, n_modes, scale, out + (size_t)t0 * frame_stride(c));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));   // offs / the tables are re-used by the next chunk; host offsets may be freed
    }
    return 0;
}

int vof_bench_sweeps_dev(vof_ctx* c, const double* movie, int n_pairs, const vof_params* p, int n_sweeps) {
    if (!c) return -1;
    if (!movie) { c->err = "NULL movie"; return -1; }
    if (n_pairs < 1 || n_pairs > c->B) { c->err = "n_pairs must be in [1, max_pairs_in_flight]"; return -1; }
    if (c->L.size() < 2) { c->err = "grid too small for the sweep benchmark"; return -1; }
    if (int rc = check_params(c, p)) return rc;
    HIPCHK(hipSetDevice(c->device));
    c->frames = movie;
    c->npairs = n_pairs;
    c->cur_units = n_pairs;
    Level& f = c->L[0];
    {
        Prof pr(c, VOF_K_RHS, 0);
        k_rhs<<<grid2d(f.ni, f.nj, n_pairs), blk2d, 0, c->stream>>>(movie, frame_stride(c), c->Nj, f.ni, f.nj, c->kb, nullptr);
    }
    HIPCHK(hipMemsetAsync(c->kx, 0, (size_t)n_pairs * 3 * f.npts * sizeof(double), c->stream));
    CycleIO io;
    if (c->vfloat) {
        size_t n = (size_t)n_pairs * 3 * f.npts;
        k_convert<double, float><<<1024, 256, 0, c->stream>>>(c->kb, (float*)c->b32, n);
        SmoothArgs<float> a;
        a.from_zero = true;
        smooth_level_t<float>(c, 0, (float*)c->ky, (float*)f.x2, (const float*)c->b32, n_sweeps, n_pairs, ALL_PAIRS, a, io);
    } else {
        SmoothArgs<double> a;
        a.from_zero = true;
        smooth_level_t<double>(c, 0, c->kx, (double*)f.x2, c->kb, n_sweeps, n_pairs, ALL_PAIRS, a, io);
    }
    if (io.failed) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int vof_profile_enable(vof_ctx* c, int on) {
    if (!c) return -1;
    if (!on) prof_collect(c);
    c->prof = on != 0;
    return 0;
}

int vof_profile_filter(vof_ctx* c, int kid, int level) {
    if (!c) return -1;
    if (kid >= VOF_K_COUNT || level > 15) { c->err = "bad kernel id / level"; return -1; }
    c->prof_kid = kid;
    c->prof_level = level;
    return 0;
}

int vof_profile_get_units(vof_ctx* c, int kid, int level, int64_t* pair_launches) {
    if (!c) return -1;
    if (kid < 0 || kid >= VOF_K_COUNT || level > 15) { c->err = "bad kernel id / level"; return -1; }
    prof_collect(c);
    long long u = 0;
    for (int l = 0; l < 16; ++l)
        if (level < 0 || l == level) u += c->prof_units[kid][l];
    if (pair_launches) *pair_launches = u;
    return 0;
}

int vof_profile_get_bytes(vof_ctx* c, int kid, int level, double* algorithmic_bytes) {
    if (!c) return -1;
    if (kid < 0 || kid >= VOF_K_COUNT || level > 15) { c->err = "bad kernel id / level"; return -1; }
    prof_collect(c);
    double u = 0;
    for (int l = 0; l < 16; ++l)
        if (level < 0 || l == level) u += c->prof_bytes[kid][l];
    if (algorithmic_bytes) *algorithmic_bytes = u;
    return 0;
}

int vof_profile_get_moved(vof_ctx* c, int kid, int level, double* moved_bytes) {
    if (!c) return -1;
    if (kid < 0 || kid >= VOF_K_COUNT || level > 15) { c->err = "bad kernel id / level"; return -1; }
    prof_collect(c);
    double u = 0;
    for (int l = 0; l < 16; ++l)
        if (level < 0 || l == level) u += c->prof_moved[kid][l];
    if (moved_bytes) *moved_bytes = u;
    return 0;
}

int vof_profile_reset(vof_ctx* c) {
    if (!c) return -1;
    prof_collect(c);
    memset(c->prof_ms, 0, sizeof c->prof_ms);
    memset(c->prof_n, 0, sizeof c->prof_n);
    memset(c->prof_units, 0, sizeof c->prof_units);
    memset(c->prof_bytes, 0, sizeof c->prof_bytes);
    memset(c->prof_moved, 0, sizeof c->prof_moved);
    c->prof_dropped = 0;
    return 0;
}

int vof_profile_get(vof_ctx* c, int kid, int level, int64_t* launches, double* total_ms) {
    if (!c) return -1;
    if (kid < 0 || kid >= VOF_K_COUNT || level > 15) { c->err = "bad kernel id / level"; return -1; }
    prof_collect(c);
    long long n = 0; double ms = 0;
    for (int l = 0; l < 16; ++l)
        if (level < 0 || l == level) { n += c->prof_n[kid][l]; ms += c->prof_ms[kid][l]; }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    return 0;
}

// ---------------------------------------------------------------------------------- debug entry points
static int dbg_ready(vof_ctx* c) {
    if (!c) return -1;
    if (!c->frames || c->npairs < 1) { c->err = "call vof_debug_setup first"; return -1; }
    return 0;
}

int vof_debug_setup(vof_ctx* c, const double* movie_host, int n_pairs, const vof_params* p) {
    if (!c) return -1;
    if (!movie_host) { c->err = "NULL movie"; return -1; }
    if (n_pairs < 1 || n_pairs > c->B) { c->err = "n_pairs must be in [1, max_pairs_in_flight]"; return -1; }
    if (int rc = check_params(c, p)) return rc;
    HIPCHK(hipSetDevice(c->device));
    size_t fs = frame_stride(c);
    if (int rc = ensure_staging(c, false)) return rc;
    if (int rc = h2d_bounced(c, c->st_movie, movie_host, (size_t)(n_pairs + 1) * fs * sizeof(double))) return rc;
    if (int rc = setup_batch(c, c->st_movie, n_pairs)) return rc;
    c->vcoarse32 = p->vcycle_precision == 3;   // vof_debug_vcycle* run the cycle as a solve would (the per-level entry points: float64)
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int vof_debug_check_canaries(vof_ctx* c) {
    if (!c) return -1;
    if (!c->dbg_canary) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    std::string rep;
    const int bad = dbg_check_canaries(c, &rep);
    if (bad != 0) { c->err = "VOF_DEBUG_CANARY: " + rep; return -5; }
    return 0;
}

int vof_debug_level_shape(vof_ctx* c, int level, int* n_i, int* n_j) {
    if (!c) return -1;
    if (level < 0 || level >= (int)c->L.size()) { c->err = "bad level"; return -1; }
    if (n_i) *n_i = c->L[level].ni;
    if (n_j) *n_j = c->L[level].nj;
    return 0;
}

#define DBG_LEVEL(level)                                                              \
    if (int rc_ = dbg_ready(c)) return rc_;                                           \
    if (level < 0 || level >= (int)c->L.size()) { c->err = "bad level"; return -1; } \
    Level& lv = c->L[level];                                                          \
    size_t nbytes = (size_t)c->npairs * 3 * lv.npts * sizeof(double);                 \
    (void)nbytes;

// The debug API moves host float64 arrays in and out of V-typed device buffers (kp, kv, kt; staging: krh).
static int dbg_up(vof_ctx* c, void* dst_v, const double* host, size_t n) {
    if (int rc = h2d_bounced(c, c->vfloat ? (void*)c->krh : dst_v, host, n * sizeof(double))) return rc;
    if (c->vfloat) k_convert<double, float><<<256, 256, 0, c->stream>>>(c->krh, (float*)dst_v, n);
    return 0;
}
static int dbg_down(vof_ctx* c, double* host, const void* src_v, size_t n) {
    const bool f32 = c->vfloat || c->h32;   // (h32: the result of vof_debug_vcycle*)
    if (f32) k_convert<float, double><<<256, 256, 0, c->stream>>>((const float*)src_v, c->krh, n);
    return d2h_bounced(c, host, f32 ? (const void*)c->krh : src_v, n * sizeof(double));
}

int vof_debug_rhs(vof_ctx* c, double* b_host) {
    DBG_LEVEL(0)
    k_rhs<<<grid2d(lv.ni, lv.nj, c->npairs), blk2d, 0, c->stream>>>(c->frames, frame_stride(c), c->Nj, lv.ni, lv.nj, c->kb, nullptr);
    return d2h_bounced(c, b_host, c->kb, nbytes);
}

int vof_debug_apply(vof_ctx* c, int level, const double* x_host, double* y_host) {
    DBG_LEVEL(level)
    size_t n = nbytes / sizeof(double);
    if (int rc = dbg_up(c, c->kp, x_host, n)) return rc;
    if (level == 0) {   // the Krylov product: V-typed x, FP64 result
        krylov_apply(c, c->kp, c->kv, c->npairs, ALL_PAIRS);
        return d2h_bounced(c, y_host, c->kv, nbytes);
    }
    VDISPATCH(c, apply_level_t<VT>(c, level, (const VT*)c->kp, (const VT*)nullptr, (VT*)c->kv, 0, c->npairs, ALL_PAIRS));
    return dbg_down(c, y_host, c->kv, n);
}

int vof_debug_gs(vof_ctx* c, int level, double* x_host, const double* b_host, int colour) {
    DBG_LEVEL(level)
    if (colour < 0 || colour > 3) { c->err = "bad colour"; return -1; }
    if (c->vfloat) { c->err = "the per-colour reference smoother works on float64 vectors only"; return -1; }
    if (int rc = h2d_bounced(c, c->kp, x_host, nbytes)) return rc;
    if (int rc = h2d_bounced(c, c->kv, b_host, nbytes)) return rc;
    gs_colour(c, level, c->kp, c->kv, colour, c->npairs, ALL_PAIRS);
    return d2h_bounced(c, x_host, c->kp, nbytes);
}

int vof_debug_sweep(vof_ctx* c, int level, double* x_host, const double* b_host, int reverse, int from_zero) {
    DBG_LEVEL(level)
    if (level + 1 >= (int)c->L.size()) { c->err = "coarsest level has no smoother"; return -1; }
    size_t n = nbytes / sizeof(double);
    if (int rc = dbg_up(c, c->kp, x_host, n)) return rc;
    if (int rc = dbg_up(c, c->kv, b_host, n)) return rc;
    CycleIO io;
    VDISPATCH(c, {
        SmoothArgs<VT> a;
        a.reverse = reverse != 0;
        sweep_level_t<VT>(c, level, from_zero ? (const VT*)nullptr : (const VT*)c->kp, (VT*)c->kt, (const VT*)c->kv, c->npairs, ALL_PAIRS, a, io);
    });
    return io.failed ? -1 : dbg_down(c, x_host, c->kt, n);
}

int vof_debug_smooth(vof_ctx* c, int level, double* x_host, const double* b_host, int nu, int reverse, int from_zero) {
    DBG_LEVEL(level)
    if (level + 1 >= (int)c->L.size()) { c->err = "coarsest level has no smoother"; return -1; }
    if (nu < 1) { c->err = "nu must be >= 1"; return -1; }
    size_t n = nbytes / sizeof(double);
    if (int rc = dbg_up(c, c->kp, x_host, n)) return rc;
    if (int rc = dbg_up(c, c->kv, b_host, n)) return rc;
    CycleIO io;
    VDISPATCH(c, {
        SmoothArgs<VT> a;
        a.from_zero = from_zero != 0;
        a.reverse = reverse != 0;
        smooth_level_t<VT>(c, level, (VT*)c->kp, (VT*)c->kt, (const VT*)c->kv, nu, c->npairs, ALL_PAIRS, a, io);
    });
    return io.failed ? -1 : dbg_down(c, x_host, c->kp, n);
}

int vof_set_fused_sweeps(vof_ctx* c, int on) {
    if (!c) return -1;
    c->fused = on != 0;
    if (!c->fused) c->vfloat = false;
    return 0;
}

int vof_debug_restrict(vof_ctx* c, int level, const double* fine_host, double* coarse_host) {
    DBG_LEVEL(level)
    if (level + 1 >= (int)c->L.size()) { c->err = "no coarser level"; return -1; }
    Level& k = c->L[level + 1];
    if (int rc = dbg_up(c, c->kp, fine_host, nbytes / sizeof(double))) return rc;
    VDISPATCH(c, restrict_level_t<VT>(c, level, (const VT*)c->kp, (VT*)c->kv, c->npairs, ALL_PAIRS));
    return dbg_down(c, coarse_host, c->kv, (size_t)c->npairs * 3 * k.npts);
}

int vof_debug_resrestrict_u(vof_ctx* c, int level, const double* x_new_host, const double* x_old_host, double* coarse_host) {
    DBG_LEVEL(level)
    if (level < 1 || level + 1 >= (int)c->L.size() || !lv.C) { c->err = "a stored level with a coarser level is needed"; return -1; }
    Level& k = c->L[level + 1];
    if (int rc = dbg_up(c, c->kp, x_new_host, nbytes / sizeof(double))) return rc;
    if (x_old_host)
        if (int rc = dbg_up(c, c->kt, x_old_host, nbytes / sizeof(double))) return rc;
    VDISPATCH(c, resrestrict_u_t<VT>(c, level, (const VT*)c->kp, x_old_host ? (const VT*)c->kt : (const VT*)nullptr, (VT*)c->kv, c->npairs, ALL_PAIRS));
    return dbg_down(c, coarse_host, c->kv, (size_t)c->npairs * 3 * k.npts);
}

int vof_debug_prolong_add(vof_ctx* c, int level, double* fine_host, const double* coarse_host) {
    DBG_LEVEL(level)
    if (level + 1 >= (int)c->L.size()) { c->err = "no coarser level"; return -1; }
    Level& k = c->L[level + 1];
    if (int rc = dbg_up(c, c->kp, fine_host, nbytes / sizeof(double))) return rc;
    if (int rc = dbg_up(c, c->kv, coarse_host, (size_t)c->npairs * 3 * k.npts)) return rc;
    VDISPATCH(c, prolong_add_level_t<VT>(c, level, (VT*)c->kp, (const VT*)c->kv, c->npairs, ALL_PAIRS));
    return dbg_down(c, fine_host, c->kp, nbytes / sizeof(double));
}

int vof_debug_stencil(vof_ctx* c, int level, double* c_host) {
    DBG_LEVEL(level)
    if (!lv.C) { c->err = "level has no stored stencil"; return -1; }
    const CLay L(lv.ni, lv.nj);
    const int fmt = level > 0 ? c->cfmt : 0;
    const int planes = fmt == 3 ? 30 : (fmt == 2 ? 45 : 81);
    const size_t n = (size_t)c->npairs * planes * L.plane;
    // colour-split device layout -> row-major [pair][81][n_i][n_j]
    auto unpack = [&](auto get) {
        for (int k = 0; k < c->npairs; ++k)
            for (int pl = 0; pl < 81; ++pl)
                for (int p = 0; p < lv.ni; ++p)
                    for (int q = 0; q < lv.nj; ++q)
                        c_host[((size_t)k * 81 + pl) * lv.npts + (size_t)p * lv.nj + q] = get((size_t)k * planes * L.plane, pl, L.idx(p, q));
    };
    if (fmt == 2) {   // 36 planes of packed bfloat16 pairs (off-diagonal blocks) + 9 float32 planes (diagonal block)
        std::vector<uint32_t> tw(n);
        if (int rc = d2h_bounced(c, tw.data(), lv.C, n * sizeof(uint32_t))) return rc;
        unpack([&](size_t base, int pl, size_t idx) -> double {
            const int d = pl / 9, e = pl % 9;
            uint32_t bits;
            if (d == 4) bits = tw[base + (size_t)(36 + e) * L.plane + idx];
            else {
                const int j = (d < 4 ? d : d - 1) * 9 + e;
                const uint32_t v = tw[base + (size_t)(j >> 1) * L.plane + idx];
                bits = (j & 1) ? (v & 0xFFFF0000u) : (v << 16);
            }
            float f;
            memcpy(&f, &bits, 4);
            return f;
        });
    } else if (fmt == 3) {   // 18 planes of four 8-bit floats (1-4-3, bias 7, no infinities) + 9 float32 planes + 3 planes of units
        std::vector<uint32_t> tw(n);
        if (int rc = d2h_bounced(c, tw.data(), lv.C, n * sizeof(uint32_t))) return rc;
        unpack([&](size_t base, int pl, size_t idx) -> double {
            const int d = pl / 9, e = pl % 9;
            if (d == 4) {
                float f;
                memcpy(&f, &tw[base + (size_t)(18 + e) * L.plane + idx], 4);
                return f;
            }
            const int j = (d < 4 ? d : d - 1) * 9 + e;
            const uint32_t v = (tw[base + (size_t)(j >> 2) * L.plane + idx] >> (8 * (j & 3))) & 0xFFu;
            const int ex = (int)((v >> 3) & 0xFu), m = (int)(v & 7u);
            const double mag = ex ? std::ldexp(1.0 + m / 8.0, ex - 7) : std::ldexp(m / 8.0, -6);
            const int eb = (int)((tw[base + (size_t)(27 + e / 3) * L.plane + idx] >> (8 * (e % 3))) & 0xFFu);
            return ((v & 0x80u) ? -mag : mag) * std::ldexp(1.0, eb - 127);
        });
    } else if (fmt == 1) {
        std::vector<float> tf(n);
        if (int rc = d2h_bounced(c, tf.data(), lv.C, n * sizeof(float))) return rc;
        unpack([&](size_t base, int pl, size_t idx) -> double { return tf[base + (size_t)pl * L.plane + idx]; });
    } else {
        std::vector<double> tmp(n);
        if (int rc = d2h_bounced(c, tmp.data(), lv.C, n * sizeof(double))) return rc;
        unpack([&](size_t base, int pl, size_t idx) -> double { return tmp[base + (size_t)pl * L.plane + idx]; });
    }
    return 0;
}

int vof_debug_vcycle(vof_ctx* c, const double* r_host, double* e_host) {
    DBG_LEVEL(0)
    size_t n = nbytes / sizeof(double);
    if (int rc = dbg_up(c, c->kp, r_host, n)) return rc;
    c->h32 = handoff32_ok(c);   // the cycle as the BiCGStab loop's first iterations run it
    CycleIO io;
    vcycle(c, &c->ky, c->kp, c->npairs, ALL_PAIRS, io);
    const int rc = io.failed ? -1 : dbg_down(c, e_host, c->ky, n);
    c->h32 = false;
    return rc;
}

// One multigrid cycle y = M r followed by the Krylov product v = A y with the dot products (v, r) and (v, v) per pair, as the
// BiCGStab loop runs them (fused into the cycle's last smoothing pass when that path applies; `fused` reports it).
int vof_debug_vcycle_apply(vof_ctx* c, const double* r_host, double* y_host, double* v_host, double* dots_host, int* fused) {
    DBG_LEVEL(0)
    size_t n = nbytes / sizeof(double);
    if (int rc = dbg_up(c, c->kp, r_host, n)) return rc;
    const int np = c->npairs;
    c->cur_units = np;
    if (int rc = h2d_bounced(c, c->krh, r_host, nbytes)) return rc;   // dot partner (float64)
    CycleIO io;
    io.trail = S0Trail{c->kv, c->krh, 1, c->partials};
    c->h32 = handoff32_ok(c);
    vcycle(c, &c->ky, c->kp, np, ALL_PAIRS, io);
    if (io.failed) { c->h32 = false; return -1; }
    int nb = io.trail_nblk ? io.trail_nblk : krylov_apply(c, c->ky, c->kv, np, ALL_PAIRS, c->krh, 1);
    if (fused) *fused = io.trail_nblk ? 1 : 0;
    if (!nb) { c->h32 = false; c->err = "the operator kernel did not fuse the dot products"; return -1; }
    const int rcd = dbg_down(c, y_host, c->ky, n);
    c->h32 = false;
    if (rcd) return rcd;
    if (int rc = d2h_bounced(c, v_host, c->kv, nbytes)) return rc;
    std::vector<double> part((size_t)np * 3 * nb);
    if (int rc = d2h_bounced(c, part.data(), c->partials, part.size() * sizeof(double))) return rc;
    for (int k = 0; k < np; ++k)
        for (int sl = 0; sl < 2; ++sl) {
            double a = 0;
            for (int i = 0; i < nb; ++i) a += part[((size_t)k * 3 + sl) * nb + i];
            dots_host[2 * k + sl] = a;
        }
    return 0;
}

int vof_debug_coarse_solve(vof_ctx* c, const double* r_host, double* e_host) {
    int last = c ? (int)c->L.size() - 1 : 0;
    DBG_LEVEL(last)
    size_t n = nbytes / sizeof(double);
    if (int rc = dbg_up(c, c->kp, r_host, n)) return rc;
    VDISPATCH(c, coarse_solve_t<VT>(c, (const VT*)c->kp, (VT*)c->kv, c->npairs, ALL_PAIRS));
    return dbg_down(c, e_host, c->kv, n);
}

// ---- box least-squares flow (conduct_optical_flow, OF.py:24-218) ------------------------------------------------
constexpr int BF_GENERAL_CHUNK = 4;       // pairs per launch of the general path (its scratch: 11 planes per pair)
constexpr int BF_FUSED_CHUNK = 16384;     // pairs per launch of the fused kernel (grid z)

static int box_flow_check(vof_ctx* c, const double* movie, int n_frames, int box_size, double delta_t, int include_remodelling,
                          const double* v_x, const double* v_y, const double* speed, const double* net_remodelling) {
    if (!movie || !v_x || !v_y || !speed) { c->err = "NULL array pointer"; return -1; }
    if (include_remodelling && !net_remodelling) { c->err = "net_remodelling is NULL with include_remodelling"; return -1; }
    if (n_frames < 2) { c->err = "need at least two frames"; return -1; }
    if (box_size < 1) { c->err = "box_size must be >= 1"; return -1; }
    if (delta_t == 0.0) { c->err = "delta_t must not be 0"; return -1; }
    return 0;
}

static bool box_flow_fused(int box_size) {                 // the fused kernel, or the general path: three kernels through scratch planes
    const char* e = getenv("VOF_BOXFLOW_FUSED");
    return box_size / 2 <= BF_HMAX && !(e && e[0] == '0');
}
// the planes of the general path, declared into the caller's arena where box_flow_pairs will take that path (none otherwise)
static void box_flow_regions(Scratch& sc, int box_size, double** planes) {
    sc.once(planes, box_flow_fused(box_size) ? 0 : (size_t)BF_GENERAL_CHUNK * 11 * frame_stride(sc.c));
}

// P pairs of a device-resident movie into device-resident outputs, enqueued on the context's stream; planes: box_flow_regions.
static int box_flow_pairs(vof_ctx* c, double* planes, const double* movie, int P, int box_size, double delta_x, double delta_t,
                          int include_remodelling, int reference_quirks, double* v_x, double* v_y, double* speed, double* net_remodelling) {
    const size_t fs = frame_stride(c);
    BoxArgs a{};
    a.fs = fs; a.Ni = c->Ni; a.Nj = c->Nj; a.h = box_size / 2;
    a.cend = reference_quirks ? std::min(c->Ni, c->Nj) : c->Nj;      // OF.py:108 clamps the column window with N_i
    a.quirks = reference_quirks ? 1 : 0;
    a.n_box = (double)box_size * (double)box_size;
    a.scale = delta_x / delta_t;
    auto at = [&](int k0) {
        a.movie = movie + (size_t)k0 * fs;
        a.vx = v_x + (size_t)k0 * fs; a.vy = v_y + (size_t)k0 * fs; a.speed = speed + (size_t)k0 * fs;
        a.gamma = net_remodelling ? net_remodelling + (size_t)k0 * fs : nullptr;
    };
    if (box_flow_fused(box_size)) {
        if (!c->bf_lds_set) {
            const int lds = (int)bf_fused_lds(BF_HMAX);
            HIPCHK(hipFuncSetAttribute((const void*)k_boxflow_fused<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            HIPCHK(hipFuncSetAttribute((const void*)k_boxflow_fused<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            c->bf_lds_set = true;
        }
        const size_t lds = bf_fused_lds(a.h);
        for (int k0 = 0; k0 < P; k0 += BF_FUSED_CHUNK) {
            const int np = std::min(BF_FUSED_CHUNK, P - k0);
            at(k0);
            const dim3 g((c->Nj + BF_TJ - 1) / BF_TJ, (c->Ni + BF_TI - 1) / BF_TI, np);
            c->cur_units = np;
            Prof prof(c, VOF_K_RHS, 0);
            if (include_remodelling) k_boxflow_fused<true><<<g, BF_THREADS, lds, c->stream>>>(a);
            else k_boxflow_fused<false><<<g, BF_THREADS, lds, c->stream>>>(a);
        }
    } else {
        double* der = planes;
        double* rows = planes + (size_t)BF_GENERAL_CHUNK * 3 * fs;
        for (int k0 = 0; k0 < P; k0 += BF_GENERAL_CHUNK) {
            const int np = std::min(BF_GENERAL_CHUNK, P - k0);
            at(k0);
            const dim3 g = grid2d(c->Ni, c->Nj, np);
            c->cur_units = np;
            Prof prof(c, VOF_K_RHS, 0);
            k_bf_derived<<<g, blk2d, 0, c->stream>>>(a, der);
            if (include_remodelling) {
                k_bf_hsum<true><<<g, blk2d, 0, c->stream>>>(a, der, rows);
                k_bf_vsum<true><<<g, blk2d, 0, c->stream>>>(a, rows);
            } else {
                k_bf_hsum<false><<<g, blk2d, 0, c->stream>>>(a, der, rows);
                k_bf_vsum<false><<<g, blk2d, 0, c->stream>>>(a, rows);
            }
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int vof_box_flow_dev(vof_ctx* c, const double* movie, int n_frames, int box_size, double delta_x, double delta_t, int include_remodelling,
                     int reference_quirks, double* v_x, double* v_y, double* speed, double* net_remodelling) {
    if (!c) return -1;
    if (int rc = box_flow_check(c, movie, n_frames, box_size, delta_t, include_remodelling, v_x, v_y, speed, net_remodelling)) return rc;
    Scratch sc(c);
    double* planes = nullptr;
    box_flow_regions(sc, box_size, &planes);
    if (int rc = sc.plan(1, 1, 0.8); rc < 0) return rc;
    if (int rc = box_flow_pairs(c, planes, movie, n_frames - 1, box_size, delta_x, delta_t, include_remodelling, reference_quirks, v_x, v_y, speed,
                                net_remodelling)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int vof_box_flow_host(vof_ctx* c, const double* movie, int n_frames, int box_size, double delta_x, double delta_t, int include_remodelling,
                      int reference_quirks, double* v_x, double* v_y, double* speed, double* net_remodelling) {
    if (!c) return -1;
    if (int rc = box_flow_check(c, movie, n_frames, box_size, delta_t, include_remodelling, v_x, v_y, speed, net_remodelling)) return rc;
    Scratch sc(c);
    double* planes = nullptr;
    box_flow_regions(sc, box_size, &planes);
    if (int rc = sc.plan(1, 1, 0.8); rc < 0) return rc;
    if (int rc = ensure_staging(c, false)) return rc;
    const size_t fs = frame_stride(c), fb = fs * sizeof(double);
    const int P = n_frames - 1;
    double* outs[4] = {v_x, v_y, speed, include_remodelling ? net_remodelling : nullptr};
    for (int k0 = 0; k0 < P; k0 += c->B) {
        const int np = std::min(c->B, P - k0);
        if (int rc = h2d_bounced(c, c->st_movie, movie + (size_t)k0 * fs, (size_t)(np + 1) * fb)) return rc;
        if (int rc = box_flow_pairs(c, planes, c->st_movie, np, box_size, delta_x, delta_t, include_remodelling, reference_quirks, c->st_out[0],
                                    c->st_out[1], c->st_out[2], include_remodelling ? c->st_out[3] : nullptr)) return rc;
        for (int f = 0; f < 4; ++f)
            if (outs[f])
                if (int rc = d2h_bounced(c, outs[f] + (size_t)k0 * fs, c->st_out[f], (size_t)np * fb)) return rc;
    }
    if (!include_remodelling && net_remodelling) memset(net_remodelling, 0, (size_t)P * fb);
    return 0;
}

// Frames k0 .. k0 + np of a pair chunk of sweep r on the device, *p: the caller's own (_dev), or `frames` - a per_unit_plus_one
// region - where they are uploaded (_host) and, with device taps, blurred in place (tmp: blur_regions)
static int pair_chunk_frames(vof_ctx* c, const SweepBase& r, int k0, int np, double* frames, const double* taps, int radius, double* tmp,
                             const double** p) {
    const size_t fs = frame_stride(c);
    *p = r.movie + (size_t)k0 * fs;
    if (r.host) {
        if (int rc = h2d_bounced(c, frames, *p, (size_t)(np + 1) * fs * sizeof(double))) return rc;
        *p = frames;
    }
    if (taps) {
        if (int rc = blur_frames(c, *p, frames, np + 1, radius, tmp, taps)) return rc;
        *p = frames;
    }
    return 0;
}

// ---- box-size sweep of the box flow (vary_boxsize; vof_boxsweep.hpp) ---------------------------------------------
struct SweepReq : SweepBase {
    const int32_t* boxes; int n_boxes;
    const double* blur_w; int blur_r;
    vof_boxsize_stats* stats;
};

static int vary_boxsize_impl(vof_ctx* c, const SweepReq& r) {
    if (!c) return -1;
    if (int rc = sweep_check(c, r, r.stats)) return rc;
    if (!r.boxes || r.n_boxes < 1) { c->err = "the list of box sizes is empty"; return -1; }
    for (int b = 0; b < r.n_boxes; ++b)
        if (r.boxes[b] < 1) { c->err = "every box size must be >= 1"; return -1; }
    if (r.blur_w && (r.blur_r < 0 || r.blur_r > 4096)) { c->err = "bad blur_radius"; return -1; }
    const size_t fs = frame_stride(c);
    const int P = r.n_frames - 1, NQ = r.remodel ? 8 : 5;
    // the arena: cap + 1 frames, and per pair 3 derived planes, R / C / W of every quantity and 4 chunk outputs
    Scratch sc(c);
    double *frames, *der, *chunk_out[4], *blur_tmp = nullptr, *blur_w = nullptr;
    SweepArgs s{};
    s.fs = fs; s.Ni = c->Ni; s.Nj = c->Nj;
    sc.per_unit_plus_one(&frames, fs);
    sc.per_unit(&der, 3 * fs);
    for (double** q : {&s.R, &s.C, &s.W}) sc.per_unit(q, (size_t)NQ * fs);
    for (double*& q : chunk_out) sc.per_unit(&q, fs);
    if (r.blur_w) blur_regions(sc, sweep_want(c, r) + 1, &blur_tmp, &blur_w, r.blur_r);
    SweepTail tail;
    sweep_tail_regions(sc, tail, r, "box-size sweep", r.n_boxes);
    const int cap = sweep_tail_begin(sc, tail, " for one pair");
    if (cap < 0) return cap;
    s.der = der;
    if (r.blur_w) if (int rc = h2d_bounced(c, blur_w, r.blur_w, (size_t)(2 * r.blur_r + 1) * sizeof(double))) return rc;

    // the steps: a half width past the longer image side adds only zeros, so the chain ends there
    const int h_stop = std::max(c->Ni, c->Nj);
    std::vector<std::vector<int>> at_h;                 // list entries that map to each half width
    for (int b = 0; b < r.n_boxes; ++b) {
        const int h = std::min(r.boxes[b] / 2, h_stop);
        if ((int)at_h.size() <= h) at_h.resize((size_t)h + 1);
        at_h[h].push_back(b);
    }
    const int h_max = (int)at_h.size() - 1;
    BoxArgs a{};
    a.fs = fs; a.Ni = c->Ni; a.Nj = c->Nj;
    a.cend = r.quirks ? std::min(c->Ni, c->Nj) : c->Nj;      // OF.py:108 clamps the column window with N_i
    a.quirks = r.quirks ? 1 : 0;
    a.scale = r.delta_x / r.delta_t;

    for (int k0 = 0; k0 < P; k0 += cap) {
        const int np = std::min(cap, P - k0);
        const dim3 g = grid2d(c->Ni, c->Nj, np);
        if (int rc = pair_chunk_frames(c, r, k0, np, frames, blur_w, r.blur_r, blur_tmp, &a.movie)) return rc;
        c->cur_units = np;
        { Prof prof(c, VOF_K_RHS, 0);
          k_bf_derived<<<g, blk2d, 0, c->stream>>>(a, der);
          if (r.remodel) k_bs_init<true><<<g, blk2d, 0, c->stream>>>(s);
          else k_bs_init<false><<<g, blk2d, 0, c->stream>>>(s); }
        for (int h = 0; h <= h_max; ++h) {
            s.h = h;
            a.h = h;
            bool stepped = h == 0;
            if (h >= 1) {
                Prof prof(c, VOF_K_RHS, 0);
                if (r.remodel) k_bs_grow<true><<<g, blk2d, 0, c->stream>>>(s);
                else k_bs_grow<false><<<g, blk2d, 0, c->stream>>>(s);
                if (at_h[h].empty()) {
                    if (r.remodel) k_bs_window<true, true, false><<<g, blk2d, 0, c->stream>>>(s, a);
                    else k_bs_window<false, true, false><<<g, blk2d, 0, c->stream>>>(s, a);
                }
            }
            for (int b : at_h[h]) {
                a.n_box = (double)r.boxes[b] * (double)r.boxes[b];
                const SweepDst d = sweep_dst(r, chunk_out, fs, b, k0);
                a.vx = d.keep_v ? d.f[0] : nullptr; a.vy = d.keep_v ? d.f[1] : nullptr; a.speed = d.f[2];
                a.gamma = d.keep_g ? d.f[3] : nullptr;
                {
                    Prof prof(c, VOF_K_RHS, 0);
                    if (!stepped) {              // the first entry of this half width takes the step with it
                        if (r.remodel) k_bs_window<true, true, true><<<g, blk2d, 0, c->stream>>>(s, a);
                        else k_bs_window<false, true, true><<<g, blk2d, 0, c->stream>>>(s, a);
                        stepped = true;
                    } else {
                        if (r.remodel) k_bs_window<true, false, true><<<g, blk2d, 0, c->stream>>>(s, a);
                        else k_bs_window<false, false, true><<<g, blk2d, 0, c->stream>>>(s, a);
                    }
                }
                sweep_tail_speed(c, tail, b, k0, np, a.speed);
                if (int rc = sweep_tail_moments(c, tail, b, k0, np, a.speed, a.gamma)) return rc;
                if (int rc = sweep_copy_out(c, r, d, fs, np)) return rc;
            }
        }
    }
    if (int rc = sweep_tail_finish(c, tail, r.stats)) return rc;
    for (int b = 0; b < r.n_boxes; ++b) r.stats[b].box_size = r.boxes[b];
    return 0;
}

#define VOF_BOXSIZE_ARGS                                                                                                              \
    vof_ctx *c, const double *movie, int n_frames, const int32_t *box_sizes, int n_boxes, double delta_x, double delta_t,             \
        int include_remodelling, int reference_quirks, const double *blur_weights, int blur_radius, const double *histogram_edges,    \
        int histogram_bins, int64_t *histograms, const int32_t *probe_ij, int n_probes, double *probe_speeds,                         \
        vof_boxsize_stats *stats, double *v_x, double *v_y, double *speed, double *net_remodelling
#define VOF_BOXSIZE_REQ(host)                                                                                                         \
    SweepReq{{movie, n_frames, delta_x, delta_t, include_remodelling, reference_quirks, histogram_edges, histogram_bins, histograms,  \
              probe_ij, n_probes, probe_speeds, {v_x, v_y, speed, net_remodelling}, host},                                            \
             box_sizes, n_boxes, blur_weights, blur_radius, stats}

int vof_vary_boxsize_dev(VOF_BOXSIZE_ARGS) { return vary_boxsize_impl(c, VOF_BOXSIZE_REQ(false)); }
int vof_vary_boxsize_host(VOF_BOXSIZE_ARGS) { return vary_boxsize_impl(c, VOF_BOXSIZE_REQ(true)); }

// ---- blur sweep of the box flow (vary_blursize; vof_blursweep.hpp) -------------------------------------------------
struct BlurSweepReq : SweepBase {
    const double* taps; const int32_t* radii; int n_sigmas;     // the tap vectors (2 radii[s] + 1 each), concatenated
    int box_size;
    int abins; int64_t* ahist; double* awhist;                  // flow direction: counts and speed-weighted sums
    const double* iedges; int ibins; int64_t* ihist;            // intensity of the blurred stack
    vof_blursize_stats* stats;
};

// np.linspace(lo, hi, bins + 1) for hi - lo exactly representable: i * step + lo, the last one the stop itself
static std::vector<double> linspace_edges(double lo, double hi, int bins) {
    std::vector<double> e((size_t)bins + 1);
    const volatile double step = (hi - lo) / (double)bins;
    for (int i = 0; i < bins; ++i) { const volatile double t = (double)i * step; e[i] = t + lo; }
    e[bins] = hi;
    return e;
}

// sum P per-pair partial histograms of `bins` bins, part[pair][bin], in pair order
static void sum_pair_histograms(const double* part, int P, int bins, double* out) {
    for (int b = 0; b < bins; ++b) {
        double w = 0.0;
        for (int k = 0; k < P; ++k) w += part[(size_t)k * bins + b];
        out[b] = w;
    }
}

// The flow-direction histogram per list entry of a sweep - the sigmas of the blur sweep, the two channels of the comparison -:
// counts and speed-weighted sums over `bins` bins of [-1, 1] (0: none).  Its integer counters belong to the span behind the
// tail's d_bad (SweepTail), so the sweep calls regions() before sweep_tail_regions and counters() after it.
struct DirectionHist {
    int bins, n, P, blk; size_t fs;       // blk: blocks per pair, by the plane size only
    double *d_edges, *d_wsum, *d_part;    // the sums [entry][pair][bin]; the partials of one chunk
    unsigned long long* d_hist;
    void regions(Scratch& sc, int bins_, int n_, int P_) {
        bins = bins_; n = n_; P = P_; fs = frame_stride(sc.c);
        blk = (int)std::min<size_t>(BZ_ANGLE_MAX_BLOCKS, std::max<size_t>(1, fs / (64 * BZ_ANGLE_PER_LANE)));
        sc.once(&d_edges, bins ? (size_t)bins + 1 : 0);
        sc.once(&d_wsum, (size_t)n * P * bins);
        sc.per_unit(&d_part, (size_t)blk * bins);
    }
    void counters(Scratch& sc) { sc.once(&d_hist, (size_t)n * bins); }
    int upload_edges(vof_ctx* c) const {                           // once the arena is planned
        if (!bins) return 0;
        const std::vector<double> e = linspace_edges(-1.0, 1.0, bins);
        return h2d_bounced(c, d_edges, e.data(), e.size() * 8);
    }
    // pairs k0 .. k0 + np of entry e, enqueued behind the kernels that wrote the fields
    void enqueue(vof_ctx* c, int e, int k0, int np, const double* vx, const double* vy, const double* speed) const {
        if (!bins) return;
        Prof prof(c, VOF_K_REDUCE, 0);
        k_bz_angles<<<dim3(blk, np), 64, (size_t)bins * 64 * sizeof(double), c->stream>>>(vx, vy, speed, fs, d_edges, bins,
                                                                                          d_hist + (size_t)e * bins, d_part);
        const int nt = np * bins;
        k_bz_angle_sum<<<(nt + 255) / 256, 256, 0, c->stream>>>(d_part, blk, bins, np, d_wsum + ((size_t)e * P + k0) * bins);
    }
    // behind sweep_tail_finish: the counts from the tail's host copy, the weighted sums summed over the pairs in pair order
    int finish(vof_ctx* c, const SweepTail& t, int64_t* hist, double* whist) const {
        std::vector<double> wsum((size_t)n * P * bins);
        if (bins) if (int rc = d2h_bounced(c, wsum.data(), d_wsum, wsum.size() * 8)) return rc;
        for (size_t i = 0; i < (size_t)n * bins; ++i) hist[i] = (int64_t)t.host(d_hist)[i];
        for (int e = 0; e < n; ++e) sum_pair_histograms(wsum.data() + (size_t)e * P * bins, P, bins, whist + (size_t)e * bins);
        return 0;
    }
};

static int vary_blursize_impl(vof_ctx* c, const BlurSweepReq& r) {
    if (!c) return -1;
    if (int rc = sweep_check(c, r, r.stats)) return rc;
    if (!r.taps || !r.radii || r.n_sigmas < 1) { c->err = "the list of blur sizes is empty"; return -1; }
    for (int s = 0; s < r.n_sigmas; ++s)
        if (r.radii[s] < 0 || r.radii[s] > 4096) { c->err = "bad blur radius"; return -1; }
    if (r.box_size < 1) { c->err = "box_size must be >= 1"; return -1; }
    if (r.iedges && (r.ibins < 1 || !r.ihist)) { c->err = "intensity_edges needs intensity_bins >= 1 and intensity_histograms"; return -1; }
    if (r.iedges && !(r.iedges[r.ibins] > r.iedges[0])) { c->err = "intensity_edges must increase"; return -1; }
    if (r.abins < 0 || r.abins > BZ_MAX_ANGLE_BINS) { c->err = "angle_bins must be 0 .. " + std::to_string(BZ_MAX_ANGLE_BINS); return -1; }
    if (r.abins && (!r.ahist || !r.awhist)) { c->err = "angle_bins needs angle_histograms and weighted_angle_histograms"; return -1; }
    const size_t fs = frame_stride(c), fb = fs * sizeof(double);
    const int T = r.n_frames, P = T - 1, n = r.n_sigmas;
    std::vector<size_t> tap_at(n);
    size_t n_taps = 0;
    for (int s = 0; s < n; ++s) { tap_at[s] = n_taps; n_taps += 2 * (size_t)r.radii[s] + 1; }
    const size_t n_ihist = r.iedges ? (size_t)n * r.ibins : 0;
    // the arena: the blurred stack, the movie (_host) and four chunk outputs per pair in flight; what the sweep's own kernels
    // read and write: taps, intensity edges, the direction histogram's; the tail's; the sweep's counters
    Scratch sc(c);
    double *blurred, *up = nullptr, *chunk_out[4], *blur_tmp, *bf_planes = nullptr, *d_taps, *d_iedges;
    unsigned long long *d_ihist, *d_ibad;
    DirectionHist dir;
    sc.once(&blurred, (size_t)T * fs);
    if (r.host) sc.once(&up, (size_t)T * fs);
    for (double*& q : chunk_out) sc.per_unit(&q, fs);
    blur_regions(sc, T, &blur_tmp);
    box_flow_regions(sc, r.box_size, &bf_planes);
    sc.once(&d_taps, n_taps);
    sc.once(&d_iedges, r.iedges ? (size_t)r.ibins + 1 : 0);
    dir.regions(sc, r.abins, n, P);
    SweepTail tail;
    sweep_tail_regions(sc, tail, r, "blur sweep", n);
    dir.counters(sc);
    sc.once(&d_ihist, n_ihist);
    sc.once(&d_ibad, 1);
    const int cap = sweep_tail_begin(sc, tail, "");
    if (cap < 0) return cap;
    if (r.host) if (int rc = h2d_bounced(c, up, r.movie, (size_t)T * fb)) return rc;     // the movie goes up once
    const double* movie = r.host ? up : r.movie;
    if (int rc = h2d_bounced(c, d_taps, r.taps, n_taps * 8)) return rc;
    if (r.iedges) if (int rc = h2d_bounced(c, d_iedges, r.iedges, (size_t)(r.ibins + 1) * 8)) return rc;
    if (int rc = dir.upload_edges(c)) return rc;

    for (int s = 0; s < n; ++s) {
        if (int rc = blur_frames(c, movie, blurred, T, r.radii[s], blur_tmp, d_taps + tap_at[s])) return rc;
        if (r.iedges) {
            const size_t m = (size_t)T * fs;
            const int nb = (int)std::min<size_t>(1024, (m + 4 * 256 - 1) / (4 * 256));
            Prof prof(c, VOF_K_REDUCE, 0);
            k_bs_counts<<<nb, 256, 0, c->stream>>>(blurred, m, d_iedges, r.ibins, d_ihist + (size_t)s * r.ibins, d_ibad);
        }
        for (int k0 = 0; k0 < P; k0 += cap) {
            const int np = std::min(cap, P - k0);
            const SweepDst d = sweep_dst(r, chunk_out, fs, s, k0);
            // exactly vof_box_flow_dev: the same kernels, the same choice between the fused and the general path
            if (int rc = box_flow_pairs(c, bf_planes, blurred + (size_t)k0 * fs, np, r.box_size, r.delta_x, r.delta_t, r.remodel, r.quirks, d.f[0], d.f[1],
                                        d.f[2], d.keep_g ? d.f[3] : nullptr)) return rc;
            sweep_tail_speed(c, tail, s, k0, np, d.f[2]);
            dir.enqueue(c, s, k0, np, d.f[0], d.f[1], d.f[2]);
            if (int rc = sweep_tail_moments(c, tail, s, k0, np, d.f[2], d.f[3])) return rc;
            if (int rc = sweep_copy_out(c, r, d, fs, np)) return rc;
        }
    }
    if (int rc = sweep_tail_finish(c, tail, r.stats)) return rc;
    if (int rc = dir.finish(c, tail, r.ahist, r.awhist)) return rc;
    for (size_t t = 0; t < n_ihist; ++t) r.ihist[t] = (int64_t)tail.host(d_ihist)[t];
    for (int s = 0; s < n; ++s) r.stats[s].sigma_index = s;
    return 0;
}

#define VOF_BLURSIZE_ARGS                                                                                                             \
    vof_ctx *c, const double *movie, int n_frames, const double *blur_weights, const int32_t *blur_radii, int n_sigmas, int box_size, \
        double delta_x, double delta_t, int include_remodelling, int reference_quirks, const double *histogram_edges,                 \
        int histogram_bins, int64_t *histograms, int angle_bins, int64_t *angle_histograms, double *weighted_angle_histograms,        \
        const double *intensity_edges, int intensity_bins, int64_t *intensity_histograms, const int32_t *probe_ij, int n_probes,      \
        double *probe_speeds, vof_blursize_stats *stats, double *v_x, double *v_y, double *speed, double *net_remodelling
#define VOF_BLURSIZE_REQ(host)                                                                                                        \
    BlurSweepReq{{movie, n_frames, delta_x, delta_t, include_remodelling, reference_quirks, histogram_edges, histogram_bins,          \
                  histograms, probe_ij, n_probes, probe_speeds, {v_x, v_y, speed, net_remodelling}, host},                            \
                 blur_weights, blur_radii, n_sigmas, box_size, angle_bins, angle_histograms, weighted_angle_histograms,               \
                 intensity_edges, intensity_bins, intensity_histograms, stats}

int vof_vary_blursize_dev(VOF_BLURSIZE_ARGS) { return vary_blursize_impl(c, VOF_BLURSIZE_REQ(false)); }
int vof_vary_blursize_host(VOF_BLURSIZE_ARGS) { return vary_blursize_impl(c, VOF_BLURSIZE_REQ(true)); }

// ---- two channels of one movie: their box flows and the joint statistics (compare_channel_flows; vof_compare.hpp) --------
struct CompareReq : SweepBase {           // movie, outs: channel a; the tail's two entries are the channels
    const double* movie_b;
    const double* taps[2]; int radius[2];
    int box_size;
    int abins; int64_t* ahist; double* awhist;                  // per-channel flow direction
    int tbins; int64_t* thist; double* twhist;                  // angle between the two flows
    const double* jedges[2]; int jbins[2]; const double* jmin; int64_t* jhist;     // the two speeds
    int64_t* jcounts;
    double* outs_b[4];
    vof_compare_stats* stats;
};

static int compare_flows_impl(vof_ctx* c, const CompareReq& r) {
    if (!c) return -1;
    if (int rc = sweep_check(c, r, r.stats)) return rc;
    if (!r.movie_b) { c->err = "movie_b is NULL"; return -1; }
    for (int f = 0; f < 4; ++f)
        if ((r.outs[f] != nullptr) != (r.outs_b[f] != nullptr)) { c->err = "the field stacks of both channels must be given together"; return -1; }
    for (int ch = 0; ch < 2; ++ch)
        if (r.taps[ch] && (r.radius[ch] < 0 || r.radius[ch] > 4096)) { c->err = "bad blur_radius"; return -1; }
    if (r.box_size < 1) { c->err = "box_size must be >= 1"; return -1; }
    if (r.abins < 0 || r.abins > CP_MAX_THETA_BINS) { c->err = "angle_bins must be 0 .. " + std::to_string(CP_MAX_THETA_BINS); return -1; }
    if (r.abins && (!r.ahist || !r.awhist)) { c->err = "angle_bins needs angle_histograms and weighted_angle_histograms"; return -1; }
    if (r.tbins < 1 || r.tbins > CP_MAX_THETA_BINS) { c->err = "relative_angle_bins must be 1 .. " + std::to_string(CP_MAX_THETA_BINS); return -1; }
    if (!r.thist || !r.twhist || !r.jcounts) { c->err = "relative_angle_histogram, weighted_relative_angle_histogram and joint_counts are required"; return -1; }
    const bool joint = r.jedges[0] || r.jedges[1];
    if (joint) {
        if (!r.jedges[0] || !r.jedges[1] || !r.jhist) { c->err = "joint_speed_edges_a, joint_speed_edges_b and joint_speed_histogram go together"; return -1; }
        for (int ch = 0; ch < 2; ++ch) {
            if (r.jbins[ch] < 1 || r.jbins[ch] > CP_MAX_SPEED_BINS) { c->err = "joint_speed_bins must be 1 .. " + std::to_string(CP_MAX_SPEED_BINS) + " per axis"; return -1; }
            if (!(r.jedges[ch][r.jbins[ch]] > r.jedges[ch][0])) { c->err = "joint_speed_edges must increase"; return -1; }
        }
    }
    const size_t fs = frame_stride(c);
    const int P = r.n_frames - 1;
    const int ba = joint ? r.jbins[0] : 0, bb = joint ? r.jbins[1] : 0;
    const size_t n_taps[2] = {r.taps[0] ? 2 * (size_t)r.radius[0] + 1 : 0, r.taps[1] ? 2 * (size_t)r.radius[1] + 1 : 0};
    const size_t n_twsum = (size_t)P * r.tbins, n_jhist = (size_t)ba * bb;
    const int cp_blk = cp_blocks(fs);
    // the arena: cap + 1 frames of the channel in progress and four chunk outputs per channel and pair in flight; what the
    // comparison's own kernels read and write; the tail's; the comparison's counters
    Scratch sc(c);
    double *frames, *chunk_out[2][4], *blur_tmp = nullptr, *bf_planes = nullptr, *d_taps[2], *d_tedges, *d_jedges[2], *d_twsum, *d_tpart;
    unsigned long long *d_thist, *d_jhist, *d_jc;
    DirectionHist dir;
    sc.per_unit_plus_one(&frames, fs);
    for (auto& ch : chunk_out) for (double*& q : ch) sc.per_unit(&q, fs);
    if (r.taps[0] || r.taps[1]) blur_regions(sc, sweep_want(c, r) + 1, &blur_tmp);
    box_flow_regions(sc, r.box_size, &bf_planes);
    for (int ch = 0; ch < 2; ++ch) { sc.once(&d_taps[ch], n_taps[ch]); sc.once(&d_jedges[ch], joint ? (size_t)r.jbins[ch] + 1 : 0); }
    dir.regions(sc, r.abins, 2, P);
    sc.once(&d_tedges, (size_t)r.tbins + 1);
    sc.once(&d_twsum, n_twsum);
    sc.per_unit(&d_tpart, (size_t)cp_blk * r.tbins);
    SweepTail tail;
    sweep_tail_regions(sc, tail, r, "channel comparison", 2);
    dir.counters(sc);
    sc.once(&d_thist, (size_t)r.tbins);
    sc.once(&d_jhist, n_jhist);
    sc.once(&d_jc, 2);
    const int cap = sweep_tail_begin(sc, tail, " for one pair");
    if (cap < 0) return cap;
    for (int ch = 0; ch < 2; ++ch) {
        if (r.taps[ch]) if (int rc = h2d_bounced(c, d_taps[ch], r.taps[ch], n_taps[ch] * 8)) return rc;
        if (joint) if (int rc = h2d_bounced(c, d_jedges[ch], r.jedges[ch], ((size_t)r.jbins[ch] + 1) * 8)) return rc;
    }
    if (int rc = dir.upload_edges(c)) return rc;
    {
        const std::vector<double> e = linspace_edges(0.0, 1.0, r.tbins);
        if (int rc = h2d_bounced(c, d_tedges, e.data(), e.size() * 8)) return rc;
    }
    SweepBase chan[2] = {r, r};            // a channel as a sweep of one entry: where its fields go
    chan[1].movie = r.movie_b;
    for (int f = 0; f < 4; ++f) chan[1].outs[f] = r.outs_b[f];

    for (int k0 = 0; k0 < P; k0 += cap) {
        const int np = std::min(cap, P - k0);
        SweepDst d[2];
        for (int ch = 0; ch < 2; ++ch) {
            const double* src;
            if (int rc = pair_chunk_frames(c, chan[ch], k0, np, frames, r.taps[ch] ? d_taps[ch] : nullptr, r.radius[ch], blur_tmp, &src)) return rc;
            d[ch] = sweep_dst(chan[ch], chunk_out[ch], fs, 0, k0);
            // exactly vof_box_flow_dev: the same kernels, the same choice between the fused and the general path
            if (int rc = box_flow_pairs(c, bf_planes, src, np, r.box_size, r.delta_x, r.delta_t, r.remodel, r.quirks, d[ch].f[0], d[ch].f[1],
                                        d[ch].f[2], d[ch].keep_g ? d[ch].f[3] : nullptr)) return rc;
            sweep_tail_speed(c, tail, ch, k0, np, d[ch].f[2]);
            dir.enqueue(c, ch, k0, np, d[ch].f[0], d[ch].f[1], d[ch].f[2]);
            if (int rc = sweep_tail_moments(c, tail, ch, k0, np, d[ch].f[2], d[ch].f[3])) return rc;
        }
        {
            CompareArgs a{};
            a.vxa = d[0].f[0]; a.vya = d[0].f[1]; a.spa = d[0].f[2];
            a.vxb = d[1].f[0]; a.vyb = d[1].f[1]; a.spb = d[1].f[2];
            a.fs = fs;
            a.tedges = d_tedges; a.tbins = r.tbins;
            a.ea = d_jedges[0]; a.eb = d_jedges[1]; a.ba = ba; a.bb = bb;
            a.has_min = r.jmin ? 1 : 0; a.min_b = r.jmin ? *r.jmin : 0.0;
            a.clip = r.quirks ? 0 : 1;
            a.thist = d_thist; a.jhist = d_jhist; a.counters = d_jc;
            a.partials = d_tpart;
            c->cur_units = np;
            Prof prof(c, VOF_K_REDUCE, 0, 48.0 * fs);
            k_cp_joint<<<dim3(cp_blk, np), 64, cp_lds(r.tbins, ba, bb), c->stream>>>(a);
            const int nt = np * r.tbins;
            k_bz_angle_sum<<<(nt + 255) / 256, 256, 0, c->stream>>>(d_tpart, cp_blk, r.tbins, np, d_twsum + (size_t)k0 * r.tbins);
        }
        if (hipGetLastError() != hipSuccess) { c->err = "channel comparison: launch failed"; return -2; }
        for (int ch = 0; ch < 2; ++ch)
            if (int rc = sweep_copy_out(c, chan[ch], d[ch], fs, np)) return rc;
    }
    if (int rc = sweep_tail_finish(c, tail, r.stats)) return rc;
    if (int rc = dir.finish(c, tail, r.ahist, r.awhist)) return rc;
    std::vector<double> twsum(n_twsum);
    if (int rc = d2h_bounced(c, twsum.data(), d_twsum, n_twsum * 8)) return rc;
    for (int b = 0; b < r.tbins; ++b) r.thist[b] = (int64_t)tail.host(d_thist)[b];
    for (size_t t = 0; t < n_jhist; ++t) r.jhist[t] = (int64_t)tail.host(d_jhist)[t];
    r.jcounts[0] = (int64_t)tail.host(d_jc)[0]; r.jcounts[1] = (int64_t)tail.host(d_jc)[1];
    sum_pair_histograms(twsum.data(), P, r.tbins, r.twhist);
    for (int ch = 0; ch < 2; ++ch) r.stats[ch].channel = ch;
    return 0;
}

#define VOF_COMPARE_ARGS                                                                                                              \
    vof_ctx *c, const double *movie_a, const double *movie_b, int n_frames, const double *blur_weights_a, int blur_radius_a,          \
        const double *blur_weights_b, int blur_radius_b, int box_size, double delta_x, double delta_t, int include_remodelling,       \
        int reference_quirks, const double *histogram_edges, int histogram_bins, int64_t *histograms, int angle_bins,                 \
        int64_t *angle_histograms, double *weighted_angle_histograms, int relative_angle_bins, int64_t *relative_angle_histogram,     \
        double *weighted_relative_angle_histogram, const double *joint_speed_edges_a, int joint_speed_bins_a,                         \
        const double *joint_speed_edges_b, int joint_speed_bins_b, const double *joint_speed_min_b, int64_t *joint_speed_histogram,   \
        int64_t *joint_counts, vof_compare_stats *stats, double *v_x_a, double *v_y_a, double *speed_a, double *net_remodelling_a,    \
        double *v_x_b, double *v_y_b, double *speed_b, double *net_remodelling_b
#define VOF_COMPARE_REQ(host)                                                                                                         \
    CompareReq{{movie_a, n_frames, delta_x, delta_t, include_remodelling, reference_quirks, histogram_edges, histogram_bins,          \
                histograms, nullptr, 0, nullptr, {v_x_a, v_y_a, speed_a, net_remodelling_a}, host},                                   \
               movie_b, {blur_weights_a, blur_weights_b}, {blur_radius_a, blur_radius_b}, box_size, angle_bins, angle_histograms,     \
               weighted_angle_histograms, relative_angle_bins, relative_angle_histogram, weighted_relative_angle_histogram,           \
               {joint_speed_edges_a, joint_speed_edges_b}, {joint_speed_bins_a, joint_speed_bins_b}, joint_speed_min_b,               \
               joint_speed_histogram, joint_counts, {v_x_b, v_y_b, speed_b, net_remodelling_b}, stats}

int vof_compare_flows_dev(VOF_COMPARE_ARGS) { return compare_flows_impl(c, VOF_COMPARE_REQ(false)); }
int vof_compare_flows_host(VOF_COMPARE_ARGS) { return compare_flows_impl(c, VOF_COMPARE_REQ(true)); }

// ---- preprocessing: adaptive threshold and CLAHE (apply_adaptive_threshold, apply_clahe; vof_preprocess.hpp) ---------------
static int adaptive_threshold_impl(vof_ctx* c, const double* movie, int n_frames, int window, double threshold, int flight, uint8_t* mask,
                                   double* range, bool host) {
    if (int rc = FrameChunks::check(c, {movie, mask}, n_frames, "n_frames")) return rc;
    if (window < 3 || window % 2 == 0 || window > PP_MAX_WINDOW) { c->err = "window_size must be odd and 3 .. " + std::to_string(PP_MAX_WINDOW); return -1; }
    if (c->Nj > PP_MAX_ROW) { c->err = "adaptive threshold: n_j must be <= " + std::to_string(PP_MAX_ROW); return -1; }
    if (c->Ni > 65535 * PP_COL_ROWS) { c->err = "adaptive threshold: n_i too large"; return -1; }
    if (std::isnan(threshold)) { c->err = "threshold is NaN"; return -1; }
    const size_t fs = frame_stride(c);
    FrameChunks fc(c, "adaptive threshold", n_frames, flight, host);
    unsigned int* H;                                                                     // row sums
    fc.sc.per_unit(&H, fs);
    fc.input(movie);
    fc.output(mask, fs);
    if (int rc = fc.plan()) return rc;
    if (int rc = fc.range(0, 0.0, INFINITY, "negative values", "", range)) return rc;
    const double m = fc.rg[0];
    if (!(m > 0)) { c->err = "adaptive threshold: the movie's maximum is not positive"; return 1; }
    const int r = window / 2;
    const int idelta = (int)std::max(-1024.0, std::min(1024.0, std::ceil(threshold)));   // u - mean lies in [-255, 255]
    return fc.run([&](int, int nf, const double* const* in, void* const* out) {
        {
            Prof prof(c, VOF_K_PREPROCESS, PP_ST_ROWSUM, 12.0 * fs);
            k_pp_rowsum<<<dim3(c->Ni, nf), PP_BLOCK, (size_t)c->Nj * sizeof(unsigned int), c->stream>>>(in[0], c->Ni, c->Nj, m, r, H);
        }
        {
            Prof prof(c, VOF_K_PREPROCESS, PP_ST_THRESHOLD, 13.0 * fs);
            k_pp_threshold<<<dim3((c->Nj + PP_BLOCK - 1) / PP_BLOCK, (c->Ni + PP_COL_ROWS - 1) / PP_COL_ROWS, nf), PP_BLOCK, 0, c->stream>>>(
                in[0], H, c->Ni, c->Nj, m, r, idelta, (uint8_t*)out[0]);
        }
        return 0;
    });
}

int vof_adaptive_threshold_dev(vof_ctx* c, const double* movie, int n_frames, int window_size, double threshold, int frames_in_flight,
                               uint8_t* mask, double* range) {
    return adaptive_threshold_impl(c, movie, n_frames, window_size, threshold, frames_in_flight, mask, range, false);
}
int vof_adaptive_threshold_host(vof_ctx* c, const double* movie, int n_frames, int window_size, double threshold, int frames_in_flight,
                                uint8_t* mask, double* range) {
    return adaptive_threshold_impl(c, movie, n_frames, window_size, threshold, frames_in_flight, mask, range, true);
}

static int clahe_impl(vof_ctx* c, const double* movie, int n_frames, double clip_limit, int tiles_x, int tiles_y, int flight, double* out,
                      double* range, bool host) {
    if (int rc = FrameChunks::check(c, {movie, out}, n_frames, "n_frames")) return rc;
    if (tiles_x < 1 || tiles_x > c->Nj - 1 || tiles_y < 1 || tiles_y > c->Ni - 1) {
        c->err = "CLAHE: the tile grid must be 1 .. n_j - 1 by 1 .. n_i - 1"; return -1;
    }
    if (std::isnan(clip_limit)) { c->err = "clip_limit is NaN"; return -1; }
    ClaheGeom g{};
    g.ni = c->Ni; g.nj = c->Nj; g.tx = tiles_x; g.ty = tiles_y;
    const bool pad = g.nj % g.tx != 0 || g.ni % g.ty != 0;          // one axis not dividing pads both, a dividing one by a full grid
    g.pj = pad ? g.nj + (g.tx - g.nj % g.tx) : g.nj;
    g.pi = pad ? g.ni + (g.ty - g.ni % g.ty) : g.ni;
    g.tw = g.pj / g.tx; g.th = g.pi / g.ty;
    const long long area = (long long)g.tw * g.th;
    if (g.pi > 65535 || area > 0x7FFFFFFFLL) { c->err = "CLAHE: image too large"; return -1; }
    if (clip_limit > 0) {
        const double cl = clip_limit * (double)area / (double)PP_BINS;
        g.clip = std::max(cl >= 2147483647.0 ? 2147483647 : (int)cl, 1);
    }
    g.lut_scale = (float)(PP_BINS - 1) / (float)area;
    g.inv_tw = 1.0f / (float)g.tw; g.inv_th = 1.0f / (float)g.th;
    const size_t fs = frame_stride(c);
    const size_t ntiles = (size_t)g.tx * g.ty, hist_bytes = ntiles * PP_BINS * sizeof(unsigned int), lut_bytes = ntiles * PP_BINS * sizeof(uint16_t);
    FrameChunks fc(c, "CLAHE", n_frames, flight, host);
    unsigned int* hist;
    uint16_t* lut;
    fc.sc.per_unit(&hist, ntiles * PP_BINS);
    fc.sc.per_unit(&lut, ntiles * PP_BINS);
    fc.input(movie);
    fc.output(out, fs * sizeof(double));
    if (int rc = fc.plan()) return rc;
    if (int rc = fc.range(0, 0.0, std::nextafter(65536.0, 0.0), "values outside [0, 65536)", "", range)) return rc;   // hi: the last double below 65536
    const double padded = (double)g.pi * g.pj;
    return fc.run([&](int, int nf, const double* const* in, void* const* dst) -> int {
        {
            Prof prof(c, VOF_K_PREPROCESS, PP_ST_HIST, 8.0 * padded + 2.0 * hist_bytes);   // the zero fill and the counters read back
            HIPCHK(hipMemsetAsync(hist, 0, (size_t)nf * hist_bytes, c->stream));
            k_pp_hist<<<dim3((g.pj + PP_BLOCK - 1) / PP_BLOCK, g.pi, nf), PP_BLOCK, 0, c->stream>>>(in[0], g, hist);
        }
        {
            Prof prof(c, VOF_K_PREPROCESS, PP_ST_LUT, (g.clip > 0 ? 2.0 : 1.0) * hist_bytes + lut_bytes, (double)hist_bytes + lut_bytes);
            k_pp_lut<<<dim3((unsigned)ntiles, nf), PP_BLOCK, 0, c->stream>>>(hist, g, lut);
        }
        {
            Prof prof(c, VOF_K_PREPROCESS, PP_ST_BLEND, 24.0 * fs, 16.0 * fs);             // 4 table entries of 2 bytes from the cache
            k_pp_blend<<<dim3((g.nj + PP_BLOCK - 1) / PP_BLOCK, g.ni, nf), PP_BLOCK, 0, c->stream>>>(in[0], g, lut, (double*)dst[0]);
        }
        return 0;
    });
}

int vof_clahe_dev(vof_ctx* c, const double* movie, int n_frames, double clip_limit, int tiles_x, int tiles_y, int frames_in_flight,
                  double* out, double* range) {
    return clahe_impl(c, movie, n_frames, clip_limit, tiles_x, tiles_y, frames_in_flight, out, range, false);
}
int vof_clahe_host(vof_ctx* c, const double* movie, int n_frames, double clip_limit, int tiles_x, int tiles_y, int frames_in_flight,
                   double* out, double* range) {
    return clahe_impl(c, movie, n_frames, clip_limit, tiles_x, tiles_y, frames_in_flight, out, range, true);
}

// ---- INTER_AREA downsampling (downsample_movie; vof_resize.hpp) --------------------------------------------------------------
// One axis of cv2.resize's INTER_AREA: the two roundings of the scale, and computeResizeAreaTab in C++ double exactly as OpenCV
// writes it; the entries of an output index are consecutive source indices, so (first index, count, weights) holds them.
struct ResizeAxis {
    double scale = 1.0;
    int iscale = 1, kmax = 0;
    std::vector<int> start, count;
    std::vector<float> w;                  // [d * kmax + k]
};

static void resize_axis_scale(int ssize, int dsize, ResizeAxis* t) {
    const double inv = (double)dsize / (double)ssize;
    t->scale = 1.0 / inv;
    t->iscale = (int)t->scale;
}

static bool resize_axis_table(int ssize, int dsize, ResizeAxis* t) {
#pragma clang fp contract(off)
    const double scale = t->scale;
    std::vector<std::vector<float>> ws((size_t)dsize);
    t->start.assign((size_t)dsize, 0);
    t->count.assign((size_t)dsize, 0);
    t->kmax = 0;
    int prev_start = 0, prev_end = 0;
    for (int d = 0; d < dsize; ++d) {
        const double f1 = d * scale;
        const double f2 = f1 + scale;
        const double cw = std::min(scale, ssize - f1);
        int s1 = (int)std::ceil(f1);
        const int s2 = std::min((int)std::floor(f2), ssize - 1);
        s1 = std::min(s1, s2);
        std::vector<float>& w = ws[(size_t)d];
        int first = s1;
        if (s1 - f1 > 1e-3) { first = s1 - 1; w.push_back((float)((s1 - f1) / cw)); }
        for (int s = s1; s < s2; ++s) w.push_back((float)(1.0 / cw));
        if (f2 - s2 > 1e-3) {
            if (w.empty()) first = s2;
            w.push_back((float)(std::min(std::min(f2 - s2, 1.0), cw) / cw));
        }
        const int n = (int)w.size(), end = first + n;
        // what the kernel's staging relies on: a non-empty run inside the row, runs that move right with d
        if (n < 1 || first < 0 || end > ssize || first < prev_start || end < prev_end) return false;
        prev_start = first; prev_end = end;
        t->start[(size_t)d] = first; t->count[(size_t)d] = n;
        t->kmax = std::max(t->kmax, n);
    }
    t->w.assign((size_t)dsize * t->kmax, 0.0f);
    for (int d = 0; d < dsize; ++d) std::copy(ws[(size_t)d].begin(), ws[(size_t)d].end(), t->w.begin() + (size_t)d * t->kmax);
    return true;
}

static int resize_area_impl(vof_ctx* c, const double* movie, int n_frames, int out_i, int out_j, int arithmetic, int flight, double* out,
                            bool host) {
    if (int rc = FrameChunks::check(c, {movie, out}, n_frames, "n_frames")) return rc;
    if (arithmetic != VOF_RESIZE_U8 && arithmetic != VOF_RESIZE_F64) { c->err = "resize: arithmetic must be VOF_RESIZE_U8 or VOF_RESIZE_F64"; return -1; }
    if (out_i < 1 || out_i > c->Ni || out_j < 1 || out_j > c->Nj) {
        c->err = "resize: 1 <= out_i <= n_i and 1 <= out_j <= n_j are required (downsampling only)"; return -1;
    }
    if (out_i > 65535) { c->err = "resize: out_i must be <= 65535"; return -1; }
    const bool u8 = arithmetic == VOF_RESIZE_U8;
    ResizeAxis ty, tx;
    resize_axis_scale(c->Ni, out_i, &ty);
    resize_axis_scale(c->Nj, out_j, &tx);
    const bool fast = std::fabs(tx.scale - tx.iscale) < DBL_EPSILON && std::fabs(ty.scale - ty.iscale) < DBL_EPSILON;
    std::vector<uint32_t> tab;                                          // start_y, count_y, start_x, count_x, w_y, w_x
    if (fast) {
        if ((long long)ty.iscale * out_i != c->Ni || (long long)tx.iscale * out_j != c->Nj) { c->err = "internal: resize scales"; return -1; }
        if ((long long)ty.iscale * tx.iscale > 0x7FFFFFFFLL / 255) { c->err = "resize: more than 2^23 source pixels per output pixel"; return -1; }
    } else {
        if (!resize_axis_table(c->Ni, out_i, &ty) || !resize_axis_table(c->Nj, out_j, &tx)) { c->err = "internal: resize table"; return -1; }
        tab.resize(2 * (size_t)out_i + 2 * (size_t)out_j + ty.w.size() + tx.w.size());
        uint32_t* q = tab.data();
        for (const ResizeAxis* t : {&ty, &tx}) {
            memcpy(q, t->start.data(), t->start.size() * 4); q += t->start.size();
            memcpy(q, t->count.data(), t->count.size() * 4); q += t->count.size();
        }
        memcpy(q, ty.w.data(), ty.w.size() * 4); q += ty.w.size();
        memcpy(q, tx.w.data(), tx.w.size() * 4);
    }
    const size_t fs = frame_stride(c), os = (size_t)out_i * out_j;
    FrameChunks fc(c, "resize", n_frames, flight, host);
    int* q;                                                             // the axis tables on the device
    fc.sc.once(&q, tab.size());
    fc.input(movie);
    fc.output(out, os * sizeof(double));
    if (int rc = fc.plan()) return rc;
    if (u8) if (int rc = fc.range(0, 0.0, 255.0, "values outside 0 .. 255", " (uint8 arithmetic)")) return rc;
    RsAxis ay{}, ax{};
    if (!fast) {
        if (int rc = h2d_bounced(c, q, tab.data(), tab.size() * 4)) return rc;
        ay.start = q; ay.count = q + out_i; ax.start = q + 2 * (size_t)out_i; ax.count = ax.start + out_j;
        ay.w = (const float*)(ax.count + out_j); ax.w = ay.w + ty.w.size();
        ay.kmax = ty.kmax; ax.kmax = tx.kmax;
    }
    const float scale_f = 1.0f / (float)(tx.iscale * ty.iscale);
    const int half_up = tx.iscale == 2 && ty.iscale == 2;
    return fc.run([&](int, int nf, const double* const* in, void* const* out_dev) {
        const double* src = in[0];
        double* dst = (double*)out_dev[0];
        Prof prof(c, VOF_K_PREPROCESS, PP_ST_RESIZE, 8.0 * fs + 8.0 * os);
        const dim3 grid((out_j + RS_BLOCK - 1) / RS_BLOCK, out_i, nf);
        if (fast && u8) k_rs_fast<true><<<grid, RS_BLOCK, 0, c->stream>>>(src, c->Ni, c->Nj, out_i, out_j, ty.iscale, tx.iscale, scale_f, half_up, dst);
        else if (fast) k_rs_fast<false><<<grid, RS_BLOCK, 0, c->stream>>>(src, c->Ni, c->Nj, out_i, out_j, ty.iscale, tx.iscale, scale_f, 0, dst);
        else if (u8) k_rs_area<true><<<grid, RS_BLOCK, 0, c->stream>>>(src, c->Ni, c->Nj, out_i, out_j, ay, ax, dst);
        else k_rs_area<false><<<grid, RS_BLOCK, 0, c->stream>>>(src, c->Ni, c->Nj, out_i, out_j, ay, ax, dst);
        return 0;
    });
}

int vof_resize_area_dev(vof_ctx* c, const double* movie, int n_frames, int out_i, int out_j, int arithmetic, int frames_in_flight, double* out) {
    return resize_area_impl(c, movie, n_frames, out_i, out_j, arithmetic, frames_in_flight, out, false);
}
int vof_resize_area_host(vof_ctx* c, const double* movie, int n_frames, int out_i, int out_j, int arithmetic, int frames_in_flight, double* out) {
    return resize_area_impl(c, movie, n_frames, out_i, out_j, arithmetic, frames_in_flight, out, true);
}

// ---- Farnebaeck's dense flow (conduct_opencv_flow; vof_farneback.hpp) ---------------------------------------------------------
// The float32 planes of one pair in flight, each n_i * n_j floats long whatever the level (a level's planes are compact at
// the start of their slots): FB_PLANES in all with the Gaussian window; FB_BOX_PLANES with the box window, whose V is five
// double planes (the slot of ten float32 ones; a pair's planes start at a multiple of 256 bytes, so V is aligned).
enum FbWindow { FB_GAUSSIAN, FB_BOX };
struct FbPair {
    float *tmp_a, *tmp_b, *image, *R[2], *M, *V, *flow[2];
    explicit FbPair(float* q, size_t fs, FbWindow window) {
        tmp_a = q; tmp_b = q + fs; image = q + 2 * fs; R[0] = q + 3 * fs; R[1] = q + 8 * fs; M = q + 13 * fs; V = q + 18 * fs;
        flow[0] = V + (window == FB_BOX ? 10 : 5) * fs; flow[1] = flow[0] + 2 * fs;
    }
};

static int farneback_impl(vof_ctx* c, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes,
                          const int* ksizes, const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig,
                          FbWindow window, int winsize, const float* window_taps, int iterations, float flow_scale, double velocity_scale,
                          int flight, double* v_x, double* v_y, double* speed, bool host) {
    const bool box = window == FB_BOX;                                          // no taps: the window is two running sums
    if (int rc = FrameChunks::check(c, {first, second, v_x, v_y, speed, level_sizes, ksizes, presmooth_taps, poly_tables, poly_ig,
                                        box ? (const void*)first : window_taps}, n_pairs, "n_pairs")) return rc;
    if (c->Ni < 16 || c->Nj < 16) { c->err = "Farneback flow: frames must be at least 16 x 16"; return -1; }
    if (n_levels < 1 || n_levels > 64) { c->err = "Farneback flow: 1 .. 64 pyramid images"; return -1; }
    if (poly_n < 1 || poly_n > FB_MAX_POLY_N) { c->err = "Farneback flow: poly_n must be 1 .. " + std::to_string(FB_MAX_POLY_N); return -1; }
    if (winsize < 1 || winsize > FB_MAX_WINSIZE) { c->err = "Farneback flow: winsize must be 1 .. " + std::to_string(FB_MAX_WINSIZE); return -1; }
    if (box && winsize < 2) {
        c->err = "Farneback flow: the box window needs winsize >= 2 (at winsize 1 OpenCV's running sums start with row 0 and column 0 counted once too often)";
        return -1;
    }
    if (iterations < 0) { c->err = "Farneback flow: iterations must be >= 0"; return -1; }
    if (level_sizes[0] != c->Ni || level_sizes[1] != c->Nj) { c->err = "Farneback flow: level 0 must have the frame's size"; return -1; }
    size_t n_taps = 0;
    std::vector<size_t> tap_at((size_t)n_levels);
    for (int k = 0; k < n_levels; ++k) {
        const int h = level_sizes[2 * k], w = level_sizes[2 * k + 1];
        if (h < 1 || w < 1 || h > c->Ni || w > c->Nj || h > 65535) { c->err = "Farneback flow: a level's size must be 1 .. the frame's (65535 rows at most)"; return -1; }
        if (ksizes[k] < 1 || ksizes[k] % 2 == 0 || ksizes[k] > 65535) { c->err = "Farneback flow: a level's tap count must be odd"; return -1; }
        tap_at[(size_t)k] = n_taps;
        n_taps += (size_t)ksizes[k];
    }
    const int m = winsize / 2, poly_len = 3 * (2 * poly_n + 1);
    std::vector<float> tab(n_taps + (size_t)poly_len + (box ? 0 : (size_t)m + 1));   // pre-smoothing taps | g, xg, xxg | Gaussian window taps
    memcpy(tab.data(), presmooth_taps, n_taps * sizeof(float));
    memcpy(tab.data() + n_taps, poly_tables, (size_t)poly_len * sizeof(float));
    if (!box) memcpy(tab.data() + n_taps + poly_len, window_taps, ((size_t)m + 1) * sizeof(float));
    const FbInvG ig{poly_ig[0], poly_ig[1], poly_ig[2], poly_ig[3]};
    const size_t fs = frame_stride(c);
    FrameChunks fc(c, "Farneback flow", n_pairs, flight, host);
    float *planes, *d_tab;
    const size_t ps = fc.sc.per_unit(&planes, (size_t)(box ? FB_BOX_PLANES : FB_PLANES) * fs, true);   // floats from a pair's planes to the next pair's
    fc.sc.once(&d_tab, tab.size());
    fc.input(first);
    fc.input(second);
    for (double* field : {v_x, v_y, speed}) fc.output(field, fs * sizeof(double));
    if (int rc = fc.plan()) return rc;
    for (int s = 0; s < 2; ++s) if (int rc = fc.range(s, -INFINITY, INFINITY, "")) return rc;
    if (int rc = h2d_bounced(c, d_tab, tab.data(), tab.size() * sizeof(float))) return rc;
    const float *d_poly = d_tab + n_taps, *d_win = d_poly + poly_len;
    const FbPair q(planes, fs, window);
    const double box_scale = 1.0 / (double)(winsize * winsize);
    const size_t vblur_lds = (size_t)(FB_VB_ROWS + 2 * m) * FB_VB_COLS * sizeof(float);
    return fc.run([&](int, int nf, const double* const* src, void* const* dst) -> int {
        int cur = 0;                                                            // q.flow[cur]: the flow of the level in progress
        for (int lv = n_levels - 1; lv >= 0; --lv) {
            const int h = level_sizes[2 * lv], w = level_sizes[2 * lv + 1], r = ksizes[lv] / 2;
            const size_t hw = (size_t)h * w;
            const float* d_w = d_tab + tap_at[(size_t)lv];
            const dim3 full((c->Nj + FB_BLOCK - 1) / FB_BLOCK, c->Ni, nf), rows((w + FB_BLOCK - 1) / FB_BLOCK, h, nf);
            for (int role = 0; role < 2; ++role) {
                {
                    Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_LEVEL, 8.0 * fs + 12.0 * fs + 4.0 * hw);
                    k_fb_smooth<double, true><<<full, FB_BLOCK, 0, c->stream>>>(src[role], fs, c->Ni, c->Nj, d_w, r, q.tmp_a, ps);
                    k_fb_smooth<float, false><<<full, FB_BLOCK, 0, c->stream>>>(q.tmp_a, ps, c->Ni, c->Nj, d_w, r, q.tmp_b, ps);
                    k_fb_resize<false><<<rows, FB_BLOCK, 0, c->stream>>>(q.tmp_b, ps, c->Ni, c->Nj, q.image, ps, h, w, 1.0 / ((double)h / c->Ni),
                                                                         1.0 / ((double)w / c->Nj), 1, 1.0f);
                }
                {
                    Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_POLY, 24.0 * hw);
                    k_fb_polyexp<<<rows, FB_BLOCK, 0, c->stream>>>(q.image, ps, h, w, poly_n, d_poly, ig, q.R[role], ps);
                }
            }
            {
                Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_FLOW, 8.0 * hw);
                if (lv == n_levels - 1) {
                    for (int k = 0; k < nf; ++k) HIPCHK(hipMemsetAsync(q.flow[cur] + (size_t)k * ps, 0, 2 * hw * sizeof(float), c->stream));
                } else {
                    const int sh = level_sizes[2 * lv + 2], sw = level_sizes[2 * lv + 3];
                    k_fb_resize<true><<<dim3(rows.x, h, 2 * nf), FB_BLOCK, 0, c->stream>>>(q.flow[cur ^ 1], ps, sh, sw, q.flow[cur], ps, h, w,
                                                                                         1.0 / ((double)h / sh), 1.0 / ((double)w / sw), 2, flow_scale);
                }
            }
            if (iterations > 0) {
                Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_MATRICES, 68.0 * hw);
                k_fb_matrices<<<rows, FB_BLOCK, 0, c->stream>>>(q.R[0], q.R[1], q.flow[cur], q.M, ps, h, w);
            }
            for (int it = 0; it < iterations; ++it) {
                const bool rebuild = it < iterations - 1;
                if (box) {
                    {
                        Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_BOX_ROWS, 80.0 * hw, 60.0 * hw);     // the row leaving the window is re-read from the caches
                        k_fb_box_rows<FB_BR_LOOK><<<dim3((w + FB_BR_BLOCK - 1) / FB_BR_BLOCK, 1, 5 * nf), FB_BR_BLOCK, 0, c->stream>>>(
                            q.M, ps, (double*)q.V, ps / 2, h, w, m);
                    }
                    Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_BOX_UPDATE, (rebuild ? 148.0 : 88.0) * hw, (rebuild ? 108.0 : 48.0) * hw);   // likewise the column
                    k_fb_box_update<<<dim3((h + FB_BU_ROWS - 1) / FB_BU_ROWS, 1, nf), FB_BLOCK, 0, c->stream>>>(
                        (const double*)q.V, ps / 2, q.R[0], q.R[1], q.flow[cur], q.M, ps, h, w, m, box_scale, rebuild ? 1 : 0);
                    continue;
                }
                {
                    Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_VBLUR, 40.0 * hw);
                    k_fb_vblur<<<dim3((w + FB_VB_COLS - 1) / FB_VB_COLS, (h + FB_VB_ROWS - 1) / FB_VB_ROWS, 5 * nf), FB_BLOCK, vblur_lds, c->stream>>>(
                        q.M, q.V, ps, h, w, m, d_win);
                }
                {
                    Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_UPDATE, (rebuild ? 88.0 : 28.0) * hw);
                    k_fb_update<<<rows, FB_BLOCK, 0, c->stream>>>(q.V, q.R[0], q.R[1], q.flow[cur], q.M, ps, h, w, m, d_win, rebuild ? 1 : 0);
                }
            }
            HIPCHK(hipGetLastError());
            cur ^= 1;
        }
        cur ^= 1;                                                               // the finished level 0
        Prof prof(c, VOF_K_PREPROCESS, PP_ST_FB_OUT, 32.0 * fs);
        k_fb_output<<<dim3((unsigned)((fs + FB_BLOCK - 1) / FB_BLOCK), 1, nf), FB_BLOCK, 0, c->stream>>>(q.flow[cur], ps, fs, velocity_scale, (double*)dst[0],
                                                                                                        (double*)dst[1], (double*)dst[2]);
        return 0;
    });
}

int vof_farneback_dev(vof_ctx* c, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes, const int* ksizes,
                      const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig, int winsize, const float* window_taps,
                      int iterations, float flow_scale, double velocity_scale, int frames_in_flight, double* v_x, double* v_y, double* speed) {
    return farneback_impl(c, first, second, n_pairs, n_levels, level_sizes, ksizes, presmooth_taps, poly_n, poly_tables, poly_ig, FB_GAUSSIAN, winsize,
                          window_taps, iterations, flow_scale, velocity_scale, frames_in_flight, v_x, v_y, speed, false);
}
int vof_farneback_host(vof_ctx* c, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes, const int* ksizes,
                       const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig, int winsize, const float* window_taps,
                       int iterations, float flow_scale, double velocity_scale, int frames_in_flight, double* v_x, double* v_y, double* speed) {
    return farneback_impl(c, first, second, n_pairs, n_levels, level_sizes, ksizes, presmooth_taps, poly_n, poly_tables, poly_ig, FB_GAUSSIAN, winsize,
                          window_taps, iterations, flow_scale, velocity_scale, frames_in_flight, v_x, v_y, speed, true);
}
int vof_farneback_box_dev(vof_ctx* c, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes, const int* ksizes,
                          const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig, int winsize, int iterations,
                          float flow_scale, double velocity_scale, int frames_in_flight, double* v_x, double* v_y, double* speed) {
    return farneback_impl(c, first, second, n_pairs, n_levels, level_sizes, ksizes, presmooth_taps, poly_n, poly_tables, poly_ig, FB_BOX, winsize, nullptr,
                          iterations, flow_scale, velocity_scale, frames_in_flight, v_x, v_y, speed, false);
}
int vof_farneback_box_host(vof_ctx* c, const double* first, const double* second, int n_pairs, int n_levels, const int* level_sizes, const int* ksizes,
                           const float* presmooth_taps, int poly_n, const float* poly_tables, const double* poly_ig, int winsize, int iterations,
                           float flow_scale, double velocity_scale, int frames_in_flight, double* v_x, double* v_y, double* speed) {
    return farneback_impl(c, first, second, n_pairs, n_levels, level_sizes, ksizes, presmooth_taps, poly_n, poly_tables, poly_ig, FB_BOX, winsize, nullptr,
                          iterations, flow_scale, velocity_scale, frames_in_flight, v_x, v_y, speed, true);
}

// ---- two finished flow results: the result filter and the comparison (filter_PIV_flow_result, compare_flow_results;
// vof_flowcompare.hpp) ------------------------------------------------------------------------------
static int flow_filter_impl(vof_ctx* c, const double* movie, int n_pairs, const double* weights, int radius, double intensity, double limit,
                            int zero_low, int flight, double* v_x, double* v_y, double* speed, int64_t* counts, bool host) {
    if (int rc = FrameChunks::check(c, {movie, weights, v_x, v_y, speed, counts}, n_pairs, "n_pairs")) return rc;
    if (radius < 0 || radius > 4096) { c->err = "bad blur_radius"; return -1; }
    if (std::isnan(intensity) || std::isnan(limit)) { c->err = "flow filter: a threshold is NaN"; return -1; }
    const size_t fs = frame_stride(c);
    FrameChunks fc(c, "flow filter", n_pairs, flight, host);
    double *blurred, *tmp, *w;                                      // the blurred frames of one chunk: never a stack
    unsigned long long* d_counts;
    fc.sc.per_unit(&blurred, fs);
    blur_regions(fc.sc, n_pairs, &tmp, &w, radius);
    fc.sc.once(&d_counts, 2);
    fc.input(movie); fc.input(v_x); fc.input(v_y); fc.input(speed);
    fc.output(v_x, fs * sizeof(double)); fc.output(v_y, fs * sizeof(double)); fc.output(speed, fs * sizeof(double));
    if (int rc = fc.plan()) return rc;
    if (int rc = h2d_bounced(c, w, weights, (size_t)(2 * radius + 1) * sizeof(double))) return rc;
    HIPCHK(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), c->stream));
    if (int rc = fc.run([&](int, int nf, const double* const* in, void* const* out) -> int {
            if (int rc = blur_frames(c, in[0], blurred, nf, radius, tmp, w)) return rc;
            const size_t n = (size_t)nf * fs;
            const int blocks = (int)std::min<size_t>(2048, (n + 8 * FC_BLOCK - 1) / (8 * FC_BLOCK));
            Prof prof(c, VOF_K_REDUCE, FC_ST_MASK, 56.0 * fs);
            k_fc_mask<<<blocks, FC_BLOCK, 0, c->stream>>>(blurred, in[1], in[2], in[3], n, intensity, limit, zero_low, (double*)out[0],
                                                          (double*)out[1], (double*)out[2], d_counts);
            return 0;
        })) return rc;
    unsigned long long h[2];
    if (int rc = d2h_bounced(c, h, d_counts, sizeof h)) return rc;
    counts[0] = (int64_t)h[0]; counts[1] = (int64_t)h[1];
    return 0;
}

int vof_flow_filter_dev(vof_ctx* c, const double* movie, int n_pairs, const double* blur_weights, int blur_radius, double intensity_threshold,
                        double speed_threshold, int zero_speed_under_low, int frames_in_flight, double* v_x, double* v_y, double* speed,
                        int64_t* counts) {
    return flow_filter_impl(c, movie, n_pairs, blur_weights, blur_radius, intensity_threshold, speed_threshold, zero_speed_under_low,
                            frames_in_flight, v_x, v_y, speed, counts, false);
}
int vof_flow_filter_host(vof_ctx* c, const double* movie, int n_pairs, const double* blur_weights, int blur_radius, double intensity_threshold,
                         double speed_threshold, int zero_speed_under_low, int frames_in_flight, double* v_x, double* v_y, double* speed,
                         int64_t* counts) {
    return flow_filter_impl(c, movie, n_pairs, blur_weights, blur_radius, intensity_threshold, speed_threshold, zero_speed_under_low,
                            frames_in_flight, v_x, v_y, speed, counts, true);
}

// ---- the illumination correction and the intensity histograms (correct_intensity_change, intensity_histograms;
// vof_intensity.hpp) ---------------------------------------------------------------------------------
// The second blur of nf frames of b less the one frame ref, and the subtraction from target: the two fused passes, mid the
// row-filtered frames between them.  Radii BL_RMIN .. BL_RMAX take the LDS tiles, the others global memory: same bits.
static bool intensity_tiled(int radius) { return radius >= BL_RMIN && radius <= BL_RMAX; }

static int intensity_passes(vof_ctx* c, const double* b, const double* ref, const double* target, int nf, int radius, const double* w,
                            double* mid, double* out, double* drift) {
    const size_t fs = frame_stride(c);
    const bool tiled = intensity_tiled(radius);
    const dim3 g0((c->Nj + BX - 1) / BX, (c->Ni + BL_TI - 1) / BL_TI, nf), g1(g0.x, (c->Ni + BL_TR - 1) / BL_TR, nf), g = grid2d(c->Ni, c->Nj, nf);
    {
        Prof prof(c, VOF_K_PREPROCESS, PP_ST_IC_AXIS0, 24.0 * fs, 16.0 * fs);       // the reference frame is re-read from the caches
        if (tiled) k_ic_axis0_tiled<<<g0, blk2d, blur_tiled_lds(0, radius), c->stream>>>(b, ref, mid, c->Ni, c->Nj, w, radius);
        else k_ic_axis0<<<g, blk2d, 0, c->stream>>>(b, ref, mid, c->Ni, c->Nj, w, radius);
    }
    {
        Prof prof(c, VOF_K_PREPROCESS, PP_ST_IC_AXIS1, (drift ? 32.0 : 24.0) * fs);
        if (tiled && drift) k_ic_axis1_tiled<true><<<g1, blk2d, blur_tiled_lds(1, radius), c->stream>>>(mid, target, out, drift, c->Ni, c->Nj, w, radius);
        else if (tiled) k_ic_axis1_tiled<false><<<g1, blk2d, blur_tiled_lds(1, radius), c->stream>>>(mid, target, out, drift, c->Ni, c->Nj, w, radius);
        else if (drift) k_ic_axis1<true><<<g, blk2d, 0, c->stream>>>(mid, target, out, drift, c->Ni, c->Nj, w, radius);
        else k_ic_axis1<false><<<g, blk2d, 0, c->stream>>>(mid, target, out, drift, c->Ni, c->Nj, w, radius);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int intensity_correct_impl(vof_ctx* c, const double* movie, int n_frames, const double* w1_host, int r1, const double* w2_host, int r2,
                                  int reference_frame, int target, int flight, double* out, double* drift, bool host) {
    if (int rc = FrameChunks::check(c, {movie, w2_host, out}, n_frames, "n_frames")) return rc;
    if ((w1_host && (r1 < 0 || r1 > 4096)) || r2 < 0 || r2 > 4096) { c->err = "bad smoothing_radius / filter_radius"; return -1; }
    if (reference_frame < 0 || reference_frame >= n_frames) { c->err = "intensity correction: reference_frame outside the stack"; return -1; }
    if (target != VOF_INTENSITY_TARGET_BLURRED && target != VOF_INTENSITY_TARGET_ORIGINAL) { c->err = "intensity correction: unknown target"; return -1; }
    const size_t fs = frame_stride(c);
    FrameChunks fc(c, "intensity correction", n_frames, flight, host);
    // once per call: the (blurred) reference frame and the taps; per frame in flight: the blurred frame and the row-filtered one,
    // which is the first blur's scratch too (a chunk of at least BLUR_CHUNK frames is blurred BLUR_CHUNK at a time)
    double *bref = nullptr, *blurred = nullptr, *mid, *w1 = nullptr, *w2;
    if (w1_host || host) fc.sc.once(&bref, fs);
    if (w1_host) { fc.sc.per_unit(&blurred, fs); fc.sc.once(&w1, (size_t)2 * r1 + 1); }
    fc.sc.per_unit(&mid, fs);
    fc.sc.once(&w2, (size_t)2 * r2 + 1);
    fc.input(movie);
    fc.output(out, fs * sizeof(double));
    if (drift) fc.output(drift, fs * sizeof(double));
    if (int rc = fc.plan()) return rc;
    // the axis-0 tile takes up to 80 KiB of dynamic LDS, past the default limit: raised for its kernel before the walk, in every
    // call that takes the tiles (a host-side setting of a few microseconds; the context keeps no record of it)
    if (intensity_tiled(r2))
        HIPCHK(hipFuncSetAttribute((const void*)k_ic_axis0_tiled, hipFuncAttributeMaxDynamicSharedMemorySize, (int)blur_tiled_lds(0, BL_RMAX)));
    if (w1_host) if (int rc = h2d_bounced(c, w1, w1_host, (size_t)(2 * r1 + 1) * sizeof(double))) return rc;
    if (int rc = h2d_bounced(c, w2, w2_host, (size_t)(2 * r2 + 1) * sizeof(double))) return rc;
    const double* ref = movie + (size_t)reference_frame * fs;
    if (host) { if (int rc = h2d_bounced(c, bref, ref, fs * sizeof(double))) return rc; ref = bref; }
    c->cur_units = 1;
    if (w1_host) { if (int rc = blur_frames(c, ref, bref, 1, r1, mid, w1)) return rc; ref = bref; }
    return fc.run([&](int, int nf, const double* const* in, void* const* dst) -> int {
        const double* b = in[0];
        if (w1_host) { if (int rc = blur_frames(c, in[0], blurred, nf, r1, mid, w1)) return rc; b = blurred; }
        return intensity_passes(c, b, ref, target == VOF_INTENSITY_TARGET_BLURRED ? b : in[0], nf, r2, w2, mid, (double*)dst[0],
                                drift ? (double*)dst[1] : nullptr);
    });
}

int vof_intensity_correct_dev(vof_ctx* c, const double* movie, int n_frames, const double* smoothing_weights, int smoothing_radius,
                              const double* filter_weights, int filter_radius, int reference_frame, int target, int frames_in_flight,
                              double* out, double* drift) {
    return intensity_correct_impl(c, movie, n_frames, smoothing_weights, smoothing_radius, filter_weights, filter_radius, reference_frame, target,
                                  frames_in_flight, out, drift, false);
}
int vof_intensity_correct_host(vof_ctx* c, const double* movie, int n_frames, const double* smoothing_weights, int smoothing_radius,
                               const double* filter_weights, int filter_radius, int reference_frame, int target, int frames_in_flight,
                               double* out, double* drift) {
    return intensity_correct_impl(c, movie, n_frames, smoothing_weights, smoothing_radius, filter_weights, filter_radius, reference_frame, target,
                                  frames_in_flight, out, drift, true);
}

static int intensity_hist_impl(vof_ctx* c, const double* movie, int n_frames, const double* w_host, int radius, const double* edges_host, int bins,
                               int flight, int64_t* counts, int64_t* nonfinite, bool host) {
    if (int rc = FrameChunks::check(c, {movie, edges_host, counts, nonfinite}, n_frames, "n_frames")) return rc;
    if (w_host && (radius < 0 || radius > 4096)) { c->err = "bad blur_radius"; return -1; }
    if (bins < 1 || bins > IH_MAX_BINS) { c->err = "intensity histograms: bins must be 1 .. " + std::to_string(IH_MAX_BINS); return -1; }
    if (!(edges_host[0] < edges_host[bins])) { c->err = "intensity histograms: the edges must increase"; return -1; }
    const size_t fs = frame_stride(c);
    FrameChunks fc(c, "intensity histograms", n_frames, flight, host);
    double *blurred = nullptr, *tmp = nullptr, *w = nullptr, *edges;
    unsigned long long *d_hist, *d_bad;                              // [frame in flight][bins], [frame in flight]
    if (w_host) { fc.sc.per_unit(&blurred, fs); blur_regions(fc.sc, n_frames, &tmp, &w, radius); }
    fc.sc.once(&edges, (size_t)bins + 1);
    fc.sc.per_unit(&d_hist, (size_t)bins);
    fc.sc.per_unit(&d_bad, 1);
    fc.input(movie);
    if (int rc = fc.plan()) return rc;
    if (w_host) if (int rc = h2d_bounced(c, w, w_host, (size_t)(2 * radius + 1) * sizeof(double))) return rc;
    if (int rc = h2d_bounced(c, edges, edges_host, ((size_t)bins + 1) * sizeof(double))) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied out as they are");
    const int blocks = (int)std::min<size_t>(IH_MAX_BLOCKS, (fs + (size_t)IH_PER_THREAD * IH_BLOCK - 1) / ((size_t)IH_PER_THREAD * IH_BLOCK));
    return fc.run([&](int k0, int nf, const double* const* in, void* const*) -> int {
        const double* x = in[0];
        if (w_host) { if (int rc = blur_frames(c, in[0], blurred, nf, radius, tmp, w)) return rc; x = blurred; }
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)nf * bins * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(d_bad, 0, (size_t)nf * sizeof(unsigned long long), c->stream));
        {
            Prof prof(c, VOF_K_PREPROCESS, PP_ST_IH_COUNTS, 8.0 * fs);
            k_ih_counts<<<dim3(blocks, nf), IH_BLOCK, 0, c->stream>>>(x, fs, edges, bins, d_hist, d_bad);
        }
        HIPCHK(hipGetLastError());
        if (int rc = d2h_bounced(c, counts + (size_t)k0 * bins, d_hist, (size_t)nf * bins * sizeof(int64_t))) return rc;
        return d2h_bounced(c, nonfinite + k0, d_bad, (size_t)nf * sizeof(int64_t));
    });
}

int vof_intensity_hist_dev(vof_ctx* c, const double* movie, int n_frames, const double* blur_weights, int blur_radius, const double* edges,
                           int bins, int frames_in_flight, int64_t* counts, int64_t* nonfinite) {
    return intensity_hist_impl(c, movie, n_frames, blur_weights, blur_radius, edges, bins, frames_in_flight, counts, nonfinite, false);
}
int vof_intensity_hist_host(vof_ctx* c, const double* movie, int n_frames, const double* blur_weights, int blur_radius, const double* edges,
                            int bins, int frames_in_flight, int64_t* counts, int64_t* nonfinite) {
    return intensity_hist_impl(c, movie, n_frames, blur_weights, blur_radius, edges, bins, frames_in_flight, counts, nonfinite, true);
}

// ---- the dense part of convert_PIV_result (upsample_PIV_vectors; vof_piv.hpp) --------------------------------
// What the kernels index with comes from the caller: every table is checked on the host before anything is uploaded.
struct PivRequest {
    int n_frames;
    const double *points, *values, *grads, *transforms;
    const int32_t *simplices, *neighbours, *pt_off, *tri_off;
};

static int piv_check(vof_ctx* c, const PivRequest& r, int* max_points, int* max_triangles) {
    if (frame_stride(c) >= (size_t)PIV_NONE) { c->err = "PIV upsampling: frames of 2^31 pixels or more are not served"; return -1; }
    if (r.pt_off[0] != 0 || r.tri_off[0] != 0) { c->err = "PIV upsampling: the offsets must start at 0"; return -1; }
    *max_points = *max_triangles = 0;
    for (int f = 0; f < r.n_frames; ++f) {
        const int np = r.pt_off[f + 1] - r.pt_off[f], nt = r.tri_off[f + 1] - r.tri_off[f];
        if (np < 0 || nt < 0 || (nt > 0 && np < 3)) { c->err = "PIV upsampling: bad offsets in frame " + std::to_string(f); return -1; }
        *max_points = std::max(*max_points, np); *max_triangles = std::max(*max_triangles, nt);
        const double* P = r.points + (size_t)2 * r.pt_off[f];
        for (int k = 0; k < 2 * np; ++k)
            if (!std::isfinite(P[k]) || !std::isfinite(r.values[(size_t)2 * r.pt_off[f] + k]) || !std::isfinite(r.grads[(size_t)4 * r.pt_off[f] + 2 * k]) ||
                !std::isfinite(r.grads[(size_t)4 * r.pt_off[f] + 2 * k + 1])) {
                c->err = "PIV upsampling: a point, a vector or a gradient of frame " + std::to_string(f) + " is not finite"; return -1;
            }
        for (size_t k = (size_t)3 * r.tri_off[f]; k < (size_t)3 * r.tri_off[f + 1]; ++k)
            if (r.simplices[k] < 0 || r.simplices[k] >= np || r.neighbours[k] < -1 || r.neighbours[k] >= nt) {
                c->err = "PIV upsampling: a simplex or a neighbour of frame " + std::to_string(f) + " is outside its tables"; return -1;
            }
        for (size_t k = (size_t)6 * r.tri_off[f]; k < (size_t)6 * r.tri_off[f + 1]; ++k)
            if (!std::isfinite(r.transforms[k])) {
                c->err = "PIV upsampling: frame " + std::to_string(f) + " has a degenerate simplex (its transform is not finite): evaluate it "
                         "on the host and pass it without triangles";
                return -1;
            }
    }
    return 0;
}

static int piv_upsample_impl(vof_ctx* c, const PivRequest& r, int flight, double* v_x, double* v_y, double* speed, int64_t* counts, bool host) {
    if (int rc = FrameChunks::check(c, {r.points, r.values, r.grads, r.transforms, r.simplices, r.neighbours, r.pt_off, r.tri_off, v_x, v_y, speed, counts},
                                    r.n_frames, "n_frames")) return rc;
    int mp = 0, mt = 0;
    if (int rc = piv_check(c, r, &mp, &mt)) return rc;
    const size_t fs = frame_stride(c);
    FrameChunks fc(c, "PIV upsampling", r.n_frames, flight, host);
    // per frame in flight: its tables at the size of the call's largest frame (a chunk's tables are uploaded frame after frame, so
    // they fit whatever the frames), the coefficients and the map; once: the offsets and the counter
    double *d_pts, *d_val, *d_grad, *d_tr, *d_coef;
    int *d_simp, *d_nb, *d_map, *d_ptoff, *d_trioff;
    unsigned long long* d_outside;
    fc.sc.per_unit(&d_pts, (size_t)2 * mp); fc.sc.per_unit(&d_val, (size_t)2 * mp); fc.sc.per_unit(&d_grad, (size_t)4 * mp);
    fc.sc.per_unit(&d_tr, (size_t)6 * mt); fc.sc.per_unit(&d_coef, (size_t)PIV_COEF * mt);
    fc.sc.per_unit(&d_simp, (size_t)3 * mt); fc.sc.per_unit(&d_nb, (size_t)3 * mt);
    fc.sc.per_unit(&d_map, fs);
    fc.sc.once(&d_ptoff, (size_t)r.n_frames + 1); fc.sc.once(&d_trioff, (size_t)r.n_frames + 1);
    fc.sc.once(&d_outside, 1);
    fc.output(v_x, fs * sizeof(double)); fc.output(v_y, fs * sizeof(double)); fc.output(speed, fs * sizeof(double));
    if (int rc = fc.plan()) return rc;
    if (int rc = h2d_bounced(c, d_ptoff, r.pt_off, ((size_t)r.n_frames + 1) * sizeof(int32_t))) return rc;
    if (int rc = h2d_bounced(c, d_trioff, r.tri_off, ((size_t)r.n_frames + 1) * sizeof(int32_t))) return rc;
    HIPCHK(hipMemsetAsync(d_outside, 0, sizeof(unsigned long long), c->stream));
    static_assert(PIV_NONE == 0x7f7f7f7f, "the map is filled bytewise");
    if (int rc = fc.run([&](int k0, int nf, const double* const*, void* const* out) -> int {
            const size_t p0 = r.pt_off[k0], np = (size_t)r.pt_off[k0 + nf] - p0, t0 = r.tri_off[k0], nt = (size_t)r.tri_off[k0 + nf] - t0;
            int most = 0;                                           // triangles of the chunk's largest frame
            for (int f = k0; f < k0 + nf; ++f) most = std::max(most, r.tri_off[f + 1] - r.tri_off[f]);
            if (np) {
                if (int rc = h2d_bounced(c, d_pts, r.points + 2 * p0, 2 * np * sizeof(double))) return rc;
                if (int rc = h2d_bounced(c, d_val, r.values + 2 * p0, 2 * np * sizeof(double))) return rc;
                if (int rc = h2d_bounced(c, d_grad, r.grads + 4 * p0, 4 * np * sizeof(double))) return rc;
            }
            if (nt) {
                if (int rc = h2d_bounced(c, d_tr, r.transforms + 6 * t0, 6 * nt * sizeof(double))) return rc;
                if (int rc = h2d_bounced(c, d_simp, r.simplices + 3 * t0, 3 * nt * sizeof(int32_t))) return rc;
                if (int rc = h2d_bounced(c, d_nb, r.neighbours + 3 * t0, 3 * nt * sizeof(int32_t))) return rc;
            }
            const PivTables tb{d_pts, d_val, d_grad, d_tr, d_simp, d_nb, d_ptoff + k0, d_trioff + k0};
            HIPCHK(hipMemsetAsync(d_map, 0x7f, (size_t)nf * fs * sizeof(int), c->stream));
            if (most) {
                {
                    Prof prof(c, VOF_K_REDUCE, PIV_ST_COEFFS, 8.0 * (PIV_COEF + 20) * (double)nt / nf);
                    k_piv_coeffs<<<dim3((most + PIV_BLOCK - 1) / PIV_BLOCK, nf), PIV_BLOCK, 0, c->stream>>>(tb, d_coef);
                }
                {
                    Prof prof(c, VOF_K_REDUCE, PIV_ST_LOCATE);
                    k_piv_locate<<<dim3((most + PIV_TRI_PER_BLOCK - 1) / PIV_TRI_PER_BLOCK, nf), PIV_BLOCK, 0, c->stream>>>(tb, d_coef, d_map, c->Ni, c->Nj);
                }
            }
            Prof prof(c, VOF_K_REDUCE, PIV_ST_EVAL, 28.0 * fs);
            k_piv_eval<<<dim3((unsigned)((fs + PIV_BLOCK - 1) / PIV_BLOCK), nf), PIV_BLOCK, 0, c->stream>>>(tb, d_coef, d_map, c->Ni, c->Nj, (double*)out[0],
                                                                                                      (double*)out[1], (double*)out[2], d_outside);
            return 0;
        })) return rc;
    unsigned long long outside;
    if (int rc = d2h_bounced(c, &outside, d_outside, sizeof outside)) return rc;
    counts[0] = (int64_t)outside; counts[1] = 0;
    for (int f = 0; f < r.n_frames; ++f) counts[1] += r.tri_off[f + 1] == r.tri_off[f];
    return 0;
}

int vof_piv_upsample_dev(vof_ctx* c, int n_frames, const double* points, const double* values, const double* gradients, const int32_t* simplices,
                         const int32_t* neighbours, const double* transforms, const int32_t* point_offsets, const int32_t* triangle_offsets,
                         int frames_in_flight, double* v_x, double* v_y, double* speed, int64_t* counts) {
    return piv_upsample_impl(c, PivRequest{n_frames, points, values, gradients, transforms, simplices, neighbours, point_offsets, triangle_offsets},
                             frames_in_flight, v_x, v_y, speed, counts, false);
}
int vof_piv_upsample_host(vof_ctx* c, int n_frames, const double* points, const double* values, const double* gradients, const int32_t* simplices,
                          const int32_t* neighbours, const double* transforms, const int32_t* point_offsets, const int32_t* triangle_offsets,
                          int frames_in_flight, double* v_x, double* v_y, double* speed, int64_t* counts) {
    return piv_upsample_impl(c, PivRequest{n_frames, points, values, gradients, transforms, simplices, neighbours, point_offsets, triangle_offsets},
                             frames_in_flight, v_x, v_y, speed, counts, true);
}

// ---- conduct_piv: windowed cross-correlation PIV of every pair of a stack (vof_pivflow.hpp) -----------------
// The passes of a request, checked: what include/vof.h lists, and that every search region stays inside the frame for the largest
// offset the pass before can hand on (its margin).  Nothing is uploaded before this returns 0.
static int piv_flow_passes(vof_ctx* c, int n_passes, const int32_t* w, const int32_t* r, const int32_t* s, PfPass* P) {
    if (n_passes < 1 || n_passes > PF_MAX_PASSES) { c->err = "PIV: n_passes must lie in [1, " + std::to_string(PF_MAX_PASSES) + "]"; return -1; }
    int m = 0;
    for (int p = 0; p < n_passes; ++p) {
        const std::string at = "PIV pass " + std::to_string(p) + ": ";
        if (w[p] < PF_MIN_W || w[p] > PF_MAX_W) { c->err = at + "the window size must lie in [4, 64]"; return -1; }
        if (r[p] < 1 || r[p] > PF_MAX_R) { c->err = at + "the search radius must lie in [1, 16]"; return -1; }
        if (s[p] < 1) { c->err = at + "the step must be >= 1"; return -1; }
        if (p > 0 && w[p] > w[p - 1]) { c->err = at + "window sizes must not increase from pass to pass"; return -1; }
        if (pf_lds_doubles(w[p], r[p]) * sizeof(double) > PF_LDS_LIMIT || pf_items(r[p]) > PF_BLOCK) {
            c->err = at + "the window and its search region do not fit the LDS of a compute unit"; return -1;
        }
        m += r[p];
        const int span = w[p] + 2 * m;
        if (c->Ni < span || c->Nj < span) { c->err = at + "the grid is empty: the frame is smaller than window + 2 * margin = " + std::to_string(span); return -1; }
        P[p] = PfPass{w[p], r[p], s[p], m, (c->Ni - span) / s[p] + 1, (c->Nj - span) / s[p] + 1};
        if (P[p].R > 65535) { c->err = at + "more than 65535 rows of windows do not fit one launch"; return -1; }
        // window (a, b) at m + a s; offsets |o| <= m - r, the margin of the pass before: rows [m + a s + o - r, ... + w + 2 r) of the frame
        const int lo = m - (m - r[p]) - r[p], hi_i = m + (P[p].R - 1) * s[p] + (m - r[p]) + r[p] + w[p], hi_j = m + (P[p].C - 1) * s[p] + (m - r[p]) + r[p] + w[p];
        if (lo < 0 || hi_i > c->Ni || hi_j > c->Nj) { c->err = at + "a search region leaves the frame"; return -1; }
    }
    return 0;
}

// one pass of np pairs; the run length of the hot loop goes with the radius (pf_run).  deform: the vectors the region is resampled by
// (a pass after the first, off NULL), or NULL for the integer path.
static int piv_flow_launch(vof_ctx* c, const PfPass& p, int np, const double* frames, const int* off, double min_correlation, double* u, double* v,
                           double* corr, unsigned long long* counts, const PfDeform* deform = nullptr) {
    const size_t lds = pf_lds_doubles(p.w, p.r) * sizeof(double);
    const int slot = (deform ? 2 : 0) + (pf_run(p.r) == PF_LONG_RUN ? 1 : 0);
    const void* const kernels[4] = {(const void*)k_pivflow_correlate<PF_SHORT_RUN, false>, (const void*)k_pivflow_correlate<PF_LONG_RUN, false>,
                                    (const void*)k_pivflow_correlate<PF_SHORT_RUN, true>, (const void*)k_pivflow_correlate<PF_LONG_RUN, true>};
    if (lds > c->pivflow_lds[slot]) {                               // raised once per context and kernel
        HIPCHK(hipFuncSetAttribute(kernels[slot], hipFuncAttributeMaxDynamicSharedMemorySize, (int)PF_LDS_LIMIT));
        c->pivflow_lds[slot] = PF_LDS_LIMIT;
    }
    const dim3 grid(p.C, p.R, np);
    const PfDeform df = deform ? *deform : PfDeform{};
#define PF_LAUNCH(K, DEFORM) k_pivflow_correlate<K, DEFORM><<<grid, PF_BLOCK, lds, c->stream>>>(p, frames, frame_stride(c), c->Nj, off, min_correlation, u, v, corr, counts, df)
    switch (slot) {
        case 0: PF_LAUNCH(PF_SHORT_RUN, false); break;
        case 1: PF_LAUNCH(PF_LONG_RUN, false); break;
        case 2: PF_LAUNCH(PF_SHORT_RUN, true); break;
        default: PF_LAUNCH(PF_LONG_RUN, true); break;
    }
#undef PF_LAUNCH
    return 0;
}

// the options of vof_piv_flow_ex_*; the plain call is PivFlowOptions{}
struct PivFlowOptions {
    int deformation = 0; double outlier_threshold = NAN, outlier_epsilon = 0.1; int validate_last = 0; int64_t* validation_counts = nullptr;
    bool validating() const { return !std::isnan(outlier_threshold); }
};
static int piv_flow_options(vof_ctx* c, const PivFlowOptions& o) {
    if (o.deformation != 0 && o.deformation != 1) { c->err = "PIV: deformation must be 0 or 1"; return -1; }
    if (o.validate_last != 0 && o.validate_last != 1) { c->err = "PIV: validate_last must be 0 or 1"; return -1; }
    if (o.validating() && !(o.outlier_threshold > 0.0 && std::isfinite(o.outlier_threshold))) { c->err = "PIV: outlier_threshold must be positive and finite, or NaN for none"; return -1; }
    if (!(o.outlier_epsilon >= 0.0 && std::isfinite(o.outlier_epsilon))) { c->err = "PIV: outlier_epsilon must be non-negative and finite"; return -1; }
    if (o.validate_last && !o.validating()) { c->err = "PIV: validate_last needs an outlier_threshold"; return -1; }
    if (o.validating() && !o.validation_counts) { c->err = "PIV: validation_counts is NULL with validation on"; return -1; }
    return 0;
}

static int piv_flow_impl(vof_ctx* c, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes, const int32_t* search_radii,
                         const int32_t* steps, double min_correlation, int flight, double* u, double* v, double* correlation, int64_t* counts, bool host,
                         const PivFlowOptions& opt = PivFlowOptions{}) {
    if (int rc = FrameChunks::check(c, {movie, window_sizes, search_radii, steps, u, v, correlation, counts}, n_pairs, "n_pairs")) return rc;
    if (int rc = piv_flow_options(c, opt)) return rc;
    PfPass P[PF_MAX_PASSES];
    if (int rc = piv_flow_passes(c, n_passes, window_sizes, search_radii, steps, P)) return rc;
    const int last = n_passes - 1;
    const bool validating = opt.validating(), deform = opt.deformation != 0;
    FrameChunks fc(c, "PIV", n_pairs, flight, host);
    fc.input(movie, true);
    // per pair in flight: the vectors of every pass but the last (and of the last where they are validated), the validated vectors at
    // the size of the largest validated grid, and - on the integer path - the offsets of a pass at the size of the largest grid
    double *d_u[PF_MAX_PASSES] = {}, *d_v[PF_MAX_PASSES] = {}, *d_val_u = nullptr, *d_val_v = nullptr;
    int* d_off = nullptr;
    unsigned long long* d_counts = nullptr;                         // 3 per pass, then the 2 of the validation per pass
    const bool validated_last = validating && opt.validate_last;
    size_t most = 0, most_validated = 0;
    for (int p = 0; p < last + (validated_last ? 1 : 0); ++p) {
        fc.sc.per_unit(&d_u[p], (size_t)P[p].R * P[p].C); fc.sc.per_unit(&d_v[p], (size_t)P[p].R * P[p].C);
        if (p < last) { most = std::max(most, (size_t)P[p + 1].R * P[p + 1].C); most_validated = std::max(most_validated, (size_t)P[p].R * P[p].C); }
    }
    if (last > 0 && !deform) fc.sc.per_unit(&d_off, 2 * most);
    if (last > 0 && validating) { fc.sc.per_unit(&d_val_u, most_validated); fc.sc.per_unit(&d_val_v, most_validated); }
    fc.sc.once(&d_counts, (size_t)5 * n_passes);
    const size_t ob = (size_t)P[last].R * P[last].C * sizeof(double);
    fc.output(u, ob); fc.output(v, ob); fc.output(correlation, ob);
    if (int rc = fc.plan()) return rc;
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)5 * n_passes * sizeof(unsigned long long), c->stream));
    if (int rc = fc.run([&](int, int np, const double* const* in, void* const* out) -> int {
            const double *from_u = nullptr, *from_v = nullptr;       // the vectors the next pass starts from
            for (int p = 0; p < n_passes; ++p) {
                PfDeform df{};
                if (p > 0 && deform) df = PfDeform{P[p - 1], from_u, from_v, c->Ni};
                else if (p > 0) {
                    Prof prof(c, VOF_K_REDUCE, PF_ST_OFFSETS);
                    k_pivflow_offsets<<<dim3((P[p].R * P[p].C + PF_BLOCK - 1) / PF_BLOCK, np), PF_BLOCK, 0, c->stream>>>(P[p], P[p - 1], from_u, from_v, d_off);
                }
                const bool raw_out = p == last && !validated_last;  // the last pass writes the outputs, unless the median test does
                double* pu = raw_out ? (double*)out[0] : d_u[p];
                double* pv = raw_out ? (double*)out[1] : d_v[p];
                double* pc = p == last ? (double*)out[2] : nullptr;
                {
                    const double S = P[p].w + 2.0 * P[p].r;
                    Prof prof(c, VOF_K_REDUCE, PF_ST_PASS0 + p, 8.0 * (P[p].w * (double)P[p].w + S * S) * P[p].R * P[p].C);
                    const int rc = piv_flow_launch(c, P[p], np, in[0], p && !deform ? d_off : nullptr, min_correlation, pu, pv, pc, d_counts + 3 * p,
                                                   p && deform ? &df : nullptr);
                    if (rc) return rc;
                }
                from_u = pu; from_v = pv;
                if (validating && (p < last || validated_last)) {   // Jacobi: from the raw vectors into a second field
                    double* vu = p == last ? (double*)out[0] : d_val_u;
                    double* vv = p == last ? (double*)out[1] : d_val_v;
                    Prof prof(c, VOF_K_REDUCE, PF_ST_OFFSETS);
                    k_pivflow_validate<<<dim3((P[p].R * P[p].C + PF_BLOCK - 1) / PF_BLOCK, np), PF_BLOCK, 0, c->stream>>>(
                        P[p].R, P[p].C, pu, pv, opt.outlier_threshold, opt.outlier_epsilon, vu, vv, d_counts + 3 * n_passes + 2 * p);
                    from_u = vu; from_v = vv;
                }
            }
            return 0;
        })) return rc;
    unsigned long long got[5 * PF_MAX_PASSES];
    if (int rc = d2h_bounced(c, got, d_counts, (size_t)5 * n_passes * sizeof(unsigned long long))) return rc;
    for (int k = 0; k < 3 * n_passes; ++k) counts[k] = (int64_t)got[k];
    if (validating) for (int k = 0; k < 2 * n_passes; ++k) opt.validation_counts[k] = (int64_t)got[3 * n_passes + k];
    return 0;
}

int vof_piv_flow_dev(vof_ctx* c, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes, const int32_t* search_radii,
                     const int32_t* steps, double min_correlation, int frames_in_flight, double* u, double* v, double* correlation, int64_t* counts) {
    return piv_flow_impl(c, movie, n_pairs, n_passes, window_sizes, search_radii, steps, min_correlation, frames_in_flight, u, v, correlation, counts, false);
}
int vof_piv_flow_host(vof_ctx* c, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes, const int32_t* search_radii,
                      const int32_t* steps, double min_correlation, int frames_in_flight, double* u, double* v, double* correlation, int64_t* counts) {
    return piv_flow_impl(c, movie, n_pairs, n_passes, window_sizes, search_radii, steps, min_correlation, frames_in_flight, u, v, correlation, counts, true);
}
int vof_piv_flow_ex_dev(vof_ctx* c, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes, const int32_t* search_radii,
                        const int32_t* steps, double min_correlation, int frames_in_flight, double* u, double* v, double* correlation, int64_t* counts,
                        int deformation, double outlier_threshold, double outlier_epsilon, int validate_last, int64_t* validation_counts) {
    return piv_flow_impl(c, movie, n_pairs, n_passes, window_sizes, search_radii, steps, min_correlation, frames_in_flight, u, v, correlation, counts, false,
                         PivFlowOptions{deformation, outlier_threshold, outlier_epsilon, validate_last, validation_counts});
}
int vof_piv_flow_ex_host(vof_ctx* c, const double* movie, int n_pairs, int n_passes, const int32_t* window_sizes, const int32_t* search_radii,
                         const int32_t* steps, double min_correlation, int frames_in_flight, double* u, double* v, double* correlation, int64_t* counts,
                         int deformation, double outlier_threshold, double outlier_epsilon, int validate_last, int64_t* validation_counts) {
    return piv_flow_impl(c, movie, n_pairs, n_passes, window_sizes, search_radii, steps, min_correlation, frames_in_flight, u, v, correlation, counts, true,
                         PivFlowOptions{deformation, outlier_threshold, outlier_epsilon, validate_last, validation_counts});
}

// the six stacks of two results as inputs of a frame-chunk walk, and those of one chunk as the kernels take them
struct FlowStacks { const double *vxa, *vya, *spa, *vxb, *vyb, *spb; };
static int flow_stacks_check(vof_ctx* c, const FlowStacks& s, int n_pairs, double speed_min, double angle_min) {
    if (int rc = FrameChunks::check(c, {s.vxa, s.vya, s.spa, s.vxb, s.vyb, s.spb}, n_pairs, "n_pairs")) return rc;
    if (std::isnan(speed_min) || std::isnan(angle_min)) { c->err = "flow comparison: a threshold is NaN"; return -1; }
    return 0;
}
static void flow_stacks_inputs(FrameChunks& fc, const FlowStacks& s) {
    for (const double* p : {s.vxa, s.vya, s.spa, s.vxb, s.vyb, s.spb}) fc.input(p);
}
static FlowPlanes flow_planes(const double* const* in, size_t fs) { return FlowPlanes{in[0], in[1], in[2], in[3], in[4], in[5], fs}; }

static int flow_extremes_impl(vof_ctx* c, const FlowStacks& s, int n_pairs, double speed_min, double angle_min, int quirks, int flight,
                              double* extremes, bool host) {
    if (int rc = flow_stacks_check(c, s, n_pairs, speed_min, angle_min)) return rc;
    if (!extremes) { c->err = "NULL pointer"; return -1; }
    const size_t fs = frame_stride(c);
    const int blk = fc_blocks(fs);
    FrameChunks fc(c, "flow extremes", n_pairs, flight, host);
    FcExtremes *part, *acc;
    fc.sc.per_unit(&part, (size_t)blk);
    fc.sc.once(&acc, 1);
    flow_stacks_inputs(fc, s);
    if (int rc = fc.plan()) return rc;
    const FcExtremes none{INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
    if (int rc = h2d_bounced(c, acc, &none, sizeof none)) return rc;
    if (int rc = fc.run([&](int, int nf, const double* const* in, void* const*) -> int {
            Prof prof(c, VOF_K_REDUCE, FC_ST_EXTREMES, 48.0 * fs);
            k_fc_extremes<<<dim3(blk, nf), FC_BLOCK, 0, c->stream>>>(flow_planes(in, fs), speed_min, angle_min, quirks ? 0 : 1, part);
            k_fc_extremes_fold<<<1, 64, 0, c->stream>>>(part, blk * nf, acc);
            return 0;
        })) return rc;
    static_assert(sizeof(FcExtremes) == 6 * sizeof(double), "extremes: six doubles");
    return d2h_bounced(c, extremes, acc, sizeof(FcExtremes));
}

#define VOF_FLOW_STACKS_ARGS const double *v_x_a, const double *v_y_a, const double *speed_a, const double *v_x_b, const double *v_y_b, const double *speed_b
#define VOF_FLOW_STACKS FlowStacks{v_x_a, v_y_a, speed_a, v_x_b, v_y_b, speed_b}

int vof_flow_extremes_dev(vof_ctx* c, VOF_FLOW_STACKS_ARGS, int n_pairs, double speed_threshold, double angle_threshold, int reference_quirks,
                          int frames_in_flight, double* extremes) {
    return flow_extremes_impl(c, VOF_FLOW_STACKS, n_pairs, speed_threshold, angle_threshold, reference_quirks, frames_in_flight, extremes, false);
}
int vof_flow_extremes_host(vof_ctx* c, VOF_FLOW_STACKS_ARGS, int n_pairs, double speed_threshold, double angle_threshold, int reference_quirks,
                           int frames_in_flight, double* extremes) {
    return flow_extremes_impl(c, VOF_FLOW_STACKS, n_pairs, speed_threshold, angle_threshold, reference_quirks, frames_in_flight, extremes, true);
}

struct FlowCompareReq {
    FlowStacks s; int n_pairs; double speed_min, angle_min; int quirks;
    const double* edges[3]; int bins[3];                      // speed of a, speed of b, theta
    int clamp_theta, flight;
    int64_t *jhist, *thist, *counts;
    bool host;
};

static int flow_compare_impl(vof_ctx* c, const FlowCompareReq& r) {
    if (int rc = flow_stacks_check(c, r.s, r.n_pairs, r.speed_min, r.angle_min)) return rc;
    if (!r.edges[0] || !r.edges[1] || !r.edges[2] || !r.jhist || !r.thist || !r.counts) { c->err = "NULL pointer"; return -1; }
    for (int e = 0; e < 3; ++e) {
        const int most = e < 2 ? CP_MAX_SPEED_BINS : CP_MAX_THETA_BINS;
        if (r.bins[e] < 1 || r.bins[e] > most) {
            c->err = std::string(e < 2 ? "joint_speed_bins must be 1 .. " : "angle_bins must be 1 .. ") + std::to_string(most) + (e < 2 ? " per axis" : "");
            return -1;
        }
        bool rising = r.edges[e][r.bins[e]] > r.edges[e][0];
        for (int b = 0; b < r.bins[e]; ++b) rising = rising && r.edges[e][b + 1] >= r.edges[e][b];
        if (!rising) { c->err = e < 2 ? "joint_speed_edges must increase" : "angle_edges must increase"; return -1; }
    }
    const size_t fs = frame_stride(c);
    const int blk = fc_blocks(fs);
    const size_t nj = (size_t)r.bins[0] * r.bins[1];
    FrameChunks fc(c, "flow comparison", r.n_pairs, r.flight, r.host);
    double* d_edges[3];
    unsigned long long *d_jhist, *d_thist, *d_counters;
    for (int e = 0; e < 3; ++e) fc.sc.once(&d_edges[e], (size_t)r.bins[e] + 1);
    fc.sc.once(&d_jhist, nj);
    fc.sc.once(&d_thist, (size_t)r.bins[2]);
    fc.sc.once(&d_counters, (size_t)FC_COUNTERS);
    flow_stacks_inputs(fc, r.s);
    if (int rc = fc.plan()) return rc;
    for (int e = 0; e < 3; ++e)
        if (int rc = h2d_bounced(c, d_edges[e], r.edges[e], ((size_t)r.bins[e] + 1) * sizeof(double))) return rc;
    HIPCHK(hipMemsetAsync(d_jhist, 0, nj * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(d_thist, 0, (size_t)r.bins[2] * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(d_counters, 0, FC_COUNTERS * sizeof(unsigned long long), c->stream));
    if (int rc = fc.run([&](int, int nf, const double* const* in, void* const*) -> int {
            FcHistArgs a{};
            a.p = flow_planes(in, fs);
            a.speed_min = r.speed_min; a.angle_min = r.angle_min; a.clip = r.quirks ? 0 : 1; a.clamp_theta = r.clamp_theta ? 1 : 0;
            a.ea = d_edges[0]; a.ba = r.bins[0]; a.eb = d_edges[1]; a.bb = r.bins[1];
            a.tedges = d_edges[2]; a.tbins = r.bins[2];
            a.jhist = d_jhist; a.thist = d_thist; a.counters = d_counters;
            Prof prof(c, VOF_K_REDUCE, FC_ST_HISTOGRAMS, 48.0 * fs);
            k_fc_histograms<<<dim3(blk, nf), FC_BLOCK, 0, c->stream>>>(a);
            return 0;
        })) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counters are copied as they are");
    if (int rc = d2h_bounced(c, r.jhist, d_jhist, nj * sizeof(int64_t))) return rc;
    if (int rc = d2h_bounced(c, r.thist, d_thist, (size_t)r.bins[2] * sizeof(int64_t))) return rc;
    return d2h_bounced(c, r.counts, d_counters, FC_COUNTERS * sizeof(int64_t));
}

#define VOF_FLOW_COMPARE_ARGS                                                                                                          \
    vof_ctx *c, VOF_FLOW_STACKS_ARGS, int n_pairs, double speed_threshold, double angle_threshold, int reference_quirks,               \
        const double *joint_speed_edges_a, int joint_speed_bins_a, const double *joint_speed_edges_b, int joint_speed_bins_b,          \
        const double *angle_edges, int angle_bins, int clamp_angle, int frames_in_flight, int64_t *joint_speed_histogram,              \
        int64_t *angle_histogram, int64_t *counts
#define VOF_FLOW_COMPARE_REQ(host)                                                                                                     \
    FlowCompareReq{VOF_FLOW_STACKS, n_pairs, speed_threshold, angle_threshold, reference_quirks,                                       \
                   {joint_speed_edges_a, joint_speed_edges_b, angle_edges}, {joint_speed_bins_a, joint_speed_bins_b, angle_bins},     \
                   clamp_angle, frames_in_flight, joint_speed_histogram, angle_histogram, counts, host}

int vof_flow_compare_dev(VOF_FLOW_COMPARE_ARGS) { return flow_compare_impl(c, VOF_FLOW_COMPARE_REQ(false)); }
int vof_flow_compare_host(VOF_FLOW_COMPARE_ARGS) { return flow_compare_impl(c, VOF_FLOW_COMPARE_REQ(true)); }

// ---- Liu-Shen Jacobi flow (liu_shen_optical_flow_jit, OF.py:426-673) ----------------------------------------------
constexpr int LS_HOST_CHUNK = 8;          // pairs per chunk of vof_liu_shen_host

static int liu_shen_check(vof_ctx* c, const double* movie, int n_frames, double delta_x, double delta_t, const double* ix, const double* iy,
                          const double* ir, int initial_kind, int max_iterations, const double* v_x, const double* v_y,
                          const double* speed, const double* remodelling) {
    if (!movie || !v_x || !v_y || !speed || !remodelling || !ix || !iy || !ir) { c->err = "NULL array pointer"; return -1; }
    if (n_frames < 2) { c->err = "need at least two frames"; return -1; }
    if (initial_kind < 0 || initial_kind > 2) { c->err = "initial_kind must be 0 (scalar), 1 (plane) or 2 (stack)"; return -1; }
    if (max_iterations < 1) { c->err = "max_iterations must be >= 1"; return -1; }
    if (c->Ni < 3 || c->Nj < 3) { c->err = "the Liu-Shen flow needs image sides >= 3"; return -1; }
    if (delta_x == 0.0 || delta_t == 0.0) { c->err = "delta_x and delta_t must not be 0"; return -1; }
    return 0;
}

// iterations per launch: VOF_LIUSHEN_FUSE, read at every call
static int liu_shen_depth(vof_ctx* c, int* depth) {
    *depth = LS_KDEF;
    if (const char* e = getenv("VOF_LIUSHEN_FUSE")) {
        *depth = atoi(e);
        if (*depth < 1 || *depth > LS_KMAX) { c->err = "VOF_LIUSHEN_FUSE must be 1 .. 8"; return -1; }
    }
    return 0;
}

// P pairs (at most 4096: a chunk of the walk) of a device-resident movie into device-resident outputs, enqueued on the context's
// stream.  The iterates ping-pong between (v_x, v_y) and (speed, remodelling); ix / iy / ir are device arrays of initial_kind 1 / 2
// (ix, iy may be any of the four outputs), sx / sy / sr the scalars of kind 0.  write_remodelling false leaves remodelling as scratch.
static int liu_shen_pairs(vof_ctx* c, const double* movie, int P, double delta_x, double delta_t, double alpha, const double* ix,
                          const double* iy, const double* ir, double sx, double sy, double sr, int kind, int iterations, int depth,
                          double* v_x, double* v_y, double* speed, double* remodelling, bool write_remodelling) {
    const size_t fs = frame_stride(c);
    if (depth > 1 && !c->ls_lds_set) {
        HIPCHK(hipFuncSetAttribute((const void*)k_ls_fused, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ls_fused_lds(LS_KMAX)));
        c->ls_lds_set = true;
    }
    const size_t n = (size_t)P * fs;
    const unsigned nb = (unsigned)((n + 255) / 256);
    double* buf[2][2] = {{v_x, v_y}, {speed, remodelling}};
    c->cur_units = P;
    Prof prof(c, VOF_K_RHS, 0);
    k_ls_init<<<nb, 256, 0, c->stream>>>(buf[0][0], buf[0][1], kind ? ix : nullptr, kind ? iy : nullptr, sx, sy, kind, fs, n, delta_t, delta_x);
    LsArgs a{};
    a.movie = movie; a.fs = fs; a.Ni = c->Ni; a.Nj = c->Nj; a.alpha = alpha;
    int cur = 0;
    for (int done = 0; done < iterations;) {
        const int k = std::min(depth, iterations - done);
        a.k = k;
        a.sx = buf[cur][0]; a.sy = buf[cur][1]; a.dx = buf[cur ^ 1][0]; a.dy = buf[cur ^ 1][1];
        if (depth == 1) {
            k_ls_step<<<grid2d(c->Ni, c->Nj, P), blk2d, 0, c->stream>>>(a);
        } else {
            const dim3 g((c->Nj + LS_TJ - 1) / LS_TJ, (c->Ni + LS_TI - 1) / LS_TI, P);
            k_ls_fused<<<g, LS_THREADS, ls_fused_lds(k), c->stream>>>(a);
        }
        done += k;
        cur ^= 1;
    }
    k_ls_finish<<<nb, 256, 0, c->stream>>>(buf[cur][0], buf[cur][1], buf[0][0], buf[0][1], buf[1][0], write_remodelling ? buf[1][1] : nullptr,
                                           kind ? ir : nullptr, sr, kind, fs, n, delta_x / delta_t);
    HIPCHK(hipGetLastError());
    return 0;
}

// The pairs in chunks: all of them for device-resident arrays, LS_HOST_CHUNK staged at a time for host arrays.  _host keeps the
// fourth iterate buffer in the arena and never uploads initial_remodelling: remodelling is filled on the host.
static int liu_shen_impl(vof_ctx* c, const double* movie, int n_frames, double delta_x, double delta_t, double alpha,
                         const double* initial_v_x, const double* initial_v_y, const double* initial_remodelling, int initial_kind,
                         int max_iterations, double* v_x, double* v_y, double* speed, double* remodelling, bool host) {
    if (!c) return -1;
    if (int rc = liu_shen_check(c, movie, n_frames, delta_x, delta_t, initial_v_x, initial_v_y, initial_remodelling, initial_kind,
                                max_iterations, v_x, v_y, speed, remodelling)) return rc;
    if (!host && initial_kind && (initial_remodelling == remodelling || initial_remodelling == speed || initial_remodelling == v_x ||
                                  initial_remodelling == v_y)) { c->err = "initial_remodelling must not be an output array"; return -1; }
    int depth;
    if (int rc = liu_shen_depth(c, &depth)) return rc;
    const size_t fs = frame_stride(c), fb = fs * sizeof(double);
    const int P = n_frames - 1;
    const bool s = initial_kind == 0;
    FrameChunks fc(c, "Liu-Shen flow", P, host ? LS_HOST_CHUNK : P, host);
    double *fourth = nullptr, *plane_x = nullptr, *plane_y = nullptr;          // _host: the fourth iterate buffer, the planes of kind 1
    fc.input(movie, true);
    if (initial_kind == 2) { fc.input(initial_v_x); fc.input(initial_v_y); if (!host) fc.input(initial_remodelling); }
    if (initial_kind == 1 && host) { fc.sc.once(&plane_x, fs); fc.sc.once(&plane_y, fs); }
    if (host) fc.sc.per_unit(&fourth, fs);
    for (double* o : {v_x, v_y, speed}) fc.output(o, fb);
    if (int rc = fc.plan()) return rc;
    if (plane_x) if (int rc = h2d_bounced(c, plane_x, initial_v_x, fb)) return rc;
    if (plane_y) if (int rc = h2d_bounced(c, plane_y, initial_v_y, fb)) return rc;
    if (int rc = fc.run([&](int k0, int np, const double* const* in, void* const* out) -> int {
            const bool stack = initial_kind == 2;
            return liu_shen_pairs(c, in[0], np, delta_x, delta_t, alpha, stack ? in[1] : host ? plane_x : initial_v_x,
                                  stack ? in[2] : host ? plane_y : initial_v_y, stack ? in[3] : host ? nullptr : initial_remodelling,
                                  s ? *initial_v_x : 0.0, s ? *initial_v_y : 0.0, s && !host ? *initial_remodelling : 0.0, initial_kind,
                                  max_iterations, depth, (double*)out[0], (double*)out[1], (double*)out[2],
                                  host ? fourth : remodelling + (size_t)k0 * fs, !host);
        })) return rc;
    // OF.py:507, 668: the initial remodelling comes back untouched
    for (int k = 0; host && k < P; ++k) {
        double* r = remodelling + (size_t)k * fs;
        const double* ir = initial_remodelling + (initial_kind == 2 ? (size_t)k * fs : 0);
        if (initial_kind == 0) std::fill(r, r + fs, *initial_remodelling);
        else if (ir != r) memcpy(r, ir, fb);
    }
    return 0;
}

#define VOF_LIU_SHEN_ARGS                                                                                                             \
    vof_ctx *c, const double *movie, int n_frames, double delta_x, double delta_t, double alpha, const double *initial_v_x,           \
        const double *initial_v_y, const double *initial_remodelling, int initial_kind, int max_iterations, double *v_x, double *v_y, \
        double *speed, double *remodelling
#define VOF_LIU_SHEN_CALL(host)                                                                                                       \
    liu_shen_impl(c, movie, n_frames, delta_x, delta_t, alpha, initial_v_x, initial_v_y, initial_remodelling, initial_kind,           \
                  max_iterations, v_x, v_y, speed, remodelling, host)

int vof_liu_shen_dev(VOF_LIU_SHEN_ARGS) { return VOF_LIU_SHEN_CALL(false); }
int vof_liu_shen_host(VOF_LIU_SHEN_ARGS) { return VOF_LIU_SHEN_CALL(true); }

}  // extern "C"
