// vof_host.hpp - internal to libvof.so, never installed: the host-side state and helpers at least two of its sources use
// (vof.hip: the solver; vof_pairs.hip: the pair calls on the sweep scaffold; vof_frames.hip: the calls that walk FrameChunks),
// and the few functions that cross from one source into another.  Everything here but vof_ctx, the C ABI's name, is in vof::host,
// which is hidden: nothing of it reaches the dynamic symbol table.
#pragma once
#include "vof_shared.hpp"
#include "../../include/vof.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace vof {
namespace host __attribute__((visibility("hidden"))) {

constexpr int MAX_PROF_RECS = 32768;
constexpr int MAX_LANES = 3;        // concurrent pair groups of one device solve (solve_range_dev, VOF_LANES)
constexpr int MAX_LANE_GROUPS = 2;  // groups of pairs a lane runs one after the other in the two-phase solve (VOF_LANE_GROUPS)

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

}  // namespace host
}  // namespace vof

using namespace vof;
using namespace vof::host;

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
    struct Alloc { void* raw; char* user; size_t bytes; const char* name; const char* file; int line; };
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

namespace vof {
namespace host __attribute__((visibility("hidden"))) {

// ---- defined in vof.hip
void dbg_sync_check(vof_ctx* c, const char* what, int level);   // VOF_DEBUG_SYNC: wait for the scope that has just ended
int d2h_bounced(vof_ctx* c, void* host, const void* dev, size_t bytes);
int h2d_bounced(vof_ctx* c, void* dev, const void* host, size_t bytes);
int dev_free(vof_ctx* c, void* user);
int ensure_staging(vof_ctx* c, bool double_buffer);            // st_movie / st_out: the solver's, and vof_box_flow_host's chunks
// the two-pass sums of np pairs of fs doubles at x, enqueued on the context's stream: first[pair][3], then second[pair][3] about
// the pair's own mean; part holds 3 * nblk doubles per pair (k_bs_moments, k_sum3: every block reduction is the solver's)
void pair_sums_enqueue(vof_ctx* c, const double* x, size_t fs, int nblk, int np, double* part, double* first, double* second);

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

constexpr size_t DBG_GUARD = 4096;       // bytes of guard pattern on either side of a buffer (VOF_DEBUG_CANARY=1)
constexpr int DBG_GUARD_BYTE = 0xC5;

template <typename T>
int dev_alloc_named(vof_ctx* c, T** p, size_t n, const char* name, const char* file, int line) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(n * sizeof(T), 256);
    if (c->dbg_canary) {
        HIPCHK(hipMalloc(&q, bytes + 2 * DBG_GUARD));
        HIPCHK(hipMemset(q, DBG_GUARD_BYTE, DBG_GUARD));
        HIPCHK(hipMemset((char*)q + DBG_GUARD + bytes, DBG_GUARD_BYTE, DBG_GUARD));
        c->allocs.push_back({q, (char*)q + DBG_GUARD, bytes, name, file, line});
        *p = (T*)((char*)q + DBG_GUARD);
    } else {
        HIPCHK(hipMalloc(&q, bytes));
        c->allocs.push_back({q, (char*)q, bytes, name, file, line});
        *p = (T*)q;
    }
    c->bytes += bytes;
    if (c->dbg_poison) HIPCHK(hipMemset(*p, 0xFF, bytes));
    if (c->dbg_alloc_log)
        fprintf(stderr, "vof alloc ctx=%p %s (%s:%d) base=%p end=%p bytes=%zu\n", (void*)c, name, file, line, (void*)*p, (void*)((char*)*p + bytes), bytes);
    return 0;
}
#define dev_alloc(c, p, n) dev_alloc_named(c, p, n, #p, __FILE__, __LINE__)

inline dim3 grid2d(int ni, int nj, int z) { return dim3((nj + BX - 1) / BX, (ni + BY - 1) / BY, z); }
const dim3 blk2d(BX, BY, 1);

inline size_t frame_stride(const vof_ctx* c) { return (size_t)c->Ni * c->Nj; }

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

// ---- defined in vof_pairs.hip, which owns the blur kernels: the workspace of a blur declared into the caller's arena, and the
// blur of device-resident frames enqueued on the context's stream
constexpr int BLUR_CHUNK = 16;             // frames a blur_frames call filters per launch at most
void blur_regions(Scratch& sc, int frames, double** tmp, double** w = nullptr, int radius = 0);
int blur_frames(vof_ctx* c, const double* in, double* out, int n_frames, int radius, double* tmp, const double* w);

}  // namespace host
}  // namespace vof
