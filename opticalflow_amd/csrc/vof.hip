// vof.hip - the solver's source of libvof.so: context, workspace, multigrid hierarchy, BiCGStab driver and their part of the C ABI
// (the pair calls: vof_pairs.hip; the frame-chunk calls: vof_frames.hip; what the three share: vof_host.hpp).
//
// Replaces the per-pair body of source/optical_flow.py::variational_optical_flow (OF.py:791-1186:
// scipy.sparse assembly + PETSc KSP bcgs / composite PC) with a batched, matrix-free solve on one
// MI355X: right-preconditioned BiCGStab (the reference's KSP type, OF.py:1081) whose preconditioner is
// one geometric-multigrid V-cycle with a 4-colour 3x3-block Gauss-Seidel smoother and Galerkin coarse
// operators; stopping rule ||b - A x|| <= rtol ||b|| (OF.py:1120,1126).  All frame pairs of a batch
// advance together; per-pair scalars stay on the device.
#include "vof_device.hpp"
#include "vof_sweepst.hpp"
#include "vof_sweep0r.hpp"
#include "vof_sweep0p.hpp"
#include "vof_stream0.hpp"
#include "vof_direct.hpp"
#include "vof_host.hpp"

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
constexpr int AUTO_F64_AFTER = 8;   // vcycle_precision == 2: switch the V-cycle vectors to float64 after this many iterations

}  // namespace

static std::string g_create_error;

// ---- what the other sources reach through vof_host.hpp
namespace vof {
namespace host {

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

}  // namespace host
}  // namespace vof

namespace {

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
            snprintf(line, sizeof line, "buffer %s (%s:%d, %zu bytes at %p): written %s%ld bytes %s; ", a.name, a.file, a.line, a.bytes, (void*)a.user,
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

inline dim3 grid2d_colour(int ni, int nj, int colour, int z) {
    int cp = colour >> 1, cq = colour & 1;
    int mi = (ni - cp + 1) / 2, mj = (nj - cq + 1) / 2;
    return dim3(std::max(1, (mj + BX - 1) / BX), std::max(1, (mi + BY - 1) / BY), z);
}


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
    // (float32 / float64 stencils; a correction `ecoarse` was added by k_prolong_add before the sweep)
    CDISPATCH(c, l, { k_sweep<CT, VT><<<g, GeoB::THREADS, lds, c->stream>>>((const CW*)lv.C, lv.ni, lv.nj, TI, po, nx, ny, nslots, x_in, x_out, b, active); });
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

}  // extern "C"

// Device staging of the host API: frames of one batch (+1) and TWO sets of output buffers, so that the device-to-host
// copies of batch k (copy stream) overlap the solve of batch k+1 (main stream).  st_* serve vof_solve_stack_host,
// vof_vary_regularisation_host, vof_debug_setup and - its chunks are the context's pairs - vof_box_flow_host; every other call
// stages through its arena.
int vof::host::ensure_staging(vof_ctx* c, bool double_buffer) {
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
// the block reductions are this source's; the moments of the pair calls (vof_pairs.hip, pair_moments_enqueue) run through here
void vof::host::pair_sums_enqueue(vof_ctx* c, const double* x, size_t fs, int nblk, int np, double* part, double* first, double* second) {
    const dim3 gm(nblk, np);
    k_bs_moments<<<gm, RBLK, 0, c->stream>>>(x, fs, nullptr, part);
    k_sum3<<<np, 64, 0, c->stream>>>(part, nblk, first);
    k_bs_moments<<<gm, RBLK, 0, c->stream>>>(x, fs, first, part);
    k_sum3<<<np, 64, 0, c->stream>>>(part, nblk, second);
}

extern "C" {

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

}  // extern "C"
