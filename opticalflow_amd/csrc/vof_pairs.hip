// vof_pairs.hip - the pair calls of libvof.so on the sweep scaffold: the blur, the box least-squares flow, vary_boxsize,
// vary_blursize and compare_channel_flows, with everything only they use.  Context, arena and the functions that cross into the
// solver's source are vof_host.hpp's.
#include "vof_boxflow.hpp"
#include "vof_boxsweep.hpp"
#include "vof_blursweep.hpp"
#include "vof_compare.hpp"
#include "vof_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

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
    double* first = m.d_mom + ((size_t)(2 * field) * m.n_entries * m.P + (size_t)b * m.P + k0) * 3;
    double* second = first + m.n_mom;
    Prof prof(c, VOF_K_REDUCE, 0, 16.0 * fs);
    pair_sums_enqueue(c, x, fs, m.mom_blk, np, m.d_part, first, second);
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

// workspace of the blur of up to `frames` frames per blur_frames call, declared into the caller's arena: one chunk of
// row-filtered frames, and room for the taps of `radius` where the caller does not bring its own (w null)
void vof::host::blur_regions(Scratch& sc, int frames, double** tmp, double** w, int radius) {
    sc.once(tmp, (size_t)std::min(frames, BLUR_CHUNK) * frame_stride(sc.c));
    if (w) sc.once(w, (size_t)2 * radius + 1);
}

// n_frames device-resident frames with the taps already on the device at w and the row-filtered chunk at tmp (blur_regions),
// enqueued on the context's stream (out may alias in).  Radii BL_RMIN .. BL_RMAX take the LDS-tiled kernels, same bits as k_blur1d.
int vof::host::blur_frames(vof_ctx* c, const double* in, double* out, int n_frames, int radius, double* tmp, const double* w) {
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

extern "C" {

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

}  // extern "C"
