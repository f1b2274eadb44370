// vof_frames.hip - the frame-chunk calls of libvof.so: FrameChunks and every call that walks it - adaptive threshold, CLAHE,
// resize, Farnebaeck's flow, the result filter and comparison, intensity correction and histograms, PIV upsampling, conduct_piv
// and the Liu-Shen flow.  Context and arena are vof_host.hpp's; the blur is vof_pairs.hip's (blur_regions, blur_frames).
#include "vof_preprocess.hpp"
#include "vof_resize.hpp"
#include "vof_farneback.hpp"
#include "vof_flowcompare.hpp"
#include "vof_intensity.hpp"
#include "vof_piv.hpp"
#include "vof_pivflow.hpp"
#include "vof_liushen.hpp"
#include "vof_host.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

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

}  // namespace

extern "C" {

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
