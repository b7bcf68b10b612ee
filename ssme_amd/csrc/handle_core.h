// handle_core.h -- host state and plumbing that the two filter handles of pf_api.hip share (the bootstrap handle ssme_pf_s and
// the Liu-West handle ssme_lw_s both derive from HandleCore): tile layout, stream and events, device buffers owned by the
// handle, the dynamic-LDS grants of the kernels (grant_lds), error reporting, the launches and shard bookkeeping that both filters
// repeat, and the entry points that both C ABIs offer under their own names.  The forecast's buffers (Forecast) and what the two
// *_sim_future_obs do around their own kernels are here too: forecast_prepare, forecast_plan, forecast_finish, forecast_elapsed.
#pragma once
#include "../../include/ssme_pf.h"
#include "pf_kernels.h"

#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace ssme {

static int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
static int ceil_log2(int n) { int k = 0; while ((1ll << k) < n) ++k; return k; }

constexpr int kStepGammaChunk = 64;     // step APIs: Gamma-table rows drawn at a time

struct Layout {
    int N, R, B, Npad, Bs, Bpow2, rshift;
    int tile;                      // particles per tile: 2048, 1024 or 512 (cfg.tile_particles or default_tile); sharded and Liu-West handles: 2048
    int split_l2;                  // level-2 by the split kernels (filters of more than kSplitLevel2Above tiles, or forced by set_debug)
    size_t lds_bytes, lds_bytes_big, lds_bytes_plan;
    int shard_rank, shard_world;   // particle-sharded filter: this handle computes tiles [rank*Bl, rank*Bl + sh_Bown); world = 0: unsharded
    int sh_Bl, sh_Bown;            // Bl = ceil(B / world) tiles per rank in every layout (gathers, halos); the last rank owns B - (world-1) Bl >= 1 of them
};

// n_filters filters of n_particles particles in tiles of `tile` particles, and rank `rank`'s share of them when world > 0.
// Returns false if the last rank would own no tile.
static bool set_layout(Layout* l, int n_particles, int n_filters, int tile, int rank, int world) {
    const int B = (n_particles + tile - 1) / tile;
    l->N = n_particles; l->R = n_filters; l->B = B; l->tile = tile; l->Npad = B * tile;
    l->Bs = (B + 1) & ~1; l->Bpow2 = next_pow2(B);
    l->rshift = 52 - ceil_log2(l->Npad);
    l->split_l2 = B > kSplitLevel2Above ? 1 : 0;
    // in-kernel level-2 keeps T' and A/A' of all tiles in LDS (possible up to 2048 tiles, whichever policy is the default)
    l->lds_bytes = sizeof(double) * (2 * (size_t)(B > kMaxTilesPerFilter ? 2 : (l->Bpow2 < 2 ? 2 : l->Bpow2)) + (size_t)kStageTiles * tile);
    l->lds_bytes_big = sizeof(double) * (4 + (size_t)kStageTiles * tile);
    l->lds_bytes_plan = sizeof(double) * (size_t)(l->Bpow2 < 2 ? 2 : l->Bpow2);
    l->shard_rank = rank; l->shard_world = world;
    l->sh_Bl = l->sh_Bown = 0;
    if (world > 0) {
        // ceil(B / world) tiles per rank; the last rank takes what is left (fewer tiles, a ragged last tile)
        l->sh_Bl = (B + world - 1) / world;
        l->sh_Bown = B - rank * l->sh_Bl < l->sh_Bl ? B - rank * l->sh_Bl : l->sh_Bl;
    }
    return world < 1 || (world - 1) * l->sh_Bl < B;
}

// forecast (forecast.h, *_sim_future_obs): buffers of its own, allocated on first use (forecast_prepare)
struct Forecast {
    std::vector<double> h_last_obs;     // [R] y_prev of this call, as uploaded
    double *T, *R;               // [R][Bs] level-2 tables of the start draw
    FilterScalars* scal;         // [R] S' of the start draw
    double* last;                // [R] h_last_obs on the device
    double* x0;                  // [planes][R][Npad] states of the start population
    uint32_t* start;             // [R][Npad] its ancestors
    double *y, *x;               // samples, rows of Ns doubles: cap_y / cap_x doubles
    size_t cap_y, cap_x;
    hipEvent_t ev[3];            // call start, horizon kernel start, horizon kernel end
    float ms_horizon, ms_call;
};

struct HandleCore : Layout {
    hipStream_t stream;            // where the handle's work is queued: own_stream, or the caller's (set_stream)
    hipStream_t own_stream;        // the stream created with the handle
    hipEvent_t ev0, ev1;           // around the last series
    float last_ms;
    std::string err;               // last_error
    int t;                         // next time index
    int32_t* plan_dev;             // [world][2] source-tile ranges (k_shard_plan)
    int32_t* plan_pin;             // the same on their way to the host (pinned): what shard_plan_to_host stages in
    double* pin;                   // pinned, device-mapped host staging; the step API's R results are written here by the device
    double* pin_dev;               // the same memory as the device sees it
    uint32_t* keybuf;              // [2] Philox key = seed (lo, hi)
    double *ybuf, *zbuf, *per_step;     // observations (ycap time rows), per-step log-likelihood terms [R][tcap]
    int ycap, tcap, gcap;          // time rows of ybuf / zbuf, per_step, the Gamma tables
    int gamma_t0, gamma_rows;      // step API: the Gamma tables hold time indices gamma_t0 .. gamma_t0 + gamma_rows - 1
    // native RCCL drivers (shard_driver.h)
    int32_t* sh_flag;              // [0] a window left the halo ON THIS RANK, [1] / [2] widest reach left / right of the own tiles (in tiles),
                                   // [3] max of [0] over all ranks (reduce_flags after the time loop): what the fallback decision reads
    int32_t sh_stats[4];           // host copy of sh_flag after the last native series
    int sh_margin, sh_rows;        // halo margin (tiles on each side) and rows [margin | Bl own | margin] of the halo buffers
    long sh_exchanged;             // tiles received from other ranks during the last native series
    std::vector<std::pair<void*, bool>> owned;     // (buffer, pinned) from own_alloc: what release_core frees
    Forecast fc;
};

static int fail(HandleCore* h, const char* what, hipError_t e) {
    if (h) h->err = std::string(what) + ": " + hipGetErrorString(e);
    return SSME_ERR_HIP;
}
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(h, #call, e_); } while (0)

// Every device buffer of a handle, and its pinned host memory, comes from here and is freed by release_core.  Whatever p
// held is freed first (growth).
enum class Mem { device, zeroed, pinned };   // pinned: host memory, device-mapped
template <class T>
static void own_free(HandleCore* h, T*& p) {
    if (!p) return;
    for (size_t i = 0; i < h->owned.size(); ++i)
        if (h->owned[i].first == p) {
            if (h->owned[i].second) hipHostFree(p); else hipFree(p);
            h->owned.erase(h->owned.begin() + i);
            break;
        }
    p = nullptr;
}
template <class T>
static hipError_t own_alloc(HandleCore* h, T*& p, size_t bytes, Mem kind = Mem::device) {
    own_free(h, p);
    void* q = nullptr;
    hipError_t e = kind == Mem::pinned ? hipHostMalloc(&q, bytes, hipHostMallocMapped) : hipMalloc(&q, bytes);
    if (e != hipSuccess) return e;
    h->owned.emplace_back(q, kind == Mem::pinned);
    p = static_cast<T*>(q);
    if (kind != Mem::zeroed) return hipSuccess;
    // hipMemset of device memory may return before the fill has run, and the handle's stream is non-blocking: it does not wait for
    // the null stream.  Wait here, so that the fill cannot land after a kernel queued on the handle's stream next (the first
    // forecast of a handle: S' of k_level2_plan was zeroed again between the start and the horizon kernel, which then wrote NaN).
    e = hipMemset(q, 0, bytes);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}

// The dynamic-LDS ceiling of a kernel is state of the (kernel, device) pair, shared by every handle of the process: it is only
// ever raised (a handle with few tiles must not lower what a handle with many tiles was granted).  Every grant of the library
// goes through here, at handle creation (not inside a stream capture), with `device` current; handles are created from several
// threads (the swarm adaptor's pool), hence the lock.
static hipError_t grant_lds(const void* kernel, size_t bytes, int device) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> granted;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = granted[{kernel, device}];
    if (bytes <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}
// the two split level-2 kernels that take a handle's lds_bytes_plan
static hipError_t grant_plan_lds(const HandleCore* h, int device) {
    const hipError_t e = grant_lds(reinterpret_cast<const void*>(&k_level2_plan), h->lds_bytes_plan, device);
    return e != hipSuccess ? e : grant_lds(reinterpret_cast<const void*>(&k_l2_ranges), h->lds_bytes_plan, device);
}

static int create_stream(HandleCore* h) {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = h->stream;
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    return SSME_OK;
}

// what the two destroy functions share: wait for the handle's work, free its buffers, events and own stream
static void release_core(HandleCore* h) {
    if (h->stream) hipStreamSynchronize(h->stream);
    for (auto& b : h->owned) { if (b.second) hipHostFree(b.first); else hipFree(b.first); }
    h->owned.clear();
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    for (hipEvent_t& e : h->fc.ev) if (e) hipEventDestroy(e);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
}

// observations (dy values per time index, and kz covariates) and per-step terms for T time indices; *moved = true if a buffer moved
static int ensure_series_buffers(HandleCore* h, int T, int dy, bool* moved, int kz = 1) {
    if (T > h->ycap) {
        HIPCHK(own_alloc(h, h->ybuf, sizeof(double) * T * dy));
        HIPCHK(own_alloc(h, h->zbuf, sizeof(double) * T * kz, Mem::zeroed));
        h->ycap = T; *moved = true;
    }
    if (T > h->tcap) {
        HIPCHK(own_alloc(h, h->per_step, sizeof(double) * (size_t)T * h->R));
        h->tcap = T; *moved = true;
    }
    return SSME_OK;
}

// ---- entry points that both ABIs repeat (H: ssme_pf_s or ssme_lw_s) -------------------------------------------------------
template <class H>
static int set_stream(H* h, void* hip_stream) {
    if (!h) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : h->own_stream;
    return SSME_OK;
}

// particles this rank owns: sh_Bown tiles, the last of them ragged on the last rank
static size_t own_particles(const HandleCore* h) {
    const size_t first = (size_t)h->shard_rank * h->sh_Bl * kTile, own = (size_t)h->sh_Bown * kTile;
    return (size_t)h->N - first < own ? (size_t)h->N - first : own;
}

// what the two *_shard_create functions check before the handle exists: one filter of n_particles over `world` ranks
static int shard_create_check(int n_particles, int n_filters, int rank, int world) {
    if (world < 1 || world > 64 || rank < 0 || rank >= world) return SSME_ERR_INVALID_ARG;
    if (n_filters != 1 || n_particles < 1) return SSME_ERR_UNSUPPORTED;
    Layout l;
    return set_layout(&l, n_particles, 1, kTile, rank, world) ? SSME_OK : SSME_ERR_UNSUPPORTED;   // every rank must own a tile
}

// flag and widest reaches of the last native series (`ran`: the driver has allocated its buffers)
static int shard_stats(const HandleCore* h, bool ran, int32_t* out4) {
    if (!h || !out4) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1 || !ran) return SSME_ERR_STATE;
    out4[0] = h->sh_stats[3]; out4[1] = h->sh_stats[0]; out4[2] = h->sh_stats[1]; out4[3] = h->sh_stats[2];
    return SSME_OK;
}

// split level-2 of a sharded filter: every tile's source range is in l2_lo / l2_hi; a rank's window is [lo of its first tile,
// hi of its last].  Queues the 2 x world downloads into `stage` ([world][2], pinned).
static int enqueue_window_download(HandleCore* h, const int32_t* l2_lo, const int32_t* l2_hi, int32_t* stage) {
    const size_t Bl = h->sh_Bl;
    for (int d = 0; d < h->shard_world; ++d) {
        const size_t last = (d + 1) * Bl - 1 < (size_t)h->B - 1 ? (d + 1) * Bl - 1 : (size_t)h->B - 1;     // the last rank may own fewer tiles
        HIPCHK(hipMemcpyAsync(stage + 2 * d, l2_lo + d * Bl, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(stage + 2 * d + 1, l2_hi + last, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    return SSME_OK;
}

// the plan buffers of a sharded handle: every rank's window on the device and its pinned staging
static int alloc_plan_buffers(HandleCore* h) {
    HIPCHK(own_alloc(h, h->plan_dev, sizeof(int32_t) * 2 * h->shard_world));
    HIPCHK(own_alloc(h, h->plan_pin, sizeof(int32_t) * 2 * h->shard_world, Mem::pinned));
    return SSME_OK;
}

static int shard_layout(const HandleCore* h, int32_t* out4) {
    if (!h || !out4) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    out4[0] = h->B; out4[1] = h->sh_Bl; out4[2] = h->sh_Bown; out4[3] = (int32_t)own_particles(h);
    return SSME_OK;
}

template <class H>
static int read_per_step(H* h, double* out, int T) {
    if (!h || !out || T < 1 || T > h->tcap) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    // device layout is [R][tcap]; return [R][T]
    for (int r = 0; r < h->R; ++r)
        HIPCHK(hipMemcpyAsync(out + (size_t)r * T, h->per_step + (size_t)r * h->tcap, sizeof(double) * T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SSME_OK;
}

// the R log-likelihoods from the device scalars (FilterScalars or LwScalars); synchronises, out may be null
template <class H>
static int read_loglik(H* h, double* out) {
    using Scalars = std::remove_pointer_t<decltype(h->scal)>;
    std::vector<Scalars> sc(h->R);
    HIPCHK(hipMemcpyAsync(sc.data(), h->scal, sizeof(Scalars) * h->R, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (out) for (int r = 0; r < h->R; ++r) out[r] = sc[r].loglik;
    return SSME_OK;
}

static int elapsed_ms(const HandleCore* h, float* ms) {
    if (!h || !ms) return SSME_ERR_INVALID_ARG;
    *ms = h->last_ms;
    return SSME_OK;
}

// ---- forecast: what ssme_pf_sim_future_obs and ssme_lw_sim_future_obs do around their own kernels ---------------------------
// The common buffers and the events on first use (x0: x0_planes planes of [R][Npad]), the samples grown to ny / nx doubles (nx = 0:
// no states asked for), the event of the call's start, and fc.h_last_obs (filled by the caller) on its way to the device.
// what forecast_plan writes: the level-2 tables and S' of the start draw, on first use (also the smoothing calls', which draw their
// terminal particles as the forecast draws its start population and need nothing else of it)
static int forecast_tables(HandleCore* h) {
    Forecast& f = h->fc;
    const size_t R = h->R, nb = R * h->Bs;
    if (!f.T) HIPCHK(own_alloc(h, f.T, sizeof(double) * nb));
    if (!f.R) HIPCHK(own_alloc(h, f.R, sizeof(double) * nb));
    if (!f.scal) HIPCHK(own_alloc(h, f.scal, sizeof(FilterScalars) * R, Mem::zeroed));
    return SSME_OK;
}

template <class H>
static int forecast_prepare(H* h, int x0_planes, size_t ny, size_t nx) {
    Forecast& f = h->fc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t R = h->R, np = R * h->Npad;
    const int rc = forecast_tables(h);
    if (rc != SSME_OK) return rc;
    if (!f.last) {
        HIPCHK(own_alloc(h, f.last, sizeof(double) * R));
        HIPCHK(own_alloc(h, f.x0, sizeof(double) * np * x0_planes));
        HIPCHK(own_alloc(h, f.start, sizeof(uint32_t) * np));
        for (hipEvent_t& e : f.ev) HIPCHK(hipEventCreate(&e));
    }
    // capacity 0 while the buffer is replaced: a failed allocation leaves none
    if (ny > f.cap_y) { f.cap_y = 0; HIPCHK(own_alloc(h, f.y, sizeof(double) * ny)); f.cap_y = ny; }
    if (nx > f.cap_x) { f.cap_x = 0; HIPCHK(own_alloc(h, f.x, sizeof(double) * nx)); f.cap_x = nx; }
    HIPCHK(hipEventRecord(f.ev[0], h->stream));
    HIPCHK(hipMemcpyAsync(f.last, f.h_last_obs.data(), sizeof(double) * R, hipMemcpyHostToDevice, h->stream));
    return SSME_OK;
}

// level-2 of the weights behind p.tsum_in / p.tmax_in (the last step's: those the expectations use) into the forecast's own tables
// and scalars; p.t = the steps done so far.  Nothing is accounted and no ranges are planned.
static void forecast_plan(HandleCore* h, StepArgs p) {
    p.l2_T = h->fc.T; p.l2_R = h->fc.R; p.scal = h->fc.scal;
    p.finalize_prev = 0; p.per_step = nullptr; p.ll_host = nullptr;
    hipLaunchKernelGGL(k_level2_plan, dim3(h->R), dim3(1024), h->lds_bytes_plan, h->stream, p, 0);
}

// After the horizon kernel: its end event, the launches' errors, the downloads of y (rows_y rows of N out of rows of Ns), x (rows_x
// rows; null: none) and the start draw's ancestors ([R][N] out of [R][Npad]; null: none), the wait, and the two times.
static int forecast_finish(HandleCore* h, double* y_out, size_t rows_y, double* x_out, size_t rows_x, uint32_t* start_out) {
    Forecast& f = h->fc;
    const size_t N = h->N, Ns = (N + 1) & ~(size_t)1;
    HIPCHK(hipEventRecord(f.ev[2], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(y_out, sizeof(double) * N, f.y, sizeof(double) * Ns, sizeof(double) * N, rows_y, hipMemcpyDeviceToHost, h->stream));
    if (x_out) HIPCHK(hipMemcpy2DAsync(x_out, sizeof(double) * N, f.x, sizeof(double) * Ns, sizeof(double) * N, rows_x, hipMemcpyDeviceToHost, h->stream));
    if (start_out) HIPCHK(hipMemcpy2DAsync(start_out, sizeof(uint32_t) * N, f.start, sizeof(uint32_t) * h->Npad, sizeof(uint32_t) * N, h->R, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventElapsedTime(&f.ms_horizon, f.ev[1], f.ev[2]));
    HIPCHK(hipEventElapsedTime(&f.ms_call, f.ev[0], f.ev[2]));
    return SSME_OK;
}

// HIP-event times of the last forecast: the horizon kernel alone, the whole call without the downloads
static int forecast_elapsed(const HandleCore* h, float* horizon_kernel_ms, float* call_ms) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (horizon_kernel_ms) *horizon_kernel_ms = h->fc.ms_horizon;
    if (call_ms) *call_ms = h->fc.ms_call;
    return SSME_OK;
}

static const char* last_error(const HandleCore* h) { return h ? h->err.c_str() : ""; }

// step APIs: the Gamma-table row of time index h->t.  The tables are drawn kStepGammaChunk time steps at a time (data
// independent), so that the table launches are paid once per chunk and not once per call.
template <class H>
static int step_gamma_row(H* h, void (*draw)(H* h, int t0, int nT)) {
    if (h->t < h->gamma_t0 || h->t >= h->gamma_t0 + h->gamma_rows) {
        draw(h, h->t, kStepGammaChunk);
        h->gamma_t0 = h->t; h->gamma_rows = kStepGammaChunk;
    }
    return h->t - h->gamma_t0;
}


// Gamma tables of one multinomial draw for time indices t0 .. t0+nT-1 into table rows 0 .. nT-1: the draws (Philox stream
// `draw_stream`), then their prefix sums and totals (`extra_stream`)
static void launch_gamma_tables(HandleCore* h, double* gam, double* pgam, double* gtot, uint32_t draw_stream, uint32_t extra_stream,
                                int tile, uint32_t first_filter, int t0, int nT) {
    hipLaunchKernelGGL(k_gamma_draw, dim3((h->B + kThreads - 1) / kThreads, nT, h->R), dim3(kThreads), 0, h->stream,
                       gam, h->N, h->B, h->R, t0, (const uint32_t*)h->keybuf, first_filter, draw_stream, tile);
    if (h->B <= 64)           // short rows: one thread per row; else one workgroup per row
        hipLaunchKernelGGL(k_gamma_prefix_rows, dim3((nT * h->R + kThreads - 1) / kThreads), dim3(kThreads), 0, h->stream,
                           (const double*)gam, pgam, gtot, h->B, h->R, nT, t0, (const uint32_t*)h->keybuf, first_filter, extra_stream);
    else
        hipLaunchKernelGGL(k_gamma_prefix, dim3(nT * h->R), dim3(kThreads), 0, h->stream,
                           (const double*)gam, pgam, gtot, h->B, h->R, nT, t0, (const uint32_t*)h->keybuf, first_filter, extra_stream);
}

}  // namespace ssme
