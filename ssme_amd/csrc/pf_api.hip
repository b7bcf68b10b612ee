// pf_api.hip -- extern "C" boundary (include/ssme_pf.h) over the gfx950 kernels.
// Host side of the drop-in: owns device buffers, the HIP stream, the hipGraph of a series.
// No torch types; no CPU fallback: without a HIP device every call fails with SSME_ERR_HIP.
#include "../../include/ssme_pf.h"
#include "pf_kernels.h"
#include "lw_kernels.h"
#include "pf_small.h"
#include "lw_small.h"
#include "user_expect.h"
#include "forecast.h"
#include "smooth.h"
#include "backward.h"
#include "marginal.h"
#include "series_history.h"
#include "marginal_state.h"
#include "handle_core.h"
#include "shard_driver.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace ssme;

// k_filter_step of one (model, tile): fn[BIG][WL2][RS + 1] at the tile's own workgroup size nt (no BIG + WL2 kernel), and the
// general 2048-particle kernel at 256 / 1024 threads (ssme_pf_set_tuning); resident[RS]: fn[0][0][RS + 1] of 2048-particle tiles
// with the schedule and store policy of a grid that is resident at once compiled in (select_step_kernel)
struct StepKernels { const void* fn[2][2][3]; const void* wide[2]; const void* resident[2]; int nt; };

struct ssme_pf_s : HandleCore {
    ssme_pf_config cfg;
    StepKernels kern;        // resolved at creation: what the handle launches and what it is granted
    bool params_set;
    int debug_anc, keep_logw;
    int graph_mode;
    double *l2_T, *l2_R;     // [R][Bs] split level-2 outputs
    double* l2_work;         // [R][Bs] + [R][32]: scratch of the multi-workgroup level-2
    int32_t *l2_lo, *l2_hi;
    int32_t* l2_ticket;      // [R] arrival counters of the one-launch level-2 (StepArgs::l2_inkernel)
    int l2_tables;           // set_debug bit 4: the split level-2 writes its tables and ranges (k_level2_plan / k_l2_ranges), as sharded filters do
    double* small_ms;        // [R][tcap][2] scratch of the one-tile whole-series kernel
    double* yz_step;         // device [2]: y and z of the step API, uploaded by ONE copy
    int32_t* ticket;         // device [R]: arrival counters of the step API's in-kernel accounting (zero between launches)
    int num_cus;             // compute units of the device (priority schedule of the step kernel)
    int small_series;        // 1: one-tile filters run the whole series in one launch (pf_small.h; series_route decides)
    double y_step_v[3];      // step API: components 1 .. of this call's vector observation
    double z_step_v[3];      // ... and covariates 1 .. of a user model with dim_cov > 1
    int dx, dy;              // state / observation dimension: 1, or the user model's dim_x / dim_y (model_api.h)
    int kcov, kz;            // dim_cov of the user model (0: none declared) and the covariates per time row of z / zbuf: max(kcov, 1)
    int nt;                  // threads per 2048-particle tile of k_filter_step (256, 512, 1024)
    // C++ shard driver (ssme_pf_shard_run_series): halo buffers [margin | own tiles | margin] x 2048 doubles, ping-pong;
    // this rank's tile sums / maxima, their gathered forms; exact-path window buffers
    double *sh_x[2], *sh_c[2], *sh_loc, *sh_tsum, *sh_tmax, *sh_winx, *sh_winc;
    int sh_path;             // path of the last native series (1 fixed halo, 2 exact)
    // device state; [2] = ping-pong (step t reads cur, writes cur ^ 1)
    double* x[2];
    double* cdf[2];          // integer-valued doubles (< 2^53)
    double* tsum[2];
    double* tmax[2];
    double *logw, *scratchR;
    double *exp_part, *exp_out;  // expectations: [R][Bs][4] per-tile numerators; [5][R] per-filter values + [5] means over filters
    double* wscratch;            // [Npad] weights of one filter (host-side functionals), allocated on first use
    double *uexp_part, *uexp_out;    // the user model's own functionals (user_expect.h): [R][Bs][n_h] per-tile numerators, [n_h][R] values; allocated on first use
    double last_z;               // covariate of the last step (0 when it had none): what the user model's h receives
    double last_zv[kMaxCov];     // ... all of them, for a header with dim_cov (zeros when the step had none)
    double* fc_zfut;             // [fc_zfut_cap] future covariates of ssme_pf_sim_future_obs_cov on the device
    size_t fc_zfut_cap;
    double *gam, *pgam, *gtot;   // Gamma tables of the multinomial resampler, gcap time rows
    uint32_t* anc;
    FilterScalars* scal;
    ModelConst* mc;
    int cur;                 // buffer index holding the latest step's output
    // graph cache
    hipGraphExec_t gexec;
    int g_T, g_has_z, g_debug, g_logw, g_nt;
    FunctionalIds g_rec_fs;      // ... and the recording configuration it was captured with
    int g_rec_user;
    // recorded series (ssme_pf_set_series_expectations): E[h(x_t) | y_{1:t}] of every step of a run_series
    FunctionalIds rec_fs;        // built-in functionals to record (n = 0: none)
    int rec_user;                // 1: the user model's n_h functionals too
    double *traj, *utraj;        // [traj_cap][rec_fs.n][R], [traj_cap][n_h][R]; held only while recording is on
    int traj_cap, traj_n;        // time rows both hold; built-in functionals traj was sized for
    int rec_T, rec_n, rec_nh;    // what the last run_series recorded: rows, built-in functionals, user functionals
    // series history and smoothing (ssme_pf_set_series_history; smooth.h): the populations and ancestors of every step of a run_series
    SeriesHistoryState hist;     // the setting, the rows the buffers hold, the history in force (series_history.h)
    double* hist_x;              // [hist_cap][dx][R][Npad]
    uint32_t* hist_anc;          // [hist_cap][R][Npad]
    int hist_live;               // enqueue_step is queuing a recording series: x and the ancestors go to the history rows
    int g_hist;                  // the cached graph was captured with the history on
    double* sm_x;                // [R][K][T][dx] sampled trajectories, sm_cap_x doubles
    uint32_t *sm_idx, *sm_term;  // [R][K][T] their lineage indices, [R][K] given terminal indices
    size_t sm_cap_x, sm_cap_idx, sm_cap_term, sm_cap_part;
    double *sm_part, *sm_out;    // [T][R][Bs][4] per-tile numerators of the sweep, [T][4][R] its rows
    hipEvent_t sm_ev[3];         // call start, backward kernel start, kernels' end
    float sm_ms_kernel, sm_ms_call;
    // backward simulation (backward.h): the pre-resampling log-weights of every step of the history, recomputed on first use
    double* bs_lw;               // [hist.lw_cap][R][Npad]; freed with the history rows
    int hist_has_z;              // the recorded series had covariates (zbuf holds them; 0: the kernels read zeros)
    // marginal smoothing (marginal.h): the weight rows om, then the column tables m and D, each [msm.cap][R][Npad]; freed with the history rows
    MarginalRowsState msm;       // do they hold the history in force?  Told of every event of `hist` (marginal_state.h)
    double* ms_rows;
    double* ms_out;              // [T][4][R] the smoothed means, ms_cap_out doubles
    size_t ms_cap_out;
    std::vector<ModelConst> h_mc;
    // forecast (HandleCore::fc): fc.x0 is [dx][R][Npad], the samples fc.y / fc.x [R][H][dy][Ns] / [R][H][dx][Ns]
    std::vector<double> h_gscale;    // per filter: scale of the observation draw (set_params)
    double* fc_gscale;               // [R] the same on the device, allocated on first use
};

// Wait for a stream with the latency of a poll: hipStreamSynchronize spins only briefly and then sleeps on an interrupt,
// which adds ~200 us to a filter() call whose kernels take longer than that window (measured: 512 filters x 2^14
// particles, 146 vs 420 us per call).  Poll for up to ~5 ms, then fall back to the blocking wait.
constexpr uint64_t kStepPending = 0x7ff8a5a5c3c3e1e1ull;     // "result not written yet" in the step API's mapped result buffer

static hipError_t wait_stream_low_latency(hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(s);
        if (q != hipErrorNotReady) return q;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) return hipStreamSynchronize(s);
    }
}

// The tail of both *_shard_plan: every rank's window [lo, hi] on its way to the caller through plan_pin.  every_tile: unsorted
// targets need every tile; else the windows come from the split level-2's per-tile ranges (more than 1024 tiles in total) or from
// plan_dev (k_shard_plan).  Synchronises.
static int shard_plan_to_host(HandleCore* h, bool every_tile, const int32_t* l2_lo, const int32_t* l2_hi, int32_t* lo_hi) {
    if (every_tile) {
        for (int d = 0; d < h->shard_world; ++d) { h->plan_pin[2 * d] = 0; h->plan_pin[2 * d + 1] = h->B - 1; }
    } else if (h->split_l2) {
        const int rc = enqueue_window_download(h, l2_lo, l2_hi, h->plan_pin);
        if (rc != SSME_OK) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(h->plan_pin, h->plan_dev, sizeof(int32_t) * 2 * h->shard_world, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(wait_stream_low_latency(h->stream));
    for (int d = 0; d < 2 * h->shard_world; ++d) lo_hi[d] = h->plan_pin[d];
    return SSME_OK;
}

// Step APIs: the R results are awaited where they land.  The host marks the mapped result slots kStepPending (a NaN
// payload no computation produces) before the launch and polls them instead of the stream's completion signal, which
// trails the kernel's last store by its end-of-kernel cache write-back.  The stream stays ordered: the next call
// queues behind this one.  A launch that takes longer than 5 ms falls back to the stream (and reports its errors).
static void mark_results_pending(double* slots, int R) {
    volatile uint64_t* res = reinterpret_cast<volatile uint64_t*>(slots);
    for (int r = 0; r < R; ++r) res[r] = kStepPending;
}
static hipError_t wait_results(hipStream_t s, const double* slots, int R) {
    const volatile uint64_t* res = reinterpret_cast<const volatile uint64_t*>(slots);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (int r = 0; r < R;) {
        if (res[r] != kStepPending) { ++r; continue; }
        if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) return hipStreamSynchronize(s);
    }
    return hipSuccess;
}

// SSME_F32 handles (the reference instantiated with float_t = float, example/main.cpp:13): float at the boundary --
// observations, covariates and parameters are rounded to float on entry, every value handed back is rounded to float --
// while the arithmetic stays fp64.  Plain fp32 VALU instructions issue at the fp64 rate on gfx950 (only packed fp32 is
// faster), so float arithmetic would buy no time; it would only coarsen the callbacks below the fixed-point weights.
static inline double f32r(double v) { return (double)(float)v; }
static void round_out(const ssme_pf_handle h, double* p, size_t n) {
    if (h->cfg.dtype == SSME_F32 && p) for (size_t i = 0; i < n; ++i) p[i] = f32r(p[i]);
}

// Derived constants; operation order mirrors oracle/ssme_oracle.cpp derive().
static ModelConst derive(int model, const double* th) {
    ModelConst c{};
#if SSME_HAS_USER_MODEL
    if (model == SSME_MODEL_USER0) return ssme_user_model0::derive(th);
#endif
    if (model == SSME_MODEL_SVOL) {            // (beta, phi, sigma)
        const double beta = th[0], phi = th[1], sigma = th[2];
        c.a0 = phi; c.a1 = sigma;
        c.a2 = sigma / dsqrt(1.0 - phi * phi);
        c.a3 = dlog(beta);
        c.a4 = 1.0 / (beta * beta);
        c.bad = !(beta > 0.0);
    } else if (model == SSME_MODEL_SVOL_LEVERAGE) {   // (phi, mu, sigma, rho)
        const double phi = th[0], mu = th[1], sigma = th[2], rho = th[3];
        c.a0 = phi; c.a1 = mu;
        c.a2 = sigma / dsqrt(1.0 - phi * phi);
        c.a3 = sigma * dsqrt(1.0 - phi * phi);
        c.a4 = rho * sigma;
        c.bad = 0;
    } else {                                    // (phi, sigma, tau)
        const double phi = th[0], sigma = th[1], tau = th[2];
        c.a0 = phi; c.a1 = sigma;
        c.a2 = sigma / dsqrt(1.0 - phi * phi);
        c.a3 = dlog(tau);
        c.a4 = 1.0 / tau;
        c.bad = !(tau > 0.0);
    }
    return c;
}

// state / observation dimension of a model: 1 for the built-in models, dim_x / dim_y of a compiled-in user model
static void dims_of(int model, int* dx, int* dy) {
    *dx = 1; *dy = 1;
#if SSME_HAS_USER_MODEL
    if (model == SSME_MODEL_USER0) { *dx = user_dims<ssme_user_model0>::dx; *dy = user_dims<ssme_user_model0>::dy; }
#endif
}
// covariates per step a model's callbacks receive as a vector: dim_cov of a compiled-in user model that declares it, else 0
static int kcov_of(int model) {
#if SSME_HAS_USER_MODEL
    if (model == SSME_MODEL_USER0) return user_cov<ssme_user_model0>::k;
#endif
    (void)model;
    return 0;
}
static int n_theta_of(int model) {
#if SSME_HAS_USER_MODEL
    if (model == SSME_MODEL_USER0) return ssme_user_model0::n_theta;
#endif
    return model == SSME_MODEL_SVOL_LEVERAGE ? 4 : 3;
}
// The bootstrap handle's pinned, device-mapped staging (pin / pin_dev), as offsets in doubles for a handle of R filters
struct PinLayout {
    static constexpr size_t kSwarmSlots = 8;                                // kMaxFunctionals means, then the mean log conditional likelihood
    static_assert(kMaxFunctionals + 1 <= kSwarmSlots, "the swarm aggregates have 8 slots");
    static constexpr size_t yz = 0;                                         // y and z of the step API
    static constexpr size_t results = 2;                                    // its R results, written by the device
    static size_t swarm(int R) { return results + (size_t)R; }              // ssme_pf_swarm_aggregate*
    static size_t user(int R) { return swarm(R) + kSwarmSlots; }            // ssme_pf_swarm_aggregate_user: kMaxUserFunctionals means + 1
    static size_t size(int R) { return user(R) + kMaxUserFunctionals + 1; }
};

static bool logw_needed(ssme_pf_handle h) { return h->keep_logw || h->cfg.resamp_sched > 1; }

// arguments of the step that reads buffers `cur` and writes `cur ^ 1`
static StepArgs step_args(ssme_pf_handle h) {
    StepArgs a{};
    const int i = h->cur, o = h->cur ^ 1;
    a.x_in = h->x[i]; a.x_out = h->x[o]; a.xplane = (size_t)h->R * h->Npad;
    a.cdf_in = h->cdf[i]; a.cdf_out = h->cdf[o];
    a.tsum_in = h->tsum[i]; a.tsum_out = h->tsum[o];
    a.tmax_in = h->tmax[i]; a.tmax_out = h->tmax[o];
    a.logw = logw_needed(h) ? h->logw : nullptr;
    a.anc = h->debug_anc ? h->anc : nullptr;
    a.scal = h->scal; a.mc = h->mc; a.y = h->ybuf; a.z = nullptr; a.per_step = nullptr;
    a.gam = h->gam; a.pgam = h->pgam; a.gtot = h->gtot;
    a.N = h->N; a.Npad = h->Npad; a.B = h->B; a.Bs = h->Bs; a.Bpow2 = h->Bpow2; a.rshift = h->rshift; a.R = h->R;
    a.tile = h->tile;
    a.Tcap = h->tcap;
    a.resampler = h->cfg.resampler; a.resamp_sched = h->cfg.resamp_sched;
    a.keyp = h->keybuf; a.first_filter = h->cfg.first_filter_id;
    a.logN = dlog((double)h->N);
    a.l2_T = h->l2_T; a.l2_R = h->l2_R; a.l2_lo = h->l2_lo; a.l2_hi = h->l2_hi; a.l2_work = h->l2_work;
    a.l2_inkernel = (h->split_l2 && h->shard_world == 0 && !h->l2_tables) ? 1 : 0; a.l2_ticket = h->l2_ticket;
    {
        double* tail = h->l2_work + (size_t)h->R * h->Bs;                     // [R][kL2Scratch] and 32 zeros after them
        a.l2_tsrc = a.l2_inkernel ? h->l2_work : h->l2_T;
        a.l2_offs = a.l2_inkernel ? tail + kL2Offsets : tail + (size_t)h->R * kL2Scratch;
        a.l2_offs_stride = a.l2_inkernel ? kL2Scratch : 0;
    }
    {
        // two 512-thread workgroups fit a CU (LDS): is the whole grid resident at once?
        const long blocks = (long)(h->shard_world > 0 ? h->sh_Bown : h->B) * h->R;
        a.prio_mode = (blocks <= 2L * h->num_cus) ? 1 : 2;
        static const char* force = getenv("SSME_PRIO_MODE");         // measurement aid: 0 none, 1 / 2 the two schedules, 3.. experimental
        if (force) a.prio_mode = atoi(force);
        // measured (profiles/r02_stream_stores.txt): 2048-particle tiles gain 7-10 % up to 3 workgroups per CU, nothing
        // or -3 % beyond; the smaller tiles (mid-size handles, latency bound) are indifferent
        a.stream_stores = (h->tile == kTile && blocks <= 3L * h->num_cus) ? 1 : 0;
        static const char* force_ss = getenv("SSME_STREAM_STORES");  // measurement aid: 0 / 1
        if (force_ss) a.stream_stores = atoi(force_ss);
    }
#ifdef SSME_ABLATE
    { const char* e = getenv("SSME_ABLATE_MASK"); a.ablate = e ? atoi(e) : 0; }
    {
        static unsigned long long* g_stamps = nullptr;       // diagnostic build only
        if (getenv("SSME_STAMPS")) {
            if (!g_stamps) { hipMalloc(&g_stamps, sizeof(unsigned long long) * 16 * (size_t)h->B * h->R); }
            a.stamps = g_stamps;
            if (getenv("SSME_STAMPS_DUMP")) {   // dump the stamps of the last launch (call after a sync)
                std::vector<unsigned long long> hs(16 * (size_t)h->B * h->R);
                hipMemcpy(hs.data(), g_stamps, hs.size() * 8, hipMemcpyDeviceToHost);
                FILE* f = fopen(getenv("SSME_STAMPS_DUMP"), "w");
                for (size_t i = 0; i < hs.size(); i += 16) { for (int k = 0; k < 16; ++k) fprintf(f, "%llu ", hs[i + k]); fprintf(f, "\n"); }
                fclose(f);
            }
        }
    }
#endif
    return a;
}

// Tile size when the caller does not choose (part of the arithmetic specification: the oracle applies the same rule).
// 2048-particle tiles are the efficient shape at full occupancy (fewer, fatter workgroups; N <= 2048 is the whole-series
// kernel).  Smaller handles get the smallest tile that still leaves every workgroup resident at once, so that mid-size
// filters spread over the 256 CUs: 512-particle tiles while they make at most 256 workgroups (one filter of 2^16: 128
// workgroups instead of 32, 10.3 -> 7.4 us per step), 1024-particle tiles while those make at most 512 (one filter of
// 2^18: 10.7 -> 8.4 us; 2^19: 11.5 -> 10.8 us), 2048 beyond (profiles/r02_tile_sweep.txt).  The rule reads N and the
// size of the BANK of filters (ssme_pf_config::n_filters_total, else the handle's n_filters): a bank that is split over
// GPUs or over one handle per member declares its total, so a filter's bits do not depend on the split.
static int default_tile(int n_particles, int n_filters) {
    if (n_particles <= kTile) return kTile;
    const long R = n_filters;
    if (R * ((n_particles + kTileSmall - 1) / kTileSmall) <= 256) return kTileSmall;   // at most one 256-thread block per CU
    if (R * ((n_particles + kTileMid - 1) / kTileMid) <= 512) return kTileMid;          // at most two 512-thread blocks per CU
    return kTile;
}

// cfg.model as a compile-time model id: f(std::integral_constant<int, MODEL_...>) for the handle's model
template <class F>
static void with_model(int model, F&& f) {
    switch (model) {
        case SSME_MODEL_SVOL: f(std::integral_constant<int, MODEL_SVOL>{}); break;
        case SSME_MODEL_SVOL_LEVERAGE: f(std::integral_constant<int, MODEL_SVOL_LEVERAGE>{}); break;
#if SSME_HAS_USER_MODEL
        case SSME_MODEL_USER0: f(std::integral_constant<int, MODEL_USER0>{}); break;
#endif
        default: f(std::integral_constant<int, MODEL_LIN_GAUSS>{}); break;
    }
}

// The instantiations of k_filter_step one (model, tile) has.  RS: the common configurations (multinomial -- the reference's --
// or systematic resampling, every step, t > 0, no debug outputs) have their own instantiations, -1 is the general kernel.
// WL2: filters of at most 128 tiles take the level-2 wave by wave; BIG (split level-2) has no such variant.
template <int MODEL, int NT, int TILE, bool BIG, bool WL2>
static void fill_rs(const void* (&fn)[3]) {
    fn[0] = reinterpret_cast<const void*>(&k_filter_step<MODEL, NT, BIG, TILE, -1, WL2>);
    fn[1] = reinterpret_cast<const void*>(&k_filter_step<MODEL, NT, BIG, TILE, 0, WL2>);
    fn[2] = reinterpret_cast<const void*>(&k_filter_step<MODEL, NT, BIG, TILE, 1, WL2>);
}
template <int MODEL, int NT, int TILE>
static void fill_step_kernels(StepKernels& k) {
    k.nt = NT;
    fill_rs<MODEL, NT, TILE, false, false>(k.fn[0][0]);
    fill_rs<MODEL, NT, TILE, false, true>(k.fn[0][1]);
    fill_rs<MODEL, NT, TILE, true, false>(k.fn[1][0]);
}
template <int MODEL>
static StepKernels step_kernels(int tile) {
    StepKernels k{};
    if (tile == kTileSmall) fill_step_kernels<MODEL, 256, kTileSmall>(k);
    else if (tile == kTileMid) fill_step_kernels<MODEL, 512, kTileMid>(k);      // 1024-particle tiles: 512 threads, one particle pair each
    else {
        fill_step_kernels<MODEL, 512, kTile>(k);
        k.wide[0] = reinterpret_cast<const void*>(&k_filter_step<MODEL, 256, false, kTile, -1>);
        k.wide[1] = reinterpret_cast<const void*>(&k_filter_step<MODEL, 1024, false, kTile, -1>);
        // the RS >= 0 kernels of filters of more than 128 tiles once more, with the schedule and store policy of a grid that is
        // resident at once compiled in (step_args: prio_mode 1, streaming stores) -- the flagship shape
        k.resident[0] = reinterpret_cast<const void*>(&k_filter_step<MODEL, 512, false, kTile, 0, false, true>);
        k.resident[1] = reinterpret_cast<const void*>(&k_filter_step<MODEL, 512, false, kTile, 1, false, true>);
    }
    return k;
}
// every kernel of the handle's table gets its LDS ceiling (handle creation)
static hipError_t grant_step_lds(const ssme_pf_s* h) {
    hipError_t e = hipSuccess;
    for (int big = 0; big < 2; ++big)
        for (int wl2 = 0; wl2 < 2; ++wl2)
            for (const void* fn : h->kern.fn[big][wl2])
                if (fn && e == hipSuccess) e = grant_lds(fn, big ? h->lds_bytes_big : h->lds_bytes, h->cfg.device);
    for (const void* fn : h->kern.wide)
        if (fn && e == hipSuccess) e = grant_lds(fn, h->lds_bytes, h->cfg.device);
    for (const void* fn : h->kern.resident)
        if (fn && e == hipSuccess) e = grant_lds(fn, h->lds_bytes, h->cfg.device);
    return e;
}

// the kernel of the handle's table that runs the step `a` describes, its workgroup size and dynamic LDS
struct StepLaunch { const void* fn; int nt; size_t lds; };
static StepLaunch select_step_kernel(const ssme_pf_s* h, const StepArgs& a) {
    int rs = -1;
    if (h->cfg.resamp_sched == 1 && a.t > 0 && !a.anc && !a.logw && !a.ticket)
        rs = h->cfg.resampler == SSME_RESAMP_MULTINOMIAL ? 0 : (h->cfg.resampler == SSME_RESAMP_SYSTEMATIC ? 1 : -1);
    if (h->split_l2) return {h->kern.fn[1][0][rs + 1], h->kern.nt, h->lds_bytes_big};
    if (h->tile == kTile && h->nt != 512) return {h->kern.wide[h->nt == 1024], h->nt, h->lds_bytes};      // ssme_pf_set_tuning
    if (rs >= 0 && a.B > 128 && a.prio_mode == 1 && a.stream_stores == 1 && h->kern.resident[rs]) return {h->kern.resident[rs], h->kern.nt, h->lds_bytes};
    return {h->kern.fn[0][a.B <= 128 ? 1 : 0][rs + 1], h->kern.nt, h->lds_bytes};
}
static void launch_step_on(ssme_pf_handle h, const StepArgs& a, dim3 grid) {
    const StepLaunch k = select_step_kernel(h, a);
    void* args[] = {const_cast<StepArgs*>(&a)};
    hipLaunchKernel(k.fn, grid, dim3(k.nt), args, k.lds, h->stream);
}
static void launch_step(ssme_pf_handle h, const StepArgs& a) { launch_step_on(h, a, dim3(h->B, h->R)); }
// Gamma tables for time indices t0 .. t0+nT-1 into table rows 0 .. nT-1
static void launch_gamma(ssme_pf_handle h, int t0, int nT) {
    if (h->cfg.resampler != SSME_RESAMP_MULTINOMIAL) return;
    launch_gamma_tables(h, h->gam, h->pgam, h->gtot, STREAM_GAMMA, STREAM_RESAMP_EXTRA, h->tile, h->cfg.first_filter_id, t0, nT);
}
// the split level-2 of one draw: one workgroup per filter up to 1024 tiles, several above (k_l2_scan_blocks + k_l2_ranges)
static void launch_level2(hipStream_t st, const StepArgs& a, int n_filters, size_t lds, int ranges) {
    if (a.l2_inkernel) {
        // unsharded bootstrap filter: one launch; k_filter_step<.., true> finds the source-tile ranges itself
        hipLaunchKernelGGL(k_l2_scan_blocks, dim3((a.B + 1023) / 1024, n_filters), dim3(1024), 0, st, a);
    } else if (a.l2_work && a.B > 1024) {
        const dim3 grid((a.B + 1023) / 1024, n_filters);
        hipLaunchKernelGGL(k_l2_scan_blocks, grid, dim3(1024), 0, st, a);
        hipLaunchKernelGGL(k_l2_ranges, grid, dim3(1024), lds, st, a, ranges);
    } else
        hipLaunchKernelGGL(k_level2_plan, dim3(n_filters), dim3(1024), lds, st, a, ranges);
}
// accounts the log conditional likelihood of step t from the buffers the step wrote (now `cur`)
// split level-2 of the buffers `cur` holds: for the step t about to run (plan_ranges) or only the accounting of step t-1
static void launch_plan(ssme_pf_handle h, int t, int gi, bool plan_ranges, bool finalize_prev, bool record_per_step,
                        double* ll_host = nullptr) {
    StepArgs a = step_args(h);
    a.t = t; a.gi = gi; a.finalize_prev = finalize_prev ? 1 : 0;
    a.ll_host = ll_host;
    a.per_step = record_per_step ? h->per_step : nullptr;
    launch_level2(h->stream, a, h->R, h->lds_bytes_plan, plan_ranges ? 1 : 0);
}
static void launch_kf(ssme_pf_handle h, int t, bool record_per_step, double* ll_host = nullptr) {
    if (h->split_l2) { launch_plan(h, t + 1, 0, false, true, record_per_step, ll_host); return; }
    StepArgs a = step_args(h);
    a.ll_host = ll_host;
    a.t = t;
    a.per_step = record_per_step ? h->per_step : nullptr;
    hipLaunchKernelGGL(kf_finalize, dim3(h->R), dim3(kThreads), 0, h->stream, a);
}

// row t of the series history: the dx planes of the population of step t
static double* hist_row(const ssme_pf_s* h, int t) { return h->hist_x + (size_t)t * h->dx * h->R * h->Npad; }

// enqueue one filter step at time index t reading y[yi] and gamma-table row gi
static void enqueue_step(ssme_pf_handle h, int t, int yi, int gi, bool has_z, bool finalize_prev, bool record_per_step,
                         bool from_step_staging = false, bool results_to_host = true) {
    StepArgs a = step_args(h);
    a.z = has_z ? h->zbuf : nullptr;
    if (from_step_staging) {
        a.by_value = 1; a.y_now = h->pin[PinLayout::yz]; a.z_now = has_z ? h->pin[PinLayout::yz + 1] : 0.0;
        for (int d = 1; d < h->dy; ++d) a.y_now_v[d - 1] = h->y_step_v[d - 1];
        for (int j = 1; j < h->kcov; ++j) a.z_now_v[j - 1] = has_z ? h->z_step_v[j - 1] : 0.0;
        if (!h->split_l2) { a.ticket = h->ticket; a.ll_host = results_to_host ? h->pin_dev + PinLayout::results : nullptr; }     // accounting inside the step kernel (its last workgroup)
    }
    a.per_step = record_per_step ? h->per_step : nullptr;
    a.t = t; a.yi = yi; a.gi = gi; a.finalize_prev = finalize_prev ? 1 : 0;
    if (h->hist_live) {
        // a recording series: the step reads the population of row t - 1 and writes row t of the history in place of the ping-pong
        // buffers (no extra traffic), and its ancestors go to row t -- which selects the general instantiation, as the debug flag does
        a.x_in = hist_row(h, t > 0 ? t - 1 : 0); a.x_out = hist_row(h, t);
        a.anc = h->hist_anc + (size_t)t * h->R * h->Npad;
    }
    if (h->split_l2 && t > 0) launch_plan(h, t, gi, true, finalize_prev, record_per_step);
    launch_step(h, a);
    h->cur ^= 1;
}

// whole series in one launch for one-tile filters (pf_small.h); reads buffers `cur`-independent, writes x[1] etc.
// What ssme_pf_run_series launches for an unsharded handle as it is configured now: the ONE place that decides it
// (ssme_pf_run_series, launch_small_m and ssme_pf_get_series_route all ask here).
// Vector user models take the whole-series kernels by default like every other model: measured for (lane | pair kernel) x
// dim_x = 2, 3, 4 at N = 100 .. 2000, the route is 1.6 to 10 us per step faster than the tiled kernel at every shape, against a
// spread of the tiled kernel's own passes of 0.01 to 0.04 us (profiles/vector_series_timing.txt).
struct SeriesRoute { int route, threads, pairs; };   // SSME_ROUTE_*; threads per workgroup; pairs per lane (pair kernel), 0 otherwise
static SeriesRoute series_route(const ssme_pf_s* h) {
    const SeriesRoute tiled = {SSME_ROUTE_TILED, h->nt, 0};
    if (!(h->B == 1 && h->tile == kTile && h->small_series)) return tiled;
    // one particle per lane up to 512 particles (twice the waves, about half the chain per wave: N = 100 3.0 -> 2.2 us per step,
    // N = 500 3.3 -> 3.1); pairs above (N = 1000: 4.6 against 4.9 us; profiles/r02_small_series.txt)
    if (h->N <= 512) return {SSME_ROUTE_SERIES_LANE, h->N <= 64 ? 64 : (h->N <= 128 ? 128 : (h->N <= 256 ? 256 : 512)), 0};
    return {SSME_ROUTE_SERIES_PAIR, 512, h->N <= 1024 ? 1 : 2};
}
// rec: nothing, or the SeriesRec of a recording handle -- the third kernel argument of the recording instantiations (pf_small.h)
template <int MODEL, class... REC>
static void launch_small_m(ssme_pf_handle h, const StepArgs& a, int T, const REC&... rec) {
    const dim3 grid(h->R);
    const SeriesRoute s = series_route(h);
    if (s.route == SSME_ROUTE_SERIES_LANE) {
        if (s.threads == 64) hipLaunchKernelGGL((k_filter_series_lane<MODEL, 64, REC...>), grid, dim3(64), 0, h->stream, a, T, rec...);
        else if (s.threads == 128) hipLaunchKernelGGL((k_filter_series_lane<MODEL, 128, REC...>), grid, dim3(128), 0, h->stream, a, T, rec...);
        else if (s.threads == 256) hipLaunchKernelGGL((k_filter_series_lane<MODEL, 256, REC...>), grid, dim3(256), 0, h->stream, a, T, rec...);
        else hipLaunchKernelGGL((k_filter_series_lane<MODEL, 512, REC...>), grid, dim3(512), 0, h->stream, a, T, rec...);
    } else if (s.pairs == 1) hipLaunchKernelGGL((k_filter_series_small<MODEL, 512, 1, REC...>), grid, dim3(512), 0, h->stream, a, T, rec...);
    else hipLaunchKernelGGL((k_filter_series_small<MODEL, 512, 2, REC...>), grid, dim3(512), 0, h->stream, a, T, rec...);
}
// is the handle recording the expectations of every step (ssme_pf_set_series_expectations)?
static bool recording(const ssme_pf_s* h) { return h->rec_fs.n > 0 || h->rec_user; }
static void enqueue_series_small(ssme_pf_handle h, int T, bool has_z) {
    launch_gamma(h, 0, T);
    h->cur = 0;
    StepArgs a = step_args(h);
    a.z = has_z ? h->zbuf : nullptr;
    a.per_step = h->per_step;
    a.small_ms = h->small_ms;
    if (h->hist.on) {
        SeriesHist hs{};
        hs.fs = h->rec_fs; hs.traj = h->traj; hs.utraj = h->rec_user ? h->utraj : nullptr;
        hs.hx = h->hist_x; hs.hanc = h->hist_anc;
        with_model(h->cfg.model, [&](auto m) { launch_small_m<decltype(m)::value>(h, a, T, hs); });
    } else if (recording(h)) {
        const SeriesRec rec = {h->rec_fs, h->traj, h->rec_user ? h->utraj : nullptr};
        with_model(h->cfg.model, [&](auto m) { launch_small_m<decltype(m)::value>(h, a, T, rec); });
    } else with_model(h->cfg.model, [&](auto m) { launch_small_m<decltype(m)::value>(h, a, T); });
    h->cur = 1;
}

static void drop_graph(ssme_pf_handle h) {
    if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
}

// Gamma tables of the multinomial resampler for T time rows (nothing else moves: the step API grows them on its own)
static int ensure_gamma_capacity(ssme_pf_handle h, int T) {
    if (h->cfg.resampler == SSME_RESAMP_MULTINOMIAL && T > h->gcap) {
        HIPCHK(own_alloc(h, h->gam, sizeof(double) * (size_t)T * h->R * h->B));
        HIPCHK(own_alloc(h, h->pgam, sizeof(double) * (size_t)T * h->R * h->B));
        HIPCHK(own_alloc(h, h->gtot, sizeof(double) * (size_t)T * h->R));
        h->gcap = T;
        drop_graph(h);
    }
    return SSME_OK;
}

static int ensure_series_capacity(ssme_pf_handle h, int T) {
    const bool grow_small = T > h->tcap && h->B == 1;
    bool moved = false;
    int rc = ensure_series_buffers(h, T, h->dy, &moved, h->kz);
    if (rc == SSME_OK) rc = ensure_gamma_capacity(h, T);
    if (rc != SSME_OK) return rc;
    if (grow_small) HIPCHK(own_alloc(h, h->small_ms, sizeof(double) * (size_t)T * h->R * 2));
    if (moved) drop_graph(h);
    return SSME_OK;
}

static int ensure_logw(ssme_pf_handle h) {
    if (logw_needed(h) && !h->logw) HIPCHK(own_alloc(h, h->logw, sizeof(double) * (size_t)h->R * h->Npad, Mem::zeroed));
    return SSME_OK;
}

static int upload_key(ssme_pf_handle h) {
    const uint32_t k[2] = {(uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32)};
    HIPCHK(hipMemcpyAsync(h->keybuf, k, sizeof(k), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // k is a temporary
    return SSME_OK;
}

static int do_reset(ssme_pf_handle h) {
    std::vector<FilterScalars> sc(h->R);
    const double logN = dlog((double)h->N);
    for (auto& s : sc) { std::memset(&s, 0, sizeof(s)); s.prev = logN; }
    HIPCHK(hipMemcpyAsync(h->scal, sc.data(), sizeof(FilterScalars) * h->R, hipMemcpyHostToDevice, h->stream));
    // arrival counters of the in-step accounting and of the one-launch level-2: every launch leaves them at zero; a reset does too
    if (h->ticket) HIPCHK(hipMemsetAsync(h->ticket, 0, sizeof(int32_t) * h->R, h->stream));
    if (h->l2_ticket) HIPCHK(hipMemsetAsync(h->l2_ticket, 0, sizeof(int32_t) * h->R, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // sc is a temporary
    h->t = 0; h->cur = 0;
    h->hist.moved_on(); h->msm.moved_on();                         // the smoothing weights live in the state that is discarded here
    h->gamma_rows = 0;                          // tables are redrawn for the new stream / the new series
    return SSME_OK;
}

// ---- the user model's own functionals (model_api.h: n_h, h; kernels in user_expect.h) -----------------------------------------
// per-filter expectations of all n_h functionals into uexp_out ([n_h][R], device); two launches, no sync
template <class M>
static int enqueue_user_expectations(ssme_pf_handle h) {
    constexpr int NH = user_nh<M>::n;
    if constexpr (NH > 0) {
        if (!h->uexp_part) {
            HIPCHK(own_alloc(h, h->uexp_part, sizeof(double) * (size_t)h->R * h->Bs * NH));
            HIPCHK(own_alloc(h, h->uexp_out, sizeof(double) * (size_t)NH * h->R));
        }
        CovVals<user_cov<M>::k> zc{};
        for (int j = 0; j < user_cov<M>::k; ++j) zc.v[j] = h->last_zv[j];
        hipLaunchKernelGGL(k_user_expect_partials<M>, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, (const double*)h->x[h->cur],
                           (size_t)h->R * h->Npad, (const double*)h->cdf[h->cur], (const ModelConst*)h->mc, h->last_z, zc, h->N, h->Npad, h->Bs,
                           h->tile, h->uexp_part);
        hipLaunchKernelGGL(k_user_expect_final<NH>, dim3(h->R), dim3(kThreads), 0, h->stream, (const double*)h->uexp_part,
                           (const double*)h->tsum[h->cur], (const double*)h->tmax[h->cur], h->B, h->Bs, h->R, h->uexp_out);
        HIPCHK(hipGetLastError());
        return SSME_OK;
    } else {
        return SSME_ERR_UNSUPPORTED;
    }
}

// Recorded series, tiled route: the same two launches behind step `row`, the covariates read from row `row` of zbuf on the device
// (a captured graph is replayed for later series: nothing about the covariates may travel by value), the values into `out`
// ([n_h][R]: slot `row` of the trajectory).  uexp_part exists (ensure_trajectory).
template <class M>
static void enqueue_user_expectations_row(ssme_pf_handle h, int row, bool has_z, double* out) {
    constexpr int NH = user_nh<M>::n;
    if constexpr (NH > 0) {
        hipLaunchKernelGGL(k_user_expect_partials_row<M>, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, (const double*)(h->hist_live ? hist_row(h, row) : h->x[h->cur]),
                           (size_t)h->R * h->Npad, (const double*)h->cdf[h->cur], (const ModelConst*)h->mc,
                           (const double*)(has_z ? h->zbuf : nullptr), row, h->N, h->Npad, h->Bs, h->tile, h->uexp_part);
        hipLaunchKernelGGL(k_user_expect_final<NH>, dim3(h->R), dim3(kThreads), 0, h->stream, (const double*)h->uexp_part,
                           (const double*)h->tsum[h->cur], (const double*)h->tmax[h->cur], h->B, h->Bs, h->R, out);
    }
}

// what both entry points check first; SSME_OK: the expectations are queued on the handle's stream
static int user_expectations_checked(ssme_pf_handle h) {
#if SSME_HAS_USER_MODEL
    if (user_nh<ssme_user_model0>::n == 0 || h->cfg.model != SSME_MODEL_USER0) return SSME_ERR_UNSUPPORTED;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    return enqueue_user_expectations<ssme_user_model0>(h);
#else
    return SSME_ERR_UNSUPPORTED;
#endif
}

// does the compiled-in user model declare its observation draw (model_api.h: gsamp / gsamp_vec)?
#if SSME_HAS_USER_MODEL
constexpr bool kUserHasGsamp = user_gsamp<ssme_user_model0>::has;
constexpr int kUserNH = user_nh<ssme_user_model0>::n;      // functionals the compiled-in header declares
constexpr bool kUserHasLogf = user_logf<ssme_user_model0>::has;     // ... and its transition density (logf / logf_vec)
#else
constexpr bool kUserHasGsamp = false;
constexpr int kUserNH = 0;
constexpr bool kUserHasLogf = false;
#endif

// Recorded series: the trajectory buffers for T time rows of the current recording configuration, and the per-tile numerators of the
// user functionals (the tiled route launches inside a stream capture, where nothing may be allocated).  Recording off: no buffers.
static int ensure_trajectory(ssme_pf_handle h, int T) {
    if (!recording(h)) {
        if (h->traj || h->utraj) { drop_graph(h); own_free(h, h->traj); own_free(h, h->utraj); }
        h->traj_cap = 0; h->traj_n = 0;
        return SSME_OK;
    }
    const bool want_u = h->rec_user != 0;
    if (T > h->traj_cap || h->rec_fs.n != h->traj_n || want_u != (h->utraj != nullptr)) {
        drop_graph(h);
        own_free(h, h->traj); own_free(h, h->utraj);
        h->traj_cap = 0;
        if (h->rec_fs.n > 0) HIPCHK(own_alloc(h, h->traj, sizeof(double) * (size_t)T * h->rec_fs.n * h->R));
        if (want_u) HIPCHK(own_alloc(h, h->utraj, sizeof(double) * (size_t)T * kUserNH * h->R));
        h->traj_cap = T; h->traj_n = h->rec_fs.n;
    }
    if (want_u && !h->uexp_part) {
        HIPCHK(own_alloc(h, h->uexp_part, sizeof(double) * (size_t)h->R * h->Bs * kUserNH));
        HIPCHK(own_alloc(h, h->uexp_out, sizeof(double) * (size_t)kUserNH * h->R));
    }
    return SSME_OK;
}

// Series history: the rows for T steps while the setting is on (a failed allocation leaves none and the handle usable); off: no buffers.
static int ensure_history(ssme_pf_handle h, int T) {
    if (!h->hist.on) {
        if (h->hist_x || h->hist_anc) { drop_graph(h); own_free(h, h->hist_x); own_free(h, h->hist_anc); }
        own_free(h, h->bs_lw); own_free(h, h->ms_rows);
        h->hist.rows_dropped(); h->msm.dropped();
        return SSME_OK;
    }
    if (T <= h->hist.cap) return SSME_OK;
    // the rows are replaced: whatever history they held is no longer in force, whether or not the new allocation succeeds
    drop_graph(h);
    own_free(h, h->hist_x); own_free(h, h->hist_anc); own_free(h, h->bs_lw); own_free(h, h->ms_rows);
    h->hist.rows_dropped(); h->msm.dropped();
    const size_t np = (size_t)h->R * h->Npad;
    hipError_t e = own_alloc(h, h->hist_x, sizeof(double) * (size_t)T * h->dx * np);
    if (e == hipSuccess) e = own_alloc(h, h->hist_anc, sizeof(uint32_t) * (size_t)T * np);
    if (e != hipSuccess) {
        own_free(h, h->hist_x); own_free(h, h->hist_anc);
        (void)hipGetLastError();                       // the refused allocation is reported here, not by the next call's launch check
        h->err = std::string("series history (ssme_pf_series_history_bytes): ") + hipGetErrorString(e);
        return SSME_ERR_HIP;
    }
    h->hist.rows_ready(T);
    return SSME_OK;
}

// the start population of a forecast (forecast.h), every state plane gathered at the ancestor's index (DX = 1: the built-in models),
// and the event of the horizon kernel's start
template <int DX>
static hipError_t launch_fc_start(ssme_pf_handle h, const FcArgs& a) {
    hipLaunchKernelGGL((k_fc_start_vec<DX>), dim3(h->B, h->R), dim3(kFcNT), 0, h->stream, a, (size_t)h->R * h->Npad);
    return hipEventRecord(h->fc.ev[1], h->stream);
}

// the horizon kernel of a forecast, one instantiation per built-in model
template <int MODEL>
static void launch_fc_horizon(ssme_pf_handle h, const FcArgs& a) {
    if constexpr (MODEL != MODEL_USER0)
        hipLaunchKernelGGL((k_fc_horizon<MODEL>), dim3((a.Ns / 2 + kFcNT - 1) / kFcNT, h->R), dim3(kFcNT), 0, h->stream, a);
}

// both kernels of a user model's forecast.  A template, so that a header without the observation draw instantiates neither
template <class M>
static hipError_t launch_fc_user(ssme_pf_handle h, const FcArgs& a) {
    if constexpr (user_gsamp<M>::has) {
        constexpr int DX = user_dims<M>::dx, DY = user_dims<M>::dy;
        const hipError_t e = launch_fc_start<DX>(h, a);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_fc_horizon_user<M, DX, DY>), dim3((a.Ns / 2 + kFcNT - 1) / kFcNT, h->R), dim3(kFcNT), 0, h->stream, a,
                           (size_t)h->R * h->Npad);
    }
    return hipSuccess;
}

extern "C" {

int ssme_pf_version(void) { return 334; }

const char* ssme_pf_strerror(int s) {
    switch (s) {
        case SSME_OK: return "ok";
        case SSME_ERR_INVALID_ARG: return "invalid argument";
        case SSME_ERR_LENGTH: return "length error (empty data)";
        case SSME_ERR_UNSUPPORTED: return "unsupported configuration";
        case SSME_ERR_HIP: return "HIP runtime error";
        case SSME_ERR_STATE: return "invalid call order";
        default: return "unknown status";
    }
}
const char* ssme_pf_last_error(ssme_pf_handle h) { return last_error(h); }

static int create_impl(const ssme_pf_config* cfg, int shard_rank, int shard_world, ssme_pf_handle* out) {
    if (!cfg || !out) return SSME_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->n_particles < 1 || cfg->n_filters < 1 || cfg->n_filters > 65535) return SSME_ERR_INVALID_ARG;
    if (cfg->model == SSME_MODEL_USER0 && !SSME_HAS_USER_MODEL) return SSME_ERR_UNSUPPORTED;   // this library was built without a user model (model_api.h)
    if (cfg->model < 0 || cfg->model > SSME_MODEL_USER0) return SSME_ERR_INVALID_ARG;
    if (cfg->resampler < 0 || cfg->resampler > SSME_RESAMP_MULTINOMIAL_IID) return SSME_ERR_INVALID_ARG;
    if (cfg->resamp_sched < 1) return SSME_ERR_INVALID_ARG;
    if (cfg->dtype != SSME_F64 && cfg->dtype != SSME_F32) return SSME_ERR_INVALID_ARG;
    if (cfg->dtype == SSME_F32 && shard_world > 0) return SSME_ERR_UNSUPPORTED;     // the sharded entry points exchange raw fp64 arrays
    {
        int dx = 1, dy = 1;
        dims_of(cfg->model, &dx, &dy);
        if ((dx > 1 || dy > 1) && (shard_world > 0 || cfg->dtype == SSME_F32)) return SSME_ERR_UNSUPPORTED;   // vector models: unsharded, fp64 boundary
        if (kcov_of(cfg->model) > 0 && shard_world > 0) return SSME_ERR_UNSUPPORTED;                            // dim_cov models: unsharded
    }
    if (cfg->tile_particles != 0 && cfg->tile_particles != kTile && cfg->tile_particles != kTileSmall && cfg->tile_particles != kTileMid) return SSME_ERR_INVALID_ARG;
    if (cfg->n_filters_total < 0 || (cfg->n_filters_total > 0 && cfg->n_filters_total < cfg->n_filters)) return SSME_ERR_INVALID_ARG;
    const int tile = shard_world > 0 ? kTile : (cfg->tile_particles ? cfg->tile_particles
                                                : default_tile(cfg->n_particles, cfg->n_filters_total > 0 ? cfg->n_filters_total : cfg->n_filters));
    ssme_pf_handle h = new (std::nothrow) ssme_pf_s();
    if (!h) return SSME_ERR_INVALID_ARG;
    set_layout(h, cfg->n_particles, cfg->n_filters, tile, shard_rank, shard_world);
    if (h->B > kMaxTilesSplit) { delete h; return SSME_ERR_UNSUPPORTED; }   // at most 16384 tiles per filter (N <= 2^25 with 2048-particle tiles)
    h->cfg = *cfg;
    h->graph_mode = 1;
    h->small_series = 1;
    dims_of(cfg->model, &h->dx, &h->dy);
    h->kcov = kcov_of(cfg->model);
    h->kz = h->kcov > 0 ? h->kcov : 1;
    with_model(cfg->model, [&](auto m) { h->kern = step_kernels<decltype(m)::value>(tile); });
    h->nt = h->kern.nt;
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) { delete h; return SSME_ERR_HIP; }
    {
        int cus = 0;
        h->num_cus = (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) ? cus : 256;
    }
    int rc = [&]() -> int {
        int rc2 = create_stream(h);
        if (rc2 != SSME_OK) return rc2;
        const size_t np = (size_t)h->R * h->Npad, nb = (size_t)h->R * h->Bs;
        if (h->shard_world > 0 && (rc2 = alloc_plan_buffers(h)) != SSME_OK) return rc2;
        for (int i = 0; i < 2 && h->shard_world == 0; ++i) {   // a sharded handle works on the caller's buffers
            HIPCHK(own_alloc(h, h->x[i], sizeof(double) * np * h->dx, Mem::zeroed));          // dim_x planes of [R][Npad]
            HIPCHK(own_alloc(h, h->cdf[i], sizeof(double) * np, Mem::zeroed));
            HIPCHK(own_alloc(h, h->tsum[i], sizeof(double) * nb, Mem::zeroed));
            HIPCHK(own_alloc(h, h->tmax[i], sizeof(double) * nb, Mem::zeroed));
        }
        HIPCHK(grant_step_lds(h));
        HIPCHK(grant_plan_lds(h, cfg->device));
        HIPCHK(own_alloc(h, h->l2_work, sizeof(double) * (nb + (size_t)h->R * kL2Scratch + 32), Mem::zeroed));
        HIPCHK(own_alloc(h, h->l2_T, sizeof(double) * nb));
        HIPCHK(own_alloc(h, h->l2_R, sizeof(double) * nb));
        HIPCHK(own_alloc(h, h->l2_lo, sizeof(int32_t) * nb, Mem::zeroed));
        HIPCHK(own_alloc(h, h->l2_hi, sizeof(int32_t) * nb, Mem::zeroed));
        HIPCHK(own_alloc(h, h->scal, sizeof(FilterScalars) * h->R, Mem::zeroed));     // ssme_pf_get_loglik before set_params: 0, as after a reset
        HIPCHK(own_alloc(h, h->mc, sizeof(ModelConst) * h->R));
        HIPCHK(own_alloc(h, h->scratchR, sizeof(double) * h->R));
        HIPCHK(own_alloc(h, h->exp_part, sizeof(double) * nb * kMaxFunctionals));
        HIPCHK(own_alloc(h, h->exp_out, sizeof(double) * ((size_t)(kMaxFunctionals + 1) * h->R + kMaxFunctionals + 1)));
        HIPCHK(own_alloc(h, h->keybuf, sizeof(uint32_t) * 2));
        HIPCHK(own_alloc(h, h->yz_step, sizeof(double) * 2));
        HIPCHK(own_alloc(h, h->ticket, sizeof(int32_t) * h->R, Mem::zeroed));
        HIPCHK(own_alloc(h, h->l2_ticket, sizeof(int32_t) * h->R, Mem::zeroed));
        HIPCHK(own_alloc(h, h->pin, sizeof(double) * PinLayout::size(h->R), Mem::pinned));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pin_dev), h->pin, 0));
        rc2 = upload_key(h);
        if (rc2 != SSME_OK) return rc2;
        rc2 = ensure_logw(h);                    // sharded, resamp_sched > 1: the carried log-weights of this rank's particles (local offsets)
        if (rc2 != SSME_OK) return rc2;
        return ensure_series_capacity(h, 1);
    }();
    if (rc != SSME_OK) { ssme_pf_destroy(h); return rc; }
    *out = h;
    return SSME_OK;
}

int ssme_pf_destroy(ssme_pf_handle h) {
    if (!h) return SSME_ERR_INVALID_ARG;
    hipSetDevice(h->cfg.device);
    if (h->gexec) { hipStreamSynchronize(h->stream); hipGraphExecDestroy(h->gexec); }
    for (hipEvent_t& e : h->sm_ev) if (e) hipEventDestroy(e);
    release_core(h);
    delete h;
    return SSME_OK;
}

int ssme_pf_create(const ssme_pf_config* cfg, ssme_pf_handle* out) { return create_impl(cfg, 0, 0, out); }
int ssme_pf_user_model_n_theta(void) {
#if SSME_HAS_USER_MODEL
    return ssme_user_model0::n_theta;
#else
    return 0;
#endif
}
int ssme_pf_user_model_dims(int32_t* dim_x, int32_t* dim_y) {
    if (!dim_x || !dim_y) return SSME_ERR_INVALID_ARG;
#if SSME_HAS_USER_MODEL
    int dx = 1, dy = 1;
    dims_of(SSME_MODEL_USER0, &dx, &dy);
    *dim_x = dx; *dim_y = dy;
    return SSME_OK;
#else
    *dim_x = 0; *dim_y = 0;
    return SSME_ERR_UNSUPPORTED;
#endif
}
int ssme_pf_user_model_n_h(void) {
#if SSME_HAS_USER_MODEL
    return user_nh<ssme_user_model0>::n;
#else
    return 0;
#endif
}
int ssme_pf_user_model_has_gsamp(void) { return kUserHasGsamp ? 1 : 0; }
int ssme_pf_user_model_has_logf(void) { return kUserHasLogf ? 1 : 0; }
int ssme_pf_user_model_dim_cov(void) { return kcov_of(SSME_MODEL_USER0); }
int ssme_pf_user_model_has_first(void) {
#if SSME_HAS_USER_MODEL
    return user_first<ssme_user_model0>::has ? 1 : 0;
#else
    return 0;
#endif
}
int ssme_pf_default_tile(int32_t n_particles, int32_t bank_filters) { return default_tile(n_particles, bank_filters < 1 ? 1 : bank_filters); }

// ---- particle-sharded filter: one filter of cfg->n_particles particles over `world` GPUs ------------------------------
//   This handle owns rank `rank`'s share: B/world consecutive tiles.  Particle buffers
// are the caller's (device pointers), so that the host side can hand the same memory to its collective library.
int ssme_pf_shard_create(const ssme_pf_config* cfg, int32_t rank, int32_t world, ssme_pf_handle* out) {
    if (!cfg || !out) return SSME_ERR_INVALID_ARG;
    const int rc = shard_create_check(cfg->n_particles, cfg->n_filters, rank, world);
    if (rc != SSME_OK) return rc;
    if (cfg->resamp_sched < 1) return SSME_ERR_UNSUPPORTED;
    return create_impl(cfg, rank, world, out);
}

int ssme_pf_shard_layout(ssme_pf_handle h, int32_t* out4) { return shard_layout(h, out4); }

int ssme_pf_set_stream(ssme_pf_handle h, void* hip_stream) {
    const int rc = set_stream(h, hip_stream);
    if (rc == SSME_OK) drop_graph(h);
    return rc;
}

int ssme_pf_shard_prepare(ssme_pf_handle h, const double* y, const double* z, int32_t T) {
    if (!h || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1 || !h->params_set) return SSME_ERR_STATE;
    if (T < 1) return SSME_ERR_LENGTH;
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = ensure_series_capacity(h, T);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->ybuf, y, sizeof(double) * T * h->dy, hipMemcpyHostToDevice, h->stream));
    if (z) HIPCHK(hipMemcpyAsync(h->zbuf, z, sizeof(double) * T * h->kz, hipMemcpyHostToDevice, h->stream));
    h->g_has_z = z != nullptr;
    rc = do_reset(h);
    if (rc != SSME_OK) return rc;
    launch_gamma(h, 0, T);                       // global tables: every rank holds all B tiles' draws
    HIPCHK(hipGetLastError());
    return SSME_OK;
}

static StepArgs shard_args(ssme_pf_handle h, int t, const double* tsum_all, const double* tmax_all) {
    StepArgs a = step_args(h);
    a.tsum_in = tsum_all; a.tmax_in = tmax_all;
    a.z = h->g_has_z ? h->zbuf : nullptr;
    a.per_step = h->per_step;
    a.t = t; a.yi = t; a.gi = t;
    a.logw = h->cfg.resamp_sched > 1 ? h->logw : nullptr;      // steps without resampling carry the log-weights (this rank's own, local offsets)
    a.anc = nullptr;
    return a;
}

// the plan of step t on the device: every rank's window into h->plan_dev (up to 1024 tiles) or every tile's range into
// l2_lo / l2_hi (split level-2, which also accounts log p(y_{t-1} | .))
static void shard_plan_device(ssme_pf_handle h, int t, const double* tsum_all, const double* tmax_all, int margin = 0,
                              int32_t* flag = nullptr) {
    StepArgs a = shard_args(h, t, tsum_all, tmax_all);
    if (h->split_l2) {
        a.finalize_prev = 1;
        launch_level2(h->stream, a, 1, h->lds_bytes_plan, 1);
        if (flag) hipLaunchKernelGGL(k_shard_window_check, dim3(1), dim3(64), 0, h->stream, (const int32_t*)nullptr, (const int32_t*)h->l2_lo,
                                     (const int32_t*)h->l2_hi, h->shard_world, h->sh_Bl, h->B, margin, flag, flag + 1);
    } else {
        hipLaunchKernelGGL(k_shard_plan, dim3(1), dim3(512), sizeof(double) * (h->Bpow2 < 2 ? 2 : h->Bpow2), h->stream, a,
                           h->shard_world, h->sh_Bl, h->plan_dev, margin, flag);
    }
}

int ssme_pf_shard_plan(ssme_pf_handle h, const double* tsum_all, const double* tmax_all, int32_t t, int32_t* lo_hi) {
    if (!h || !tsum_all || !tmax_all || !lo_hi || t < 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    shard_plan_device(h, t, tsum_all, tmax_all);
    HIPCHK(hipGetLastError());
    return shard_plan_to_host(h, h->split_l2 && h->cfg.resampler == SSME_RESAMP_MULTINOMIAL_IID, h->l2_lo, h->l2_hi, lo_hi);
}

// Step t of this rank's tiles: sources in the window that starts at global tile win_tile0, outputs in the caller's buffers.
// check_halo (the native driver's fixed-halo path): the window is the whole halo buffer, and a step that resamples verifies its
// source tiles against it (StepArgs::win_tiles / win_flag).
static int shard_launch_step(ssme_pf_handle h, int t, const double* x_win, const double* cdf_win, int win_tile0, const double* tsum_all,
                             const double* tmax_all, double* x_out, double* cdf_out, double* tsum_out, double* tmax_out, uint32_t* anc_out,
                             bool check_halo) {
    StepArgs a = shard_args(h, t, tsum_all, tmax_all);
    a.x_in = x_win; a.cdf_in = cdf_win; a.win_tile0 = win_tile0;
    if (check_halo && (t % h->cfg.resamp_sched) == 0) { a.win_tiles = h->sh_rows; a.win_flag = h->sh_flag; }
    a.x_out = x_out; a.cdf_out = cdf_out; a.tsum_out = tsum_out; a.tmax_out = tmax_out;
    a.anc = anc_out;
    a.finalize_prev = t > 0 ? 1 : 0;
    a.tile0 = h->shard_rank * h->sh_Bl;
    launch_step_on(h, a, dim3(h->sh_Bown, 1));
    HIPCHK(hipGetLastError());
    h->t = t + 1;
    return SSME_OK;
}

int ssme_pf_shard_step(ssme_pf_handle h, int32_t t, const double* x_win, const double* cdf_win, int32_t win_tile0,
                       const double* tsum_all, const double* tmax_all, double* x_out, double* cdf_out, double* tsum_out,
                       double* tmax_out, uint32_t* anc_out) {
    if (!h || !x_out || !cdf_out || !tsum_out || !tmax_out || t < 0) return SSME_ERR_INVALID_ARG;
    // win_tile0 may be negative on the C++ driver's fixed-halo path: rank 0's halo buffer starts `margin` (never-read) rows before tile 0
    // (on a step without resampling -- t % resamp_sched != 0 -- x_win is this rank's OWN particles of step t - 1, stored as the
    //  outputs are: the kernel reads them in place, cdf_win is not read)
    if (t > 0 && (!x_win || !cdf_win || !tsum_all || !tmax_all || win_tile0 < -h->sh_margin)) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1 || !h->params_set) return SSME_ERR_STATE;
    if (t >= h->tcap) return SSME_ERR_STATE;            // ssme_pf_shard_prepare sizes the series
    HIPCHK(hipSetDevice(h->cfg.device));
    return shard_launch_step(h, t, x_win, cdf_win, win_tile0, tsum_all, tmax_all, x_out, cdf_out, tsum_out, tmax_out, anc_out, false);
}

int ssme_pf_shard_finalize(ssme_pf_handle h, int32_t t, const double* tsum_all, const double* tmax_all) {
    if (!h || !tsum_all || !tmax_all || t < 0) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    StepArgs a = shard_args(h, t, tsum_all, tmax_all);
    if (h->split_l2) {
        a.t = t + 1; a.finalize_prev = 1;
        launch_level2(h->stream, a, 1, h->lds_bytes_plan, 0);
    } else
        hipLaunchKernelGGL(kf_finalize, dim3(1), dim3(kThreads), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return SSME_OK;
}

// ---- C++ driver of the sharded filter over RCCL (shard_driver.h) ----------------------------------------------------------

int ssme_shard_comm_get_unique_id(void* id128) {
    HandleCore* h = nullptr;
    if (!id128) return SSME_ERR_INVALID_ARG;
    if (!rccl().ok) return SSME_ERR_UNSUPPORTED;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    NCCLCHK(rccl().GetUniqueId(reinterpret_cast<ncclUniqueId*>(id128)));
    return SSME_OK;
}
int ssme_shard_comm_init(const void* id128, int32_t rank, int32_t world, int32_t device, void** comm_out) {
    HandleCore* h = nullptr;
    if (!id128 || !comm_out || world < 1 || rank < 0 || rank >= world) return SSME_ERR_INVALID_ARG;
    if (!rccl().ok) return SSME_ERR_UNSUPPORTED;
    if (hipSetDevice(device) != hipSuccess) return SSME_ERR_HIP;
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    NCCLCHK(rccl().CommInitRank(&c, world, id, rank));
    *comm_out = c;
    return SSME_OK;
}
int ssme_shard_comm_destroy(void* comm) {
    HandleCore* h = nullptr;
    if (!comm) return SSME_ERR_INVALID_ARG;
    if (!rccl().ok) return SSME_ERR_UNSUPPORTED;
    NCCLCHK(rccl().CommDestroy(reinterpret_cast<ncclComm_t>(comm)));
    return SSME_OK;
}

static int shard_alloc(ssme_pf_handle h, bool exact) {
    const int Bl = h->sh_Bl;
    if (!h->sh_x[0]) {
        h->sh_margin = halo_margin(Bl, h->shard_world); h->sh_rows = Bl + 2 * h->sh_margin;
        const size_t nb = sizeof(double) * (size_t)h->sh_rows * kTile;
        for (int i = 0; i < 2; ++i) {
            HIPCHK(own_alloc(h, h->sh_x[i], nb, Mem::zeroed));
            HIPCHK(own_alloc(h, h->sh_c[i], nb, Mem::zeroed));
        }
        HIPCHK(own_alloc(h, h->sh_loc, sizeof(double) * 2 * Bl, Mem::zeroed));
        HIPCHK(own_alloc(h, h->sh_tsum, sizeof(double) * gathered_len(h)));
        HIPCHK(own_alloc(h, h->sh_tmax, sizeof(double) * gathered_len(h)));
        HIPCHK(own_alloc(h, h->sh_flag, sizeof(int32_t) * 4));
    }
    if (exact && !h->sh_winx) {
        HIPCHK(own_alloc(h, h->sh_winx, sizeof(double) * (size_t)h->B * kTile));
        HIPCHK(own_alloc(h, h->sh_winc, sizeof(double) * (size_t)h->B * kTile));
    }
    return SSME_OK;
}

// One series on one path.  fast: fixed halo exchange, no host synchronisation inside the loop; exact: planned exchange.
static int shard_series(ssme_pf_handle h, void* nccl_comm, const double* y, const double* z, int T, bool fast, bool* overflow) {
    const int rank = h->shard_rank, Bl = h->sh_Bl, m = h->sh_margin, tile0 = rank * Bl;
    const size_t TL = kTile;
    ncclComm_t comm;
    int rc = native_begin(h, nccl_comm, &comm);
    if (rc == SSME_OK) rc = ssme_pf_shard_prepare(h, y, z, T);
    if (rc != SSME_OK) return rc;
    int cur = 0;
    std::vector<int32_t> lo_hi(2 * (size_t)h->shard_world);
    // tile sums and tile maxima of all ranks, each straight into its final [B] array
    auto gather = [&] { return all_gather(h, comm, {{h->sh_loc, h->sh_tsum, (size_t)Bl}, {h->sh_loc + Bl, h->sh_tmax, (size_t)Bl}}); };
    for (int t = 0; t < T; ++t) {
        double* xs = h->sh_x[cur]; double* cs = h->sh_c[cur];                     // sources: own rows + halos
        double* xo = h->sh_x[cur ^ 1] + (size_t)m * TL; double* co = h->sh_c[cur ^ 1] + (size_t)m * TL;   // outputs: the own rows of the other pair
        const double *xw = nullptr, *cw = nullptr;
        int win0 = 0;
        const bool resampled = t > 0 && (t % h->cfg.resamp_sched) == 0;     // the draw that closes step t - 1 runs now (lazily)
        if (t > 0) {
            rc = gather();
            if (rc != SSME_OK) return rc;
            if (!resampled) {
                // no draw: every particle continues itself with its carried log-weight -- sources = this rank's own tiles, no exchange;
                // the gathered tile sums still give every rank the step's log p(y_{t-1} | .)
                if (h->split_l2) { shard_plan_device(h, t, h->sh_tsum, h->sh_tmax); HIPCHK(hipGetLastError()); }
                xw = xs + (size_t)m * TL; cw = cs + (size_t)m * TL; win0 = tile0;
            } else if (fast) {
                // up to 1024 tiles the step kernel runs level-2 itself and checks its own source tiles against the fixed
                // halo (StepArgs::win_flag): no plan launch at all; above, k_level2_plan is needed anyway and a small check follows it
                if (h->split_l2) {
                    shard_plan_device(h, t, h->sh_tsum, h->sh_tmax, m, h->sh_flag);
                    HIPCHK(hipGetLastError());
                }
                rc = halo_exchange(h, comm, {{xs, TL}, {cs, TL}});
                if (rc != SSME_OK) return rc;
                xw = xs; cw = cs; win0 = tile0 - m;                                   // row 0 of the halo buffer is global tile tile0 - m
            } else {
                rc = ssme_pf_shard_plan(h, h->sh_tsum, h->sh_tmax, t, lo_hi.data());   // synchronises: the exact path is host-planned
                if (rc == SSME_OK) rc = planned_exchange(h, comm, lo_hi.data(), {{xs + (size_t)m * TL, h->sh_winx, TL}, {cs + (size_t)m * TL, h->sh_winc, TL}});
                if (rc != SSME_OK) return rc;
                xw = h->sh_winx; cw = h->sh_winc; win0 = lo_hi[2 * rank];
            }
        }
        rc = shard_launch_step(h, t, xw, cw, win0, h->sh_tsum, h->sh_tmax, xo, co, h->sh_loc, h->sh_loc + Bl, nullptr,
                               /*check_halo=*/fast && t > 0);
        if (rc != SSME_OK) return rc;
        cur ^= 1;
    }
    rc = gather();
    if (rc != SSME_OK) return rc;
    rc = ssme_pf_shard_finalize(h, T - 1, h->sh_tsum, h->sh_tmax);                    // synchronises
    if (rc != SSME_OK) return rc;
    h->cur = cur;                                                                     // sh_x[cur] holds the final particles
    *overflow = false;
    // (the exact path has no halo to leave; sh_stats keeps the record of the fixed-halo pass it may be the rerun of)
    return fast ? reduce_flags(h, comm, overflow) : SSME_OK;
}

int ssme_pf_shard_run_series(ssme_pf_handle h, void* nccl_comm, const double* y, const double* z, int32_t T, int32_t mode, double* loglik_out) {
    if (!h || !nccl_comm || !y || mode < 0 || mode > 2) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1 || !h->params_set) return SSME_ERR_STATE;
    if (T < 1) return SSME_ERR_LENGTH;
    if (h->cfg.resampler == SSME_RESAMP_MULTINOMIAL_IID && mode == 1) return SSME_ERR_UNSUPPORTED;      // unsorted targets need every tile
    HIPCHK(hipSetDevice(h->cfg.device));
    const bool want_fast = mode != 2 && h->cfg.resampler != SSME_RESAMP_MULTINOMIAL_IID;
    int rc = shard_alloc(h, !want_fast);
    if (rc != SSME_OK) return rc;
    bool overflow = false;
    std::memset(h->sh_stats, 0, sizeof(h->sh_stats));
    h->sh_path = want_fast ? 1 : 2;
    rc = shard_series(h, nccl_comm, y, z, T, want_fast, &overflow);
    if (rc != SSME_OK) return rc;
    if (overflow) {
        // a window left the fixed halo on SOME rank (the reduced flag: every rank reads the same value and takes the same branch):
        // mode 1 reports it, mode 0 runs the series again on the exact path
        if (mode == 1) { h->err = "a resampling window left the fixed halo"; return SSME_ERR_STATE; }
        rc = shard_alloc(h, true);
        if (rc != SSME_OK) return rc;
        h->sh_path = 2;
        rc = shard_series(h, nccl_comm, y, z, T, false, &overflow);
        if (rc != SSME_OK) return rc;
    }
    if (loglik_out) return ssme_pf_get_loglik(h, loglik_out);
    return SSME_OK;
}

// this rank's particles and integer cdf after the last native series (N / world values each); path / statistics
int ssme_pf_shard_download(ssme_pf_handle h, double* x_local, uint64_t* cdf_local, int32_t* path, int64_t* exchanged_tiles) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1 || !h->sh_x[0]) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t off = (size_t)h->sh_margin * kTile, n = own_particles(h);
    if (x_local) HIPCHK(hipMemcpy(x_local, h->sh_x[h->cur] + off, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (cdf_local) {
        HIPCHK(hipMemcpy(cdf_local, h->sh_c[h->cur] + off, sizeof(double) * n, hipMemcpyDeviceToHost));
        double dv;
        for (size_t i = 0; i < n; ++i) { std::memcpy(&dv, &cdf_local[i], 8); cdf_local[i] = (uint64_t)dv; }
    }
    if (path) *path = h->sh_path;
    if (exchanged_tiles) *exchanged_tiles = h->sh_exchanged;
    return SSME_OK;
}

int ssme_pf_shard_stats(ssme_pf_handle h, int32_t* out4) { return shard_stats(h, h && h->sh_x[0], out4); }

int ssme_pf_set_params(ssme_pf_handle h, const double* theta, int32_t n_theta, int32_t n_rows) {
    if (!h || !theta) return SSME_ERR_INVALID_ARG;
    if (n_theta != n_theta_of(h->cfg.model)) return SSME_ERR_INVALID_ARG;
    if (n_rows != 1 && n_rows != h->R) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    h->h_mc.resize(h->R);
    h->h_gscale.assign(h->R, 1.0);
    for (int r = 0; r < h->R; ++r) {
        double th[8];
        for (int d = 0; d < n_theta; ++d) {
            const double v = theta[(size_t)(n_rows == 1 ? 0 : r) * n_theta + d];
            th[d] = h->cfg.dtype == SSME_F32 ? f32r(v) : v;
        }
        h->h_mc[r] = derive(h->cfg.model, th);
        if (h->cfg.model == SSME_MODEL_SVOL) h->h_gscale[r] = th[0];            // beta
        else if (h->cfg.model == SSME_MODEL_LIN_GAUSS) h->h_gscale[r] = th[2];  // tau
    }
    HIPCHK(hipMemcpyAsync(h->mc, h->h_mc.data(), sizeof(ModelConst) * h->R, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->params_set = true;
    return do_reset(h);
}

// New random stream for the next evaluation (PMMH draws a fresh likelihood estimate per proposal; the reference
// seeds every model object from the clock).  The key lives in device memory: a captured graph stays valid.
int ssme_pf_set_seed(ssme_pf_handle h, uint64_t seed) {
    if (!h) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    h->cfg.seed = seed;
    int rc = upload_key(h);
    if (rc != SSME_OK) return rc;
    return h->params_set ? do_reset(h) : SSME_OK;
}

int ssme_pf_reset(ssme_pf_handle h) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (!h->params_set) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    return do_reset(h);
}

// flags: bit 0 = record ancestor indices, bit 1 = keep the log-weights in memory, bits 2-4 = level-2 policy (below)
int ssme_pf_set_debug(ssme_pf_handle h, int32_t flags) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    if ((flags & 1) && !h->anc) HIPCHK(own_alloc(h, h->anc, sizeof(uint32_t) * (size_t)h->R * h->Npad, Mem::zeroed));
    h->debug_anc = (flags & 1) ? 1 : 0;
    h->keep_logw = (flags & 2) ? 1 : 0;
    {
        // bit 2 forces the split level-2, bit 3 the in-kernel one (where it exists: <= 2048 tiles); default by size.
        // bit 4: the split level-2 by the table kernels (two launches above 1024 tiles) instead of one launch + ranges in the step kernel
        const int want = (h->B > kMaxTilesPerFilter || (flags & 4)) ? 1 : ((flags & 8) ? 0 : (h->B > kSplitLevel2Above ? 1 : 0));
        const int tables = (flags & 16) ? 1 : 0;
        if ((want != h->split_l2 || tables != h->l2_tables) && h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
        h->split_l2 = want;
        h->l2_tables = tables;
    }
    return ensure_logw(h);
}

int ssme_pf_set_tuning(ssme_pf_handle h, int32_t threads_per_tile) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (threads_per_tile != 256 && threads_per_tile != 512 && threads_per_tile != 1024) return SSME_ERR_INVALID_ARG;
    if (h->tile == kTileSmall && threads_per_tile != 256) return SSME_ERR_UNSUPPORTED;     // 512-particle tiles run 256 threads
    if (h->tile == kTileMid && threads_per_tile != 512) return SSME_ERR_UNSUPPORTED;       // 1024-particle tiles run 512 threads
    h->nt = threads_per_tile;
    return SSME_OK;
}

int ssme_pf_set_small_series(ssme_pf_handle h, int32_t enable) {
    if (!h || enable < 0 || enable > 1) return SSME_ERR_INVALID_ARG;
    h->small_series = enable;
    return SSME_OK;
}

int ssme_pf_get_series_route(ssme_pf_handle h, int32_t* route, int32_t* threads_per_block) {
    if (!h || !route || !threads_per_block) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles are driven by ssme_pf_shard_*
    const SeriesRoute s = series_route(h);
    *route = s.route;
    *threads_per_block = s.threads;
    return SSME_OK;
}

int ssme_pf_set_graph_mode(ssme_pf_handle h, int32_t mode) {
    if (!h || mode < 0 || mode > 1) return SSME_ERR_INVALID_ARG;
    h->graph_mode = mode;
    return SSME_OK;
}

int ssme_pf_step(ssme_pf_handle h, const double* y, const double* z, double* out) {
    if (!h || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles are driven by ssme_pf_shard_*
    if (!h->params_set) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->cfg.resampler == SSME_RESAMP_MULTINOMIAL && h->gcap < kStepGammaChunk) {
        int rc = ensure_gamma_capacity(h, kStepGammaChunk);
        if (rc != SSME_OK) return rc;
    }
    // y and z travel in the kernel arguments; the R results come back through device-mapped pinned memory, written by the
    // last workgroup of the step kernel itself: a filter() call is one launch and a poll (two launches with the split
    // level-2 of very large filters), no copy operation in either direction
    double* const yz = h->pin + PinLayout::yz;
    yz[0] = *y; yz[1] = z ? *z : 0.0;
    for (int d = 1; d < h->dy; ++d) h->y_step_v[d - 1] = y[d];
    for (int j = 1; j < h->kcov; ++j) h->z_step_v[j - 1] = z ? z[j] : 0.0;
    if (h->cfg.dtype == SSME_F32) {
        yz[0] = f32r(yz[0]); yz[1] = f32r(yz[1]);
        for (int j = 1; j < h->kcov; ++j) h->z_step_v[j - 1] = f32r(h->z_step_v[j - 1]);
    }
    h->last_z = yz[1];
    h->last_zv[0] = yz[1];
    for (int j = 1; j < kMaxCov; ++j) h->last_zv[j] = j < h->kcov ? h->z_step_v[j - 1] : 0.0;
    const int gi = h->cfg.resampler == SSME_RESAMP_MULTINOMIAL ? step_gamma_row(h, launch_gamma) : 0;
    // out == NULL (the swarm classes: the aggregation that follows hands the data back): the step is only queued -- no result
    // slots, no wait; anything that reads the handle afterwards is ordered behind it on the stream
    const bool want = out != nullptr;
    double* const res = h->pin + PinLayout::results;
    if (want) mark_results_pending(res, h->R);
    enqueue_step(h, h->t, 0, gi, z != nullptr, /*finalize_prev=*/false, /*per_step=*/false, /*from_step_staging=*/true, want);
    if (h->split_l2) launch_kf(h, h->t, false, want ? h->pin_dev + PinLayout::results : nullptr);
    HIPCHK(hipGetLastError());
    h->t += 1;
    h->hist.moved_on(); h->msm.moved_on();                                // the final weights of the recorded series are gone
    if (want) HIPCHK(wait_results(h->stream, res, h->R));
    if (out) for (int r = 0; r < h->R; ++r) out[r] = res[r];
    round_out(h, out, h->R);
    return SSME_OK;
}

// the covariates of row T - 1 of a series (kz per row; null: zeros) are what the user model's functionals receive afterwards
static void set_last_z(ssme_pf_handle h, const double* z, int T) {
    for (int j = 0; j < kMaxCov; ++j) h->last_zv[j] = (z && j < h->kz) ? z[(size_t)(T - 1) * h->kz + j] : 0.0;
    h->last_z = h->last_zv[0];
}

// Recorded series, tiled route: behind step t the partial and final expectation kernels of the step API, writing slot t of the
// trajectories instead of exp_out / uexp_out.  They read the buffers the step wrote (now `cur`), as after ssme_pf_step.
// the particles step t of the series being queued wrote: the ping-pong buffer, or row t of the history
static const double* series_x(const ssme_pf_s* h, int t) { return h->hist_live ? hist_row(h, t) : h->x[h->cur]; }
static void enqueue_step_expectations(ssme_pf_handle h, int t, bool has_z) {
    if (h->rec_fs.n > 0) {
        hipLaunchKernelGGL(k_expect_partials, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, series_x(h, t), h->cdf[h->cur], h->N,
                           h->Npad, h->Bs, h->tile, h->rec_fs, h->exp_part);
        hipLaunchKernelGGL(k_expect_final, dim3(h->R), dim3(kThreads), 0, h->stream, h->exp_part, h->tsum[h->cur], h->tmax[h->cur],
                           h->B, h->Bs, h->R, h->rec_fs, h->traj + (size_t)t * h->rec_fs.n * h->R);
    }
#if SSME_HAS_USER_MODEL
    if (h->rec_user) enqueue_user_expectations_row<ssme_user_model0>(h, t, has_z, h->utraj + (size_t)t * kUserNH * h->R);
#endif
}

static hipError_t enqueue_series(ssme_pf_handle h, int T, bool has_z) {
    launch_gamma(h, 0, T);
    const bool rec = recording(h);
    h->hist_live = h->hist.on;
    for (int t = 0; t < T; ++t) {
        enqueue_step(h, t, t, t, has_z, /*finalize_prev=*/t > 0, /*per_step=*/true);
        if (rec) enqueue_step_expectations(h, t, has_z);
    }
    launch_kf(h, T - 1, true);
    hipError_t e = hipSuccess;
    if (h->hist_live) {
        // the final population where every later call looks for it, and the debug ancestors as a non-recording run leaves them: the
        // indices of the LAST DRAW, i.e. of the last step that resampled (a step that did not wrote no row; no draw at all: untouched)
        const size_t np = (size_t)h->R * h->Npad;
        const int t_draw = ((T - 1) / h->cfg.resamp_sched) * h->cfg.resamp_sched;
        e = hipMemcpyAsync(h->x[h->cur], hist_row(h, T - 1), sizeof(double) * np * h->dx, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess && h->debug_anc && t_draw >= 1)
            e = hipMemcpyAsync(h->anc, h->hist_anc + (size_t)t_draw * np, sizeof(uint32_t) * np, hipMemcpyDeviceToDevice, h->stream);
    }
    h->hist_live = 0;
    return e;
}

int ssme_pf_run_series(ssme_pf_handle h, const double* y, const double* z, int32_t T, double* loglik_out) {
    if (!h || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles are driven by ssme_pf_shard_*
    if (T < 1) return SSME_ERR_LENGTH;
    if (!h->params_set) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    h->rec_T = 0;                                      // rows are valid once the series is queued; a failure below leaves none
    h->hist.moved_on(); h->msm.moved_on();                                // ... and no history in force: the one of an earlier series ends here
    int rc = ensure_series_capacity(h, T);
    if (rc == SSME_OK) rc = ensure_trajectory(h, T);
    if (rc == SSME_OK) rc = ensure_history(h, T);
    if (rc != SSME_OK) return rc;
    std::vector<double> y32, z32;
    if (h->cfg.dtype == SSME_F32) {
        y32.resize(T);
        for (int t = 0; t < T; ++t) y32[t] = f32r(y[t]);
        y = y32.data();
        if (z) { z32.resize((size_t)T * h->kz); for (size_t i = 0; i < z32.size(); ++i) z32[i] = f32r(z[i]); z = z32.data(); }
    }
    HIPCHK(hipMemcpyAsync(h->ybuf, y, sizeof(double) * T * h->dy, hipMemcpyHostToDevice, h->stream));
    if (z) HIPCHK(hipMemcpyAsync(h->zbuf, z, sizeof(double) * T * h->kz, hipMemcpyHostToDevice, h->stream));
    set_last_z(h, z, T);
    h->hist_has_z = z != nullptr;
    if (h->cfg.dtype == SSME_F32) HIPCHK(hipStreamSynchronize(h->stream));      // the staging vectors go out of scope
    rc = do_reset(h);
    if (rc != SSME_OK) return rc;
    const bool has_z = z != nullptr;
    const int lw = logw_needed(h) ? 1 : 0;
    if (series_route(h).route != SSME_ROUTE_TILED) {
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        enqueue_series_small(h, T, has_z);
        HIPCHK(hipEventRecord(h->ev1, h->stream));
    } else if (h->graph_mode) {
        if (!h->gexec || h->g_T != T || h->g_has_z != (int)has_z || h->g_debug != h->debug_anc || h->g_logw != lw ||
            h->g_nt != h->nt || h->g_hist != h->hist.on || h->g_rec_user != h->rec_user || std::memcmp(&h->g_rec_fs, &h->rec_fs, sizeof(FunctionalIds)) != 0) {
            if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            h->cur = 0;
            const hipError_t queued = enqueue_series(h, T, has_z);
            HIPCHK(hipStreamEndCapture(h->stream, &g));
            if (queued != hipSuccess) { hipGraphDestroy(g); return fail(h, "enqueue_series (capture)", queued); }
            HIPCHK(hipGraphInstantiate(&h->gexec, g, nullptr, nullptr, 0));
            HIPCHK(hipGraphDestroy(g));
            h->g_T = T; h->g_has_z = has_z; h->g_debug = h->debug_anc; h->g_logw = lw; h->g_nt = h->nt;
            h->g_rec_fs = h->rec_fs; h->g_rec_user = h->rec_user; h->g_hist = h->hist.on;
        }
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        HIPCHK(hipGraphLaunch(h->gexec, h->stream));
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        h->cur = (T & 1);
    } else {
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        h->cur = 0;
        HIPCHK(enqueue_series(h, T, has_z));
        HIPCHK(hipEventRecord(h->ev1, h->stream));
    }
    HIPCHK(hipGetLastError());
    h->t = T;
    h->rec_T = recording(h) ? T : 0; h->rec_n = h->rec_fs.n; h->rec_nh = h->rec_user ? kUserNH : 0;
    rc = read_loglik(h, loglik_out);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    h->hist.recorded(T); h->msm.moved_on();                               // in force until the handle moves on (run_series, do_reset, ssme_pf_step)
    round_out(h, loglik_out, h->R);
    return SSME_OK;
}

// ---- recorded series: the expectations of every step of ssme_pf_run_series (kernels: pf_small.h, enqueue_step_expectations) ----
int ssme_pf_set_series_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n, int32_t user) {
    if (!h || n < 0 || n > kMaxFunctionals || (n > 0 && !functionals)) return SSME_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        if (functionals[i] < SSME_H_X || functionals[i] > SSME_H_CONST42) return SSME_ERR_INVALID_ARG;
    if (user && (h->cfg.model != SSME_MODEL_USER0 || kUserNH == 0)) return SSME_ERR_UNSUPPORTED;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    FunctionalIds fs{};
    fs.n = n;
    for (int i = 0; i < n; ++i) fs.id[i] = functionals[i];
    h->rec_fs = fs;
    h->rec_user = user ? 1 : 0;
    // a cached graph of another recording configuration is not replayed (the cache key of ssme_pf_run_series holds both); the
    // trajectory buffers follow at the next run_series (ensure_trajectory), which also frees them once recording is off
    if (h->gexec && (h->g_rec_user != h->rec_user || std::memcmp(&h->g_rec_fs, &h->rec_fs, sizeof(FunctionalIds)) != 0)) {
        HIPCHK(hipSetDevice(h->cfg.device));
        HIPCHK(hipStreamSynchronize(h->stream));
        drop_graph(h);
    }
    return SSME_OK;
}

// rows 0 .. T-1 of a trajectory of `n` functionals per row ([rows][n][R] on the device), rounded for SSME_F32 handles
static int read_trajectory(ssme_pf_handle h, const double* dev, int n, double* out, int T) {
    if (!h || !out || T < 1) return SSME_ERR_INVALID_ARG;
    if (h->rec_T < 1 || n < 1 || !dev) return SSME_ERR_STATE;
    if (T > h->rec_T) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t cnt = (size_t)T * n * h->R;
    HIPCHK(hipMemcpyAsync(out, dev, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    round_out(h, out, cnt);
    return SSME_OK;
}
int ssme_pf_get_series_expectations(ssme_pf_handle h, double* out, int32_t T) {
    return read_trajectory(h, h ? h->traj : nullptr, h ? h->rec_n : 0, out, T);
}
int ssme_pf_get_series_user_expectations(ssme_pf_handle h, double* out, int32_t T) {
    return read_trajectory(h, h ? h->utraj : nullptr, h ? h->rec_nh : 0, out, T);
}

// ---- series history and smoothing (kernels: smooth.h; recording: enqueue_step, enqueue_series_small) ----
int ssme_pf_set_series_history(ssme_pf_handle h, int32_t enable) {
    if (!h || enable < 0 || enable > 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    h->hist.on = enable;
    // a cached graph of the other configuration is not replayed (the cache key of ssme_pf_run_series holds the setting); the history
    // rows follow at the next run_series (ensure_history), which also frees them once the setting is off
    if (h->gexec && h->g_hist != h->hist.on) {
        HIPCHK(hipSetDevice(h->cfg.device));
        HIPCHK(hipStreamSynchronize(h->stream));
        drop_graph(h);
    }
    return SSME_OK;
}

int ssme_pf_series_history_bytes(ssme_pf_handle h, int32_t T, uint64_t* bytes) {
    if (!h || !bytes || T < 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    *bytes = (uint64_t)T * (uint64_t)h->R * (uint64_t)h->Npad * (uint64_t)(8 * h->dx + 4);
    return SSME_OK;
}

// What both smoothing calls check after their own arguments, and what they share: the level-2 tables of the final weights (the
// forecast's, by the forecast's code), the events, the start event.  SSME_OK: `a` describes the history in force.
static int smoothing_begin(ssme_pf_handle h, int T, SmArgs* a) {
    if (h->shard_world > 0) { h->err = "smoothing of particle-sharded filters is not implemented"; return SSME_ERR_STATE; }
    switch (h->hist.query(h->hist_x && h->hist_anc, T)) {
        case SeriesHistoryState::none: h->err = "no series history in force: ssme_pf_set_series_history, then ssme_pf_run_series"; return SSME_ERR_STATE;
        case SeriesHistoryState::other_length: return SSME_ERR_INVALID_ARG;
        default: break;
    }
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = forecast_tables(h);                       // the level-2 tables and S' alone: nothing else of the forecast is touched
    if (rc != SSME_OK) return rc;
    for (hipEvent_t& e : h->sm_ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(h->sm_ev[0], h->stream));
    StepArgs p = step_args(h);
    p.t = h->t;
    forecast_plan(h, p);
    SmArgs s{};
    s.hx = h->hist_x; s.hanc = h->hist_anc; s.cdf = h->cdf[h->cur]; s.l2_T = h->fc.T; s.l2_R = h->fc.R; s.scal = h->fc.scal;
    s.keyp = h->keybuf; s.first_filter = h->cfg.first_filter_id;
    s.N = h->N; s.Npad = h->Npad; s.B = h->B; s.Bs = h->Bs; s.Bpow2 = h->Bpow2; s.tile = h->tile; s.R = h->R; s.T = T;
    s.resamp_sched = h->cfg.resamp_sched; s.dx = h->dx;
    *a = s;
    HIPCHK(hipEventRecord(h->sm_ev[1], h->stream));
    return SSME_OK;
}
// ... and after their downloads are queued: the wait and the two times
static int smoothing_end(ssme_pf_handle h) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventElapsedTime(&h->sm_ms_kernel, h->sm_ev[1], h->sm_ev[2]));
    HIPCHK(hipEventElapsedTime(&h->sm_ms_call, h->sm_ev[0], h->sm_ev[2]));
    return SSME_OK;
}
extern "C++" {
// a device buffer of the smoothing calls grown to n elements (capacity 0 while it is replaced: a failed allocation leaves none)
template <class T>
static int sm_grow(ssme_pf_handle h, T*& p, size_t& cap, size_t n) {
    if (n <= cap) return SSME_OK;
    cap = 0;
    const hipError_t e = own_alloc(h, p, sizeof(T) * n);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, "smoothing output buffer", e); }
    cap = n;
    return SSME_OK;
}

template <int DX>
static void launch_sm_trajectories(ssme_pf_handle h, const SmArgs& a, int K, const uint32_t* term, uint32_t* idx) {
    hipLaunchKernelGGL((k_sm_trajectories<DX>), dim3((K + kSmChains * kThreads - 1) / (kSmChains * kThreads), h->R), dim3(kThreads), 0, h->stream,
                       a, K, term, h->sm_x, idx);
}
}  // extern "C++"

int ssme_pf_sample_trajectories(ssme_pf_handle h, int32_t K, const uint32_t* terminal, double* x_out, uint32_t* index_out, int32_t T) {
    if (!h || !x_out || K < 1 || K > h->N || T < 1) return SSME_ERR_INVALID_ARG;
    if (terminal)
        for (size_t i = 0; i < (size_t)h->R * K; ++i)
            if (terminal[i] >= (uint32_t)h->N) return SSME_ERR_INVALID_ARG;
    SmArgs a;
    int rc = smoothing_begin(h, T, &a);
    if (rc != SSME_OK) return rc;
    const size_t nk = (size_t)h->R * K, ni = nk * T, nx = ni * h->dx;
    rc = sm_grow(h, h->sm_x, h->sm_cap_x, nx);
    if (rc == SSME_OK && index_out) rc = sm_grow(h, h->sm_idx, h->sm_cap_idx, ni);
    if (rc == SSME_OK && terminal) rc = sm_grow(h, h->sm_term, h->sm_cap_term, nk);
    if (rc != SSME_OK) return rc;
    if (terminal) HIPCHK(hipMemcpyAsync(h->sm_term, terminal, sizeof(uint32_t) * nk, hipMemcpyHostToDevice, h->stream));
    const uint32_t* term = terminal ? h->sm_term : nullptr;
    uint32_t* idx = index_out ? h->sm_idx : nullptr;
    switch (h->dx) {
        case 1: launch_sm_trajectories<1>(h, a, K, term, idx); break;
        case 2: launch_sm_trajectories<2>(h, a, K, term, idx); break;
        case 3: launch_sm_trajectories<3>(h, a, K, term, idx); break;
        default: launch_sm_trajectories<4>(h, a, K, term, idx); break;
    }
    HIPCHK(hipEventRecord(h->sm_ev[2], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(x_out, h->sm_x, sizeof(double) * nx, hipMemcpyDeviceToHost, h->stream));
    if (index_out) HIPCHK(hipMemcpyAsync(index_out, h->sm_idx, sizeof(uint32_t) * ni, hipMemcpyDeviceToHost, h->stream));
    rc = smoothing_end(h);
    if (rc != SSME_OK) return rc;
    round_out(h, x_out, nx);
    return SSME_OK;
}

int ssme_pf_get_smoothed_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* out, int32_t T) {
    if (!h || !out || !functionals || n < 1 || n > kMaxFunctionals || T < 1) return SSME_ERR_INVALID_ARG;
    FunctionalIds fs{};
    fs.n = n;
    for (int i = 0; i < n; ++i) {
        if (functionals[i] < SSME_H_X || functionals[i] > SSME_H_CONST42) return SSME_ERR_INVALID_ARG;
        fs.id[i] = functionals[i];
    }
    SmArgs a;
    int rc = smoothing_begin(h, T, &a);
    if (rc != SSME_OK) return rc;
    const size_t npart = (size_t)T * h->R * h->Bs * kMaxFunctionals, nout = (size_t)T * n * h->R;
    if (npart > h->sm_cap_part) {
        h->sm_cap_part = 0;
        hipError_t e = own_alloc(h, h->sm_part, sizeof(double) * npart);
        if (e == hipSuccess) e = own_alloc(h, h->sm_out, sizeof(double) * (size_t)T * kMaxFunctionals * h->R);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, "smoothing sweep buffers", e); }
        h->sm_cap_part = npart;
    }
    const dim3 grid(h->B, h->R);
    if (h->tile == kTileSmall) hipLaunchKernelGGL((k_sm_sweep<kTileSmall / kThreads>), grid, dim3(kThreads), 0, h->stream, a, fs, h->sm_part);
    else if (h->tile == kTileMid) hipLaunchKernelGGL((k_sm_sweep<kTileMid / kThreads>), grid, dim3(kThreads), 0, h->stream, a, fs, h->sm_part);
    else hipLaunchKernelGGL((k_sm_sweep<kTile / kThreads>), grid, dim3(kThreads), 0, h->stream, a, fs, h->sm_part);
    hipLaunchKernelGGL(k_sm_final, dim3((unsigned)((size_t)T * h->R)), dim3(kThreads), 0, h->stream, (const double*)h->sm_part,
                       (const double*)h->tsum[h->cur], (const double*)h->tmax[h->cur], h->B, h->Bs, h->R, fs, h->sm_out);
    HIPCHK(hipEventRecord(h->sm_ev[2], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->sm_out, sizeof(double) * nout, hipMemcpyDeviceToHost, h->stream));
    rc = smoothing_end(h);
    if (rc != SSME_OK) return rc;
    round_out(h, out, nout);
    return SSME_OK;
}

// ---- backward simulation (kernels: backward.h) ----
int ssme_pf_backward_bytes(ssme_pf_handle h, int32_t T, uint64_t* bytes) {
    if (!h || !bytes || T < 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    *bytes = (uint64_t)8 * (uint64_t)T * (uint64_t)h->R * (uint64_t)h->Npad;
    return SSME_OK;
}

extern "C++" {
template <int MODEL>
static void launch_bsim_logw(ssme_pf_handle h, const BsimArgs& a) {
    if constexpr (MODEL != MODEL_USER0 || kUserHasLogf)
        hipLaunchKernelGGL((k_bsim_logw<MODEL>), dim3(h->Npad / kThreads, h->R), dim3(kThreads), 0, h->stream, a);
}
template <int MODEL>
static void launch_bsim(ssme_pf_handle h, const BsimArgs& a, int K, const uint32_t* term, uint32_t* idx) {
    if constexpr (MODEL != MODEL_USER0 || kUserHasLogf) {
        const dim3 grid((K + kBsimG - 1) / kBsimG, h->R);
        if (h->N <= 2 * kThreads) hipLaunchKernelGGL((k_bsim<MODEL, 2>), grid, dim3(kThreads), 0, h->stream, a, K, term, h->sm_x, idx);
        else hipLaunchKernelGGL((k_bsim<MODEL, 8>), grid, dim3(kThreads), 0, h->stream, a, K, term, h->sm_x, idx);
    }
}
}  // extern "C++"

// The log-weight rows of the history in force (T steps), filled on the first call after the recording run and reused while that
// history stays in force (series_history.h).  `a`: what both backward kernels read of the handle, a->s of the caller left alone.
static int backward_weights(ssme_pf_handle h, int T, BsimArgs* a) {
    if (h->hist.weights_query(h->bs_lw != nullptr) == SeriesHistoryState::allocate) {
        h->hist.weights_dropped();
        const hipError_t e = own_alloc(h, h->bs_lw, sizeof(double) * (size_t)T * h->R * h->Npad);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, "backward-simulation weights (ssme_pf_backward_bytes)", e); }
        h->hist.weights_ready(T);
    }
    a->y = h->ybuf; a->z = h->hist_has_z ? h->zbuf : nullptr; a->mc = h->mc; a->lw = h->bs_lw;
    int lg = 0;
    while ((1L << lg) < (long)h->N) ++lg;                        // ceil(log2 N)
    a->shift = 52 - lg < kTileShift ? 52 - lg : kTileShift;
    if (h->hist.weights_query(true) == SeriesHistoryState::fill) {
        BsimArgs w = *a;
        w.s = SmArgs{};
        w.s.hx = h->hist_x; w.s.N = h->N; w.s.Npad = h->Npad; w.s.R = h->R; w.s.T = T; w.s.resamp_sched = h->cfg.resamp_sched; w.s.dx = h->dx;
        with_model(h->cfg.model, [&](auto m) { launch_bsim_logw<decltype(m)::value>(h, w); });
        HIPCHK(hipGetLastError());
        h->hist.weights_filled();
    }
    return SSME_OK;
}

int ssme_pf_download_series_logweights(ssme_pf_handle h, int32_t filter, int32_t t, double* lw) {
    if (!h || !lw || filter < 0 || filter >= h->R || t < 0) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->cfg.model == SSME_MODEL_USER0 && !kUserHasLogf) return SSME_ERR_UNSUPPORTED;
    if (h->hist.query(h->hist_x && h->hist_anc, h->hist.T) != SeriesHistoryState::in_force) {
        h->err = "no series history in force: ssme_pf_set_series_history, then ssme_pf_run_series";
        return SSME_ERR_STATE;
    }
    if (t >= h->hist.T) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    BsimArgs a{};
    const int rc = backward_weights(h, h->hist.T, &a);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipMemcpyAsync(lw, h->bs_lw + ((size_t)t * h->R + filter) * h->Npad, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    round_out(h, lw, h->N);
    return SSME_OK;
}

int ssme_pf_sample_trajectories_backward(ssme_pf_handle h, int32_t K, const uint32_t* terminal, double* x_out, uint32_t* index_out, int32_t T) {
    if (!h || !x_out || K < 1 || K > h->N || T < 1) return SSME_ERR_INVALID_ARG;
    if (terminal)
        for (size_t i = 0; i < (size_t)h->R * K; ++i)
            if (terminal[i] >= (uint32_t)h->N) return SSME_ERR_INVALID_ARG;
    if (h->cfg.model == SSME_MODEL_USER0 && !kUserHasLogf && h->shard_world == 0) return SSME_ERR_UNSUPPORTED;
    BsimArgs a{};
    int rc = smoothing_begin(h, T, &a.s);
    if (rc == SSME_OK) rc = backward_weights(h, T, &a);
    if (rc != SSME_OK) return rc;
    const size_t nk = (size_t)h->R * K, ni = nk * T, nx = ni * h->dx;
    rc = sm_grow(h, h->sm_x, h->sm_cap_x, nx);
    if (rc == SSME_OK && index_out) rc = sm_grow(h, h->sm_idx, h->sm_cap_idx, ni);
    if (rc == SSME_OK && terminal) rc = sm_grow(h, h->sm_term, h->sm_cap_term, nk);
    if (rc != SSME_OK) return rc;
    if (terminal) HIPCHK(hipMemcpyAsync(h->sm_term, terminal, sizeof(uint32_t) * nk, hipMemcpyHostToDevice, h->stream));
    const uint32_t* term = terminal ? h->sm_term : nullptr;
    uint32_t* idx = index_out ? h->sm_idx : nullptr;
    with_model(h->cfg.model, [&](auto m) { launch_bsim<decltype(m)::value>(h, a, K, term, idx); });
    HIPCHK(hipEventRecord(h->sm_ev[2], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(x_out, h->sm_x, sizeof(double) * nx, hipMemcpyDeviceToHost, h->stream));
    if (index_out) HIPCHK(hipMemcpyAsync(index_out, h->sm_idx, sizeof(uint32_t) * ni, hipMemcpyDeviceToHost, h->stream));
    rc = smoothing_end(h);
    if (rc != SSME_OK) return rc;
    round_out(h, x_out, nx);
    return SSME_OK;
}

// ---- marginal smoothing weights (kernels: marginal.h; the state of the rows: marginal_state.h) ----
int ssme_pf_marginal_smoothing_bytes(ssme_pf_handle h, int32_t T, uint64_t* bytes) {
    if (!h || !bytes || T < 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    // 8 (the log-weight rows, shared with backward simulation: ssme_pf_backward_bytes) + 8 (om) + 16 (m and D) bytes per particle and step
    *bytes = (uint64_t)32 * (uint64_t)T * (uint64_t)h->R * (uint64_t)h->Npad;
    return SSME_OK;
}

extern "C++" {
constexpr int kMsmNJ = 2;          // columns per thread of k_msm_columns
template <int MODEL>
static void launch_msm_fill(ssme_pf_handle h, const MsmArgs& a, int T) {
    if constexpr (MODEL != MODEL_USER0 || kUserHasLogf) {
        hipLaunchKernelGGL(k_msm_start, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, a, (const double*)h->tmax[h->cur]);
        if (T < 2) return;
        const unsigned gx = (unsigned)((h->N + kThreads * kMsmNJ - 1) / (kThreads * kMsmNJ));
        for (int t0 = 0; t0 < T - 1; t0 += 65535) {
            const int steps = T - 1 - t0 < 65535 ? T - 1 - t0 : 65535;
            hipLaunchKernelGGL((k_msm_columns<MODEL, kMsmNJ>), dim3(gx, steps, h->R), dim3(kThreads), 0, h->stream, a, t0);
        }
        const dim3 grid((h->N + 63) / 64, h->R);
        for (int t = T - 2; t >= 0; --t) hipLaunchKernelGGL((k_msm_rows<MODEL>), grid, dim3(64 * kMsmSeg), 0, h->stream, a, t);
    }
}
}  // extern "C++"

// The weight rows of the history in force (T steps): the log-weight rows first (backward_weights), then om, m and D, filled on the first
// marginal call after the recording run and reused while that history stays in force (marginal_state.h).  a->b.s: smoothing_begin's.
static int marginal_rows(ssme_pf_handle h, int T, MsmArgs* a) {
    int rc = backward_weights(h, T, &a->b);
    if (rc != SSME_OK) return rc;
    const size_t n = (size_t)T * h->R * h->Npad;
    if (h->msm.query(h->ms_rows != nullptr, T) == MarginalRowsState::rows_allocate) {
        h->msm.dropped();
        const hipError_t e = own_alloc(h, h->ms_rows, sizeof(double) * 3 * n);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, "marginal smoothing rows (ssme_pf_marginal_smoothing_bytes)", e); }
        h->msm.ready(T);
    }
    const size_t cap = (size_t)h->msm.cap * h->R * h->Npad;
    a->om = h->ms_rows; a->cm = h->ms_rows + cap; a->cD = h->ms_rows + 2 * cap;
    if (h->msm.query(true, T) == MarginalRowsState::rows_fill) {
        with_model(h->cfg.model, [&](auto m) { launch_msm_fill<decltype(m)::value>(h, *a, T); });
        HIPCHK(hipGetLastError());
        h->msm.filled(T);
    }
    return SSME_OK;
}

int ssme_pf_download_smoothing_weights(ssme_pf_handle h, int32_t filter, int32_t t, double* x, double* w) {
    if (!h || !w || filter < 0 || filter >= h->R || t < 0) return SSME_ERR_INVALID_ARG;
    // as ssme_pf_download_series_logweights: the handle's state, then the range of t, before any HIP call
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->cfg.model == SSME_MODEL_USER0 && !kUserHasLogf) return SSME_ERR_UNSUPPORTED;
    if (h->hist.query(h->hist_x && h->hist_anc, h->hist.T) != SeriesHistoryState::in_force) {
        h->err = "no series history in force: ssme_pf_set_series_history, then ssme_pf_run_series";
        return SSME_ERR_STATE;
    }
    if (t >= h->hist.T) return SSME_ERR_INVALID_ARG;
    MsmArgs a{};
    int rc = smoothing_begin(h, h->hist.T, &a.b.s);
    if (rc == SSME_OK) rc = marginal_rows(h, h->hist.T, &a);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipEventRecord(h->sm_ev[2], h->stream));
    const size_t plane = (size_t)h->R * h->Npad, off = (size_t)filter * h->Npad;
    HIPCHK(hipMemcpyAsync(w, a.om + (size_t)t * plane + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    if (x) for (int d = 0; d < h->dx; ++d)                 // vector models: dim_x planes, x[d * N + i]
        HIPCHK(hipMemcpyAsync(x + (size_t)d * h->N, h->hist_x + ((size_t)t * h->dx + d) * plane + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    rc = smoothing_end(h);
    if (rc != SSME_OK) return rc;
    round_out(h, x, (size_t)h->dx * h->N);
    round_out(h, w, h->N);
    return SSME_OK;
}

int ssme_pf_get_marginal_smoothed_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* out, int32_t T) {
    if (!h || !out || !functionals || n < 1 || n > kMaxFunctionals || T < 1) return SSME_ERR_INVALID_ARG;
    FunctionalIds fs{};
    fs.n = n;
    for (int i = 0; i < n; ++i) {
        if (functionals[i] < SSME_H_X || functionals[i] > SSME_H_CONST42) return SSME_ERR_INVALID_ARG;
        fs.id[i] = functionals[i];
    }
    if (h->cfg.model == SSME_MODEL_USER0 && !kUserHasLogf && h->shard_world == 0) return SSME_ERR_UNSUPPORTED;
    MsmArgs a{};
    int rc = smoothing_begin(h, T, &a.b.s);
    if (rc == SSME_OK) rc = marginal_rows(h, T, &a);
    const size_t nout = (size_t)T * n * h->R;
    if (rc == SSME_OK) rc = sm_grow(h, h->ms_out, h->ms_cap_out, (size_t)T * kMaxFunctionals * h->R);
    if (rc != SSME_OK) return rc;
    hipLaunchKernelGGL(k_msm_expect, dim3((unsigned)((size_t)T * h->R)), dim3(kThreads), 0, h->stream, a, fs, h->ms_out);
    HIPCHK(hipEventRecord(h->sm_ev[2], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->ms_out, sizeof(double) * nout, hipMemcpyDeviceToHost, h->stream));
    rc = smoothing_end(h);
    if (rc != SSME_OK) return rc;
    round_out(h, out, nout);
    return SSME_OK;
}

int ssme_pf_smoothing_elapsed_ms(ssme_pf_handle h, float* kernel_ms, float* call_ms) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (kernel_ms) *kernel_ms = h->sm_ms_kernel;
    if (call_ms) *call_ms = h->sm_ms_call;
    return SSME_OK;
}

int ssme_pf_get_per_step(ssme_pf_handle h, double* out, int32_t T) {
    const int rc = read_per_step(h, out, T);
    if (rc == SSME_OK) round_out(h, out, (size_t)h->R * T);
    return rc;
}

int ssme_pf_get_loglik(ssme_pf_handle h, double* out) {
    if (!h || !out) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    const int rc = read_loglik(h, out);
    if (rc == SSME_OK) round_out(h, out, h->R);
    return rc;
}

int ssme_pf_log_mean_exp(ssme_pf_handle h, double* out) {
    if (!h || !out) return SSME_ERR_INVALID_ARG;
    std::vector<double> ll(h->R);
    int rc = ssme_pf_get_loglik(h, ll.data());
    if (rc != SSME_OK) return rc;
    // thread_pool.h:263-268, host side (R is small): m + log(sum exp(v - m)) - log R
    double m = ll[0];
    for (double v : ll) if (v > m) m = v;
    double s = 0.0;
    for (double v : ll) s += std::exp(v - m);
    *out = m + std::log(s) - std::log((double)h->R);
    round_out(h, out, 1);
    return SSME_OK;
}

// per-filter expectations of n built-in functionals into exp_out rows 0..n-1 (device); three small launches, no sync
static int enqueue_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n) {
    if (n < 1 || n > kMaxFunctionals) return SSME_ERR_INVALID_ARG;
    FunctionalIds fs{};
    fs.n = n;
    for (int i = 0; i < n; ++i) {
        if (functionals[i] < 0 || functionals[i] > SSME_H_CONST42) return SSME_ERR_INVALID_ARG;
        fs.id[i] = functionals[i];
    }
    hipLaunchKernelGGL(k_expect_partials, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, h->x[h->cur], h->cdf[h->cur], h->N,
                       h->Npad, h->Bs, h->tile, fs, h->exp_part);
    hipLaunchKernelGGL(k_expect_final, dim3(h->R), dim3(kThreads), 0, h->stream, h->exp_part, h->tsum[h->cur], h->tmax[h->cur],
                       h->B, h->Bs, h->R, fs, h->exp_out);
    HIPCHK(hipGetLastError());
    return SSME_OK;
}

int ssme_pf_get_expectations_multi(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* out) {
    if (!h || !out || !functionals) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = enqueue_expectations(h, functionals, n);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, h->exp_out, sizeof(double) * (size_t)n * h->R, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    round_out(h, out, (size_t)n * h->R);
    return SSME_OK;
}

int ssme_pf_get_expectations(ssme_pf_handle h, int32_t functional, double* out) {
    return ssme_pf_get_expectations_multi(h, &functional, 1, out);
}

// Swarm::update's aggregation (pswarm_filter.h:96-160,233-235): the plain means over the R member filters of the last
// step's log conditional likelihoods and of the expectations, reduced ON THE DEVICE; one download of n + 1 doubles.
int ssme_pf_swarm_aggregate(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* mean_logcondlike,
                            double* mean_expectations) {
    return ssme_pf_swarm_aggregate_threads(h, functionals, n, 0, mean_logcondlike, mean_expectations);
}

int ssme_pf_swarm_aggregate_threads(ssme_pf_handle h, const int32_t* functionals, int32_t n, int32_t num_threads, double* mean_logcondlike,
                                    double* mean_expectations) {
    if (!h || !mean_logcondlike || n < 0 || n > kMaxFunctionals || (n > 0 && (!functionals || !mean_expectations)))
        return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (n > 0) {
        int rc = enqueue_expectations(h, functionals, n);
        if (rc != SSME_OK) return rc;
    }
    // one launch writes the n + 1 means straight into mapped host memory, where the host waits for them (see wait_results)
    const size_t slot0 = PinLayout::swarm(h->R);
    double* pin = h->pin + slot0;
    mark_results_pending(pin, n);
    mark_results_pending(pin + kMaxFunctionals, 1);
    hipLaunchKernelGGL(k_swarm_means, dim3(n + 1), dim3(kThreads), 0, h->stream, (const double*)h->exp_out, (const FilterScalars*)h->scal,
                       h->R, n, kMaxFunctionals, h->pin_dev + slot0, (int)num_threads);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_results(h->stream, pin + kMaxFunctionals, 1));
    if (n > 0) HIPCHK(wait_results(h->stream, pin, n));
    *mean_logcondlike = pin[kMaxFunctionals];
    for (int i = 0; i < n; ++i) mean_expectations[i] = pin[i];
    round_out(h, mean_logcondlike, 1);
    round_out(h, mean_expectations, (size_t)n);
    return SSME_OK;
}

// ---- the user model's own functionals: entry points (the launches: enqueue_user_expectations, above) ----
int ssme_pf_get_user_expectations(ssme_pf_handle h, double* out) {
    if (!h || !out) return SSME_ERR_INVALID_ARG;
    const int rc = user_expectations_checked(h);
    if (rc != SSME_OK) return rc;
    const size_t n = (size_t)ssme_pf_user_model_n_h() * h->R;
    HIPCHK(hipMemcpyAsync(out, h->uexp_out, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    round_out(h, out, n);
    return SSME_OK;
}

// ssme_pf_swarm_aggregate_threads for the user model's functionals: the same launch of k_swarm_means over n_h rows, its n_h + 1
// means written into mapped host memory (slots of their own behind the built-ins')
int ssme_pf_swarm_aggregate_user(ssme_pf_handle h, int32_t num_threads, double* mean_logcondlike, double* mean_expectations) {
    if (!h || !mean_logcondlike || !mean_expectations) return SSME_ERR_INVALID_ARG;
    const int rc = user_expectations_checked(h);
    if (rc != SSME_OK) return rc;
    const int n = ssme_pf_user_model_n_h();
    const size_t slot0 = PinLayout::user(h->R);
    double* pin = h->pin + slot0;
    mark_results_pending(pin, kMaxUserFunctionals + 1);
    hipLaunchKernelGGL(k_swarm_means, dim3(n + 1), dim3(kThreads), 0, h->stream, (const double*)h->uexp_out, (const FilterScalars*)h->scal,
                       h->R, n, kMaxUserFunctionals, h->pin_dev + slot0, (int)num_threads);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_results(h->stream, pin + kMaxUserFunctionals, 1));
    HIPCHK(wait_results(h->stream, pin, n));
    *mean_logcondlike = pin[kMaxUserFunctionals];
    for (int i = 0; i < n; ++i) mean_expectations[i] = pin[i];
    round_out(h, mean_logcondlike, 1);
    round_out(h, mean_expectations, (size_t)n);
    return SSME_OK;
}

// Particles and normalisable weights of one filter after the last step, for functionals that cannot run on the device
// (arbitrary std::function h, pswarm_filter.h:44): w_j = exp(logw_j - max logw) up to the 2^-41 fixed point -- the same
// weights the device expectations and the resampler use.  No debug mode needed (the weights are rebuilt from the cdf).
int ssme_pf_download_weights(ssme_pf_handle h, int32_t f, double* x, double* w) {
    if (!h || f < 0 || f >= h->R || !w) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->wscratch) HIPCHK(own_alloc(h, h->wscratch, sizeof(double) * (size_t)h->Npad));
    const size_t off = (size_t)f * h->Npad;
    hipLaunchKernelGGL(k_weights, dim3(h->B), dim3(kThreads), 0, h->stream, (const double*)(h->cdf[h->cur] + off),
                       (const double*)(h->tmax[h->cur] + (size_t)f * h->Bs), h->N, h->B, h->tile, h->wscratch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w, h->wscratch, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    if (x) for (int d = 0; d < h->dx; ++d)                 // vector models: dim_x planes, x[d * N + i]
        HIPCHK(hipMemcpyAsync(x + (size_t)d * h->N, h->x[h->cur] + (size_t)d * h->R * h->Npad + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    round_out(h, x, h->N);
    round_out(h, w, h->N);
    return SSME_OK;
}

int ssme_pf_download_state(ssme_pf_handle h, int32_t f, double* x, double* logw, uint64_t* cdf, uint32_t* anc) {
    if (!h || f < 0 || f >= h->R) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t off = (size_t)f * h->Npad;
    if (x) for (int d = 0; d < h->dx; ++d)                 // vector models: dim_x planes, x[d * N + i]
        HIPCHK(hipMemcpyAsync(x + (size_t)d * h->N, h->x[h->cur] + (size_t)d * h->R * h->Npad + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    if (logw) {
        if (!h->logw || !logw_needed(h)) return SSME_ERR_STATE;      // set_debug(2) before stepping
        HIPCHK(hipMemcpyAsync(logw, h->logw + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    }
    if (cdf) HIPCHK(hipMemcpyAsync(cdf, h->cdf[h->cur] + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    if (anc) {
        if (!h->anc) return SSME_ERR_STATE;
        HIPCHK(hipMemcpyAsync(anc, h->anc + off, sizeof(uint32_t) * h->N, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (cdf) {   // the device holds the integers in fp64 registers/memory; hand them out as integers
        double dv;
        for (int i = 0; i < h->N; ++i) { std::memcpy(&dv, &cdf[i], 8); cdf[i] = (uint64_t)dv; }
    }
    return SSME_OK;
}

int ssme_pf_download_scalars(ssme_pf_handle h, int32_t f, double* max_logw, uint64_t* sum_q, uint64_t* tile_sums,
                             double* tile_max, int32_t* rshift) {
    if (!h || f < 0 || f >= h->R) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    FilterScalars sc;
    HIPCHK(hipMemcpyAsync(&sc, h->scal + f, sizeof(sc), hipMemcpyDeviceToHost, h->stream));
    if (tile_sums) HIPCHK(hipMemcpyAsync(tile_sums, h->tsum[h->cur] + (size_t)f * h->Bs, sizeof(double) * h->B,
                                         hipMemcpyDeviceToHost, h->stream));
    if (tile_max) HIPCHK(hipMemcpyAsync(tile_max, h->tmax[h->cur] + (size_t)f * h->Bs, sizeof(double) * h->B,
                                        hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (tile_sums) { double dv; for (int i = 0; i < h->B; ++i) { std::memcpy(&dv, &tile_sums[i], 8); tile_sums[i] = (uint64_t)dv; } }
    if (max_logw) *max_logw = sc.m;
    if (sum_q) *sum_q = (sc.S == sc.S && sc.S > 0.0) ? (uint64_t)sc.S : 0;
    if (rshift) *rshift = h->rshift;
    return SSME_OK;
}

int ssme_pf_get_layout(ssme_pf_handle h, int32_t* tile_particles, int32_t* n_tiles) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (tile_particles) *tile_particles = h->tile;
    if (n_tiles) *n_tiles = h->B;
    return SSME_OK;
}

// ---- forecast: simulated future observations (forecast.h) -------------------------------------------
// z_future: null (ssme_pf_sim_future_obs: y_prev is the covariate) or [num_steps][dim_cov] exogenous covariates (.._cov)
static int sim_future_obs_impl(ssme_pf_handle h, int32_t num_steps, const double* last_obs, const double* z_future, bool cov,
                               double* y_out, double* x_out, uint32_t* start_out) {
    if (!h || !y_out || num_steps < 1 || num_steps > kFcMaxSteps || (cov && !z_future)) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) { h->err = "forecasts of particle-sharded filters are not implemented"; return SSME_ERR_UNSUPPORTED; }
    const bool user = h->cfg.model == SSME_MODEL_USER0;
    if (cov && h->kcov == 0) { h->err = "sim_future_obs_cov needs a user model that declares dim_cov (model_api.h)"; return SSME_ERR_UNSUPPORTED; }
    if (!cov && h->kcov > 0) { h->err = "a dim_cov model is forecast with future covariates: ssme_pf_sim_future_obs_cov"; return SSME_ERR_UNSUPPORTED; }
    if (user && !kUserHasGsamp) { h->err = "this user model declares no observation draw (gsamp / gsamp_vec, model_api.h)"; return SSME_ERR_UNSUPPORTED; }
    if (!h->params_set || h->t < 1) { h->err = "sim_future_obs before the first step"; return SSME_ERR_STATE; }
    const int H = num_steps, R = h->R, N = h->N;
    const int dx = h->dx, dy = h->dy;                      // 1 unless this is a vector user model
    const size_t Ns = (N + 1) & ~1, rows = (size_t)R * H;
    h->fc.h_last_obs.assign(R, 0.0);
    if (last_obs) for (int r = 0; r < R; ++r) h->fc.h_last_obs[r] = h->cfg.dtype == SSME_F32 ? f32r(last_obs[r]) : last_obs[r];
    int rc = forecast_prepare(h, dx, rows * dy * Ns, x_out ? rows * dx * Ns : 0);
    if (rc != SSME_OK) return rc;
    if (!h->fc_gscale) HIPCHK(own_alloc(h, h->fc_gscale, sizeof(double) * R));
    HIPCHK(hipMemcpyAsync(h->fc_gscale, h->h_gscale.data(), sizeof(double) * R, hipMemcpyHostToDevice, h->stream));
    std::vector<double> zf;                                  // lives until forecast_finish has waited for the stream
    if (cov) {
        const size_t nz = (size_t)H * h->kcov;               // what k_fc_horizon_user reads: z_future[k * dim_cov + j], k < H
        if (nz > h->fc_zfut_cap) { HIPCHK(own_alloc(h, h->fc_zfut, sizeof(double) * nz)); h->fc_zfut_cap = nz; }
        zf.assign(z_future, z_future + nz);
        if (h->cfg.dtype == SSME_F32) for (double& v : zf) v = f32r(v);
        HIPCHK(hipMemcpyAsync(h->fc_zfut, zf.data(), sizeof(double) * nz, hipMemcpyHostToDevice, h->stream));
    }
    {
        // level-2 of the last step's weights (the weights ssme_pf_get_expectations uses): step_args reads buffers `cur`
        StepArgs p = step_args(h);
        p.t = h->t;
        forecast_plan(h, p);
    }
    FcArgs a{};
    a.x = h->x[h->cur]; a.cdf = h->cdf[h->cur]; a.l2_T = h->fc.T; a.l2_R = h->fc.R; a.scal = h->fc.scal; a.mc = h->mc;
    a.gscale = h->fc_gscale; a.z_future = cov ? h->fc_zfut : nullptr; a.last_obs = h->fc.last; a.x0 = h->fc.x0; a.start = h->fc.start;
    a.y_out = h->fc.y; a.x_out = x_out ? h->fc.x : nullptr;
    a.keyp = h->keybuf; a.first_filter = h->cfg.first_filter_id;
    a.N = N; a.Npad = h->Npad; a.Ns = (int)Ns; a.B = h->B; a.Bs = h->Bs; a.Bpow2 = h->Bpow2; a.tile = h->tile; a.t0 = h->t; a.H = H;
    if (user) {
#if SSME_HAS_USER_MODEL
        HIPCHK(launch_fc_user<ssme_user_model0>(h, a));
#endif
    } else {
        HIPCHK(launch_fc_start<1>(h, a));
        with_model(h->cfg.model, [&](auto m) { launch_fc_horizon<decltype(m)::value>(h, a); });
    }
    rc = forecast_finish(h, y_out, rows * dy, x_out, rows * dx, start_out);
    if (rc != SSME_OK) return rc;
    round_out(h, y_out, rows * dy * N);
    round_out(h, x_out, rows * dx * N);
    return SSME_OK;
}

int ssme_pf_sim_future_obs(ssme_pf_handle h, int32_t num_steps, const double* last_obs, double* y_out, double* x_out,
                           uint32_t* start_out) {
    return sim_future_obs_impl(h, num_steps, last_obs, nullptr, false, y_out, x_out, start_out);
}

int ssme_pf_sim_future_obs_cov(ssme_pf_handle h, int32_t num_steps, const double* z_future, double* y_out, double* x_out,
                               uint32_t* start_out) {
    return sim_future_obs_impl(h, num_steps, nullptr, z_future, true, y_out, x_out, start_out);
}

int ssme_pf_forecast_elapsed_ms(ssme_pf_handle h, float* horizon_kernel_ms, float* call_ms) { return forecast_elapsed(h, horizon_kernel_ms, call_ms); }

int ssme_pf_last_elapsed_ms(ssme_pf_handle h, float* ms) { return elapsed_ms(h, ms); }

int ssme_pf_profile_series(ssme_pf_handle h, const double* y, const double* z, int32_t T, double* mean_us,
                           int32_t* launches) {
    if (!h || !y || !mean_us || !launches) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (T < 1) return SSME_ERR_LENGTH;
    if (!h->params_set) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = ensure_series_capacity(h, T);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->ybuf, y, sizeof(double) * T * h->dy, hipMemcpyHostToDevice, h->stream));
    if (z) HIPCHK(hipMemcpyAsync(h->zbuf, z, sizeof(double) * T * h->kz, hipMemcpyHostToDevice, h->stream));
    rc = do_reset(h);
    if (rc != SSME_OK) return rc;
    set_last_z(h, z, T);
    // one event every kGroup launches: an event pair around a single 20-us kernel adds ~3 us of its own
    const int kGroup = 32;
    const int nev = (T + kGroup - 1) / kGroup + 1;
    std::vector<hipEvent_t> ev((size_t)nev);
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    const bool has_z = z != nullptr;
    h->cur = 0;
    launch_gamma(h, 0, T);
    HIPCHK(hipEventRecord(ev[0], h->stream));
    for (int t = 0; t < T; ++t) {
        enqueue_step(h, t, t, t, has_z, t > 0, false);
        if ((t + 1) % kGroup == 0 || t + 1 == T) HIPCHK(hipEventRecord(ev[(t + kGroup) / kGroup], h->stream));
    }
    launch_kf(h, T - 1, false);
    HIPCHK(hipStreamSynchronize(h->stream));
    double sa = 0;
    for (int g = 0; g + 1 < nev; ++g) {
        float m1 = 0;
        HIPCHK(hipEventElapsedTime(&m1, ev[g], ev[g + 1]));
        sa += m1;
    }
    for (auto& e : ev) hipEventDestroy(e);
    mean_us[0] = sa * 1000.0 / T;
    launches[0] = T;
    h->t = T;
    return SSME_OK;
}

}  // extern "C"

// ---- device primitives for bit-parity tests ------------------------------------------------
__global__ void k_test_math(int fn, const double* in, double* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    double r, s, c;
    switch (fn) {
        case 0: r = dexp(x); break;
        case 1: r = dlog(x); break;
        case 2: dsincos2pi(x, &s, &c); r = s; break;
        case 3: dsincos2pi(x, &s, &c); r = c; break;
        case 4: r = dsqrt(x); break;
        case 6: r = dlog_u(x, kLogTable); break;
        case 7: r = dexp_scaled_t(x, 0, kExpTable); break;
        case 8: dsincos_k24((uint32_t)x, kSinCosTable, &s, &c); r = s; break;
        case 9: dsincos_k24((uint32_t)x, kSinCosTable, &s, &c); r = c; break;
        case 10: r = dlog_u32(x, kLogTable); break;
        case 11: r = dsqrt_pn(x); break;
        default: r = dlog_pn(x); break;
    }
    out[i] = r;
}
__global__ void k_test_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    const u32x4 o = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    out[0] = o.v0; out[1] = o.v1; out[2] = o.v2; out[3] = o.v3;
}
__global__ void k_test_quantize(const double* in, int shift, u64* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (u64)__builtin_rint(dexp_scaled_t(in[i], shift, kExpTable));
}
__global__ void k_test_rescale(const u64* A, const double* dm, int shift, u64* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (u64)__builtin_rint((double)A[i] * dexp_scaled_t(dm[i], shift, kExpTable));
}
template <int NT>
__global__ __launch_bounds__(NT) void k_test_block_scan(const u64* in, u64* incl, u64* total) {
    __shared__ double lds_seg[16];
    constexpr int NK = 1024 / NT;
    const int tid = threadIdx.x;
    double q[NK][2], inc[NK][2], tot;
    for (int k = 0; k < NK; ++k) { q[k][0] = (double)in[(k * NT + tid) * 2]; q[k][1] = (double)in[(k * NT + tid) * 2 + 1]; }
    block_scan_f64<NT, 1024 / NT>(q, inc, tot, lds_seg);
    for (int k = 0; k < NK; ++k) { incl[(k * NT + tid) * 2] = (u64)inc[k][0]; incl[(k * NT + tid) * 2 + 1] = (u64)inc[k][1]; }
    if (tid == 0) *total = (u64)tot;
}
// streaming copy with the step kernel's access shape (16 B per lane): calibrates FETCH_SIZE / WRITE_SIZE
__global__ __launch_bounds__(512) void k_calib_copy(const double* in, double* out, long n2) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<double2*>(out)[i] = reinterpret_cast<const double2*>(in)[i];
}
__global__ void k_test_gamma(uint32_t key0, uint32_t key1, uint32_t rep, int t, double shape, int n, double* out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) out[b] = gamma_draw((uint32_t)b, (uint32_t)t, rep, key0, key1, shape);
}

extern "C" {

#define HIPCHK0(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = SSME_ERR_HIP; goto done; } } while (0)

int ssme_pf_test_math(int32_t device, int32_t fn, const double* in, double* out, int64_t n) {
    if (!in || !out || n < 1) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    double *din = nullptr, *dout = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&din, sizeof(double) * n));
    HIPCHK0(hipMalloc(&dout, sizeof(double) * n));
    HIPCHK0(hipMemcpy(din, in, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, din, dout, (long)n);
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipMemcpy(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost));
done:
    if (din) hipFree(din);
    if (dout) hipFree(dout);
    return rc;
}

int ssme_pf_test_philox(int32_t device, const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4) {
    if (!ctr4 || !key2 || !out4) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    uint32_t* d = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&d, sizeof(uint32_t) * 10));
    HIPCHK0(hipMemcpy(d, ctr4, 16, hipMemcpyHostToDevice));
    HIPCHK0(hipMemcpy(d + 4, key2, 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_philox, dim3(1), dim3(1), 0, 0, d, d + 4, d + 6);
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipMemcpy(out4, d + 6, 16, hipMemcpyDeviceToHost));
done:
    if (d) hipFree(d);
    return rc;
}

int ssme_pf_test_quantize(int32_t device, const double* in, int32_t shift, uint64_t* out, int64_t n) {
    if (!in || !out || n < 1) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    double* din = nullptr; u64* dout = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&din, sizeof(double) * n));
    HIPCHK0(hipMalloc(&dout, sizeof(u64) * n));
    HIPCHK0(hipMemcpy(din, in, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_quantize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, din, shift, dout, (long)n);
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipMemcpy(out, dout, sizeof(u64) * n, hipMemcpyDeviceToHost));
done:
    if (din) hipFree(din);
    if (dout) hipFree(dout);
    return rc;
}

int ssme_pf_test_rescale(int32_t device, const uint64_t* tile_sums, const double* dm, int32_t shift, uint64_t* out, int64_t n) {
    if (!tile_sums || !dm || !out || n < 1) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    double* ddm = nullptr; u64 *dA = nullptr, *dout = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&ddm, sizeof(double) * n));
    HIPCHK0(hipMalloc(&dA, sizeof(u64) * n));
    HIPCHK0(hipMalloc(&dout, sizeof(u64) * n));
    HIPCHK0(hipMemcpy(ddm, dm, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK0(hipMemcpy(dA, tile_sums, sizeof(u64) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_rescale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dA, ddm, shift, dout, (long)n);
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipMemcpy(out, dout, sizeof(u64) * n, hipMemcpyDeviceToHost));
done:
    if (ddm) hipFree(ddm);
    if (dA) hipFree(dA);
    if (dout) hipFree(dout);
    return rc;
}

int ssme_pf_test_block_scan(int32_t device, int32_t threads, const uint64_t* in, uint64_t* incl, uint64_t* total) {
    if (!in || !incl || !total) return SSME_ERR_INVALID_ARG;
    if (threads != 256 && threads != 512 && threads != 1024) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    u64* d = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&d, sizeof(u64) * (2 * kTile + 1)));
    HIPCHK0(hipMemcpy(d, in, sizeof(u64) * kTile, hipMemcpyHostToDevice));
    if (threads == 256) hipLaunchKernelGGL(k_test_block_scan<256>, dim3(1), dim3(256), 0, 0, d, d + kTile, d + 2 * kTile);
    else if (threads == 512) hipLaunchKernelGGL(k_test_block_scan<512>, dim3(1), dim3(512), 0, 0, d, d + kTile, d + 2 * kTile);
    else hipLaunchKernelGGL(k_test_block_scan<1024>, dim3(1), dim3(1024), 0, 0, d, d + kTile, d + 2 * kTile);
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipMemcpy(incl, d + kTile, sizeof(u64) * kTile, hipMemcpyDeviceToHost));
    HIPCHK0(hipMemcpy(total, d + 2 * kTile, sizeof(u64), hipMemcpyDeviceToHost));
done:
    if (d) hipFree(d);
    return rc;
}

int ssme_pf_test_copy(int32_t device, int64_t n_doubles, int32_t repeats) {
    if (n_doubles < 2 || repeats < 1) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    double *a = nullptr, *b = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&a, sizeof(double) * n_doubles));
    HIPCHK0(hipMalloc(&b, sizeof(double) * n_doubles));
    HIPCHK0(hipMemset(a, 0, sizeof(double) * n_doubles));
    for (int i = 0; i < repeats; ++i)
        hipLaunchKernelGGL(k_calib_copy, dim3(512), dim3(512), 0, 0, (i & 1) ? b : a, (i & 1) ? a : b, (long)(n_doubles / 2));
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipDeviceSynchronize());
done:
    if (a) hipFree(a);
    if (b) hipFree(b);
    return rc;
}

int ssme_pf_test_gamma(int32_t device, uint64_t seed, uint32_t rep, int32_t t, double shape, int32_t n, double* out) {
    if (!out || n < 1) return SSME_ERR_INVALID_ARG;
    int rc = SSME_OK;
    double* d = nullptr;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMalloc(&d, sizeof(double) * n));
    hipLaunchKernelGGL(k_test_gamma, dim3((n + 255) / 256), dim3(256), 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32), rep, t,
                       shape, n, d);
    HIPCHK0(hipGetLastError());
    HIPCHK0(hipMemcpy(out, d, sizeof(double) * n, hipMemcpyDeviceToHost));
done:
    if (d) hipFree(d);
    return rc;
}

}  // extern "C"

// =============================================================================================
// Liu-West filter (LWFilterWithCovs, include/ssme/liu_west_filter.h:971-1159)
// =============================================================================================
struct ssme_lw_s : HandleCore {
    ssme_lw_config cfg;
    int debug;
    double *xB, *thB, *xr, *thr, *lw1, *cdfA, *tsumA, *tmaxA, *cdfB, *tsumB, *tmaxB, *mom, *prop;
    double* momtot;                  // [R][16] moment totals of k_lw_mom_totals (filters of more than 1024 tiles)
    double* lwB;                     // carried second-stage log-weights (resamp_sched > 1 only)
    double* wscratch;                // [5][Npad] weights + untransformed parameters of one filter (host-side functionals)
    int form, rs;                    // 0 auxiliary form / 1 SISR form; resampling schedule m_rs
    double* scratch;
    double *gamA, *pgamA, *gtotA, *gamB, *pgamB, *gtotB;
    uint32_t *anc, *kidx;
    uint32_t* ancbuf;        // unsharded handles: this step's resampling ancestors, stage 1 -> stage 2 (compose mode, lw_kernels.h)
    int fixed_trans;                 // the transform set is (logit, null, log, twice_fisher): stage kernels with it compiled in (lw_trans_kind)
    int small_series;                // 1: one-tile filters run steps 1 .. T-1 of a series in one launch (lw_small.h; lw_series_route decides)
    // recorded series (ssme_lw_set_series_expectations): the eight filtered expectations of every step of a run_series
    int rec_series;                  // the switch; survives reset, run_series and step
    double* traj;                    // [traj_cap][R][8]; held only while recording is on
    int traj_cap, traj_T;            // time rows traj holds; rows the last run_series recorded (0: none)
    // C++ shard driver (ssme_lw_shard_run_series): halo buffers ([margin | own | margin] rows of 2048 doubles; theta rows of 8192),
    // this rank's stage outputs for the gathers, the gathered arrays
    double *sh_xB, *sh_thB, *sh_cdfB, *sh_xr, *sh_thr, *sh_g1, *sh_cdfA;
    double *sh_locB, *sh_locA, *sh_allB_s, *sh_allB_m, *sh_allA_s, *sh_allA_m, *sh_mom_all;
    double *l2T[2], *l2R[2];         // [draw: 0 resampling (B), 1 k draw (A)][R][Bs]
    double* l2_work;                 // scratch of the multi-workgroup level-2 (the two draws run one after the other)
    int32_t *l2lo[2], *l2hi[2];
    FilterScalars* l2s[2];
    LwScalars* scal;
    // forecast (HandleCore::fc; samples [R][H][Ns]): the start population's parameter records [R][Npad][4], their moment partials
    // [R][B][16] and totals [R][16], theta-bar and L [R][16]; allocated on first use
    double *fc_th0, *fc_mom, *fc_momtot, *fc_prop;
};

static LwArgs lw_args(ssme_lw_handle h) {
    LwArgs a{};
    a.xB = h->xB; a.thB = h->thB; a.xr = h->xr; a.thr = h->thr; a.lw1 = h->lw1;
    a.lwB = h->rs > 1 ? h->lwB : nullptr; a.form = h->form; a.resamp_sched = h->rs;
    a.cdfA = h->cdfA; a.tsumA = h->tsumA; a.tmaxA = h->tmaxA; a.cdfB = h->cdfB; a.tsumB = h->tsumB; a.tmaxB = h->tmaxB;
    a.mom = h->mom; a.prop = h->prop;
    a.anc = (h->debug & 1) ? h->anc : nullptr; a.kidx = (h->debug & 1) ? h->kidx : nullptr;
    a.ancbuf = h->ancbuf; a.compose = (h->shard_world == 0 && h->ancbuf) ? 1 : 0;
    a.scal = h->scal; a.y = h->ybuf; a.z = h->zbuf; a.per_step = nullptr;
    a.gamA = h->gamA; a.pgamA = h->pgamA; a.gtotA = h->gtotA; a.gamB = h->gamB; a.pgamB = h->pgamB; a.gtotB = h->gtotB;
    a.N = h->N; a.Npad = h->Npad; a.B = h->B; a.Bs = h->Bs; a.Bpow2 = h->Bpow2; a.rshift = h->rshift; a.R = h->R;
    a.Tcap = h->tcap;
    a.key0 = (uint32_t)h->cfg.seed; a.key1 = (uint32_t)(h->cfg.seed >> 32); a.first_filter = h->cfg.first_filter_id;
    a.logN = dlog((double)h->N);
    a.a_shrink = (3.0 * h->cfg.delta - 1.0) / (2.0 * h->cfg.delta);          // liu_west_filter.h:960
    a.tile0 = 0; a.win_tile0 = 0;
    a.l2B_T = h->l2T[0]; a.l2B_R = h->l2R[0]; a.l2B_lo = h->l2lo[0]; a.l2B_hi = h->l2hi[0]; a.l2B_s = h->l2s[0];
    a.l2A_T = h->l2T[1]; a.l2A_R = h->l2R[1]; a.l2A_lo = h->l2lo[1]; a.l2A_hi = h->l2hi[1]; a.l2A_s = h->l2s[1];
    for (int d = 0; d < kDP; ++d) { a.trans[d] = h->cfg.transforms[d]; a.lo[d] = h->cfg.prior_lo[d]; a.hi[d] = h->cfg.prior_hi[d]; }
    return a;
}

static int lw_ensure_gamma(ssme_lw_handle h, int T) {
    if (T > h->gcap) {
        const size_t nb = sizeof(double) * (size_t)T * h->R * h->B, nr = sizeof(double) * (size_t)T * h->R;
        HIPCHK(own_alloc(h, h->gamA, nb)); HIPCHK(own_alloc(h, h->pgamA, nb)); HIPCHK(own_alloc(h, h->gtotA, nr));
        HIPCHK(own_alloc(h, h->gamB, nb)); HIPCHK(own_alloc(h, h->pgamB, nb)); HIPCHK(own_alloc(h, h->gtotB, nr));
        h->gcap = T;
    }
    return SSME_OK;
}

static int lw_ensure_capacity(ssme_lw_handle h, int T) {
    bool moved = false;
    const int rc = ensure_series_buffers(h, T, 1, &moved);
    return rc == SSME_OK ? lw_ensure_gamma(h, T) : rc;
}

// Gamma tables of both draws for time indices t0 .. t0+nT-1 into rows 0 .. nT-1
static void lw_launch_gamma(ssme_lw_handle h, int t0, int nT) {
    launch_gamma_tables(h, h->gamB, h->pgamB, h->gtotB, STREAM_GAMMA, STREAM_RESAMP_EXTRA, kTile, h->cfg.first_filter_id, t0, nT);
    launch_gamma_tables(h, h->gamA, h->pgamA, h->gtotA, STREAM_GAMMA_K, STREAM_LW_K_EXTRA, kTile, h->cfg.first_filter_id, t0, nT);
}

// the stage kernels: stage 1 / 2, BIG (split level-2), FT (the reference test models' transform set compiled in)
static const void* lw_stage_kernel(int stage, bool big, bool ft) {
    static const void* const tab[2][2][2] = {
        {{reinterpret_cast<const void*>(&k_lw_stage1<false, false>), reinterpret_cast<const void*>(&k_lw_stage1<false, true>)},
         {reinterpret_cast<const void*>(&k_lw_stage1<true, false>), reinterpret_cast<const void*>(&k_lw_stage1<true, true>)}},
        {{reinterpret_cast<const void*>(&k_lw_stage2<false, false>), reinterpret_cast<const void*>(&k_lw_stage2<false, true>)},
         {reinterpret_cast<const void*>(&k_lw_stage2<true, false>), reinterpret_cast<const void*>(&k_lw_stage2<true, true>)}}};
    return tab[stage - 1][big][ft];
}
static void lw_launch_stage(ssme_lw_handle h, int stage, dim3 grid, const LwArgs& a) {
    void* args[] = {const_cast<LwArgs*>(&a)};
    hipLaunchKernel(lw_stage_kernel(stage, h->split_l2, h->fixed_trans), grid, dim3(kLwNT), args,
                    h->split_l2 ? h->lds_bytes_big : h->lds_bytes, h->stream);
}

// the StepArgs of a level-2 of draw 0 (resampling, second-stage weights, Gamma tables B) or 1 (k draw, first-stage weights, tables A)
// from the given tile sums / maxima: what k_level2_plan / k_l2_scan_blocks / k_l2_ranges and k_shard_plan read
static StepArgs lw_plan_args(ssme_lw_handle h, int draw, int t, int gi, const double* tsum, const double* tmax) {
    StepArgs a{};
    a.tsum_in = tsum; a.tmax_in = tmax;
    a.l2_T = h->l2T[draw]; a.l2_R = h->l2R[draw]; a.l2_lo = h->l2lo[draw]; a.l2_hi = h->l2hi[draw];
    a.scal = h->l2s[draw];
    a.B = h->B; a.Bs = h->Bs; a.Bpow2 = h->Bpow2; a.rshift = h->rshift; a.R = h->R; a.N = h->N; a.tile = kTile;
    a.resampler = RESAMP_MULTINOMIAL; a.resamp_sched = 1;
    a.t = t; a.gi = gi; a.finalize_prev = 0;
    a.pgam = draw ? h->pgamA : h->pgamB; a.gtot = draw ? h->gtotA : h->gtotB;
    a.keyp = h->keybuf; a.first_filter = h->cfg.first_filter_id;
    a.l2_work = h->l2_work;
    return a;
}
static void lw_launch_plan(ssme_lw_handle h, int draw, int t, int gi, const double* tsum, const double* tmax, bool ranges) {
    launch_level2(h->stream, lw_plan_args(h, draw, t, gi, tsum, tmax), h->shard_world > 0 ? 1 : h->R, h->lds_bytes_plan, ranges ? 1 : 0);
}

// between the stages: theta-bar and the Cholesky factor of n_filters filters by one workgroup each (k_lw_mid); `totals`: the
// moment totals by one wave per moment first
static void lw_launch_mid(ssme_lw_handle h, LwArgs& a, int n_filters, bool totals) {
    if (totals) {
        a.momtot = h->momtot;
        hipLaunchKernelGGL(k_lw_mom_totals, dim3(kNMom, n_filters), dim3(64), 0, h->stream, a);
    }
    if (h->split_l2) hipLaunchKernelGGL(k_lw_mid<true>, dim3(n_filters), dim3(kThreads), 0, h->stream, a);
    else hipLaunchKernelGGL(k_lw_mid<false>, dim3(n_filters), dim3(kThreads), 0, h->stream, a);
}

static void lw_enqueue_step(ssme_lw_handle h, int t, int yi, int gi, bool record, bool finalize_prev, const double* yz_now = nullptr) {
    LwArgs a = lw_args(h);
    if (yz_now) { a.by_value = 1; a.y_now = yz_now[0]; a.z_now = yz_now[1]; }
    a.t = t; a.yi = yi; a.gi = gi; a.finalize_prev = finalize_prev ? 1 : 0;
    a.per_step = record ? h->per_step : nullptr;
    const dim3 grid(h->B, h->R);
    if (t == 0) {
        hipLaunchKernelGGL(k_lw_init, grid, dim3(kLwNT), 0, h->stream, a);
        return;
    }
    if (h->split_l2) {
        // a resampling draw closes step t-1 only if t % rs == 0 (lazily: it runs at the start of step t)
        lw_launch_plan(h, 0, t, gi, h->tsumB, h->tmaxB, (t % h->rs) == 0);
    } else {
        // two launches when the tile partials ([B][14] doubles) fit the window area of stage 2's LDS: every workgroup of stage 2
        // then takes theta-bar and the Cholesky factor from them itself.  Otherwise (586 .. 1024 tiles, and the split level-2):
        // the totals by one wave per moment, then the one-workgroup rest
        a.fuse_mid = ((size_t)h->B * kNMom * sizeof(double) <= h->lds_bytes) ? 1 : 0;
    }
    lw_launch_stage(h, 1, grid, a);
    if (h->split_l2 && h->form == 0) lw_launch_plan(h, 1, t, gi, h->tsumA, h->tmaxA, true);
    if (!a.fuse_mid) lw_launch_mid(h, a, h->R, true);
    lw_launch_stage(h, 2, grid, a);
    if (a.compose) { std::swap(h->xB, h->xr); std::swap(h->thB, h->thr); }      // the new population is where stage 2 wrote it
}
static void lw_enqueue_finalize(ssme_lw_handle h, int t, bool record, double* ll_host = nullptr) {
    LwArgs a = lw_args(h);
    a.t = t; a.ll_host = ll_host;
    a.per_step = record ? h->per_step : nullptr;
    if (h->split_l2) {
        lw_launch_plan(h, 0, t + 1, 0, h->tsumB, h->tmaxB, false);
        hipLaunchKernelGGL(k_lw_finalize<true>, dim3(h->R), dim3(kThreads), 0, h->stream, a);
    } else
        hipLaunchKernelGGL(k_lw_finalize<false>, dim3(h->R), dim3(kThreads), 0, h->stream, a);
}

// The one place that decides what ssme_lw_run_series launches (it and ssme_lw_get_series_route ask here): the whole-series kernel
// for an unsharded handle of one tile with small series enabled, the tiled stage launches otherwise.
constexpr int kLwSmallSeriesDefault = 1;     // the default route of a new handle, by the rule and the figures of profiles/lw_series_timing.txt
static int lw_series_route(const ssme_lw_s* h) {
    return (h->shard_world == 0 && h->B == 1 && h->small_series) ? SSME_ROUTE_LW_SERIES : SSME_ROUTE_TILED;
}
static const void* lw_series_kernel(bool ft, bool rec) {
    static const void* const tab[2][2] = {
        {reinterpret_cast<const void*>(&k_lw_series<false>), reinterpret_cast<const void*>(&k_lw_series<true>)},
        {reinterpret_cast<const void*>(&k_lw_series<false, LwSeriesRec>), reinterpret_cast<const void*>(&k_lw_series<true, LwSeriesRec>)}};
    return tab[rec][ft];
}
// steps 1 .. T-1, the accounting of every step and the hand-over, behind k_lw_init; a recording handle: rows 0 .. T-1 of the trajectory
static void lw_launch_series(ssme_lw_handle h, int T) {
    LwArgs a = lw_args(h);
    a.per_step = h->per_step;
    LwSeriesRec rec = {h->traj};
    void* args[] = {&a, &T, &rec};           // (the non-recording instantiations take the first two)
    hipLaunchKernel(lw_series_kernel(h->fixed_trans, h->rec_series), dim3(h->R), dim3(kLwNT), args, kLwSeriesLdsBytes, h->stream);
}
// The trajectory buffer for T time rows while recording is on; the first non-recording run_series frees it.  Nothing counts as
// recorded until the series has been queued.
static int lw_ensure_trajectory(ssme_lw_handle h, int T) {
    h->traj_T = 0;
    if (!h->rec_series) {
        own_free(h, h->traj);
        h->traj_cap = 0;
        return SSME_OK;
    }
    if (T > h->traj_cap) {
        h->traj_cap = 0;                     // capacity 0 while the buffer is replaced: a failed allocation leaves none
        HIPCHK(own_alloc(h, h->traj, sizeof(double) * (size_t)T * h->R * kLwNExp));
        h->traj_cap = T;
    }
    return SSME_OK;
}
// tiled route, recording: the step API's read-out behind step t, with row t of the trajectory as its output.  The per-tile moment
// scratch is free between steps (stage 1 rewrites it before k_lw_mid reads it), and the buffers of step t are `xB` / `thB` by now.
static void lw_enqueue_expect_row(ssme_lw_handle h, int t) {
    LwArgs a = lw_args(h);
    hipLaunchKernelGGL(k_lw_param_partials, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, a);
    hipLaunchKernelGGL(k_lw_param_means, dim3(h->R), dim3(kWave), 0, h->stream, a, h->traj + (size_t)t * h->R * kLwNExp);
}

static int lw_reset(ssme_lw_handle h) {
    std::vector<LwScalars> sc(h->R);
    const double logN = dlog((double)h->N);
    for (auto& s : sc) { std::memset(&s, 0, sizeof(s)); s.prev = logN; }
    HIPCHK(hipMemcpyAsync(h->scal, sc.data(), sizeof(LwScalars) * h->R, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->t = 0;
    h->gamma_rows = 0;
    return SSME_OK;
}

extern "C" {

int ssme_lw_destroy(ssme_lw_handle h) {
    if (!h) return SSME_ERR_INVALID_ARG;
    hipSetDevice(h->cfg.device);
    release_core(h);
    delete h;
    return SSME_OK;
}

static int lw_create_impl(const ssme_lw_config* cfg, int shard_rank, int shard_world, ssme_lw_handle* out) {
    if (!cfg || !out) return SSME_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->n_particles < 1 || cfg->n_filters < 1 || cfg->n_filters > 65535) return SSME_ERR_INVALID_ARG;
    if (!(cfg->delta > 0.0 && cfg->delta <= 1.0)) return SSME_ERR_INVALID_ARG;
    if (cfg->form < 0 || cfg->form > 1 || cfg->resamp_sched < 0) return SSME_ERR_INVALID_ARG;
    for (int d = 0; d < kDP; ++d) {
        if (cfg->transforms[d] < 0 || cfg->transforms[d] > 3) return SSME_ERR_INVALID_ARG;     // parameters.h:283 invalid_argument
        if (!(cfg->prior_lo[d] <= cfg->prior_hi[d])) return SSME_ERR_INVALID_ARG;
    }
    ssme_lw_handle h = new (std::nothrow) ssme_lw_s();
    if (!h) return SSME_ERR_INVALID_ARG;
    set_layout(h, cfg->n_particles, cfg->n_filters, kTile, shard_rank, shard_world);
    if (h->B > kMaxTilesSplit) { delete h; return SSME_ERR_UNSUPPORTED; }          // N <= 2^25
    h->cfg = *cfg;
    h->form = cfg->form; h->rs = cfg->resamp_sched < 1 ? 1 : cfg->resamp_sched;
    h->small_series = kLwSmallSeriesDefault;
    h->fixed_trans = (cfg->transforms[0] == TR_LOGIT && cfg->transforms[1] == TR_NULL && cfg->transforms[2] == TR_LOG && cfg->transforms[3] == TR_TWICE_FISHER) ? 1 : 0;
    if (hipSetDevice(cfg->device) != hipSuccess) { delete h; return SSME_ERR_HIP; }
    int rc = [&]() -> int {
        int rc2 = create_stream(h);
        if (rc2 != SSME_OK) return rc2;
        const size_t np = (size_t)h->R * h->Npad, nb = (size_t)h->R * h->Bs;
        HIPCHK(own_alloc(h, h->l2_work, sizeof(double) * (nb + (size_t)h->R * kL2Scratch + 32), Mem::zeroed));
        for (int d = 0; d < 2; ++d) {
            HIPCHK(own_alloc(h, h->l2T[d], sizeof(double) * nb));
            HIPCHK(own_alloc(h, h->l2R[d], sizeof(double) * nb));
            HIPCHK(own_alloc(h, h->l2lo[d], sizeof(int32_t) * nb, Mem::zeroed));
            HIPCHK(own_alloc(h, h->l2hi[d], sizeof(int32_t) * nb, Mem::zeroed));
            HIPCHK(own_alloc(h, h->l2s[d], sizeof(FilterScalars) * (size_t)h->R, Mem::zeroed));
        }
        HIPCHK(grant_plan_lds(h, cfg->device));
        for (int stage = 1; stage <= 2; ++stage)
            for (int big = 0; big < 2; ++big)
                for (int ft = 0; ft < 2; ++ft)
                    HIPCHK(grant_lds(lw_stage_kernel(stage, big, ft), big ? h->lds_bytes_big : h->lds_bytes, cfg->device));
        if (h->shard_world == 0 && h->B == 1)
            for (int ft = 0; ft < 2; ++ft)
                for (int rec = 0; rec < 2; ++rec) HIPCHK(grant_lds(lw_series_kernel(ft, rec), kLwSeriesLdsBytes, cfg->device));
        if (h->shard_world == 0) {               // a sharded handle works on the caller's buffers
            for (double** p : {&h->xB, &h->xr, &h->lw1, &h->cdfA, &h->cdfB}) HIPCHK(own_alloc(h, *p, sizeof(double) * np, Mem::zeroed));
            if (h->rs > 1) HIPCHK(own_alloc(h, h->lwB, sizeof(double) * np, Mem::zeroed));
            for (double** p : {&h->thB, &h->thr}) HIPCHK(own_alloc(h, *p, sizeof(double) * np * kDP, Mem::zeroed));
            for (double** p : {&h->tsumA, &h->tmaxA, &h->tsumB, &h->tmaxB}) HIPCHK(own_alloc(h, *p, sizeof(double) * nb, Mem::zeroed));
            HIPCHK(own_alloc(h, h->ancbuf, sizeof(uint32_t) * np, Mem::zeroed));
        } else {
            if ((rc2 = alloc_plan_buffers(h)) != SSME_OK) return rc2;
            if (h->rs > 1)                       // the carried second-stage log-weights of this rank's own particles (local offsets)
                HIPCHK(own_alloc(h, h->lwB, sizeof(double) * (size_t)h->sh_Bl * kTile, Mem::zeroed));
        }
        HIPCHK(own_alloc(h, h->mom, sizeof(double) * (size_t)h->R * h->B * 16));
        HIPCHK(own_alloc(h, h->prop, sizeof(double) * (size_t)h->R * 16, Mem::zeroed));
        HIPCHK(own_alloc(h, h->momtot, sizeof(double) * (size_t)h->R * 16));
        HIPCHK(own_alloc(h, h->scal, sizeof(LwScalars) * h->R));
        HIPCHK(own_alloc(h, h->scratch, sizeof(double) * h->R * kLwNExp));
        HIPCHK(own_alloc(h, h->pin, sizeof(double) * (size_t)h->R, Mem::pinned));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pin_dev), h->pin, 0));
        HIPCHK(own_alloc(h, h->keybuf, sizeof(uint32_t) * 2));
        {
            const uint32_t k[2] = {(uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32)};
            HIPCHK(hipMemcpy(h->keybuf, k, sizeof(k), hipMemcpyHostToDevice));
        }
        rc2 = lw_ensure_capacity(h, 1);
        if (rc2 != SSME_OK) return rc2;
        return lw_reset(h);
    }();
    if (rc != SSME_OK) { ssme_lw_destroy(h); return rc; }
    *out = h;
    return SSME_OK;
}

int ssme_lw_create(const ssme_lw_config* cfg, ssme_lw_handle* out) { return lw_create_impl(cfg, 0, 0, out); }

// ---- particle-sharded Liu-West filter: one filter over `world` GPUs (BASELINE.json configs[4]) ------------------------
// Same scheme as ssme_pf_shard_* with two exchanges per step: the resampling draw reads windows of (cdfB, x, theta) and the
// k draw windows of (cdfA, lw1, x, theta); the 14 moment partials of every tile are gathered like the tile sums and summed
// in tile order by every rank (k_lw_mid), so theta-bar, the Cholesky factor and all draws equal the unsharded filter's.
int ssme_lw_shard_create(const ssme_lw_config* cfg, int32_t rank, int32_t world, ssme_lw_handle* out) {
    if (!cfg || !out) return SSME_ERR_INVALID_ARG;
    const int rc = shard_create_check(cfg->n_particles, cfg->n_filters, rank, world);
    return rc != SSME_OK ? rc : lw_create_impl(cfg, rank, world, out);
}

int ssme_lw_shard_layout(ssme_lw_handle h, int32_t* out4) { return shard_layout(h, out4); }

int ssme_lw_set_stream(ssme_lw_handle h, void* hip_stream) { return set_stream(h, hip_stream); }

int ssme_lw_shard_prepare(ssme_lw_handle h, const double* y, const double* z, int32_t T) {
    if (!h || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    if (T < 1) return SSME_ERR_LENGTH;
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = lw_ensure_capacity(h, T);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->ybuf, y, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    if (z) HIPCHK(hipMemcpyAsync(h->zbuf, z, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(hipMemsetAsync(h->zbuf, 0, sizeof(double) * T, h->stream));
    rc = lw_reset(h);
    if (rc != SSME_OK) return rc;
    lw_launch_gamma(h, 0, T);
    HIPCHK(hipGetLastError());
    return SSME_OK;
}

// check_halo (the native driver's stages on the fixed halo): the source windows are whole halo buffers, and the stage kernel
// verifies its source tiles against them (LwArgs::win_tiles / win_flag)
static LwArgs lw_shard_args(ssme_lw_handle h, int t, bool check_halo = false) {
    LwArgs a = lw_args(h);
    a.t = t; a.yi = t; a.gi = t; a.finalize_prev = t >= 1 ? 1 : 0;
    a.per_step = h->per_step;
    a.tile0 = h->shard_rank * h->sh_Bl;
    a.anc = nullptr; a.kidx = nullptr;
    if (check_halo) { a.win_tiles = h->sh_rows; a.win_flag = h->sh_flag; }
    return a;
}

int ssme_lw_shard_init(ssme_lw_handle h, double* xB, double* thB, double* cdfB, double* tsumB, double* tmaxB) {
    if (!h || !xB || !thB || !cdfB || !tsumB || !tmaxB) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    LwArgs a = lw_shard_args(h, 0);
    a.xB = xB; a.thB = thB; a.cdfB = cdfB; a.tsumB = tsumB; a.tmaxB = tmaxB;
    hipLaunchKernelGGL(k_lw_init, dim3(h->sh_Bown, 1), dim3(kLwNT), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    h->t = 1;
    return SSME_OK;
}

// which = 0: the resampling draw of stage 1 (second-stage weights, Gamma tables B); 1: the k draw of stage 2 (first-stage weights)
int ssme_lw_shard_plan(ssme_lw_handle h, int32_t which, int32_t t, const double* tsum_all, const double* tmax_all, int32_t* lo_hi) {
    if (!h || !tsum_all || !tmax_all || !lo_hi || t < 1 || which < 0 || which > 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->split_l2)
        lw_launch_plan(h, which, t, t, tsum_all, tmax_all, true);
    else
        hipLaunchKernelGGL(k_shard_plan, dim3(1), dim3(512), sizeof(double) * (h->Bpow2 < 2 ? 2 : h->Bpow2), h->stream,
                           lw_plan_args(h, which, t, t, tsum_all, tmax_all), h->shard_world, h->sh_Bl, h->plan_dev);
    HIPCHK(hipGetLastError());
    return shard_plan_to_host(h, false, h->l2lo[which], h->l2hi[which], lo_hi);
}

// Stage 1 of step t on this rank's tiles: sources in the windows that start at global tile win_tile0, outputs in the caller's buffers
static int lw_shard_launch_stage1(ssme_lw_handle h, int t, int win_tile0, const double* w_xB, const double* w_thB, const double* w_cdfB,
                                  const double* tsumB_all, const double* tmaxB_all, double* xr, double* thr, double* lw1, double* cdfA,
                                  double* tsumA, double* tmaxA, double* mom, uint32_t* anc, bool check_halo) {
    LwArgs a = lw_shard_args(h, t, check_halo);
    a.xB = const_cast<double*>(w_xB); a.thB = const_cast<double*>(w_thB); a.cdfB = const_cast<double*>(w_cdfB);
    a.tsumB = const_cast<double*>(tsumB_all); a.tmaxB = const_cast<double*>(tmaxB_all);
    a.win_tile0 = win_tile0;
    a.xr = xr; a.thr = thr; a.lw1 = lw1; a.cdfA = cdfA; a.tsumA = tsumA; a.tmaxA = tmaxA; a.mom = mom;
    a.anc = anc;
    lw_launch_stage(h, 1, dim3(h->sh_Bown, 1), a);
    HIPCHK(hipGetLastError());
    return SSME_OK;
}

// (win_tiles of the two stage calls is validated and not read: the window's first tile is all a stage kernel needs)
int ssme_lw_shard_stage1(ssme_lw_handle h, int32_t t, int32_t win_tile0, int32_t win_tiles, const double* w_xB, const double* w_thB,
                         const double* w_cdfB, const double* tsumB_all, const double* tmaxB_all, double* xr, double* thr, double* lw1,
                         double* cdfA, double* tsumA, double* tmaxA, double* mom, uint32_t* anc) {
    if (!h || t < 1 || win_tile0 < -h->sh_margin || win_tiles < 1 || !w_xB || !w_thB || !w_cdfB || !tsumB_all || !tmaxB_all || !xr || !thr || !lw1 ||
        !cdfA || !tsumA || !tmaxA || !mom)
        return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    if (t >= h->tcap) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    return lw_shard_launch_stage1(h, t, win_tile0, w_xB, w_thB, w_cdfB, tsumB_all, tmaxB_all, xr, thr, lw1, cdfA, tsumA, tmaxA, mom, anc, false);
}

int ssme_lw_shard_mid(ssme_lw_handle h, int32_t t, const double* tsumA_all, const double* tmaxA_all, const double* mom_all) {
    if (!h || t < 1 || !tsumA_all || !tmaxA_all || !mom_all) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    LwArgs a = lw_shard_args(h, t);
    a.tsumA = const_cast<double*>(tsumA_all); a.tmaxA = const_cast<double*>(tmaxA_all); a.mom = const_cast<double*>(mom_all);
    // split level-2: the plan of the k draw (ssme_lw_shard_plan(which = 1)) must precede this call -- it provides m and S
    lw_launch_mid(h, a, 1, h->split_l2 || h->B > 256);
    HIPCHK(hipGetLastError());
    return SSME_OK;
}

// Stage 2 of step t, likewise
static int lw_shard_launch_stage2(ssme_lw_handle h, int t, int win_tile0, const double* w_xr, const double* w_thr, const double* w_lw1,
                                  const double* w_cdfA, const double* tsumA_all, const double* tmaxA_all, double* xB, double* thB,
                                  double* cdfB, double* tsumB, double* tmaxB, uint32_t* kidx, bool check_halo) {
    LwArgs a = lw_shard_args(h, t, check_halo);
    a.xr = const_cast<double*>(w_xr); a.thr = const_cast<double*>(w_thr); a.lw1 = const_cast<double*>(w_lw1);
    a.cdfA = const_cast<double*>(w_cdfA); a.tsumA = const_cast<double*>(tsumA_all); a.tmaxA = const_cast<double*>(tmaxA_all);
    a.win_tile0 = win_tile0;
    a.xB = xB; a.thB = thB; a.cdfB = cdfB; a.tsumB = tsumB; a.tmaxB = tmaxB;
    a.kidx = kidx;
    lw_launch_stage(h, 2, dim3(h->sh_Bown, 1), a);
    HIPCHK(hipGetLastError());
    h->t = t + 1;
    return SSME_OK;
}

int ssme_lw_shard_stage2(ssme_lw_handle h, int32_t t, int32_t win_tile0, int32_t win_tiles, const double* w_xr, const double* w_thr,
                         const double* w_lw1, const double* w_cdfA, const double* tsumA_all, const double* tmaxA_all, double* xB,
                         double* thB, double* cdfB, double* tsumB, double* tmaxB, uint32_t* kidx) {
    if (!h || t < 1 || win_tile0 < -h->sh_margin || win_tiles < 1 || !w_xr || !w_thr || !w_lw1 || !w_cdfA || !tsumA_all || !tmaxA_all || !xB || !thB ||
        !cdfB || !tsumB || !tmaxB)
        return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    return lw_shard_launch_stage2(h, t, win_tile0, w_xr, w_thr, w_lw1, w_cdfA, tsumA_all, tmaxA_all, xB, thB, cdfB, tsumB, tmaxB, kidx, false);
}

int ssme_lw_shard_finalize(ssme_lw_handle h, int32_t t, const double* tsumB_all, const double* tmaxB_all) {
    if (!h || t < 0 || !tsumB_all || !tmaxB_all) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    LwArgs a = lw_shard_args(h, t);
    a.tsumB = const_cast<double*>(tsumB_all); a.tmaxB = const_cast<double*>(tmaxB_all);
    if (h->split_l2) {
        lw_launch_plan(h, 0, t + 1, 0, tsumB_all, tmaxB_all, false);
        hipLaunchKernelGGL(k_lw_finalize<true>, dim3(1), dim3(kThreads), 0, h->stream, a);
    } else
        hipLaunchKernelGGL(k_lw_finalize<false>, dim3(1), dim3(kThreads), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return SSME_OK;
}

// ---- C++ driver of the sharded Liu-West filter over RCCL (BASELINE.json configs[4]; fixed-halo path) ------------------------
// Per step, on one HIP stream, no host synchronisation inside the time loop:
//   grouped all-gather (tsumB, tmaxB)  [-> plan(0) above 1024 tiles]  -> halo exchange of (xB, theta B, cdfB)  -> stage 1
//   grouped all-gather (tsumA, tmaxA, 16 moment slots per tile)  [-> plan(1)]  -> mid  -> halo exchange of (xr, theta r, g1, cdfA)  -> stage 2
// The stage kernels check their own source tiles against the exchanged window and raise a flag (read once, after the
// series): SSME_ERR_STATE then tells the caller to run the exact, host-planned loop (ssme_amd/sharded.py: ShardedLiuWest).

static int lw_shard_alloc(ssme_lw_handle h) {
    if (h->sh_xB) return SSME_OK;
    const int Bl = h->sh_Bl;
    h->sh_margin = halo_margin(Bl, h->shard_world); h->sh_rows = Bl + 2 * h->sh_margin;
    const size_t rows = sizeof(double) * kTile * h->sh_rows, nall = gathered_len(h);
    for (double** p : {&h->sh_xB, &h->sh_cdfB, &h->sh_xr, &h->sh_g1, &h->sh_cdfA}) HIPCHK(own_alloc(h, *p, rows, Mem::zeroed));
    for (double** p : {&h->sh_thB, &h->sh_thr}) HIPCHK(own_alloc(h, *p, rows * kDP, Mem::zeroed));
    HIPCHK(own_alloc(h, h->sh_locB, sizeof(double) * 2 * Bl, Mem::zeroed));
    HIPCHK(own_alloc(h, h->sh_locA, sizeof(double) * 18 * Bl, Mem::zeroed));        // tile sums | tile maxima | 16 moment slots per tile
    for (double** p : {&h->sh_allB_s, &h->sh_allB_m, &h->sh_allA_s, &h->sh_allA_m}) HIPCHK(own_alloc(h, *p, sizeof(double) * nall));
    HIPCHK(own_alloc(h, h->sh_mom_all, sizeof(double) * nall * 16));
    HIPCHK(own_alloc(h, h->sh_flag, sizeof(int32_t) * 4));
    return SSME_OK;
}

int ssme_lw_shard_run_series(ssme_lw_handle h, void* nccl_comm, const double* y, const double* z, int32_t T, double* loglik_out) {
    if (!h || !nccl_comm || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1) return SSME_ERR_STATE;
    if (T < 1) return SSME_ERR_LENGTH;
    HIPCHK(hipSetDevice(h->cfg.device));
    ncclComm_t comm;
    int rc = lw_shard_alloc(h);
    if (rc == SSME_OK) rc = native_begin(h, nccl_comm, &comm);
    if (rc != SSME_OK) return rc;
    const int Bl = h->sh_Bl, m = h->sh_margin, tile0 = h->shard_rank * Bl;
    const size_t TL = kTile, off = (size_t)m * TL;
    rc = ssme_lw_shard_prepare(h, y, z, T);
    if (rc != SSME_OK) return rc;
    double *tsB = h->sh_locB, *tmB = h->sh_locB + Bl;
    double *tsA = h->sh_locA, *tmA = h->sh_locA + Bl, *momL = h->sh_locA + 2 * Bl;
    auto gatherB = [&] { return all_gather(h, comm, {{tsB, h->sh_allB_s, (size_t)Bl}, {tmB, h->sh_allB_m, (size_t)Bl}}); };
    rc = ssme_lw_shard_init(h, h->sh_xB + off, h->sh_thB + off * kDP, h->sh_cdfB + off, tsB, tmB);
    if (rc != SSME_OK) return rc;
    for (int t = 1; t < T; ++t) {
        // resampling schedule m_rs (liu_west_filter.h:1139-1140): a draw closes step t - 1 only if t % m_rs == 0; otherwise every
        // particle continues itself with its carried second-stage weight -- stage 1 reads this rank's own rows, nothing travels
        const bool resampled = (t % h->rs) == 0;
        rc = gatherB();
        if (rc != SSME_OK) return rc;
        if (h->split_l2) { lw_launch_plan(h, 0, t, t, h->sh_allB_s, h->sh_allB_m, resampled); HIPCHK(hipGetLastError()); }
        if (resampled) {
            rc = halo_exchange(h, comm, {{h->sh_xB, TL}, {h->sh_thB, TL * kDP}, {h->sh_cdfB, TL}});
            if (rc != SSME_OK) return rc;
        }
        const size_t src = resampled ? 0 : off;                   // the whole halo buffers, or this rank's own rows
        rc = lw_shard_launch_stage1(h, t, resampled ? tile0 - m : tile0, h->sh_xB + src, h->sh_thB + src * kDP, h->sh_cdfB + src, h->sh_allB_s,
                                    h->sh_allB_m, h->sh_xr + off, h->sh_thr + off * kDP, h->sh_g1 + off, h->sh_cdfA + off, tsA, tmA, momL, nullptr,
                                    /*check_halo=*/resampled);
        if (rc != SSME_OK) return rc;
        rc = all_gather(h, comm, {{tsA, h->sh_allA_s, (size_t)Bl}, {tmA, h->sh_allA_m, (size_t)Bl}, {momL, h->sh_mom_all, (size_t)Bl * 16}});
        if (rc != SSME_OK) return rc;
        // the plan of the k draw first: above 1024 tiles it provides the (m, S) that mid turns into the first-stage log-sum-exp
        // (SISR form, form 1: no first-stage weights and no k draw -- every particle continues itself, so stage 2 reads this
        //  rank's own stage-1 outputs and the second exchange does not exist: ONE exchange per step)
        if (h->split_l2 && h->form == 0) { lw_launch_plan(h, 1, t, t, h->sh_allA_s, h->sh_allA_m, true); HIPCHK(hipGetLastError()); }
        rc = ssme_lw_shard_mid(h, t, h->sh_allA_s, h->sh_allA_m, h->sh_mom_all);
        if (rc != SSME_OK) return rc;
        if (h->form == 0) {
            rc = halo_exchange(h, comm, {{h->sh_xr, TL}, {h->sh_thr, TL * kDP}, {h->sh_g1, TL}, {h->sh_cdfA, TL}});
            if (rc != SSME_OK) return rc;
        }
        rc = lw_shard_launch_stage2(h, t, tile0 - m, h->sh_xr, h->sh_thr, h->sh_g1, h->sh_cdfA, h->sh_allA_s, h->sh_allA_m,
                                    h->sh_xB + off, h->sh_thB + off * kDP, h->sh_cdfB + off, tsB, tmB, nullptr, /*check_halo=*/true);
        if (rc != SSME_OK) return rc;
    }
    rc = gatherB();
    if (rc != SSME_OK) return rc;
    rc = ssme_lw_shard_finalize(h, T - 1, h->sh_allB_s, h->sh_allB_m);           // synchronises
    if (rc != SSME_OK) return rc;
    bool overflow = false;
    rc = reduce_flags(h, comm, &overflow);
    if (rc != SSME_OK) return rc;
    if (overflow) { h->err = "a resampling window left the fixed halo on some rank: run the exact host-planned loop"; return SSME_ERR_STATE; }
    if (loglik_out) return ssme_lw_get_loglik(h, loglik_out);
    return SSME_OK;
}

// this rank's particles and transformed parameters (theta[d * n + i]) after ssme_lw_shard_run_series
int ssme_lw_shard_download(ssme_lw_handle h, double* x_local, double* theta_local, int64_t* exchanged_tiles) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (h->shard_world < 1 || !h->sh_xB) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t off = (size_t)h->sh_margin * kTile, n = own_particles(h);
    if (x_local) HIPCHK(hipMemcpy(x_local, h->sh_xB + off, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (theta_local) {
        std::vector<double> rec(n * kDP);
        HIPCHK(hipMemcpy(rec.data(), h->sh_thB + off * kDP, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) for (int d = 0; d < kDP; ++d) theta_local[(size_t)d * n + i] = rec[i * kDP + d];
    }
    if (exchanged_tiles) *exchanged_tiles = h->sh_exchanged;
    return SSME_OK;
}

int ssme_lw_shard_stats(ssme_lw_handle h, int32_t* out4) { return shard_stats(h, h && h->sh_xB, out4); }

int ssme_lw_get_loglik(ssme_lw_handle h, double* out) {
    if (!h || !out) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    return read_loglik(h, out);
}

int ssme_lw_reset(ssme_lw_handle h) {
    if (!h) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    return lw_reset(h);
}

int ssme_lw_set_debug(ssme_lw_handle h, int32_t flags) {
    if (!h) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0 && (flags & 1)) return SSME_ERR_STATE;   // index recording needs the handle's own buffers
    HIPCHK(hipSetDevice(h->cfg.device));
    if ((flags & 1) && !h->anc) {
        HIPCHK(own_alloc(h, h->anc, sizeof(uint32_t) * (size_t)h->R * h->Npad, Mem::zeroed));
        HIPCHK(own_alloc(h, h->kidx, sizeof(uint32_t) * (size_t)h->R * h->Npad, Mem::zeroed));
    }
    h->debug = flags;
    h->split_l2 = (h->B > kMaxTilesPerFilter || (flags & 4)) ? 1 : ((flags & 8) ? 0 : (h->B > kSplitLevel2Above ? 1 : 0));
    return SSME_OK;
}

int ssme_lw_set_small_series(ssme_lw_handle h, int32_t enable) {
    if (!h || enable < 0 || enable > 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles are driven by ssme_lw_shard_*
    h->small_series = enable;
    return SSME_OK;
}

int ssme_lw_get_series_route(ssme_lw_handle h, int32_t* route, int32_t* threads_per_block) {
    if (!h || !route || !threads_per_block) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    *route = lw_series_route(h);
    *threads_per_block = kLwNT;
    return SSME_OK;
}

int ssme_lw_step(ssme_lw_handle h, const double* y, const double* z, double* out) {
    if (!h || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles own no particle buffers: ssme_lw_shard_* drives them
    HIPCHK(hipSetDevice(h->cfg.device));
    const double z0 = z ? *z : 0.0;
    if (h->gcap < kStepGammaChunk) {
        int rc = lw_ensure_gamma(h, kStepGammaChunk);
        if (rc != SSME_OK) return rc;
    }
    // y and z travel in the kernel arguments, the R results come back through device-mapped pinned memory written by the
    // accounting kernel: no copy operation in either direction
    const double yz[2] = {*y, z0};
    const int gi = h->t > 0 ? step_gamma_row(h, lw_launch_gamma) : 0;      // Gamma tables of both draws
    mark_results_pending(h->pin, h->R);
    lw_enqueue_step(h, h->t, 0, gi, false, /*finalize_prev=*/false, yz);
    lw_enqueue_finalize(h, h->t, false, h->pin_dev);          // the step API accounts each step right away
    HIPCHK(hipGetLastError());
    HIPCHK(wait_results(h->stream, h->pin, h->R));
    if (out) for (int r = 0; r < h->R; ++r) out[r] = h->pin[r];
    h->t += 1;
    return SSME_OK;
}

int ssme_lw_run_series(ssme_lw_handle h, const double* y, const double* z, int32_t T, double* loglik_out) {
    if (!h || !y) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles own no particle buffers: ssme_lw_shard_* drives them
    if (T < 1) return SSME_ERR_LENGTH;
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = lw_ensure_capacity(h, T);
    if (rc == SSME_OK) rc = lw_ensure_trajectory(h, T);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->ybuf, y, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    if (z) HIPCHK(hipMemcpyAsync(h->zbuf, z, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(hipMemsetAsync(h->zbuf, 0, sizeof(double) * T, h->stream));
    rc = lw_reset(h);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    lw_launch_gamma(h, 0, T);
    if (lw_series_route(h) == SSME_ROUTE_LW_SERIES) {
        lw_enqueue_step(h, 0, 0, 0, true, false);             // k_lw_init
        lw_launch_series(h, T);
    } else {
        for (int t = 0; t < T; ++t) {
            lw_enqueue_step(h, t, t, t, true, /*finalize_prev=*/t > 0);
            if (h->rec_series) lw_enqueue_expect_row(h, t);
        }
        lw_enqueue_finalize(h, T - 1, true);
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipGetLastError());
    h->t = T;
    if (h->rec_series) h->traj_T = T;
    rc = read_loglik(h, loglik_out);
    if (rc != SSME_OK) return rc;
    HIPCHK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    return SSME_OK;
}

int ssme_lw_get_per_step(ssme_lw_handle h, double* out, int32_t T) { return read_per_step(h, out, T); }

// the table's slot of a functional id: ids 0-3: x, x^2, exp(x/2), 42; 4-7: phi, mu, sigma, rho
static const int kLwExpectSlot[8] = {4, 5, 6, 7, 0, 1, 2, 3};
// [R][8] on the host: E[theta_d] (4), E[x], E[x^2], E[exp(x/2)], E[42] under the last step's weights
static int lw_expect_table(ssme_lw_handle h, std::vector<double>& tab) {
    LwArgs a = lw_args(h);
    // the per-tile moment scratch is free between steps (stage 1 rewrites it before k_lw_mid reads it)
    hipLaunchKernelGGL(k_lw_param_partials, dim3(h->B, h->R), dim3(kThreads), 0, h->stream, a);
    hipLaunchKernelGGL(k_lw_param_means, dim3(h->R), dim3(kWave), 0, h->stream, a, h->scratch);
    HIPCHK(hipGetLastError());
    tab.resize((size_t)h->R * kLwNExp);
    HIPCHK(hipMemcpyAsync(tab.data(), h->scratch, sizeof(double) * tab.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SSME_OK;
}

int ssme_lw_get_param_means(ssme_lw_handle h, double* out) {
    if (!h || !out) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles own no particle buffers: ssme_lw_shard_* drives them
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    std::vector<double> tab;
    int rc = lw_expect_table(h, tab);
    if (rc != SSME_OK) return rc;
    for (int r = 0; r < h->R; ++r) for (int d = 0; d < kDP; ++d) out[(size_t)r * kDP + d] = tab[(size_t)r * kLwNExp + d];
    return SSME_OK;
}

int ssme_lw_get_expectations(ssme_lw_handle h, const int32_t* functionals, int32_t n, double* out) {
    if (!h || !out || !functionals || n < 1) return SSME_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) if (functionals[i] < 0 || functionals[i] > 7) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    std::vector<double> tab;
    int rc = lw_expect_table(h, tab);
    if (rc != SSME_OK) return rc;
    for (int i = 0; i < n; ++i) for (int r = 0; r < h->R; ++r) out[(size_t)i * h->R + r] = tab[(size_t)r * kLwNExp + kLwExpectSlot[functionals[i]]];
    return SSME_OK;
}

int ssme_lw_set_series_expectations(ssme_lw_handle h, int32_t enable) {
    if (!h || enable < 0 || enable > 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles are driven by ssme_lw_shard_*
    // the trajectory buffer follows at the next run_series (lw_ensure_trajectory), which also frees it once recording is off
    h->rec_series = enable;
    return SSME_OK;
}

int ssme_lw_get_series_expectations(ssme_lw_handle h, const int32_t* functionals, int32_t n, double* out, int32_t T) {
    if (!h || !out || !functionals || n < 1 || n > kLwNExp) return SSME_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) if (functionals[i] < 0 || functionals[i] > 7) return SSME_ERR_INVALID_ARG;
    if (T < 1) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->traj_T < 1) { h->err = "no recorded series: ssme_lw_set_series_expectations(1), then ssme_lw_run_series"; return SSME_ERR_STATE; }
    if (T > h->traj_T) return SSME_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->cfg.device));
    std::vector<double> tab((size_t)T * h->R * kLwNExp);
    HIPCHK(hipMemcpyAsync(tab.data(), h->traj, sizeof(double) * tab.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < n; ++i)
            for (int r = 0; r < h->R; ++r)
                out[((size_t)t * n + i) * h->R + r] = tab[((size_t)t * h->R + r) * kLwNExp + kLwExpectSlot[functionals[i]]];
    return SSME_OK;
}

int ssme_lw_download_weights(ssme_lw_handle h, int32_t f, double* x, double* theta_untrans, double* w) {
    if (!h || f < 0 || f >= h->R || !w) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;
    if (h->t < 1) return SSME_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->wscratch) HIPCHK(own_alloc(h, h->wscratch, sizeof(double) * (size_t)h->Npad * (1 + kDP)));
    LwArgs a = lw_args(h);
    hipLaunchKernelGGL(k_lw_weights, dim3(h->B), dim3(kThreads), 0, h->stream, a, (int)f, h->wscratch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w, h->wscratch, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    if (theta_untrans) for (int d = 0; d < kDP; ++d)
        HIPCHK(hipMemcpyAsync(theta_untrans + (size_t)d * h->N, h->wscratch + (size_t)(1 + d) * h->Npad, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    if (x) HIPCHK(hipMemcpyAsync(x, h->xB + (size_t)f * h->Npad, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SSME_OK;
}

int ssme_lw_download_state(ssme_lw_handle h, int32_t f, double* x, double* theta, uint32_t* kidx, uint32_t* anc, double* thetabar,
                           double* chol) {
    if (!h || f < 0 || f >= h->R) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) return SSME_ERR_STATE;     // sharded handles own no particle buffers: ssme_lw_shard_* drives them
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t off = (size_t)f * h->Npad;
    if (x) HIPCHK(hipMemcpyAsync(x, h->xB + off, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    std::vector<double> rec;                       // the device keeps one [4]-record per particle; callers get parameter planes
    if (theta) {
        rec.resize((size_t)h->N * kDP);
        HIPCHK(hipMemcpyAsync(rec.data(), h->thB + (size_t)f * h->Npad * kDP, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, h->stream));
    }
    if (kidx || anc) {
        if (!h->anc) return SSME_ERR_STATE;
        if (kidx) HIPCHK(hipMemcpyAsync(kidx, h->kidx + off, sizeof(uint32_t) * h->N, hipMemcpyDeviceToHost, h->stream));
        if (anc) HIPCHK(hipMemcpyAsync(anc, h->anc + off, sizeof(uint32_t) * h->N, hipMemcpyDeviceToHost, h->stream));
    }
    double p[16];
    HIPCHK(hipMemcpyAsync(p, h->prop + (size_t)f * 16, sizeof(p), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (theta) for (int i = 0; i < h->N; ++i) for (int d = 0; d < kDP; ++d) theta[(size_t)d * h->N + i] = rec[(size_t)i * kDP + d];
    if (thetabar) for (int d = 0; d < kDP; ++d) thetabar[d] = p[d];
    if (chol) { int q = kDP; for (int d = 0; d < kDP; ++d) for (int e = 0; e < kDP; ++e) chol[d * kDP + e] = (e <= d) ? p[q++] : 0.0; }
    return SSME_OK;
}

// Liu-West forecast (forecast.h): start draw with the parameter records and their moment partials, moment
// totals and proposal components by the filter's own kernels / function, then all horizons in one launch
int ssme_lw_sim_future_obs(ssme_lw_handle h, int32_t num_steps, const double* last_obs, double* y_out, double* x_out,
                           uint32_t* start_out, double* prop_out) {
    if (!h || !y_out || !last_obs || num_steps < 1 || num_steps > kFcMaxSteps) return SSME_ERR_INVALID_ARG;
    if (h->shard_world > 0) { h->err = "forecasts of particle-sharded filters are not implemented"; return SSME_ERR_UNSUPPORTED; }
    if (h->t < 1) { h->err = "sim_future_obs before the first step"; return SSME_ERR_STATE; }
    const int H = num_steps, R = h->R, N = h->N;
    const size_t Ns = (N + 1) & ~1, rows = (size_t)R * H;
    h->fc.h_last_obs.assign(last_obs, last_obs + R);
    int rc = forecast_prepare(h, 1, rows * Ns, x_out ? rows * Ns : 0);
    if (rc != SSME_OK) return rc;
    if (!h->fc_th0) {
        HIPCHK(own_alloc(h, h->fc_th0, sizeof(double) * (size_t)R * h->Npad * kDP));
        HIPCHK(own_alloc(h, h->fc_mom, sizeof(double) * (size_t)R * h->B * 16));
        HIPCHK(own_alloc(h, h->fc_momtot, sizeof(double) * (size_t)R * 16, Mem::zeroed));
        HIPCHK(own_alloc(h, h->fc_prop, sizeof(double) * (size_t)R * 16, Mem::zeroed));
    }
    // level-2 of the second-stage weights of the last step (the weights ssme_lw_get_expectations uses)
    forecast_plan(h, lw_plan_args(h, 0, h->t, 0, h->tsumB, h->tmaxB));
    FcLwArgs a{};
    a.x = h->xB; a.th = h->thB; a.cdf = h->cdfB; a.l2_T = h->fc.T; a.l2_R = h->fc.R; a.scal = h->fc.scal; a.last_obs = h->fc.last;
    a.x0 = h->fc.x0; a.th0 = h->fc_th0; a.start = h->fc.start; a.mom = h->fc_mom; a.prop = h->fc_prop;
    a.y_out = h->fc.y; a.x_out = x_out ? h->fc.x : nullptr;
    a.keyp = h->keybuf; a.first_filter = h->cfg.first_filter_id;
    a.N = N; a.Npad = h->Npad; a.Ns = (int)Ns; a.B = h->B; a.Bs = h->Bs; a.Bpow2 = h->Bpow2; a.t0 = h->t; a.H = H;
    a.a_shrink = (3.0 * h->cfg.delta - 1.0) / (2.0 * h->cfg.delta);
    for (int d = 0; d < kDP; ++d) a.trans[d] = h->cfg.transforms[d];
    hipLaunchKernelGGL(k_fc_lw_start, dim3(h->B, R), dim3(kLwNT), 0, h->stream, a);
    {
        LwArgs m{};                                   // the filter's own totals kernel on the forecast's partials
        m.B = h->B; m.mom = h->fc_mom; m.momtot = h->fc_momtot;
        hipLaunchKernelGGL(k_lw_mom_totals, dim3(kNMom, R), dim3(64), 0, h->stream, m);
    }
    hipLaunchKernelGGL(k_fc_lw_prop, dim3(R), dim3(64), 0, h->stream, (const double*)h->fc_momtot, N, a.a_shrink, h->fc_prop);
    HIPCHK(hipEventRecord(h->fc.ev[1], h->stream));
    hipLaunchKernelGGL(k_fc_lw_horizon, dim3((a.Ns / 2 + kFcNT - 1) / kFcNT, R), dim3(kFcNT), 0, h->stream, a);
    rc = forecast_finish(h, y_out, rows, x_out, rows, start_out);
    if (rc != SSME_OK) return rc;
    if (prop_out) {                                   // after the times are taken: ev[2] closes on the horizon kernel, as for the bootstrap
        HIPCHK(hipMemcpyAsync(prop_out, h->fc_prop, sizeof(double) * (size_t)R * 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return SSME_OK;
}

int ssme_lw_forecast_elapsed_ms(ssme_lw_handle h, float* horizon_kernel_ms, float* call_ms) { return forecast_elapsed(h, horizon_kernel_ms, call_ms); }

int ssme_lw_last_elapsed_ms(ssme_lw_handle h, float* ms) { return elapsed_ms(h, ms); }

const char* ssme_lw_last_error(ssme_lw_handle h) { return last_error(h); }

}  // extern "C"
