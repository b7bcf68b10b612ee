/* ssme_pf.h -- C ABI of the MI355X-native bootstrap-particle-filter core.
 *
 * Drop-in boundary for the hot path behind ssme's BSFilter<>::filter() step.  In the
 * reference this boundary is compile-time C++ inheritance from the external `pf` library
 * (no FFI exists): a model derives from pf::filters::BSFilter<nparts,dimx,dimy,resampT,
 * float_t> (example/univ_svol_bootstrap_filter.h:18) and callers use
 *     mod.filter(y_t);  logLike += mod.getLogCondLike();     example/estimate_univ_svol.h:124-125
 *     mods[i].filter(y_t, z_t, fs); getExpectations(); getLogCondLike();
 *                                                             include/ssme/pswarm_filter.h:86-92,380-388
 * Host virtual callbacks cannot run per particle on a GPU, so the model is selected by
 * enum and compiled into the kernels.  Plain pointers and sizes only; no C++/torch types.
 * Every function returns an int status (0 = ok); nothing throws across this boundary.
 * NaN / -inf log-likelihoods are VALUES, not errors (reference: ada_pmmh_mvn.h:349,357).
 *
 * Threading: re-entrant, no global mutable state.  One handle = one HIP stream; distinct
 * handles may be used concurrently from distinct host threads (as thread_pool.h:242-245
 * calls log_like_eval concurrently on distinct model objects); a single handle is not
 * thread-safe (same as one BSFilter object).
 */
#ifndef SSME_PF_H
#define SSME_PF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
enum {
    SSME_OK = 0,
    SSME_ERR_INVALID_ARG = 1,   /* reference: std::invalid_argument                     */
    SSME_ERR_LENGTH = 2,        /* reference: std::length_error (empty data, :113)      */
    SSME_ERR_UNSUPPORTED = 3,   /* valid request this build does not implement          */
    SSME_ERR_HIP = 4,           /* HIP runtime failure; text via ssme_pf_last_error     */
    SSME_ERR_STATE = 5          /* call order (e.g. step before set_params)             */
};

/* models: per-particle callbacks compiled into the kernels */
enum {
    SSME_MODEL_SVOL = 0,          /* svol_bs, example/univ_svol_bootstrap_filter.h:55-103;
                                     theta = (beta, phi, sigma)  [sigma = sqrt(ss), :58-60] */
    SSME_MODEL_SVOL_LEVERAGE = 1, /* svol_leverage, test/test_pswarm.cpp:80-134;
                                     theta = (phi, mu, sigma, rho); covariate z_t = y_{t-1} */
    SSME_MODEL_LIN_GAUSS = 2,     /* x' = phi x + sigma e, y ~ N(x, tau^2); theta = (phi, sigma, tau).
                                     Not in the reference: exact-Kalman correctness anchor.  */
    SSME_MODEL_USER0 = 3          /* the model compiled in from a user header (ssme_amd/csrc/model_api.h: the counterpart of
                                     deriving a class from BSFilter and overriding fSamp / logGEv / q1Samp,
                                     example/univ_svol_bootstrap_filter.h:37-41); SSME_ERR_UNSUPPORTED in a library
                                     built without one.  theta has ssme_pf_user_model_n_theta() entries.  */
};

/* resamplers (pf::resamplers::*, in-tree twin include/ssme/liu_west_filter.h:91-145) */
enum {
    SSME_RESAMP_MULTINOMIAL = 0,     /* multinomial by sorted uniforms (exponential spacings),
                                        the algorithm of liu_west_filter.h:105-139 / mn_resamp_fast1 */
    SSME_RESAMP_SYSTEMATIC = 1,
    SSME_RESAMP_STRATIFIED = 2,
    SSME_RESAMP_MULTINOMIAL_IID = 3  /* multinomial with unsorted iid uniforms (mn_resampler form) */
};

enum { SSME_F64 = 0, SSME_F32 = 1 };

/* built-in functionals h(x) for weighted expectations (std::function cannot run on device) */
enum { SSME_H_X = 0, SSME_H_X2 = 1, SSME_H_VOL = 2 /* exp(x/2) */, SSME_H_CONST42 = 3 };

typedef struct ssme_pf_s* ssme_pf_handle;

typedef struct ssme_pf_config {
    int32_t  model;            /* SSME_MODEL_*                                               */
    int32_t  n_particles;      /* N per filter (reference: template parameter nparts)        */
    int32_t  n_filters;        /* R independent filters/replicates held by this handle:
                                  thread_pool's num_pfilters (thread_pool.h:189-215) or the
                                  swarm's nparamparts (pswarm_filter.h:280-304)              */
    int32_t  dtype;            /* SSME_F64, or SSME_F32 = float at the boundary (the reference
                                  built with float_t = float, example/main.cpp:13): y, z and theta
                                  are rounded to float on entry and every returned log-likelihood,
                                  expectation, particle and weight is rounded to float; the
                                  arithmetic stays fp64 (plain fp32 VALU issues at the fp64 rate on
                                  gfx950, so float arithmetic would buy no time).  Not for sharded
                                  handles or the parity downloads (ssme_pf_download_state / _scalars
                                  hand out the raw fp64 state)                                 */
    int32_t  resampler;        /* SSME_RESAMP_*                                              */
    int32_t  resamp_sched;     /* resample every k-th step; 1 = reference default            */
    uint64_t seed;             /* Philox4x32-10 key (reference RNGs are clock-seeded)        */
    int32_t  device;           /* HIP device ordinal                                         */
    uint32_t first_filter_id;  /* global id of filter 0 of this handle; enters the Philox
                                  counter, so sharding R over GPUs keeps every stream        */
    int32_t  tile_particles;   /* particles per tile: 2048, 1024 or 512, or 0 = ssme_pf_default_tile(N, bank size), where
                                  the bank size is n_filters_total if > 0, else n_filters.
                                  Part of the arithmetic specification:
                                  weights are fixed point relative to their tile's maximum and
                                  the resampler draws one Gamma variate per tile */
    int32_t  n_filters_total;  /* 0, or the size of the WHOLE bank this handle holds a part of (replicates or swarm
                                  members dealt to several GPUs, or one handle per member): the default tile is then
                                  chosen from the bank, so that filter (seed, id, N) gives the same bits however the
                                  bank is split over handles.  Ignored when tile_particles != 0.             */
} ssme_pf_config;

/* Allocates device state for R filters of N particles.  Replaces construction of the
 * model object (estimate_univ_svol.h:119), but the handle is reusable across theta. */
int ssme_pf_create(const ssme_pf_config* cfg, ssme_pf_handle* out);
int ssme_pf_destroy(ssme_pf_handle h);
/* The tile size tile_particles = 0 stands for: 2048 for N <= 2048; else 512 while bank_filters * ceil(N / 512) <= 256
 * (one workgroup per CU), else 1024 while bank_filters * ceil(N / 1024) <= 512, else 2048 -- a mid-size bank then spreads
 * over the chip (profiles/r02_tile_sweep.txt).  It reads the BANK, not the handle: callers that split a bank over GPUs or
 * handles pass n_filters_total (or this value as tile_particles) so that results do not depend on the split. */
int ssme_pf_default_tile(int32_t n_particles, int32_t bank_filters);
/* Length of theta for SSME_MODEL_USER0, or 0 when this library was built without a user model. */
int ssme_pf_user_model_n_theta(void);
/* State and observation dimension of SSME_MODEL_USER0 (BSFilter<nparts, dimx, dimy, ...>: 1 .. 4 each; ssme_amd/csrc/model_api.h);
 * SSME_ERR_UNSUPPORTED and zeros without a user model.  With dim_y > 1 every y argument of this interface is dim_y values per time
 * step (run_series: y[t * dim_y + j]; step: dim_y values); with dim_x > 1 ssme_pf_download_state and ssme_pf_download_weights return
 * x[d * N + i] (dim_x planes; the weights are what a host-side functional h(x) of the whole state needs) and the device functionals
 * see component 0.  A forecast (ssme_pf_sim_future_obs, for a header that declares the observation draw) returns
 * y_out[((r * num_steps + k) * dim_y + j) * N + i] and x_out[((r * num_steps + k) * dim_x + d) * N + i]; the covariate of a simulated
 * step is component 0 of the previous simulated observation.  Vector models are unsharded, SSME_F64. */
int ssme_pf_user_model_dims(int32_t* dim_x, int32_t* dim_y);
/* 1 when the compiled-in user model declares its observation draw (gsamp, or gsamp_vec for a vector model: ssme_amd/csrc/model_api.h)
 * and SSME_MODEL_USER0 handles can therefore be forecast; 0 for the stock library and for a header without the draw.  Needs no device. */
int ssme_pf_user_model_has_gsamp(void);
/* Covariates of SSME_MODEL_USER0 (BSFilterWC<nparts, dimx, dimy, dimcov, ...>): dim_cov of the compiled-in header (1 .. 4;
 * ssme_amd/csrc/model_api.h), or 0 for the stock library and for a header without dim_cov.  Needs no device.  With dim_cov = K > 0
 * every z argument of this interface is K values per time step -- ssme_pf_step: K values; ssme_pf_run_series /
 * ssme_pf_profile_series: z[t * K + j]; NULL means zeros in both -- and every callback of the header (prop, logg, gsamp, their
 * vector forms, first / first_logw, h) receives the K covariates of its step.  One z_t serves all filters of the handle.  Such a
 * model is forecast with future covariates (ssme_pf_sim_future_obs_cov; ssme_pf_sim_future_obs is SSME_ERR_UNSUPPORTED) and is
 * unsharded (ssme_pf_shard_create: SSME_ERR_UNSUPPORTED).  SSME_F32 handles round all K values to float on entry. */
int ssme_pf_user_model_dim_cov(void);
/* 1 when the compiled-in header declares a first step of its own (first and first_logw: q1Samp(y1, z1) and
 * logMuEv(x1, z1) - logQ1Ev(x1, y1, z1) of the reference), 0 otherwise.  Needs no device. */
int ssme_pf_user_model_has_first(void);

/* UNTRANSFORMED parameters, as the reference's model ctors receive them from
 * pack::get_untrans_params (univ_svol_bootstrap_filter.h:55-61).  theta is
 * [n_rows][n_theta]; n_rows = 1 broadcasts one theta to all filters (PMMH replicates),
 * n_rows = n_filters gives each filter its own row (swarm).  Also resets time to 0. */
int ssme_pf_set_params(ssme_pf_handle h, const double* theta, int32_t n_theta, int32_t n_rows);

/* Back to t = 0 with the current parameters (a fresh model object in the reference). */
/* New random stream for the next evaluation; resets the filters.  The reference seeds every model object from the clock
 * (a fresh likelihood estimate per PMMH proposal, estimate_univ_svol.h:119); here the caller supplies the seed. */
int ssme_pf_set_seed(ssme_pf_handle h, uint64_t seed);
int ssme_pf_reset(ssme_pf_handle h);

/* One filter() call on every filter of the handle: BSFilter::filter(y_t) /
 * BSFilterWC::filter(y_t, z_t).  y: 1 value; z: 1 value or NULL (dim_cov values for a user model
 * that declares them, ssme_pf_user_model_dim_cov).  logcondlike_out (R
 * values, nullable) receives getLogCondLike() of each filter.  With logcondlike_out = NULL the
 * step is only queued on the handle's stream (the swarm classes: ssme_pf_swarm_aggregate, which
 * follows, hands the data back); every later call on the handle is ordered behind it. */
int ssme_pf_step(ssme_pf_handle h, const double* y, const double* z, double* logcondlike_out);

/* The whole log_like_eval loop (estimate_univ_svol.h:121-127) for all R filters in one
 * call: reset, T steps, sum of log p(y_t | y_{1:t-1}).  loglik_out: R values. */
int ssme_pf_run_series(ssme_pf_handle h, const double* y, const double* z, int32_t T, double* loglik_out);

/* Per-step log conditional likelihoods of the last run_series: out[r*T + t]. */
int ssme_pf_get_per_step(ssme_pf_handle h, double* out, int32_t T);

/* Accumulated log-likelihood since the last reset: R values. */
int ssme_pf_get_loglik(ssme_pf_handle h, double* out);

/* E[h(x_t) | y_{1:t}] with the pre-resampling weights of the last step
 * (getExpectations(); twin liu_west_filter.h:1662-1683).  out: R values.  The built-in functionals see component 0 of a
 * vector state: users of a vector model declare their functionals in the model header and call
 * ssme_pf_get_user_expectations (below). */
int ssme_pf_get_expectations(ssme_pf_handle h, int32_t functional, double* out);
/* The same for n <= 4 built-in functionals at once (filter(y, z, fs) takes a VECTOR of functions, pswarm_filter.h:87):
 * one pass over the particles, one download.  out[i*R + r] = E[h_i] of filter r. */
int ssme_pf_get_expectations_multi(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* out);
/* Swarm::update's aggregation over the R member filters of this handle (pswarm_filter.h:96-160,233-235: uniform
 * weights, i.e. plain means), reduced on the device: mean of the last step's log conditional likelihoods and mean of each
 * requested expectation (n may be 0).  One download of n + 1 doubles. */
int ssme_pf_swarm_aggregate(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* mean_logcondlike /*1*/,
                            double* mean_expectations /*n*/);
/* The same as the reference computes it when its pool has num_threads workers: member i is dealt to thread i % num_threads
 * (thread_pool.h:443-447), every thread averages its members and the thread averages are averaged (pswarm_filter.h:96-160) --
 * the plain mean exactly when num_threads divides R, a slightly differently weighted mean otherwise (a thread with one member
 * fewer counts each of its members more).  num_threads <= 0 or >= R: ssme_pf_swarm_aggregate's plain mean / one member per thread. */
int ssme_pf_swarm_aggregate_threads(ssme_pf_handle h, const int32_t* functionals, int32_t n, int32_t num_threads,
                                    double* mean_logcondlike /*1*/, double* mean_expectations /*n*/);
/* Functionals of the user model's own (SSME_MODEL_USER0 whose header declares n_h and h, ssme_amd/csrc/model_api.h): functions
 * h(x, z, theta) of the WHOLE state, compiled into an expectation kernel.  ssme_pf_user_model_n_h: their number, 0 for the stock
 * library and for a user model without functionals; needs no device.
 * ssme_pf_get_user_expectations: out[k*R + r] = E[h_k(x_t) | y_{1:t}] of filter r with the weights ssme_pf_get_expectations uses
 * (any resamp_sched); z is the covariate of the handle's last step (0 if it had none).  One pass over the particles, one download
 * of n_h * R doubles -- no ssme_pf_download_weights per filter.  ssme_pf_swarm_aggregate_user: the means over the R members of the
 * last log conditional likelihoods and of the n_h expectations, as ssme_pf_swarm_aggregate_threads forms them (num_threads <= 0:
 * plain means); one download of n_h + 1 doubles.  Both: SSME_ERR_UNSUPPORTED when n_h == 0 or the handle's model is not
 * SSME_MODEL_USER0, SSME_ERR_STATE before the first step and on sharded handles; ordered behind steps queued on the handle's
 * stream (ssme_pf_step with logcondlike_out = NULL); SSME_F32 handles round the results to float. */
int ssme_pf_user_model_n_h(void);
int ssme_pf_get_user_expectations(ssme_pf_handle h, double* out /* [n_h][R] */);
int ssme_pf_swarm_aggregate_user(ssme_pf_handle h, int32_t num_threads, double* mean_logcondlike /*1*/, double* mean_expectations /*n_h*/);
/* The filtered PATH: E[h(x_t) | y_{1:t}] for every step t of ssme_pf_run_series (the reference calls filter(y_t, fs) and
 * getExpectations() at every step, pswarm_filter.h:87-89,383-385), recorded by the series itself -- the whole-series kernels of
 * one-tile filters form the rows in LDS, the tiled route queues the expectation kernels behind every step, graph or eager.
 * ssme_pf_set_series_expectations: record the n built-in functionals (0 .. 4 ids SSME_H_X .. SSME_H_CONST42) and, with
 * user != 0, all n_h functionals of the compiled-in user model at every step of the run_series calls that follow.  n = 0 and
 * user = 0 switch recording off (the default of a new handle; nothing about a non-recording run changes).  The setting survives
 * run_series, set_params, set_seed and reset; a cached graph of another recording configuration is dropped.  Validated before any
 * HIP call: NULL handle, an id out of range, n < 0 or n > 4, n > 0 with NULL functionals: SSME_ERR_INVALID_ARG; user != 0 on a handle
 * whose model is not SSME_MODEL_USER0 or in a library with n_h == 0: SSME_ERR_UNSUPPORTED; sharded handles: SSME_ERR_STATE.
 * ssme_pf_get_series_expectations / ssme_pf_get_series_user_expectations: rows 0 .. T-1 of the last run_series,
 * out[(t*n + i)*R + r] / out[(t*n_h + k)*R + r].  Row t is, to the bit, what ssme_pf_get_expectations_multi /
 * ssme_pf_get_user_expectations return after step t of a handle stepped with ssme_pf_step: the pre-resampling weights of step t
 * at any resamp_sched, the covariates of row t for the user model's h, NaN where the filter's weights are NaN, infinite or all
 * zero (the call still returns SSME_OK).  NULL arguments, T < 1 or T beyond the last recorded series: SSME_ERR_INVALID_ARG; nothing
 * recorded of that kind (recording off during the last run_series, or no run_series yet): SSME_ERR_STATE.  SSME_F32 handles round
 * the rows to float.  ssme_pf_step neither records nor clears.  The trajectory (T (n + n_h) R doubles on the device) exists only
 * while recording is on. */
int ssme_pf_set_series_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n, int32_t user);
int ssme_pf_get_series_expectations(ssme_pf_handle h, double* out /* [T][n][R] */, int32_t T);
int ssme_pf_get_series_user_expectations(ssme_pf_handle h, double* out /* [T][n_h][R] */, int32_t T);
/* SMOOTHING: the distribution p(x_{0:T-1} | y_{0:T-1}) of a series, as sampled state trajectories and as smoothed means (what a
 * particle-marginal Metropolis-Hastings caller needs to sample the latent states jointly with theta; the reference has no
 * counterpart: its filters keep no genealogy).  DESIGN.md section 12; kernels in ssme_amd/csrc/smooth.h.
 * Definitions.  The population of step t is x_t[j], pre-resampling, as ssme_pf_download_state returns it (dim_x planes for a vector
 * model).  A step t >= 1 with t % resamp_sched == 0 drew anc_t[j], an index into the population of step t - 1; on every other step
 * anc_t is the identity.  The lineage of final particle j is B_{T-1}(j) = j, B_{t-1}(j) = anc_t[B_t(j)].  The smoothing weights are
 * the final step's fixed-point weights (q_j of the integer cdf, tile scales e^{m_b - m}): exactly the weights
 * ssme_pf_get_expectations_multi and the start draw of ssme_pf_sim_future_obs use.
 * ssme_pf_set_series_history: with enable = 1 the ssme_pf_run_series calls that follow keep every step's population (all planes) and
 * ancestors on the device -- T R Npad (8 dim_x + 4) bytes, Npad = tiles x tile_particles (ssme_pf_get_layout), which
 * ssme_pf_series_history_bytes reports before the run.  On the tiled route (graph or eager) the step kernel writes its particles
 * straight into the history rows (no extra traffic) and runs its general instantiation, as under set_debug(1); one-tile filters
 * (N <= 2048) keep their whole-series kernels, in a recording instantiation that also serves ssme_pf_set_series_expectations.  A
 * recording run returns the log-likelihoods, per-step values, final state and recorded expectations of a non-recording run, to the
 * bit; a run that records neither the history nor series expectations launches the kernels it launched before this setting existed,
 * instruction for instruction (profiles/series_history_stock_kernels.txt, which also lists what moved in the recording kernels).
 * With set_debug(1) as well, ssme_pf_download_state's ancestors after a recording run are those of the last step that resampled, as
 * after a non-recording run.
 * The setting (default 0) survives run_series, set_params, set_seed and reset; a cached graph of the other configuration is dropped;
 * the rows are allocated by run_series (a refused allocation: SSME_ERR_HIP with ssme_pf_last_error; the handle stays usable, holds no
 * rows and no history is in force: the smoothing calls answer SSME_ERR_STATE until a recording run_series has succeeded) and
 * freed by the first run_series with the setting off.  NULL handle, enable outside {0, 1}: SSME_ERR_INVALID_ARG; sharded: SSME_ERR_STATE.
 * ssme_pf_series_history_bytes: NULL handle or bytes, T < 1: SSME_ERR_INVALID_ARG; sharded: SSME_ERR_STATE.  Makes no HIP call.
 * ssme_pf_sample_trajectories: K (1 .. N) trajectories per filter, traced back on the device in ONE launch.  terminal[r * K + k]:
 * the final particle trajectory k of filter r ends at; NULL: drawn from the smoothing weights by the forecast's start draw
 * (counter (k, t0 = T, filter id, start stream), the same search), so index_out[(r K + k) T + T - 1] == start_out[r N + k] of
 * ssme_pf_sim_future_obs from the same origin -- a sampled path and its simulated continuation join.
 * x_out[((r K + k) T + t) dim_x + d] = component d of x_t[B_t]; index_out[(r K + k) T + t] = B_t, or NULL.
 * ssme_pf_get_smoothed_expectations: out[(t n + i) R + r] = sum_j h_i(x_t[B_t(j)]) w_j / sum_j w_j over all N final particles, for
 * n = 1 .. 4 built-in functionals (SSME_H_*; component 0 of a vector state), by the summation trees of the filtered expectations:
 * row T - 1 is ssme_pf_get_expectations_multi after the series, to the bit.  One backward launch and one finishing launch.
 * Both: a filter without weight (all weights zero, -inf or NaN, e.g. `bad` parameters) gets NaN states / NaN rows and the call
 * returns SSME_OK; its index_out still holds the in-range lineage indices (< N) of the terminals it was given or drew; two calls from one history return the same bits; SSME_F32 handles round x_out / out to float.
 * Validated before any HIP call -- SSME_ERR_INVALID_ARG: NULL handle or x_out / out / functionals, K < 1 or K > N, a terminal index
 * >= N, n < 1 or n > 4, a functional id out of range, T different from the recorded series' length; SSME_ERR_STATE: a sharded
 * handle (as ssme_pf_run_series answers), or no history in force -- recording off during the last ssme_pf_run_series, no
 * ssme_pf_run_series yet, a ssme_pf_run_series that failed, or any later ssme_pf_step, ssme_pf_run_series, ssme_pf_profile_series, ssme_pf_reset, ssme_pf_set_params
 * or ssme_pf_set_seed on the handle (they change or discard the state the smoothing weights live in).  Forecasts, expectation
 * getters and downloads do not invalidate the history.
 * ssme_pf_smoothing_elapsed_ms: HIP-event times of the last of the smoothing calls (ssme_pf_sample_trajectories_backward included): its
 * kernels alone, and the call without the download.
 * Out of scope: the functionals of a user header, fixed-lag smoothing, Liu-West handles and sharded handles; the trajectories above are
 * the filter's genealogy and share ancestors -- backward simulation (below) draws them without that defect. */
int ssme_pf_set_series_history(ssme_pf_handle h, int32_t enable);
int ssme_pf_series_history_bytes(ssme_pf_handle h, int32_t T, uint64_t* bytes);
int ssme_pf_sample_trajectories(ssme_pf_handle h, int32_t K, const uint32_t* terminal /*[R][K] or NULL: drawn as above*/,
                                double* x_out /*[((r*K + k)*T + t)*dim_x + d]*/, uint32_t* index_out /*[(r*K + k)*T + t] or NULL*/, int32_t T);
int ssme_pf_get_smoothed_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* out /*[(t*n + i)*R + r]*/, int32_t T);
int ssme_pf_smoothing_elapsed_ms(ssme_pf_handle h, float* kernel_ms, float* call_ms);
/* Backward-simulation smoothing (forward filtering, backward simulation: Godsill, Doucet and West 2004; ssme_amd/csrc/backward.h,
 * DESIGN.md section 12.1): trajectories from the same recorded history whose earlier states are drawn AGAIN from all N particles of
 * their step, P(B_t = i | x~_{t+1}) prop. W_t[i] f(x~_{t+1} | x_t[i], z_{t+1}), so that they do not coalesce as the genealogy does.
 * ssme_pf_sample_trajectories_backward: arguments, layouts and validation of ssme_pf_sample_trajectories.  B_{T-1} is given or
 * drawn exactly as there (both calls return the same index_out[.., T - 1]: the join with a forecast's start draw is kept; T = 1 returns
 * that call's output).  For t = T-2 .. 0, with x~ = x_{t+1}[B_{t+1}] and the covariates of step t + 1:
 *   a_i = lw_t[i] + logf(x~ | x_t[i], z_{t+1}) (NaN counts as -inf), m = max a_i, q_i = rint(exp(a_i - m) 2^sh) by the filter's
 *   quantiser at sh = min(41, 52 - ceil(log2 N)), S = sum q_i and the inclusive sums C_i exact integers below 2^53;
 *   u = the 40-bit midpoint uniform of words 0-1 of Philox(k, t, filter id, stream 165), target = ceil(u S), B_t = the first i with
 *   C_i >= target.  m not finite or S not > 0 (a degenerate transition): B_t = the genealogical ancestor (anc_{t+1}[B_{t+1}], or
 *   B_{t+1} where step t + 1 did not resample).  No index leaves [0, N).
 * lw_t are the pre-resampling log-weights the filter had at step t, recomputed from the history, the series and the covariates
 * (which the handle keeps on the device) with the filter's own device functions: 8 T R Npad bytes (ssme_pf_backward_bytes; no HIP
 * call), filled by the first backward call after a recording run, reused while that history is in force and freed with its rows.
 * ssme_pf_download_series_logweights hands out row t of one filter (N values): bit-equal to ssme_pf_download_state's logw after step
 * t of a handle stepped under ssme_pf_set_debug(2).  The cost is O(K N T) density evaluations, sequential in t; N up to the handle's limit.
 * A filter without final weight gets NaN states and in-range indices (SSME_OK); SSME_F32 handles round x_out; two calls from one
 * history return the same bits; a call changes nothing a later call returns.  SSME_ERR_STATE: sharded handles, no history in force
 * (as above); SSME_ERR_UNSUPPORTED: SSME_MODEL_USER0 whose header declares no transition density (logf / logf_vec of
 * ssme_amd/csrc/model_api.h; ssme_pf_user_model_has_logf, which needs no device: 0 for the stock library).  Built-in models:
 * log f = -((xn - mean) / sd)^2 / 2 with the mean of the proposal in its own operation order.
 * Out of scope: Liu-West and sharded handles, rejection-sampling / MCMC backward steps and backward-simulated expectations of a user
 * header's functionals; the marginal O(N^2) smoothing weights follow below. */
int ssme_pf_user_model_has_logf(void);
int ssme_pf_backward_bytes(ssme_pf_handle h, int32_t T, uint64_t* bytes);
int ssme_pf_download_series_logweights(ssme_pf_handle h, int32_t filter, int32_t t, double* lw /*N*/);
int ssme_pf_sample_trajectories_backward(ssme_pf_handle h, int32_t K, const uint32_t* terminal /*[R][K] or NULL*/,
                                         double* x_out /*[((r*K + k)*T + t)*dim_x + d]*/, uint32_t* index_out /*[(r*K + k)*T + t] or NULL*/, int32_t T);
/* Marginal smoothing weights (forward filtering, backward smoothing: Doucet, Godsill and Andrieu 2000; ssme_amd/csrc/marginal.h,
 * DESIGN.md section 12.2): the EXPECTATION of the backward draws above, a weight per particle of every step of the recorded history,
 *   om_{T-1}[j] = w_j, the unnormalised final weights of ssme_pf_download_weights, bit for bit;  for t = T-2 .. 0, with the covariates
 *   of step t + 1:  a_ij = lw_t[i] + logf(x_{t+1}[j] | x_t[i], z_{t+1}) (NaN counts as -inf), m_j = max_i a_ij,
 *   q_ij = rint(exp(a_ij - m_j) 2^sh) (the quantiser and sh of backward simulation), D_j = sum_i q_ij (an exact integer below 2^53);
 *   column j is live when m_j is finite and D_j > 0, then c_j = om_{t+1}[j] / D_j; otherwise it is degenerate and its mass goes to its
 *   genealogical parent g(j) = min(anc_{t+1}[j], N - 1) where step t + 1 resampled, j otherwise:
 *   om_t[i] = sum_{j live} c_j q_ij + sum_{j degenerate, g(j) = i} om_{t+1}[j].
 * q_ij / D_j and the fallback are, to the bit, what ssme_pf_sample_trajectories_backward draws B_t from given B_{t+1} = j, so om_t is
 * the exact law of B_t when B_{T-1} is drawn from the final weights: smoothed means without the noise of K draws and without the path
 * degeneracy of the genealogy, at 3 N^2 (T - 1) density evaluations.  The sum over j is a floating-point sum of non-negative terms in a
 * FIXED order that depends on N alone (no atomics; chunks of 64 columns dealt round-robin to 8 partial sums, each in ascending j, the
 * 8 then added in order): two calls from one history return the same bits, whatever the bank shape or the route.  Rows are not normalised: sum_i
 * om_t[i] equals sum_j w_j up to rounding.
 * ssme_pf_marginal_smoothing_bytes: the device bytes a T-step history needs for this, 32 T R Npad -- 8 T R Npad of them the
 * log-weight rows it shares with backward simulation (ssme_pf_backward_bytes), 8 T R Npad the weight rows, 16 T R Npad the column
 * tables m and D.  Makes no HIP call.  All of it is filled by the first marginal call after a recording run (the log-weight rows
 * first, unless backward simulation already did), reused while that history is in force, stale the moment the handle moves on and
 * freed with the history rows; a refused allocation is SSME_ERR_HIP, the handle stays usable and the history in force.
 * ssme_pf_download_smoothing_weights: x_t (x[d * N + i], dim_x planes, or NULL) and om_t (w, N values) of one filter, for host-side
 * functionals: the caller forms sum h(x_t[i]) om_t[i] / sum om_t[i].
 * ssme_pf_get_marginal_smoothed_expectations: out[(t n + i) R + r] = sum_j h_i(x_t[j]) om_t[j] / sum_j om_t[j] for n = 1 .. 4 built-in
 * functionals (SSME_H_*; component 0 of a vector state) in a fixed summation tree; NaN where sum_j om_t[j] is not > 0.
 * A filter without final weight gets all-zero weight rows and NaN expectation rows (SSME_OK).  SSME_F32 handles round x, w and out to
 * float.  A call changes nothing the other smoothing calls return.  ssme_pf_smoothing_elapsed_ms reports these calls too.
 * Validated before any HIP call, as ssme_pf_sample_trajectories_backward validates -- SSME_ERR_INVALID_ARG: NULL handle, bytes, w,
 * out or functionals, filter or t out of range, n < 1 or n > 4, a functional id out of range, T < 1 or different from the recorded
 * length; SSME_ERR_STATE: sharded handles, no history in force; SSME_ERR_UNSUPPORTED: SSME_MODEL_USER0 without logf / logf_vec.
 * Out of scope: Liu-West and sharded handles, device-side expectations of a user header's own functionals (the weight rows serve
 * those on the host), two-filter smoothing and sub-quadratic approximations. */
int ssme_pf_marginal_smoothing_bytes(ssme_pf_handle h, int32_t T, uint64_t* bytes);
int ssme_pf_download_smoothing_weights(ssme_pf_handle h, int32_t filter, int32_t t, double* x /*[dim_x][N] or NULL*/, double* w /*N*/);
int ssme_pf_get_marginal_smoothed_expectations(ssme_pf_handle h, const int32_t* functionals, int32_t n, double* out /*[(t*n + i)*R + r]*/, int32_t T);
/* Arbitrary host-side h (the reference's filt_func is a std::function, pswarm_filter.h:44,87-89): particles x (N,
 * nullable) and weights w (N) of one filter after the last step, w_j = exp(logw_j - max logw) in the 2^-41 fixed point
 * the resampler and ssme_pf_get_expectations use; the caller forms sum h(x_j) w_j / sum w_j.  Needs no debug mode. */
int ssme_pf_download_weights(ssme_pf_handle h, int32_t filter, double* x, double* w);

/* Replicate aggregation of thread_pool.h:263-268: log-mean-exp of the R log-likelihoods. */
int ssme_pf_log_mean_exp(ssme_pf_handle h, double* out);

/* Parity/debug: state of one filter after the last step.  Any pointer may be NULL.
 * x: N pre-resampling particles; logw: their log-weights (only kept in memory after
 * set_debug(flags & 2), or when resamp_sched > 1); cdf: N tile-local inclusive sums of the
 * fixed-point weights q_i = rne(exp(logw_i - max_tile) * 2^41) (exact integers < 2^53, carried in fp64 on the device);
 * ancestors: N indices used by the last step (requires set_debug(flags & 1)). */
int ssme_pf_download_state(ssme_pf_handle h, int32_t filter, double* x, double* logw, uint64_t* cdf,
                           uint32_t* ancestors);
/* The tile decomposition in use: particles per tile (2048, 1024 or 512) and tiles per filter. */
int ssme_pf_get_layout(ssme_pf_handle h, int32_t* tile_particles, int32_t* n_tiles);
/* max_logw: max log-weight of the last step; sum_q: exact integer sum of the rescaled tile sums;
 * tile_sums / tile_max: one integer weight sum and one max log-weight per tile;
 * rshift: the fixed-point exponent rg = 52 - ceil(log2(Npad)) of sum_q. */
int ssme_pf_download_scalars(ssme_pf_handle h, int32_t filter, double* max_logw, uint64_t* sum_q,
                             uint64_t* tile_sums, double* tile_max, int32_t* rshift);
/* flags: bit 0 = record ancestor indices, bit 1 = keep log-weights in memory (parity tests), bit 2 = compute level-2 (global
 * max, rescaled tile sums, their scan, every tile's source range) once per filter in its own launch instead of in every
 * workgroup; bit 3 = the opposite (in-kernel level-2, possible up to 2048 tiles).  Default: split above 1024 tiles
 * (N > 2^20), where it is faster; always split above 2048 tiles (N > 2^22; limit N <= 2^25).  Same results to the bit. */
int ssme_pf_set_debug(ssme_pf_handle h, int32_t flags);

/* Threads per 2048-particle tile of the step kernel: 256, 512 (default) or 1024.  Results do
 * not depend on it (the weight cdf is exact integer arithmetic). */
int ssme_pf_set_tuning(ssme_pf_handle h, int32_t threads_per_tile);

/* Filters of one tile (N <= 2048) run ssme_pf_run_series as ONE launch that loops over the series with the state in
 * LDS (the default, vector user models included: all dim_x planes live in LDS); 0 forces the tiled per-step kernel, 1 the
 * one-launch kernels.  Results are bit-identical either way (parity tests). */
int ssme_pf_set_small_series(ssme_pf_handle h, int32_t enable);
/* What ssme_pf_run_series launches for this handle as it is configured now: the tiled step kernel (threads per tile), or one of
 * the two whole-series kernels of one-tile filters -- one particle per lane (N <= 512) or one particle pair per lane -- and the
 * threads of its one workgroup per filter.  Needs no prior step.  Sharded handles: SSME_ERR_STATE, as for ssme_pf_run_series. */
enum { SSME_ROUTE_TILED = 0, SSME_ROUTE_SERIES_LANE = 1, SSME_ROUTE_SERIES_PAIR = 2,
       SSME_ROUTE_LW_SERIES = 3 /* Liu-West handles: ssme_lw_get_series_route */ };
int ssme_pf_get_series_route(ssme_pf_handle h, int32_t* route, int32_t* threads_per_block);
/* Execution policy of run_series: 0 = eager launches, 1 = one hipGraph per series (default). */
int ssme_pf_set_graph_mode(ssme_pf_handle h, int32_t mode);

/* HIP-event time (ms) of the last run_series on the handle's stream (kernels only, the
 * 8*T-byte upload of y and the 8*R-byte download of the result excluded). */
int ssme_pf_last_elapsed_ms(ssme_pf_handle h, float* ms);

/* Forecast: simulated future observations from the filtered cloud -- sim_future_obs(num_future_steps) of the reference's
 * *FutureSimulator add-ons, which Swarm::simFutureObs / SwarmWithCovs::simFutureObs call on every member
 * (pswarm_filter.h:247-253, 547-553); ONE call for all R filters of the handle, everything on the device.
 * From a handle that has done t0 >= 1 steps: N ancestors per filter are drawn from the weights ssme_pf_get_expectations uses (an iid
 * two-level search of the integer weight cdf; always taken, also on a step of a resamp_sched > 1 schedule that did not resample),
 * then for k = 0 .. num_steps-1:  x <- fSamp(x, y_prev),  y <- gSamp(x),  y_prev <- y   (gSamp: SVOL beta exp(x/2) z, leverage
 * exp(x/2) z, linear Gaussian x + tau z).  last_obs: y_prev of the first horizon, one value per filter (read by the leverage model
 * only; NULL = 0).  y_out[(r * num_steps + k) * N + i] ("param, time, then state particle", pswarm_filter.h:49-50); x_out: the
 * simulated states in the same shape, or NULL; start_out: [R][N] ancestors of the start draw, or NULL.  A filter whose weights are all
 * zero, -inf or NaN (e.g. `bad` parameters) gets NaN samples and the call returns SSME_OK.  The call changes nothing a later call on
 * the handle returns (buffers and Philox streams of its own: two forecasts from one origin return the same bits) and is ordered
 * behind steps queued with logcondlike_out = NULL.  SSME_F32 handles round last_obs on entry and every output to float.
 * SSME_MODEL_USER0 whose header declares the observation draw (ssme_pf_user_model_has_gsamp; gsamp / gsamp_vec of
 * ssme_amd/csrc/model_api.h): the same start draw gathers all dim_x state planes, then  x <- prop / prop_vec(x, zs, zcov = y_prev[0]),
 * y <- gsamp / gsamp_vec(x, zo),  y_prev <- y: the covariate of a simulated step is component 0 of the previous simulated
 * observation (last_obs at the first horizon), the built-in leverage model's convention; a header with dim_cov has exogenous
 * covariates and is forecast by ssme_pf_sim_future_obs_cov (here: SSME_ERR_UNSUPPORTED).  Layouts: y_out[((r * num_steps + k) * dim_y + j) * N + i], x_out[((r * num_steps + k) * dim_x + d) * N + i],
 * start_out[R][N]; with dim = 1 these are the layouts above, and a scalar user model consumes the random numbers a built-in one does.
 * Arguments are validated before any HIP call: NULL handle or y_out, num_steps < 1 or > 65535: SSME_ERR_INVALID_ARG; sharded handles,
 * and SSME_MODEL_USER0 when the compiled-in header declares no observation draw: SSME_ERR_UNSUPPORTED; before the first step:
 * SSME_ERR_STATE. */
int ssme_pf_sim_future_obs(ssme_pf_handle h, int32_t num_steps, const double* last_obs /*R or NULL*/,
                           double* y_out /*[R][num_steps][dim_y][N]*/, double* x_out /*[R][num_steps][dim_x][N] or NULL*/,
                           uint32_t* start_out /*[R][N] or NULL*/);
/* The forecast of a SSME_MODEL_USER0 handle whose header declares dim_cov = K (ssme_pf_user_model_dim_cov) and the observation
 * draw: the covariates of horizon k are z_future[k * K + j], exogenous and the same for every filter and particle, and reach both
 * calls:  x <- prop / prop_vec(x, zs, z_k),  y <- gsamp / gsamp_vec(x, zo, z_k).  The previous simulated observation is not a
 * covariate here.  Start draw, Philox counters, layouts of y_out / x_out / start_out, the NaN rule, the ordering and "changes nothing
 * a later call returns" are those of ssme_pf_sim_future_obs.  SSME_F32 handles round z_future on entry.  Validated before any HIP call:
 * NULL handle, y_out or z_future, num_steps < 1 or > 65535: SSME_ERR_INVALID_ARG; a model without dim_cov, a header without the
 * draw, a sharded handle: SSME_ERR_UNSUPPORTED; before the first step: SSME_ERR_STATE. */
int ssme_pf_sim_future_obs_cov(ssme_pf_handle h, int32_t num_steps, const double* z_future /*[num_steps][K]*/,
                               double* y_out /*[R][num_steps][dim_y][N]*/, double* x_out /*[R][num_steps][dim_x][N] or NULL*/,
                               uint32_t* start_out /*[R][N] or NULL*/);
/* HIP-event times (ms) of the last ssme_pf_sim_future_obs: the horizon kernel alone, and the whole call without the download. */
int ssme_pf_forecast_elapsed_ms(ssme_pf_handle h, float* horizon_kernel_ms, float* call_ms);

/* Measurement aid for bench.py: runs a T-step series eagerly (no graph) with a HIP event on the handle's
 * stream after every 32 launches of the step kernel (k_filter_step); returns the mean launch duration in
 * microseconds (mean_us_out[0]) and the launch count (launches_out[0]). */
int ssme_pf_profile_series(ssme_pf_handle h, const double* y, const double* z, int32_t T,
                           double* mean_us_out /*1*/, int32_t* launches_out /*1*/);

/* Device-side primitives exposed for bit-parity tests against the oracle. */
int ssme_pf_test_math(int32_t device, int32_t fn /*0 exp,1 log,2 sin2pi,3 cos2pi,4 sqrt,5 log (normal-only core),6 log of a uniform (table),7 exp (table form of the bootstrap filter),8 / 9 sin / cos of 2 pi k / 2^24 (in = k),10 log of a spacing uniform,11 sqrt of a positive normal*/,
                      const double* in, double* out, int64_t n);
int ssme_pf_test_philox(int32_t device, const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4);
/* q = rne(exp(in) * 2^shift) as uint64, n values */
int ssme_pf_test_quantize(int32_t device, const double* in, int32_t shift, uint64_t* out, int64_t n);
/* out = rint((double)tile_sum * exp(dm) * 2^shift): the cross-tile rescaling of tile sums */
int ssme_pf_test_rescale(int32_t device, const uint64_t* tile_sums, const double* dm, int32_t shift, uint64_t* out,
                         int64_t n);
/* exact inclusive scan of 2048 integers (< 2^53 in total) by one block of 256/512/1024 threads (fp64 DPP wave scans) */
int ssme_pf_test_block_scan(int32_t device, int32_t threads, const uint64_t* in2048, uint64_t* incl2048,
                            uint64_t* total);
/* measurement aid: `repeats` streaming copies of n doubles with 16-byte-per-lane accesses (counter calibration) */
int ssme_pf_test_copy(int32_t device, int64_t n_doubles, int32_t repeats);
/* n Gamma(shape) draws for tiles 0..n-1 at time t of filter `rep` */
int ssme_pf_test_gamma(int32_t device, uint64_t seed, uint32_t rep, int32_t t, double shape, int32_t n, double* out);

/* ============================================================================================
 * Particle-sharded filter: ONE filter of cfg->n_particles particles over `world` GPUs,
 * one process per GPU.  A tile = 2048 particles, B = ceil(n_particles / 2048) tiles, Bl = ceil(B / world): rank g owns tiles
 * [g Bl, min((g+1) Bl, B)) -- any n_particles up to 2^25 for which every rank owns at least one tile, (world-1) Bl < B (always
 * true from world (world-1) tiles on; SSME_ERR_UNSUPPORTED otherwise): the last rank may own fewer tiles and a ragged last
 * tile, and every per-rank layout (the gathered tile arrays: world x Bl entries of which the first B are tiles; buffers; halos)
 * has Bl rows per rank -- ssme_pf_shard_layout.  n_filters = 1; any resamp_sched: a step without a resampling draw exchanges
 * nothing but the tile sums and carries this rank's log-weights.  Per time step the host side (the C++ driver below, or
 * ssme_amd/sharded.py over torch.distributed) does:   all_gather of the tile sums / maxima  ->  ssme_pf_shard_plan (which source tiles each
 * rank's resampling touches)  ->  exchange of those tiles (cdf + particles)  ->  ssme_pf_shard_step.
 * The level-2 arithmetic, the RNG counters (global particle index) and the Gamma tables (global tile id) are those of
 * the unsharded filter, so a sharded run is bit-identical to ssme_pf_run_series with the same N and seed.
 * Buffers are the caller's device pointers; all launches go to the stream given to ssme_pf_set_stream.
 * Reference counterpart: none (the reference is single-process); the semantics reproduced are those of BSFilter::filter
 * driven by the log_like_eval loop (example/estimate_univ_svol.h:121-127), the decomposition is SURVEY.md section 8e's.
 * ============================================================================================ */
int ssme_pf_shard_create(const ssme_pf_config* cfg, int32_t rank, int32_t world, ssme_pf_handle* out);
/* out4 = { B (tiles of the filter), Bl (rows per rank in every layout), tiles this rank owns, particles this rank owns } */
int ssme_pf_shard_layout(ssme_pf_handle h, int32_t* out4);
/* Launch on the caller's HIP stream (hipStream_t as void*; NULL = the handle's own stream). */
int ssme_pf_set_stream(ssme_pf_handle h, void* hip_stream);
/* Uploads the series, draws the Gamma tables of all T steps (every rank holds all tiles' draws), resets the scalars. */
int ssme_pf_shard_prepare(ssme_pf_handle h, const double* y, const double* z, int32_t T);
/* Step t >= 1: from the gathered tile sums / maxima of step t-1 (device, world x Bl doubles each) the inclusive source-tile range
 * [lo, hi] of every rank: lo_hi_host[2*g], lo_hi_host[2*g+1].  Synchronises the stream. */
int ssme_pf_shard_plan(ssme_pf_handle h, const double* tsum_all, const double* tmax_all, int32_t t, int32_t* lo_hi_host);
/* One filter step on this rank's tiles.  x_win / cdf_win hold source tiles win_tile0 .. (at least) this rank's hi,
 * 2048 doubles per tile (ignored at t = 0); outputs: this rank's particles, integer cdf, tile sums and maxima.
 * anc_out (optional): global ancestor index of every output particle.  Accounts log p(y_{t-1} | .) on every rank. */
int ssme_pf_shard_step(ssme_pf_handle h, int32_t t, const double* x_win, const double* cdf_win, int32_t win_tile0,
                       const double* tsum_all, const double* tmax_all, double* x_out, double* cdf_out, double* tsum_out,
                       double* tmax_out, uint32_t* anc_out);
/* Accounts the log conditional likelihood of the last step t from its gathered tile arrays; then
 * ssme_pf_get_loglik / ssme_pf_get_per_step return the same values on every rank. */
int ssme_pf_shard_finalize(ssme_pf_handle h, int32_t t, const double* tsum_all, const double* tmax_all);

/* ---- the same loop in C++ over RCCL: a C or C++ caller of ssme needs no Python to use several GPUs ------------------------
 * RCCL is resolved at run time from what the process has loaded (dlsym; `librccl.so` from the loader path otherwise); this
 * library does not link against it.  comm = an ncclComm_t whose rank / size equal the handle's (pass your own, or make
 * one: rank 0 calls ssme_shard_comm_get_unique_id, ships the 128 bytes to the other ranks by any means, every rank calls
 * ssme_shard_comm_init).
 * ssme_pf_shard_run_series runs the whole series on the handle's stream.  mode 0: fixed-halo exchange with the two
 * neighbouring ranks and no host synchronisation inside the time loop; a device flag per rank records whether one of its
 * resampling windows ever left the halo, the flags are reduced over the ranks after the loop (ncclAllReduce, max), and if any is
 * set EVERY rank runs the series again on the exact path; mode 1: fixed halo only
 * (SSME_ERR_STATE if a window left it); mode 2: exact path (the plan is downloaded every step, exactly the planned tiles
 * travel between any two ranks).  Results are bit-identical to the unsharded filter on every path.  loglik_out: 1 value,
 * identical on every rank.  Buffers are owned by the handle. */
int ssme_shard_comm_get_unique_id(void* id128 /*128 bytes*/);
int ssme_shard_comm_init(const void* id128, int32_t rank, int32_t world, int32_t device, void** comm_out);
int ssme_shard_comm_destroy(void* comm);
int ssme_pf_shard_run_series(ssme_pf_handle h, void* nccl_comm, const double* y, const double* z, int32_t T, int32_t mode,
                             double* loglik_out);
/* after ssme_pf_shard_run_series: this rank's particles (ssme_pf_shard_layout's out4[3]) and integer cdf (nullable), the path the last series
 * took (1 fixed halo, 2 exact) and the number of tiles this rank received from other ranks */
int ssme_pf_shard_download(ssme_pf_handle h, double* x_local, uint64_t* cdf_local, int32_t* path, int64_t* exchanged_tiles);
/* after ssme_pf_shard_run_series, of its last FIXED-HALO pass: out4[0] = 1 if a resampling window left the halo on ANY rank (the
 * per-rank flags reduced by one ncclAllReduce(max) after the time loop -- every rank reads the same value, so every rank takes
 * the same fallback decision), out4[1] = this rank's own flag, out4[2] / out4[3] = widest reach left / right of the own tiles
 * where the split level-2 planned the exchange (0 otherwise) */
int ssme_pf_shard_stats(ssme_pf_handle h, int32_t* out4);

/* ============================================================================================
 * Liu-West filter: LWFilterWithCovs<nparts,1,1,1,4,float_t>::filter (include/ssme/liu_west_filter.h:971-1159)
 * with the model of svol_lw_1_par (test/test_liu_west.cpp:22-157): parameters (phi, mu, sigma, rho), one
 * transform per parameter (parameters.h:27 enum order: 0 null, 1 twice_fisher, 2 logit, 3 log), uniform priors,
 * shrinkage a = (3 delta - 1) / (2 delta), resampling of states and parameters every step (:91-145).
 * ============================================================================================ */
typedef struct ssme_lw_s* ssme_lw_handle;
typedef struct ssme_lw_config {
    int32_t  n_particles;       /* N per filter                                                        */
    int32_t  n_filters;         /* independent filters in this handle                                   */
    uint64_t seed;
    int32_t  device;
    uint32_t first_filter_id;
    double   delta;             /* discount factor, ctor argument `delta` (liu_west_filter.h:954-960)    */
    int32_t  transforms[4];     /* ctor argument `transforms`; svol_lw_1_par: logit, null, log, twice_fisher */
    double   prior_lo[4];       /* paramPriorSamp(): theta_d ~ U(lo_d, hi_d), test_liu_west.cpp:140-150  */
    double   prior_hi[4];
    int32_t  form;              /* 0: auxiliary-particle form, LWFilterWithCovs::filter (liu_west_filter.h:971-1159, model
                                   svol_lw_1_par); 1: SISR form, LWFilter2WithCovs::filter (:2191-2343, model svol_lw_2_par,
                                   test/test_liu_west.cpp:214-358)                                           */
    int32_t  resamp_sched;      /* m_rs / m_resampSched: resample when (t + 1) % m_rs == 0; 0 or 1 = every step (default) */
} ssme_lw_config;

int ssme_lw_create(const ssme_lw_config* cfg, ssme_lw_handle* out);
int ssme_lw_destroy(ssme_lw_handle h);
int ssme_lw_reset(ssme_lw_handle h);
/* filter(y_t, z_t): one step on every filter; logcondlike_out (R values) = getLogCondLike() */
int ssme_lw_step(ssme_lw_handle h, const double* y, const double* z, double* logcondlike_out);
/* T steps; loglik_out (R values) = sum of the log conditional likelihoods */
int ssme_lw_run_series(ssme_lw_handle h, const double* y, const double* z, int32_t T, double* loglik_out);
int ssme_lw_get_per_step(ssme_lw_handle h, double* out, int32_t T);
/* Liu-West filters of one tile (N <= 2048) can run ssme_lw_run_series as k_lw_init plus ONE launch that loops over steps
 * 1 .. T-1 with the population, the parameter records and the integer cdf in LDS, one workgroup of 512 threads per filter
 * (ssme_amd/csrc/lw_small.h).  enable = 1 takes that kernel where it applies (unsharded handle, N <= 2048), 0 forces the tiled
 * launches (two per step).  Results are bit-identical either way, and so is every call that follows the series.  The setting
 * survives ssme_lw_reset and ssme_lw_run_series.  NULL handle: SSME_ERR_INVALID_ARG; sharded handle: SSME_ERR_STATE.
 * Default of a new handle: see profiles/lw_series_timing.txt. */
int ssme_lw_set_small_series(ssme_lw_handle h, int32_t enable);
/* What ssme_lw_run_series launches for this handle as it is configured now: SSME_ROUTE_TILED or SSME_ROUTE_LW_SERIES, and the
 * threads per workgroup (512 on both).  Needs no prior step and makes no HIP call.  NULL arguments: SSME_ERR_INVALID_ARG;
 * sharded handle: SSME_ERR_STATE. */
int ssme_lw_get_series_route(ssme_lw_handle h, int32_t* route, int32_t* threads_per_block);
/* weighted means of the untransformed parameters under the last step's weights: out[r*4 + d] */
int ssme_lw_get_param_means(ssme_lw_handle h, double* out);
/* E[h | y_{1:t}] under the last step's (pre-resampling) weights for built-in functionals (the reference takes
 * std::function h(x, z, theta), liu_west_filter.h:1054-1075 / :2267-2290): ids 0-3 = SSME_H_X, SSME_H_X2, SSME_H_VOL,
 * SSME_H_CONST42 of the state; 4-7 = the untransformed parameters phi, mu, sigma, rho.  out[i*R + r]. */
int ssme_lw_get_expectations(ssme_lw_handle h, const int32_t* functionals, int32_t n, double* out);
/* Recorded series: with enable = 1 every following ssme_lw_run_series also stores, for every step t = 0 .. T-1 and every filter,
 * the eight values ssme_lw_get_expectations can return (E[x], E[x^2], E[exp(x/2)], E[42], E[phi], E[mu], E[sigma], E[rho] under
 * the pre-resampling second-stage weights of step t) -- the path of the parameter means and of the filtered state.  A switch with
 * no list of functionals: the read-out forms all eight in one pass.  The device buffer ([T][R][8] doubles) belongs to the handle,
 * is allocated by run_series while recording is on and freed by the first run_series with recording off.  enable is 0 or 1; the
 * default of a new handle is 0; the setting survives ssme_lw_reset, ssme_lw_run_series and ssme_lw_step (which neither records
 * nor clears).  Recording changes nothing else that any call returns.  Makes no HIP call.
 * NULL handle or enable outside {0, 1}: SSME_ERR_INVALID_ARG; sharded handle: SSME_ERR_STATE. */
int ssme_lw_set_series_expectations(ssme_lw_handle h, int32_t enable);
/* Rows 0 .. T-1 of the last recorded series: out[(t*n + i)*R + r] = E[functionals[i]] of filter r after step t, ids as for
 * ssme_lw_get_expectations (chosen here, at read time).  Row t equals, bit for bit and NaN for NaN, what
 * ssme_lw_get_expectations returns after step t of a handle of the same configuration and seed stepped with ssme_lw_step: for
 * both forms, any resamp_sched, and on both routes of ssme_lw_get_series_route.  Where a filter's weights are NaN, infinite or
 * all zero its rows are NaN and the call returns SSME_OK.
 * Checked before any HIP call: NULL handle, out or functionals, n outside 1..8, an id outside 0..7, T < 1 or T beyond the last
 * recorded series: SSME_ERR_INVALID_ARG; sharded handle: SSME_ERR_STATE; nothing recorded (recording was off during the last
 * ssme_lw_run_series, or there has been none): SSME_ERR_STATE. */
int ssme_lw_get_series_expectations(ssme_lw_handle h, const int32_t* functionals, int32_t n, double* out /* [T][n][R] */, int32_t T);
/* Arbitrary host-side h: particles x (N), UNTRANSFORMED parameters theta[d*N + i] (4N) and weights w (N) of one filter
 * after the last step, w_i = exp(logw_i - max logw) in the resampler's fixed point; any pointer but w may be NULL. */
int ssme_lw_download_weights(ssme_lw_handle h, int32_t filter, double* x, double* theta_untrans, double* w);
/* parity/debug: particles, transformed parameters theta[d*N + i] (getParamSamples()), k indices and resampling
 * ancestors of the last step (after set_debug(1)), theta-bar and the Cholesky factor of (1 - a^2) V (row-major 4x4) */
int ssme_lw_download_state(ssme_lw_handle h, int32_t filter, double* x, double* theta, uint32_t* kidx, uint32_t* ancestors,
                           double* thetabar, double* chol);
int ssme_lw_set_debug(ssme_lw_handle h, int32_t flags);
int ssme_lw_last_elapsed_ms(ssme_lw_handle h, float* ms);
/* Forecast of the Liu-West filters, both forms (sim_future_obs of the *FutureSimulator add-ons, liu_west_filter.h:1315-1363; see
 * ssme_pf_sim_future_obs for the start draw, the layout of y_out / x_out / start_out and the error codes).  The start population
 * carries its parameters; theta-bar and the Cholesky factor L of (1 - a^2) V, a = (3 delta - 1) / (2 delta), are taken once over its
 * transformed parameters; per horizon  theta <- a theta + (1 - a) theta-bar + L e,  x <- fSamp(x, y_prev, theta),
 * y <- exp(x / 2) z,  y_prev <- y.  last_obs: R values, required.  prop_out: [R][16] = theta-bar[4], L[10] (lower triangle by rows) as
 * used, 2 unused, or NULL. */
int ssme_lw_sim_future_obs(ssme_lw_handle h, int32_t num_steps, const double* last_obs /*R*/, double* y_out /*[R][num_steps][N]*/,
                           double* x_out /*same shape or NULL*/, uint32_t* start_out /*[R][N] or NULL*/, double* prop_out /*[R][16] or NULL*/);
int ssme_lw_forecast_elapsed_ms(ssme_lw_handle h, float* horizon_kernel_ms, float* call_ms);
const char* ssme_lw_last_error(ssme_lw_handle h);

/* ---- particle-sharded Liu-West filter: ONE filter of cfg->n_particles particles over `world` GPUs (BASELINE.json configs[4]).
 * Rank g owns tiles [g Bl, min((g+1) Bl, B)), Bl = ceil(B / world), as ssme_pf_shard_create lays a filter out (any n_particles
 * up to 2^25 with (world-1) Bl < B; ssme_lw_shard_layout); n_filters = 1; any resampling schedule (a step
 * without a resampling draw, t % resamp_sched != 0: ssme_lw_shard_stage1 is given this rank's OWN rows, win_tile0 = its first tile,
 * and nothing is exchanged for it; the handle carries the second-stage log-weights); both forms -- the SISR form, form = 1, has no k draw, so its stage 2 reads this rank's own stage-1 outputs and a step
 * has ONE window exchange instead of two).  Per step the
 * host side (ssme_amd/sharded.py, ShardedLiuWest) gathers the tile sums / maxima of the second-stage weights, plans and
 * exchanges windows of (cdfB, x, theta) for the resampling draw (stage 1), gathers the first-stage tile sums / maxima and
 * the 14 moment partials per tile, runs ssme_lw_shard_mid on every rank (theta-bar, Cholesky factor: the moment sums are
 * added in tile order, so every rank gets the unsharded filter's bits), plans and exchanges windows of (cdfA, lw1, x, theta)
 * for the k draw (stage 2) -- call ssme_lw_shard_plan(which = 1) BEFORE ssme_lw_shard_mid: above 1024 tiles the plan also
 * provides the first-stage (m, S) that mid turns into the log-sum-exp.  theta buffers hold one record of 4 doubles per particle:
 * rows of 2048 records ([tiles][2048][4]) that travel with their tile.  `win_tiles` of the two stage calls is accepted (>= 1) and not
 * read: the window's first tile is all a stage kernel needs to address its sources.  Bit-identical to ssme_lw_run_series. */
int ssme_lw_shard_create(const ssme_lw_config* cfg, int32_t rank, int32_t world, ssme_lw_handle* out);
int ssme_lw_shard_layout(ssme_lw_handle h, int32_t* out4);      /* as ssme_pf_shard_layout */
int ssme_lw_set_stream(ssme_lw_handle h, void* hip_stream);
int ssme_lw_shard_prepare(ssme_lw_handle h, const double* y, const double* z, int32_t T);
/* t = 0 on this rank's tiles: prior draws, q1Samp, first weights */
int ssme_lw_shard_init(ssme_lw_handle h, double* xB, double* thB, double* cdfB, double* tsumB, double* tmaxB);
/* which = 0: source-tile ranges of the resampling draw (from the gathered second-stage tile sums), 1: of the k draw
 * (from the gathered first-stage tile sums); lo_hi_host[2g], [2g+1] per rank.  Synchronises the stream. */
int ssme_lw_shard_plan(ssme_lw_handle h, int32_t which, int32_t t, const double* tsum_all, const double* tmax_all,
                       int32_t* lo_hi_host);
int ssme_lw_shard_stage1(ssme_lw_handle h, int32_t t, int32_t win_tile0, int32_t win_tiles, const double* w_xB, const double* w_thB,
                         const double* w_cdfB, const double* tsumB_all, const double* tmaxB_all, double* xr, double* thr, double* lw1,
                         double* cdfA, double* tsumA, double* tmaxA, double* mom /*[tiles][16]*/, uint32_t* anc);
int ssme_lw_shard_mid(ssme_lw_handle h, int32_t t, const double* tsumA_all, const double* tmaxA_all, const double* mom_all);
int ssme_lw_shard_stage2(ssme_lw_handle h, int32_t t, int32_t win_tile0, int32_t win_tiles, const double* w_xr, const double* w_thr,
                         const double* w_lw1, const double* w_cdfA, const double* tsumA_all, const double* tmaxA_all, double* xB,
                         double* thB, double* cdfB, double* tsumB, double* tmaxB, uint32_t* kidx);
/* accounts the last step t from its gathered second-stage tile sums; then ssme_lw_get_loglik / get_per_step */
int ssme_lw_shard_finalize(ssme_lw_handle h, int32_t t, const double* tsumB_all, const double* tmaxB_all);
/* The same loop in C++ over RCCL (see ssme_pf_shard_run_series; comm from ssme_shard_comm_init or the caller's own
 * ncclComm_t): fixed-halo exchange with the two neighbouring ranks, no host synchronisation inside the time loop.  The
 * stage kernels verify their own source tiles against the exchanged window; if one ever left it ON ANY RANK (flags reduced by
 * ncclAllReduce after the loop) the call returns SSME_ERR_STATE ON EVERY RANK and the caller runs the exact host-planned loop over the step-wise entry points above.  loglik_out: 1. */
int ssme_lw_shard_run_series(ssme_lw_handle h, void* nccl_comm, const double* y, const double* z, int32_t T, double* loglik_out);
/* after ssme_lw_shard_run_series: this rank's n particles (ssme_lw_shard_layout), transformed parameters theta[d * n + i], tiles received */
int ssme_lw_shard_download(ssme_lw_handle h, double* x_local, double* theta_local, int64_t* exchanged_tiles);
/* as ssme_pf_shard_stats: out4[0] the reduced flag (SSME_ERR_STATE was returned on EVERY rank if it is set), out4[1] this rank's own */
int ssme_lw_shard_stats(ssme_lw_handle h, int32_t* out4);
int ssme_lw_get_loglik(ssme_lw_handle h, double* out);


const char* ssme_pf_strerror(int status);
const char* ssme_pf_last_error(ssme_pf_handle h);
int ssme_pf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SSME_PF_H */
