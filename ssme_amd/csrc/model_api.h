// model_api.h -- the model extension point of the bootstrap-filter kernels.
//
// The reference's models are five virtual callbacks on a class derived from pf::filters::BSFilter
// (example/univ_svol_bootstrap_filter.h:37-41: logQ1Ev, logMuEv, logGEv, fSamp, q1Samp).  Host virtuals cannot run per
// particle on a GPU, so a model here is a POLICY: a struct of static functions compiled into the step kernels.  The three
// built-in models (svol_bs, svol_leverage, linear Gaussian) are written against the same interface below, and ONE more
// model can be compiled in without touching a kernel:
//
//     python -c "from ssme_amd import build; print(build.build_user_model('path/to/my_model.h', 'mymodel'))"
//         -> build/user/libssme_pf_mymodel.so          (hipcc ... -DSSME_USER_MODEL_HEADER="path/to/my_model.h")
//     SSME_PF_LIB=build/user/libssme_pf_mymodel.so ...      ssme_pf_config::model = SSME_MODEL_USER0
//
// The header defines `struct ssme_user_model0` with
//     static constexpr int n_theta = ...;                         // length of the untransformed parameter vector (<= 8)
//     static ssme::ModelConst derive(const double* theta);           // per-filter constants a0..a6, computed ONCE on the host:
//                                                                  // a2 is the standard deviation of the t = 0 draw
//                                                                  // x_0 = a2 * z (q1Samp with logMuEv == logQ1Ev, as in
//                                                                  // both reference models); bad != 0 => logG = -inf
//     static __device__ double prop(const ssme::ModelConst& c, double x, double zn, double zcov, const ssme::ExpTabEntry* etab);
//                                                                  // fSamp: the new state from x, a standard normal zn
//                                                                  // and the covariate
//     static __device__ double logg(const ssme::ModelConst& c, double y, double x, const ssme::ExpTabEntry* etab);
//                                                                  // logGEv
// using only + - * fma and the functions of ssme_math.h (dexp_scaled_t(x, 0, etab), dlog, dsqrt, ...): fixed IEEE operation
// sequences, so that a CPU restatement of the same sequence reproduces the filter bit for bit (the parity test of
// tests/models/svol_student_t.h does exactly that against the oracle's callback-driven model).
//
// VECTOR state / observation (BSFilter<nparts, dimx, dimy, ...> with dimx, dimy > 1; up to 4 each).  The header adds
//     static constexpr int dim_x = 2, dim_y = 1;
//     static __device__ void init_vec(const ssme::ModelConst& c, const double* zn, double* x0);
//                                                                  // q1Samp: x_0 from dim_x standard normals
//     static __device__ void prop_vec(const ssme::ModelConst& c, const double* x, const double* zn, double zcov, double* xn,
//                                     const ssme::ExpTabEntry* etab);      // fSamp: dim_x normals in, dim_x components out
//     static __device__ double logg_vec(const ssme::ModelConst& c, const double* y, const double* x, const ssme::ExpTabEntry* etab);
// INSTEAD of prop / logg.  Particles are stored as dim_x planes ([dim_x][n_filters][N]; ssme_pf_download_state returns them in that
// order), a series is T rows of dim_y values, component 0 of the normals is the pair's Box-Muller draw of the scalar kernels and
// component d >= 1 comes from one more Philox call per particle pair (counter stream STREAM_XDIM + d).  Such a model is unsharded;
// at N <= 2048 ssme_pf_run_series runs its whole series in one launch with all dim_x planes in LDS, like a scalar model
// (pf_small.h; ssme_pf_get_series_route says which route a handle takes); device functionals see component 0.
// tests/models/svol_two_factor.h is the test model (two volatility factors, two observed series).
//
// FUNCTIONALS of the model's own (optional; getExpectations() of the functions h the reference's callers pass to filter(y[, z], fs),
// pswarm_filter.h:47,340: h(x, z, theta)).  Host std::functions cannot run per particle either, so the header may declare
//     static constexpr int n_h = K;                                // 1 .. 16 scalar outputs: a mean vector, the entries of a moment matrix, ...
//     static __device__ __forceinline__ void h(const ssme::ModelConst& c, const double* x /*dim_x*/, double zcov,
//                                              const ssme::ExpTabEntry* etab, double* out /*n_h*/);
// and they are compiled into an expectation kernel of their own (user_expect.h): E[h_k(x_t) | y_{1:t}] for all K outputs in one pass
// over the particles, with the weights the built-in functionals and the resampler use.  x is the WHOLE state of one particle (a scalar
// model gets x[0]), zcov the covariate of the last step (as for prop; 0 when the step had none), theta reaches h through c, and etab is
// what logg receives (dexp_scaled_t(v, 0, etab)).  The same rule holds as for the callbacks: only + - * fma and the functions of
// ssme_math.h, written so that out[] and x[] stay in registers (constant indices; the build refuses kernels that use scratch memory).
// Callers: ssme_pf_user_model_n_h / ssme_pf_get_user_expectations / ssme_pf_swarm_aggregate_user (include/ssme_pf.h),
// user_bs_gpu::getModelExpectations (bsfilter_gpu.hpp), ParticleFilterBank.user_expectations / swarm_aggregate_user.  A header
// without n_h compiles and behaves as before (n_h reads 0).  tests/models/svol_two_factor_h.h declares seven of them.
//
// OBSERVATION DRAW (optional; gSamp of the reference's FutureSimulator add-on, test/test_pswarm.cpp:64-67, 112-116).  A header that
// declares it can be forecast: ssme_pf_sim_future_obs simulates from the model on the device (forecast.h).
//     static __device__ double gsamp(const ssme::ModelConst& c, double x, double zo, const ssme::ExpTabEntry* etab);     // scalar model
//     static __device__ void gsamp_vec(const ssme::ModelConst& c, const double* x /*dim_x*/, const double* zo /*dim_y*/,
//                                      double* y /*dim_y*/, const ssme::ExpTabEntry* etab);                              // vector model
// y from the state and dim_y standard normals, under the rules of the other callbacks (+ - * fma, ssme_math.h; constant indices).
// A plain `/` and ssme::dsqrt are within those rules in every callback: both are correctly rounded on the device under the library's
// flags (-fno-fast-math), as on the host, so a restatement reproduces them (lin_gauss_4d_h.h's init_vec, lin_gauss_4d_g.h's gsamp_vec).
// What is excluded is libm (exp, log, pow, sin ...), whose results differ between the two.
// A simulated step is x <- prop / prop_vec(c, x, zs, zcov = y_prev[0]), y <- gsamp / gsamp_vec(c, x, zo): the covariate of a
// simulated step is component 0 of the previous simulated observation (fSamp(x, y_prev) of the reference, the built-in leverage
// model's convention).  A model whose covariates are exogenous declares dim_cov and is forecast with future covariates (below).
// A header without the draw compiles and behaves as before (ssme_pf_user_model_has_gsamp reads 0, a forecast is
// SSME_ERR_UNSUPPORTED).  tests/models/svol_leverage_user.h, svol_two_factor_g.h, lin_gauss_3d_g.h, lin_gauss_4d_g.h declare it.
//
// TRANSITION DENSITY (optional; what backward-simulation smoothing needs: ssme_pf_sample_trajectories_backward, backward.h, DESIGN.md
// section 12.1).  A header that declares it can be smoothed by backward simulation:
//     static __device__ double logf(const ssme::ModelConst& c, double xn, double x, double zcov, const ssme::ExpTabEntry* etab);   // scalar model
//     static __device__ double logf_vec(const ssme::ModelConst& c, const double* xn /*dim_x*/, const double* x /*dim_x*/, double zcov,
//                                       const ssme::ExpTabEntry* etab);                                                         // vector model
// log f(xn | x, zcov), the density of the header's own prop / prop_vec, up to a constant that does not depend on x (it cancels in the
// backward weights); zcov is the covariate of the step that made xn and is `const double*` in a dim_cov header, as in every callback.
// The rules of the other callbacks hold.  A header without it compiles and behaves as before (ssme_pf_user_model_has_logf reads 0, the
// backward call is SSME_ERR_UNSUPPORTED).  tests/models/svol_student_t_f.h, svol_two_factor_f.h and svol_reg_cov_f.h declare it.
//
// COVARIATES (optional; pf::filters::BSFilterWC<nparts, dimx, dimy, dimcov, ...> of the reference, pswarm_filter.h:309-352: z_t enters
// fSamp, logGEv, q1Samp, logMuEv, logQ1Ev and the functionals).  A header that declares
//     static constexpr int dim_cov = K;                            // 1 .. 4 covariates per step
// opts in: its callbacks keep their names and receive ALL K covariates of the step as `const double* zcov` (constant indices only,
// like y and x), in every callback, not only in prop:
//                  without dim_cov                                  with dim_cov
//     scalar       prop(c, x, zn, double zcov, etab)                prop(c, x, zn, const double* zcov, etab)
//                  logg(c, y, x, etab)                              logg(c, y, x, const double* zcov, etab)
//                  gsamp(c, x, zo, etab)                            gsamp(c, x, zo, const double* zcov, etab)
//     vector       prop_vec(c, x, zn, double zcov, xn, etab)        prop_vec(c, x, zn, const double* zcov, xn, etab)
//                  logg_vec(c, y, x, etab)                          logg_vec(c, y, x, const double* zcov, etab)
//                  gsamp_vec(c, x, zo, y, etab)                     gsamp_vec(c, x, zo, const double* zcov, y, etab)
//     functionals  h(c, x, double zcov, etab, out)                  h(c, x, const double* zcov, etab, out)
// filter(y_t, z_t) uses the same z_t for fSamp into x_t and for logGEv of y_t, as BSFilterWC::filter does; one z_t serves all filters
// of a handle; z = NULL means zeros.  Callers pass K values per step (ssme_pf_step) or z[t * K + j] (ssme_pf_run_series); h receives
// the covariates of the last step.  A dim_cov model of at most 2048 particles, scalar or vector, still runs the whole series in one launch.
// FIRST STEP of its own (optional, dim_cov headers only; both or neither -- one without the other is a static_assert):
//     static __device__ void first(const ssme::ModelConst& c, const double* zn /*dim_x*/, const double* y /*dim_y*/,
//                                  const double* zcov, double* x0 /*dim_x*/, const ssme::ExpTabEntry* etab);           // q1Samp(y1, z1)
//     static __device__ double first_logw(const ssme::ModelConst& c, const double* y, const double* x0, const double* zcov,
//                                         const ssme::ExpTabEntry* etab);                  // logMuEv(x1, z1) - logQ1Ev(x1, y1, z1)
// At t = 0 the particle is first(...) and its log-weight first_logw(...) + logg(...) (-inf for a `bad` filter, as ever); a2 and
// init_vec are then not read at t = 0.  The normals are those the first step draws anyway: component 0 the pair's Box-Muller draw,
// component d >= 1 from stream STREAM_XDIM + d -- no Philox counter changes and every step consumes the random numbers it did.
// Scalar models use the pointer forms with one element.  A model WITHOUT covariates that wants its own first step declares
// dim_cov = 1, is run with z = NULL and reads zcov[0] == 0.
// FORECAST of a dim_cov model: its covariates are exogenous, so the caller supplies those of the horizons
// (ssme_pf_sim_future_obs_cov: z_future[k * K + j]) and a simulated step is x <- prop / prop_vec(c, x, zs, z_k),
// y <- gsamp / gsamp_vec(c, x, zo, z_k); the previous simulated observation is NOT a covariate of such a model, and
// ssme_pf_sim_future_obs is SSME_ERR_UNSUPPORTED for it.  Start draw and counters are those of every forecast.
// Such models are unsharded.  ssme_pf_user_model_dim_cov / ssme_pf_user_model_has_first report what the header declares;
// user_bswc_gpu (bsfilter_gpu.hpp) is the BSFilterWC-shaped caller.  tests/models/svol_reg_cov.h (K = 3, first, gsamp, n_h = 3),
// svol_reg_cov_nofirst.h, svol_leverage_cov1.h (K = 1) and svol_two_factor_cov.h ((dim_x, dim_y, K) = (2, 2, 4)) are the test models.
#pragma once
#include <type_traits>
#include "ssme_math.h"

namespace ssme {

// Derived per-filter constants (the host computes them with the same ssme_math functions).
struct ModelConst {
    double a0, a1, a2, a3, a4, a5, a6;
    int32_t bad;
    int32_t pad;
};

enum { MODEL_SVOL = 0, MODEL_SVOL_LEVERAGE = 1, MODEL_LIN_GAUSS = 2, MODEL_USER0 = 3 };

}  // namespace ssme

#ifdef SSME_USER_MODEL_HEADER
#include SSME_USER_MODEL_HEADER
#define SSME_HAS_USER_MODEL 1
#else
#define SSME_HAS_USER_MODEL 0
#endif

namespace ssme {
constexpr int kMaxDim = 4;                 // largest dim_x / dim_y of a user model
enum { STREAM_XDIM = 96 };                 // counter stream of state component d >= 1: STREAM_XDIM + d
template <class M, class = void> struct user_dims { static constexpr int dx = 1, dy = 1; };
template <class M> struct user_dims<M, std::void_t<decltype(M::dim_x), decltype(M::dim_y)>> {
    static constexpr int dx = M::dim_x, dy = M::dim_y;
    static_assert(dx >= 1 && dx <= kMaxDim && dy >= 1 && dy <= kMaxDim, "dim_x and dim_y of a user model: 1 .. 4");
};
// number of functionals a user model declares (n_h and h above): 0 for a header without them
constexpr int kMaxUserFunctionals = 16;
template <class M, class = void> struct user_nh { static constexpr int n = 0; };
template <class M> struct user_nh<M, std::void_t<decltype(M::n_h)>> {
    static constexpr int n = M::n_h;
    static_assert(n >= 1 && n <= kMaxUserFunctionals, "n_h of a user model: 1 .. 16");
};
// does the header declare the observation draw, in the form its dimensions ask for (gsamp / gsamp_vec above)?
template <class M, class = void> struct declares_gsamp : std::false_type {};
template <class M> struct declares_gsamp<M, std::void_t<decltype(&M::gsamp)>> : std::true_type {};
template <class M, class = void> struct declares_gsamp_vec : std::false_type {};
template <class M> struct declares_gsamp_vec<M, std::void_t<decltype(&M::gsamp_vec)>> : std::true_type {};
template <class M> struct user_gsamp {
    static constexpr bool vec = user_dims<M>::dx > 1 || user_dims<M>::dy > 1;
    static_assert(!(vec && declares_gsamp<M>::value && !declares_gsamp_vec<M>::value),
                  "a vector user model (dim_x or dim_y > 1) declares its observation draw as gsamp_vec, not gsamp");
    static_assert(!(!vec && declares_gsamp_vec<M>::value && !declares_gsamp<M>::value),
                  "a scalar user model declares its observation draw as gsamp, not gsamp_vec");
    static constexpr bool has = vec ? declares_gsamp_vec<M>::value : declares_gsamp<M>::value;
};
// does the header declare the transition log-density, in the form its dimensions ask for (logf / logf_vec above)?
template <class M, class = void> struct declares_logf : std::false_type {};
template <class M> struct declares_logf<M, std::void_t<decltype(&M::logf)>> : std::true_type {};
template <class M, class = void> struct declares_logf_vec : std::false_type {};
template <class M> struct declares_logf_vec<M, std::void_t<decltype(&M::logf_vec)>> : std::true_type {};
template <class M> struct user_logf {
    static constexpr bool vec = user_dims<M>::dx > 1 || user_dims<M>::dy > 1;
    static_assert(!(vec && declares_logf<M>::value && !declares_logf_vec<M>::value),
                  "a vector user model (dim_x or dim_y > 1) declares its transition density as logf_vec, not logf");
    static_assert(!(!vec && declares_logf_vec<M>::value && !declares_logf<M>::value),
                  "a scalar user model declares its transition density as logf, not logf_vec");
    static constexpr bool has = vec ? declares_logf_vec<M>::value : declares_logf<M>::value;
};
// COVARIATES (dim_cov above): how many a user model declares, 0 for a header without them
constexpr int kMaxCov = 4;
template <class M, class = void> struct user_cov { static constexpr int k = 0; };
template <class M> struct user_cov<M, std::void_t<decltype(M::dim_cov)>> {
    static constexpr int k = M::dim_cov;
    static_assert(k >= 1 && k <= kMaxCov, "dim_cov of a user model: 1 .. 4");
};
// does a dim_cov header declare a first step of its own (first AND first_logw above)?
template <class M, class = void> struct declares_first : std::false_type {};
template <class M> struct declares_first<M, std::void_t<decltype(&M::first)>> : std::true_type {};
template <class M, class = void> struct declares_first_logw : std::false_type {};
template <class M> struct declares_first_logw<M, std::void_t<decltype(&M::first_logw)>> : std::true_type {};
template <class M> struct user_first {
    static_assert(declares_first<M>::value == declares_first_logw<M>::value,
                  "a user model declares both first and first_logw, or neither");
    static_assert(!declares_first<M>::value || user_cov<M>::k > 0,
                  "first / first_logw belong to a header that declares dim_cov (dim_cov = 1 for a model without covariates)");
    static constexpr bool has = declares_first<M>::value && declares_first_logw<M>::value;
};
// what the kernels call: a scalar model through its prop / logg, a vector model through its *_vec functions (the other set is a
// stub that no launch reaches: vector models never run the scalar kernels and the other way round).  COV selects the grammar: a
// header without dim_cov takes one scalar covariate into prop only, one with dim_cov takes `const double* zcov` everywhere.
template <class M, bool VEC = (user_dims<M>::dx > 1 || user_dims<M>::dy > 1), bool COV = (user_cov<M>::k > 0)> struct user_calls;
template <class M> struct user_calls<M, false, false> {
    static __device__ __forceinline__ double prop(const ModelConst& c, double x, double zn, double zcov, const ExpTabEntry* etab) { return M::prop(c, x, zn, zcov, etab); }
    static __device__ __forceinline__ double logg(const ModelConst& c, double y, double x, const ExpTabEntry* etab) { return M::logg(c, y, x, etab); }
    static __device__ __forceinline__ void init_vec(const ModelConst& c, const double* zn, double* x0) { x0[0] = zn[0] * c.a2; }
    static __device__ __forceinline__ void prop_vec(const ModelConst& c, const double* x, const double* zn, double zcov, double* xn, const ExpTabEntry* etab) { xn[0] = M::prop(c, x[0], zn[0], zcov, etab); }
    static __device__ __forceinline__ double logg_vec(const ModelConst& c, const double* y, const double* x, const ExpTabEntry* etab) { return M::logg(c, y[0], x[0], etab); }
    static __device__ __forceinline__ void gsamp_vec(const ModelConst& c, const double* x, const double* zo, double* y, const ExpTabEntry* etab) { y[0] = M::gsamp(c, x[0], zo[0], etab); }
    static __device__ __forceinline__ double logf(const ModelConst& c, double xn, double x, double zcov, const ExpTabEntry* etab) { return M::logf(c, xn, x, zcov, etab); }
    static __device__ __forceinline__ double logf_vec(const ModelConst& c, const double* xn, const double* x, double zcov, const ExpTabEntry* etab) { return M::logf(c, xn[0], x[0], zcov, etab); }
};
template <class M> struct user_calls<M, true, false> {
    static __device__ __forceinline__ double prop(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logg(const ModelConst&, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ void init_vec(const ModelConst& c, const double* zn, double* x0) { M::init_vec(c, zn, x0); }
    static __device__ __forceinline__ void prop_vec(const ModelConst& c, const double* x, const double* zn, double zcov, double* xn, const ExpTabEntry* etab) { M::prop_vec(c, x, zn, zcov, xn, etab); }
    static __device__ __forceinline__ double logg_vec(const ModelConst& c, const double* y, const double* x, const ExpTabEntry* etab) { return M::logg_vec(c, y, x, etab); }
    static __device__ __forceinline__ void gsamp_vec(const ModelConst& c, const double* x, const double* zo, double* y, const ExpTabEntry* etab) { M::gsamp_vec(c, x, zo, y, etab); }
    static __device__ __forceinline__ double logf(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logf_vec(const ModelConst& c, const double* xn, const double* x, double zcov, const ExpTabEntry* etab) { return M::logf_vec(c, xn, x, zcov, etab); }
};
// dim_cov headers: the kernels reach them through the vector forms alone (cov_step / cov_sim below); the scalar-covariate
// entry points of the other grammar are stubs that no launch of such a model reaches
template <class M> struct user_calls<M, false, true> {
    static __device__ __forceinline__ double prop(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logg(const ModelConst&, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ void init_vec(const ModelConst& c, const double* zn, double* x0) { x0[0] = zn[0] * c.a2; }
    static __device__ __forceinline__ void prop_vec(const ModelConst& c, const double* x, const double* zn, const double* zcov, double* xn, const ExpTabEntry* etab) { xn[0] = M::prop(c, x[0], zn[0], zcov, etab); }
    static __device__ __forceinline__ double logg_vec(const ModelConst& c, const double* y, const double* x, const double* zcov, const ExpTabEntry* etab) { return M::logg(c, y[0], x[0], zcov, etab); }
    static __device__ __forceinline__ void gsamp_vec(const ModelConst& c, const double* x, const double* zo, const double* zcov, double* y, const ExpTabEntry* etab) { y[0] = M::gsamp(c, x[0], zo[0], zcov, etab); }
    static __device__ __forceinline__ double logf(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logf_vec(const ModelConst& c, const double* xn, const double* x, const double* zcov, const ExpTabEntry* etab) { return M::logf(c, xn[0], x[0], zcov, etab); }
};
template <class M> struct user_calls<M, true, true> {
    static __device__ __forceinline__ double prop(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logg(const ModelConst&, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ void init_vec(const ModelConst& c, const double* zn, double* x0) { M::init_vec(c, zn, x0); }
    static __device__ __forceinline__ void prop_vec(const ModelConst& c, const double* x, const double* zn, const double* zcov, double* xn, const ExpTabEntry* etab) { M::prop_vec(c, x, zn, zcov, xn, etab); }
    static __device__ __forceinline__ double logg_vec(const ModelConst& c, const double* y, const double* x, const double* zcov, const ExpTabEntry* etab) { return M::logg_vec(c, y, x, zcov, etab); }
    static __device__ __forceinline__ void gsamp_vec(const ModelConst& c, const double* x, const double* zo, const double* zcov, double* y, const ExpTabEntry* etab) { M::gsamp_vec(c, x, zo, zcov, y, etab); }
    static __device__ __forceinline__ double logf(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logf_vec(const ModelConst& c, const double* xn, const double* x, const double* zcov, const ExpTabEntry* etab) { return M::logf_vec(c, xn, x, zcov, etab); }
};
// One filter step of one particle of a dim_cov model: xn <- first (t = 0, when declared; init_vec / a2 * zn otherwise) or prop,
// and the increment of its log-weight: [first_logw +] logg, -inf for a `bad` filter.  x, zn, xn: dim_x values; y: dim_y; zcov: dim_cov.
template <class M>
__device__ __forceinline__ double cov_step(const ModelConst& c, bool first_step, const double* x, const double* zn, const double* y,
                                           const double* zcov, double* xn, const ExpTabEntry* etab) {
    using UC = user_calls<M>;
    double g;
    if (first_step) {
        if constexpr (user_first<M>::has) {
            M::first(c, zn, y, zcov, xn, etab);
            g = M::first_logw(c, y, xn, zcov, etab) + UC::logg_vec(c, y, xn, zcov, etab);
        } else {
            UC::init_vec(c, zn, xn);
            g = UC::logg_vec(c, y, xn, zcov, etab);
        }
    } else {
        UC::prop_vec(c, x, zn, zcov, xn, etab);
        g = UC::logg_vec(c, y, xn, zcov, etab);
    }
    return c.bad ? -dinf() : g;
}
// The weight part of cov_step alone, for a particle xn that exists already (backward.h recomputes the log-weights of a recorded
// series from its populations): [first_logw +] logg in cov_step's own order, -inf for a `bad` filter.
template <class M>
__device__ __forceinline__ double cov_logw(const ModelConst& c, bool first_step, const double* y, const double* zcov, const double* xn,
                                           const ExpTabEntry* etab) {
    using UC = user_calls<M>;
    double g;
    if (first_step) {
        if constexpr (user_first<M>::has) g = M::first_logw(c, y, xn, zcov, etab) + UC::logg_vec(c, y, xn, zcov, etab);
        else g = UC::logg_vec(c, y, xn, zcov, etab);
    } else g = UC::logg_vec(c, y, xn, zcov, etab);
    return c.bad ? -dinf() : g;
}
#if SSME_HAS_USER_MODEL
template <int MODEL> constexpr int model_dx() { return MODEL == MODEL_USER0 ? user_dims<ssme_user_model0>::dx : 1; }
template <int MODEL> constexpr int model_dy() { return MODEL == MODEL_USER0 ? user_dims<ssme_user_model0>::dy : 1; }
template <int MODEL> constexpr int model_kcov() { return MODEL == MODEL_USER0 ? user_cov<ssme_user_model0>::k : 0; }
// the user model as a type that depends on the kernel's MODEL, so that a discarded `if constexpr` branch is not checked against
// the other covariate grammar
template <int MODEL> struct user_model_of { using type = ssme_user_model0; };
#else
template <int MODEL> constexpr int model_dx() { return 1; }
template <int MODEL> constexpr int model_dy() { return 1; }
template <int MODEL> constexpr int model_kcov() { return 0; }
#endif
// the covariates of one step as the kernels hold them: KC uniform values (one slot when KC = 0, never read)
template <int KC> struct CovVals {
    double v[KC > 0 ? KC : 1];
    // row `row` of the covariates z[rows][KC] of a series
    __device__ __forceinline__ void load(const double* z, size_t row) {
#pragma unroll
        for (int j = 0; j < KC; ++j) v[j] = z[row * KC + j];
    }
};
}  // namespace ssme
