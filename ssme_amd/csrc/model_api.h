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
// component d >= 1 comes from one more Philox call per particle pair (counter stream STREAM_XDIM + d).  Such a model runs on the
// tiled step kernel at every N (no whole-series kernel), unsharded; device functionals see component 0.
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
// model's convention).  A model whose covariate is exogenous cannot be forecast without future covariates; that is not offered.
// A header without the draw compiles and behaves as before (ssme_pf_user_model_has_gsamp reads 0, a forecast is
// SSME_ERR_UNSUPPORTED).  tests/models/svol_leverage_user.h, svol_two_factor_g.h, lin_gauss_3d_g.h, lin_gauss_4d_g.h declare it.
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
// what the kernels call: a scalar model through its prop / logg, a vector model through its *_vec functions (the other set is a
// stub that no launch reaches: vector models never run the scalar kernels and the other way round)
template <class M, bool VEC = (user_dims<M>::dx > 1 || user_dims<M>::dy > 1)> struct user_calls;
template <class M> struct user_calls<M, false> {
    static __device__ __forceinline__ double prop(const ModelConst& c, double x, double zn, double zcov, const ExpTabEntry* etab) { return M::prop(c, x, zn, zcov, etab); }
    static __device__ __forceinline__ double logg(const ModelConst& c, double y, double x, const ExpTabEntry* etab) { return M::logg(c, y, x, etab); }
    static __device__ __forceinline__ void init_vec(const ModelConst& c, const double* zn, double* x0) { x0[0] = zn[0] * c.a2; }
    static __device__ __forceinline__ void prop_vec(const ModelConst& c, const double* x, const double* zn, double zcov, double* xn, const ExpTabEntry* etab) { xn[0] = M::prop(c, x[0], zn[0], zcov, etab); }
    static __device__ __forceinline__ double logg_vec(const ModelConst& c, const double* y, const double* x, const ExpTabEntry* etab) { return M::logg(c, y[0], x[0], etab); }
    static __device__ __forceinline__ void gsamp_vec(const ModelConst& c, const double* x, const double* zo, double* y, const ExpTabEntry* etab) { y[0] = M::gsamp(c, x[0], zo[0], etab); }
};
template <class M> struct user_calls<M, true> {
    static __device__ __forceinline__ double prop(const ModelConst&, double, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ double logg(const ModelConst&, double, double, const ExpTabEntry*) { return 0.0; }
    static __device__ __forceinline__ void init_vec(const ModelConst& c, const double* zn, double* x0) { M::init_vec(c, zn, x0); }
    static __device__ __forceinline__ void prop_vec(const ModelConst& c, const double* x, const double* zn, double zcov, double* xn, const ExpTabEntry* etab) { M::prop_vec(c, x, zn, zcov, xn, etab); }
    static __device__ __forceinline__ double logg_vec(const ModelConst& c, const double* y, const double* x, const ExpTabEntry* etab) { return M::logg_vec(c, y, x, etab); }
    static __device__ __forceinline__ void gsamp_vec(const ModelConst& c, const double* x, const double* zo, double* y, const ExpTabEntry* etab) { M::gsamp_vec(c, x, zo, y, etab); }
};
#if SSME_HAS_USER_MODEL
template <int MODEL> constexpr int model_dx() { return MODEL == MODEL_USER0 ? user_dims<ssme_user_model0>::dx : 1; }
template <int MODEL> constexpr int model_dy() { return MODEL == MODEL_USER0 ? user_dims<ssme_user_model0>::dy : 1; }
#else
template <int MODEL> constexpr int model_dx() { return 1; }
template <int MODEL> constexpr int model_dy() { return 1; }
#endif
}  // namespace ssme
