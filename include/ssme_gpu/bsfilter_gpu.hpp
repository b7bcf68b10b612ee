// bsfilter_gpu.hpp -- header-only C++ adaptor: the caller-visible surface of ssme's bootstrap-filter
// models over the C ABI of include/ssme_pf.h.
//
// Reference surface reproduced (files under /root/reference):
//   svol_bs<nparts,dimx,dimy,resampT,float_t>               example/univ_svol_bootstrap_filter.h:17-61
//       ctor (phi, beta, sigma); ctor from param::pack<float_t,3> in the order beta, phi, ss (sigma = sqrt(ss))
//       void filter(const osv&);  float_t getLogCondLike() const;          example/estimate_univ_svol.h:124-125
//   svol_leverage<nparts,resampT,float_t> : BSFilterWC<...>                test/test_pswarm.cpp:32-76
//       default ctor + copy-assign (Swarm requires both, pswarm_filter.h:292), ctor (phi, mu, sigma, rho, dte)
//       void filter(const osv&, const cvsv&, const std::vector<func>&); getExpectations(); getLogCondLike()
//                                                                          include/ssme/pswarm_filter.h:380-388
//   typedefs float_type, dynamic_matrix, func                              include/ssme/pswarm_filter.h:29,41,44
// The classes are templated on the pack / vector / matrix types (duck typing), so they compile with the reference's
// Eigen-based param::pack, Eigen vectors and Eigen dynamic matrices as well as with plain stand-ins (tests/cpp).
// svol_leverage_gpu satisfies what the UNMODIFIED Swarm / SwarmWithCovs templates ask of ModType
// (pswarm_filter.h:29-60,86-92,272-304,380-388): float_type / dynamic_matrix / func typedefs with func a
// std::function returning a dynamic matrix, default ctor + copy-assign, filter(y, z, const std::vector<func>&),
// std::vector<dynamic_matrix> getExpectations(), and -- through the optional `Base` template parameter -- inheritance
// from pf::bases::pf_withcov_base<float_t,dimy,dimx,dimcov>, so that the static_assert at :352 holds as written.
// Host std::function callbacks cannot run on the device.  By default every h in fs is evaluated ON THE HOST over the
// particles and weights of the member (one ssme_pf_download_weights per filter() call) -- correct for every h, of any
// shape, stateful or not.  The device functionals (SSME_H_*: x, x^2, exp(x/2), the constant 42) are used only when the
// caller says so: gpu_options::declared_functionals[j] = SSME_H_* declares that fs[j] of every filter() call IS that
// functional (the swarm templates hand their functions over as std::bind objects inside std::function, so a tag on the
// function itself would not survive; the user who writes instantiate_mod knows the swarm's functions).
// gpu_options::probe_functionals = true (opt-in, off by default since round 3) additionally classifies undeclared functions
// by evaluating them at six fixed states; a function that only differs from x / x^2 / exp(x/2) / a constant OUTSIDE
// [-1.7, 3.25] (a tail indicator, a clamp) is misclassified by such a probe, which is why it is no longer the default.
// Every model object draws its own random stream (the reference clock-seeds each object): the filter id defaults to a
// process-wide counter.  Errors: std::invalid_argument / std::runtime_error, as the reference throws; NaN/-inf are values.
// What the classes share is written once, in the first namespace detail below: weighted_mean (every host sum
// sum_i h(x_i) w_i / sum_i w_i: swarm members, Liu-West, user models), classify (the six-probe classifier, with 0 or 4
// parameter columns), dispatch_expectations (declared -> probe -> one device call -> one lazy download -> results in the
// caller's order; the declared range and the cap on device functionals are arguments), column0 / svol_theta (series and pack
// of the two log-likelihood evaluators).  detail::user_core carries user_bs_gpu and user_bswc_gpu, detail::member_core the two
// swarm-member models, detail::swarm_impl swarm_gpu and swarm_with_covs_gpu.
#ifndef SSME_GPU_BSFILTER_GPU_HPP
#define SSME_GPU_BSFILTER_GPU_HPP

#include <array>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <functional>
#include <fstream>
#include <limits>
#include <sstream>
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../ssme_pf.h"

namespace ssme_gpu {

inline void check(int status, ssme_pf_handle h = nullptr) {
    if (status == SSME_OK) return;
    std::string msg = ssme_pf_strerror(status);
    if (h && status == SSME_ERR_HIP) msg += std::string(" (") + ssme_pf_last_error(h) + ")";
    if (status == SSME_ERR_INVALID_ARG || status == SSME_ERR_LENGTH) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}

// RAII owner of one C-ABI handle holding R filters.
class handle {
public:
    handle() = default;
    handle(int model, int nparts, int nfilters, std::uint64_t seed, int resampler, int rs, int device, unsigned first_id,
           int dtype = SSME_F64, int bank_filters = 0) {
        ssme_pf_config c{};
        c.model = model; c.n_particles = nparts; c.n_filters = nfilters; c.dtype = dtype; c.resampler = resampler;
        c.resamp_sched = rs; c.seed = seed; c.device = device; c.first_filter_id = first_id;
        c.n_filters_total = bank_filters > nfilters ? bank_filters : 0;
        ssme_pf_handle raw = nullptr;
        check(ssme_pf_create(&c, &raw));
        h_ = std::shared_ptr<ssme_pf_s>(raw, [](ssme_pf_handle p) { if (p) ssme_pf_destroy(p); });
    }
    ssme_pf_handle get() const { return h_.get(); }
    explicit operator bool() const { return (bool)h_; }
private:
    std::shared_ptr<ssme_pf_s> h_;   // copy-assignable like the reference's models; copies share device state
};

struct gpu_options {
    std::uint64_t seed = 0;          // the reference seeds from the clock; here the stream is reproducible
    int resampler = SSME_RESAMP_MULTINOMIAL;
    int resamp_sched = 1;
    int device = 0;
    bool probe_functionals = false;  // opt-in: classify undeclared functionals by six probe evaluations (see the header comment)
    std::vector<int> declared_functionals;   // [j] = SSME_H_* : fs[j] of every filter() call IS that device functional; -1 / absent = host
    int bank_filters = 0;            // size of the whole bank of filters this model object belongs to (swarm members, replicates):
                                     // the default tile size follows the bank (ssme_pf_config::n_filters_total), so a member gives
                                     // the same bits in its own handle as inside a batched handle.  0 = this handle alone
};

// Filter id of a model object constructed without one: a process-wide counter, so that every object has its own random
// stream under one seed (the reference seeds every sampler of every model object from the clock, liu_west_filter.h:75-76).
constexpr unsigned auto_filter_id = 0xffffffffu;
namespace detail {
struct no_base {};
// float_t = float (the shipped example, example/main.cpp:13) -> SSME_F32: float at the boundary (ssme_pf.h)
template <typename float_t> constexpr int dtype_of() { return sizeof(float_t) == sizeof(float) ? SSME_F32 : SSME_F64; }
inline unsigned resolve_filter_id(unsigned id) {
    static std::atomic<unsigned> next{0};
    return id == auto_filter_id ? next.fetch_add(1) : id;
}
template <typename T>
class small_matrix {                                  // the least a dynamic matrix must offer here
public:
    small_matrix() = default;
    small_matrix(long r, long c) : r_(r), c_(c), v_((std::size_t)(r * c), T(0)) {}
    long rows() const { return r_; }
    long cols() const { return c_; }
    T& operator()(long i, long j) { return v_[(std::size_t)(i * c_ + j)]; }
    const T& operator()(long i, long j) const { return v_[(std::size_t)(i * c_ + j)]; }
private:
    long r_ = 0, c_ = 0;
    std::vector<T> v_;
};
// ---- expectations of host-side functionals: the pieces every model class shares ---------------------------------
// sum_i v(i) w[i] / sum_i w[i], entry by entry (twin liu_west_filter.h:1662-1683).  v(i): the value of particle i, anything
// with rows(), cols(), (r, c); the shape is that of particle 0.  One double accumulator per entry, particles in ascending
// order, the weight sum in the same loop, one division at the end: the order of the roundings is part of the contract
// (a member gives the same bits in its own handle, in a swarm_context and through every class of this header).
template <typename float_t, typename Out, typename V>
Out weighted_mean(std::size_t n, const std::vector<double>& w, const V& v) {
    std::vector<double> acc;
    long rows = 0, cols = 0;
    double wsum = 0.0;
    for (std::size_t i = 0; i < n; ++i) {
        const auto& hv = v(i);
        if (i == 0) { rows = (long)hv.rows(); cols = (long)hv.cols(); acc.assign((std::size_t)(rows * cols), 0.0); }
        for (long r = 0; r < rows; ++r)
            for (long c = 0; c < cols; ++c) acc[(std::size_t)(r * cols + c)] += (double)hv(r, c) * w[i];
        wsum += w[i];
    }
    Out m(rows, cols);
    for (long r = 0; r < rows; ++r)
        for (long c = 0; c < cols; ++c) m(r, c) = (float_t)(acc[(std::size_t)(r * cols + c)] / wsum);
    return m;
}
// E[f_k], k < n_fs, of SCALAR-valued functions of a vector state (the user-model classes): eval(k, x_i) = f_k at particle i,
// x[d * n + i] as ssme_pf_download_weights fills it.  The n_fs values of one particle are one 1 x n_fs value of weighted_mean,
// so the functions are called particle by particle, k ascending within a particle.
template <std::size_t dimx, typename Eval>
std::vector<double> state_means(std::size_t n, const std::vector<double>& x, const std::vector<double>& w, std::size_t n_fs, const Eval& eval) {
    small_matrix<double> hv(1, (long)n_fs);
    const small_matrix<double> m = weighted_mean<double, small_matrix<double>>(n, w, [&](std::size_t i) -> const small_matrix<double>& {
        std::array<double, dimx> xi;
        for (std::size_t d = 0; d < dimx; ++d) xi[d] = x[d * n + i];
        for (std::size_t k = 0; k < n_fs; ++k) hv(0, (long)k) = eval(k, xi);
        return hv;
    });
    std::vector<double> e(n_fs);
    for (std::size_t k = 0; k < n_fs; ++k) e[k] = m(0, (long)k);
    return e;
}
// Which built-in functional reproduces h?  Probed at six states (and six parameter vectors); exact agreement required
// (exp(x/2): 4 ulp).  eval(x, p) = h at state x and parameters p[0..3], a matrix; n_par = how many parameter columns h can
// see (0: the bootstrap members, 4: Liu-West).  Returns SSME_H_* or 4 + d for parameter d (and the factor to apply to the
// device value), or -1 = evaluate on the host.  Precedence: constant, x, x^2, exp(x/2), then the parameters in order.
template <typename float_t, typename Eval>
int classify(const Eval& eval, int n_par, double* scale) {
    static const double px[6] = {-1.7, -0.3125, 0.0, 0.5625, 1.9, 3.25};
    static const double pp[6][4] = {{0.91, -0.07, 0.021, -0.31}, {0.83, 0.02, 0.034, -0.12}, {0.95, 0.09, 0.077, -0.45},
                                    {0.88, -0.03, 0.055, -0.02}, {0.97, 0.05, 0.012, -0.27}, {0.81, -0.09, 0.093, -0.38}};
    bool is_const = true, is_x = true, is_x2 = true, is_vol = true, is_p[4] = {true, true, true, true};
    float_t c0 = 0;
    for (int q = 0; q < 6; ++q) {
        const float_t xx = (float_t)px[q];
        float_t p[4];
        for (int d = 0; d < 4; ++d) p[d] = (float_t)pp[q][d];
        const auto m = eval(xx, (const float_t*)p);
        if (m.rows() != 1 || m.cols() != 1) return -1;
        const float_t v = m(0, 0);
        if (q == 0) c0 = v;
        is_const = is_const && (v == c0);
        is_x = is_x && (v == xx);
        is_x2 = is_x2 && (v == xx * xx);
        const float_t e = (float_t)std::exp((float_t)0.5 * xx);
        is_vol = is_vol && (std::fabs(v - e) <= 4 * std::numeric_limits<float_t>::epsilon() * e);
        for (int d = 0; d < n_par; ++d) is_p[d] = is_p[d] && (v == p[d]);
    }
    *scale = 1.0;
    if (is_const) { *scale = (double)c0 / 42.0; return SSME_H_CONST42; }   // E[c] = c E[42] / 42 (a NaN filter stays NaN)
    if (is_x) return SSME_H_X;
    if (is_x2) return SSME_H_X2;
    if (is_vol) return SSME_H_VOL;
    for (int d = 0; d < n_par; ++d) if (is_p[d]) return 4 + d;
    return -1;
}
// What a filter type lets run on the device: the declared ids it accepts, and how many device functionals one call takes
// (those beyond the cap are summed on the host).  Two filter types, two policies, each stated where it is used.
struct device_policy {
    int declared_lo, declared_hi;
    std::size_t cap;
};
constexpr device_policy bootstrap_policy{SSME_H_X, SSME_H_CONST42, 4};                      // ssme_pf_get_expectations_multi takes 4
constexpr device_policy liu_west_policy{0, 7, std::numeric_limits<std::size_t>::max()};     // 0-3 SSME_H_*, 4-7 phi, mu, sigma, rho; no cap
// E[h_j], j < n_funcs, after the last step, in the caller's order: a functional declared as a built-in (or, with `probe`,
// classified as one: classify_j(j, &scale)) goes to the device, all of them in ONE call device(ids); everything else is
// host(j) over ONE download(), made when the first host functional is met.  Device results are 1 x 1 matrices.
template <typename float_t, typename Mat, typename Classify, typename Device, typename Download, typename Host>
std::vector<Mat> dispatch_expectations(std::size_t n_funcs, const std::vector<int>& declared, const device_policy& pol, bool probe,
                                       const Classify& classify_j, const Device& device, const Download& download, const Host& host) {
    std::vector<Mat> out;
    if (n_funcs == 0) return out;
    std::vector<int> kind(n_funcs, -1);
    std::vector<double> scale(n_funcs, 1.0);
    std::vector<int32_t> ids;
    for (std::size_t j = 0; j < n_funcs; ++j) {
        if (j < declared.size() && declared[j] >= pol.declared_lo && declared[j] <= pol.declared_hi) kind[j] = declared[j];
        else if (probe) kind[j] = classify_j(j, &scale[j]);
        if (kind[j] >= 0 && ids.size() == pol.cap) kind[j] = -1;       // more device functionals than one call takes: the rest on the host
        if (kind[j] >= 0) ids.push_back(kind[j]);
    }
    std::vector<double> dev;
    if (!ids.empty()) dev = device(ids);
    bool downloaded = false;
    std::size_t d = 0;
    for (std::size_t j = 0; j < n_funcs; ++j) {
        if (kind[j] >= 0) {
            Mat m(1, 1);
            m(0, 0) = (float_t)(dev[d++] * scale[j]);
            out.push_back(m);
            continue;
        }
        if (!downloaded) { download(); downloaded = true; }
        out.push_back(host(j));
    }
    return out;
}
// ---- the two log-likelihood evaluators' inputs -------------------------------------------------------------------
// column 0 of `data`, any container of vectors with operator()(0)
template <typename Data>
std::vector<double> column0(const Data& data) {
    std::vector<double> y(data.size());
    for (std::size_t i = 0; i < data.size(); ++i) y[i] = (double)data[i](0);
    return y;
}
// a param::pack in the reference's order beta, phi, ss -> the C ABI's (beta, phi, sigma = sqrt(ss))
template <typename Pack>
std::array<double, 3> svol_theta(const Pack& theta) {
    return {(double)theta.get_untrans_params(0, 0)(0), (double)theta.get_untrans_params(1, 1)(0),
            std::sqrt((double)theta.get_untrans_params(2, 2)(0))};
}
}  // namespace detail

// ---- svol_bs ---------------------------------------------------------------------------------------------
template <std::size_t nparts, typename float_t = double>
class svol_bs_gpu {
public:
    using float_type = float_t;
    svol_bs_gpu(const float_t& phi, const float_t& beta, const float_t& sigma, gpu_options o = gpu_options(),
                unsigned filter_id = auto_filter_id)
        : h_(SSME_MODEL_SVOL, (int)nparts, 1, o.seed, o.resampler, o.resamp_sched, o.device, detail::resolve_filter_id(filter_id),
             detail::dtype_of<float_t>()) {
        const double th[3] = {(double)beta, (double)phi, (double)sigma};
        check(ssme_pf_set_params(h_.get(), th, 3, 1), h_.get());
    }
    // ctor from a param::pack: order beta, phi, ss (univ_svol_bootstrap_filter.h:55-61)
    template <typename Pack>
    explicit svol_bs_gpu(const Pack& pp, gpu_options o = gpu_options(), unsigned filter_id = auto_filter_id)
        : svol_bs_gpu((float_t)pp.get_untrans_params(1, 1)(0), (float_t)pp.get_untrans_params(0, 0)(0),
                      (float_t)std::sqrt((double)pp.get_untrans_params(2, 2)(0)), o, filter_id) {}

    template <typename Osv>
    void filter(const Osv& yt) {
        const double y = (double)yt(0);
        double out = 0.0;
        check(ssme_pf_step(h_.get(), &y, nullptr, &out), h_.get());
        last_ = (float_t)out;
    }
    float_t getLogCondLike() const { return last_; }
    ssme_pf_handle native() const { return h_.get(); }

private:
    handle h_;
    float_t last_ = 0;
};

// ---- a model of the user's own (ssme_amd/csrc/model_api.h: SSME_MODEL_USER0) -------------------------------------------------------
// The reference's way to a new model is a class derived from pf::filters::BSFilter<nparts, dimx, dimy, resampT, float_t> with five
// callbacks (example/univ_svol_bootstrap_filter.h:17-41); here the callbacks live in the header that was compiled into the library
// this program links (build.build_user_model), and user_bs_gpu is the caller-visible rest: filter(y), getLogCondLike(), and
// getExpectations() of ANY functions h(x) of the whole state, evaluated on the host over the downloaded particles and weights
// (liu_west_filter.h:1662-1683); functions the model's header itself declares are summed on the device: getModelExpectations().
// dimx / dimy must be the model's (checked against ssme_pf_user_model_dims).
// detail::user_core is what user_bs_gpu and user_bswc_gpu (the model with covariates) share: everything but the arity of func, the
// filter overloads and the forecast call.
namespace detail {
template <std::size_t nparts, std::size_t dimx, std::size_t dimy, typename float_t>
class user_core {
public:
    using float_type = float_t;
    using state_vector = std::array<double, dimx>;
    float_t getLogCondLike() const { return last_; }
    const std::vector<double>& getExpectations() const { return expectations_; }
    // the n_h functionals the model's header declares (model_api.h: n_h, h; with covariates h(x_t, z_t)) after the last filter(),
    // summed ON THE DEVICE: one small download instead of filter(y, fs)'s (dimx + 1) * nparts doubles.  Throws what check throws
    // (std::runtime_error) when the linked library declares none.
    std::vector<double> getModelExpectations() const {
        const int n = ssme_pf_user_model_n_h();
        if (n < 1) check(SSME_ERR_UNSUPPORTED, h_.get());
        std::vector<double> out((std::size_t)n);
        check(ssme_pf_get_user_expectations(h_.get(), out.data()), h_.get());
        return out;
    }
    ssme_pf_handle native() const { return h_.get(); }

protected:
    // who: the public class, for the messages.  dimcov: the class's covariate dimension; -1: the class without covariates
    user_core(const char* who, int dimcov, const std::vector<double>& theta, const gpu_options& o, unsigned filter_id) {
        std::int32_t dx = 0, dy = 0;
        check(ssme_pf_user_model_dims(&dx, &dy));                      // SSME_ERR_UNSUPPORTED: the stock library was linked
        if (dx != (std::int32_t)dimx || dy != (std::int32_t)dimy) throw std::invalid_argument(std::string(who) + ": dimx / dimy are not the compiled-in model's");
        if (dimcov >= 0 && ssme_pf_user_model_dim_cov() != dimcov) throw std::invalid_argument(std::string(who) + ": dimcov is not the compiled-in model's dim_cov");
        h_ = handle(SSME_MODEL_USER0, (int)nparts, 1, o.seed, o.resampler, o.resamp_sched, o.device, resolve_filter_id(filter_id));
        check(ssme_pf_set_params(h_.get(), theta.data(), (std::int32_t)theta.size(), 1), h_.get());
    }
    // one step on obs[j], j < dimy, with the step's covariates z (nullptr: none); then E[f_k], k < n_fs, on the host over one
    // download of (x, weights): eval(k, x_i) = f_k at particle i (detail::state_means)
    template <typename Osv, typename Eval>
    void step(const Osv& yt, const double* z, std::size_t n_fs, const Eval& eval) {
        double y[dimy];
        for (std::size_t j = 0; j < dimy; ++j) y[j] = (double)yt[j];
        double out = 0.0;
        check(ssme_pf_step(h_.get(), y, z, &out), h_.get());
        last_ = (float_t)out;
        expectations_.assign(n_fs, 0.0);
        if (n_fs == 0) return;
        std::vector<double> x(dimx * nparts), w(nparts);
        check(ssme_pf_download_weights(h_.get(), 0, x.data(), w.data()), h_.get());
        expectations_ = state_means<dimx>(nparts, x, w, n_fs, eval);
    }

private:
    handle h_;
    float_t last_ = 0;
    std::vector<double> expectations_;
};
}  // namespace detail

template <std::size_t nparts, std::size_t dimx = 1, std::size_t dimy = 1, typename float_t = double>
class user_bs_gpu : public detail::user_core<nparts, dimx, dimy, float_t> {
public:
    using state_vector = std::array<double, dimx>;
    using func = std::function<double(const state_vector&)>;
    explicit user_bs_gpu(const std::vector<double>& theta, gpu_options o = gpu_options(), unsigned filter_id = auto_filter_id)
        : detail::user_core<nparts, dimx, dimy, float_t>("user_bs_gpu", -1, theta, o, filter_id) {}
    // filter(obs) / filter(obs, fs): obs(j), j < dimy (an Eigen vector, a std::array, ...)
    template <typename Osv>
    void filter(const Osv& yt, const std::vector<func>& fs = std::vector<func>()) {
        this->step(yt, nullptr, fs.size(), [&fs](std::size_t k, const state_vector& xi) { return fs[k](xi); });
    }
    // sim_future_obs(num_future_steps) of the model's FutureSimulator add-on (test/test_pswarm.cpp:64-67, 112-116) after the last
    // filter(), ON THE DEVICE, for a model whose header declares its observation draw (model_api.h: gsamp / gsamp_vec):
    // y[time][component][particle], row-major (ssme_pf_sim_future_obs).  last_obs: the covariate of the first simulated step (the
    // later ones read component 0 of the previous simulated observation).  Throws what check throws (std::runtime_error) when the
    // linked library declares no draw (SSME_ERR_UNSUPPORTED of the call itself).
    std::vector<double> sim_future_obs(unsigned num_steps, double last_obs = 0.0) {
        std::vector<double> y((std::size_t)num_steps * dimy * nparts);
        check(ssme_pf_sim_future_obs(this->native(), (std::int32_t)num_steps, &last_obs, y.data(), nullptr, nullptr), this->native());
        return y;
    }
};

// ---- a model of the user's own WITH COVARIATES (model_api.h: dim_cov) ---------------------------------------------------------------
// The counterpart of pf::filters::BSFilterWC<nparts, dimx, dimy, dimcov, resampT, float_t> (pswarm_filter.h:309-352): the header
// compiled into the linked library declares dim_cov = dimcov, and z_t reaches fSamp, logGEv, the first step (q1Samp, logMuEv, logQ1Ev,
// when the header declares first / first_logw), gSamp and the functionals.  filter(y_t, z_t, fs): fs are functions h(x_t, z_t) of the
// whole state and the step's covariates, evaluated on the host over the downloaded particles and weights as user_bs_gpu does;
// functions the header declares are summed on the device: getModelExpectations().  dimx / dimy / dimcov must be the model's.
template <std::size_t nparts, std::size_t dimx, std::size_t dimy, std::size_t dimcov, typename float_t = double>
class user_bswc_gpu : public detail::user_core<nparts, dimx, dimy, float_t> {
public:
    using state_vector = std::array<double, dimx>;
    using cov_vector = std::array<double, dimcov>;
    using func = std::function<double(const state_vector&, const cov_vector&)>;
    explicit user_bswc_gpu(const std::vector<double>& theta, gpu_options o = gpu_options(), unsigned filter_id = auto_filter_id)
        : detail::user_core<nparts, dimx, dimy, float_t>("user_bswc_gpu", (int)dimcov, theta, o, filter_id) {}
    // filter(obs, cov) / filter(obs, cov, fs): obs[j], j < dimy; cov[j], j < dimcov (an Eigen vector, a std::array, ...)
    template <typename Osv, typename Csv>
    void filter(const Osv& yt, const Csv& zt, const std::vector<func>& fs = std::vector<func>()) {
        cov_vector z;
        for (std::size_t j = 0; j < dimcov; ++j) z[j] = (double)zt[j];
        this->step(yt, z.data(), fs.size(), [&fs, &z](std::size_t k, const state_vector& xi) { return fs[k](xi, z); });
    }
    // sim_future_obs with the exogenous covariates of the horizons, future_covs[k * dimcov + j] (ssme_pf_sim_future_obs_cov):
    // y[time][component][particle], row-major.  Throws std::invalid_argument when future_covs is not num_steps * dimcov long.
    std::vector<double> sim_future_obs(unsigned num_steps, const std::vector<double>& future_covs) {
        if (future_covs.size() != (std::size_t)num_steps * dimcov) throw std::invalid_argument("user_bswc_gpu::sim_future_obs: num_steps * dimcov covariates");
        std::vector<double> y((std::size_t)num_steps * dimy * nparts);
        check(ssme_pf_sim_future_obs_cov(this->native(), (std::int32_t)num_steps, future_covs.data(), y.data(), nullptr, nullptr), this->native());
        return y;
    }
};

// ---- swarm_context: ONE launch per observation behind the UNMODIFIED Swarm / SwarmWithCovs templates ----------------------
// The reference's swarm calls filter(y_t[, z_t], fs) -> getExpectations() -> getLogCondLike() on every member, from the
// workers of split_data_thread_pool (pswarm_filter.h:86-92,380-388; thread_pool.h:542-554).  A member with its own handle
// costs one launch and one wait per call: 512 members x 18 us = 9 ms per observation where the batched step takes 0.1 ms.
// A swarm_context is the members' shared device state: created once by the user's swarm class, handed to every model its
// instantiate_mod() constructs (member i = filter i of ONE C-ABI handle, theta row i).  The FIRST member whose filter() call
// arrives for a new observation advances ALL members (one ssme_pf_step, one ssme_pf_get_expectations_multi for the declared
// device functionals); every other member's call for that observation checks that it was given the same (y_t, z_t) and
// reads its cached row.  Calls are serialised by a mutex, so the reference's concurrent workers are safe; a member may lag
// the context by at most the observation in flight (the swarm finishes one update before it starts the next).
// Results are those of one handle per member, to the bit (same filter ids, same theta, same tile: the tile follows the bank).
template <typename float_t = double>
class swarm_context {
public:
    // model: SSME_MODEL_SVOL_LEVERAGE (SwarmWithCovs members) or SSME_MODEL_SVOL (Swarm members); n_members = nparamparts
    swarm_context(int model, std::size_t nparts, std::size_t n_members, gpu_options o = gpu_options())
        : model_(model), nparts_(nparts), n_members_(n_members), opt_(o), n_theta_(model == SSME_MODEL_SVOL_LEVERAGE ? 4 : 3) {
        if (n_members == 0) throw std::invalid_argument("a swarm needs members");
        for (std::size_t j = 0; j < o.declared_functionals.size(); ++j) {
            const int id = o.declared_functionals[j];
            if (id >= SSME_H_X && id <= SSME_H_CONST42) { slot_of_func_.push_back((int)ids_.size()); ids_.push_back(id); }
            else slot_of_func_.push_back(-1);
        }
        if (ids_.size() > 4) throw std::invalid_argument("at most 4 device functionals per swarm");
        theta_.reserve(n_members * (std::size_t)n_theta_);
    }
    // called by a member model's constructor; theta in the C ABI's order for the model.  Returns the member's index.
    unsigned add_member(const double* theta) {
        std::lock_guard<std::mutex> lk(mu_);
        if (h_) throw std::runtime_error("swarm_context: members cannot be added after the first filter() call");
        if (theta_.size() / (std::size_t)n_theta_ >= n_members_) throw std::runtime_error("swarm_context: more members than declared");
        theta_.insert(theta_.end(), theta, theta + n_theta_);
        return (unsigned)(theta_.size() / (std::size_t)n_theta_ - 1);
    }
    // member `i`, which has seen `member_steps` observations so far, is given (y, z); z = nullptr: no covariate
    void filter(unsigned i, unsigned long member_steps, double y, const double* z) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!h_) start();
        if (i >= n_members_) throw std::invalid_argument("swarm_context: no such member");
        if (member_steps == steps_) {                                   // first arrival for this observation: everybody moves
            check(ssme_pf_step(h_.get(), &y, z, lcl_.data()), h_.get());
            if (!ids_.empty()) check(ssme_pf_get_expectations_multi(h_.get(), ids_.data(), (int32_t)ids_.size(), dev_.data()), h_.get());
            y_ = y; z_ = z ? *z : 0.0; has_z_ = z != nullptr;
            ++steps_;
        } else if (member_steps + 1 == steps_) {
            const bool same = y == y_ && has_z_ == (z != nullptr) && (!z || *z == z_);
            if (!same) throw std::invalid_argument("swarm_context: the members of one swarm must be given the same observation and covariate");
        } else throw std::runtime_error("swarm_context: a member is more than one observation behind the swarm");
    }
    double log_cond_like(unsigned i) const { std::lock_guard<std::mutex> lk(mu_); return lcl_[i]; }
    // slot of functional j among the device functionals, or -1: evaluate it on the host
    int device_slot(std::size_t j) const { return j < slot_of_func_.size() ? slot_of_func_[j] : -1; }
    double device_expectation(int slot, unsigned i) const { std::lock_guard<std::mutex> lk(mu_); return dev_[(std::size_t)slot * n_members_ + i]; }
    // particles and weights of member i after the observation it has just been given (host functionals)
    void download(unsigned i, unsigned long member_steps, std::vector<double>& x, std::vector<double>& w) const {
        std::lock_guard<std::mutex> lk(mu_);
        if (member_steps != steps_) throw std::runtime_error("swarm_context: the swarm has moved on; this member's weights are gone");
        x.resize(nparts_); w.resize(nparts_);
        check(ssme_pf_download_weights(h_.get(), (int32_t)i, x.data(), w.data()), h_.get());
    }
    // sim_future_obs(num_steps) of member i (pswarm_filter.h:247-253, 547-553 call it on every member), which has seen
    // `member_steps` observations: the first member that asks after an observation forecasts ALL members in one device call
    // (ssme_pf_sim_future_obs); the others take their slice.  A member that is behind the swarm is refused, as download() refuses it:
    // the handle's weights are those of the swarm's last observation, not the member's.  The cache key (steps, H, last_obs) is
    // complete: members and parameters cannot change after the first filter() call, and a forecast is a function of the origin alone.
    // The host copy is released once every member has taken its slice.  Returns y[time][particle] of the member;
    // last_obs = the last observation (read by the leverage model only).
    std::vector<double> sim_future_obs(unsigned i, unsigned long member_steps, unsigned num_steps, double last_obs) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!h_) throw std::runtime_error("swarm_context: sim_future_obs before the first filter() call");
        if (i >= n_members_) throw std::invalid_argument("swarm_context: no such member");
        if (member_steps != steps_) throw std::runtime_error("swarm_context: the swarm has moved on; this member cannot forecast from its own origin");
        if (fc_y_.empty() || fc_steps_ != steps_ || fc_H_ != num_steps || fc_last_ != last_obs) {
            const std::vector<double> lo(n_members_, last_obs);
            fc_y_.assign(n_members_ * (std::size_t)num_steps * nparts_, 0.0);
            fc_taken_.assign(n_members_, 0);
            const int rc = ssme_pf_sim_future_obs(h_.get(), (int32_t)num_steps, lo.data(), fc_y_.data(), nullptr, nullptr);
            if (rc != SSME_OK) fc_y_.clear();
            check(rc, h_.get());
            fc_steps_ = steps_; fc_H_ = num_steps; fc_last_ = last_obs;
        }
        const std::size_t per = (std::size_t)num_steps * nparts_;
        std::vector<double> y(fc_y_.begin() + (std::ptrdiff_t)(i * per), fc_y_.begin() + (std::ptrdiff_t)((i + 1) * per));
        fc_taken_[i] = 1;
        bool all = true;
        for (char t : fc_taken_) all = all && t;
        if (all) { fc_y_.clear(); fc_y_.shrink_to_fit(); }          // everybody is served: a later call forecasts again (the same bits)
        return y;
    }
    std::size_t nparts() const { return nparts_; }
    std::size_t members() const { return n_members_; }
    bool probe() const { return opt_.probe_functionals; }
    ssme_pf_handle native() const { return h_.get(); }

private:
    void start() {
        if (theta_.size() != n_members_ * (std::size_t)n_theta_) throw std::runtime_error("swarm_context: fewer members were constructed than declared");
        h_ = handle(model_, (int)nparts_, (int)n_members_, opt_.seed, opt_.resampler, opt_.resamp_sched, opt_.device, 0,
                    detail::dtype_of<float_t>(), opt_.bank_filters);
        check(ssme_pf_set_params(h_.get(), theta_.data(), n_theta_, (int32_t)n_members_), h_.get());
        lcl_.assign(n_members_, 0.0);
        dev_.assign(ids_.size() * n_members_, 0.0);
    }
    int model_;
    std::size_t nparts_, n_members_;
    gpu_options opt_;
    int n_theta_;
    mutable std::mutex mu_;
    handle h_;
    std::vector<double> theta_, lcl_, dev_;
    std::vector<int32_t> ids_;
    std::vector<int> slot_of_func_;
    unsigned long steps_ = 0;
    double y_ = 0.0, z_ = 0.0;
    bool has_z_ = false;
    std::vector<double> fc_y_;            // the last forecast of all members: [member][time][particle], until every member has its slice
    std::vector<char> fc_taken_;          // which members have taken theirs
    unsigned long fc_steps_ = 0;
    unsigned fc_H_ = 0;
    double fc_last_ = 0.0;
};

namespace detail {
// what the two member model types share: their own handle, or a slot in a swarm_context
template <std::size_t nparts, typename float_t, typename Mat, typename Ssv>
class member_core {
public:
    member_core() = default;
    member_core(int model, const double* theta, int n_theta, const gpu_options& o, unsigned filter_id)
        : h_(model, (int)nparts, 1, o.seed, o.resampler, o.resamp_sched, o.device, resolve_filter_id(filter_id), dtype_of<float_t>(),
             o.bank_filters),
          probe_(o.probe_functionals), declared_(o.declared_functionals) {
        check(ssme_pf_set_params(h_.get(), theta, n_theta, 1), h_.get());
    }
    member_core(const std::shared_ptr<swarm_context<float_t>>& ctx, const double* theta) : ctx_(ctx) {
        if (!ctx) throw std::invalid_argument("null swarm_context");
        if (ctx->nparts() != nparts) throw std::invalid_argument("swarm_context was made for another particle count");
        idx_ = ctx->add_member(theta);
        probe_ = ctx->probe();
    }
    // hs: the functionals with the covariate (if any) already bound.  In a swarm_context the device slots are the context's
    // (declared once for all members); a member of its own goes through dispatch_expectations.  Host sums are the same function.
    template <typename H>
    void step(double y, const double* z, const std::vector<H>& hs) {
        std::vector<double> x, w;
        // sum_i h(x_i) w_i / sum_i w_i, any matrix shape; the state is cast to float_t before h sees it
        const auto host_mean = [&x, &w](const H& h) {
            return weighted_mean<float_t, Mat>(x.size(), w, [&h, &x](std::size_t i) { Ssv xv; xv(0) = (float_t)x[i]; return h(xv); });
        };
        if (ctx_) {
            ctx_->filter(idx_, steps_, y, z);
            ++steps_;
            last_ = (float_t)ctx_->log_cond_like(idx_);
            expectations_.clear();
            for (std::size_t j = 0; j < hs.size(); ++j) {
                int slot = ctx_->device_slot(j);
                if (slot >= 0) {
                    Mat m(1, 1);
                    m(0, 0) = (float_t)ctx_->device_expectation(slot, idx_);
                    expectations_.push_back(m);
                    continue;
                }
                if (w.empty()) ctx_->download(idx_, steps_, x, w);
                expectations_.push_back(host_mean(hs[j]));
            }
            return;
        }
        if (!h_) throw std::runtime_error("model not constructed");
        double out = 0.0;
        check(ssme_pf_step(h_.get(), &y, z, &out), h_.get());
        last_ = (float_t)out;
        const ssme_pf_handle hd = h_.get();
        expectations_ = dispatch_expectations<float_t, Mat>(
            hs.size(), declared_, bootstrap_policy, probe_,
            [&hs](std::size_t j, double* scale) {
                return classify<float_t>([&hs, j](float_t xx, const float_t*) { Ssv xv; xv(0) = xx; return hs[j](xv); }, 0, scale);
            },
            [hd](const std::vector<int32_t>& ids) {
                std::vector<double> dev(ids.size());
                check(ssme_pf_get_expectations_multi(hd, ids.data(), (int32_t)ids.size(), dev.data()), hd);
                return dev;
            },
            [hd, &x, &w] { x.resize(nparts); w.resize(nparts); check(ssme_pf_download_weights(hd, 0, x.data(), w.data()), hd); },
            [&hs, &host_mean](std::size_t j) { return host_mean(hs[j]); });
    }
    // y[time][particle] of this member (ssme_pf_sim_future_obs; in a swarm_context one device call serves all members)
    std::vector<double> sim_future_obs(unsigned num_steps, double last_obs) {
        if (ctx_) return ctx_->sim_future_obs(idx_, steps_, num_steps, last_obs);
        if (!h_) throw std::runtime_error("model not constructed");
        std::vector<double> y((std::size_t)num_steps * nparts);
        check(ssme_pf_sim_future_obs(h_.get(), (int32_t)num_steps, &last_obs, y.data(), nullptr, nullptr), h_.get());
        return y;
    }
    float_t last() const { return last_; }
    const std::vector<Mat>& expectations() const { return expectations_; }
    ssme_pf_handle native() const { return ctx_ ? ctx_->native() : h_.get(); }

private:
    handle h_;
    std::shared_ptr<swarm_context<float_t>> ctx_;
    unsigned idx_ = 0;
    unsigned long steps_ = 0;
    bool probe_ = false;
    std::vector<int> declared_;
    float_t last_ = 0;
    std::vector<Mat> expectations_;
};
}  // namespace detail

// ---- svol_leverage (BSFilterWC): a ModType for the unmodified SwarmWithCovs ------------------------------------------
// Template parameters: Mat = the model's dynamic_matrix (Eigen::Matrix<float_t,-1,-1> in the reference), Osv / Ssv / Cvsv =
// observation / state / covariate vectors (Eigen::Matrix<float_t,1,1>), Base = pf::bases::pf_withcov_base<float_t,1,1,1>
// when the pf headers are present (its pure virtuals filter / getLogCondLike are overridden by the members below
// [pf-recollection: pf_base.h]); detail::no_base otherwise.  Needs of the types: Mat(rows, cols), rows(), cols(),
// operator()(i, j); vectors: default ctor, operator()(i).
template <std::size_t nparts, typename float_t, typename Mat, typename Osv, typename Ssv, typename Cvsv,
          typename Base = detail::no_base>
class svol_leverage_gpu : public Base {
public:
    using float_type = float_t;
    using dynamic_matrix = Mat;
    using func = std::function<const Mat(const Ssv&, const Cvsv&)>;     // pf_withcov_base::func; what Swarm binds (:272-275)
    using context = swarm_context<float_t>;
    svol_leverage_gpu() = default;    // Swarm default-constructs its array of models (pswarm_filter.h:71,367)
    // its own handle: one launch and one wait per filter() call
    svol_leverage_gpu(const float_t& phi, const float_t& mu, const float_t& sigma, const float_t& rho, unsigned /*dte*/ = 0,
                      gpu_options o = gpu_options(), unsigned filter_id = auto_filter_id)
        : core_(SSME_MODEL_SVOL_LEVERAGE, theta4(phi, mu, sigma, rho).data(), 4, o, filter_id) {}
    // member of a swarm_context: all members of the swarm advance in ONE launch per observation (the context decides the
    // member's filter id: its index, in construction order -- the order of the swarm's instantiate_mod calls)
    svol_leverage_gpu(const float_t& phi, const float_t& mu, const float_t& sigma, const float_t& rho,
                      const std::shared_ptr<context>& ctx)
        : core_(ctx, theta4(phi, mu, sigma, rho).data()) {}
    // BSFilterWC::filter(y_t, z_t, fs) as SwarmWithCovs::comp_func calls it (pswarm_filter.h:383)
    void filter(const Osv& yt, const Cvsv& zt, const std::vector<func>& fs = std::vector<func>()) {
        const double z = (double)zt(0);
        std::vector<std::function<const Mat(const Ssv&)>> hs;
        for (const func& f : fs) hs.push_back([&f, &zt](const Ssv& xv) { return f(xv, zt); });
        core_.step((double)yt(0), &z, hs);
    }
    float_t getLogCondLike() const { return core_.last(); }
    std::vector<Mat> getExpectations() const { return core_.expectations(); }   // E[h(x_t) | y_{1:t}], pre-resampling weights
    // sim_future_obs(num_future_steps) of the model's GenFutureSimulator add-on (test/test_pswarm.cpp:64-67, 112-116), on the
    // device: y[time][particle], row-major.  last_obs = the last observation, the covariate of the first future step.
    std::vector<double> sim_future_obs(unsigned num_future_steps, double last_obs = 0.0) { return core_.sim_future_obs(num_future_steps, last_obs); }
    ssme_pf_handle native() const { return core_.native(); }

private:
    static std::array<double, 4> theta4(float_t phi, float_t mu, float_t sigma, float_t rho) {
        return {(double)phi, (double)mu, (double)sigma, (double)rho};
    }
    detail::member_core<nparts, float_t, Mat, Ssv> core_;
};

// ---- svol_bs as a ModType for the unmodified Swarm (no covariates; pswarm_filter.h:23-320, comp_func :86-92) -----------
// Base = pf::bases::pf_base<float_t,1,1> when pf is present.  Same model as svol_bs_gpu (ctor order phi, beta, sigma).
template <std::size_t nparts, typename float_t, typename Mat, typename Osv, typename Ssv, typename Base = detail::no_base>
class svol_bs_member_gpu : public Base {
public:
    using float_type = float_t;
    using dynamic_matrix = Mat;
    using func = std::function<const Mat(const Ssv&)>;                   // pf_base::func
    using context = swarm_context<float_t>;
    svol_bs_member_gpu() = default;
    svol_bs_member_gpu(const float_t& phi, const float_t& beta, const float_t& sigma, gpu_options o = gpu_options(),
                       unsigned filter_id = auto_filter_id)
        : core_(SSME_MODEL_SVOL, theta3(phi, beta, sigma).data(), 3, o, filter_id) {}
    svol_bs_member_gpu(const float_t& phi, const float_t& beta, const float_t& sigma, const std::shared_ptr<context>& ctx)
        : core_(ctx, theta3(phi, beta, sigma).data()) {}
    void filter(const Osv& yt, const std::vector<func>& fs = std::vector<func>()) { core_.step((double)yt(0), nullptr, fs); }
    float_t getLogCondLike() const { return core_.last(); }
    std::vector<Mat> getExpectations() const { return core_.expectations(); }
    // sim_future_obs(num_future_steps): y[time][particle], row-major (ssme_pf_sim_future_obs; the model reads no last observation)
    std::vector<double> sim_future_obs(unsigned num_future_steps, double last_obs = 0.0) { return core_.sim_future_obs(num_future_steps, last_obs); }
    ssme_pf_handle native() const { return core_.native(); }

private:
    static std::array<double, 3> theta3(float_t phi, float_t beta, float_t sigma) {      // C ABI order: beta, phi, sigma
        return {(double)beta, (double)phi, (double)sigma};
    }
    detail::member_core<nparts, float_t, Mat, Ssv> core_;
};

// ---- log_like_eval with replicate batching -----------------------------------------------------------------
// example/estimate_univ_svol.h:108-131 + thread_pool's num_pfilters replicates (thread_pool.h:189-215,263-268)
// in ONE call: R filters on the device, whole series, log-mean-exp.  `data` is any container of vectors with
// operator()(0) (std::vector<Eigen::Matrix<float_t,1,1>> in the reference).
template <typename Pack, typename Data>
double log_like_eval_gpu(const Pack& theta, const Data& data, int nparts, int num_pfilters, gpu_options o = gpu_options()) {
    if (data.empty()) throw std::length_error("can't read in data\n");   // estimate_univ_svol.h:112-113
    const std::vector<double> y = detail::column0(data);
    handle h(SSME_MODEL_SVOL, nparts, num_pfilters, o.seed, o.resampler, o.resamp_sched, o.device, 0);
    check(ssme_pf_set_params(h.get(), detail::svol_theta(theta).data(), 3, 1), h.get());
    std::vector<double> ll((std::size_t)num_pfilters);
    check(ssme_pf_run_series(h.get(), y.data(), nullptr, (int)y.size(), ll.data()), h.get());
    double out = 0.0;
    check(ssme_pf_log_mean_exp(h.get(), &out), h.get());
    return out;
}

namespace detail {
// rows 0 .. T-1 of the last recorded series of a handle: [(t * n + i) * R + r] (ssme_pf_get_series_[user_]expectations)
inline std::vector<double> series_rows(ssme_pf_handle h, std::size_t T, std::size_t n, std::size_t R, bool user) {
    std::vector<double> out(T * (n ? n : 1) * R);
    check(user ? ssme_pf_get_series_user_expectations(h, out.data(), (std::int32_t)T)
               : ssme_pf_get_series_expectations(h, out.data(), (std::int32_t)T), h);
    return out;
}
// Smoothing (ssme_pf_set_series_history; ssme_pf.h): K trajectories per filter drawn from the final weights and traced back through the
// resampling ancestors, [((r * K + k) * T + t) * dimx + d], and the smoothed means of built-in functionals, [(t * ids + i) * R + r]
inline std::vector<double> sampled_trajectories(ssme_pf_handle h, std::size_t K, std::size_t T, std::size_t R, std::size_t dimx) {
    std::vector<double> out(R * K * T * dimx);
    check(ssme_pf_sample_trajectories(h, (std::int32_t)K, nullptr, out.data(), nullptr, (std::int32_t)T), h);
    return out;
}
// ... and K trajectories per filter by backward simulation over the same history (ssme_pf_sample_trajectories_backward): the same layout
inline std::vector<double> backward_trajectories(ssme_pf_handle h, std::size_t K, std::size_t T, std::size_t R, std::size_t dimx) {
    std::vector<double> out(R * K * T * dimx);
    check(ssme_pf_sample_trajectories_backward(h, (std::int32_t)K, nullptr, out.data(), nullptr, (std::int32_t)T), h);
    return out;
}
inline std::vector<double> smoothed_rows(ssme_pf_handle h, const std::vector<std::int32_t>& ids, std::size_t T, std::size_t R) {
    std::vector<double> out(T * (ids.empty() ? 1 : ids.size()) * R);
    check(ssme_pf_get_smoothed_expectations(h, ids.data(), (std::int32_t)ids.size(), out.data(), (std::int32_t)T), h);
    return out;
}
// Marginal smoothing (ssme_pf.h): om_t of replicate r, N weights (not normalised), and the smoothed means under them, [(t * ids + i) * R + r]
inline std::vector<double> smoothing_weight_row(ssme_pf_handle h, std::size_t N, std::size_t r, std::size_t t) {
    std::vector<double> w(N);
    check(ssme_pf_download_smoothing_weights(h, (std::int32_t)r, (std::int32_t)t, nullptr, w.data()), h);
    return w;
}
inline std::vector<double> marginal_rows(ssme_pf_handle h, const std::vector<std::int32_t>& ids, std::size_t T, std::size_t R) {
    std::vector<double> out(T * (ids.empty() ? 1 : ids.size()) * R);
    check(ssme_pf_get_marginal_smoothed_expectations(h, ids.data(), (std::int32_t)ids.size(), out.data(), (std::int32_t)T), h);
    return out;
}
}  // namespace detail

// ---- persistent evaluator: one handle, one captured graph, a fresh random stream per call --------------------------
// The PMMH caller evaluates log_like_eval once per MCMC iteration (ada_pmmh_mvn.h:344,363 through thread_pool::work).
// Constructing a model per evaluation (estimate_univ_svol.h:119) costs device allocations and a graph capture; this
// object keeps the handle, so an evaluation is: upload theta, new seed, replay the graph, log-mean-exp.
class svol_log_like_evaluator {
public:
    template <typename Data>
    svol_log_like_evaluator(const Data& data, int nparts, int num_pfilters, gpu_options o = gpu_options())
        : h_(SSME_MODEL_SVOL, nparts, num_pfilters, o.seed, o.resampler, o.resamp_sched, o.device, 0), ll_((std::size_t)num_pfilters),
          nparts_((std::size_t)(nparts > 0 ? nparts : 0)) {
        if (data.empty()) throw std::length_error("can't read in data\n");
        y_ = detail::column0(data);
    }
    // theta in the reference's pack order: beta, phi, ss (sigma = sqrt(ss))
    template <typename Pack>
    double operator()(const Pack& theta, std::uint64_t seed) {
        const std::array<double, 3> th = detail::svol_theta(theta);
        check(ssme_pf_set_seed(h_.get(), seed), h_.get());
        check(ssme_pf_set_params(h_.get(), th.data(), 3, 1), h_.get());
        check(ssme_pf_run_series(h_.get(), y_.data(), nullptr, (int)y_.size(), ll_.data()), h_.get());
        n_run_ = n_rec_;                                   // what THIS series recorded: series_expectations() is sized from it
        double out = 0.0;
        check(ssme_pf_log_mean_exp(h_.get(), &out), h_.get());
        return out;
    }
    float device_ms() const { float ms = 0; ssme_pf_last_elapsed_ms(h_.get(), &ms); return ms; }
    ssme_pf_handle native() const { return h_.get(); }
    // The filtered path: record E[h(x_t) | y_{1:t}] of the built-in functionals `ids` (SSME_H_*, at most 4; none: off) at every step of
    // the evaluations that follow; series_expectations() is valid after operator(): [(t * ids + i) * num_pfilters + r].  It returns the
    // rows of the LAST evaluation, with the ids that were set when it ran, whatever record_expectations was told since.
    void record_expectations(const std::vector<std::int32_t>& ids) {
        check(ssme_pf_set_series_expectations(h_.get(), ids.empty() ? nullptr : ids.data(), (std::int32_t)ids.size(), 0), h_.get());
        n_rec_ = ids.size();                               // after the check: a rejected list changes nothing
    }
    std::vector<double> series_expectations() const { return detail::series_rows(h_.get(), y_.size(), n_run_, ll_.size(), false); }
    // Smoothing: record_history(true) makes the evaluations that follow keep every step's particles and ancestors on the device
    // (ssme_pf_set_series_history).  Valid after operator(), until the next one: sample_trajectories(K)[(r * K + k) * T + t], K state
    // paths per replicate from p(x_{0:T-1} | y_{0:T-1}) -- a PMMH iteration that accepts theta picks replicate r with probability
    // proportional to exp(logliks()[r]) and takes trajectory 0 of it -- and smoothed_expectations(ids)[(t * ids + i) * num_pfilters + r].
    void record_history(bool on = true) { check(ssme_pf_set_series_history(h_.get(), on ? 1 : 0), h_.get()); }
    std::vector<double> sample_trajectories(std::size_t K) const { return detail::sampled_trajectories(h_.get(), K, y_.size(), ll_.size(), 1); }
    // sample_backward(K): the same K paths per replicate drawn by backward simulation (ssme_pf.h) -- they end at the same particles but
    // do not share ancestors, at O(K N T) density evaluations
    std::vector<double> sample_backward(std::size_t K) const { return detail::backward_trajectories(h_.get(), K, y_.size(), ll_.size(), 1); }
    std::vector<double> smoothed_expectations(const std::vector<std::int32_t>& ids) const { return detail::smoothed_rows(h_.get(), ids, y_.size(), ll_.size()); }
    // Marginal smoothing (ssme_pf.h): smoothing_weights(r, t), the N weights om_t of replicate r -- the exact law of the backward draw
    // B_t, not normalised -- and marginal_smoothed_expectations(ids)[(t * ids + i) * num_pfilters + r], the smoothed means under them:
    // no draw noise, no shared ancestors, at 3 N^2 (T - 1) density evaluations on the first call after operator()
    std::vector<double> smoothing_weights(std::size_t r, std::size_t t) const { return detail::smoothing_weight_row(h_.get(), nparts_, r, t); }
    std::vector<double> marginal_smoothed_expectations(const std::vector<std::int32_t>& ids) const { return detail::marginal_rows(h_.get(), ids, y_.size(), ll_.size()); }
    const std::vector<double>& logliks() const { return ll_; }          // the replicates' log-likelihoods of the last evaluation

private:
    handle h_;
    std::vector<double> y_, ll_;
    std::size_t nparts_ = 0;
    std::size_t n_rec_ = 0, n_run_ = 0;                    // built-in functionals set for the next evaluation / recorded by the last one
};

// The same for a model of the caller's own (the library built with a user model header, model_api.h): one handle of num_pfilters
// replicate filters of nparts particles, the whole series per evaluation through ssme_pf_run_series -- one launch per evaluation
// for a filter of at most 2048 particles, vector states included (ssme_pf_get_series_route on native() says which route).
// y: T rows of dimy values (row-major); z: T rows of dimcov covariates when dimcov > 0, empty otherwise.  Dimensions are checked
// against the compiled-in model as user_bs_gpu / user_bswc_gpu check them (std::invalid_argument); empty data is std::length_error.
template <std::size_t dimx, std::size_t dimy, std::size_t dimcov = 0>
class user_log_like_evaluator {
public:
    user_log_like_evaluator(const std::vector<double>& y, const std::vector<double>& z, int nparts, int num_pfilters,
                            gpu_options o = gpu_options())
        : y_(y), z_(z), ll_((std::size_t)(num_pfilters > 0 ? num_pfilters : 0)), nparts_((std::size_t)(nparts > 0 ? nparts : 0)) {
        std::int32_t dx = 0, dy = 0;
        check(ssme_pf_user_model_dims(&dx, &dy));                      // SSME_ERR_UNSUPPORTED: the stock library was linked
        if (dx != (std::int32_t)dimx || dy != (std::int32_t)dimy) throw std::invalid_argument("user_log_like_evaluator: dimx / dimy are not the compiled-in model's");
        if (ssme_pf_user_model_dim_cov() != (int)dimcov) throw std::invalid_argument("user_log_like_evaluator: dimcov is not the compiled-in model's dim_cov");
        if (y.empty()) throw std::length_error("can't read in data\n");
        if (y.size() % dimy != 0) throw std::invalid_argument("user_log_like_evaluator: y holds T rows of dimy values");
        T_ = y.size() / dimy;
        if (z.size() != T_ * dimcov) throw std::invalid_argument("user_log_like_evaluator: z holds T rows of dimcov values");
        h_ = handle(SSME_MODEL_USER0, nparts, num_pfilters, o.seed, o.resampler, o.resamp_sched, o.device, 0);
    }
    // theta: the model's untransformed parameters (n_theta of its header), shared by the replicates
    double operator()(const std::vector<double>& theta, std::uint64_t seed) {
        check(ssme_pf_set_seed(h_.get(), seed), h_.get());
        check(ssme_pf_set_params(h_.get(), theta.data(), (std::int32_t)theta.size(), 1), h_.get());
        check(ssme_pf_run_series(h_.get(), y_.data(), dimcov > 0 ? z_.data() : nullptr, (std::int32_t)T_, ll_.data()), h_.get());
        n_run_ = ids_.size();                              // what THIS series recorded: series_expectations() is sized from it
        double out = 0.0;
        check(ssme_pf_log_mean_exp(h_.get(), &out), h_.get());
        return out;
    }
    const std::vector<double>& logliks() const { return ll_; }          // the replicates' log-likelihoods of the last evaluation
    float device_ms() const { float ms = 0; ssme_pf_last_elapsed_ms(h_.get(), &ms); return ms; }
    ssme_pf_handle native() const { return h_.get(); }
    // The filtered path, as svol_log_like_evaluator records it: the built-in functionals `ids` (they see component 0 of the state) and /
    // or all n_h functionals of the model's header, which receive the covariates of row t.  Valid after operator():
    // series_expectations()[(t * ids + i) * num_pfilters + r], series_user_expectations()[(t * n_h + k) * num_pfilters + r]: the rows of
    // the LAST evaluation, with the ids that were set when it ran, whatever the two record calls were told since.
    void record_expectations(const std::vector<std::int32_t>& ids) { apply_recording(ids, user_); }
    void record_user_expectations(bool on = true) { apply_recording(ids_, on); }
    std::vector<double> series_expectations() const { return detail::series_rows(h_.get(), T_, n_run_, ll_.size(), false); }
    std::vector<double> series_user_expectations() const {
        return detail::series_rows(h_.get(), T_, (std::size_t)ssme_pf_user_model_n_h(), ll_.size(), true);
    }
    // Smoothing, as svol_log_like_evaluator offers it: sample_trajectories(K)[((r * K + k) * T + t) * dimx + d] (all state components),
    // smoothed_expectations(ids) of built-in functionals (component 0 of the state); the header's own functionals are not smoothed.
    void record_history(bool on = true) { check(ssme_pf_set_series_history(h_.get(), on ? 1 : 0), h_.get()); }
    std::vector<double> sample_trajectories(std::size_t K) const { return detail::sampled_trajectories(h_.get(), K, T_, ll_.size(), dimx); }
    // sample_backward(K): by backward simulation, for a header that declares its transition density (logf / logf_vec; else the call
    // throws SSME_ERR_UNSUPPORTED)
    std::vector<double> sample_backward(std::size_t K) const { return detail::backward_trajectories(h_.get(), K, T_, ll_.size(), dimx); }
    std::vector<double> smoothed_expectations(const std::vector<std::int32_t>& ids) const { return detail::smoothed_rows(h_.get(), ids, T_, ll_.size()); }
    // smoothing_weights(r, t) / marginal_smoothed_expectations(ids): marginal smoothing as svol_log_like_evaluator offers it, for a
    // header that declares its transition density (else SSME_ERR_UNSUPPORTED is thrown); the functionals see component 0 of the state
    std::vector<double> smoothing_weights(std::size_t r, std::size_t t) const { return detail::smoothing_weight_row(h_.get(), nparts_, r, t); }
    std::vector<double> marginal_smoothed_expectations(const std::vector<std::int32_t>& ids) const { return detail::marginal_rows(h_.get(), ids, T_, ll_.size()); }

private:
    void apply_recording(const std::vector<std::int32_t>& ids, bool user) {
        check(ssme_pf_set_series_expectations(h_.get(), ids.empty() ? nullptr : ids.data(), (std::int32_t)ids.size(), user ? 1 : 0), h_.get());
        const std::vector<std::int32_t> keep = ids;        // after the check: a rejected request changes nothing (ids may alias ids_)
        ids_ = keep; user_ = user;
    }
    handle h_;
    std::vector<double> y_, z_, ll_;
    std::vector<std::int32_t> ids_;                        // set for the next evaluation
    bool user_ = false;
    std::size_t nparts_ = 0;
    std::size_t T_ = 0, n_run_ = 0;                        // n_run_: built-in functionals the last evaluation recorded
};

// ---- svol_lw_1_par / svol_lw_2_par (Liu-West filters) ------------------------------------------------------------
// test/test_liu_west.cpp:22-157: ctor (delta, phi_l, phi_u, mu_l, mu_u, sig_l, sig_u, rho_l, rho_u[, dte]);
// filter(y, z[, fs]), getLogCondLike(), getExpectations() (liu_west_filter.h:971-1159).  Transforms as svol_lw_1_par passes
// them to its base: logit, null, log, twice_fisher (test_liu_west.cpp:70).
// FORM 0 = auxiliary-particle form (LWFilterWithCovs, svol_lw_1_par); 1 = SISR form (LWFilter2WithCovs::filter,
// liu_west_filter.h:2191-2343, svol_lw_2_par of test/test_liu_west.cpp:214-358).  gpu_options::resamp_sched = m_rs.
// filter(y[, fs]) without a covariate is the call of the no-covariate LWFilter / LWFilter2 (:238, :1447): the same model
// with the covariate term at zero.
// Functionals: the reference's std::function<const Mat(const ssv&, const csv&, const psv&)> (no-covariate forms:
// (const ssv&, const psv&)) with the UNTRANSFORMED parameters (:1054-1075, :2267-2290).  A functional DECLARED as a built-in
// (gpu_options::declared_functionals[j] = 0-3: SSME_H_* of the state, 4-7: phi, mu, sigma, rho) runs on the device
// (ssme_lw_get_expectations); anything else is summed on the host over one download of (x, theta, weights);
// gpu_options::probe_functionals opts into classification by six probe evaluations (see the header comment).  Mat = the caller's dynamic matrix
// (Eigen::Matrix<float_t,-1,-1> in the reference); detail::small_matrix when none is given.
namespace detail {
// argument types of the two functional signatures
template <typename F> struct lw_func_traits;
template <typename M, typename S, typename C, typename P>
struct lw_func_traits<std::function<const M(const S&, const C&, const P&)>> {
    using Mat = M; using Ssv = S; using Psv = P;
    static M call(const std::function<const M(const S&, const C&, const P&)>& f, const S& x, double z, const P& p) {
        C zv;
        zv(0) = z;
        return f(x, zv, p);
    }
};
template <typename M, typename S, typename P>
struct lw_func_traits<std::function<const M(const S&, const P&)>> {
    using Mat = M; using Ssv = S; using Psv = P;
    static M call(const std::function<const M(const S&, const P&)>& f, const S& x, double, const P& p) { return f(x, p); }
};
}  // namespace detail

template <std::size_t nparts, typename float_t = double, int FORM = 0, typename Mat = detail::small_matrix<float_t>>
class svol_lw_1_par_gpu {
public:
    using float_type = float_t;
    using dynamic_matrix = Mat;
    svol_lw_1_par_gpu(const float_t& delta, const float_t& phi_l, const float_t& phi_u, const float_t& mu_l, const float_t& mu_u,
                      const float_t& sig_l, const float_t& sig_u, const float_t& rho_l, const float_t& rho_u, unsigned /*dte*/ = 0,
                      gpu_options o = gpu_options(), unsigned filter_id = auto_filter_id)
        : probe_(o.probe_functionals), declared_(o.declared_functionals) {
        ssme_lw_config c{};
        c.n_particles = (int)nparts; c.n_filters = 1; c.seed = o.seed; c.device = o.device;
        c.first_filter_id = detail::resolve_filter_id(filter_id);
        c.form = FORM; c.resamp_sched = o.resamp_sched;
        c.delta = (double)delta;
        const int tr[4] = {2, 0, 3, 1};
        const double lo[4] = {(double)phi_l, (double)mu_l, (double)sig_l, (double)rho_l};
        const double hi[4] = {(double)phi_u, (double)mu_u, (double)sig_u, (double)rho_u};
        for (int d = 0; d < 4; ++d) { c.transforms[d] = tr[d]; c.prior_lo[d] = lo[d]; c.prior_hi[d] = hi[d]; }
        ssme_lw_handle raw = nullptr;
        check(ssme_lw_create(&c, &raw));
        h_ = std::shared_ptr<ssme_lw_s>(raw, [](ssme_lw_handle p) { if (p) ssme_lw_destroy(p); });
    }
    // LWFilterWithCovs::filter(obs, cov) / LWFilter2WithCovs::filter (:840, :2050)
    template <typename Osv, typename Cvsv>
    void filter(const Osv& yt, const Cvsv& zt) { step((double)yt(0), (double)zt(0)); expectations_.clear(); }
    // ... with functionals
    template <typename Osv, typename Cvsv, typename F>
    void filter(const Osv& yt, const Cvsv& zt, const std::vector<F>& fs) {
        step((double)yt(0), (double)zt(0));
        compute_expectations(fs, (double)zt(0));
    }
    // LWFilter::filter(data[, fs]) / LWFilter2::filter (:238, :1447): no covariate
    template <typename Osv>
    void filter(const Osv& yt) { step((double)yt(0), 0.0); expectations_.clear(); }
    template <typename Osv, typename F>
    void filter(const Osv& yt, const std::vector<F>& fs) {
        step((double)yt(0), 0.0);
        compute_expectations(fs, 0.0);
    }
    float_t getLogCondLike() const { return last_; }
    // the reference's getExpectations(): one matrix per functional of the last filter() call (:1177-1180)
    std::vector<Mat> getExpectations() const { return expectations_; }
    // weighted posterior means of (phi, mu, sigma, rho) under the last step's weights
    std::vector<double> getParamMeans() const {
        std::vector<double> m(4);
        check(ssme_lw_get_param_means(h_.get(), m.data()));
        return m;
    }
    // built-in functionals by id: 0-3 = SSME_H_* of the state, 4-7 = phi, mu, sigma, rho
    std::vector<double> getExpectations(const std::vector<int32_t>& ids) const {
        std::vector<double> e(ids.size());
        if (!ids.empty()) check(ssme_lw_get_expectations(h_.get(), ids.data(), (int32_t)ids.size(), e.data()));
        return e;
    }
    // sim_future_obs(num_future_steps) of the *FutureSimulator add-ons (liu_west_filter.h:1315-1363), on the device
    // (ssme_lw_sim_future_obs): y[time][particle], row-major.  last_obs = the last observation.
    std::vector<double> sim_future_obs(unsigned num_future_steps, double last_obs) {
        std::vector<double> y((std::size_t)num_future_steps * nparts);
        lw_check(ssme_lw_sim_future_obs(h_.get(), (int32_t)num_future_steps, &last_obs, y.data(), nullptr, nullptr, nullptr));
        return y;
    }
    ssme_lw_handle native() const { return h_.get(); }

private:
    // the Liu-West calls' error: the status text and, always, what the handle recorded
    void lw_check(int rc) const {
        if (rc != SSME_OK) throw std::runtime_error(std::string(ssme_pf_strerror(rc)) + " (" + ssme_lw_last_error(h_.get()) + ")");
    }
    void step(double y, double z) {
        double out = 0.0;
        lw_check(ssme_lw_step(h_.get(), &y, &z, &out));
        last_ = (float_t)out;
    }
    // declared / probed built-ins (0-3 of the state, 4-7 the parameters) on the device through getExpectations(ids), everything
    // else summed on the host over one download of (x, untransformed theta, weights): detail::dispatch_expectations
    template <typename F>
    void compute_expectations(const std::vector<F>& fs, double z) {
        using T = detail::lw_func_traits<F>;
        // f at state xx and parameters p[0..3], both already float_t
        const auto at = [z](const F& f, float_t xx, const float_t* p) -> Mat {
            typename T::Ssv xv; typename T::Psv pv;
            xv(0) = xx;
            for (int d = 0; d < 4; ++d) pv(d) = p[d];
            return T::call(f, xv, z, pv);
        };
        std::vector<double> x, th, w;
        expectations_ = detail::dispatch_expectations<float_t, Mat>(
            fs.size(), declared_, detail::liu_west_policy, probe_,
            [&fs, &at](std::size_t j, double* scale) {
                return detail::classify<float_t>([&fs, &at, j](float_t xx, const float_t* p) { return at(fs[j], xx, p); }, 4, scale);
            },
            [this](const std::vector<int32_t>& ids) { return getExpectations(ids); },
            [this, &x, &th, &w] {
                x.resize(nparts); th.resize(4 * nparts); w.resize(nparts);
                lw_check(ssme_lw_download_weights(h_.get(), 0, x.data(), th.data(), w.data()));
            },
            [&fs, &at, &x, &th, &w](std::size_t j) {
                return detail::weighted_mean<float_t, Mat>(nparts, w, [&fs, &at, &x, &th, j](std::size_t i) {
                    float_t p[4];
                    for (int q = 0; q < 4; ++q) p[q] = (float_t)th[(std::size_t)q * nparts + i];
                    return at(fs[j], (float_t)x[i], p);
                });
            });
    }

    std::shared_ptr<ssme_lw_s> h_;
    float_t last_ = 0;
    bool probe_ = false;
    std::vector<int> declared_;
    std::vector<Mat> expectations_;
};

template <std::size_t nparts, typename float_t = double, typename Mat = detail::small_matrix<float_t>>
using svol_lw_2_par_gpu = svol_lw_1_par_gpu<nparts, float_t, 1, Mat>;

// ---- the batched swarms: all nparamparts member filters in ONE handle --------------------------------------------------
// (n_filters = nparamparts, one theta row each): an update is one launch; the swarm's log conditional likelihood and
// expectations are the plain averages over the members, as the reference's intra/inter_agg_func compute them
// (pswarm_filter.h:392-460).  samp_untrans_params() is the reference's pure virtual.  detail::swarm_impl is everything the
// two public classes share; they add the model, the order of its parameters and the signature of update().
namespace detail {
template <std::size_t n_state_parts, std::size_t n_param_parts, typename float_t>
class swarm_impl {
public:
    using float_type = float_t;
    using func = int;                                            // SSME_H_* functional id
    virtual ~swarm_impl() = default;
    virtual std::vector<float_t> samp_untrans_params() = 0;      // in the order the public class states
    float_t getLogCondLike() const { return log_cond_like_; }
    std::vector<double> getExpectations() const { return expectations_; }
    // Swarm / SwarmWithCovs::simFutureObs (pswarm_filter.h:247-253, 547-553): sim_future_obs of every member, here ONE device call
    // for all of them.  Returns y[member][time][particle], row-major ("param, time, then state particle", :49-50).
    // last_obs = the last observation (read by the leverage model only).
    std::vector<double> simFutureObs(unsigned num_future_steps, double last_obs = 0.0) {
        if (!h_) finish_construction();
        const std::vector<double> lo(n_param_parts, last_obs);
        std::vector<double> y(n_param_parts * (std::size_t)num_future_steps * n_state_parts);
        check(ssme_pf_sim_future_obs(h_.get(), (int32_t)num_future_steps, lo.data(), y.data(), nullptr, nullptr), h_.get());
        return y;
    }
    ssme_pf_handle native() const { return h_.get(); }                  // the one handle of all members (null before the first update)

protected:
    // order[d] = which entry of samp_untrans_params() is parameter d of the C ABI; what = the message for a vector of another length
    swarm_impl(int model, std::vector<int> order, const char* what, const std::vector<func>& fs, const gpu_options& o)
        : model_(model), order_(std::move(order)), what_(what), fs_(fs), opt_(o) {}
    void step(double y, const double* z) {                        // z = nullptr: no covariate
        if (!h_) finish_construction();
        check(ssme_pf_step(h_.get(), &y, z, nullptr), h_.get());
        aggregate();
    }
    std::vector<double> theta_;                                   // [n_param_parts][order.size()], C ABI order

private:
    // intra/inter_agg_func (pswarm_filter.h:96-160): plain means over the members, reduced on the device, one download
    void aggregate() {
        if (fs_.size() > 4) throw std::invalid_argument("at most 4 device functionals per swarm");
        std::vector<int32_t> ids(fs_.begin(), fs_.end());
        double lcl = 0.0;
        expectations_.assign(fs_.size(), 0.0);
        check(ssme_pf_swarm_aggregate(h_.get(), ids.data(), (int32_t)ids.size(), &lcl, expectations_.data()), h_.get());
        log_cond_like_ = (float_t)lcl;
    }
    void finish_construction() {                                  // pswarm_filter.h:280-304
        const std::size_t n_theta = order_.size();
        theta_.resize(n_param_parts * n_theta);
        for (std::size_t i = 0; i < n_param_parts; ++i) {
            const std::vector<float_t> p = samp_untrans_params();
            if (p.size() != n_theta) throw std::invalid_argument(what_);
            for (std::size_t d = 0; d < n_theta; ++d) theta_[i * n_theta + d] = (double)p[(std::size_t)order_[d]];
        }
        h_ = handle(model_, (int)n_state_parts, (int)n_param_parts, opt_.seed, opt_.resampler, opt_.resamp_sched, opt_.device, 0,
                    dtype_of<float_t>());
        check(ssme_pf_set_params(h_.get(), theta_.data(), (int)n_theta, (int)n_param_parts), h_.get());
    }
    int model_;
    std::vector<int> order_;
    const char* what_;
    std::vector<func> fs_;
    gpu_options opt_;
    handle h_;
    std::vector<double> expectations_;
    float_t log_cond_like_ = 0;
};
}  // namespace detail

// SwarmWithCovs over SVOL-leverage members (include/ssme/pswarm_filter.h:325-560; test/test_pswarm.cpp:146-208):
// samp_untrans_params() returns (phi, mu, sigma, rho), the C ABI's own order.
template <std::size_t n_state_parts, std::size_t n_param_parts, typename float_t = double>
class swarm_with_covs_gpu : public detail::swarm_impl<n_state_parts, n_param_parts, float_t> {
public:
    explicit swarm_with_covs_gpu(const std::vector<int>& fs, gpu_options o = gpu_options())
        : detail::swarm_impl<n_state_parts, n_param_parts, float_t>(SSME_MODEL_SVOL_LEVERAGE, {0, 1, 2, 3},
                                                                     "samp_untrans_params must return phi, mu, sigma, rho", fs, o) {}
    template <typename Osv, typename Csv>
    void update(const Osv& yt, const Csv& zt) {
        const double z = (double)zt(0);
        this->step((double)yt(0), &z);
    }
    const std::vector<double>& params() const { return this->theta_; }   // [n_param_parts][4]
};

// Swarm over univariate-SVOL members (include/ssme/pswarm_filter.h:23-320: the variant without covariates): update(y) =
// filter(y, fs) on every member; parameters in the model's ctor order of svol_bs: samp_untrans_params() returns
// (phi, beta, sigma) (univ_svol_bootstrap_filter.h:34), the C ABI takes (beta, phi, sigma).
template <std::size_t n_state_parts, std::size_t n_param_parts, typename float_t = double>
class swarm_gpu : public detail::swarm_impl<n_state_parts, n_param_parts, float_t> {
public:
    explicit swarm_gpu(const std::vector<int>& fs, gpu_options o = gpu_options())
        : detail::swarm_impl<n_state_parts, n_param_parts, float_t>(SSME_MODEL_SVOL, {1, 0, 2},
                                                                     "samp_untrans_params must return phi, beta, sigma", fs, o) {}
    template <typename Osv>
    void update(const Osv& yt) { this->step((double)yt(0), nullptr); }
};

// ---- headerless CSV -> rows of doubles (utils::read_data, include/ssme/utils.h:25-64) -------------------------------
// Same tolerance as the reference: rows that fail to parse are skipped; an unreadable file yields an empty vector
// (callers then throw length_error, estimate_univ_svol.h:112-113).
struct csv_row {
    std::vector<double> v;
    double operator()(std::size_t i) const { return v[i]; }
};
inline std::vector<csv_row> read_data(const std::string& file_loc, std::size_t ncols = 1) {
    std::vector<csv_row> rows;
    std::ifstream in(file_loc);
    std::string line, cell;
    while (std::getline(in, line)) {
        csv_row r;
        std::istringstream ls(line);
        bool ok = true;
        while (ok && std::getline(ls, cell, ',')) {
            try { r.v.push_back(std::stod(cell)); } catch (const std::exception&) { ok = false; }
        }
        if (ok && r.v.size() >= ncols) { r.v.resize(ncols); rows.push_back(r); }
    }
    return rows;
}

}  // namespace ssme_gpu
#endif
