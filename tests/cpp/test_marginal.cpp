// The marginal smoothing methods of the evaluators (include/ssme_gpu/bsfilter_gpu.hpp: smoothing_weights,
// marginal_smoothed_expectations) against the C ABI's bits: a handle of the same configuration made and driven through ssme_pf.h alone.
//   test_marginal spy_returns.csv        prints one "<name> ok" line per comparison (or "<name> DIFFERS")
// Driven by tests/test_cpp_marginal.py.  Compiled against the stock library; the user-model evaluator's methods are instantiated
// (they compile) and not run: its constructor refuses a library without a user model.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"
#include "swarm_shape.hpp"

using vec1 = shape::vec1<double>;
struct pack3 { double p[3]; vec1 get_untrans_params(unsigned a, unsigned) const { return vec1{p[a]}; } };   // stand-in for the reference's param::pack

static void report(const char* name, bool same) { std::printf("%s %s\n", name, same ? "ok" : "DIFFERS"); }
template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// never called with the stock library: shows that the methods of the user-model evaluator compile
static double user_evaluator_marginal(const std::vector<double>& y) {
    ssme_gpu::user_log_like_evaluator<2, 2> ev(y, {}, 100, 2);
    ev.record_history();
    ev({1.0, 0.9, 0.8, 0.2, 0.2, 0.1}, 1);
    return ev.smoothing_weights(0, 0)[0] + ev.marginal_smoothed_expectations({SSME_H_X})[0];
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (argc > 2) { std::printf("%g\n", user_evaluator_marginal({0.1, 0.2, 0.3, 0.4})); return 0; }
    const int N = 500, R = 3, T = 12;
    std::vector<vec1> data;
    std::vector<double> y;
    std::ifstream f(argv[1]);
    double v;
    while (f >> v && (int)data.size() < T) { data.push_back(vec1{v}); y.push_back(v); }
    if ((int)data.size() != T) return 3;
    ssme_gpu::gpu_options o;
    o.seed = 5;
    const pack3 theta{{1.0, 0.95, 0.0625}};              // beta, phi, ss (sigma = sqrt(ss) = 0.25)
    const std::vector<std::int32_t> ids = {SSME_H_X, SSME_H_VOL};

    ssme_gpu::svol_log_like_evaluator ev(data, N, R, o);
    ev.record_history();
    ev(theta, 77);
    const std::vector<double> means = ev.marginal_smoothed_expectations(ids);
    const std::vector<double> w0 = ev.smoothing_weights(1, 0), wl = ev.smoothing_weights(2, T - 1);

    // the same through the C ABI alone
    ssme_pf_config c{};
    c.model = SSME_MODEL_SVOL; c.n_particles = N; c.n_filters = R; c.dtype = SSME_F64; c.resampler = o.resampler; c.resamp_sched = o.resamp_sched;
    c.seed = o.seed; c.device = o.device;
    ssme_pf_handle h = nullptr;
    if (ssme_pf_create(&c, &h) != SSME_OK) return 4;
    const double th[3] = {1.0, 0.95, 0.25};
    std::vector<double> ll(R), means_c((size_t)T * ids.size() * R), w0_c(N), wl_c(N), x0(N), wfin(N);
    int rc = ssme_pf_set_series_history(h, 1);
    rc |= ssme_pf_set_seed(h, 77);
    rc |= ssme_pf_set_params(h, th, 3, 1);
    rc |= ssme_pf_run_series(h, y.data(), nullptr, T, ll.data());
    rc |= ssme_pf_get_marginal_smoothed_expectations(h, ids.data(), (std::int32_t)ids.size(), means_c.data(), T);
    rc |= ssme_pf_download_smoothing_weights(h, 1, 0, x0.data(), w0_c.data());
    rc |= ssme_pf_download_smoothing_weights(h, 2, T - 1, nullptr, wl_c.data());
    rc |= ssme_pf_download_weights(h, 2, nullptr, wfin.data());
    if (rc != SSME_OK) { std::printf("C ABI status %d: %s\n", rc, ssme_pf_last_error(h)); return 5; }
    report("logliks", same_bits(ev.logliks(), ll));
    report("means", same_bits(means, means_c));
    report("weights_first_step", same_bits(w0, w0_c));
    report("weights_last_step", same_bits(wl, wl_c));
    report("last_row_is_final_weights", same_bits(wl, wfin));
    bool spread = false;                                   // the weights of step 0 are not all alike
    for (int i = 1; i < N; ++i) spread = spread || w0[i] != w0[0];
    report("first_row_has_spread", spread);
    // a second evaluation discards the rows of the first and fills its own; switched off, the getters refuse
    ev(theta, 78);
    report("second_evaluation_differs", !same_bits(ev.marginal_smoothed_expectations(ids), means));
    ev.record_history(false);
    ev(theta, 77);
    bool refused = false;
    try { ev.smoothing_weights(0, 0); } catch (const std::exception&) { refused = true; }
    report("off_refuses", refused);
    ssme_pf_destroy(h);
    return 0;
}
