// The host half of the adaptor's functionals, without a device: the probe classifier, the weighted mean and the
// declared / probe / device / host dispatch of include/ssme_gpu/bsfilter_gpu.hpp (namespace detail), called directly on small
// hand-made inputs.  Every expected value follows by hand from the definitions (dyadic inputs), so every comparison is exact.
// Exit status: 0 when every check passed, 1 otherwise; each failure is printed.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"

namespace d = ssme_gpu::detail;
using Mat = d::small_matrix<double>;
using MatF = d::small_matrix<float>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

template <typename T>
static d::small_matrix<T> one(T v) { d::small_matrix<T> m(1, 1); m(0, 0) = v; return m; }

// classify an h of the state alone, as the bootstrap members do (no parameter columns)
template <typename float_t, typename H>
static std::pair<int, double> kind0(const H& h) {
    double scale = -1.0;
    const int k = d::classify<float_t>([&h](float_t x, const float_t*) { return h(x); }, 0, &scale);
    return {k, scale};
}
// ... and of the state and four parameters, as the Liu-West filters do
template <typename H>
static std::pair<int, double> kind4(const H& h, int n_par = 4) {
    double scale = -1.0;
    const int k = d::classify<double>([&h](double x, const double* p) { return h(x, p); }, n_par, &scale);
    return {k, scale};
}

static void test_classifier() {
    EXPECT(kind0<double>([](double x) { return one(x); }) == std::make_pair((int)SSME_H_X, 1.0));
    EXPECT(kind0<double>([](double x) { return one(x * x); }) == std::make_pair((int)SSME_H_X2, 1.0));
    EXPECT(kind0<double>([](double x) { return one(std::exp(0.5 * x)); }) == std::make_pair((int)SSME_H_VOL, 1.0));
    EXPECT(kind0<float>([](float x) { return one((float)std::exp(0.5f * x)); }) == std::make_pair((int)SSME_H_VOL, 1.0));
    EXPECT(kind0<float>([](float x) { return one(x * x); }) == std::make_pair((int)SSME_H_X2, 1.0));
    EXPECT(kind0<double>([](double) { return one(7.0); }) == std::make_pair((int)SSME_H_CONST42, 7.0 / 42.0));
    EXPECT(kind0<double>([](double) { return one(42.0); }) == std::make_pair((int)SSME_H_CONST42, 1.0));
    // a tail indicator: 0 at all six probe states, so "the constant 0" -- why the probe is opt-in
    EXPECT(kind0<double>([](double x) { return one(x < -3.0 ? 1.0 : 0.0); }) == std::make_pair((int)SSME_H_CONST42, 0.0));
    // a clamp that equals x on [-1.7, 3.25] is taken for x
    EXPECT(kind0<double>([](double x) { return one(x > 5.0 ? 5.0 : x); }).first == SSME_H_X);
    // not a built-in: host
    EXPECT(kind0<double>([](double x) { return one(std::sin(x)); }).first == -1);
    EXPECT(kind0<double>([](double x) { return one(x + 1.0); }).first == -1);
    // not 1 x 1: host, whatever the entries are
    EXPECT(kind0<double>([](double x) { Mat m(2, 2); m(0, 0) = x; m(1, 1) = x; return m; }).first == -1);
    EXPECT(kind0<double>([](double x) { Mat m(1, 2); m(0, 0) = x; m(0, 1) = x; return m; }).first == -1);

    // four parameter columns: parameter d -> 4 + d; the state built-ins as before; a product -> host
    for (int k = 0; k < 4; ++k)
        EXPECT(kind4([k](double, const double* p) { return one(p[k]); }) == std::make_pair(4 + k, 1.0));
    EXPECT(kind4([](double x, const double*) { return one(x); }) == std::make_pair((int)SSME_H_X, 1.0));
    EXPECT(kind4([](double x, const double*) { return one(x * x); }) == std::make_pair((int)SSME_H_X2, 1.0));
    EXPECT(kind4([](double, const double*) { return one(7.0); }) == std::make_pair((int)SSME_H_CONST42, 7.0 / 42.0));
    EXPECT(kind4([](double x, const double* p) { return one(x * p[2]); }).first == -1);
    EXPECT(kind4([](double x, const double* p) { Mat m(2, 2); m(0, 0) = x; m(1, 1) = p[3]; return m; }).first == -1);
    // the number of parameter columns is an argument: with none, a parameter is not recognised
    EXPECT(kind4([](double, const double* p) { return one(p[0]); }, 0).first == -1);
    EXPECT(kind4([](double, const double* p) { return one(p[3]); }, 3).first == -1);
}

static void test_weighted_mean() {
    const std::vector<double> x = {1.0, 2.0, 4.0, 8.0};
    const std::vector<double> w = {0.5, 0.25, 0.125, 0.125};          // sum 1
    const std::vector<double> w4 = {2.0, 1.0, 0.5, 0.5};              // the same weights, not normalised: sum 4
    for (const std::vector<double>* ww : {&w, &w4}) {
        // scalar-valued: E[x] = 0.5 + 0.5 + 0.5 + 1 = 2.5, E[x^2] = 0.5 + 1 + 2 + 8 = 11.5
        const Mat ex = d::weighted_mean<double, Mat>(4, *ww, [&x](std::size_t i) { return one(x[i]); });
        EXPECT(ex.rows() == 1 && ex.cols() == 1 && ex(0, 0) == 2.5);
        const Mat ex2 = d::weighted_mean<double, Mat>(4, *ww, [&x](std::size_t i) { return one(x[i] * x[i]); });
        EXPECT(ex2(0, 0) == 11.5);
        // 2 x 2-valued, entry by entry: [[x, x^2], [1, 2 x]] -> [[2.5, 11.5], [1, 5]]
        const Mat e = d::weighted_mean<double, Mat>(4, *ww, [&x](std::size_t i) {
            Mat m(2, 2); m(0, 0) = x[i]; m(0, 1) = x[i] * x[i]; m(1, 0) = 1.0; m(1, 1) = 2.0 * x[i]; return m; });
        EXPECT(e.rows() == 2 && e.cols() == 2);
        EXPECT(e(0, 0) == 2.5 && e(0, 1) == 11.5 && e(1, 0) == 1.0 && e(1, 1) == 5.0);
    }
    // a 1 x 3 value keeps its shape (taken from particle 0)
    const Mat r = d::weighted_mean<double, Mat>(4, w, [&x](std::size_t i) { Mat m(1, 3); m(0, 0) = x[i]; m(0, 1) = -x[i]; m(0, 2) = 4.0; return m; });
    EXPECT(r.rows() == 1 && r.cols() == 3 && r(0, 0) == 2.5 && r(0, 1) == -2.5 && r(0, 2) == 4.0);
    // a division by the weight sum, not a product with its reciprocal: (1 * 1 + 2 * 2) / 3 = 5 / 3, and 5 * (1 / 3) is another double
    const std::vector<double> w3 = {1.0, 2.0};
    const Mat t = d::weighted_mean<double, Mat>(2, w3, [](std::size_t i) { return one(i == 0 ? 1.0 : 2.0); });
    EXPECT(t(0, 0) == 5.0 / 3.0 && 5.0 / 3.0 != 5.0 * (1.0 / 3.0));
    // accumulated in double, rounded to float_t once at the end
    const MatF tf = d::weighted_mean<float, MatF>(2, w3, [](std::size_t i) { return one(i == 0 ? 1.0f : 2.0f); });
    EXPECT(tf(0, 0) == (float)(5.0 / 3.0));
    // particles in ascending order, each exactly once
    std::vector<std::size_t> seen;
    d::weighted_mean<double, Mat>(4, w, [&seen](std::size_t i) { seen.push_back(i); return one(0.0); });
    EXPECT((seen == std::vector<std::size_t>{0, 1, 2, 3}));
    // zero weights everywhere: 0 / 0, a NaN and not an exception
    const Mat z = d::weighted_mean<double, Mat>(2, std::vector<double>{0.0, 0.0}, [](std::size_t) { return one(1.0); });
    EXPECT(std::isnan(z(0, 0)));
}

static void test_vector_state() {
    // dimension 2, component-major as the download fills it: x0 = {1, 2, 4, 8}, x1 = {8, 4, 2, 1}
    const std::vector<double> x = {1.0, 2.0, 4.0, 8.0, 8.0, 4.0, 2.0, 1.0};
    const std::vector<double> w = {0.5, 0.25, 0.125, 0.125};
    std::vector<std::pair<std::size_t, double>> calls;                 // (k, x0) of every call, in order
    const std::vector<double> e = d::state_means<2>(4, x, w, 3, [&calls](std::size_t k, const std::array<double, 2>& xi) {
        calls.push_back({k, xi[0]});
        return k == 0 ? xi[0] + xi[1] : k == 1 ? xi[0] * xi[1] : xi[1];
    });
    // x0 + x1 = {9, 6, 6, 9} -> 4.5 + 1.5 + 0.75 + 1.125; x0 x1 = 8 everywhere; x1 -> 4 + 1 + 0.25 + 0.125
    EXPECT(e.size() == 3 && e[0] == 7.875 && e[1] == 8.0 && e[2] == 5.375);
    // particle by particle, the functions in order within a particle
    bool order = calls.size() == 12;
    for (std::size_t c = 0; order && c < 12; ++c) order = calls[c].first == c % 3 && calls[c].second == x[c / 3];
    EXPECT(order);
    // dimension 1 is the same function
    const std::vector<double> e1 = d::state_means<1>(4, std::vector<double>{1.0, 2.0, 4.0, 8.0}, w, 1,
                                                     [](std::size_t, const std::array<double, 1>& xi) { return xi[0]; });
    EXPECT(e1.size() == 1 && e1[0] == 2.5);
}

// dispatch with stand-ins for the device and the download: device functional `id` "is" 100 + id
struct dispatch_run {
    std::vector<Mat> out;
    std::vector<std::vector<int32_t>> device_calls;
    int downloads = 0;
    std::vector<std::size_t> hosted, classified;
};
static dispatch_run run_dispatch(std::size_t n, const std::vector<int>& declared, const d::device_policy& pol, bool probe,
                                 const std::vector<int>& probe_says) {
    dispatch_run r;
    r.out = d::dispatch_expectations<double, Mat>(
        n, declared, pol, probe,
        [&](std::size_t j, double* scale) { r.classified.push_back(j); *scale = 0.5; return probe_says[j]; },
        [&](const std::vector<int32_t>& ids) {
            r.device_calls.push_back(ids);
            std::vector<double> v;
            for (int32_t id : ids) v.push_back(100.0 + id);
            return v;
        },
        [&] { ++r.downloads; },
        [&](std::size_t j) { EXPECT(r.downloads == 1); r.hosted.push_back(j); Mat m(2, 1); m(0, 0) = (double)j; m(1, 0) = -1.0; return m; });
    return r;
}

static void test_dispatch() {
    using ids_t = std::vector<int32_t>;
    const std::vector<int> none;
    // nothing declared, no probe: everything on the host, one download, no device call
    dispatch_run r = run_dispatch(3, none, d::bootstrap_policy, false, {0, 0, 0});
    EXPECT(r.device_calls.empty() && r.downloads == 1 && (r.hosted == std::vector<std::size_t>{0, 1, 2}) && r.classified.empty());
    EXPECT(r.out.size() == 3 && r.out[2].rows() == 2 && r.out[2](0, 0) == 2.0);
    // no functionals: nothing is called
    r = run_dispatch(0, {SSME_H_X}, d::bootstrap_policy, true, {});
    EXPECT(r.out.empty() && r.device_calls.empty() && r.downloads == 0);
    // declared wins over the probe; -1 and out-of-range declarations fall to the probe; results in the caller's order; the
    // probe's scale applies to probed slots only
    r = run_dispatch(4, {SSME_H_CONST42, -1, 9, SSME_H_X}, d::bootstrap_policy, true, {-1, SSME_H_X2, -1, -1});
    EXPECT(r.device_calls.size() == 1 && (r.device_calls[0] == ids_t{SSME_H_CONST42, SSME_H_X2, SSME_H_X}));
    EXPECT((r.classified == std::vector<std::size_t>{1, 2}) && (r.hosted == std::vector<std::size_t>{2}) && r.downloads == 1);
    EXPECT(r.out[0].rows() == 1 && r.out[0](0, 0) == 100.0 + SSME_H_CONST42 && r.out[1](0, 0) == (100.0 + SSME_H_X2) * 0.5);
    EXPECT(r.out[2].rows() == 2 && r.out[2](0, 0) == 2.0 && r.out[3](0, 0) == 100.0 + SSME_H_X);
    // everything on the device: no download
    r = run_dispatch(2, {SSME_H_X, SSME_H_VOL}, d::bootstrap_policy, false, {-1, -1});
    EXPECT(r.downloads == 0 && r.hosted.empty() && r.device_calls.size() == 1);
    // the bootstrap cap: the fifth device functional goes to the host; ids 4-7 are not declarable there
    r = run_dispatch(6, {SSME_H_X, SSME_H_X, SSME_H_X2, SSME_H_VOL, SSME_H_CONST42, 5}, d::bootstrap_policy, false, {});
    EXPECT((r.device_calls[0] == ids_t{SSME_H_X, SSME_H_X, SSME_H_X2, SSME_H_VOL}) && (r.hosted == std::vector<std::size_t>{4, 5}) && r.downloads == 1);
    // Liu-West: ids 0-7 declarable, no cap
    r = run_dispatch(6, {0, 1, 2, 3, 4, 7}, d::liu_west_policy, false, {});
    EXPECT((r.device_calls[0] == ids_t{0, 1, 2, 3, 4, 7}) && r.hosted.empty() && r.downloads == 0);
    r = run_dispatch(2, {8, -1}, d::liu_west_policy, true, {-1, 6});
    EXPECT((r.device_calls[0] == ids_t{6}) && (r.hosted == std::vector<std::size_t>{0}) && r.out[1](0, 0) == 106.0 * 0.5);
}

static void test_evaluator_inputs() {
    struct v1 { double v; double operator()(int) const { return v; } };
    struct pack { double p[3]; v1 get_untrans_params(unsigned a, unsigned) const { return v1{p[a]}; } };
    const std::vector<v1> data = {{0.5}, {-1.25}, {3.0}};
    EXPECT((d::column0(data) == std::vector<double>{0.5, -1.25, 3.0}));
    EXPECT(d::column0(std::vector<v1>()).empty());
    const std::array<double, 3> th = d::svol_theta(pack{{1.0, 0.95, 0.0625}});     // beta, phi, ss -> beta, phi, sqrt(ss)
    EXPECT(th[0] == 1.0 && th[1] == 0.95 && th[2] == 0.25);
}

int main() {
    test_classifier();
    test_weighted_mean();
    test_vector_state();
    test_dispatch();
    test_evaluator_inputs();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("functional_host ok\n");
    return failures ? 1 : 0;
}
