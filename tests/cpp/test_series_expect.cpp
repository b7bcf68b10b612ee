// The filtered path through the adaptor's evaluators (include/ssme_gpu/bsfilter_gpu.hpp): record_expectations /
// record_user_expectations, then series_expectations() / series_user_expectations() after operator() -- every row against a second
// handle that is stepped through the C ABI (ssme_pf_step + ssme_pf_get_expectations_multi / ssme_pf_get_user_expectations), bit for bit.
//   stock library:                      test_series_expect DATA.csv
//   -DSERIES_EXPECT_USER (svol_reg_cov: dimx = dimy = 1, dim_cov = 3, n_h = 3), linked with that library
// Prints "name value" lines; tests/test_series_expectations_cpu.py compiles it and, on a GPU, runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

#ifndef SERIES_EXPECT_USER
struct vec1 { double v; double operator()(unsigned) const { return v; } };
struct pack3 {                         // stand-in for param::pack<double,3>::get_untrans_params(i,i): beta, phi, ss
    double p[3];
    vec1 get_untrans_params(unsigned a, unsigned) const { return vec1{p[a]}; }
};

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s spy_returns.csv\n", argv[0]); return 2; }
    std::vector<ssme_gpu::csv_row> data = ssme_gpu::read_data(argv[1]);
    data.resize(48);
    const pack3 theta{{1.0, 0.95, 0.0625}};
    const std::vector<std::int32_t> ids = {SSME_H_VOL, SSME_H_X};
    const int shapes[2] = {500, 1500};                     // the lane and the pair kernel
    for (int nparts : shapes) {
        const int R = 3;
        ssme_gpu::gpu_options o;
        o.seed = 1;
        ssme_gpu::svol_log_like_evaluator ev(data, nparts, R, o);
        const double plain = ev(theta, 77);
        ev.record_expectations(ids);
        const double recorded = ev(theta, 77);
        const std::vector<double> traj = ev.series_expectations();
        // the yardstick: a handle of the same configuration and seed, stepped
        ssme_gpu::handle h(SSME_MODEL_SVOL, nparts, R, 77, o.resampler, o.resamp_sched, o.device, 0);
        const double th[3] = {1.0, 0.95, 0.25};
        ssme_gpu::check(ssme_pf_set_params(h.get(), th, 3, 1), h.get());
        std::vector<double> want, row(ids.size() * R), lcl(R);
        for (std::size_t t = 0; t < data.size(); ++t) {
            const double y = data[t](0);
            ssme_gpu::check(ssme_pf_step(h.get(), &y, nullptr, lcl.data()), h.get());
            ssme_gpu::check(ssme_pf_get_expectations_multi(h.get(), ids.data(), (std::int32_t)ids.size(), row.data()), h.get());
            want.insert(want.end(), row.begin(), row.end());
        }
        std::printf("n%d_rows %zu\n", nparts, traj.size() / (ids.size() * R));
        std::printf("n%d_equals_stepping %d\n", nparts, same_bits(traj, want) ? 1 : 0);
        std::printf("n%d_loglik_unchanged %d\n", nparts, std::memcmp(&plain, &recorded, sizeof(double)) == 0 ? 1 : 0);
        std::printf("n%d_vol_last %.17g\n", nparts, traj[(data.size() - 1) * ids.size() * R]);
        // What was recorded stays readable, at its own size, whatever record_expectations is told afterwards: switched off, a shorter
        // list, a rejected list.  (The C call copies the rows of the LAST run: a result sized from the new list would be overrun.)
        ev.record_expectations({});
        std::printf("n%d_off_then_read %d\n", nparts, same_bits(ev.series_expectations(), want) ? 1 : 0);
        ev.record_expectations({SSME_H_X});
        std::printf("n%d_shrink_then_read %d\n", nparts, same_bits(ev.series_expectations(), want) ? 1 : 0);
        bool rejected = false;
        try { ev.record_expectations({SSME_H_CONST42 + 1}); } catch (const std::invalid_argument&) { rejected = true; }
        std::printf("n%d_bad_id_rejected %d\n", nparts, rejected ? 1 : 0);
        ev(theta, 77);                                     // the list before the rejected one is still set: SSME_H_X alone
        const std::vector<double> one = ev.series_expectations();
        bool x_rows = one.size() == data.size() * R;
        for (std::size_t t = 0; x_rows && t < data.size(); ++t)
            x_rows = std::memcmp(&one[t * R], &want[(t * ids.size() + 1) * R], R * sizeof(double)) == 0;
        std::printf("n%d_after_rejection_x_alone %d\n", nparts, x_rows ? 1 : 0);
        ev.record_expectations(ids);                       // a longer list set, the shorter one recorded
        std::printf("n%d_grow_then_read %d\n", nparts, same_bits(ev.series_expectations(), one) ? 1 : 0);
        ev.record_expectations({});
        ev(theta, 77);
        bool threw = false;
        try { ev.series_expectations(); } catch (const std::exception&) { threw = true; }
        std::printf("n%d_off_throws %d\n", nparts, threw ? 1 : 0);
    }
    return 0;
}
#else
int main() {
    const std::size_t T = 12, K = 3;
    std::vector<double> y(T), z(T * K);
    for (std::size_t t = 0; t < T; ++t) {
        y[t] = 0.01 * (double)((int)(t * 7 % 5) - 2);
        for (std::size_t j = 0; j < K; ++j) z[t * K + j] = 0.1 * (double)j - 0.05 * (double)(t % 4);
    }
    const std::vector<double> theta = {0.95, -0.2, 0.25, 0.3, -0.15, 0.1};      // phi, mu, sigma, b0, b2, g
    const std::vector<std::int32_t> ids = {SSME_H_X};
    const int nh = ssme_pf_user_model_n_h();
    const int shapes[3] = {500, 1500, 3000};               // lane kernel, pair kernel, tiled route
    for (int nparts : shapes) {
        const int R = 2;
        ssme_gpu::gpu_options o;
        ssme_gpu::user_log_like_evaluator<1, 1, 3> ev(y, z, nparts, R, o);
        ev.record_expectations(ids);
        ev.record_user_expectations();
        ev(theta, 5);
        const std::vector<double> traj = ev.series_expectations(), utraj = ev.series_user_expectations();
        ssme_gpu::handle h(SSME_MODEL_USER0, nparts, R, 5, o.resampler, o.resamp_sched, o.device, 0);
        ssme_gpu::check(ssme_pf_set_params(h.get(), theta.data(), (std::int32_t)theta.size(), 1), h.get());
        std::vector<double> want, uwant, row(ids.size() * R), urow((std::size_t)nh * R), lcl(R);
        for (std::size_t t = 0; t < T; ++t) {
            ssme_gpu::check(ssme_pf_step(h.get(), &y[t], &z[t * K], lcl.data()), h.get());
            ssme_gpu::check(ssme_pf_get_expectations_multi(h.get(), ids.data(), (std::int32_t)ids.size(), row.data()), h.get());
            ssme_gpu::check(ssme_pf_get_user_expectations(h.get(), urow.data()), h.get());
            want.insert(want.end(), row.begin(), row.end());
            uwant.insert(uwant.end(), urow.begin(), urow.end());
        }
        std::printf("n%d_equals_stepping %d\n", nparts, same_bits(traj, want) ? 1 : 0);
        std::printf("n%d_user_equals_stepping %d\n", nparts, same_bits(utraj, uwant) ? 1 : 0);
        std::printf("n%d_user_rows %zu\n", nparts, utraj.size() / ((std::size_t)nh * R));
        // off, then read; a rejected list leaves the evaluator's own list as it was
        ev.record_expectations({});
        ev.record_user_expectations(false);
        std::printf("n%d_off_then_read %d\n", nparts, (same_bits(ev.series_expectations(), want) && same_bits(ev.series_user_expectations(), uwant)) ? 1 : 0);
        bool rejected = false;
        try { ev.record_expectations({SSME_H_X, SSME_H_X2, -1}); } catch (const std::invalid_argument&) { rejected = true; }
        std::printf("n%d_bad_id_rejected %d\n", nparts, rejected ? 1 : 0);
        std::printf("n%d_rejected_then_read %d\n", nparts, same_bits(ev.series_expectations(), want) ? 1 : 0);
        ev.record_expectations({SSME_H_X, SSME_H_VOL});
        std::printf("n%d_grow_then_read %d\n", nparts, same_bits(ev.series_expectations(), want) ? 1 : 0);
        ev(theta, 5);
        std::printf("n%d_two_ids_rows %zu\n", nparts, ev.series_expectations().size() / (2 * (std::size_t)R));
        bool threw = false;
        try { ev.series_user_expectations(); } catch (const std::exception&) { threw = true; }
        std::printf("n%d_user_off_throws %d\n", nparts, threw ? 1 : 0);
    }
    return 0;
}
#endif
