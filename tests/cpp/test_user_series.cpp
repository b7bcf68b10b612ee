// user_log_like_evaluator<dimx, dimy, dimcov> (include/ssme_gpu/bsfilter_gpu.hpp) against a library built with a vector user model:
// -DDIMCOV=0 with tests/models/svol_two_factor.h, -DDIMCOV=4 with tests/models/svol_two_factor_cov.h (both (dim_x, dim_y) = (2, 2)).
//   test_user_series              the argument checks alone (no device is touched): prints wrong_dimx_throws, wrong_dimcov_throws,
//                                 empty_throws, ragged_throws
//   test_user_series ROWS SEED    ROWS: a text file of T rows of dimy + dimcov values.  N = 500, 4 replicates: prints route, threads,
//                                 ll_0 .. ll_3 (logliks()) and lme (the returned log-mean-exp) as hexadecimal floats
// tests/test_user_series_cpp.py compares them with ParticleFilterBank at the same seed, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"

#ifndef DIMCOV
#define DIMCOV 0
#endif

template <typename Ex, typename F>
static int throws(F f) {
    try { f(); } catch (const Ex&) { return 1; } catch (...) { return 0; }
    return 0;
}

int main(int argc, char** argv) {
    using eval_t = ssme_gpu::user_log_like_evaluator<2, 2, DIMCOV>;
    const std::vector<double> none, y4(4, 0.5), z2(2 * DIMCOV, 0.0);
    if (argc < 3) {
        std::printf("wrong_dimx_throws %d\n", throws<std::invalid_argument>([&] { ssme_gpu::user_log_like_evaluator<3, 2, DIMCOV> e(y4, z2, 500, 4); }));
        std::printf("wrong_dimcov_throws %d\n", throws<std::invalid_argument>([&] { ssme_gpu::user_log_like_evaluator<2, 2, DIMCOV + 1> e(y4, z2, 500, 4); }));
        std::printf("empty_throws %d\n", throws<std::length_error>([&] { eval_t e(none, none, 500, 4); }));
        std::printf("ragged_throws %d\n", throws<std::invalid_argument>([&] { eval_t e(std::vector<double>(3, 0.5), z2, 500, 4); }));
        return 0;
    }
    std::ifstream in(argv[1]);
    std::vector<double> y, z;
    for (;;) {
        double row[2 + DIMCOV];
        bool ok = true;
        for (int j = 0; j < 2 + DIMCOV; ++j) ok = ok && (bool)(in >> row[j]);
        if (!ok) break;
        y.push_back(row[0]); y.push_back(row[1]);
        for (int j = 0; j < DIMCOV; ++j) z.push_back(row[2 + j]);
    }
    eval_t ev(y, z, 500, 4);
    const std::vector<double> theta = {1.1, 0.95, 0.9, 0.2, 0.15, -0.4};
    const double lme = ev(theta, (std::uint64_t)std::strtoull(argv[2], nullptr, 10));
    std::int32_t route = -1, threads = 0;
    ssme_gpu::check(ssme_pf_get_series_route(ev.native(), &route, &threads), ev.native());
    std::printf("route %d\nthreads %d\nrows %zu\n", (int)route, (int)threads, y.size() / 2);
    for (std::size_t r = 0; r < ev.logliks().size(); ++r) std::printf("ll_%zu %a\n", r, ev.logliks()[r]);
    std::printf("lme %a\n", lme);
    std::printf("device_ms_positive %d\n", ev.device_ms() > 0.0f ? 1 : 0);
    return 0;
}
