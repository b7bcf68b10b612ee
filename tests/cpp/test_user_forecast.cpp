// user_bs_gpu<nparts, 2, 2>::sim_future_obs (include/ssme_gpu/bsfilter_gpu.hpp): the forecast of a user model whose header declares
// its observation draw (tests/models/svol_two_factor_g.h), y[time][component][particle].  Linked against the library built with that
// header.  Prints "name value" lines that tests/test_forecast_user_gpu.py compares with ParticleFilterBank.sim_future_obs of the same
// seed and filter id: a few values and a 64-bit sum of all bit patterns.
#include <array>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<double> spy;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) if (!line.empty()) spy.push_back(std::stod(line));
    }
    constexpr std::size_t N = 3001;
    constexpr unsigned H = 3;
    using model = ssme_gpu::user_bs_gpu<N, 2, 2>;
    ssme_gpu::gpu_options o;
    o.seed = 21;
    model mod({1.1, 0.95, 0.9, 0.2, 0.15, -0.4}, o, /*filter_id=*/1);
    for (int t = 0; t < 4; ++t) {
        const std::array<double, 2> y = {spy[t], spy[100 + t]};
        mod.filter(y);
    }
    std::printf("has_gsamp %d\n", ssme_pf_user_model_has_gsamp());
    const std::vector<double> y = mod.sim_future_obs(H, 0.25), again = mod.sim_future_obs(H, 0.25);
    if (y.size() != (std::size_t)H * 2 * N) return 3;
    std::uint64_t sum = 0;
    for (double v : y) { std::uint64_t b; std::memcpy(&b, &v, 8); sum += b; }
    std::printf("size %zu\n", y.size());
    std::printf("bitsum %" PRIu64 "\n", sum);
    const std::size_t probes[6] = {0, N - 1, N, 2 * N + 17, (std::size_t)(H - 1) * 2 * N + N + 5, (std::size_t)H * 2 * N - 1};
    for (int k = 0; k < 6; ++k) std::printf("y_%zu %.17g\n", probes[k], y[probes[k]]);
    std::printf("repeat %s\n", y == again ? "same" : "different");
    return 0;
}
