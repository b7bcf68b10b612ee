// user_bswc_gpu<nparts, 1, 1, 3> (include/ssme_gpu/bsfilter_gpu.hpp): the BSFilterWC counterpart for a user model whose header declares
// covariates (tests/models/svol_reg_cov.h: dim_cov = 3, first / first_logw, gsamp, three functionals).  Linked against the library
// built with that header.  Reads "y z0 z1 z2" rows from the file given as argv[1] and prints "name value" lines (doubles as hex
// floats, bit for bit) that tests/test_user_cov_gpu.py compares with ParticleFilterBank of the same seed and filter id.
#include <array>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<std::array<double, 4>> rows;
    {
        std::ifstream f(argv[1]);
        std::array<double, 4> r;
        while (f >> r[0] >> r[1] >> r[2] >> r[3]) rows.push_back(r);
    }
    if (rows.empty()) return 3;
    constexpr std::size_t N = 500;
    using model = ssme_gpu::user_bswc_gpu<N, 1, 1, 3>;
    ssme_gpu::gpu_options o;
    o.seed = 77;
    model mod({0.9, 0.1, 0.3, -0.2, 0.25, -0.05}, o, /*filter_id=*/1);
    std::printf("dim_cov %d\n", ssme_pf_user_model_dim_cov());
    std::printf("has_first %d\n", ssme_pf_user_model_has_first());
    // two host functions of (x_t, z_t); the first is the header's h_0
    const std::vector<model::func> fs = {
        [](const model::state_vector& x, const model::cov_vector&) { return x[0]; },
        [](const model::state_vector& x, const model::cov_vector& z) { return x[0] + 0.25 * z[2]; },
    };
    for (std::size_t t = 0; t < rows.size(); ++t) {
        const std::array<double, 1> y = {rows[t][0]};
        const std::array<double, 3> z = {rows[t][1], rows[t][2], rows[t][3]};
        mod.filter(y, z, fs);
        std::printf("ll_%zu %a\n", t, (double)mod.getLogCondLike());
    }
    const std::vector<double> me = mod.getModelExpectations();
    for (std::size_t k = 0; k < me.size(); ++k) std::printf("me_%zu %a\n", k, me[k]);
    for (std::size_t k = 0; k < fs.size(); ++k) std::printf("host_%zu %a\n", k, mod.getExpectations()[k]);
    const std::vector<double> zf = {0.5, -0.25, 1.0, -1.5, 0.75, 0.125};
    const std::vector<double> ys = mod.sim_future_obs(2, zf);
    std::printf("fc_size %zu\n", ys.size());
    std::printf("fc_0 %a\n", ys[0]);
    std::printf("fc_last %a\n", ys[ys.size() - 1]);
    bool threw = false;
    try { mod.sim_future_obs(2, std::vector<double>(5)); } catch (const std::invalid_argument&) { threw = true; }
    std::printf("short_covs_throw %d\n", threw ? 1 : 0);
    return 0;
}
