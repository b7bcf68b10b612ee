// Forecasts through the C++ adaptor (include/ssme_gpu/bsfilter_gpu.hpp): member sim_future_obs and swarm simFutureObs must return
// the bits of the C ABI call on the same handle at the same origin (a forecast is repeatable), in the shape [member][time][particle].
//   test_forecast spy_returns.csv        prints one "<name> ok" line per object; exit status 1 on any mismatch
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include "../../include/ssme_gpu/bsfilter_gpu.hpp"
#include "swarm_shape.hpp"

using vec1 = shape::vec1<double>;
using Mat = shape::dynmat<double>;
constexpr unsigned H = 3;

static int failures = 0;
static void report(const char* name, bool ok) {
    std::printf("%s %s\n", name, ok ? "ok" : "MISMATCH");
    if (!ok) ++failures;
}
static bool same(const std::vector<double>& a, const double* b, std::size_t n) { return a.size() == n && std::memcmp(a.data(), b, n * sizeof(double)) == 0; }

// what the C ABI returns for all R filters of a bootstrap handle
static std::vector<double> abi_pf(ssme_pf_handle h, int R, std::size_t N, double last) {
    std::vector<double> lo((std::size_t)R, last), y((std::size_t)R * H * N);
    const int rc = ssme_pf_sim_future_obs(h, (int32_t)H, lo.data(), y.data(), nullptr, nullptr);
    if (rc != SSME_OK) { std::printf("ssme_pf_sim_future_obs status %d\n", rc); ++failures; }
    return y;
}

struct cov_swarm : ssme_gpu::swarm_with_covs_gpu<600, 5, double> {
    using ssme_gpu::swarm_with_covs_gpu<600, 5, double>::swarm_with_covs_gpu;
    int k = 0;
    std::vector<double> samp_untrans_params() override {
        const double u = 0.1 + 0.2 * k++;
        return {0.8 + 0.19 * u, -0.1 + 0.2 * u, 0.01 + 0.09 * u, -0.5 + 0.49 * u};
    }
};
struct nocov_swarm : ssme_gpu::swarm_gpu<400, 3, double> {
    using ssme_gpu::swarm_gpu<400, 3, double>::swarm_gpu;
    int k = 0;
    std::vector<double> samp_untrans_params() override { const double u = 0.2 + 0.3 * k++; return {0.9 + 0.05 * u, 0.8 + 0.4 * u, 0.2 + 0.1 * u}; }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<vec1> data;
    std::ifstream f(argv[1]);
    double v;
    while (f >> v && data.size() < 8) data.push_back(vec1{v});
    if (data.size() < 8) return 2;
    const std::size_t T = 5;
    const double last = data[T - 1](0);
    ssme_gpu::gpu_options o;
    o.seed = 91;
    {   // a leverage model object with its own handle
        using lev = ssme_gpu::svol_leverage_gpu<700, double, Mat, vec1, vec1, vec1>;
        lev m(0.9, 0.0, 0.3, -0.2, 0, o, 2);
        for (std::size_t t = 0; t < T; ++t) m.filter(data[t], t ? data[t - 1] : vec1{0.0});
        const std::vector<double> y = m.sim_future_obs(H, last);
        const std::vector<double> w = abi_pf(m.native(), 1, 700, last);
        report("svol_leverage_gpu", same(y, w.data(), (std::size_t)H * 700));
    }
    {   // a no-covariate member with its own handle
        using bs = ssme_gpu::svol_bs_member_gpu<400, double, Mat, vec1, vec1>;
        bs m(0.95, 1.0, 0.25, o, 1);
        for (std::size_t t = 0; t < T; ++t) m.filter(data[t]);
        const std::vector<double> y = m.sim_future_obs(H);
        const std::vector<double> w = abi_pf(m.native(), 1, 400, 0.0);
        report("svol_bs_member_gpu", same(y, w.data(), (std::size_t)H * 400));
    }
    {   // members of one swarm_context: one device call serves all of them; member i gets slice i of [member][time][particle]
        using lev = ssme_gpu::svol_leverage_gpu<600, double, Mat, vec1, vec1, vec1>;
        auto ctx = std::make_shared<lev::context>(SSME_MODEL_SVOL_LEVERAGE, 600, 3, o);
        std::vector<lev> ms;
        for (int i = 0; i < 3; ++i) ms.emplace_back(0.9 + 0.02 * i, 0.0, 0.2 + 0.05 * i, -0.1 * (i + 1), ctx);
        for (std::size_t t = 0; t < T; ++t) for (auto& m : ms) m.filter(data[t], t ? data[t - 1] : vec1{0.0});
        std::vector<std::vector<double>> ys;
        for (auto& m : ms) ys.push_back(m.sim_future_obs(H, last));
        const std::vector<double> w = abi_pf(ctx->native(), 3, 600, last);
        bool ok = true;
        for (int i = 0; i < 3; ++i) ok = ok && same(ys[i], w.data() + (std::size_t)i * H * 600, (std::size_t)H * 600);
        ok = ok && std::memcmp(w.data(), w.data() + (std::size_t)H * 600, sizeof(double) * H * 600) != 0;      // members differ
        report("swarm_context members", ok);
    }
    {   // the Liu-West filters, both forms
        ssme_gpu::svol_lw_1_par_gpu<800> m1(0.99, 0.8, 0.99, -0.1, 0.1, 0.01, 0.1, -0.5, -0.01, 0, o, 0);
        ssme_gpu::svol_lw_2_par_gpu<800> m2(0.99, 0.8, 0.99, -0.1, 0.1, 0.01, 0.1, -0.5, -0.01, 0, o, 0);
        for (std::size_t t = 0; t < T; ++t) { m1.filter(data[t], t ? data[t - 1] : vec1{0.0}); m2.filter(data[t], t ? data[t - 1] : vec1{0.0}); }
        std::vector<double> w((std::size_t)H * 800);
        const std::vector<double> y1 = m1.sim_future_obs(H, last);
        int rc = ssme_lw_sim_future_obs(m1.native(), (int32_t)H, &last, w.data(), nullptr, nullptr, nullptr);
        report("svol_lw_1_par_gpu", rc == SSME_OK && same(y1, w.data(), w.size()));
        const std::vector<double> y2 = m2.sim_future_obs(H, last);
        rc = ssme_lw_sim_future_obs(m2.native(), (int32_t)H, &last, w.data(), nullptr, nullptr, nullptr);
        report("svol_lw_2_par_gpu", rc == SSME_OK && same(y2, w.data(), w.size()) && y1 != y2);
    }
    {   // the batched swarms: one call for all members, the whole [member][time][particle] block equals the C ABI call on the
        // swarm's handle at the same origin (last_obs handed to every member)
        cov_swarm sw({SSME_H_X});
        for (std::size_t t = 0; t < T; ++t) sw.update(data[t], t ? data[t - 1] : vec1{0.0});
        const std::vector<double> y = sw.simFutureObs(H, last);
        const std::vector<double> w = abi_pf(sw.native(), 5, 600, last);
        const std::vector<double> w0 = abi_pf(sw.native(), 5, 600, 0.0);
        report("swarm_with_covs_gpu", same(y, w.data(), (std::size_t)5 * H * 600) && y != w0 &&           // last_obs reaches the leverage model
                                       std::memcmp(y.data(), y.data() + (std::size_t)H * 600, sizeof(double) * H * 600) != 0);
        nocov_swarm sn({SSME_H_X});
        for (std::size_t t = 0; t < T; ++t) sn.update(data[t]);
        const std::vector<double> yn = sn.simFutureObs(H);
        const std::vector<double> wn = abi_pf(sn.native(), 3, 400, 0.0);
        report("swarm_gpu", same(yn, wn.data(), (std::size_t)3 * H * 400) &&
                             std::memcmp(yn.data(), yn.data() + (std::size_t)H * 400, sizeof(double) * H * 400) != 0);
    }
    {   // a member that is one observation behind its swarm_context is refused; after everybody was served a new call forecasts again
        using lev = ssme_gpu::svol_leverage_gpu<600, double, Mat, vec1, vec1, vec1>;
        auto ctx = std::make_shared<lev::context>(SSME_MODEL_SVOL_LEVERAGE, 600, 2, o);
        lev a(0.9, 0.0, 0.2, -0.1, ctx), b(0.95, 0.0, 0.3, -0.2, ctx);
        a.filter(data[0], vec1{0.0}); b.filter(data[0], vec1{0.0});
        a.filter(data[1], data[0]);                                   // b lags by one observation
        bool refused = false;
        try { b.sim_future_obs(H, data[1](0)); } catch (const std::runtime_error&) { refused = true; }
        b.filter(data[1], data[0]);
        const std::vector<double> ya = a.sim_future_obs(H, data[1](0)), yb = b.sim_future_obs(H, data[1](0));   // both served: the copy is released
        const std::vector<double> w = abi_pf(ctx->native(), 2, 600, data[1](0));
        report("swarm_context lagging member", refused && same(ya, w.data(), (std::size_t)H * 600) && same(yb, w.data() + (std::size_t)H * 600, (std::size_t)H * 600) &&
                                                a.sim_future_obs(H, data[1](0)) == ya);
    }
    return failures ? 1 : 0;
}
