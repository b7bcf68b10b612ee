// The whole-series Liu-West route through the C ABI from C++ (include/ssme_pf.h): route query, setter, and ssme_lw_run_series on
// both routes with equal results.  argv[1]: spy_returns.csv.  Prints one "<name> ok" line per check; exit status 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/ssme_pf.h"

static int failures = 0;
static void check(bool ok, const char* name) {
    std::printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}
static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (std::isnan(a[i]) && std::isnan(b[i])) continue;
        if (std::memcmp(&a[i], &b[i], sizeof(double)) != 0) return false;
    }
    return true;
}

static ssme_lw_config config(int n, int r, int form) {
    ssme_lw_config c;
    std::memset(&c, 0, sizeof(c));
    c.n_particles = n; c.n_filters = r; c.seed = 11; c.device = 0; c.first_filter_id = 0; c.delta = 0.99;
    const int32_t tr[4] = {2, 0, 3, 1};                    // logit, null, log, twice Fisher
    const double lo[4] = {0.8, -0.1, 0.01, -0.5}, hi[4] = {0.99, 0.1, 0.1, -0.01};
    for (int d = 0; d < 4; ++d) { c.transforms[d] = tr[d]; c.prior_lo[d] = lo[d]; c.prior_hi[d] = hi[d]; }
    c.form = form; c.resamp_sched = 1;
    return c;
}

struct Result { std::vector<double> tot, per, x, th, means; };
static bool run(ssme_lw_handle h, const std::vector<double>& y, const std::vector<double>& z, int n, int r, Result* out) {
    const int T = (int)y.size();
    out->tot.assign(r, 0.0); out->per.assign((size_t)r * T, 0.0); out->x.assign(n, 0.0); out->th.assign((size_t)4 * n, 0.0);
    out->means.assign((size_t)4 * r, 0.0);
    if (ssme_lw_run_series(h, y.data(), z.data(), T, out->tot.data()) != SSME_OK) return false;
    if (ssme_lw_get_per_step(h, out->per.data(), T) != SSME_OK) return false;
    if (ssme_lw_get_param_means(h, out->means.data()) != SSME_OK) return false;
    return ssme_lw_download_state(h, r - 1, out->x.data(), out->th.data(), nullptr, nullptr, nullptr, nullptr) == SSME_OK;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_lw_series spy_returns.csv\n"); return 2; }
    std::vector<double> y, z;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line) && y.size() < 40) if (!line.empty()) y.push_back(std::stod(line));
        z.assign(y.size(), 0.0);
        for (size_t i = 1; i < y.size(); ++i) z[i] = y[i - 1];
    }
    if (y.size() != 40) { std::fprintf(stderr, "series too short\n"); return 2; }

    int32_t route = -1, threads = -1;
    check(ssme_lw_set_small_series(nullptr, 1) == SSME_ERR_INVALID_ARG, "setter refuses a null handle");
    check(ssme_lw_get_series_route(nullptr, &route, &threads) == SSME_ERR_INVALID_ARG && route == -1, "query refuses a null handle");

    for (int form = 0; form < 2; ++form) {
        const int n = 500, r = 3;
        ssme_lw_config c = config(n, r, form);
        ssme_lw_handle hs = nullptr, ht = nullptr, big = nullptr;
        if (ssme_lw_create(&c, &hs) != SSME_OK || ssme_lw_create(&c, &ht) != SSME_OK) { std::fprintf(stderr, "create failed\n"); return 1; }
        check(ssme_lw_get_series_route(hs, nullptr, &threads) == SSME_ERR_INVALID_ARG &&
              ssme_lw_get_series_route(hs, &route, nullptr) == SSME_ERR_INVALID_ARG, "query refuses null outputs");
        check(ssme_lw_set_small_series(hs, 2) == SSME_ERR_INVALID_ARG, "setter refuses a value other than 0 and 1");
        check(ssme_lw_set_small_series(hs, 1) == SSME_OK && ssme_lw_get_series_route(hs, &route, &threads) == SSME_OK &&
              route == SSME_ROUTE_LW_SERIES && threads == 512, "series route after set_small_series(1)");
        check(ssme_lw_set_small_series(ht, 0) == SSME_OK && ssme_lw_get_series_route(ht, &route, &threads) == SSME_OK &&
              route == SSME_ROUTE_TILED && threads == 512, "tiled route after set_small_series(0)");
        ssme_lw_config cb = config(2049, 1, form);
        if (ssme_lw_create(&cb, &big) != SSME_OK) { std::fprintf(stderr, "create failed\n"); return 1; }
        check(ssme_lw_set_small_series(big, 1) == SSME_OK && ssme_lw_get_series_route(big, &route, &threads) == SSME_OK &&
              route == SSME_ROUTE_TILED, "two tiles stay tiled");
        ssme_lw_destroy(big);

        Result a, b;
        const bool ran = run(hs, y, z, n, r, &a) && run(ht, y, z, n, r, &b);
        check(ran, "run_series on both routes");
        check(ran && same_bits(a.tot, b.tot) && same_bits(a.per, b.per), "log-likelihoods equal");
        check(ran && same_bits(a.x, b.x) && same_bits(a.th, b.th) && same_bits(a.means, b.means), "state and parameter means equal");
        check(ssme_lw_reset(hs) == SSME_OK && ssme_lw_get_series_route(hs, &route, &threads) == SSME_OK && route == SSME_ROUTE_LW_SERIES,
              "the setting survives reset");
        ssme_lw_destroy(hs);
        ssme_lw_destroy(ht);
    }
    return failures ? 1 : 0;
}
