// Recorded Liu-West series through the C ABI from C++ (include/ssme_pf.h): the setter's refusals, a recording ssme_lw_run_series on
// both routes with equal rows, the last row against ssme_lw_get_expectations, and the [T][n][R] layout with a permuted id list.
// argv[1]: spy_returns.csv.  Prints one "<name> ok" line per check; exit status 1 on a mismatch.
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

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_lw_series_expect spy_returns.csv\n"); return 2; }
    std::vector<double> y, z;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line) && y.size() < 40) if (!line.empty()) y.push_back(std::stod(line));
        z.assign(y.size(), 0.0);
        for (size_t i = 1; i < y.size(); ++i) z[i] = y[i - 1];
    }
    if (y.size() != 40) { std::fprintf(stderr, "series too short\n"); return 2; }
    const int T = (int)y.size();
    const int32_t all[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    double one = -1.0;

    check(ssme_lw_set_series_expectations(nullptr, 1) == SSME_ERR_INVALID_ARG, "setter refuses a null handle");
    check(ssme_lw_get_series_expectations(nullptr, all, 8, &one, 1) == SSME_ERR_INVALID_ARG && one == -1.0, "getter refuses a null handle");

    for (int form = 0; form < 2; ++form) {
        const int n = 500, r = 3;
        ssme_lw_config c = config(n, r, form);
        ssme_lw_handle hs = nullptr, ht = nullptr;
        if (ssme_lw_create(&c, &hs) != SSME_OK || ssme_lw_create(&c, &ht) != SSME_OK) { std::fprintf(stderr, "create failed\n"); return 1; }
        check(ssme_lw_set_series_expectations(hs, 2) == SSME_ERR_INVALID_ARG && ssme_lw_set_series_expectations(hs, -1) == SSME_ERR_INVALID_ARG,
              "setter refuses a value other than 0 and 1");
        std::vector<double> rows_s((size_t)T * 8 * r, -1.0), rows_t(rows_s), tot(r, 0.0);
        check(ssme_lw_get_series_expectations(hs, all, 8, rows_s.data(), 1) == SSME_ERR_STATE, "nothing recorded before a series");
        check(ssme_lw_set_series_expectations(hs, 1) == SSME_OK && ssme_lw_set_series_expectations(ht, 1) == SSME_OK &&
              ssme_lw_set_small_series(hs, 1) == SSME_OK && ssme_lw_set_small_series(ht, 0) == SSME_OK, "recording on, one handle per route");
        int32_t route_s = -1, route_t = -1, threads = -1;
        check(ssme_lw_get_series_route(hs, &route_s, &threads) == SSME_OK && ssme_lw_get_series_route(ht, &route_t, &threads) == SSME_OK &&
              route_s == SSME_ROUTE_LW_SERIES && route_t == SSME_ROUTE_TILED, "a recording handle of one tile keeps the series route");
        const bool ran = ssme_lw_run_series(hs, y.data(), z.data(), T, tot.data()) == SSME_OK &&
                         ssme_lw_run_series(ht, y.data(), z.data(), T, tot.data()) == SSME_OK &&
                         ssme_lw_get_series_expectations(hs, all, 8, rows_s.data(), T) == SSME_OK &&
                         ssme_lw_get_series_expectations(ht, all, 8, rows_t.data(), T) == SSME_OK;
        check(ran, "recording run_series on both routes");
        check(ran && same_bits(rows_s, rows_t), "rows of both routes equal");
        bool finite = true;
        for (double v : rows_s) finite = finite && std::isfinite(v);
        check(finite, "every row written");
        std::vector<double> last((size_t)8 * r, -1.0);
        check(ssme_lw_get_expectations(hs, all, 8, last.data()) == SSME_OK &&
              same_bits(last, std::vector<double>(rows_s.begin() + (size_t)(T - 1) * 8 * r, rows_s.end())),
              "row T-1 equals ssme_lw_get_expectations after the series");
        // out[(t*n + i)*R + r] with a permuted list
        const int32_t perm[3] = {6, 0, 5};
        std::vector<double> some((size_t)T * 3 * r, -1.0);
        bool layout = ssme_lw_get_series_expectations(hs, perm, 3, some.data(), T) == SSME_OK;
        for (int t = 0; layout && t < T; ++t)
            for (int i = 0; i < 3; ++i)
                for (int f = 0; f < r; ++f)
                    layout = layout && std::memcmp(&some[((size_t)t * 3 + i) * r + f], &rows_s[((size_t)t * 8 + perm[i]) * r + f], sizeof(double)) == 0;
        check(layout, "[T][n][R] layout with a permuted id list");
        check(ssme_lw_get_series_expectations(hs, all, 8, rows_s.data(), T + 1) == SSME_ERR_INVALID_ARG, "T beyond the recorded series is refused");
        ssme_lw_destroy(hs);
        ssme_lw_destroy(ht);
    }
    return failures ? 1 : 0;
}
