// test_shard_threads.cpp -- the C++ shard drivers with SEVERAL ranks on one GPU: every rank is a host thread with its own
// handle, the "RCCL" underneath is tests/cpp/mock_rccl.cpp (linked before anything else, so dlsym finds it).  Prints, per
// configuration, what every rank got and what the unsharded filter gives; tests/test_sharded_gpu.py compares.
//   usage: test_shard_threads CSV WORLD N T MODEL RESAMPLER MODE SEED [TAU [YSCALE [RESAMP_SCHED [LW_FORM [DUMP]]]]]     (MODEL -1: Liu-West, RESAMPLER = delta x 1000)
//   TAU (linear-Gaussian model only): observation noise; a tiny value puts all the weight of a step on the one particle next to
//   y_t, so every rank's next resampling window is that particle's tile -- far ranks leave their halo, near ranks do not.
//   YSCALE: the observations are multiplied by it (outliers: the stochastic-volatility weights then degenerate the same way).
//   DUMP: a file that receives rank 0's per-step log conditional likelihoods and the ranks' concatenated final state, for comparison
//   with stored oracle records (tests/test_sharded_gpu.py: _read_dump):  "SSMEDMP1", int64 T, N, kind (0 bootstrap, 1 Liu-West),
//   complete (1 if the state follows), double per[T], then double x[N] and uint64 cdf[N] (bootstrap) or double theta[4][N] (Liu-West).
//   It is written on whichever path the run ended ("-": no dump).
//   Optional, after DUMP (tests/test_shard_edges_gpu.py; "-" leaves one out):  YSET ZSET THETA RERUN
//   YSET / ZSET: "t:value,t:value": single observations / covariates overwritten after YSCALE and after z was taken as the lag of y
//   (strtod: nan, inf, 1e200, -0 are values like any other); THETA: "a,b,c[,d]" in place of the bootstrap model's fixed parameters;
//   RERUN = 1 (bootstrap): every rank first runs the series WITH the overrides and then, on the same handle, the series without them;
//   everything printed, dumped and compared is that second run, the unsharded side a fresh handle on the series without overrides.
//   A rank whose driver returns SSME_ERR_STATE (mode 1 and Liu-West: a window left the fixed halo) is reported ("err_state R 1"), the
//   other ranks are still joined and printed; the exit status is then 5 for a bootstrap run.  All comparisons are by bits: a NaN equals
//   the same NaN, -0 differs from +0.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <thread>
#include <vector>

#include "../../include/ssme_pf.h"

// _Exit: the other ranks' threads are still running (or waiting for this one in a collective); static destructors under them crash
static void overrides(std::vector<double>& v, const char* spec) {             // "t:value,t:value"
    if (!spec || !std::strcmp(spec, "-")) return;
    for (const char* p = spec; *p;) {
        char* e = nullptr;
        const long t = std::strtol(p, &e, 10);
        if (e == p || *e != ':') { std::fprintf(stderr, "bad override list %s\n", spec); std::_Exit(2); }
        const double val = std::strtod(e + 1, &e);
        if (t >= 0 && (size_t)t < v.size()) v[(size_t)t] = val;
        p = *e == ',' ? e + 1 : e;
        if (*e && *e != ',') { std::fprintf(stderr, "bad override list %s\n", spec); std::_Exit(2); }
    }
}
static unsigned long long bits_of(double a) { unsigned long long u; std::memcpy(&u, &a, 8); return u; }

static void die(const char* what, int rc, const char* msg) { std::fprintf(stderr, "%s: status %d (%s)\n", what, rc, msg ? msg : ""); std::fflush(nullptr); std::_Exit(3); }

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    const int world = std::atoi(argv[2]), N = std::atoi(argv[3]), T = std::atoi(argv[4]), model = std::atoi(argv[5]), rs = std::atoi(argv[6]),
              mode = std::atoi(argv[7]);
    const unsigned long long seed = std::strtoull(argv[8], nullptr, 10);
    const int sched = argc > 11 ? std::atoi(argv[11]) : 1;
    const int lw_form = argc > 12 ? std::atoi(argv[12]) : 0;
    const char* dump = (argc > 13 && std::strcmp(argv[13], "-")) ? argv[13] : nullptr;
    const bool rerun = argc > 17 && std::atoi(argv[17]) == 1 && model >= 0;
    std::vector<double> y, z;
    { std::ifstream f(argv[1]); double v; while (f >> v && (int)y.size() < T) y.push_back(v); }
    if (argc > 10) for (double& v : y) v *= std::atof(argv[10]);
    z.assign(y.size(), 0.0);
    for (size_t t = 1; t < y.size(); ++t) z[t] = y[t - 1];
    const std::vector<double> y_plain = y, z_plain = z;                        // RERUN: the second series
    overrides(z, argc > 15 ? argv[15] : nullptr);
    overrides(y, argc > 14 ? argv[14] : nullptr);
    double th_svol[3] = {1.0, 0.95, 0.25}, th_lev[4] = {0.9, 0.0, 1.0, -0.1}, th_lg[3] = {0.9, 0.5, argc > 9 ? std::atof(argv[9]) : 0.7};
    if (argc > 16 && std::strcmp(argv[16], "-") && model >= 0) {
        double* th = model == 0 ? th_svol : (model == 1 ? th_lev : th_lg);
        const char* p = argv[16];
        const int want = model == 1 ? 4 : 3;
        int got = 0;
        for (; got < want && *p; ++got) {
            char* e = nullptr;
            th[got] = std::strtod(p, &e);
            if (e == p || (*e && *e != ',')) break;
            p = *e == ',' ? e + 1 : e;
        }
        if (got != want || *p) { std::fprintf(stderr, "bad theta list %s: model %d takes %d values\n", argv[16], model, want); return 2; }
    }
    char id[128];
    ssme_shard_comm_get_unique_id(id);
    std::vector<double> ll(world, 0.0);
    std::vector<int> path(world, 0), own_flag(world, 0), any_flag(world, 0), err_state(world, 0);
    std::vector<long long> exch(world, 0);
    std::vector<int> reach_l(world, 0), reach_r(world, 0);
    std::vector<std::vector<double>> xs(world), ths(world), pers(world);
    std::vector<std::vector<uint64_t>> cdfs(world);
    std::vector<size_t> first(world, 0);
    std::vector<std::vector<int>> lays(world, std::vector<int>(4, 0));         // ssme_*_shard_layout per rank
    std::vector<std::thread> ranks;
    const auto t_start = std::chrono::steady_clock::now();
    for (int r = 0; r < world; ++r) ranks.emplace_back([&, r] {
        void* comm = nullptr;
        int rc = ssme_shard_comm_init(id, r, world, 0, &comm);
        if (rc) die("comm_init", rc, "");
        int32_t lay[4] = {0, 0, 0, 0};                 // {B, Bl, tiles this rank owns, particles this rank owns}
        if (model >= 0) {
            ssme_pf_config c{};
            c.model = model; c.n_particles = N; c.n_filters = 1; c.dtype = SSME_F64; c.resampler = rs; c.resamp_sched = sched; c.seed = seed; c.device = 0;
            ssme_pf_handle h = nullptr;
            rc = ssme_pf_shard_create(&c, r, world, &h);
            if (rc) die("shard_create", rc, "");
            if (ssme_pf_shard_layout(h, lay)) die("shard_layout", 1, "");
            lays[r].assign(lay, lay + 4);
            xs[r].resize((size_t)lay[3]); cdfs[r].resize((size_t)lay[3]); first[r] = (size_t)r * lay[1] * 2048;
            rc = ssme_pf_set_params(h, model == 0 ? th_svol : (model == 1 ? th_lev : th_lg), model == 1 ? 4 : 3, 1);
            if (rc) die("set_params", rc, ssme_pf_last_error(h));
            rc = ssme_pf_shard_run_series(h, comm, y.data(), model == 1 ? z.data() : nullptr, T, mode, &ll[r]);
            if (rerun) {
                if (rc && rc != SSME_ERR_STATE) die("shard_run_series (first of two)", rc, ssme_pf_last_error(h));
                rc = ssme_pf_shard_run_series(h, comm, y_plain.data(), model == 1 ? z_plain.data() : nullptr, T, mode, &ll[r]);
            }
            if (rc && rc != SSME_ERR_STATE) die("shard_run_series", rc, ssme_pf_last_error(h));
            err_state[r] = rc == SSME_ERR_STATE;               // every rank reads the same reduced flag: all of them or none
            int32_t p = 0; int64_t e = 0;
            ssme_pf_shard_download(h, xs[r].data(), cdfs[r].data(), &p, &e);
            path[r] = p; exch[r] = e;
            int32_t st[4] = {0, 0, 0, 0};
            ssme_pf_shard_stats(h, st);
            any_flag[r] = st[0]; own_flag[r] = st[1]; reach_l[r] = st[2]; reach_r[r] = st[3];
            pers[r].resize((size_t)T);
            if (!err_state[r]) {
                rc = ssme_pf_get_per_step(h, pers[r].data(), T);
                if (rc) die("get_per_step", rc, ssme_pf_last_error(h));
            }
            ssme_pf_destroy(h);
        } else {
            ssme_lw_config c{};
            c.n_particles = N; c.n_filters = 1; c.seed = seed; c.device = 0; c.delta = rs / 1000.0; c.form = lw_form; c.resamp_sched = sched;
            const int tr[4] = {2, 0, 3, 1};
            const double lo[4] = {0.8, -0.1, 0.01, -0.5}, hi[4] = {0.99, 0.1, 0.1, -0.01};
            for (int d = 0; d < 4; ++d) { c.transforms[d] = tr[d]; c.prior_lo[d] = lo[d]; c.prior_hi[d] = hi[d]; }
            ssme_lw_handle h = nullptr;
            rc = ssme_lw_shard_create(&c, r, world, &h);
            if (rc) die("lw_shard_create", rc, "");
            if (ssme_lw_shard_layout(h, lay)) die("lw_shard_layout", 1, "");
            lays[r].assign(lay, lay + 4);
            xs[r].resize((size_t)lay[3]); first[r] = (size_t)r * lay[1] * 2048;
            rc = ssme_lw_shard_run_series(h, comm, y.data(), z.data(), T, &ll[r]);
            path[r] = rc == SSME_ERR_STATE ? 2 : 1;                        // 2: a window left the halo (caller falls back)
            err_state[r] = rc == SSME_ERR_STATE;
            if (rc && rc != SSME_ERR_STATE) die("lw_shard_run_series", rc, ssme_lw_last_error(h));
            int64_t e = 0;
            if (!rc) { ths[r].resize(4 * (size_t)lay[3]); ssme_lw_shard_download(h, xs[r].data(), ths[r].data(), &e); }
            exch[r] = e;
            int32_t st[4] = {0, 0, 0, 0};
            ssme_lw_shard_stats(h, st);
            any_flag[r] = st[0]; own_flag[r] = st[1]; reach_l[r] = st[2]; reach_r[r] = st[3];
            if (!rc) {
                pers[r].resize((size_t)T);
                const int rp = ssme_lw_get_per_step(h, pers[r].data(), T);
                if (rp) die("lw_get_per_step", rp, ssme_lw_last_error(h));
            }
            ssme_lw_destroy(h);
        }
        ssme_shard_comm_destroy(comm);
    });
    for (auto& t : ranks) t.join();
    const auto t_sharded = std::chrono::steady_clock::now();
    // the unsharded filter with the same N and seed
    double ll_ref = 0.0;
    std::vector<double> xref(N), thref, perref((size_t)T);
    std::vector<uint64_t> cdfref;
    if (model >= 0) {
        ssme_pf_config c{};
        c.model = model; c.n_particles = N; c.n_filters = 1; c.dtype = SSME_F64; c.resampler = rs; c.resamp_sched = sched; c.seed = seed; c.device = 0;
        c.tile_particles = 2048;
        ssme_pf_handle h = nullptr;
        if (ssme_pf_create(&c, &h)) die("create", 1, "");
        ssme_pf_set_params(h, model == 0 ? th_svol : (model == 1 ? th_lev : th_lg), model == 1 ? 4 : 3, 1);
        ssme_pf_run_series(h, (rerun ? y_plain : y).data(), model == 1 ? (rerun ? z_plain : z).data() : nullptr, T, &ll_ref);
        cdfref.resize((size_t)N);
        ssme_pf_download_state(h, 0, xref.data(), nullptr, cdfref.data(), nullptr);
        ssme_pf_get_per_step(h, perref.data(), T);
        ssme_pf_destroy(h);
    } else {
        ssme_lw_config c{};
        c.n_particles = N; c.n_filters = 1; c.seed = seed; c.device = 0; c.delta = rs / 1000.0; c.form = lw_form; c.resamp_sched = sched;
        const int tr[4] = {2, 0, 3, 1};
        const double lo[4] = {0.8, -0.1, 0.01, -0.5}, hi[4] = {0.99, 0.1, 0.1, -0.01};
        for (int d = 0; d < 4; ++d) { c.transforms[d] = tr[d]; c.prior_lo[d] = lo[d]; c.prior_hi[d] = hi[d]; }
        ssme_lw_handle h = nullptr;
        if (ssme_lw_create(&c, &h)) die("lw_create", 1, "");
        ssme_lw_run_series(h, y.data(), z.data(), T, &ll_ref);
        thref.resize(4 * (size_t)N);
        ssme_lw_download_state(h, 0, xref.data(), thref.data(), nullptr, nullptr, nullptr, nullptr);
        ssme_lw_get_per_step(h, perref.data(), T);
        ssme_lw_destroy(h);
    }
    const auto t_end = std::chrono::steady_clock::now();
    auto differ = [](double a, double b) { uint64_t u, v; std::memcpy(&u, &a, 8); std::memcpy(&v, &b, 8); return u != v; };   // bits, not values
    size_t mism = 0, held = 0, aux_mism = 0, per_ranks = 0, per_ref = 0, sum_mism = 0;
    int compared = 0;                                  // ranks whose state and per-step values entered the counts below
    bool complete = true;                              // every rank ended with a state to compare
    int r0 = 0;                                        // the first rank that ended with values: what the other ranks' per-step values are compared with
    while (r0 < world - 1 && err_state[r0]) ++r0;
    for (int r = 0; r < world; ++r) {
        held += xs[r].size();
        const size_t n = xs[r].size();
        if (!err_state[r]) {
            sum_mism += differ(ll[r], ll_ref);
            for (size_t i = 0; i < n; ++i) mism += differ(xs[r][i], xref[first[r] + i]);
            if (model >= 0) for (size_t i = 0; i < n; ++i) aux_mism += cdfs[r][i] != cdfref[first[r] + i];
            else for (int d = 0; d < 4; ++d) for (size_t i = 0; i < n; ++i) aux_mism += differ(ths[r][d * n + i], thref[(size_t)d * N + first[r] + i]);
            for (int t = 0; t < T; ++t) per_ranks += differ(pers[r][t], pers[r0][t]);
            ++compared;
        } else complete = false;
    }
    if (complete) for (int t = 0; t < T; ++t) per_ref += differ(pers[0][t], perref[t]);
    if (held != (size_t)N) mism += 1;                  // the ranks' shares add up to the filter
    if (dump) {
        std::FILE* f = std::fopen(dump, "wb");
        if (!f) die("dump", 1, dump);
        const int64_t hdr[4] = {T, N, model < 0 ? 1 : 0, complete ? 1 : 0};
        std::fwrite("SSMEDMP1", 1, 8, f);
        std::fwrite(hdr, 8, 4, f);
        if (complete) {
            std::fwrite(pers[0].data(), 8, (size_t)T, f);
            for (int r = 0; r < world; ++r) std::fwrite(xs[r].data(), 8, xs[r].size(), f);
            if (model >= 0) for (int r = 0; r < world; ++r) std::fwrite(cdfs[r].data(), 8, cdfs[r].size(), f);
            else for (int d = 0; d < 4; ++d) for (int r = 0; r < world; ++r) std::fwrite(ths[r].data() + d * xs[r].size(), 8, xs[r].size(), f);
        }
        if (std::fclose(f)) die("dump close", 1, dump);
    }
    std::printf("ref %.17g\n", ll_ref);
    // any_left_halo: the reduced flag of the last fixed-halo pass (identical on every rank); own_left_halo: what this rank's own workgroups saw
    for (int r = 0; r < world; ++r) std::printf("rank %d ll %.17g path %d exchanged %lld any_left_halo %d own_left_halo %d\n", r, ll[r], path[r], exch[r], any_flag[r], own_flag[r]);
    // widest reach left / right of the rank's own tiles (ssme_*_shard_stats out4[2], out4[3]) beside the two flags above
    for (int r = 0; r < world; ++r) std::printf("stats %d any_left_halo %d own_left_halo %d reach_left %d reach_right %d\n", r, any_flag[r], own_flag[r], reach_l[r], reach_r[r]);
    for (int r = 0; r < world; ++r) std::printf("layout %d B %d Bl %d tiles %d particles %d\n", r, lays[r][0], lays[r][1], lays[r][2], lays[r][3]);
    for (int r = 0; r < world; ++r) std::printf("sum_hex %d %016llx\n", r, bits_of(ll[r]));
    std::printf("ref_hex %016llx\n", bits_of(ll_ref));
    for (int r = 0; r < world; ++r) std::printf("err_state %d %d\n", r, err_state[r]);
    std::printf("sum_mismatches %zu\n", sum_mism);
    std::printf("compared_ranks %d\n", compared);
    std::printf("per_step_mismatches_between_ranks %zu\n", per_ranks);
    std::printf("per_step_mismatches_vs_unsharded %zu\n", per_ref);
    std::printf("%s_mismatches %zu\n", model >= 0 ? "cdf" : "theta", aux_mism);
    std::printf("seconds sharded %.3f unsharded %.3f\n", std::chrono::duration<double>(t_sharded - t_start).count(),
                std::chrono::duration<double>(t_end - t_sharded).count());
    std::printf("particle_mismatches %zu\n", mism);
    if (model >= 0) for (int r = 0; r < world; ++r) if (err_state[r]) return 5;
    return 0;
}
