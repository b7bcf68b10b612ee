// test_window_check.hip -- k_shard_window_check (csrc/shard_driver.h) on its own: the decision "a rank's window left the fixed halo" and the
// widest reach it records, for windows given by hand.  On the drivers' split level-2 path k_filter_step repeats the comparison for its own
// tiles and raises the same flag, so only a direct launch shows what THIS kernel decides (tests/test_shard_edges_gpu.py:
// test_window_check_kernel_decides_at_the_margin).
//   usage: test_window_check CASES.txt     one case per line: WORLD BL B MARGIN then LO HI for every rank (valid layouts: (WORLD-1) BL < B,
//   0 <= LO <= HI < B).  Prints per case "case I form F flag X left L right R": F = 0 the [world][2] plan (k_shard_plan's output), F = 1
//   the per-tile tables of k_level2_plan, where every other entry says "my own tile" and only a rank's first lo and last hi carry the window.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../ssme_amd/csrc/shard_driver.h"

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    int32_t *d_plan = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_flag = nullptr;
    const int kMaxB = 8192;
    CHECK(hipMalloc(&d_plan, sizeof(int32_t) * 128));
    CHECK(hipMalloc(&d_lo, sizeof(int32_t) * kMaxB));
    CHECK(hipMalloc(&d_hi, sizeof(int32_t) * kMaxB));
    CHECK(hipMalloc(&d_flag, sizeof(int32_t) * 4));
    for (int i = 0; std::getline(f, line); ++i) {
        std::istringstream in(line);
        int world, Bl, B, margin;
        if (!(in >> world >> Bl >> B >> margin)) continue;
        if (world < 1 || world > 64 || Bl < 1 || B < 1 || B > kMaxB || (world - 1) * Bl >= B) { std::fprintf(stderr, "bad layout in case %d\n", i); return 2; }
        std::vector<int32_t> plan(2 * (size_t)world), lo((size_t)B), hi((size_t)B);
        for (int j = 0; j < B; ++j) { lo[j] = j; hi[j] = j; }
        for (int g = 0; g < world; ++g) {
            int l, h;
            if (!(in >> l >> h) || l < 0 || h < l || h >= B) { std::fprintf(stderr, "bad window in case %d\n", i); return 2; }
            plan[2 * g] = l; plan[2 * g + 1] = h;
            const int last = (g + 1) * Bl - 1 < B - 1 ? (g + 1) * Bl - 1 : B - 1;
            lo[(size_t)g * Bl] = l; hi[(size_t)last] = h;
        }
        CHECK(hipMemcpy(d_plan, plan.data(), sizeof(int32_t) * plan.size(), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_lo, lo.data(), sizeof(int32_t) * lo.size(), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_hi, hi.data(), sizeof(int32_t) * hi.size(), hipMemcpyHostToDevice));
        for (int form = 0; form < 2; ++form) {
            int32_t out[4] = {0, 0, 0, 0};
            CHECK(hipMemset(d_flag, 0, sizeof(int32_t) * 4));
            hipLaunchKernelGGL(ssme::k_shard_window_check, dim3(1), dim3(64), 0, 0, form == 0 ? (const int32_t*)d_plan : (const int32_t*)nullptr,
                               (const int32_t*)d_lo, (const int32_t*)d_hi, world, Bl, B, margin, d_flag, d_flag + 1);
            CHECK(hipGetLastError());
            CHECK(hipMemcpy(out, d_flag, sizeof(out), hipMemcpyDeviceToHost));
            std::printf("case %d form %d flag %d left %d right %d\n", i, form, out[0], out[1], out[2]);
        }
    }
    hipFree(d_plan); hipFree(d_lo); hipFree(d_hi); hipFree(d_flag);
    return 0;
}
