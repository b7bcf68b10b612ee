// test_block_max.hip -- block_max_nanprop / wave_max_f64 (csrc/pf_kernels.h) against a verbatim copy of the form they replaced
// (dmaxnum maxima, __syncthreads_or for the NaN flag), bit for bit (u64), EVERY thread's return value, one workgroup per case, for
// blocks of 64 .. 1024 threads (tests/test_block_max_gpu.py).
//   usage: test_block_max        prints one line per (case, NT): "case NAME nt NT threads N mismatch A expect B" -- A threads whose bits differ
//   from the reference's, B threads whose bits differ from what the host expects (dnan() exactly if any flag is set, else the maximum; the sign
//   of a zero maximum is the reference's), and for the loop case the same counts summed over its 256 iterations; then "done CASES".
//   The loop case calls the function 256 times in ONE launch on two alternating LDS buffers with inputs that change per iteration, the way
//   the step kernels reuse a buffer with one barrier in between: a missing barrier between the reads of call i and the writes of call i + 2
//   would show as a wrong maximum.  The loop is bounded; nothing waits for data.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ssme_amd/csrc/pf_kernels.h"

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)

namespace ref {
using namespace ssme;
// ---- verbatim: the functions as they were before the one-barrier form ----
__device__ __forceinline__ double wave_max_f64(double v) {
    v = dmaxnum(v, dpp_f64_perm<0xB1>(v));            // quad_perm [1,0,3,2]
    v = dmaxnum(v, dpp_f64_perm<0x4E>(v));            // quad_perm [2,3,0,1]
    v = dmaxnum(v, dpp_f64_perm<0x141>(v));           // row_half_mirror
    v = dmaxnum(v, dpp_f64_perm<0x140>(v));           // row_mirror: every lane of a row holds the row's maximum
    v = dmaxnum(v, dpp_f64_neginf<0x142, 0xA>(v));
    v = dmaxnum(v, dpp_f64_neginf<0x143, 0xC>(v));
    return bits2d(readlane_u64(d2bits(v), 63));
}

// Block max with NaN propagation: returns NaN if any thread passes nan = true.
// lds: NT/64 doubles, not reused by the caller before its next barrier.  One barrier.
template <int NT>
__device__ __forceinline__ double block_max_nanprop(double m, bool nan, double* lds) {
    m = wave_max_f64(m);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
    const int any_nan = __syncthreads_or(nan ? 1 : 0);
    double r = lds[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = dmaxnum(r, lds[w]);
    return any_nan ? dnan() : r;
}
// ---- end of the copy ----
}  // namespace ref

constexpr int kIters = 256;

// iters calls in one launch; call i takes m[i][NT], flag[i][NT] and LDS buffer i & 1; out[i][NT] = bits of every thread's result
template <int NT, bool REF>
__global__ __launch_bounds__(NT) void k_block_max(const double* m, const unsigned char* flag, unsigned long long* out, int iters) {
    __shared__ double lds[2][16];
    const int tid = threadIdx.x;
    for (int i = 0; i < iters; ++i) {
        const double v = m[(size_t)i * NT + tid];
        const bool f = flag[(size_t)i * NT + tid] != 0;
        const double r = REF ? ref::block_max_nanprop<NT>(v, f, lds[i & 1]) : ssme::block_max_nanprop<NT>(v, f, lds[i & 1]);
        out[(size_t)i * NT + tid] = ssme::d2bits(r);
    }
}

static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static double from_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }
static const uint64_t kNaNBits = 0x7ff8000000000000ull, kNegInf = 0xfff0000000000000ull;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double rnd_val() { return -60.0 * (double)(rng() >> 11) * 0x1.0p-53 - 700.0 * (double)((rng() & 7) == 0); }   // log-weight-like, some far down

struct Case { std::string name; std::vector<double> m; std::vector<unsigned char> f; };

template <int NT>
static int run_nt(int& ncases) {
    const double ninf = from_bits(kNegInf), pinf = from_bits(0x7ff0000000000000ull);
    const int spots[5] = {0, 63, NT > 64 ? 64 : 1, NT > 64 ? NT - 64 : NT - 2, NT - 1};
    std::vector<Case> cases;
    auto add = [&](const std::string& name, double fill) -> Case& { cases.push_back(Case{name, std::vector<double>(NT, fill), std::vector<unsigned char>(NT, 0)}); return cases.back(); };
    add("all-neginf", ninf);
    for (int s = 0; s < 5; ++s) add("single-finite-" + std::to_string(s), ninf).m[spots[s]] = -3.25 - s;
    { Case& c = add("posinf", -1.5); c.m[spots[3]] = pinf; }
    { Case& c = add("posinf-among-neginf", ninf); c.m[spots[1]] = pinf; }
    for (int s = 0; s < 5; ++s) { Case& c = add("single-flag-" + std::to_string(s), 0.0); for (int i = 0; i < NT; ++i) c.m[i] = rnd_val(); c.f[spots[s]] = 1; }
    { Case& c = add("flag-with-posinf", 2.0); c.m[spots[4]] = pinf; c.f[spots[2]] = 1; }
    { Case& c = add("all-flags", -2.0); for (int i = 0; i < NT; ++i) c.f[i] = 1; }
    { Case& c = add("all-flags-all-neginf", ninf); for (int i = 0; i < NT; ++i) c.f[i] = 1; }
    // signed zeros: in two waves (first / last wave, both orders), and in adjacent lanes of one wave (both orders); everything else below zero
    if (NT > 64) {
        { Case& c = add("zeros-two-waves-neg-first", -1.0); c.m[5] = -0.0; c.m[NT - 7] = 0.0; }
        { Case& c = add("zeros-two-waves-pos-first", -1.0); c.m[5] = 0.0; c.m[NT - 7] = -0.0; }
        { Case& c = add("zeros-two-waves-mid", ninf); c.m[64] = -0.0; c.m[130 < NT ? 130 : 127] = 0.0; }
    }
    { Case& c = add("zeros-one-wave-neg-first", -1.0); c.m[NT - 30] = -0.0; c.m[NT - 29] = 0.0; }
    { Case& c = add("zeros-one-wave-pos-first", -1.0); c.m[NT - 30] = 0.0; c.m[NT - 29] = -0.0; }
    { Case& c = add("zeros-row-edge", ninf); c.m[15] = -0.0; c.m[16] = 0.0; }
    { Case& c = add("zeros-row-edge-rev", ninf); c.m[15] = 0.0; c.m[16] = -0.0; }
    { Case& c = add("negzero-only", ninf); c.m[spots[3]] = -0.0; }
    { Case& c = add("all-negzero", -0.0); (void)c; }
    // denormals: positive and negative, largest and smallest, alone above -inf and among normals
    { Case& c = add("denormals", ninf); for (int i = 0; i < NT; ++i) c.m[i] = from_bits((uint64_t)(i + 1) * 0x0000000100000001ull); }
    { Case& c = add("denormal-max-in-normals", -1e-300); c.m[spots[1]] = from_bits(1ull); c.m[spots[3]] = -from_bits(1ull); }
    { Case& c = add("negative-denormals", ninf); for (int i = 0; i < NT; ++i) c.m[i] = -from_bits((uint64_t)(i + 3)); }
    { Case& c = add("random", 0.0); for (int i = 0; i < NT; ++i) c.m[i] = rnd_val(); }
    { Case& c = add("random-flags-1pct", 0.0); for (int i = 0; i < NT; ++i) { c.m[i] = rnd_val(); c.f[i] = (rng() % 100) == 0; } c.f[(int)(rng() % NT)] = 1; }
    // the loop: 256 calls, inputs per iteration; about a third of the iterations carry one flag, some are all -inf, some hold signed zeros
    Case loop{"loop-256", std::vector<double>((size_t)kIters * NT), std::vector<unsigned char>((size_t)kIters * NT, 0)};
    for (int it = 0; it < kIters; ++it) {
        const int kind = (int)(rng() % 8);
        for (int i = 0; i < NT; ++i) loop.m[(size_t)it * NT + i] = kind == 7 ? ninf : rnd_val();
        if (kind == 6) { loop.m[(size_t)it * NT + (int)(rng() % NT)] = 0.0; loop.m[(size_t)it * NT + (int)(rng() % NT)] = -0.0; }
        if (kind < 3) loop.f[(size_t)it * NT + (int)(rng() % NT)] = 1;
    }

    double* d_m = nullptr; unsigned char* d_f = nullptr; unsigned long long *d_new = nullptr, *d_ref = nullptr;
    const size_t cap = (size_t)kIters * NT;
    CHECK(hipMalloc(&d_m, cap * 8)); CHECK(hipMalloc(&d_f, cap)); CHECK(hipMalloc(&d_new, cap * 8)); CHECK(hipMalloc(&d_ref, cap * 8));
    std::vector<unsigned long long> h_new(cap), h_ref(cap);
    cases.push_back(loop);
    for (const Case& c : cases) {
        const int iters = (int)(c.m.size() / NT);
        const size_t n = c.m.size();
        CHECK(hipMemcpy(d_m, c.m.data(), n * 8, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_f, c.f.data(), n, hipMemcpyHostToDevice));
        CHECK(hipMemset(d_new, 0x5a, n * 8)); CHECK(hipMemset(d_ref, 0xa5, n * 8));
        hipLaunchKernelGGL((k_block_max<NT, true>), dim3(1), dim3(NT), 0, 0, d_m, d_f, d_ref, iters);
        CHECK(hipGetLastError());
        hipLaunchKernelGGL((k_block_max<NT, false>), dim3(1), dim3(NT), 0, 0, d_m, d_f, d_new, iters);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(h_ref.data(), d_ref, n * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h_new.data(), d_new, n * 8, hipMemcpyDeviceToHost));
        long mismatch = 0, expect = 0;
        for (int it = 0; it < iters; ++it) {
            bool any = false;
            double mx = ninf;
            for (int i = 0; i < NT; ++i) { any = any || c.f[(size_t)it * NT + i]; const double v = c.m[(size_t)it * NT + i]; mx = v > mx ? v : mx; }
            for (int i = 0; i < NT; ++i) {
                const uint64_t bn = h_new[(size_t)it * NT + i], br = h_ref[(size_t)it * NT + i];
                mismatch += bn != br;
                if (any) expect += bn != kNaNBits;
                else expect += !(from_bits(bn) == mx) || (mx != 0.0 && bn != bits(mx));     // (+0 == -0: the sign of a zero maximum is held to the reference above)
            }
        }
        std::printf("case %s nt %d threads %zu mismatch %ld expect %ld\n", c.name.c_str(), NT, n, mismatch, expect);
        ++ncases;
    }
    hipFree(d_m); hipFree(d_f); hipFree(d_new); hipFree(d_ref);
    return 0;
}

int main() {
    int ncases = 0, rc;
    if ((rc = run_nt<64>(ncases))) return rc;
    if ((rc = run_nt<128>(ncases))) return rc;
    if ((rc = run_nt<256>(ncases))) return rc;
    if ((rc = run_nt<512>(ncases))) return rc;
    if ((rc = run_nt<1024>(ncases))) return rc;
    std::printf("done %d\n", ncases);
    return 0;
}
