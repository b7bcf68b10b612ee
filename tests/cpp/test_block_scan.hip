// test_block_scan.hip -- block_scan_f64 (csrc/pf_kernels.h) against a verbatim copy of the form it replaced (a lane-shifted copy of the
// wave scan and two chains of additions per pair) and against a host prefix sum, bit for bit (u64), EVERY thread's incl and total, one
// workgroup per case (tests/test_block_scan_gpu.py).
//   usage: test_block_scan       prints one line per (case, NT, NK): "scan NAME nt NT nk NK values P mismatch A expect B" -- A values (incl of
//   every position and every thread's total) whose bits differ from the reference's, B whose bits differ from the host's sums; then
//   "done LINES".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ssme_amd/csrc/pf_kernels.h"

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)

namespace ref {
using namespace ssme;
// ---- verbatim: the functions as they were before the subtracting form ----
__device__ __forceinline__ double wave_shr1_f64(double v) { return dpp_f64_zero<0x138, 0xF>(v); }
template <int NT, int NK>
__device__ __forceinline__ void block_scan_f64(const double (&q)[NK][2], double (&incl)[NK][2], double& total, double* lds_seg) {
    constexpr int WPR = NT / 64, NSEG = NK * WPR;
    static_assert(NSEG <= 16, "segment totals are scanned inside one 16-lane row");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double s0[NK], s1[NK], exc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        s0[k] = q[k][0];
        s1[k] = s0[k] + q[k][1];
        const double inc = wave_incl_scan_f64(s1[k]);
        exc[k] = wave_shr1_f64(inc);
        if (lane == 63) lds_seg[k * WPR + wave] = inc;
    }
    __syncthreads();
    const double sv = row16_incl_scan((lane & 15) < NSEG ? lds_seg[lane & 15] : 0.0);
    total = readlane_f64(sv, 15);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int seg = k * WPR + wave;
        const double pre = seg ? readlane_f64(sv, seg - 1) : 0.0;
        const double base = pre + exc[k];
        incl[k][0] = base + s0[k];
        incl[k][1] = base + s1[k];
    }
}
// ---- end of the copy ----
}  // namespace ref

// v[P] -> out[P] = bits of incl at every position, out[P + tid] = bits of thread tid's total
template <int NT, int NK, bool REF>
__global__ __launch_bounds__(NT) void k_block_scan(const double* v, unsigned long long* out) {
    __shared__ double lds_seg[16];
    const int tid = threadIdx.x;
    double q[NK][2], incl[NK][2], total;
#pragma unroll
    for (int k = 0; k < NK; ++k) { q[k][0] = v[(k * NT + tid) * 2]; q[k][1] = v[(k * NT + tid) * 2 + 1]; }
    if (REF) ref::block_scan_f64<NT, NK>(q, incl, total, lds_seg);
    else ssme::block_scan_f64<NT, NK>(q, incl, total, lds_seg);
#pragma unroll
    for (int k = 0; k < NK; ++k) { out[(k * NT + tid) * 2] = ssme::d2bits(incl[k][0]); out[(k * NT + tid) * 2 + 1] = ssme::d2bits(incl[k][1]); }
    out[2 * NT * NK + tid] = ssme::d2bits(total);
}

static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Case { std::string name; std::vector<double> v; };

template <int NT, int NK>
static int run_scan(int& nlines) {
    constexpr int P = 2 * NT * NK;
    const double big = 2199023255552.0;   // 2^41: P <= 2048 of them sum to at most 2^52
    std::vector<Case> cases;
    auto add = [&](const std::string& name, double fill) -> Case& { cases.push_back(Case{name, std::vector<double>(P, fill)}); return cases.back(); };
    add("all-zero", 0.0);
    add("all-2p41", big);
    add("one-first", 0.0).v[0] = 12345.0;
    add("one-last", 0.0).v[P - 1] = big;
    add("one-wave-last", 0.0).v[127] = 7.0;                 // the second element of lane 63 of the first wave (pair 63)
    add("one-wave-first", 0.0).v[P > 128 ? 128 : 126] = 9.0;   // the first element of lane 0 of the second wave / segment (one-wave blocks: lane 63)
    { Case& c = add("random", 0.0); for (int i = 0; i < P; ++i) c.v[i] = (double)(rng() >> 23); }        // integers below 2^41
    { Case& c = add("random-sparse", 0.0); for (int i = 0; i < P; ++i) c.v[i] = (rng() & 3) ? 0.0 : (double)(rng() >> 23); }

    double* d_v = nullptr; unsigned long long *d_new = nullptr, *d_ref = nullptr;
    const size_t nout = (size_t)P + NT;
    CHECK(hipMalloc(&d_v, P * 8)); CHECK(hipMalloc(&d_new, nout * 8)); CHECK(hipMalloc(&d_ref, nout * 8));
    std::vector<unsigned long long> h_new(nout), h_ref(nout);
    for (const Case& c : cases) {
        CHECK(hipMemcpy(d_v, c.v.data(), P * 8, hipMemcpyHostToDevice));
        CHECK(hipMemset(d_new, 0x5a, nout * 8)); CHECK(hipMemset(d_ref, 0xa5, nout * 8));
        hipLaunchKernelGGL((k_block_scan<NT, NK, true>), dim3(1), dim3(NT), 0, 0, d_v, d_ref);
        CHECK(hipGetLastError());
        hipLaunchKernelGGL((k_block_scan<NT, NK, false>), dim3(1), dim3(NT), 0, 0, d_v, d_new);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(h_ref.data(), d_ref, nout * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h_new.data(), d_new, nout * 8, hipMemcpyDeviceToHost));
        long mismatch = 0, expect = 0;
        double run = 0.0;                  // exact: integers, every partial sum <= 2^52
        for (int i = 0; i < P; ++i) { run += c.v[i]; mismatch += h_new[i] != h_ref[i]; expect += h_new[i] != bits(run); }
        for (int t = 0; t < NT; ++t) { mismatch += h_new[P + t] != h_ref[P + t]; expect += h_new[P + t] != bits(run); }
        std::printf("scan %s nt %d nk %d values %zu mismatch %ld expect %ld\n", c.name.c_str(), NT, NK, nout, mismatch, expect);
        ++nlines;
    }
    hipFree(d_v); hipFree(d_new); hipFree(d_ref);
    return 0;
}

int main() {
    int nlines = 0, rc;
    if ((rc = run_scan<64, 1>(nlines)) || (rc = run_scan<64, 2>(nlines)) || (rc = run_scan<64, 4>(nlines))) return rc;
    if ((rc = run_scan<128, 1>(nlines)) || (rc = run_scan<128, 2>(nlines)) || (rc = run_scan<128, 4>(nlines))) return rc;
    if ((rc = run_scan<256, 1>(nlines)) || (rc = run_scan<256, 2>(nlines)) || (rc = run_scan<256, 4>(nlines))) return rc;
    if ((rc = run_scan<512, 1>(nlines)) || (rc = run_scan<512, 2>(nlines))) return rc;
    if ((rc = run_scan<1024, 1>(nlines))) return rc;

    std::printf("done %d\n", nlines);
    return 0;
}
