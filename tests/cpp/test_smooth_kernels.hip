// test_smooth_kernels.hip -- the smoothing kernels (csrc/smooth.h) on their own, on histories written by hand: no filter runs, every
// buffer of SmArgs comes from the case file (tests/smooth_kernel_cases.py writes it and holds the reference; all comparisons happen in
// tests/test_smooth_kernels_gpu.py).  Per case: k_sm_trajectories<dx> with given terminals, k_sm_sweep<tile / 256> and k_sm_final, and
// as the anchor k_expect_partials / k_expect_final per step t on a plain array xg[t] (the host's gather x_t[B_t(j)]) with the same
// cdf, tile sums and maxima -- smooth.h's header claims rows of the sweep equal those to the bit.
//   usage: test_smooth_kernels CASES.bin OUT.bin
//   CASES.bin: "SSMESMK1", int64 ncases; per case int32 hdr[16] = N tile B Bs R T sched dx K nf id0 id1 id2 id3 0 0, then raw arrays
//     hx f64[T dx R Npad], hanc u32[T R Npad], cdf f64[R Npad], tsum f64[R Bs], tmax f64[R Bs], S f64[R], terminal u32[R K],
//     xg f64[T R Npad]                                                                                         (Npad = B tile)
//   OUT.bin:   "SSMESMO1", int64 ncases; per case int64 index, then x_out f64[R K T dx], idx_out u32[R K T], part f64[T R Bs 4],
//     out f64[T nf R], apart f64[T R Bs 4], aout f64[T nf R].  Every output buffer starts as bytes 0xFF (a NaN / 0xFFFFFFFF no kernel
//     writes), so a slot a kernel skipped is visible.  Prints "case I done" per case and "all N done" at the end.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ssme_amd/csrc/smooth.h"

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <class T>
static bool wr(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n = 0;
    ~Dev() { if (p) (void)hipFree(p); }
    hipError_t up(const std::vector<T>& v) {
        n = v.size();
        hipError_t e = hipMalloc(&p, sizeof(T) * (n ? n : 1));
        return (e != hipSuccess || !n) ? e : hipMemcpy(p, v.data(), sizeof(T) * n, hipMemcpyHostToDevice);
    }
    hipError_t blank(size_t count) {
        n = count;
        hipError_t e = hipMalloc(&p, sizeof(T) * (n ? n : 1));
        return (e != hipSuccess || !n) ? e : hipMemset(p, 0xFF, sizeof(T) * n);
    }
    hipError_t down(std::vector<T>& v) const { v.resize(n); return n ? hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost) : hipSuccess; }
};

int main(int argc, char** argv) {
    using namespace ssme;
    if (argc < 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* outf = std::fopen(argv[2], "wb");
    if (!in || !outf) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    char magic[8];
    int64_t ncases = 0;
    if (std::fread(magic, 1, 8, in) != 8 || std::memcmp(magic, "SSMESMK1", 8) != 0 || std::fread(&ncases, 8, 1, in) != 1) return 2;
    std::fwrite("SSMESMO1", 1, 8, outf);
    std::fwrite(&ncases, 8, 1, outf);
    for (int64_t i = 0; i < ncases; ++i) {
        int32_t hd[16];
        if (std::fread(hd, 4, 16, in) != 16) { std::fprintf(stderr, "case %lld: short header\n", (long long)i); return 2; }
        const int N = hd[0], tile = hd[1], B = hd[2], Bs = hd[3], R = hd[4], T = hd[5], sched = hd[6], dx = hd[7], K = hd[8], nf = hd[9];
        // the layout the kernels index by: refuse anything they could leave a buffer with
        const bool ok = (tile == 512 || tile == 1024 || tile == 2048) && N >= 1 && B >= 1 && B <= 8 && (B - 1) * tile < N && N <= B * tile &&
                        Bs >= B && Bs <= 16 && R >= 1 && R <= 8 && T >= 1 && T <= 64 && sched >= 1 && dx >= 1 && dx <= 4 && K >= 1 && K <= N &&
                        nf >= 1 && nf <= kMaxFunctionals;
        if (!ok) { std::fprintf(stderr, "case %lld: bad shape\n", (long long)i); return 2; }
        FunctionalIds fs{};
        fs.n = nf;
        for (int f = 0; f < kMaxFunctionals; ++f) {
            fs.id[f] = hd[10 + f];
            if (fs.id[f] < 0 || fs.id[f] > 3) { std::fprintf(stderr, "case %lld: bad functional\n", (long long)i); return 2; }
        }
        const size_t Npad = (size_t)B * tile, row = (size_t)R * Npad;
        std::vector<double> hx, cdf, tsum, tmax, S, xg;
        std::vector<uint32_t> hanc, term;
        if (!rd(in, hx, (size_t)T * dx * row) || !rd(in, hanc, (size_t)T * row) || !rd(in, cdf, row) || !rd(in, tsum, (size_t)R * Bs) ||
            !rd(in, tmax, (size_t)R * Bs) || !rd(in, S, (size_t)R) || !rd(in, term, (size_t)R * K) || !rd(in, xg, (size_t)T * row)) {
            std::fprintf(stderr, "case %lld: short arrays\n", (long long)i);
            return 2;
        }
        for (uint32_t v : term)
            if (v >= (uint32_t)N) { std::fprintf(stderr, "case %lld: terminal out of range\n", (long long)i); return 2; }   // the API refuses these
        std::vector<FilterScalars> scal((size_t)R);
        std::memset(scal.data(), 0, sizeof(FilterScalars) * scal.size());
        for (int r = 0; r < R; ++r) scal[(size_t)r].S = S[(size_t)r];

        Dev<double> d_hx, d_cdf, d_tsum, d_tmax, d_xg, d_x, d_part, d_out, d_apart, d_aout;
        Dev<uint32_t> d_hanc, d_term, d_idx;
        Dev<FilterScalars> d_scal;
        CHECK(d_hx.up(hx)); CHECK(d_hanc.up(hanc)); CHECK(d_cdf.up(cdf)); CHECK(d_tsum.up(tsum)); CHECK(d_tmax.up(tmax));
        CHECK(d_xg.up(xg)); CHECK(d_term.up(term)); CHECK(d_scal.up(scal));
        const size_t npart = (size_t)T * R * Bs * kMaxFunctionals, nout = (size_t)T * nf * R;
        CHECK(d_x.blank((size_t)R * K * T * dx)); CHECK(d_idx.blank((size_t)R * K * T));
        CHECK(d_part.blank(npart)); CHECK(d_out.blank(nout)); CHECK(d_apart.blank(npart)); CHECK(d_aout.blank(nout));

        SmArgs a{};
        a.hx = d_hx.p; a.hanc = d_hanc.p; a.cdf = d_cdf.p; a.l2_T = nullptr; a.l2_R = nullptr; a.scal = d_scal.p; a.keyp = nullptr;
        a.first_filter = 0; a.N = N; a.Npad = (int32_t)Npad; a.B = B; a.Bs = Bs; a.Bpow2 = 1; while (a.Bpow2 < B) a.Bpow2 *= 2;
        a.tile = tile; a.R = R; a.T = T; a.resamp_sched = sched; a.dx = dx;

        const dim3 gt((unsigned)((K + kSmChains * kThreads - 1) / (kSmChains * kThreads)), (unsigned)R), blk(kThreads);
        const uint32_t* tp = d_term.p;
        if (dx == 1) hipLaunchKernelGGL((k_sm_trajectories<1>), gt, blk, 0, 0, a, K, tp, d_x.p, d_idx.p);
        else if (dx == 2) hipLaunchKernelGGL((k_sm_trajectories<2>), gt, blk, 0, 0, a, K, tp, d_x.p, d_idx.p);
        else if (dx == 3) hipLaunchKernelGGL((k_sm_trajectories<3>), gt, blk, 0, 0, a, K, tp, d_x.p, d_idx.p);
        else hipLaunchKernelGGL((k_sm_trajectories<4>), gt, blk, 0, 0, a, K, tp, d_x.p, d_idx.p);
        CHECK(hipGetLastError());

        const dim3 gs((unsigned)B, (unsigned)R);
        if (tile == 512) hipLaunchKernelGGL((k_sm_sweep<2>), gs, blk, 0, 0, a, fs, d_part.p);
        else if (tile == 1024) hipLaunchKernelGGL((k_sm_sweep<4>), gs, blk, 0, 0, a, fs, d_part.p);
        else hipLaunchKernelGGL((k_sm_sweep<8>), gs, blk, 0, 0, a, fs, d_part.p);
        CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_sm_final, dim3((unsigned)(T * R)), blk, 0, 0, (const double*)d_part.p, (const double*)d_tsum.p, (const double*)d_tmax.p, B, Bs, R,
                           fs, d_out.p);
        CHECK(hipGetLastError());

        for (int t = 0; t < T; ++t) {
            double* pt = d_apart.p + (size_t)t * R * Bs * kMaxFunctionals;
            hipLaunchKernelGGL(k_expect_partials, gs, blk, 0, 0, (const double*)(d_xg.p + (size_t)t * row), (const double*)d_cdf.p, N, (int)Npad, Bs, tile,
                               fs, pt);
            hipLaunchKernelGGL(k_expect_final, dim3((unsigned)R), blk, 0, 0, (const double*)pt, (const double*)d_tsum.p, (const double*)d_tmax.p, B, Bs, R,
                               fs, d_aout.p + (size_t)t * nf * R);
        }
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());

        std::vector<double> x, part, out, apart, aout;
        std::vector<uint32_t> idx;
        CHECK(d_x.down(x)); CHECK(d_idx.down(idx)); CHECK(d_part.down(part)); CHECK(d_out.down(out)); CHECK(d_apart.down(apart)); CHECK(d_aout.down(aout));
        if (std::fwrite(&i, 8, 1, outf) != 1 || !wr(outf, x) || !wr(outf, idx) || !wr(outf, part) || !wr(outf, out) || !wr(outf, apart) || !wr(outf, aout)) {
            std::fprintf(stderr, "case %lld: write failed\n", (long long)i);
            return 4;
        }
        std::printf("case %lld done\n", (long long)i);
    }
    std::fclose(in);
    if (std::fclose(outf) != 0) return 4;
    std::printf("all %lld done\n", (long long)ncases);
    return 0;
}
