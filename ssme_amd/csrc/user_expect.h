// user_expect.h -- weighted expectations of the functionals a USER model declares (model_api.h: n_h, h), on the device.
//
// The reference's callers hand filter(y[, z], fs) a vector of functions h and read getExpectations() (pswarm_filter.h:87-89,
// 383-385).  For the built-in functionals k_expect_partials / k_expect_final (pf_kernels.h) do that; a user model's own functions
// are compiled in here, as its callbacks are compiled into the step kernel.  Weights are the fixed-point weights of the resampler:
// w_j = q_j exp(m_tile - m), q_j = cdf_j - cdf_{j-1} (tile-local, integer valued), so sum_j q_j of a tile is its exact tile sum A_b.
//   k_user_expect_partials  grid (B tiles, R), 256 threads: per tile sum_j h_k(x_j) q_j for ALL n_h outputs in one pass; the dim_x
//                           planes and the cdf are read once, two neighbouring particles (16 bytes) per lane and access
//   k_user_expect_partials_row  the same with the covariates read from a row of the series' covariates on the device (recorded series)
//   k_user_expect_final     grid (R), 256 threads: E_k = sum_b num_{b,k} e^{m_b - m} / sum_b A_b e^{m_b - m}; m NaN => NaN
// The swarm means over the R members come from k_swarm_means (pf_kernels.h), whose row count is a launch argument.
//
// SUMMATION TREES (fixed: a result depends on the particles and weights alone -- not on the run, not on the threads-per-tile setting
// of the step kernel, which these kernels do not read, and not on how a bank is split over handles, since a workgroup sees one filter):
//   partials: thread t adds, in this order, particles 2t, 2t+1, 2t+512, 2t+513, 2t+1024, ... of the tile (valid ones only);
//             the 64 lanes of a wave are combined by the xor butterfly 32, 16, 8, 4, 2, 1; the 4 waves as ((w0 + w1) + w2) + w3.
//   final:    thread t adds tiles t, t+256, t+512, ... in this order; lanes and waves are combined as above.
#pragma once
#include "pf_kernels.h"

namespace ssme {

template <class M>
__device__ __forceinline__ void user_expect_partials_tile(const double* x, size_t xplane, const double* cdf, const ModelConst* mcs,
                                                          double zcov, const CovVals<user_cov<M>::k>& zc /*dim_cov headers*/,
                                                          int N, int Npad, int Bs, int tile,
                                                          double* part /*[R][Bs][n_h]*/) {
    constexpr int NH = user_nh<M>::n, DX = user_dims<M>::dx, KC = user_cov<M>::k;
    __shared__ ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    __shared__ double lds[NH][4];
    const int tid = threadIdx.x, b = blockIdx.x, r = blockIdx.y;
    load_exp_table<kThreads>(lds_etab);
    __syncthreads();
    const ModelConst mc = mcs[r];
    // every tile is a multiple of 512 particles and the planes are padded to whole tiles: the 16-byte accesses below are aligned
    // and stay inside the filter's row even in the ragged last tile (what lies beyond nvalid is loaded, never used)
    const size_t base = (size_t)r * Npad + (size_t)b * tile;
    const double* cr = cdf + base;
    const int nvalid = (N - b * tile) < tile ? (N - b * tile) : tile;
    double num[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) num[k] = 0.0;
    for (int j0 = 0; j0 < nvalid; j0 += 2 * kThreads) {                    // uniform trip count: the shuffle below needs whole waves
        const int j = j0 + 2 * tid;
        const double2 c = *reinterpret_cast<const double2*>(cr + j);
        double2 xv[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) xv[d] = *reinterpret_cast<const double2*>(x + (size_t)d * xplane + base + j);
        double prev = __shfl_up(c.y, 1, kWave);                            // cdf_{j-1}: the lane below holds it
        if ((tid & 63) == 0) prev = j ? cr[j - 1] : 0.0;
        const double q0 = c.x - prev, q1 = c.y - c.x;
        double xs[DX], hv[NH];
        if (j < nvalid) {
#pragma unroll
            for (int d = 0; d < DX; ++d) xs[d] = xv[d].x;
            if constexpr (KC > 0) M::h(mc, xs, zc.v, lds_etab, hv);
            else M::h(mc, xs, zcov, lds_etab, hv);
#pragma unroll
            for (int k = 0; k < NH; ++k) num[k] = num[k] + hv[k] * q0;
        }
        if (j + 1 < nvalid) {
#pragma unroll
            for (int d = 0; d < DX; ++d) xs[d] = xv[d].y;
            if constexpr (KC > 0) M::h(mc, xs, zc.v, lds_etab, hv);
            else M::h(mc, xs, zcov, lds_etab, hv);
#pragma unroll
            for (int k = 0; k < NH; ++k) num[k] = num[k] + hv[k] * q1;
        }
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        num[k] = wave_sum_xor(num[k]);
        if ((tid & 63) == 0) lds[k][tid >> 6] = num[k];
    }
    __syncthreads();
    if (tid < NH) part[((size_t)r * Bs + b) * NH + tid] = ((lds[tid][0] + lds[tid][1]) + lds[tid][2]) + lds[tid][3];
}

template <class M>
__global__ __launch_bounds__(kThreads) void k_user_expect_partials(const double* x, size_t xplane, const double* cdf, const ModelConst* mcs,
                                                                   double zcov, const CovVals<user_cov<M>::k> zc /*dim_cov headers*/,
                                                                   int N, int Npad, int Bs, int tile,
                                                                   double* part /*[R][Bs][n_h]*/) {
    user_expect_partials_tile<M>(x, xplane, cdf, mcs, zcov, zc, N, Npad, Bs, tile, part);
}

// The same for step `row` of a recorded series (ssme_pf_set_series_expectations): the covariates are READ from row `row` of the series'
// uploaded covariates z ([T][max(dim_cov, 1)]; null: zeros), not passed by value -- a captured graph is replayed for later series, whose
// covariates differ, and a value baked into the launch would be those of the series that was captured.
template <class M>
__global__ __launch_bounds__(kThreads) void k_user_expect_partials_row(const double* x, size_t xplane, const double* cdf, const ModelConst* mcs,
                                                                       const double* z, int row, int N, int Npad, int Bs, int tile,
                                                                       double* part /*[R][Bs][n_h]*/) {
    constexpr int KC = user_cov<M>::k;
    double zcov = 0.0;
    CovVals<KC> zc;
#pragma unroll
    for (int j = 0; j < (KC > 0 ? KC : 1); ++j) zc.v[j] = 0.0;
    if (z) {
        if constexpr (KC > 0) zc.load(z, (size_t)row);
        else zcov = z[row];
    }
    user_expect_partials_tile<M>(x, xplane, cdf, mcs, zcov, zc, N, Npad, Bs, tile, part);
}

template <int NH>
__global__ __launch_bounds__(kThreads) void k_user_expect_final(const double* part, const double* tsum, const double* tmax, int B, int Bs,
                                                                int R, double* out /*[n_h][R]*/) {
    __shared__ double lds[NH + 1][4];
    __shared__ double lds_m[16];
    const int tid = threadIdx.x, r = blockIdx.x;
    double mx = -dinf();
    bool nan = false;
    for (int j = tid; j < B; j += kThreads) { const double v = tmax[(size_t)r * Bs + j]; nan = nan || (v != v); mx = (v > mx) ? v : mx; }
    const double m = block_max_nanprop<kThreads>(mx, nan, lds_m);
    double acc[NH + 1];
#pragma unroll
    for (int k = 0; k <= NH; ++k) acc[k] = 0.0;
    for (int j = tid; j < B; j += kThreads) {
        const double sc = dexp(tmax[(size_t)r * Bs + j] - m);
#pragma unroll
        for (int k = 0; k < NH; ++k) acc[k] = acc[k] + part[((size_t)r * Bs + j) * NH + k] * sc;
        acc[NH] = acc[NH] + tsum[(size_t)r * Bs + j] * sc;
    }
#pragma unroll
    for (int k = 0; k <= NH; ++k) {
        acc[k] = wave_sum_xor(acc[k]);
        if ((tid & 63) == 0) lds[k][tid >> 6] = acc[k];
    }
    __syncthreads();
    if (tid < NH) {
        const double n4 = ((lds[tid][0] + lds[tid][1]) + lds[tid][2]) + lds[tid][3];
        const double d4 = ((lds[NH][0] + lds[NH][1]) + lds[NH][2]) + lds[NH][3];
        out[(size_t)tid * R + r] = (m != m) ? dnan() : n4 / d4;
    }
}

}  // namespace ssme
