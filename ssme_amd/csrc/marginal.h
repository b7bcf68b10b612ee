// marginal.h -- marginal smoothing weights of a recorded series (forward filtering, backward smoothing: Doucet, Godsill and Andrieu
// 2000), gfx950.
//
// backward.h draws B_t given B_{t+1} = j from the quantised weights q_ij / D_j.  Here the EXPECTATION of those draws is formed: a
// weight per particle of every step,
//     om_{T-1}[j] = w_j  (the final weights of ssme_pf_download_weights; zeros for a filter without final weight),
//     om_t[i] = sum_{j live} c_j q_ij  +  sum_{j degenerate, g(j) = i} om_{t+1}[j],          c_j = om_{t+1}[j] / D_j,
//               summed over j in a fixed order: see k_msm_rows,
//     a_ij = lw_t[i] + logf(x_{t+1}[j] | x_t[i], z_{t+1})  (NaN counts as -inf),  m_j = max_i a_ij,
//     q_ij = rint(exp_t(a_ij - m_j) 2^sh),  D_j = sum_i q_ij  (an exact integer < 2^53: any order gives the same bits),
//     column j is live when m_j is finite and D_j > 0, degenerate otherwise: its mass goes to its genealogical parent
//     g(j) = min(anc_{t+1}[j], N - 1) where step t + 1 resampled, j otherwise
// -- the law of B_t under k_bsim's draw, to the bit, when B_{T-1} is drawn from the final weights.  The N x N matrix is never stored:
// every a_ij is computed three times (maximum, integer sum, propagation), as k_bsim recomputes its candidates above one chunk.
//
//   k_msm_start             row T - 1: k_weights' arithmetic per filter.
//   k_msm_columns<MODEL,NJ> m_j and D_j of EVERY step in one launch (they do not depend on om): a thread keeps x_{t+1}[j] of its NJ
//                           columns in registers and sweeps i twice over chunks of kMsmChunk rows (x_t[i], lw_t[i]) staged in LDS, which
//                           all lanes read at one address (a broadcast).  D = 0 marks a degenerate column.
//   k_msm_rows<MODEL>       om_t from om_{t+1}, one launch per step.  A workgroup owns 64 rows, one per lane (x_t[i], lw_t[i] in registers),
//                           and has kMsmSeg waves: wave s walks the chunks s, s + kMsmSeg, .. of 64 columns, staged in its own LDS
//                           (x_{t+1}[j], m_j, c_j -- the lane that stages j does the one division -- and g(j) of a degenerate column),
//                           each in ascending j; wave 0 then adds the kMsmSeg partial sums in ascending s.  That order is FIXED: it does
//                           not depend on the grid, the shape of the bank or the route.  A step is parallel in i only through N R / 64
//                           workgroups, which leaves this machine idle at the bank shapes; the segments are what fills it.
//   k_msm_expect            one workgroup per (t, r): sum_j h_f(x_t[j]) om_t[j] and sum_j om_t[j] by expect_add / expect_wave_sums
//                           (thread-strided, wave xor tree, waves in order), one division at the end.
// No floating-point atomics; two passes over one history give the same bits.
#pragma once
#include "backward.h"

namespace ssme {

constexpr int kMsmChunk = kThreads;        // rows k_msm_columns stages in LDS at a time: one per thread
#ifndef SSME_MSM_SEG               // builds with another value are for timing only (profiles/marginal_smoothing_timing.txt): it is part of
#define SSME_MSM_SEG 8             // the summation order, so the last bits of the rows change with it
#endif
constexpr int kMsmSeg = SSME_MSM_SEG;      // waves of a workgroup of k_msm_rows: the interleaved segments the columns of a row sum are split into

struct MsmArgs {
    BsimArgs b;                // the history in force, its log-weight rows, series, covariates, model constants and sh
    double* om;                // [T][R][Npad] the weight rows
    double* cm;                // [T][R][Npad] m_j of the columns j of step t + 1 (row T - 1 is not used)
    double* cD;                // [T][R][Npad] D_j, 0 for a degenerate column
};

// grid = (B tiles, R), block = kThreads: om_{T-1} of filter r, k_weights' operations; zeros where S' is not > 0.
__global__ __launch_bounds__(kThreads) void k_msm_start(const MsmArgs a, const double* tmax /*[R][Bs]*/) {
    __shared__ double lds_m[16];
    const SmArgs& s = a.b.s;
    const int tid = threadIdx.x, b = blockIdx.x, r = blockIdx.y;
    const double* tm = tmax + (size_t)r * s.Bs;
    double mx = -dinf();
    bool nan = false;
    for (int j = tid; j < s.B; j += kThreads) { const double v = tm[j]; nan = nan || (v != v); mx = (v > mx) ? v : mx; }
    const double m = block_max_nanprop<kThreads>(mx, nan, lds_m);
    const double sc = (m != m) ? dnan() : dexp_scaled(tm[b] - m, -kTileShift);
    const bool alive = s.scal[r].S > 0.0;
    const double* cr = s.cdf + (size_t)r * s.Npad + (size_t)b * s.tile;
    double* out = a.om + ((size_t)(s.T - 1) * s.R + r) * s.Npad + (size_t)b * s.tile;
    for (int j = tid; j < s.tile; j += kThreads)
        if (b * s.tile + j < s.N) out[j] = alive ? (cr[j] - (j ? cr[j - 1] : 0.0)) * sc : 0.0;
}

// One sweep of k_msm_columns over all rows i of step t.  SUM false: m[e] = max_i a_ie; true: D[e] = sum_i q_ie given m.
template <int MODEL, int NJ, bool SUM>
__device__ __forceinline__ void msm_column_sweep(const MsmArgs& a, const ModelConst& mc, const double* xt, const double* lwt, size_t plane,
                                                 const double (&xs)[NJ][model_dx<MODEL>()], double zcov, const CovVals<model_kcov<MODEL>()>& zc,
                                                 const ExpTabEntry* etab, double (*lds_x)[kMsmChunk], double* lds_lw, double (&m)[NJ],
                                                 double (&D)[NJ]) {
    constexpr int DX = model_dx<MODEL>();
    const int N = a.b.s.N, tid = threadIdx.x;
    for (int i0 = 0; i0 < N; i0 += kMsmChunk) {
        __syncthreads();                                   // the chunk before this one is consumed (first: the exp table is loaded)
        {
            const int i = i0 + tid;
            lds_lw[tid] = i < N ? lwt[i] : -dinf();
#pragma unroll
            for (int d = 0; d < DX; ++d) lds_x[d][tid] = i < N ? xt[(size_t)d * plane + i] : 0.0;
        }
        __syncthreads();
        const int n = N - i0 < kMsmChunk ? N - i0 : kMsmChunk;
        for (int k = 0; k < n; ++k) {
            double xi[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) xi[d] = lds_x[d][k];
            const double lw = lds_lw[k];
#pragma unroll
            for (int e = 0; e < NJ; ++e) {
                double v = lw + bsim_logf<MODEL>(mc, xs[e], xi, zcov, zc, etab);
                v = (v != v) ? -dinf() : v;
                if constexpr (SUM) D[e] = D[e] + __builtin_rint(dexp_scaled_t(v - m[e], a.b.shift, etab));
                else m[e] = v > m[e] ? v : m[e];
            }
        }
    }
}

// grid = (ceil(N / (kThreads NJ)), steps, R), block = kThreads: block (., y, r) forms the columns of step t + 1 for t = t0 + y.
template <int MODEL, int NJ>
__global__ __launch_bounds__(kThreads) void k_msm_columns(const MsmArgs a, const int t0) {
    constexpr int DX = model_dx<MODEL>(), KC = model_kcov<MODEL>();
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    __shared__ double lds_x[DX][kMsmChunk], lds_lw[kMsmChunk];
    const SmArgs& s = a.b.s;
    const int tid = threadIdx.x, t = t0 + (int)blockIdx.y, r = blockIdx.z;
    const int j0 = (int)blockIdx.x * (kThreads * NJ) + tid;
    const size_t rowoff = (size_t)r * s.Npad, plane = (size_t)s.R * s.Npad;
    const double* xt = s.hx + (size_t)t * plane * DX + rowoff;
    const double* xn = s.hx + (size_t)(t + 1) * plane * DX + rowoff;
    const double* lwt = a.b.lw + (size_t)t * plane + rowoff;
    const ModelConst mc = a.b.mc[r];
    double zcov;
    CovVals<KC> zc;
    bsim_cov<KC>(a.b.z, t + 1, &zcov, &zc);
    load_exp_table<kThreads>(lds_etab);
    double xs[NJ][DX], m[NJ], D[NJ];
#pragma unroll
    for (int e = 0; e < NJ; ++e) {
        const int j = j0 + e * kThreads;
#pragma unroll
        for (int d = 0; d < DX; ++d) xs[e][d] = j < s.N ? xn[(size_t)d * plane + j] : 0.0;
        m[e] = -dinf(); D[e] = 0.0;
    }
    msm_column_sweep<MODEL, NJ, false>(a, mc, xt, lwt, plane, xs, zcov, zc, lds_etab, lds_x, lds_lw, m, D);
    msm_column_sweep<MODEL, NJ, true>(a, mc, xt, lwt, plane, xs, zcov, zc, lds_etab, lds_x, lds_lw, m, D);
#pragma unroll
    for (int e = 0; e < NJ; ++e) {
        const int j = j0 + e * kThreads;
        if (j < s.N) {
            a.cm[(size_t)t * plane + rowoff + j] = m[e];
            a.cD[(size_t)t * plane + rowoff + j] = (__builtin_isfinite(m[e]) && D[e] > 0.0) ? D[e] : 0.0;
        }
    }
}

// what a wave of k_msm_rows stages of a chunk of columns: one column per lane
template <int DX>
struct MsmColumns {
    double x[DX][64];          // x_{t+1}[j]
    double m[64];              // m_j
    double c[64];              // c_j of a live column, om_{t+1}[j] of a degenerate one
    int32_t g[64];             // -1: live; else g(j)
};

// grid = (ceil(N / 64), R), block = 64 kMsmSeg: om_t of the 64 rows i = 64 blockIdx.x + lane from om_{t+1} and the columns of step
// t + 1.  Wave s sums the chunks c = s, s + kMsmSeg, .. of 64 columns, each in ascending j; wave 0 adds the kMsmSeg partial sums in
// ascending s.  One launch per step, T - 2 .. 0, on the handle's stream.
template <int MODEL>
__global__ __launch_bounds__(64 * kMsmSeg) void k_msm_rows(const MsmArgs a, const int t) {
    constexpr int DX = model_dx<MODEL>(), KC = model_kcov<MODEL>(), NT = 64 * kMsmSeg;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    __shared__ MsmColumns<DX> cols[kMsmSeg];
    __shared__ double lds_part[kMsmSeg][64];
    const SmArgs& s = a.b.s;
    const int N = s.N, lane = threadIdx.x & 63, seg = threadIdx.x >> 6, r = blockIdx.y, i = (int)blockIdx.x * 64 + lane;
    const size_t rowoff = (size_t)r * s.Npad, plane = (size_t)s.R * s.Npad;
    const double* xt = s.hx + (size_t)t * plane * DX + rowoff;
    const double* xn = s.hx + (size_t)(t + 1) * plane * DX + rowoff;
    const double* cm = a.cm + (size_t)t * plane + rowoff;
    const double* cD = a.cD + (size_t)t * plane + rowoff;
    const double* omn = a.om + (size_t)(t + 1) * plane + rowoff;
    const uint32_t* anc1 = s.hanc + (size_t)(t + 1) * plane + rowoff;
    const bool res = sm_resampled(t + 1, s.resamp_sched);
    const ModelConst mc = a.b.mc[r];
    double zcov;
    CovVals<KC> zc;
    bsim_cov<KC>(a.b.z, t + 1, &zcov, &zc);
    load_exp_table<NT>(lds_etab);                          // first read behind the first barrier below
    MsmColumns<DX>& col = cols[seg];
    double xi[DX];
    const double lw = i < N ? a.b.lw[(size_t)t * plane + rowoff + i] : -dinf();
#pragma unroll
    for (int d = 0; d < DX; ++d) xi[d] = i < N ? xt[(size_t)d * plane + i] : 0.0;
    double acc = 0.0;
    const int nchunks = (N + 63) / 64;
    for (int c0 = 0; c0 < nchunks; c0 += kMsmSeg) {        // the same trip count in every wave: the barriers are uniform
        const int jc = (c0 + seg) * 64;                    // this wave's chunk; beyond N: nothing staged is used
        __syncthreads();                                   // the chunk before this one is consumed
        {
            const int j = jc + lane;
            double w = 0.0, D = 0.0, mj = 0.0;
            int32_t g = -1;
            if (j < N) {
                w = omn[j]; D = cD[j]; mj = cm[j];
                if (!(D > 0.0)) {
                    const uint32_t p = res ? anc1[j] : (uint32_t)j;
                    g = (int32_t)(p < (uint32_t)(N - 1) ? p : (uint32_t)(N - 1));
                }
            }
            col.g[lane] = g;
            col.m[lane] = mj;
            col.c[lane] = (j < N && g < 0) ? w / D : w;
#pragma unroll
            for (int d = 0; d < DX; ++d) col.x[d][lane] = j < N ? xn[(size_t)d * plane + j] : 0.0;
        }
        __syncthreads();
        const int n = N - jc < 64 ? N - jc : 64;           // <= 0 beyond N
        for (int k = 0; k < n; ++k) {
            const int32_t g = col.g[k];
            const double c = col.c[k];
            if (g < 0) {
                double xj[DX];
#pragma unroll
                for (int d = 0; d < DX; ++d) xj[d] = col.x[d][k];
                double v = lw + bsim_logf<MODEL>(mc, xj, xi, zcov, zc, lds_etab);
                v = (v != v) ? -dinf() : v;
                acc = acc + c * __builtin_rint(dexp_scaled_t(v - col.m[k], a.b.shift, lds_etab));
            } else if (i == g) {
                acc = acc + c;
            }
        }
    }
    lds_part[seg][lane] = acc;
    __syncthreads();
    if (seg == 0 && i < N) {
        double w = lds_part[0][lane];
#pragma unroll
        for (int q = 1; q < kMsmSeg; ++q) w = w + lds_part[q][lane];
        a.om[(size_t)t * plane + rowoff + i] = w;
    }
}

// grid = (T R), block = kThreads: block t R + r forms out[(t n + f) R + r] = sum_j h_f(x_t[j]) om_t[j] / sum_j om_t[j] (component 0 of
// the state); NaN where the denominator is not > 0.
__global__ __launch_bounds__(kThreads) void k_msm_expect(const MsmArgs a, const FunctionalIds fs, double* out) {
    __shared__ double lds[kMaxFunctionals][4], lds_den[4];
    const SmArgs& s = a.b.s;
    const int tid = threadIdx.x, t = blockIdx.x / s.R, r = blockIdx.x % s.R;
    const size_t rowoff = (size_t)r * s.Npad, plane = (size_t)s.R * s.Npad;
    const double* xt = s.hx + (size_t)t * plane * (size_t)s.dx + rowoff;
    const double* om = a.om + (size_t)t * plane + rowoff;
    double num[kMaxFunctionals] = {0.0, 0.0, 0.0, 0.0}, den = 0.0;
    for (int j = tid; j < s.N; j += kThreads) {
        const double w = om[j];
        expect_add(num, fs, xt[j], w);
        den = den + w;
    }
    expect_wave_sums(num, lds, tid);
    den = wave_sum_xor(den);
    if ((tid & 63) == 0) lds_den[tid >> 6] = den;
    __syncthreads();
    if (tid < fs.n) {
        const double d4 = ((lds_den[0] + lds_den[1]) + lds_den[2]) + lds_den[3];
        out[((size_t)t * fs.n + tid) * s.R + r] = d4 > 0.0 ? expect_tile_sum(lds, tid) / d4 : dnan();
    }
}

}  // namespace ssme
