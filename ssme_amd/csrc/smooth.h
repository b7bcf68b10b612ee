// smooth.h -- the smoothing distribution p(x_{0:T-1} | y_{0:T-1}) of a recorded series, gfx950.
//
// ssme_pf_set_series_history makes ssme_pf_run_series keep, per step t, the pre-resampling population x_t (all state planes) and the
// ancestors anc_t the resampling draw of step t took in the population of step t - 1 (pf_small.h: the recording instantiations of the
// whole-series kernels; pf_api.hip: the tiled route, whose step kernel then writes straight into the history rows).  The lineage of
// final particle j is  B_{T-1}(j) = j,  B_{t-1}(j) = anc_t[B_t(j)]  where step t resampled (t >= 1 and t % resamp_sched == 0) and
// B_{t-1}(j) = B_t(j) otherwise: the kernels here read the schedule, so rows of anc that no draw wrote are never looked at.
// The smoothing weights are the final step's fixed-point weights q_j (tile-local differences of the integer cdf, tile scales
// e^{m_b - m}): the weights of ssme_pf_get_expectations_multi and of the forecast's start draw.
//
// Tracing is independent per final particle, so the whole backward pass is ONE launch.  A lane owns several final particles and
// carries their lineage indices (and weights) in registers; per step it issues, for all of them at once, one 4-byte gather
// anc_t[B] and one 8-byte gather per plane x_t[B], both of which depend on B alone -- a step costs one dependent memory round trip,
// and the lane's chains plus the resident waves (256-thread workgroups of few registers: 8 waves per SIMD) keep the loads in flight.
//   k_sm_trajectories<DX>  K terminal indices per filter (given, or drawn by fc_draw_ancestor at i = k, t0 = T: the forecast's start
//                          draw), states of all planes and optionally the lineage indices, 4 trajectories per lane.
//   k_sm_sweep<NPL>        all N final particles: per step and tile sum_j h_f(x_t[B_t(j)]) q_j for up to 4 built-in functionals by
//                          the summation tree of k_expect_partials (expect_add / expect_wave_sums / expect_tile_sum, pf_kernels.h):
//                          thread v of 256 owns particles v, v + 256, ... of its tile (NPL = tile / 256 of them).
//   k_sm_final             k_expect_final's arithmetic (expect_final_filter) per (t, r) with the FINAL step's tile sums and maxima.
// Row T - 1 of the sweep is therefore, to the bit, what ssme_pf_get_expectations_multi returns after the series.
// Every gathered index is clamped to N - 1 before it is used: no lineage can leave its filter's row.
#pragma once
#include "pf_kernels.h"
#include "forecast.h"

namespace ssme {

constexpr int kSmChains = 4;               // trajectories per lane of k_sm_trajectories

struct SmArgs {
    const double* hx;          // [T][DX][R][Npad] populations of every step
    const uint32_t* hanc;      // [T][R][Npad] ancestors of the steps that resampled
    const double* cdf;         // [R][Npad] tile-local inclusive integer sums of the final step's fixed-point weights
    const double* l2_T;        // [R][Bs] level-2 tables of the final weights (k_level2_plan; the forecast's buffers)
    const double* l2_R;
    const FilterScalars* scal; // [R] S' of the final weights
    const uint32_t* keyp;      // [2] Philox key
    uint32_t first_filter;
    int32_t N, Npad, B, Bs, Bpow2, tile, R, T, resamp_sched;
    int32_t dx;                // state planes per history row (k_sm_trajectories<DX>: DX == dx)
};

// does step t draw ancestors (the filters' schedule)?
__device__ __forceinline__ bool sm_resampled(int t, int sched) { return t >= 1 && (t % sched) == 0; }

// grid = (ceil(K / (kSmChains kThreads)), R), block = kThreads.  x_out[((r K + k) T + t) DX + d], idx_out[(r K + k) T + t] or null.
// A filter without weight (S' not > 0) gets NaN states.
template <int DX>
__global__ __launch_bounds__(kThreads) void k_sm_trajectories(const SmArgs a, const int K, const uint32_t* terminal /*[R][K] or null*/,
                                                             double* x_out, uint32_t* idx_out) {
    const int r = blockIdx.y, tid = threadIdx.x;
    const size_t rowoff = (size_t)r * a.Npad, plane = (size_t)a.R * a.Npad;
    const bool alive = a.scal[r].S > 0.0;
    const uint32_t last = (uint32_t)(a.N - 1);
    int k[kSmChains];
    uint32_t Bi[kSmChains];
#pragma unroll
    for (int c = 0; c < kSmChains; ++c) {
        k[c] = ((int)blockIdx.x * kSmChains + c) * kThreads + tid;
        Bi[c] = 0u;
        if (k[c] < K) {
            const uint32_t j = terminal ? terminal[(size_t)r * K + k[c]]
                                        : (uint32_t)fc_draw_ancestor(a.l2_T + (size_t)r * a.Bs, a.l2_R + (size_t)r * a.Bs, a.cdf + rowoff, a.scal[r].S, a.B,
                                                                     a.Bpow2, a.tile, a.N, k[c], (uint32_t)a.T, a.first_filter + (uint32_t)r, a.keyp[0], a.keyp[1]);
            Bi[c] = j < last ? j : last;
        }
    }
    for (int t = a.T - 1; t >= 0; --t) {
        const bool res = sm_resampled(t, a.resamp_sched);
        const double* xt = a.hx + (size_t)t * plane * DX + rowoff;
        const uint32_t* at = a.hanc + (size_t)t * plane + rowoff;
        double xv[kSmChains][DX];
        uint32_t nb[kSmChains];
#pragma unroll
        for (int c = 0; c < kSmChains; ++c) {
            nb[c] = Bi[c];
            if (k[c] < K) {
#pragma unroll
                for (int d = 0; d < DX; ++d) xv[c][d] = xt[(size_t)d * plane + Bi[c]];
                if (res) nb[c] = at[Bi[c]];
            }
        }
#pragma unroll
        for (int c = 0; c < kSmChains; ++c) {
            if (k[c] < K) {
                const size_t o = ((size_t)r * K + k[c]) * a.T + t;
#pragma unroll
                for (int d = 0; d < DX; ++d) x_out[o * DX + d] = alive ? xv[c][d] : dnan();
                if (idx_out) idx_out[o] = Bi[c];
                Bi[c] = nb[c] < last ? nb[c] : last;
            }
        }
    }
}

// grid = (B tiles, R), block = kThreads.  part[((t R + r) Bs + b) 4 + f]: the numerators of tile b at step t, by k_expect_partials'
// tree.  The wave sums are double-buffered, so a step has one barrier.
template <int NPL>
__global__ __launch_bounds__(kThreads) void k_sm_sweep(const SmArgs a, const FunctionalIds fs, double* part /*[T][R][Bs][kMaxFunctionals]*/) {
    __shared__ double lds[2][kMaxFunctionals][4];
    const int tid = threadIdx.x, b = blockIdx.x, r = blockIdx.y;
    const size_t rowoff = (size_t)r * a.Npad, plane = (size_t)a.R * a.Npad;
    const double* cr = a.cdf + rowoff + (size_t)b * a.tile;
    const int nvalid = (a.N - b * a.tile) < a.tile ? (a.N - b * a.tile) : a.tile;
    const uint32_t last = (uint32_t)(a.N - 1);
    double q[NPL];
    uint32_t Bi[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int j = tid + k * kThreads;
        q[k] = 0.0; Bi[k] = 0u;
        if (j < nvalid) { q[k] = cr[j] - (j ? cr[j - 1] : 0.0); Bi[k] = (uint32_t)(b * a.tile + j); }
    }
    for (int t = a.T - 1; t >= 0; --t) {
        const bool res = sm_resampled(t, a.resamp_sched);
        const double* xt = a.hx + (size_t)t * plane * (size_t)a.dx + rowoff;           // component 0 of the state
        const uint32_t* at = a.hanc + (size_t)t * plane + rowoff;
        double xv[NPL];
        uint32_t nb[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            xv[k] = 0.0; nb[k] = Bi[k];
            if (tid + k * kThreads < nvalid) {
                xv[k] = xt[Bi[k]];
                if (res) nb[k] = at[Bi[k]];
            }
        }
        double num[kMaxFunctionals] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            if (tid + k * kThreads < nvalid) expect_add(num, fs, xv[k], q[k]);
            Bi[k] = nb[k] < last ? nb[k] : last;
        }
        expect_wave_sums(num, lds[t & 1], tid);
        __syncthreads();
        if (tid < kMaxFunctionals) part[(((size_t)t * a.R + r) * a.Bs + b) * kMaxFunctionals + tid] = expect_tile_sum(lds[t & 1], tid);
    }
}

// grid = (T R), block = kThreads: block t R + r forms row t of filter r.  out[(t n + i) R + r].
__global__ __launch_bounds__(kThreads) void k_sm_final(const double* part, const double* tsum, const double* tmax, int B, int Bs, int R,
                                                      FunctionalIds fs, double* out) {
    const int t = blockIdx.x / R, r = blockIdx.x % R;
    expect_final_filter(part + (size_t)t * R * Bs * kMaxFunctionals, tsum, tmax, B, Bs, R, r, fs, out + (size_t)t * fs.n * R);
}

}  // namespace ssme
