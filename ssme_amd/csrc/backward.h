// backward.h -- backward-simulation smoothing of a recorded series (forward filtering, backward simulation: Godsill, Doucet and
// West 2004), gfx950.
//
// smooth.h traces the filter's own genealogy, whose lineages coalesce a few multiples of N steps back (path degeneracy).  Here every
// earlier state of a trajectory is drawn AGAIN from all N particles of its step, reweighted by the transition density to the state
// already chosen:
//     P(B_t = i | x~_{t+1})  prop.  W_t[i] f(x~_{t+1} | x_t[i], z_{t+1}),      x~_{t+1} = x_{t+1}[B_{t+1}].
// The history rows hold every x_t; the log-weights log W_t are recomputed from them, the series and the covariates by k_bsim_logw with
// the device functions the filter calls (model_logg, logg_vec, cov_logw), so a row is bit-equal to the log-weights the filter had
// before the resampling of step t.  The cost is O(K N T) density evaluations, sequential in t: large N is allowed up to the handle's
// limit and simply costs that.
//
// The draw (the specification a restatement follows; tests/backward_ref.py):
//     a_i = lw_t[i] + logf(x~ | x_t[i], z_{t+1})  (NaN counts as -inf),  m = max a_i,
//     q_i = rint(exp_t(a_i - m) 2^sh),  sh = min(41, 52 - ceil(log2 N))  (the filter's quantiser: every partial sum is an integer < 2^53),
//     S = sum q_i,  u = u01_mid40 of words 0-1 of Philox(k, t, filter id, STREAM_BSIM),  target = ceil(u S),
//     B_t = the first i whose inclusive sum C_i >= target.
// S and every C_i are exact integers, so the result does not depend on how the block adds them (block_scan_f64's argument).
// Fallback: m not finite or S not > 0 (a degenerate transition): B_t = anc_{t+1}[B_{t+1}], or B_{t+1} where step t + 1 did not
// resample -- the genealogy.  Every index is clamped to N - 1.
//
//   k_bsim_logw<MODEL>      one thread per particle, the log-weight carried in a register over the T steps of its row.
//   k_bsim<MODEL, NE>       one workgroup of kThreads per (filter, group of kBsimG trajectories), looping over t.  Thread v owns the NE
//                           consecutive particles v NE .. of a chunk of kThreads NE; x_t and lw_t are loaded once per group and used
//                           for all kBsimG chosen states.  N <= chunk: the candidates stay in registers across the maximum, the scan
//                           and the selection (three barriers per step).  Above, the workgroup walks the row chunk by chunk three
//                           times and recomputes a_i per pass (deterministic: the same bits).  NE = 2 up to 512 particles, 8 above.
#pragma once
#include "smooth.h"

namespace ssme {

enum { STREAM_BSIM = 165 };
constexpr int kBsimG = 4;                  // trajectories per workgroup of k_bsim

struct BsimArgs {
    SmArgs s;                  // the history in force (hx, hanc, schedule, shapes); k_bsim: also the terminal draw's tables
    const double* y;           // [T][dy] the series the history was recorded from
    const double* z;           // [T][max(dim_cov, 1)] its covariates, or null: zeros
    const ModelConst* mc;      // [R]
    double* lw;                // [T][R][Npad] pre-resampling log-weights of every step
    int32_t shift;             // sh of the quantiser
};

// log g of particle x (dim_x values) at a step, as the filter's step forms it: the increment of the particle's log-weight
template <int MODEL>
__device__ __forceinline__ double bsim_logg(const ModelConst& c, bool first_step, const double* y, const double* x,
                                            const CovVals<model_kcov<MODEL>()>& zc, const ExpTabEntry* etab) {
#if SSME_HAS_USER_MODEL
    if constexpr (MODEL == MODEL_USER0 && model_kcov<MODEL>() > 0) {
        return cov_logw<typename user_model_of<MODEL>::type>(c, first_step, y, zc.v, x, etab);
    } else if constexpr (MODEL == MODEL_USER0 && (model_dx<MODEL>() > 1 || model_dy<MODEL>() > 1)) {
        return c.bad ? -dinf() : user_calls<typename user_model_of<MODEL>::type>::logg_vec(c, y, x, etab);
    } else
#endif
        return model_logg<MODEL>(c, y[0], x[0], etab);
}

// log f(xn | x, covariates of the step that made xn), all state planes
template <int MODEL>
__device__ __forceinline__ double bsim_logf(const ModelConst& c, const double* xn, const double* x, double zcov,
                                            const CovVals<model_kcov<MODEL>()>& zc, const ExpTabEntry* etab) {
#if SSME_HAS_USER_MODEL
    if constexpr (MODEL == MODEL_USER0 && model_kcov<MODEL>() > 0) {
        return user_calls<typename user_model_of<MODEL>::type>::logf_vec(c, xn, x, zc.v, etab);
    } else if constexpr (MODEL == MODEL_USER0 && (model_dx<MODEL>() > 1 || model_dy<MODEL>() > 1)) {
        return user_calls<typename user_model_of<MODEL>::type>::logf_vec(c, xn, x, zcov, etab);
    } else
#endif
        return model_logf<MODEL>(c, xn[0], x[0], zcov, etab);
}

// the covariates of time row t: the scalar one of the built-in grammar and the KC of a dim_cov header (z null: zeros)
template <int KC>
__device__ __forceinline__ void bsim_cov(const double* z, int t, double* zcov, CovVals<KC>* zc) {
    *zcov = 0.0;
    if constexpr (KC > 0) {
#pragma unroll
        for (int j = 0; j < KC; ++j) zc->v[j] = z ? z[(size_t)t * KC + j] : 0.0;
    } else {
        zc->v[0] = 0.0;
        if (z) *zcov = z[t];
    }
}

// grid = (Npad / kThreads, R), block = kThreads.  lw[(t R + r) Npad + i]; -inf beyond N.
template <int MODEL>
__global__ __launch_bounds__(kThreads) void k_bsim_logw(const BsimArgs a) {
    constexpr int DX = model_dx<MODEL>(), DY = model_dy<MODEL>(), KC = model_kcov<MODEL>();
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    load_exp_table<kThreads>(lds_etab);
    __syncthreads();
    const int r = blockIdx.y, i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (i >= a.s.Npad) return;
    const size_t rowoff = (size_t)r * a.s.Npad, plane = (size_t)a.s.R * a.s.Npad;
    const ModelConst mc = a.mc[r];
    double lw = 0.0;
    for (int t = 0; t < a.s.T; ++t) {
        double yv[DY], xv[DX], zcov;
        CovVals<KC> zc;
#pragma unroll
        for (int d = 0; d < DY; ++d) yv[d] = a.y[(size_t)t * DY + d];
        bsim_cov<KC>(a.z, t, &zcov, &zc);
#pragma unroll
        for (int d = 0; d < DX; ++d) xv[d] = a.s.hx[((size_t)t * DX + d) * plane + rowoff + i];
        const double g = bsim_logg<MODEL>(mc, t == 0, yv, xv, zc, lds_etab);
        lw = ((t == 0 || sm_resampled(t, a.s.resamp_sched)) ? 0.0 : lw) + g;        // the step kernel's lw_old + gv
        a.lw[(size_t)t * plane + rowoff + i] = i < a.s.N ? lw : -dinf();
    }
}

// a_i of the NE particles i0 .. of one thread for the kBsimG chosen states xs; -inf beyond N and for NaN
template <int MODEL, int NE>
__device__ __forceinline__ void bsim_candidates(const ModelConst& mc, const double* xt, size_t plane, const double* lwt, int i0, int N,
                                                const double (&xs)[kBsimG][model_dx<MODEL>()], double zcov,
                                                const CovVals<model_kcov<MODEL>()>& zc, const ExpTabEntry* etab, double (&av)[NE][kBsimG]) {
    constexpr int DX = model_dx<MODEL>();
    if (i0 >= N) {
#pragma unroll
        for (int e = 0; e < NE; ++e)
#pragma unroll
            for (int g = 0; g < kBsimG; ++g) av[e][g] = -dinf();
        return;
    }
    double xv[NE][DX], lw[NE];
    if (i0 + NE <= N) {
#pragma unroll
        for (int e = 0; e < NE; e += 2) {
            const double2 l = *reinterpret_cast<const double2*>(lwt + i0 + e);
            lw[e] = l.x; lw[e + 1] = l.y;
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                const double2 v = *reinterpret_cast<const double2*>(xt + (size_t)d * plane + i0 + e);
                xv[e][d] = v.x; xv[e + 1][d] = v.y;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool in = i0 + e < N;
            lw[e] = in ? lwt[i0 + e] : -dinf();
#pragma unroll
            for (int d = 0; d < DX; ++d) xv[e][d] = in ? xt[(size_t)d * plane + i0 + e] : 0.0;
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        double xi[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) xi[d] = xv[e][d];
#pragma unroll
        for (int g = 0; g < kBsimG; ++g) {
            const double v = lw[e] + bsim_logf<MODEL>(mc, xs[g], xi, zcov, zc, etab);
            av[e][g] = (v != v || !(i0 + e < N)) ? -dinf() : v;
        }
    }
}

// the block's maximum of kBsimG values per thread (none is NaN); slots: [kBsimG][kThreads / 64], one barrier
__device__ __forceinline__ void bsim_block_max(double (&m)[kBsimG], double (*slots)[kThreads / 64]) {
    constexpr int NW = kThreads / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < kBsimG; ++g) {
        const double w = wave_max_f64(m[g]);
        if (lane == 0) slots[g][wave] = w;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kBsimG; ++g) {
        double v = slots[g][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) { const double o = slots[g][w]; v = o > v ? o : v; }
        m[g] = v;
    }
}

// exclusive prefix over the threads (in thread order) and the block's total of kBsimG integer-valued doubles per thread: exact while
// every partial sum is below 2^53.  slots: [kBsimG][kThreads / 64], one barrier.
__device__ __forceinline__ void bsim_block_prefix(const double (&v)[kBsimG], double (&pre)[kBsimG], double (&tot)[kBsimG],
                                                  double (*slots)[kThreads / 64]) {
    constexpr int NW = kThreads / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double inc[kBsimG];
#pragma unroll
    for (int g = 0; g < kBsimG; ++g) {
        inc[g] = wave_incl_scan_f64(v[g]);
        if (lane == 63) slots[g][wave] = inc[g];
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kBsimG; ++g) {
        double before = 0.0, all = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { const double s = slots[g][w]; all = all + s; if (w < wave) before = before + s; }
        pre[g] = before + (inc[g] - v[g]);
        tot[g] = all;
    }
}

// grid = (ceil(K / kBsimG), R), block = kThreads.  Outputs as k_sm_trajectories: x_out[((r K + k) T + t) DX + d], idx_out[(r K + k) T + t]
// or null.  A filter without final weight (S' not > 0) gets NaN states.
template <int MODEL, int NE>
__global__ __launch_bounds__(kThreads) void k_bsim(const BsimArgs a, const int K, const uint32_t* terminal /*[R][K] or null*/, double* x_out,
                                                  uint32_t* idx_out) {
    constexpr int DX = model_dx<MODEL>(), KC = model_kcov<MODEL>(), G = kBsimG, NW = kThreads / 64, CHUNK = kThreads * NE;
    static_assert(NE % 2 == 0, "candidates are loaded in pairs");
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    __shared__ double lds_m[2][G][NW], lds_s[2][G][NW], lds_u[2][G];
    __shared__ uint32_t lds_b[2][G];
    const SmArgs& s = a.s;
    const int tid = threadIdx.x, r = blockIdx.y, k0 = (int)blockIdx.x * G;
    const size_t rowoff = (size_t)r * s.Npad, plane = (size_t)s.R * s.Npad;
    const uint32_t last = (uint32_t)(s.N - 1);
    const bool alive = s.scal[r].S > 0.0;
    const ModelConst mc = a.mc[r];
    const int nch = (s.N + CHUNK - 1) / CHUNK;
    load_exp_table<kThreads>(lds_etab);
    if (tid < G) {
        uint32_t j = 0u;
        if (k0 + tid < K)
            j = terminal ? terminal[(size_t)r * K + k0 + tid]
                         : (uint32_t)fc_draw_ancestor(s.l2_T + (size_t)r * s.Bs, s.l2_R + (size_t)r * s.Bs, s.cdf + rowoff, s.scal[r].S, s.B, s.Bpow2,
                                                      s.tile, s.N, k0 + tid, (uint32_t)s.T, s.first_filter + (uint32_t)r, s.keyp[0], s.keyp[1]);
        lds_b[1][tid] = j < last ? j : last;
    }
    __syncthreads();
    uint32_t Bi[G];
    double xs[G][DX];
#pragma unroll
    for (int g = 0; g < G; ++g) Bi[g] = lds_b[1][g];
    int pm = 0, ps = 0;                    // which half of lds_m / lds_s the next block reduction writes
    for (int t = s.T - 1; t >= 0; --t) {
        const double* xt = s.hx + (size_t)t * plane * DX + rowoff;
        if (t < s.T - 1) {
            // ---- B_t of the G trajectories from B_{t+1} (Bi) and x~ = x_{t+1}[B_{t+1}] (xs) ----
            const int pb = t & 1;
            const double* lwt = a.lw + (size_t)t * plane + rowoff;
            double zcov;
            CovVals<KC> zc;
            bsim_cov<KC>(a.z, t + 1, &zcov, &zc);
            if (tid < G) {
                const u32x4 o = philox4x32_10((uint32_t)(k0 + tid), (uint32_t)t, s.first_filter + (uint32_t)r, (uint32_t)STREAM_BSIM, s.keyp[0], s.keyp[1]);
                lds_u[pb][tid] = u01_mid40(o.v0, o.v1);
            }
            double av[NE][G], m[G], S[G], target[G];
#pragma unroll
            for (int g = 0; g < G; ++g) { m[g] = -dinf(); S[g] = 0.0; }
            for (int ch = 0; ch < nch; ++ch) {
                bsim_candidates<MODEL, NE>(mc, xt, plane, lwt, ch * CHUNK + tid * NE, s.N, xs, zcov, zc, lds_etab, av);
#pragma unroll
                for (int e = 0; e < NE; ++e)
#pragma unroll
                    for (int g = 0; g < G; ++g) m[g] = av[e][g] > m[g] ? av[e][g] : m[g];
            }
            bsim_block_max(m, lds_m[pm]);
            pm ^= 1;
            if (nch > 1) {
                // the sum first: the target is needed before the chunks are scanned
                double part[G], pre[G];
#pragma unroll
                for (int g = 0; g < G; ++g) part[g] = 0.0;
                for (int ch = 0; ch < nch; ++ch) {
                    bsim_candidates<MODEL, NE>(mc, xt, plane, lwt, ch * CHUNK + tid * NE, s.N, xs, zcov, zc, lds_etab, av);
#pragma unroll
                    for (int e = 0; e < NE; ++e)
#pragma unroll
                        for (int g = 0; g < G; ++g) part[g] = part[g] + __builtin_rint(dexp_scaled_t(av[e][g] - m[g], a.shift, lds_etab));
                }
                bsim_block_prefix(part, pre, S, lds_s[ps]);
                ps ^= 1;
            }
            double run[G];
#pragma unroll
            for (int g = 0; g < G; ++g) { run[g] = 0.0; target[g] = 0.0; }
            for (int ch = 0; ch < nch; ++ch) {
                if (nch > 1) bsim_candidates<MODEL, NE>(mc, xt, plane, lwt, ch * CHUNK + tid * NE, s.N, xs, zcov, zc, lds_etab, av);
                // q in place, then the thread's own inclusive sums
                double tsum[G], pre[G], tot[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const double q = __builtin_rint(dexp_scaled_t(av[e][g] - m[g], a.shift, lds_etab));
                        av[e][g] = e ? av[e - 1][g] + q : q;
                    }
                    tsum[g] = av[NE - 1][g];
                }
                bsim_block_prefix(tsum, pre, tot, lds_s[ps]);
                ps ^= 1;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (nch == 1) S[g] = tot[g];
                    if (ch == 0) target[g] = __builtin_ceil(lds_u[pb][g] * S[g]);
                    const double base = run[g] + pre[g];
                    if (__builtin_isfinite(m[g]) && S[g] > 0.0) {
#pragma unroll
                        for (int e = 0; e < NE; ++e) {
                            const double lo = base + (e ? av[e - 1][g] : 0.0), hi = base + av[e][g];
                            if (lo < target[g] && target[g] <= hi) lds_b[pb][g] = (uint32_t)(ch * CHUNK + tid * NE + e);
                        }
                    }
                    run[g] = run[g] + tot[g];
                }
            }
            __syncthreads();
            const bool res = sm_resampled(t + 1, s.resamp_sched);
            const uint32_t* anc1 = s.hanc + (size_t)(t + 1) * plane + rowoff;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                uint32_t nb;
                if (__builtin_isfinite(m[g]) && S[g] > 0.0) nb = lds_b[pb][g];
                else nb = res ? anc1[Bi[g]] : Bi[g];                   // a degenerate transition: the genealogy
                Bi[g] = nb < last ? nb : last;
            }
        }
        // ---- the states at B_t, and the outputs of step t ----
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int d = 0; d < DX; ++d) xs[g][d] = xt[(size_t)d * plane + Bi[g]];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (tid == g && k0 + g < K) {
                const size_t o = ((size_t)r * K + k0 + g) * s.T + t;
#pragma unroll
                for (int d = 0; d < DX; ++d) x_out[o * DX + d] = alive ? xs[g][d] : dnan();
                if (idx_out) idx_out[o] = Bi[g];
            }
        }
    }
}

}  // namespace ssme
