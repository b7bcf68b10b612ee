// pf_small.h -- whole-series kernel for filters that fit one tile (N <= 2048): the T steps of
// BSFilter::filter (call site example/estimate_univ_svol.h:121-127) run inside ONE launch, one workgroup
// per filter.  Particles and the integer weight cdf stay in LDS, log-weights in registers; there is no
// kernel boundary and no HBM round trip per step, which is what bounds small filters (a step of the
// tiled kernel costs ~10 us of launch + dependent-latency chain however small N is).
//
// The arithmetic is the tiled kernel's (k_filter_step with B = 1) operation for operation: same Philox
// counters, same spacings / targets / count-search, same tile max and exact fp64-integer scan.  The two
// paths are bit-identical (tests/test_parity_gpu.py::test_small_series_kernel_*); the oracle does not
// distinguish them.  Used by ssme_pf_run_series when the filter has one tile (the shipped example's
// N = 500, example/main.cpp:9) -- the step API and multi-tile filters use k_filter_step.
//
// Two kernels, one particle pair per lane (k_filter_series_small) and one particle per lane (k_filter_series_lane), built
// from the same pieces: a step is prefetch (SeriesInputs), level-2 (one_tile_level2), draws, targets (target_of), search
// (count_less_radix8) and gather, model step (scalar_step; vector_step for a vector user model), maximum, weights and scan, publish;
// after the loop series_accounting and hand_over_state.
//
// A vector user model (dim_x or dim_y > 1, model_api.h) runs the same two kernels: `if constexpr` on model_dx / model_dy adds the
// planes d >= 1 of the state to LDS (lds_x[DX][P]: at most (4 + 1) x 2048 x 8 B + tables = 84 KiB at (dim_x, N) = (4, 2048), one
// workgroup per CU), their normals (xdim_words) and the DY values of an observation row; component 0 and everything about the weights
// is the scalar text.  Shapes are the scalar models' (512 threads x 1 or 2 pairs; lanes up to 512): no instantiation of the four test
// headers spills a VGPR (profiles/vector_series_kernels.txt).
//
// Recording instantiations (ssme_pf_set_series_expectations): the same two kernels with a third argument,
// SeriesRec, write E[h(x_t) | y_{1:t}] of every step from LDS (record_step_expectations) with the bits of the step API's
// expectation kernels.  The instantiations without it are untouched by that code.
#pragma once
#include "pf_kernels.h"

#include <type_traits>

#ifndef SSME_LANE_XDIM_AHEAD
#define SSME_LANE_XDIM_AHEAD 1             // lane kernel, vector models: the d >= 1 normals of step t + 1 are drawn during step t, as
#endif                                     // component 0's are (0: at the model step).  Same bits.  Measured both ways: within 0.06 us per
                                           // step of each other in either direction, except the dim_cov model (2.28 against 2.41 us at
                                           // N = 100 ahead): kept ahead (profiles/vector_series_timing.txt, section 2)

namespace ssme {

// The inputs of a step that do not depend on the filter's state, requested one step ahead (uniform scalar loads).
// Components 1 .. DY-1 of a vector observation (a row of a series is DY values); nothing for a scalar one.
template <int DY>
struct ObsTail {
    double yv[DY - 1];
    __device__ __forceinline__ void load_tail(const double* y, int row) {
#pragma unroll
        for (int d = 1; d < DY; ++d) yv[d - 1] = y[row * DY + d];
    }
    __device__ __forceinline__ double tail(int d) const { return yv[d - 1]; }
};
template <>
struct ObsTail<1> {
    __device__ __forceinline__ void load_tail(const double*, int) {}
    __device__ __forceinline__ double tail(int) const { return 0.0; }
};
template <int KC, int DY = 1>
struct SeriesInputs : ObsTail<DY> {
    double y, z;                 // observation (component 0 of a vector one); scalar covariate (0 without one)
    CovVals<KC> zc;              // dim_cov user model: its KC covariates take the scalar one's place
    double gam, pgam, G;         // sorted-multinomial resampling steps: Gamma of tile 0, the prefix before it, the total (B = 1)

    __device__ __forceinline__ void load_row(const StepArgs& a, int r, int row) {
        y = a.y[row * DY];
        this->load_tail(a.y, row);
        if (a.z) {                   // a series without covariates keeps the zeros of load_first
            if constexpr (KC > 0) zc.load(a.z, (size_t)row);
            else z = a.z[row];
        }
        if (a.resampler == RESAMP_MULTINOMIAL && row > 0 && row % a.resamp_sched == 0) {
            const size_t g = (size_t)row * a.R + r;
            gam = a.gam[g * a.B]; pgam = a.pgam[g * a.B]; G = a.gtot[g];
        }
    }
    __device__ __forceinline__ void load_first(const StepArgs& a, int r) {
        z = 0.0; gam = 0.0; pgam = 0.0; G = 1.0;
#pragma unroll
        for (int j = 0; j < KC; ++j) zc.v[j] = 0.0;
        load_row(a, r, 0);
    }
    // Row `row` of a series of T, requested by the step before it.  (The step copies the struct and then calls this: a
    // member that returned the copy cost the lane kernel 11 VGPRs and a wave per SIMD.)
    __device__ __forceinline__ void request(const StepArgs& a, int r, int row, int T) {
        if (row < T) load_row(a, r, row);
    }
    // the DY values of the observation, as the vector callbacks take them
    __device__ __forceinline__ void obs(double* yv) const {
        yv[0] = y;
#pragma unroll
        for (int d = 1; d < DY; ++d) yv[d] = this->tail(d);
    }
};

// One step of one particle of a vector model inside the series kernels: vector_step on component 0 from the scalar path (x0, zn0)
// and components d >= 1 from xv / znv (slot 0 of both unused); the new components d >= 1 return in xnv[d], component 0 in *xn0.
template <int MODEL, class IN>
__device__ __forceinline__ double series_vector_step(const ModelConst& mc, bool first_step, double x0, double zn0, const double* xv,
                                                     const double* znv, const IN& in, double* xn0, double* xnv, const ExpTabEntry* etab) {
    constexpr int DX = model_dx<MODEL>();
    double x[kMaxDim], zn[kMaxDim], y[kMaxDim], xn[kMaxDim];
    x[0] = x0; zn[0] = zn0;
#pragma unroll
    for (int d = 1; d < DX; ++d) { x[d] = xv[d]; zn[d] = znv[d]; }
    in.obs(y);
    const double g = vector_step<MODEL>(mc, first_step, x, zn, y, in.z, in.zc, xn, etab);
    *xn0 = xn[0];
#pragma unroll
    for (int d = 1; d < DX; ++d) xnv[d] = xn[d];
    return g;
}

// Level-2 of a filter of one tile (level2_scan for B = 1) from the previous step's tile sum and maximum: m, S = A' and
// R0 = A / A'.  Thread 0 records (m, S) at ms_t; the logarithm is taken after the loop (series_accounting).
// One tile: m_b - m is +0 unless the max is NaN or infinite, and the shift is 0 (Npad = 2048); exp(0) 2^0 = 1 exactly
// (dexp_scaled_t: n = 0, r = 0, table entry (1, 0)), so the shortcut gives the bits of the full form wherever it is taken.
struct Level2 { double m, S, R0; };
__device__ __forceinline__ Level2 one_tile_level2(double A_prev, double mb_prev, int rshift, const ExpTabEntry* etab, double* ms_t) {
    Level2 l;
    l.m = (mb_prev != mb_prev) ? dnan() : mb_prev;
    const double dm = mb_prev - l.m;
    const int sh = rshift - kTileShift;
    l.S = (dm == 0.0 && sh == 0) ? __builtin_rint(A_prev) : __builtin_rint(A_prev * dexp_scaled_t(dm, sh, etab));
    l.R0 = A_prev / l.S;
    if (threadIdx.x == 0) { ms_t[0] = l.m; ms_t[1] = l.S; }
    return l;
}

// Integer resampling target of particle i under the systematic, stratified and iid-multinomial resamplers (the sorted
// multinomial one comes from the scanned spacings).  u0: the step's systematic offset; v: the particle's own uniform
// (stratified, iid), drawn by the caller; t_scale = S / N.  k_filter_step forms the same targets pair by pair.
__device__ __forceinline__ double target_of(int resampler, int i, double v, double u0, double t_scale, double S) {
    if (resampler == RESAMP_SYSTEMATIC) return __builtin_ceil(((double)i + u0) * t_scale);
    if (resampler == RESAMP_STRATIFIED) return __builtin_ceil(((double)i + v) * t_scale);
    return __builtin_ceil(v * S);
}

// j[q] = min(#{ i < P : tile[i] < target[q] }, P-1) for NQ targets at once by a radix-8 descent: the probes of one level, of
// all queries, are independent loads, so a search costs log8(P) dependent LDS round trips instead of log2(P) -- these kernels
// run one or two waves per SIMD and are bound by dependent latency, not by issue slots.  Same count as count_less_pow2
// (monotone tile).
template <int P, int NQ>
__device__ __forceinline__ void count_less_radix8(const double* tile, const double (&target)[NQ], int (&j)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) j[q] = 0;
#pragma unroll
    for (int w = P; w > 1;) {
        const int radix = (w >= 8) ? 8 : w;          // P is a power of two: the last level may be radix 2 or 4
        const int s = w / radix;
        int c[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) c[q] = 0;
#pragma unroll
        for (int k = 1; k < radix; ++k) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) c[q] += (tile[j[q] + k * s - 1] < target[q]) ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) j[q] += c[q] * s;
        w = s;
    }
}

// NOPS independent block scans of one value per lane behind ONE barrier (their DPP chains interleave):
// v[o] -> (incl[o], total[o]).  lds_seg: 16 doubles per operand, private to this call (no trailing barrier).
template <int NT, int NOPS>
__device__ __forceinline__ void block_scan_lanes_f64(const double (&v)[NOPS], double (&incl)[NOPS], double (&total)[NOPS],
                                                     double (*lds_seg)[16]) {
    constexpr int NSEG = NT / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double inc[NOPS];
#pragma unroll
    for (int o = 0; o < NOPS; ++o) inc[o] = wave_incl_scan_f64(v[o]);
    if constexpr (NSEG == 1) {
#pragma unroll
        for (int o = 0; o < NOPS; ++o) { incl[o] = inc[o]; total[o] = readlane_f64(inc[o], 63); }
        return;
    }
    if (lane == 63) {
#pragma unroll
        for (int o = 0; o < NOPS; ++o) lds_seg[o][wave] = inc[o];
    }
    __syncthreads();
    double sv[NOPS];
#pragma unroll
    for (int o = 0; o < NOPS; ++o) sv[o] = row16_incl_scan((lane & 15) < NSEG ? lds_seg[o][lane & 15] : 0.0);
#pragma unroll
    for (int o = 0; o < NOPS; ++o) {
        total[o] = readlane_f64(sv[o], 15);
        incl[o] = (wave ? readlane_f64(sv[o], wave - 1) : 0.0) + inc[o];
    }
}

// The PPT consecutive slots a lane owns, as one store (PPT = 2: p is 16-byte aligned)
template <int PPT>
__device__ __forceinline__ void store_slots(double* p, const double* v) {
    static_assert(PPT == 1 || PPT == 2, "one particle or one pair per lane");
    if constexpr (PPT == 2) *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    else *p = v[0];
}

// The end of a series, called by every thread after the last step's closing barrier.
// Log conditional likelihoods outside the time loop: the loop only records (m_t, S_t) of the step before (one_tile_level2);
// here the last step's pair joins them, the T logarithms are evaluated in parallel and one wave replays the sequential
// accounting (ll_t = lse_t - prev_t, loglik += ll_t) in loop order, 64 steps per load.  Same arithmetic and order as
// kf_finalize step by step, so the same bits.
template <int NT>
__device__ __forceinline__ void series_accounting(const StepArgs& a, int r, int T, double* ms, double A_prev, double mb_prev,
                                                  const ExpTabEntry* etab) {
    const int tid = threadIdx.x;
    const Level2 last = one_tile_level2(A_prev, mb_prev, a.rshift, etab, ms + 2 * (T - 1));
    __syncthreads();
    for (int t = tid; t < T; t += NT) {
        ms[2 * t] = lse_of(ms[2 * t], ms[2 * t + 1], a.rshift);      // (m_t, S_t) -> lse_t
    }
    __syncthreads();
    if (tid < 64) {
        double prev = a.scal[r].prev, loglik = a.scal[r].loglik, last_ll = 0.0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + tid;
            const double lse = (t < T) ? ms[2 * t] : 0.0;
            double mine = 0.0;
            const int nb = (T - t0 < 64) ? T - t0 : 64;
            for (int j = 0; j < nb; ++j) {
                const double lj = readlane_f64(lse, j);
                const double ll = lj - prev;
                loglik = loglik + ll;
                prev = (((t0 + j + 1) % a.resamp_sched) == 0) ? a.logN : lj;
                last_ll = ll;
                if (tid == j) mine = ll;
            }
            if (t < T && a.per_step) a.per_step[(size_t)r * a.Tcap + t] = mine;
        }
        if (tid == 0) {
            FilterScalars* o = a.scal + r;
            o->m = last.m; o->S = last.S; o->prev = prev; o->loglik = loglik; o->last_ll = last_ll;
            a.tsum_out[(size_t)r * a.Bs] = A_prev;
            a.tmax_out[(size_t)r * a.Bs] = mb_prev;
        }
    }
}

// State hand-over after the series, as k_filter_step leaves it: a lane's NK runs of PPT slots (x, lw: [NK][PPT], slot
// (k NT + tid) PPT), the cdf from LDS, and beyond P = NT NK PPT: x = 0, cdf flat at the tile sum, log-weight -inf.
// A vector state: xv holds components 1 .. DX-1 as [DX][NK][PPT] (slot 0 unused); plane d goes to x_out + d * xplane, zeros up
// to the tile end in every plane.
template <int NT, int NK, int PPT, int DX = 1>
__device__ __forceinline__ void hand_over_state(const StepArgs& a, size_t rowoff, const double* x, const double* xv, const double* lw,
                                                const double* lds_cdf, double A_prev) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i = (k * NT + tid) * PPT;
        store_slots<PPT>(a.x_out + rowoff + i, x + k * PPT);
#pragma unroll
        for (int d = 1; d < DX; ++d) store_slots<PPT>(a.x_out + (size_t)d * a.xplane + rowoff + i, xv + (d * NK + k) * PPT);
        store_slots<PPT>(a.cdf_out + rowoff + i, lds_cdf + i);
        if (a.logw) store_slots<PPT>(a.logw + rowoff + i, lw + k * PPT);
    }
    const double zero[2] = {0.0, 0.0}, flat[2] = {A_prev, A_prev}, ninf[2] = {-dinf(), -dinf()};
    for (int i = (NT * NK + tid) * PPT; i < kTile; i += NT * PPT) {
        store_slots<PPT>(a.x_out + rowoff + i, zero);
#pragma unroll
        for (int d = 1; d < DX; ++d) store_slots<PPT>(a.x_out + (size_t)d * a.xplane + rowoff + i, zero);
        store_slots<PPT>(a.cdf_out + rowoff + i, flat);
        if (a.logw) store_slots<PPT>(a.logw + rowoff + i, ninf);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Recorded series (ssme_pf_set_series_expectations): the filtered expectations of EVERY step, E[h(x_t) | y_{1:t}], written by the
// series kernels themselves.  After the closing barrier of step t the workgroup holds what k_expect_partials / k_user_expect_partials
// and the two final kernels read from memory after a step of the step API -- the particles of step t (all planes) and their
// tile-local cdf in LDS, the tile sum A and the tile maximum mb -- and it forms the same numbers by THEIR summation trees, not by
// its own thread layout, so a row has the bits of the two-launch path:
//   built-ins  virtual thread v of 256 adds particles v, v + 256, ... < N in this order (q_j = cdf_j - cdf_{j-1}, as there);
//   user h     virtual thread v adds 2v, 2v + 1, 2v + 512, 2v + 513, ... (valid ones only), all n_h outputs in one pass;
//   combining  the 64 virtual lanes of a wave by the xor butterfly 32 .. 1, the four waves as ((w0 + w1) + w2) + w3;
//   final      one tile: s = dexp(mb - m) with m = mb (NaN if mb is), E = (num s + 0) / (A s + 0), NaN where m is NaN.  The + 0 is
//              what the final kernels' sums over 255 idle threads amount to (-0 becomes +0); s is evaluated, not taken as 1:
//              mb = +-inf gives s = NaN and a NaN row, as the two launches do.
// The first 256 threads play the virtual threads (a workgroup of 64 or 128 takes them in 4 or 2 passes).  Nothing is staged: LDS
// grows by the wave sums alone ((4 + n_h) x 4 doubles).  One more barrier per step.  Thread f writes row t of functional f.
// ---------------------------------------------------------------------------------------------------------------------
struct SeriesRec {
    FunctionalIds fs;          // built-in functionals to record (n = 0: none)
    double* traj;              // [T][fs.n][R]
    double* utraj;             // [T][n_h][R] the user model's own functionals, or null
};
#if SSME_HAS_USER_MODEL
template <int MODEL> constexpr int model_nh() { return MODEL == MODEL_USER0 ? user_nh<ssme_user_model0>::n : 0; }
#else
template <int MODEL> constexpr int model_nh() { return 0; }
#endif

__device__ __forceinline__ const SeriesRec& the_rec(const SeriesRec& rec) { return rec; }      // the one element of RECARG...

// Series history (ssme_pf_set_series_history; smooth.h): a third kind of instantiation, RECARG = SeriesHist,
// that also keeps every step's population (all planes, as hand_over_state lays them out) and the ancestors of every resampling draw:
// hx row t is [DX][R][Npad] (plane stride a.xplane), hanc row t [R][Npad].  A step that does not resample writes no ancestors: the
// backward pass reads the schedule.  The expectations are recorded as in the SeriesRec instantiation when any are asked for.
struct SeriesHist : SeriesRec {
    double* hx;                // [T][DX][R][Npad]
    uint32_t* hanc;            // [T][R][Npad]
};
template <class... RECARG> constexpr bool series_hist_v = (std::is_same<RECARG, SeriesHist>::value || ...);
__device__ __forceinline__ const SeriesHist& the_hist(const SeriesHist& hs) { return hs; }

template <int MODEL, int NT, class IN>
__device__ __forceinline__ void record_step_expectations(const SeriesRec& rec, const StepArgs& a, const ModelConst& mc, const IN& in, int r,
                                                         int t, const double* lds_x, int xstride, const double* lds_cdf, double A,
                                                         double mb, const ExpTabEntry* etab, double (*lds_red)[4]) {
    constexpr int NH = model_nh<MODEL>();
    [[maybe_unused]] constexpr int DX = model_dx<MODEL>();
    constexpr int PASSES = NT >= kThreads ? 1 : kThreads / NT;
    const int tid = threadIdx.x, N = a.N;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int v = p * NT + tid;                                    // the virtual thread this lane plays (whole waves: v >> 6 is uniform)
        if (v < kThreads) {
            if (rec.fs.n > 0) {
                double num[kMaxFunctionals] = {0.0, 0.0, 0.0, 0.0};
                for (int j = v; j < N; j += kThreads) {
                    const double q = lds_cdf[j] - (j ? lds_cdf[j - 1] : 0.0);
                    const double xv = lds_x[j];
#pragma unroll
                    for (int f = 0; f < kMaxFunctionals; ++f)
                        if (f < rec.fs.n) num[f] = num[f] + builtin_h(rec.fs.id[f], xv) * q;
                }
#pragma unroll
                for (int f = 0; f < kMaxFunctionals; ++f) {
                    num[f] = wave_sum_xor(num[f]);
                    if ((v & 63) == 0) lds_red[f][v >> 6] = num[f];
                }
            }
#if SSME_HAS_USER_MODEL
            if constexpr (NH > 0) {
                if (rec.utraj) {
                    using M = typename user_model_of<MODEL>::type;
                    double num[NH];
#pragma unroll
                    for (int k = 0; k < NH; ++k) num[k] = 0.0;
                    for (int j = 2 * v; j < N; j += 2 * kThreads) {
                        const double c0 = lds_cdf[j], c1 = lds_cdf[j + 1];     // j + 1 < P: P is even
                        const double prev = j ? lds_cdf[j - 1] : 0.0;
                        const double q0 = c0 - prev, q1 = c1 - c0;
                        double xs[DX], hv[NH];
                        {
#pragma unroll
                            for (int d = 0; d < DX; ++d) xs[d] = lds_x[d * xstride + j];
                            if constexpr (model_kcov<MODEL>() > 0) M::h(mc, xs, in.zc.v, etab, hv);
                            else M::h(mc, xs, in.z, etab, hv);
#pragma unroll
                            for (int k = 0; k < NH; ++k) num[k] = num[k] + hv[k] * q0;
                        }
                        if (j + 1 < N) {
#pragma unroll
                            for (int d = 0; d < DX; ++d) xs[d] = lds_x[d * xstride + j + 1];
                            if constexpr (model_kcov<MODEL>() > 0) M::h(mc, xs, in.zc.v, etab, hv);
                            else M::h(mc, xs, in.z, etab, hv);
#pragma unroll
                            for (int k = 0; k < NH; ++k) num[k] = num[k] + hv[k] * q1;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        num[k] = wave_sum_xor(num[k]);
                        if ((v & 63) == 0) lds_red[kMaxFunctionals + k][v >> 6] = num[k];
                    }
                }
            }
#endif
        }
    }
    __syncthreads();
    const int nrec = kMaxFunctionals + ((NH > 0 && rec.utraj) ? NH : 0);
    if (tid < nrec && (tid >= kMaxFunctionals || tid < rec.fs.n)) {
        const double part = ((lds_red[tid][0] + lds_red[tid][1]) + lds_red[tid][2]) + lds_red[tid][3];
        const double m = (mb != mb) ? dnan() : mb;
        const double sc = dexp(mb - m);
        const double n4 = part * sc + 0.0;
        const double d4 = A * sc + 0.0;
        const double e = (m != m) ? dnan() : n4 / d4;
        if (tid < kMaxFunctionals) rec.traj[((size_t)t * rec.fs.n + tid) * a.R + r] = e;
        else rec.utraj[((size_t)t * NH + (tid - kMaxFunctionals)) * a.R + r] = e;
    }
}

// One particle PAIR per lane.
// grid = (R filters), block = NT, covers P = 2*NT*NK >= N particle slots (P a power of two, 256 .. 2048).
// a.x_out / cdf_out / tsum_out / tmax_out / logw receive the state after the last step (as k_filter_step
// leaves it), a.scal the accumulated log-likelihood; a.t / yi / gi are ignored (t = yi = gi = 0 .. T-1).
// a.small_ms: [R][Tcap][2] scratch.
// RECARG: empty, or SeriesRec for the recording instantiation, which takes it as a third kernel argument; `if constexpr` keeps every
// line of the recording out of the other instantiation, whose arguments and code are what they were without it.
template <int MODEL, int NT, int NK, class... RECARG>
__global__ __launch_bounds__(NT) void k_filter_series_small(const StepArgs a, const int T, const RECARG... recarg) {
    constexpr bool REC = sizeof...(RECARG) > 0;
    [[maybe_unused]] constexpr bool HIST = series_hist_v<RECARG...>;       // ... and the one that also keeps the series history
    constexpr int P = 2 * NT * NK;
    // A vector user model (model_api.h): component 0 travels the scalar path below unchanged; components d >= 1 live in planes
    // lds_x + d P, are gathered at the same ancestor, and draw their normals from stream STREAM_XDIM + d (xdim_words) for the
    // pair index k NT + tid, as k_filter_step's VEC branch does with B = 1.
    constexpr int DX = model_dx<MODEL>(), DY = model_dy<MODEL>();
    constexpr bool VEC = DX > 1 || DY > 1;
    __shared__ __attribute__((aligned(16))) double lds_x[DX * P];
    __shared__ __attribute__((aligned(16))) double lds_cdf[P];
    __shared__ double lds_seg_a[16];
    __shared__ double lds_seg_c[16];
    __shared__ double lds_d2[16];
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    double (*lds_red)[4] = nullptr;                    // recording: the wave sums of the expectations' numerators
    if constexpr (REC) {
        __shared__ double red[kMaxFunctionals + model_nh<MODEL>()][4];
        lds_red = red;
    }

    const int tid = threadIdx.x;
    load_log_table<NT>(&lds_dtab);
    load_exp_table<NT>(lds_etab);
    __syncthreads();
    const int r = blockIdx.x;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const uint32_t key0 = a.keyp[0], key1 = a.keyp[1];
    const size_t rowoff = (size_t)r * a.Npad;
    const ModelConst mc = a.mc[r];

    double* ms = a.small_ms + (size_t)r * a.Tcap * 2;
    double xcur[NK][2], lwcur[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k) { xcur[k][0] = 0.0; xcur[k][1] = 0.0; lwcur[k][0] = 0.0; lwcur[k][1] = 0.0; }
    double xcv[DX][NK][2];                             // components d >= 1 of the lane's particles (slot 0 unused)
    if constexpr (DX > 1) {
#pragma unroll
        for (int d = 1; d < DX; ++d)
#pragma unroll
            for (int k = 0; k < NK; ++k) { xcv[d][k][0] = 0.0; xcv[d][k][1] = 0.0; }
    }
    double A_prev = 0.0, mb_prev = 0.0;
    SeriesInputs<model_kcov<MODEL>(), DY> in_n;
    in_n.load_first(a, r);

    for (int t = 0; t < T; ++t) {
        const auto in = in_n;
        in_n.request(a, r, t + 1, T);
        const bool resampled = (t > 0) && (t % a.resamp_sched == 0);
        const bool multinomial = resampled && a.resampler == RESAMP_MULTINOMIAL;

        // --- level-2 of step t-1 ---
        Level2 l2 = {0.0, 0.0, 0.0};
        if (t > 0) l2 = one_tile_level2(A_prev, mb_prev, a.rshift, lds_etab, ms + 2 * (t - 1));

        // --- standard normals of this step: independent of the resampling chain, issued next to the spacings so that the
        //     two instruction streams interleave ---
        // one Philox call per pair feeds the normals (words 0-1) and the pair's two spacings (words 2-3): pair_words
        double zn[NK][2];
        double le[NK][2], se = 1.0;
        {
            double qe[NK][2];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const u32x4 o = pair_words((uint32_t)(k * NT + tid), (uint32_t)t, rep, key0, key1);
                pair_normals(o.v0, o.v1, &lds_dtab, &zn[k][0], &zn[k][1]);
                qe[k][0] = 0.0; qe[k][1] = 0.0;
                if (multinomial) {
                    const int i0 = (k * NT + tid) * 2;
                    double e0, e1;
                    pair_spacings(o, lds_dtab.log, &e0, &e1);
                    qe[k][0] = (i0 < a.N) ? __builtin_rint(e0 * 34359738368.0 /* 2^35 */) : 0.0;
                    qe[k][1] = (i0 + 1 < a.N) ? __builtin_rint(e1 * 34359738368.0) : 0.0;
                }
            }
            // --- exponential spacings (multinomial), exact scan ---
            if (multinomial) block_scan_f64<NT, NK>(qe, le, se, lds_seg_a);
        }

        double xin[NK][2], lw_old[NK][2];
        double xinv[DX][NK][2];                        // vector state: the inputs of components d >= 1 (nothing is read at t = 0)
        if constexpr (DX > 1) {
#pragma unroll
            for (int d = 1; d < DX; ++d)
#pragma unroll
                for (int k = 0; k < NK; ++k) { xinv[d][k][0] = (t == 0) ? 0.0 : xcv[d][k][0]; xinv[d][k][1] = (t == 0) ? 0.0 : xcv[d][k][1]; }
        }
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < NK; ++k) { xin[k][0] = 0.0; xin[k][1] = 0.0; lw_old[k][0] = 0.0; lw_old[k][1] = 0.0; }
        } else if (!resampled) {
#pragma unroll
            for (int k = 0; k < NK; ++k) { xin[k][0] = xcur[k][0]; xin[k][1] = xcur[k][1]; lw_old[k][0] = lwcur[k][0]; lw_old[k][1] = lwcur[k][1]; }
        } else {
            // --- targets, search in the cdf, gather ---
            double t_scale, u0 = 0.0;
            if (a.resampler == RESAMP_MULTINOMIAL) t_scale = l2.S / in.G;
            else {
                t_scale = l2.S / (double)a.N;
                if (a.resampler == RESAMP_SYSTEMATIC) u0 = systematic_u0((uint32_t)t, rep, key0, key1);
            }
            const double ratio = in.gam / se;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i0 = (k * NT + tid) * 2;
                double tau[2];
                if (a.resampler == RESAMP_MULTINOMIAL) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const double t1 = ratio * le[k][c];
                        const double t2 = in.pgam + t1;
                        tau[c] = __builtin_ceil(t2 * t_scale);
                    }
                } else {
                    double v[2] = {0.0, 0.0};
                    if (a.resampler != RESAMP_SYSTEMATIC) {
                        const u32x4 o = philox4x32_10((uint32_t)(i0 >> 1), (uint32_t)t, rep, STREAM_RESAMP, key0, key1);
                        v[0] = u01_co(o.v0, o.v1); v[1] = u01_co(o.v2, o.v3);
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c) tau[c] = target_of(a.resampler, i0 + c, v[c], u0, t_scale, l2.S);
                }
                const double tl[2] = {__builtin_ceil((tau[0] - 0.0) * l2.R0), __builtin_ceil((tau[1] - 0.0) * l2.R0)};
                int jj[2];
                count_less_radix8<P, 2>(lds_cdf, tl, jj);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int anc = jj[c] < a.N - 1 ? jj[c] : a.N - 1;
                    if (a.anc && (i0 + c) < a.N) a.anc[rowoff + i0 + c] = (uint32_t)anc;
                    if constexpr (HIST) { if ((i0 + c) < a.N) the_hist(recarg...).hanc[(size_t)t * a.xplane + rowoff + i0 + c] = (uint32_t)anc; }
                    xin[k][c] = lds_x[anc];
                    if constexpr (DX > 1) {            // every plane at the one clamped ancestor
#pragma unroll
                        for (int d = 1; d < DX; ++d) xinv[d][k][c] = lds_x[d * P + anc];
                    }
                    lw_old[k][c] = 0.0;
                }
            }
        }

        // --- fSamp / q1Samp, logGEv, tile max ---
        double lg[NK][2];
        double mx = -dinf();
        bool nan = false;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i0 = (k * NT + tid) * 2;
            double znv[DX][2];                         // vector state: the pair's normals of components d >= 1
            if constexpr (DX > 1) {
#pragma unroll
                for (int d = 1; d < DX; ++d) {
                    const u32x4 o = xdim_words((uint32_t)(k * NT + tid), (uint32_t)t, rep, d, key0, key1);
                    pair_normals(o.v0, o.v1, &lds_dtab, &znv[d][0], &znv[d][1]);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                double xn, l;
                const bool valid = (i0 + c) < a.N;
                if constexpr (VEC) {
                    double xv[DX], zv[DX], xnv[DX];
#pragma unroll
                    for (int d = 1; d < DX; ++d) { xv[d] = xinv[d][k][c]; zv[d] = znv[d][c]; }
                    l = lw_old[k][c] + series_vector_step<MODEL>(mc, t == 0, xin[k][c], zn[k][c], xv, zv, in, &xn, xnv, lds_etab);
#pragma unroll
                    for (int d = 1; d < DX; ++d) xcv[d][k][c] = valid ? xnv[d] : 0.0;
                } else l = lw_old[k][c] + scalar_step<MODEL>(mc, t == 0, xin[k][c], zn[k][c], in.y, in.z, in.zc, &xn, lds_etab);
                xcur[k][c] = valid ? xn : 0.0;
                lg[k][c] = valid ? l : -dinf();
                if (valid) { nan = nan || (l != l); mx = (l > mx) ? l : mx; }
            }
            lwcur[k][0] = lg[k][0]; lwcur[k][1] = lg[k][1];
        }
        const double mb = block_max_nanprop<NT>(mx, nan, lds_d2);    // barrier: every search / gather of this step is done

        // --- tile-local fixed-point weights, exact scan -> the next step's cdf (LDS) ---
        double q[NK][2], inc[NK][2], total;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i0 = (k * NT + tid) * 2;
            q[k][0] = (i0 < a.N) ? __builtin_rint(dexp_scaled_t(lg[k][0] - mb, kTileShift, lds_etab)) : 0.0;
            q[k][1] = (i0 + 1 < a.N) ? __builtin_rint(dexp_scaled_t(lg[k][1] - mb, kTileShift, lds_etab)) : 0.0;
        }
        block_scan_f64<NT, NK>(q, inc, total, lds_seg_c);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i0 = (k * NT + tid) * 2;
            store_slots<2>(lds_cdf + i0, inc[k]);
            store_slots<2>(lds_x + i0, xcur[k]);
#pragma unroll
            for (int d = 1; d < DX; ++d) store_slots<2>(lds_x + d * P + i0, xcv[d][k]);
            if constexpr (HIST) {                                     // row t of the history: slots i0, i0 + 1 < P <= Npad of every plane
                double* hx = the_hist(recarg...).hx + (size_t)t * DX * a.xplane + rowoff + i0;
                store_slots<2>(hx, xcur[k]);
#pragma unroll
                for (int d = 1; d < DX; ++d) store_slots<2>(hx + (size_t)d * a.xplane, xcv[d][k]);
            }
        }
        A_prev = total;
        mb_prev = mb;
        __syncthreads();                                              // cdf / x of step t visible to step t+1
        if constexpr (HIST) {
            if (the_rec(recarg...).fs.n > 0 || the_rec(recarg...).utraj)
                record_step_expectations<MODEL, NT>(the_rec(recarg...), a, mc, in, r, t, lds_x, P, lds_cdf, A_prev, mb_prev, lds_etab, lds_red);
        } else if constexpr (REC) record_step_expectations<MODEL, NT>(the_rec(recarg...), a, mc, in, r, t, lds_x, P, lds_cdf, A_prev, mb_prev, lds_etab, lds_red);
    }

    series_accounting<NT>(a, r, T, ms, A_prev, mb_prev, lds_etab);
    hand_over_state<NT, NK, 2, DX>(a, rowoff, &xcur[0][0], &xcv[0][0][0], &lwcur[0][0], lds_cdf, A_prev);
}

// ---------------------------------------------------------------------------------------------------------------------
// One particle per lane (N <= 512; measured slower than the pair kernel at 1024).  The pair kernel above runs one wave per SIMD, each carrying the ~1000-instruction
// chain of a particle PAIR, and is bound by dependent-instruction latency.  Here a lane owns ONE particle: the two lanes
// of a pair both evaluate the pair's Philox call and Box-Muller (lanes are free, instructions are not) and each keeps
// its own half, so a wave's chain per step is ~55 % of the pair kernel's and twice as many waves share a SIMD.
// grid = (R), block = NT = P particle slots (64 .. 512); a.small_ms: [R][Tcap][2] scratch.
// ---------------------------------------------------------------------------------------------------------------------
template <int MODEL, int NT, class... RECARG>
__global__ __launch_bounds__(NT) void k_filter_series_lane(const StepArgs a, const int T, const RECARG... recarg) {
    constexpr bool REC = sizeof...(RECARG) > 0;                // the recording instantiation: RECARG = SeriesRec (see k_filter_series_small)
    [[maybe_unused]] constexpr bool HIST = series_hist_v<RECARG...>;
    constexpr int P = NT;
    // A vector user model: as in the pair kernel; the pair index of the d >= 1 draws is tid >> 1 and the lane keeps half tid & 1.
    constexpr int DX = model_dx<MODEL>(), DY = model_dy<MODEL>();
    constexpr bool VEC = DX > 1 || DY > 1;
    __shared__ double lds_x[DX * P];
    __shared__ double lds_cdf[P];
    __shared__ double lds_seg[2][16];                 // the weights' scan and the spacings' scan, behind one barrier
    __shared__ double lds_d2[16];
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    double (*lds_red)[4] = nullptr;                    // recording: the wave sums of the expectations' numerators
    if constexpr (REC) {
        __shared__ double red[kMaxFunctionals + model_nh<MODEL>()][4];
        lds_red = red;
    }

    const int tid = threadIdx.x;
    load_log_table<NT>(&lds_dtab);
    load_exp_table<NT>(lds_etab);
    __syncthreads();
    const int r = blockIdx.x;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const uint32_t key0 = a.keyp[0], key1 = a.keyp[1];
    const size_t rowoff = (size_t)r * a.Npad;
    const ModelConst mc = a.mc[r];
    const bool multinomial_kind = a.resampler == RESAMP_MULTINOMIAL;
    const bool valid = tid < a.N;
    const int c = tid & 1;                            // which half of the pair (tid >> 1) this lane keeps
    double* ms = a.small_ms + (size_t)r * a.Tcap * 2;

    double xcur = 0.0, lwcur = 0.0;
    double xcv[DX];                                   // components d >= 1 of the lane's particle (slot 0 unused)
#pragma unroll
    for (int d = 1; d < DX; ++d) xcv[d] = 0.0;
    double A_prev = 0.0, mb_prev = 0.0;
    SeriesInputs<model_kcov<MODEL>(), DY> in_n;
    in_n.load_first(a, r);

    // The draws of a step do not depend on the filter's state, and at one or two waves per SIMD the step is a chain of dependent
    // instructions: the Philox call, the Box-Muller pair and the spacing of step t + 1 are therefore computed DURING step t, in the
    // block that waits for the search's LDS reads, and the spacings' block scan shares the barrier of the weights' scan
    // (block_scan_lanes_f64).  Carried to the next iteration: the normal, the spacing's inclusive sum and the total.  Same arithmetic.
    double zn_n = 0.0, le_n = 0.0, se_n = 1.0, qe_n = 0.0;
    double znv_n[DX];                                 // vector state: the lane's normals of components d >= 1, drawn with component 0's
    auto draw_xdim = [&](int tn, double (&out)[DX]) {
#pragma unroll
        for (int d = 1; d < DX; ++d) {
            const u32x4 o = xdim_words((uint32_t)(tid >> 1), (uint32_t)tn, rep, d, key0, key1);
            double z0, z1;
            pair_normals(o.v0, o.v1, &lds_dtab, &z0, &z1);
            out[d] = c ? z1 : z0;
        }
    };
    auto draw_for = [&](int tn) {
        if constexpr (DX > 1 && SSME_LANE_XDIM_AHEAD) draw_xdim(tn, znv_n);
        // the pair's Philox call: words 0-1 -> Box-Muller (this lane keeps cos or sin), words 2 / 3 -> this lane's spacing
        const u32x4 o = pair_words((uint32_t)(tid >> 1), (uint32_t)tn, rep, key0, key1);
        double z0, z1;
        pair_normals(o.v0, o.v1, &lds_dtab, &z0, &z1);
        zn_n = c ? z1 : z0;
        const bool mult = multinomial_kind && tn > 0 && (tn % a.resamp_sched == 0);
        const double e = -dlog_u32(u01_mid32(c ? o.v3 : o.v2), lds_dtab.log);
        qe_n = (valid && mult) ? __builtin_rint(e * 34359738368.0 /* 2^35 */) : 0.0;
    };
    draw_for(0);

    for (int t = 0; t < T; ++t) {
        const auto in = in_n;
        in_n.request(a, r, t + 1, T);
        const double zn = zn_n, le = le_n, se = se_n;
        double znv[DX], xinv[DX];
        if constexpr (DX > 1) {
            if constexpr (SSME_LANE_XDIM_AHEAD) {
#pragma unroll
                for (int d = 1; d < DX; ++d) znv[d] = znv_n[d];
            }
#pragma unroll
            for (int d = 1; d < DX; ++d) xinv[d] = (t == 0) ? 0.0 : xcv[d];       // nothing is read at t = 0; the lane's own otherwise
        }
        const bool resampled = (t > 0) && (t % a.resamp_sched == 0);

        // --- level-2 of step t-1: one_tile_level2's text, written out.  Called as the function (struct or reference results) this
        //     kernel took 0.03 to 0.06 us per step longer at N = 500 (profiles/small_series_refactor.txt, section 4) ---
        double S = 0.0, R0 = 0.0;
        if (t > 0) {
            const double m = (mb_prev != mb_prev) ? dnan() : mb_prev;
            const double dm = mb_prev - m;
            const int sh = a.rshift - kTileShift;
            const double Ap = (dm == 0.0 && sh == 0) ? __builtin_rint(A_prev) : __builtin_rint(A_prev * dexp_scaled_t(dm, sh, lds_etab));
            S = Ap;
            R0 = A_prev / Ap;
            if (tid == 0) { ms[2 * (t - 1)] = m; ms[2 * (t - 1) + 1] = S; }
        }

        double xin = 0.0, lw_old = 0.0;
        if (t == 0) {
            draw_for(t + 1);
        } else if (!resampled) {
            xin = xcur; lw_old = lwcur;
            draw_for(t + 1);
        } else {
            // --- target, search in the cdf, gather ---
            double tau;
            if (a.resampler == RESAMP_MULTINOMIAL) {
                const double t_scale = S / in.G;
                const double ratio = in.gam / se;
                const double t1 = ratio * le;
                const double t2 = in.pgam + t1;
                tau = __builtin_ceil(t2 * t_scale);
            } else {
                // the division ahead of the draw, and the draw in the branch that needs it: with both draws joined before one
                // call of target_of the step took 0.08 us longer
                const double t_scale = S / (double)a.N;
                if (a.resampler == RESAMP_SYSTEMATIC) {
                    tau = target_of(RESAMP_SYSTEMATIC, tid, 0.0, systematic_u0((uint32_t)t, rep, key0, key1), t_scale, S);
                } else {      // the pair's Philox call; this lane keeps its half
                    const u32x4 o = philox4x32_10((uint32_t)(tid >> 1), (uint32_t)t, rep, STREAM_RESAMP, key0, key1);
                    tau = target_of(a.resampler, tid, c ? u01_co(o.v2, o.v3) : u01_co(o.v0, o.v1), 0.0, t_scale, S);
                }
            }
            const double tl[1] = {__builtin_ceil((tau - 0.0) * R0)};
            int jj[1];
            count_less_radix8<P, 1>(lds_cdf, tl, jj);
            draw_for(t + 1);                                   // fills the waits of the descent's LDS reads and of the gather
            const int anc = jj[0] < a.N - 1 ? jj[0] : a.N - 1;
            if (a.anc && valid) a.anc[rowoff + tid] = (uint32_t)anc;
            if constexpr (HIST) { if (valid) the_hist(recarg...).hanc[(size_t)t * a.xplane + rowoff + tid] = (uint32_t)anc; }
            xin = lds_x[anc];
            if constexpr (DX > 1) {                            // every plane at the one clamped ancestor
#pragma unroll
                for (int d = 1; d < DX; ++d) xinv[d] = lds_x[d * P + anc];
            }
        }

        // --- fSamp / q1Samp, logGEv, tile max ---
        double xn, l;
        if constexpr (VEC) {
            double xnv[DX];
            if constexpr (DX > 1 && !SSME_LANE_XDIM_AHEAD) draw_xdim(t, znv);
            l = lw_old + series_vector_step<MODEL>(mc, t == 0, xin, zn, xinv, znv, in, &xn, xnv, lds_etab);
#pragma unroll
            for (int d = 1; d < DX; ++d) xcv[d] = valid ? xnv[d] : 0.0;
        } else l = lw_old + scalar_step<MODEL>(mc, t == 0, xin, zn, in.y, in.z, in.zc, &xn, lds_etab);
        xcur = valid ? xn : 0.0;
        const double lg = valid ? l : -dinf();
        lwcur = lg;
        const bool nan = valid && (l != l);
        const double mx = (valid && l > -dinf()) ? l : -dinf();
        const double mb = block_max_nanprop<NT>(mx, nan, lds_d2);    // barrier: every search / gather of this step is done

        // --- tile-local fixed-point weights, exact scan -> the next step's cdf (LDS); the next step's spacings ride along ---
        const double sv[2] = {valid ? __builtin_rint(dexp_scaled_t(lg - mb, kTileShift, lds_etab)) : 0.0, qe_n};
        double sinc[2], stot[2];
        block_scan_lanes_f64<NT, 2>(sv, sinc, stot, lds_seg);
        le_n = sinc[1]; se_n = stot[1];
        lds_cdf[tid] = sinc[0];
        lds_x[tid] = xcur;
#pragma unroll
        for (int d = 1; d < DX; ++d) lds_x[d * P + tid] = xcv[d];
        if constexpr (HIST) {                                         // row t of the history: slot tid < P <= Npad of every plane
            double* hx = the_hist(recarg...).hx + (size_t)t * DX * a.xplane + rowoff + tid;
            *hx = xcur;
#pragma unroll
            for (int d = 1; d < DX; ++d) hx[(size_t)d * a.xplane] = xcv[d];
        }
        A_prev = stot[0];
        mb_prev = mb;
        __syncthreads();                                              // cdf / x of step t visible to step t+1
        if constexpr (HIST) {
            if (the_rec(recarg...).fs.n > 0 || the_rec(recarg...).utraj)
                record_step_expectations<MODEL, NT>(the_rec(recarg...), a, mc, in, r, t, lds_x, P, lds_cdf, A_prev, mb_prev, lds_etab, lds_red);
        } else if constexpr (REC) record_step_expectations<MODEL, NT>(the_rec(recarg...), a, mc, in, r, t, lds_x, P, lds_cdf, A_prev, mb_prev, lds_etab, lds_red);
    }

    series_accounting<NT>(a, r, T, ms, A_prev, mb_prev, lds_etab);
    hand_over_state<NT, 1, 1, DX>(a, rowoff, &xcur, xcv, &lwcur, lds_cdf, A_prev);
}

}  // namespace ssme
