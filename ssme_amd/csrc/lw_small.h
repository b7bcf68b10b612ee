// lw_small.h -- whole-series kernel for Liu-West filters that fit one tile (N <= 2048): steps 1 .. T-1 of
// LWFilterWithCovs::filter / LWFilter2WithCovs::filter run inside ONE launch, one workgroup per filter (grid = R).
// k_lw_init (step 0) and the Gamma tables of both draws run in front of it as they do on the tiled route.
//
// The arithmetic is that of k_lw_stage1, the fused mid of k_lw_stage2 and k_lw_stage2 at B = 1, operation for operation, with
// barriers where the launches were: same thread-to-particle map (512 threads, pair k * 512 + tid, NK = 2), same Philox counters,
// same targets (multinomial_targets), the one-tile level-2 of pf_small.h (one_tile_level2 == level2_scan at B = 1), a count over
// the exact integer cdf (count_less_radix8: the count staged_search returns), the moment sums in stage 1's tree and the single-tile
// total as the fused mid adds it (0.0 + partial in lane 0, carried through wave_incl_scan_f64 over 63 zero lanes: a moment that
// is exactly -0.0 leaves as +0.0 on both routes).  The two routes are bit-identical (tests/test_lw_series_gpu.py).
//
// State in dynamic LDS (112 KiB; one workgroup per CU): theta records [2048][4], x [2048], ONE integer cdf [2048] (cdf B of the
// step before, then cdf A, then the new cdf B), g1 [2048] (form 0: logG(y | propMu) of the resampled particle; form 1: the carried
// log-weight).  There is one copy of the population: a thread reads all of its sources into registers, passes a barrier, then
// stores (the resampling gather and the k gather alike).  The second-stage log-weights stay in registers (schedules m_rs > 1
// carry them).  After the loop the kernel accounts step T-1 as k_lw_finalize does and writes back what a later call reads.
//
// Recording instantiations (ssme_lw_set_series_expectations): the same kernel with a third argument,
// LwSeriesRec, writes the eight filtered expectations of EVERY step (lw_record_expectations) with the bits of the step API's
// read-out, k_lw_param_partials + k_lw_param_means.  The instantiations without it are untouched by that code.
#pragma once
#include "lw_kernels.h"
#include "pf_small.h"

namespace ssme {

constexpr size_t kLwSeriesLdsBytes = sizeof(double) * (size_t)kTile * (kDP + 3);      // theta | x | cdf | g1

// the inputs of a step that do not depend on the filter's state, requested one step ahead (uniform scalar loads)
struct LwSeriesInputs {
    double y, z;
    double gamB, pgamB, GB;          // resampling draw (Gamma tables B)
    double gamA, pgamA, GA;          // k draw (tables A)
    __device__ __forceinline__ void load(const LwArgs& a, int r, int t, int T) {
        if (t >= T) return;
        y = a.y[t];
        z = a.z ? a.z[t] : 0.0;
        const size_t g = (size_t)t * a.R + r;          // B = 1
        if (t % a.resamp_sched == 0) { gamB = a.gamB[g]; pgamB = a.pgamB[g]; GB = a.gtotB[g]; }
        if (a.form == 0) { gamA = a.gamA[g]; pgamA = a.pgamA[g]; GA = a.gtotA[g]; }
    }
};

// lw_store_cdf's arithmetic with the cdf kept in LDS: tile maximum (one barrier), `mid()` between the two barriers, fixed-point
// weights, exact scan (one barrier), store.  Returns the tile sum and the tile maximum.
template <class MID>
__device__ __forceinline__ void lw_cdf_to_lds(const double (&lg)[2][2], double* lds_cdf, double* lds_d, double* lds_seg,
                                              const ExpTabEntry* etab, double& total, double& mb, MID mid) {
    constexpr int NT = kLwNT, NK = 2;
    const int tid = threadIdx.x;
    double mx = -dinf();
    bool nan = false;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int c = 0; c < 2; ++c) { const double l = lg[k][c]; nan = nan || (l != l); mx = (l > mx) ? l : mx; }
    }
    mb = block_max_nanprop<NT>(mx, nan, lds_d);
    mid();
    double q[NK][2], inc[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        q[k][0] = __builtin_rint(dexp_scaled_t(lg[k][0] - mb, kTileShift, etab));
        q[k][1] = __builtin_rint(dexp_scaled_t(lg[k][1] - mb, kTileShift, etab));
    }
    block_scan_f64<NT, NK>(q, inc, total, lds_seg);
#pragma unroll
    for (int k = 0; k < NK; ++k) *reinterpret_cast<double2*>(lds_cdf + (k * NT + tid) * 2) = make_double2(inc[k][0], inc[k][1]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Recorded series: row t of the trajectory is what k_lw_param_partials + k_lw_param_means form from memory after step t of the
// step API.  At the recording points LDS holds what they read -- the particles, the transformed theta records and the tile-local
// integer cdf of step t -- and mb is the tile maximum.  The sums follow THEIR trees at B = 1, not this kernel's 512 x 2 x 2 map:
//   terms      virtual thread v of 256 adds particles v, v + 256, ... < N in this order, w = (cdf_j - cdf_{j-1}) dexp(mb - m) with
//              m = mb through the NaN-propagating maximum (the scale is evaluated: mb = +-inf gives NaN rows there and here);
//              lw_expect_terms is the one statement of the eight terms
//   combining  the 64 virtual lanes of a wave by the xor butterfly 32 .. 1, the four waves as ((w0 + w1) + w2) + w3
//   final      one tile: 0.0 + partial, then lw_expect_store (the quotients and 42 (den / den))
// The first 256 threads play the virtual threads.  One barrier in front of the reads (the cdf stores of this step), one before the
// wave sums are combined; every later store to lds_x / lds_th / lds_cdf lies behind the second one.  LDS grows by 4 x 8 doubles.
// ---------------------------------------------------------------------------------------------------------------------
struct LwSeriesRec {
    double* traj;              // [T][R][8]
};
__device__ __forceinline__ const LwSeriesRec& the_lw_rec(const LwSeriesRec& rec) { return rec; }      // the one element of RECARG...

// the wave sums of the running sums Q0 .. Q1-1 (the first 256 threads)
template <bool FT, int Q0, int Q1>
__device__ __forceinline__ void lw_record_pass(const LwArgs& a, const double* lds_x, const double* lds_th, const double* lds_cdf, double mb,
                                               const ExpTabEntry* etab, double (*lds_n)[kLwNExp]) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));          // opaque: the pass's addresses are formed here, not hoisted out of the time loop (6 VGPRs spill otherwise)
    const double m = (mb != mb) ? dnan() : mb;
    const double scale = dexp(mb - m);
    double acc[kLwNExp] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = tid; j < a.N; j += kThreads) {
        const double c1 = lds_cdf[j];
        const double c0 = j ? lds_cdf[j - 1] : 0.0;
        const double w = (c1 - c0) * scale;
        const double xv = lds_x[j];
        double trec[kDP];
        th_load(lds_th, (size_t)j, trec);
        lw_expect_terms<Q0, Q1>(acc, w, xv, trec, [&](int d) { return lw_trans_kind<FT>(a.trans, d); }, etab);
    }
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
        const double v = wave_sum_xor(acc[q]);
        if ((tid & 63) == 0) lds_n[tid >> 6][q] = v;
    }
}

template <bool FT>
__device__ __forceinline__ void lw_record_expectations(const LwSeriesRec& rec, const LwArgs& a, int r, int t, const double* lds_x,
                                                       const double* lds_th, const double* lds_cdf, double mb, const ExpTabEntry* etab,
                                                       double (*lds_n)[kLwNExp]) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < kThreads) {
        // three passes (phi, mu | sigma, rho, the weight total | the state): the kernel has no registers to spare, and in one pass
        // or two the FT instantiation spills 2 VGPRs (profiles/lw_series_expectations_kernels.txt).  Every sum is its own chain, so
        // the passes change no bit.
        lw_record_pass<FT, 0, 2>(a, lds_x, lds_th, lds_cdf, mb, etab, lds_n);
        lw_record_pass<FT, 2, kDP + 1>(a, lds_x, lds_th, lds_cdf, mb, etab, lds_n);
        lw_record_pass<FT, kDP + 1, kLwNExp>(a, lds_x, lds_th, lds_cdf, mb, etab, lds_n);
    }
    __syncthreads();
    if (tid < kLwNExp) {
        const double part = ((lds_n[0][tid] + lds_n[1][tid]) + lds_n[2][tid]) + lds_n[3][tid];
        const double wsum = ((lds_n[0][kDP] + lds_n[1][kDP]) + lds_n[2][kDP]) + lds_n[3][kDP];
        lw_expect_store(rec.traj + ((size_t)t * a.R + r) * kLwNExp, tid, 0.0 + part, 0.0 + wsum);
    }
}

// grid = (R), block = 512, dynamic LDS = kLwSeriesLdsBytes.  a.t / yi / gi are ignored (t = yi = gi = 1 .. T-1); a.per_step
// receives the T log conditional likelihoods, a.scal the sums; a.xB / thB / cdfB / tsumB / tmaxB (/ lwB) hold step 0 on entry
// (k_lw_init) and the population after step T-1 on exit.
// RECARG: empty, or LwSeriesRec for the recording instantiation, which takes it as a third kernel argument; `if constexpr` keeps every
// line of the recording out of the other instantiation, whose arguments and code are what they were without it.
template <bool FT, class... RECARG>
__global__ __launch_bounds__(kLwNT) void k_lw_series(const LwArgs a, const int T, const RECARG... recarg) {
    constexpr bool REC = sizeof...(RECARG) > 0;
    constexpr int NT = kLwNT, NK = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lds_th = reinterpret_cast<double*>(smem);       // [2048][4]
    double* lds_x = lds_th + (size_t)kTile * kDP;
    double* lds_cdf = lds_x + kTile;
    double* lds_g1 = lds_cdf + kTile;
    __shared__ double lds_seg_a[16];                        // spacings of the resampling draw
    __shared__ double lds_seg_k[16];                        // spacings of the k draw
    __shared__ double lds_seg_cA[16];
    __shared__ double lds_seg_cB[16];
    __shared__ double lds_dA[16];
    __shared__ double lds_dB[16];
    __shared__ double lds_mom[8][4][16];                    // [wave][DPP row][moment]: row totals of the 14 moment sums
    __shared__ double lds_sums[16];
    __shared__ double lds_prop[16];
    __shared__ double lds_ms[2];
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    double (*lds_n)[kLwNExp] = nullptr;                     // recording: the wave sums of the eight expectation sums
    if constexpr (REC) {
        __shared__ double red[4][kLwNExp];
        lds_n = red;
    }
    load_log_table<NT>(&lds_dtab);
    load_exp_table<NT>(lds_etab);

    const int tid = threadIdx.x, r = blockIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const size_t rowoff = (size_t)r * a.Npad;
    const int N = a.N;

    // step 0 as k_lw_init left it: every thread takes its own slots
    double lgB[NK][2];                                      // second-stage log-weights of the last step
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i0 = (k * NT + tid) * 2;
        *reinterpret_cast<double2*>(lds_x + i0) = *reinterpret_cast<const double2*>(a.xB + rowoff + i0);
        *reinterpret_cast<double2*>(lds_cdf + i0) = *reinterpret_cast<const double2*>(a.cdfB + rowoff + i0);
        const double2* ts = reinterpret_cast<const double2*>(a.thB + (rowoff + (size_t)i0) * kDP);
        double2* td = reinterpret_cast<double2*>(lds_th + (size_t)i0 * kDP);
#pragma unroll
        for (int u = 0; u < 4; ++u) td[u] = ts[u];
        lgB[k][0] = 0.0; lgB[k][1] = 0.0;
        if (a.lwB) { const double2 w = *reinterpret_cast<const double2*>(a.lwB + rowoff + i0); lgB[k][0] = w.x; lgB[k][1] = w.y; }
    }
    double A_prev = a.tsumB[(size_t)r * a.Bs], mb_prev = a.tmaxB[(size_t)r * a.Bs];
    // accounting state (thread 0's copy is the one that counts)
    double prev = a.scal[r].prev, loglik = a.scal[r].loglik, lse1 = a.scal[r].lse1;
    LwSeriesInputs in_n;
    in_n.y = 0.0; in_n.z = 0.0; in_n.gamB = 0.0; in_n.pgamB = 0.0; in_n.GB = 1.0; in_n.gamA = 0.0; in_n.pgamA = 0.0; in_n.GA = 1.0;
    in_n.load(a, r, 1, T);
    __syncthreads();
    if constexpr (REC) lw_record_expectations<FT>(the_lw_rec(recarg...), a, r, 0, lds_x, lds_th, lds_cdf, mb_prev, lds_etab, lds_n);

    for (int t = 1; t < T; ++t) {
        const LwSeriesInputs in = in_n;
        in_n.load(a, r, t + 1, T);
        const double y = in.y, z = in.z;
        const bool resampled = (t % a.resamp_sched) == 0;

        // ---- stage 1 ----
        // level-2 of the second-stage weights of step t-1 and its accounting (k_lw_stage1's formula)
        const Level2 lB = one_tile_level2(A_prev, mb_prev, a.rshift, lds_etab, lds_ms);
        if (tid == 0) {
            const double lseB = lse_of(lB.m, lB.S, a.rshift);
            const double ll = (a.form == 0 && t > 1) ? (lseB + lse1) - 2.0 * prev : lseB - prev;
            loglik = loglik + ll;
            prev = resampled ? a.logN : lseB;
            if (a.per_step) a.per_step[(size_t)r * a.Tcap + (t - 1)] = ll;
        }
        int anc[NK][2];
        if (resampled) {
            u32x4 draw[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k)
                draw[k] = philox4x32_10((uint32_t)(k * NT + tid), (uint32_t)t, rep, STREAM_RESAMP, a.key0, a.key1);
            double tau[NK][2];
            multinomial_targets<NT, NK, kTile>([&](int k, double& e0, double& e1) { pair_spacings(draw[k], lds_dtab.log, &e0, &e1); },
                                               0, N, in.gamB, in.pgamB, lB.S / in.GB, lds_seg_a, tau);     // (a barrier inside)
            const double tl[4] = {__builtin_ceil((tau[0][0] - 0.0) * lB.R0), __builtin_ceil((tau[0][1] - 0.0) * lB.R0),
                                  __builtin_ceil((tau[1][0] - 0.0) * lB.R0), __builtin_ceil((tau[1][1] - 0.0) * lB.R0)};
            int jj[4];
            count_less_radix8<kTile, 4>(lds_cdf, tl, jj);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) anc[k][c] = jj[2 * k + c] < N - 1 ? jj[2 * k + c] : N - 1;
            }
        } else {
            __syncthreads();                                // the stores of step t-1 (the resampling draw has this barrier in its scan)
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) { const int i = (k * NT + tid) * 2 + c; anc[k][c] = i < N - 1 ? i : N - 1; }
            }
        }
        // all four ancestors' records into registers, then (behind a barrier) back to the thread's own slots
        double xall[NK][2], ttall[NK][kDP][2];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = anc[k][c];
                xall[k][c] = lds_x[j];
                double trec[kDP];
                th_load(lds_th, (size_t)j, trec);
#pragma unroll
                for (int d = 0; d < kDP; ++d) ttall[k][d][c] = trec[d];
            }
        }
        if (resampled) __syncthreads();
        double lg[NK][2];
        double fold[kNMom][2];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i0 = (k * NT + tid) * 2;
            double xo[2], tt[kDP][2], g1[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                xo[c] = xall[k][c];
#pragma unroll
                for (int d = 0; d < kDP; ++d) tt[d][c] = ttall[k][d][c];
                if (a.anc && t == T - 1 && i0 + c < N) a.anc[rowoff + i0 + c] = (uint32_t)anc[k][c];
            }
            if (resampled) {
                *reinterpret_cast<double2*>(lds_x + i0) = make_double2(xo[0], xo[1]);
                th_store_pair(lds_th, (size_t)i0, tt);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                double tu[kDP];
#pragma unroll
                for (int d = 0; d < kDP; ++d) tu[d] = tr_inv(lw_trans_kind<FT>(a.trans, d), tt[d][c], lds_etab);
                const bool valid = (i0 + c) < N;
                const double lw_old = (resampled || !valid) ? 0.0 : lgB[k][c];
                g1[c] = (a.form == 0) ? lw_logg(y, lw_propmu(xo[c], z, tu, lds_etab), lds_etab) : lw_old;
                lg[k][c] = (a.form == 0) ? lw_old + g1[c] : lw_old;
                if (!valid) { lg[k][c] = -dinf(); g1[c] = -dinf(); }
                int q = 0;
#pragma unroll
                for (int d = 0; d < kDP; ++d) { const double v = valid ? tt[d][c] : 0.0; fold[q][c] = (k == 0) ? v : fold[q][c] + v; ++q; }
#pragma unroll
                for (int d = 0; d < kDP; ++d) {
#pragma unroll
                    for (int e = 0; e <= d; ++e) { const double v = valid ? tt[d][c] * tt[e][c] : 0.0; fold[q][c] = (k == 0) ? v : fold[q][c] + v; ++q; }
                }
            }
            *reinterpret_cast<double2*>(lds_g1 + i0) = make_double2(g1[0], g1[1]);
        }
        {
            double v[16];
#pragma unroll
            for (int q = 0; q < kNMom; ++q) v[q] = fold[q][0] + fold[q][1];
            v[14] = 0.0; v[15] = 0.0;
            const double rowtot = lw_row_tree14(v, tid);
            lds_mom[tid >> 6][(tid >> 4) & 3][lw_row_tree_index(tid & 15)] = rowtot;
        }
        // between the two barriers of cdf A (form 1: two plain barriers): the eight waves in order, then the single-tile total as
        // the fused mid adds it -- wave w takes moments w and w + 8
        auto tile_totals = [&]() {
#pragma unroll
            for (int qi = 0; qi < 2; ++qi) {
                const int q = wave + 8 * qi;
                double acc = 0.0;
                if (q < kNMom && lane == 0) {
                    double s = 0.0;
#pragma unroll
                    for (int w = 0; w < 8; ++w) s = s + ((lds_mom[w][3][q] + lds_mom[w][2][q]) + (lds_mom[w][1][q] + lds_mom[w][0][q]));
                    acc = acc + s;
                }
                const double sw = wave_incl_scan_f64(acc);
                if (lane == 63 && q < kNMom) lds_sums[q] = sw;
            }
        };
        double tsumA = 0.0, tmaxA = 0.0;
        if (a.form == 0) lw_cdf_to_lds(lg, lds_cdf, lds_dA, lds_seg_cA, lds_etab, tsumA, tmaxA, tile_totals);
        else { __syncthreads(); tile_totals(); __syncthreads(); }

        // ---- mid + stage 2 ----
        Level2 lA = {0.0, 0.0, 0.0};
        if (a.form == 0) lA = one_tile_level2(tsumA, tmaxA, a.rshift, lds_etab, lds_ms);
        if (tid == 0) {
            lw_proposal_components(lds_sums, N, a.a_shrink, lds_prop);
            if (a.form == 0) lse1 = lse_of(lA.m, lA.S, a.rshift);
        }
        u32x4 draw[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k)
            draw[k] = philox4x32_10((uint32_t)(k * NT + tid), (uint32_t)t, rep, STREAM_LW_K, a.key0, a.key1);
        int kk[NK][2];
        if (a.form == 0) {
            double tau[NK][2];
            multinomial_targets<NT, NK, kTile>([&](int k, double& e0, double& e1) { pair_spacings(draw[k], lds_dtab.log, &e0, &e1); },
                                               0, N, in.gamA, in.pgamA, lA.S / in.GA, lds_seg_k, tau);     // (a barrier inside: cdf A, lds_prop)
            const double tl[4] = {__builtin_ceil((tau[0][0] - 0.0) * lA.R0), __builtin_ceil((tau[0][1] - 0.0) * lA.R0),
                                  __builtin_ceil((tau[1][0] - 0.0) * lA.R0), __builtin_ceil((tau[1][1] - 0.0) * lA.R0)};
            int jj[4];
            count_less_radix8<kTile, 4>(lds_cdf, tl, jj);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) kk[k][c] = jj[2 * k + c] < N - 1 ? jj[2 * k + c] : N - 1;
            }
        } else {
            __syncthreads();                                // lds_prop
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) { const int i = (k * NT + tid) * 2 + c; kk[k][c] = i < N - 1 ? i : N - 1; }
            }
        }
        double prop[16];
#pragma unroll
        for (int q = 0; q < 14; ++q) prop[q] = readfirstlane_f64(lds_prop[q]);
        // the k gather: every source into registers, a barrier, then the stores
        double kx[NK][2], kg[NK][2], kth[NK][2][kDP];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = kk[k][c];
                kx[k][c] = lds_x[j];
                kg[k][c] = lds_g1[j];
                th_load(lds_th, (size_t)j, kth[k][c]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i0 = (k * NT + tid) * 2;
            double zs[2];
            pair_normals(draw[k].v0, draw[k].v1, &lds_dtab, &zs[0], &zs[1]);
            double xo[2], tho[kDP][2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int i = i0 + c;
                const double xk = kx[k][c], lw1k = kg[k][c];
                double e[kDP];
                {
                    const u32x4 o1 = philox4x32_10((uint32_t)i, (uint32_t)t, rep, STREAM_LW_JIT, a.key0, a.key1);
                    pair_normals(o1.v0, o1.v1, &lds_dtab, &e[0], &e[1]);
                    pair_normals(o1.v2, o1.v3, &lds_dtab, &e[2], &e[3]);
                }
                double tu[kDP];
                int q = kDP;
#pragma unroll
                for (int d = 0; d < kDP; ++d) {
                    const double thk = kth[k][c][d];
                    const double mm = a.a_shrink * thk + (1.0 - a.a_shrink) * prop[d];
                    double acc = 0.0;
#pragma unroll
                    for (int w = 0; w <= d; ++w) { acc = acc + prop[q] * e[w]; ++q; }
                    tho[d][c] = mm + acc;
                    tu[d] = tr_inv(lw_trans_kind<FT>(a.trans, d), tho[d][c], lds_etab);
                }
                const double mean = (tu[1] + tu[0] * (xk - tu[1])) + ((z * tu[3]) * tu[2]) * dexp_scaled_t(-0.5 * xk, 0, lds_etab);
                xo[c] = mean + zs[c] * (tu[2] * dsqrt(1.0 - tu[3] * tu[3]));
                lgB[k][c] = (a.form == 0) ? lw_logg(y, xo[c], lds_etab) - lw1k : lw1k + lw_logg(y, xo[c], lds_etab);
                if (a.kidx && t == T - 1 && i < N) a.kidx[rowoff + i] = (uint32_t)kk[k][c];
                if (i >= N) { xo[c] = 0.0; lgB[k][c] = -dinf(); }
            }
            *reinterpret_cast<double2*>(lds_x + i0) = make_double2(xo[0], xo[1]);
            th_store_pair(lds_th, (size_t)i0, tho);
        }
        lw_cdf_to_lds(lgB, lds_cdf, lds_dB, lds_seg_cB, lds_etab, A_prev, mb_prev, []() {});
        // (no closing barrier: the next step's first use of these stores is behind the barrier of its resampling draw's scan, or
        // the one it passes instead)
        if constexpr (REC) lw_record_expectations<FT>(the_lw_rec(recarg...), a, r, t, lds_x, lds_th, lds_cdf, mb_prev, lds_etab, lds_n);
    }
    __syncthreads();

    // ---- hand-over: account step T-1 as k_lw_finalize does, then everything a later call reads ----
    const Level2 lF = one_tile_level2(A_prev, mb_prev, a.rshift, lds_etab, lds_ms);
    if (tid == 0) {
        LwScalars* sc = a.scal + r;
        const int t = T - 1;
        const double lseB = lse_of(lF.m, lF.S, a.rshift);
        const double ll = (a.form == 0 && t > 0) ? (lseB + lse1) - 2.0 * prev : lseB - prev;
        sc->mB = lF.m; sc->SB = lF.S; sc->last_ll = ll; sc->loglik = loglik + ll;
        sc->prev = ((t + 1) % a.resamp_sched == 0) ? a.logN : lseB;
        if (a.form == 0 && T > 1) sc->lse1 = lse1;
        if (a.per_step) a.per_step[(size_t)r * a.Tcap + t] = ll;
        a.tsumB[(size_t)r * a.Bs] = A_prev;
        a.tmaxB[(size_t)r * a.Bs] = mb_prev;
    }
    if (T > 1 && tid < 14) a.prop[(size_t)r * 16 + tid] = lds_prop[tid];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i0 = (k * NT + tid) * 2;
        *reinterpret_cast<double2*>(a.xB + rowoff + i0) = *reinterpret_cast<const double2*>(lds_x + i0);
        *reinterpret_cast<double2*>(a.cdfB + rowoff + i0) = *reinterpret_cast<const double2*>(lds_cdf + i0);
        double2* td = reinterpret_cast<double2*>(a.thB + (rowoff + (size_t)i0) * kDP);
        const double2* ts = reinterpret_cast<const double2*>(lds_th + (size_t)i0 * kDP);
#pragma unroll
        for (int u = 0; u < 4; ++u) td[u] = ts[u];
        if (a.lwB) *reinterpret_cast<double2*>(a.lwB + rowoff + i0) = make_double2(lgB[k][0], lgB[k][1]);
    }
}

}  // namespace ssme
