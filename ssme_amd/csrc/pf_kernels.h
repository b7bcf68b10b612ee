// pf_kernels.h -- HIP kernels of the bootstrap-particle-filter step for gfx950 (wave64).
//
// One filter step = ONE kernel, k_filter_step.  Per 2048-particle tile:
//   level-2: rescale + exact scan of the previous step's tile sums (per-tile weight scales, so no
//            global max pass and no separate normalisation kernel)       twin liu_west_filter.h:1652-1659
//   resampling targets (sorted uniforms by exponential spacings)          twin :105-139
//   search of the previous step's integer weight cdf, tiles staged in LDS  twin :112-139
//   gather ancestor state, fSamp, logGEv                                  example/univ_svol_bootstrap_filter.h:74-86
//   tile max, q = rne(exp(logw - max_tile) 2^41), exact integer tile scan  twin :96-104
// It replaces pf::BSFilter::filter (call site example/estimate_univ_svol.h:124).
//
// Particles are a structure of arrays in HBM: x[R][Npad] (fp64, ping-pong), cdf[R][Npad] (fixed point:
// integers < 2^53 held exactly in fp64, ping-pong), per-tile sums/maxima; one row per filter.  A tile is 2048 consecutive
// particles = NT threads x (1024/NT) pairs, so every streaming access is one 16-byte load/store
// per lane, fully coalesced.  Log-weights never leave registers (unless resampling is not every
// step, or in debug mode).
//
// The weight cdf is EXACT integer arithmetic: every value is an integer below
// 2^53 carried in an fp64 register, so v_add_f64 adds exactly; sums are associative, the cdf is
// monotone by construction and the ancestor of a target is an integer count -- independent of scan
// tree, search strategy and block shape.
#pragma once
#include "ssme_math.h"
#include "model_api.h"

namespace ssme {

typedef unsigned long long u64;

constexpr int kThreads = 256;            // helper kernels; KA/KR are templated on their block size
constexpr int kWave = 64;
constexpr int kRow = 512;
constexpr int kTile = 2048;                // large tile: N <= 2048 (one-tile series kernel), N > 2^18, Liu-West, sharded filters
constexpr int kTileSmall = 512;
constexpr int kTileMid = 1024;            // small tile: 2048 < N <= 2^18, so that a mid-size filter spreads over the chip (N = 2^16: 128 workgroups)
constexpr int kMaxTilesPerFilter = 2048;   // in-kernel level-2 (one entry per thread at NT = 512 .. four at 512 threads)
constexpr int kSplitLevel2Above = 1024;    // measured (profiles/r02_level2_split.txt): in-kernel 24.7 vs split 25.4 us at 768 tiles, equal at 1024, 67.9 vs 43.3 at 1536
constexpr int kL2Scratch = 64;             // doubles of l2_work per filter after the block-local scans: [0, 16) block totals, [16] m,
constexpr int kL2Offsets = 32;             //   [kL2Offsets, + 17) exclusive offsets of the blocks and S' (l2_inkernel)
constexpr int kMaxTilesSplit = 16384;      // split level-2 (k_level2_plan + k_filter_step<.., true>): N <= 2^25
#ifndef SSME_SEARCH_WINDOW
#define SSME_SEARCH_WINDOW 16              // staged_search: a pair's second target is counted in a window of this many elements (0: off)
#endif
constexpr int kStageTiles = 3;             // cdf tiles staged in LDS per output tile
constexpr int kEShift = 35;                // exponential spacings: qE = rne(E * 2^35)
constexpr int kTileShift = 41;             // tile-local fixed point: q = rne(exp(logw - m_tile) * 2^41), tile sums <= 2^52

enum { RESAMP_MULTINOMIAL = 0, RESAMP_SYSTEMATIC = 1, RESAMP_STRATIFIED = 2, RESAMP_MULTINOMIAL_IID = 3 };

#define SSME_HALF_LOG_2PI 0.91893853320467274178

#ifdef SSME_ABLATE
#define ABL(a, bit) (((a).ablate >> (bit)) & 1)
// diagnostic phase stamps (100 MHz constant clock), one row of 16 per block; never in the product build
#define STAMP(a, i) do { if ((a).stamps && threadIdx.x == 0) (a).stamps[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ABL(a, bit) 0
#define STAMP(a, i) do {} while (0)
#endif

// Per-filter scalars living in device memory.
struct FilterScalars {
    double m;        // max log-weight of the last step (NaN if any log-weight is NaN)
    double S;        // exact integer sum of the rescaled tile sums of the last step
    double prev;     // m_old + log S_old (log N after a resampling step)
    double loglik;   // running sum of log p(y_t | y_{1:t-1})
    double last_ll;  // last log conditional likelihood
    double pad[3];
};

struct StepArgs {
    const double* x_in;        // [R][Npad] particles of step t-1 (pre-resampling)
    double* x_out;             // [R][Npad]
    double* logw;              // [R][Npad] or null: only kept when resampling is not every step, or in debug mode
    const double* cdf_in;      // [R][Npad] tile-local inclusive integer sums of q, step t-1
    double* cdf_out;           // [R][Npad] step t
    const double* tsum_in;     // [R][Bs] tile sums A_b (tile scale), step t-1
    double* tsum_out;
    const double* tmax_in;     // [R][Bs] tile maxima m_b, step t-1
    double* tmax_out;
    uint32_t* anc;             // [R][Npad] or null
    FilterScalars* scal;       // [R]
    const ModelConst* mc;      // [R]
    const double* y;           // [T]
    const double* z;           // [T] or null
    double y_now, z_now;       // step API: the observation and covariate of THIS call travel in the kernel arguments (by_value = 1)
    double y_now_v[3];         // ... components 1 .. 3 of a vector observation (user models with dim_y > 1, model_api.h)
    double z_now_v[3];         // ... covariates 1 .. 3 of a user model with dim_cov > 1
    size_t xplane;             // user models with dim_x > 1: component d of the particles lives at x_in / x_out + d * xplane
    int32_t by_value;          // 1: use y_now / z_now instead of y[yi] / z[yi] (no upload, no memory read)
    double* ll_host;           // step API: host-mapped buffer that receives the R log conditional likelihoods from the accounting kernel, or null
    double* per_step;          // [R][Tcap] or null
    double* small_ms;          // [R][Tcap][2] scratch of k_filter_series_lane: (m_t, S_t), then lse_t
    const double* gam;         // [nT][R][B] Gamma(n_b) draws          (multinomial)
    const double* pgam;        // [nT][R][B] exclusive prefixes of gam
    const double* gtot;        // [nT][R]    sum(gam) + E_{N+1}
    int32_t N, Npad, B, Bs, Bpow2, rshift, R;
    int32_t tile;              // particles per tile (2048, 1024 or 512): part of the arithmetic specification
    int32_t t, yi, gi, Tcap;   // t: time index (RNG counter, schedule); yi / gi: rows of y / gamma tables
    int32_t resampler, resamp_sched;
    int32_t finalize_prev;     // account log p(y_{t-1}|.) of the previous step
    int32_t tile0;             // particle-sharded filter: global id of this launch's first OUTPUT tile (0 otherwise); outputs
                               // are stored at local offsets (tile - tile0)
    int32_t win_tile0;         // global id of the first SOURCE tile held in x_in / cdf_in (0 otherwise)
    int32_t win_tiles;         // C++ shard driver, fixed-halo path: tiles held in the source window (0: unchecked)
    int32_t* win_flag;         // ... and where to record that some output tile's sources left it ([0] flag), or null
    int32_t* ticket;           // step API: [R] arrival counters; the last workgroup of a filter accounts the step in the same launch (null: kf_finalize does)
    // split level-2 (filters of more than 2048 tiles, or forced for tests): written by k_level2_plan, read by k_filter_step<..,true>
    double* l2_T;              // [R][Bs] inclusive prefixes T'_b of the rescaled tile sums
    double* l2_R;              // [R][Bs] A_b / A'_b
    int32_t* l2_lo;            // [R][Bs] first / last source tile of every output tile's targets
    int32_t* l2_hi;
    double* l2_work;           // [R][Bs] block-local scans + [R][64] per filter: [0,16) block totals, [16] m, [17] S', [32,49) exclusive
                               // offsets of the blocks: scratch of the multi-workgroup level-2 (k_l2_scan_blocks / k_l2_ranges,
                               // filters of more than 1024 tiles), or null
    int32_t l2_inkernel;       // 1 (round 3, unsharded bootstrap filters of more than 1024 tiles): the level-2 is ONE launch --
                               // k_l2_scan_blocks, whose last-arriving workgroup takes the block offsets, S' and the accounting --
                               // and k_filter_step<.., true> finds its own source-tile range in T'_j = offset[j / 1024] + local
                               // scan[j] (a 64-entry window around its own tile id, binary search beyond it): no k_l2_ranges launch
    int32_t* l2_ticket;        // [R] arrival counters of that launch (zero between launches)
    const double* l2_tsrc;     // k_filter_step<.., true> reads T'_j = l2_offs[r * l2_offs_stride + j / 1024] + l2_tsrc[r * Bs + j]:
    const double* l2_offs;     //   l2_T and zeros (stride 0) after the table kernels, l2_work's scans and offsets (stride 64) with l2_inkernel
    int32_t l2_offs_stride;
    int32_t prio_mode;         // wave-priority schedule of k_filter_step (prio_at): 0 none, 1 single residency wave, 2 several
    int32_t stream_stores;     // 1: particles and cdf are stored non-temporally (grids that are resident all at once)
    const uint32_t* keyp;      // [2] Philox key (the seed), device resident so that a captured graph survives ssme_pf_set_seed
    uint32_t first_filter;
    double logN;
    int32_t ablate;            // measurement builds only (-DSSME_ABLATE): skip sections, results invalid
    unsigned long long* stamps;  // measurement builds only: phase time stamps
};

// ---------------------------------------------------------------------------------------
// DPP wave primitives.  update_dpp(old = fill, ...) with bound_ctrl = 0: lanes whose source is
// out of range, or whose row is masked off, receive `fill`.
// ---------------------------------------------------------------------------------------
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64_neginf(double v) {    // fill = -inf
    const u64 b = d2bits(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROWMASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)0xfff00000, (int)(uint32_t)(b >> 32), CTRL, ROWMASK, 0xF, false);
    return bits2d(((u64)(uint32_t)hi << 32) | (u64)(uint32_t)lo);
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64_zero(double v) {      // fill = +0.0
    const u64 b = d2bits(v);
    int lo, hi;
    if (ROWMASK == 0xF) {
        // all rows enabled: a lane either has a source lane or is out of range, and bound_ctrl supplies the 0 --
        // no `old` operand, so the compiler need not zero the destination before every DPP move
        lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)b, CTRL, 0xF, 0xF, true);
        hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
    } else {
        lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROWMASK, 0xF, false);
        hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, ROWMASK, 0xF, false);
    }
    return bits2d(((u64)(uint32_t)hi << 32) | (u64)(uint32_t)lo);
}
// inclusive wave scan of integer-valued doubles (exact while every partial sum < 2^53)
__device__ __forceinline__ double wave_incl_scan_f64(double v) {
    v = v + dpp_f64_zero<0x111, 0xF>(v);
    v = v + dpp_f64_zero<0x112, 0xF>(v);
    v = v + dpp_f64_zero<0x114, 0xF>(v);
    v = v + dpp_f64_zero<0x118, 0xF>(v);
    v = v + dpp_f64_zero<0x142, 0xA>(v);
    v = v + dpp_f64_zero<0x143, 0xC>(v);
    return v;
}
// the same inside every row of 16 lanes: lane l of a row receives the sum of the row's lanes 0 .. l (the segment totals of the
// block scans and the block totals of the level-2 kernels live in one row)
__device__ __forceinline__ double row16_incl_scan(double v) {
    v = v + dpp_f64_zero<0x111, 0xF>(v);
    v = v + dpp_f64_zero<0x112, 0xF>(v);
    v = v + dpp_f64_zero<0x114, 0xF>(v);
    v = v + dpp_f64_zero<0x118, 0xF>(v);
    return v;
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const u64 b = d2bits(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
    return bits2d(((u64)hi << 32) | lo);
}
__device__ __forceinline__ double readfirstlane_f64(double v) {       // a value every lane holds -> scalar registers
    const u64 b = d2bits(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return bits2d(((u64)hi << 32) | lo);
}

// row_shr:n = 0x110+n ; row_bcast:15 = 0x142 ; row_bcast:31 = 0x143 ; wave_shr:1 = 0x138
__device__ __forceinline__ u64 readlane_u64(u64 v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// max over the wave of non-NaN doubles (lane 63 holds it after the scan; broadcast by readlane)
// Inside a row of 16 lanes the reduction is a BUTTERFLY (quad_perm xor 1, xor 2, row_half_mirror, row_mirror): every lane has
// a source lane, so the DPP moves need no fill value -- 3 instructions per step instead of 5 with the -inf fill of a shifted
// scan; only the two cross-row steps (row_bcast:15 / :31) keep it.  A maximum does not depend on the order: same bits.
template <int CTRL>
__device__ __forceinline__ double dpp_f64_perm(double v) {       // full permutations inside a row: no fill needed
    const u64 b = d2bits(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
    return bits2d(((u64)(uint32_t)hi << 32) | (u64)(uint32_t)lo);
}
// The v_max_f64 that dmaxnum ends in, alone.  __builtin_fmax first canonicalises both operands (v_max_f64 x, x, x: quiets a
// signalling NaN, changes nothing else), three instructions per maximum; the maxima below never see a signalling NaN (NaN travels
// as a flag, or as the quiet dnan() in an LDS slot), so the same instruction on the same operands in the same order gives the
// same bits, signed zeros included.  (Not compare + select: that differs at (-0, +0).)
// The result feeds DPP moves directly (wave_max_f64), which must not read a VGPR within two wait states of the VALU write: this
// relies on the compiler's hazard recognizer tracking the register an inline-asm statement defines.  It does (an s_nop or two
// independent instructions follow every maximum in the assembly); look at that again after a compiler upgrade.
__device__ __forceinline__ double dmax_raw(double a, double b) {
    double d;
    asm("v_max_f64 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ double wave_max_f64(double v) {
    v = dmax_raw(v, dpp_f64_perm<0xB1>(v));            // quad_perm [1,0,3,2]
    v = dmax_raw(v, dpp_f64_perm<0x4E>(v));            // quad_perm [2,3,0,1]
    v = dmax_raw(v, dpp_f64_perm<0x141>(v));           // row_half_mirror
    v = dmax_raw(v, dpp_f64_perm<0x140>(v));           // row_mirror: every lane of a row holds the row's maximum
    v = dmax_raw(v, dpp_f64_neginf<0x142, 0xA>(v));
    v = dmax_raw(v, dpp_f64_neginf<0x143, 0xC>(v));
    return bits2d(readlane_u64(d2bits(v), 63));
}

// Block max with NaN propagation: returns dnan() if any thread passes nan = true.
// Precondition: m is not NaN in any thread -- a NaN is reported through the flag, as every caller does (mx starts at -inf and is
// replaced only where v > mx).  A NaN in m is not defined behaviour of this function: one that only some lanes of a wave pass is
// dropped by v_max_f64, one that every lane of a wave passes reaches the slot and makes the result dnan().
// lds: NT/64 doubles, not reused by the caller before its next barrier.  One barrier.
// The flag rides in the wave's own slot (a wave with a flagged lane writes dnan() instead of its maximum), so there is no
// block-wide or-reduction (__syncthreads_or is three barriers and an LDS atomic) and no LDS beyond the slots.  Every thread
// folds the slots with v_max_f64, which drops a quiet NaN operand, and finds a NaN slot with unordered compares, two slots each.
template <int NT>
__device__ __forceinline__ double block_max_nanprop(double m, bool nan, double* lds) {
    constexpr int NW = NT / 64;
    m = wave_max_f64(m);
    const bool any = __ballot(nan) != 0;               // scalar
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = any ? dnan() : m;
    __syncthreads();
    double s[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) s[w] = lds[w];
    double r = s[0];
    bool un = false;
#pragma unroll
    for (int w = 1; w < NW; ++w) r = dmax_raw(r, s[w]);
#pragma unroll
    for (int w = 0; w < NW; w += 2) un = un || __builtin_isunordered(s[w], s[w + 1 < NW ? w + 1 : w]);   // (one-wave blocks: NW = 1)
    return un ? dnan() : r;
}

// ---------------------------------------------------------------------------------------
// Exact inclusive scan of P = 2*NT*NK integer-valued doubles by a block of NT threads; every partial sum < 2^53, so each
// v_add_f64 is exact and the sums are associative: any wave/segment decomposition gives the same.
// Thread tid holds NK pairs: q[k][c] = value[(k*NT + tid)*2 + c].
// incl[k][c] = sum of all values up to and including that position; total = sum of all.
// lds_seg: 16 doubles private to this call (no trailing barrier).  One __syncthreads().
// The first element of a pair is the pair's inclusive sum MINUS the second element, not a second chain of additions from a
// lane-shifted copy of the wave scan: q is finite, non-negative and integer-valued and every partial sum is an integer below
// 2^53, so the sum, the difference and the sum built the other way round are the same exactly representable integer -- the same
// bits (a zero is +0 either way: x - x = +0 in round-to-nearest).  q must be finite: inf - inf would be NaN where the additive
// form gave inf.
// ---------------------------------------------------------------------------------------
template <int NT, int NK>
__device__ __forceinline__ void block_scan_f64(const double (&q)[NK][2], double (&incl)[NK][2], double& total, double* lds_seg) {
    constexpr int WPR = NT / 64, NSEG = NK * WPR;
    static_assert(NSEG <= 16, "segment totals are scanned inside one 16-lane row");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double inc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        inc[k] = wave_incl_scan_f64(q[k][0] + q[k][1]);
        if (lane == 63) lds_seg[k * WPR + wave] = inc[k];
    }
    __syncthreads();
    const double sv = row16_incl_scan((lane & 15) < NSEG ? lds_seg[lane & 15] : 0.0);
    total = readlane_f64(sv, 15);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int seg = k * WPR + wave;
        const double pre = seg ? readlane_f64(sv, seg - 1) : 0.0;
        incl[k][1] = pre + inc[k];
        incl[k][0] = incl[k][1] - q[k][1];
    }
}

// ---------------------------------------------------------------------------------------
// Model callbacks, compiled in (the reference's virtual fSamp/q1Samp/logGEv).
// ---------------------------------------------------------------------------------------
template <int MODEL>
__device__ __forceinline__ double model_prop(const ModelConst& c, double x, double zn, double zcov, const ExpTabEntry* etab) {
#if SSME_HAS_USER_MODEL
    if constexpr (MODEL == MODEL_USER0) return user_calls<ssme_user_model0>::prop(c, x, zn, zcov, etab);      // model_api.h
#endif
    if (MODEL == MODEL_SVOL_LEVERAGE) {   // test/test_pswarm.cpp:90-97
        const double e = dexp_scaled_t(-0.5 * x, 0, etab);
        const double mean = (c.a1 + c.a0 * (x - c.a1)) + (c.a4 * zcov) * e;
        return mean + zn * c.a3;
    }
    return c.a0 * x + zn * c.a1;          // univ_svol_bootstrap_filter.h:74-79
}

// log f(xn | x, zcov) up to a constant that does not depend on x: the density of model_prop's draw, with the mean formed in
// model_prop's own operation order (backward simulation, backward.h; a user model: its logf, model_api.h).
template <int MODEL>
__device__ __forceinline__ double model_logf(const ModelConst& c, double xn, double x, double zcov, const ExpTabEntry* etab) {
#if SSME_HAS_USER_MODEL
    if constexpr (MODEL == MODEL_USER0) return user_calls<ssme_user_model0>::logf(c, xn, x, zcov, etab);      // model_api.h
#endif
    double mean, sd;
    if (MODEL == MODEL_SVOL_LEVERAGE) {
        const double e = dexp_scaled_t(-0.5 * x, 0, etab);
        mean = (c.a1 + c.a0 * (x - c.a1)) + (c.a4 * zcov) * e;
        sd = c.a3;
    } else {
        mean = c.a0 * x;
        sd = c.a1;
    }
    const double d = (xn - mean) / sd;
    return -0.5 * (d * d);
}

template <int MODEL>
__device__ __forceinline__ double model_logg(const ModelConst& c, double y, double x, const ExpTabEntry* etab) {
#if SSME_HAS_USER_MODEL
    if constexpr (MODEL == MODEL_USER0) return c.bad ? -dinf() : user_calls<ssme_user_model0>::logg(c, y, x, etab);
#endif
    if (MODEL == MODEL_LIN_GAUSS) {
        const double d = (y - x) * c.a4;
        const double v = (-c.a3 - SSME_HALF_LOG_2PI) - 0.5 * (d * d);
        return c.bad ? -dinf() : v;
    }
    // univ_svol_bootstrap_filter.h:83-86 / test_pswarm.cpp:101-108 in kernel form
    const double logb = (MODEL == MODEL_SVOL) ? c.a3 : 0.0;
    const double ib2 = (MODEL == MODEL_SVOL) ? c.a4 : 1.0;
    const double hl = logb + 0.5 * x;
    const double e = dexp_scaled_t(-x, 0, etab);
    const double q = (y * y) * ib2;
    double v = (-hl - SSME_HALF_LOG_2PI) - 0.5 * (q * e);
    if (hl < -745.1332191019412) v = -dinf();
    if (MODEL == MODEL_SVOL && c.bad) v = -dinf();
    return v;
}

// One filter step of one scalar particle: *xn <- a2 * zn at the first step (a dim_cov user model: its own first / init), else the
// proposal from x; returns log g(y | *xn), the increment of the particle's log-weight.  zcov: the scalar covariate of the step,
// zc: the KC covariates of a dim_cov user model (the model reads one of the two).
template <int MODEL>
__device__ __forceinline__ double scalar_step(const ModelConst& c, bool first_step, double x, double zn, double y, double zcov,
                                              const CovVals<model_kcov<MODEL>()>& zc, double* xn, const ExpTabEntry* etab) {
    if constexpr (model_kcov<MODEL>() > 0) {
#if SSME_HAS_USER_MODEL
        return cov_step<typename user_model_of<MODEL>::type>(c, first_step, &x, &zn, &y, zc.v, xn, etab);
#else
        return 0.0;      // no model has covariates of its own without a user model: never instantiated
#endif
    } else {
        *xn = first_step ? zn * c.a2 : model_prop<MODEL>(c, x, zn, zcov, etab);
        return model_logg<MODEL>(c, y, *xn, etab);
    }
}

// One filter step of one particle of a VECTOR user model (dim_x or dim_y > 1): xn[dim_x] <- the model's first step (first of a
// dim_cov header that declares it, init_vec otherwise) or prop_vec from x[dim_x] and the normals zn[dim_x]; returns the increment of
// the particle's log-weight, -inf for a `bad` filter (the model is called first, the select applied afterwards).  y: dim_y values;
// zcov / zc as in scalar_step.  The one text k_filter_step and both whole-series kernels (pf_small.h) run for such a model.
template <int MODEL>
__device__ __forceinline__ double vector_step(const ModelConst& c, bool first_step, const double* x, const double* zn, const double* y,
                                              double zcov, const CovVals<model_kcov<MODEL>()>& zc, double* xn, const ExpTabEntry* etab) {
#if SSME_HAS_USER_MODEL
    using M = typename user_model_of<MODEL>::type;
    if constexpr (model_kcov<MODEL>() > 0) return cov_step<M>(c, first_step, x, zn, y, zc.v, xn, etab);
    else {
        using UC = user_calls<M>;
        if (first_step) UC::init_vec(c, zn, xn);
        else UC::prop_vec(c, x, zn, zcov, xn, etab);
        return c.bad ? -dinf() : UC::logg_vec(c, y, xn, etab);
    }
#else
    return 0.0;          // no vector model without a user model: never instantiated
#endif
}
// the normals of state component d >= 1 of particle pair `pair` at time t: one more Philox call per pair and component
__device__ __forceinline__ u32x4 xdim_words(uint32_t pair, uint32_t t, uint32_t rep, int d, uint32_t k0, uint32_t k1) {
    return philox4x32_10(pair, t, rep, (uint32_t)(STREAM_XDIM + d), k0, k1);
}

// two standard normals for the pair `pair` at time t (Box-Muller)
__device__ __forceinline__ void normal_pair(uint32_t pair, uint32_t t, uint32_t rep, uint32_t k0, uint32_t k1,
                                            double* z0, double* z1) {
    const u32x4 o = philox4x32_10(pair, t, rep, STREAM_PROP, k0, k1);
    const double u1 = u01_oc(o.v0, o.v1), u2 = u01_co(o.v2, o.v3);
    const double rad = dsqrt(-2.0 * dlog_pn(u1));
    double sn, cs;
    dsincos2pi(u2, &sn, &cs);
    *z0 = rad * cs;
    *z1 = rad * sn;
}

// the same in two halves, so that memory latency can be hidden between them
__device__ __forceinline__ void normal_pair_radius(uint32_t pair, uint32_t t, uint32_t rep, uint32_t k0, uint32_t k1,
                                                   double* rad, double* u2) {
    const u32x4 o = philox4x32_10(pair, t, rep, STREAM_PROP, k0, k1);
    *rad = dsqrt(-2.0 * dlog_pn(u01_oc(o.v0, o.v1)));
    *u2 = u01_co(o.v2, o.v3);
}
__device__ __forceinline__ void normal_pair_angle(double rad, double u2, double* z0, double* z1) {
    double sn, cs;
    dsincos2pi(u2, &sn, &cs);
    *z0 = rad * cs;
    *z1 = rad * sn;
}

// ---- bootstrap filter: ONE Philox call per particle pair and time step -------------------------------------------------
// The thread that propagates pair p at time t also draws that pair's two exponential spacings of the multinomial resampler,
// so one counter (pair, t, filter, STREAM_PROP) feeds both: words 0-1 -> Box-Muller (radius uniform: 40 bits, strictly inside
// (0,1), i.e. |z| < 7.45; angle: the low 24 bits of word 1), words 2-3 -> E_0, E_1 = -log(u), u on the 2^-32 midpoint grid
// (the spacings are quantised to 2^-35 right away).  Logs by dlog_u (table in LDS, no division).  DESIGN.md section 4.1.
__device__ __forceinline__ u32x4 pair_words(uint32_t pair, uint32_t t, uint32_t rep, uint32_t k0, uint32_t k1) {
    return philox4x32_10(pair, t, rep, STREAM_PROP, k0, k1);
}
__device__ __forceinline__ void pair_spacings(const u32x4& o, const LogTabEntry* tab, double* e0, double* e1) {
    *e0 = -dlog_u32(u01_mid32(o.v2), tab);
    *e1 = -dlog_u32(u01_mid32(o.v3), tab);
}
// the draw tables of a hot kernel in LDS: dlog_u / dlog_u32 and dsincos_k24 (2 KiB)
struct DrawTabs {
    LogTabEntry log[SSME_LOG_TABLE_SIZE];
    SinCosEntry sc[SSME_SINCOS_TABLE_SIZE];
};
__device__ __forceinline__ void pair_normals(uint32_t w0, uint32_t w1, const DrawTabs* tab, double* z0, double* z1) {
    const double rad = dsqrt_pn(-2.0 * dlog_u(u01_mid40(w0, w1), tab->log));
    double sn, cs;
    dsincos_k24(w1, tab->sc, &sn, &cs);
    *z0 = rad * cs;
    *z1 = rad * sn;
}
// the tables of dlog_u, dsincos_k24 and dexp_scaled_t, in device memory; every workgroup of the hot kernels copies them
// into LDS (3 x 64 x 16 bytes) before its first use
static __device__ const LogTabEntry kLogTable[SSME_LOG_TABLE_SIZE] = {SSME_LOG_TABLE_ROWS};
static __device__ const SinCosEntry kSinCosTable[SSME_SINCOS_TABLE_SIZE] = {SSME_SINCOS_TABLE_ROWS};
static __device__ const ExpTabEntry kExpTable[SSME_EXP_TABLE_SIZE] = {SSME_EXP_TABLE_ROWS};
template <int NT>
__device__ __forceinline__ void load_log_table(DrawTabs* lds_tab) {
    static_assert(SSME_LOG_TABLE_SIZE == SSME_SINCOS_TABLE_SIZE, "one pass fills both");
    for (int i = threadIdx.x; i < SSME_LOG_TABLE_SIZE; i += NT) { lds_tab->log[i] = kLogTable[i]; lds_tab->sc[i] = kSinCosTable[i]; }
}
template <int NT>
__device__ __forceinline__ void load_exp_table(ExpTabEntry* lds_tab) {
    for (int i = threadIdx.x; i < SSME_EXP_TABLE_SIZE; i += NT) lds_tab[i] = kExpTable[i];
}
// Gamma(shape) draw, Marsaglia & Tsang (2000), attempts driven by the Philox counter
__device__ __forceinline__ double gamma_draw(uint32_t b, uint32_t t, uint32_t rep, uint32_t k0, uint32_t k1, double shape,
                                             uint32_t stream_base = STREAM_GAMMA) {
    const double d = shape - 0.3333333333333333;
    const double c = 1.0 / dsqrt(9.0 * d);
    for (int a = 0; a < 32; ++a) {
        const u32x4 o1 = philox4x32_10(b, t, rep, stream_base + 2 * a, k0, k1);
        const u32x4 o2 = philox4x32_10(b, t, rep, stream_base + 2 * a + 1, k0, k1);
        const double rad = dsqrt(-2.0 * dlog_pn(u01_oc(o1.v0, o1.v1)));
        double sn, cs;
        dsincos2pi(u01_co(o1.v2, o1.v3), &sn, &cs);
        const double xn = rad * cs;
        const double v = 1.0 + c * xn;
        if (v > 0.0) {
            const double v3 = (v * v) * v;
            const double lhs = dlog_pn(u01_oc(o2.v0, o2.v1));
            const double rhs = ((0.5 * (xn * xn) + d) - d * v3) + d * dlog(v3);
            if (lhs < rhs) return d * v3;
        }
    }
    return d;
}

// #{ j < n : get(j) < target } for monotone get, n = 2^k (a NaN target counts nothing)
template <class F>
__device__ __forceinline__ int count_less_pow2(int n, double target, F get) {
    int pos = 0;
    for (int step = n >> 1; step >= 1; step >>= 1)
        if (get(pos + step - 1) < target) pos += step;
    // pos in [0, n-1]; the last element is not probed: callers clamp the count to n-1 anyway
    return pos;
}

// Level-2 of one filter: global max m over the tile maxima (NaN propagating), rescaled integer
// tile sums A'_b = rint(A_b exp(m_b - m) 2^(rg-41)), their exact inclusive scan.  Thread tid holds
// entries j = e*NT + tid, e < NE = 2048/NT: at B <= NT every wave owns live entries, so the serial
// exp / divide per entry is spread over the whole block.  Rows without live entries are skipped.
// 1 + nrows barriers.  lds_d: NT/64 doubles, lds_seg: 16 doubles per row (4 rows).
template <int NT>
__device__ __forceinline__ void level2_load(const double* ts, const double* tm, int B, double (&A)[2048 / NT],
                                            double (&mb)[2048 / NT]) {
    constexpr int NE = 2048 / NT;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int j = e * NT + threadIdx.x;
        if (j < B) { A[e] = ts[j]; mb[e] = tm[j]; } else { A[e] = 0.0; mb[e] = 0.0; }
    }
}

template <int NT>
__device__ __forceinline__ void level2_scan(const double (&A)[2048 / NT], const double (&mb)[2048 / NT], int B, int rshift,
                                            double& m, double (&Ap)[2048 / NT], double (&Tinc)[2048 / NT], double& S,
                                            double* lds_d, double* lds_seg, const ExpTabEntry* etab) {
    constexpr int NE = 2048 / NT, NW = NT / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double mx = -dinf();
    bool nan = false;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        if (e * NT < B) {
            // legs e >= 1 exist only in filters of more than NT tiles: kept a uniform branch (as selects under scalar masks they
            // cost every filter some 20 instructions per wave)
            if (e) asm volatile("");
            const int j = e * NT + threadIdx.x;
            if (j < B) { const double v = mb[e]; nan = nan || (v != v); mx = (v > mx) ? v : mx; }
        }
    }
    m = block_max_nanprop<NT>(mx, nan, lds_d);
    double inc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        Ap[e] = 0.0; inc[e] = 0.0;
        if (e * NT < B) {
            const int j = e * NT + threadIdx.x;
            // NaN (m or m_b NaN) is squashed to 0 by dexp_scaled's clamp: A' = rint(A * 0) = 0
            if (j < B) Ap[e] = __builtin_rint(A[e] * dexp_scaled_t(mb[e] - m, rshift - kTileShift, etab));
            inc[e] = wave_incl_scan_f64(Ap[e]);
            if (lane == 63) lds_seg[e * 16 + wave] = inc[e];
        }
    }
    __syncthreads();
    double carry = 0.0;
    S = 0.0;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        Tinc[e] = 0.0;
        if (e * NT < B) {
            const double sv = row16_incl_scan((lane & 15) < NW ? lds_seg[e * 16 + (lane & 15)] : 0.0);
            const double pre = wave ? readlane_f64(sv, wave - 1) : 0.0;
            Tinc[e] = (carry + pre) + inc[e];
            carry = carry + readlane_f64(sv, 15);
        }
    }
    S = carry;
}

// Workgroup -> tile map.  Workgroups are dispatched round-robin over the 8 XCDs (workgroup id mod 8), and each XCD has
// its own L2.  Consecutive tiles share source cdf tiles (a tile's sorted targets fall into 1-3 neighbouring tiles), so
// XCD k is given a CONTIGUOUS range of tiles: the re-reads of a neighbour's tile then hit that XCD's L2 instead of
// being fetched once per XCD.  Any bijection is correct (results do not depend on the map).
__device__ __forceinline__ int xcd_tile_of_block(int bid, int nblocks) {
    constexpr int kXcd = 8;
    const int q = nblocks / kXcd, r = nblocks % kXcd;
    const int k = bid % kXcd, idx = bid / kXcd;
    return k * q + (k < r ? k : r) + idx;
}

// Bounds [t_lo, t_hi] of the integer resampling targets of output tile b (first particle i_first, nvalid valid
// outputs), known without the random spacings.  Shared by k_filter_step and the shard planner (k_shard_plan),
// which must agree to the bit on which source tiles a tile touches.
__device__ __forceinline__ void tile_target_bounds(int resampler, double S, int N, int i_first, int nvalid, double pgam,
                                                   double pgam_next, double G, double u0, double& t_scale, double& t_lo,
                                                   double& t_hi) {
    if (resampler == RESAMP_MULTINOMIAL) {
        t_scale = S / G;                          // targets: (pgam + Gamma_b E_cum/E_tile) * S'/G  
        t_lo = __builtin_ceil(pgam * t_scale);
        t_hi = __builtin_ceil(pgam_next * t_scale) + (S * 0x1.0p-40 + 2.0);   // slack covers the rounding of ratio*E_tile vs Gamma_b
    } else if (resampler == RESAMP_SYSTEMATIC) {
        t_scale = S / (double)N;
        t_lo = __builtin_ceil(((double)i_first + u0) * t_scale);
        t_hi = __builtin_ceil(((double)(i_first + nvalid - 1) + u0) * t_scale);
    } else {
        t_scale = S / (double)N;
        t_lo = __builtin_ceil((double)i_first * t_scale);
        t_hi = __builtin_ceil((double)(i_first + nvalid) * t_scale);
    }
}

// The draw constants of a step's resampling that do not depend on the tile: G = sum(Gamma) + E_{N+1} of the multinomial draw
// (gtot row a.gi), or the systematic offset u0 (Philox counter (0, t, filter, STREAM_RESAMP_EXTRA)); 1 and 0 where unused.
__device__ __forceinline__ double systematic_u0(uint32_t t, uint32_t rep, uint32_t key0, uint32_t key1) {
    const u32x4 ox = philox4x32_10(0u, t, rep, STREAM_RESAMP_EXTRA, key0, key1);
    return u01_co(ox.v0, ox.v1);
}
__device__ __forceinline__ void draw_consts(const StepArgs& a, int resampler, int r, uint32_t rep, double& G, double& u0) {
    G = 1.0; u0 = 0.0;
    if (resampler == RESAMP_MULTINOMIAL) G = a.gtot[(size_t)a.gi * a.R + r];
    else if (resampler == RESAMP_SYSTEMATIC) u0 = systematic_u0((uint32_t)a.t, rep, a.keyp[0], a.keyp[1]);
}

// log-sum-exp of a step's log-weights from the level-2 results: m + log(S 2^-rshift); NaN when no weight is positive
__device__ __forceinline__ double lse_of(double m, double S, int rshift) {
    const double Sd = (S > 0.0) ? dldexp(S, -rshift) : dnan();
    return m + dlog(Sd);
}
// Accounts one step of a bootstrap filter: log p(y_t | y_{1:t-1}) = lse_t - prev, where prev is the log-sum-exp the step started
// from (log N after a resampling).  `resampled`: the NEXT step starts from equal weights.  Returns the log conditional likelihood.
__device__ __forceinline__ double account_step(FilterScalars* sc, double m, double S, int rshift, bool resampled, double logN) {
    const double lse = lse_of(m, S, rshift);
    const double ll = lse - sc->prev;
    sc->m = m;
    sc->S = S;
    sc->last_ll = ll;
    sc->loglik = sc->loglik + ll;
    sc->prev = resampled ? logN : lse;
    return ll;
}

// Maximum of the KMAX tile maxima a thread of the split level-2 kernels holds in registers (tile k * NT + tid), NaN reported as a
// flag (block_max_nanprop's precondition).
template <int NT, int KMAX>
__device__ __forceinline__ void reg_max_nanflag(const double (&Mreg)[KMAX], int B, double& mx, bool& nan) {
    mx = -dinf();
    nan = false;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k * NT + (int)threadIdx.x < B) { const double v = Mreg[k]; nan = nan || (v != v); mx = (v > mx) ? v : mx; }
    }
}

// Wave priority by phase.  Two workgroups share a CU and the hardware issues the OLDER waves first, so without this the
// first-dispatched workgroup runs at full speed, the second one lags by ~5 us, and for that tail the CU holds half its
// waves.  Lowering the priority as a workgroup advances lets the one that is behind catch up:
// both then finish together and the CU stays full.  mode 1 (the whole grid is resident at once: 20.3 -> 19.2 us at
// N = 2^20): 3 | after the tile loads are issued 2 | after the search 1 | after logG 0.  mode 2 (several residency waves of
// workgroups, e.g. 4096 filters' tiles; +2 %): 3 | 2 | after the LDS fill 1 | after the search 0.  Scheduling only --
// results do not depend on it.
__device__ __forceinline__ void prio_at(int mode, int idx) {
    if (mode == 1) {
        if (idx == 0) __builtin_amdgcn_s_setprio(3); else if (idx == 3) __builtin_amdgcn_s_setprio(2);
        else if (idx == 6) __builtin_amdgcn_s_setprio(1); else if (idx == 8) __builtin_amdgcn_s_setprio(0);
    } else if (mode == 2) {
        if (idx == 0) __builtin_amdgcn_s_setprio(3); else if (idx == 3) __builtin_amdgcn_s_setprio(2);
        else if (idx == 5) __builtin_amdgcn_s_setprio(1); else if (idx == 6) __builtin_amdgcn_s_setprio(0);
    } else if (mode == 3) {          // experimental schedules (SSME_PRIO_MODE): later drops
        if (idx == 0) __builtin_amdgcn_s_setprio(3); else if (idx == 4) __builtin_amdgcn_s_setprio(2);
        else if (idx == 7) __builtin_amdgcn_s_setprio(1); else if (idx == 9) __builtin_amdgcn_s_setprio(0);
    } else if (mode == 4) {          // earlier drops
        if (idx == 0) __builtin_amdgcn_s_setprio(3); else if (idx == 2) __builtin_amdgcn_s_setprio(2);
        else if (idx == 4) __builtin_amdgcn_s_setprio(1); else if (idx == 6) __builtin_amdgcn_s_setprio(0);
    } else if (mode == 5) {          // two levels only
        if (idx == 0) __builtin_amdgcn_s_setprio(1); else if (idx == 6) __builtin_amdgcn_s_setprio(0);
    }
}
#define PRIO_AT(i) prio_at(RESIDENT ? 1 : a.prio_mode, i)        // (k_filter_step only)

// ---------------------------------------------------------------------------------------
// k_filter_step: one bootstrap-filter step for every tile of every filter.
// grid = (B tiles, R filters), block = NT threads, NK = TILE/(2 NT) particle pairs per thread (TILE = 2048: NT = 256/512/1024;
// TILE = 512: NT = 256), dynamic LDS = (2*max(Bpow2,2) + 3*TILE) * 8 bytes.
// RS >= 0 compiles the reference's configuration in (resampler RS, resampling every step, t > 0, no debug outputs): the
// uniform branches of the general kernel disappear and the compiler schedules across what they separated; RS = -1 is
// the general kernel (any resampler / schedule / t = 0 / ancestor and log-weight recording).  Same arithmetic, same bits.
// RESIDENT (RS >= 0 only) compiles in what the host chooses for a grid that is resident at once -- prio_mode 1 and streaming
// stores: each of the twelve PRIO_AT sites is then one s_setprio or nothing instead of a chain of scalar compares and
// branches on a.prio_mode, and store_pair does not branch.  Scheduling and cache policy only.
// Phase order is chosen so that arithmetic hides memory latency: the cdf tiles are requested,
// then the Box-Muller radii are computed while they arrive; the ancestor states are requested,
// then the Box-Muller angles are computed while they arrive.
// ---------------------------------------------------------------------------------------
// The count-searches of a thread in the staged tiles, all NQ of them descending TOGETHER, one level per round: a round is NQ
// independent ds_read_b64 (position = absolute LDS byte address, the level's offset in the immediate field), ONE wait, then per
// search compare + select + add -- 3 VALU instructions per probe and log2(TILE) dependent LDS round trips per thread.
// Written as inline assembly because the compiler, given the same loop in C++, either spends a fourth instruction per probe
// on the address or serialises the NQ chains (44 dependent round trips; both seen in the ISA, round 3).  The wait names the
// loaded values as in/out operands, so nothing that consumes them can be scheduled above it.
template <int STEP, int NQ>
struct lds_count_search {
    static __device__ __forceinline__ void run(uint32_t (&pa)[NQ], const double (&t)[NQ]) {
        static_assert(NQ == 1 || NQ == 2 || NQ == 4 || NQ == 8, "one to eight searches per thread");
        double v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(v[q]) : "v"(pa[q]), "n"((STEP - 1) * 8) : "memory");
        if constexpr (NQ == 8) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
        else if constexpr (NQ == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
        else if constexpr (NQ == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]));
#pragma unroll
        for (int q = 0; q < NQ; ++q) pa[q] = (v[q] < t[q]) ? pa[q] + (uint32_t)(STEP * 8) : pa[q];
        lds_count_search<STEP / 2, NQ>::run(pa, t);
    }
};
template <int NQ>
struct lds_count_search<0, NQ> {
    static __device__ __forceinline__ void run(uint32_t (&)[NQ], const double (&)[NQ]) {}
};

// The staged search of one thread: targets tau (integers in the filter's global fixed point) -> positions among the `span`
// (<= 3) cdf tiles staged in LDS at lds_stage.  staged_search_pos returns them as they are held during the search, ABSOLUTE LDS
// BYTE ADDRESSES pos = lds_addr(lds_stage) + 8 * (element offset from the first staged tile, 0 .. span TILE - 1): k_filter_step
// turns one into the gather's byte offset with a single add of a uniform; staged_search returns the element offsets (the
// Liu-West selection, lw_select, which indexes several arrays with them).
// Pm / T0 / T1: inclusive prefixes T' of the tile before the first staged tile and of the first two staged tiles;
// R0..R2: A / A' of the staged tiles.
// A position has the tile select folded in, so a probe is ds_read_b64 (constant offset field) + compare + add + select.  The
// target's tile is a uniform case split on `span`; with two or three staged tiles a WAVE whose targets all fall into one of them
// (a ballot over the thread's targets: the targets of a workgroup are sorted, so at most span - 1 of its waves contain a
// crossing) takes a uniform branch with scalar operands and no selects; a wave with a crossing pays one compare and five selects
// per particle (two staged tiles) or two and nine (three).  The same values either way.
__device__ __forceinline__ uint32_t lds_addr(const double* p) {
    typedef __attribute__((address_space(3))) const double lds_cdouble;
    return (uint32_t)(__UINTPTR_TYPE__)(lds_cdouble*)p;
}
template <int TILE, int NK>
__device__ __forceinline__ void staged_search_pos(const double (&tau)[NK][2], int span, double Pm, double T0, double T1, double R0, double R1,
                                                  double R2, const double* lds_stage, uint32_t (&pos)[NK][2]) {
    double tloc[NK][2];
    uint32_t pb[NK][2];
    const uint32_t stage_a = lds_addr(lds_stage);
    auto one_tile = [&](double P, double R, uint32_t base) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int c = 0; c < 2; ++c) { tloc[k][c] = __builtin_ceil((tau[k][c] - P) * R); pb[k][c] = base; }
        }
    };
    if (span == 1) one_tile(Pm, R0, stage_a);
    else if (span == 2) {
        bool any_up = false, all_up = true;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int c = 0; c < 2; ++c) { const bool up = T0 < tau[k][c]; any_up = any_up || up; all_up = all_up && up; }
        }
        if (!__builtin_amdgcn_ballot_w64(any_up)) {            // the whole wave in the first staged tile
            asm volatile("");                                  // (kept a branch, as the ragged tile's)
            one_tile(Pm, R0, stage_a);
        } else if (!__builtin_amdgcn_ballot_w64(!all_up)) {    // the whole wave in the second
            asm volatile("");
            one_tile(T0, R1, stage_a + (uint32_t)(TILE * 8));
        } else {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const bool up = T0 < tau[k][c];
                    tloc[k][c] = __builtin_ceil((tau[k][c] - (up ? T0 : Pm)) * (up ? R1 : R0));
                    pb[k][c] = up ? stage_a + (uint32_t)(TILE * 8) : stage_a;
                }
            }
        }
    } else {
        int sel[NK][2];
        bool differs = false;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int s = (T0 < tau[k][c] ? 1 : 0) + (T1 < tau[k][c] ? 1 : 0);
                sel[k][c] = s < span - 1 ? s : span - 1;
            }
        }
        const int sel_u = __builtin_amdgcn_readfirstlane(sel[0][0]);
#pragma unroll
        for (int k = 0; k < NK; ++k) differs = differs || sel[k][0] != sel_u || sel[k][1] != sel_u;
        if (!__builtin_amdgcn_ballot_w64(differs)) {           // the whole wave in one staged tile
            asm volatile("");
            one_tile(sel_u == 0 ? Pm : (sel_u == 1 ? T0 : T1), sel_u == 0 ? R0 : (sel_u == 1 ? R1 : R2), stage_a + (uint32_t)sel_u * (uint32_t)(TILE * 8));
        } else {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int s = sel[k][c];
                    const double Pb = s == 0 ? Pm : (s == 1 ? T0 : T1);
                    const double Rb = s == 0 ? R0 : (s == 1 ? R1 : R2);
                    tloc[k][c] = __builtin_ceil((tau[k][c] - Pb) * Rb);
                    pb[k][c] = stage_a + (uint32_t)s * (uint32_t)(TILE * 8);
                }
            }
        }
    }
    // With one pair per thread the window is not used: its log2 W probes lengthen a chain that then runs alone (N = 2^16,
    // 512-particle tiles: 6.73 -> 7.00 us per step, profiles/r04_search_philox_ab.txt); with two or more the chains of the pairs overlap.
    if constexpr (SSME_SEARCH_WINDOW > 0 && NK >= 2) {
        // The pair's first targets: a full descent, NK chains together.
        constexpr int W = SSME_SEARCH_WINDOW > 0 ? SSME_SEARCH_WINDOW : 2;
        static_assert(W >= 2 && (W & (W - 1)) == 0 && W <= TILE, "the window is a power of two inside the tile");
        uint32_t pa0[NK], pa1[NK], top[NK];
        double t0[NK], t1[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) { pa0[k] = pb[k][0]; t0[k] = tloc[k][0]; t1[k] = tloc[k][1]; }
        lds_count_search<TILE / 2, NK>::run(pa0, t0);
        // The second target is not below the first (both resampling orders are sorted), so in the same tile every element below
        // the first count is below it too and its count starts there; in a later tile it starts at that tile's first element.
        // It is counted inside a window of W elements, moved down if it would leave the tile (an element below the start is
        // below the target as well): log2 W probes.  A count that reaches the window's last element is not bracketed; then
        // the wave repeats the full descent for its second targets (a uniform branch), so the result is the full search's
        // for any weights.
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const uint32_t lo = pb[k][1], hi = pb[k][1] + (uint32_t)((TILE - W) * 8);
            const uint32_t st = pa0[k] > lo ? pa0[k] : lo;
            pa1[k] = st < hi ? st : hi;
            top[k] = pa1[k] + (uint32_t)((W - 1) * 8);
        }
        lds_count_search<W / 2, NK>::run(pa1, t1);
        bool open = false;
#pragma unroll
        for (int k = 0; k < NK; ++k) open = open || pa1[k] == top[k];
        if (__builtin_amdgcn_ballot_w64(open)) {
#pragma unroll
            for (int k = 0; k < NK; ++k) pa1[k] = pb[k][1];
            lds_count_search<TILE / 2, NK>::run(pa1, t1);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) { pos[k][0] = pa0[k]; pos[k][1] = pa1[k]; }
    } else {
        uint32_t pa[2 * NK];
        double tq[2 * NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) { pa[2 * k] = pb[k][0]; pa[2 * k + 1] = pb[k][1]; tq[2 * k] = tloc[k][0]; tq[2 * k + 1] = tloc[k][1]; }
        lds_count_search<TILE / 2, 2 * NK>::run(pa, tq);
#pragma unroll
        for (int k = 0; k < NK; ++k) { pos[k][0] = pa[2 * k]; pos[k][1] = pa[2 * k + 1]; }
    }
}
template <int TILE, int NK>
__device__ __forceinline__ void staged_search(const double (&tau)[NK][2], int span, double Pm, double T0, double T1, double R0, double R1,
                                              double R2, const double* lds_stage, int (&off)[NK][2]) {
    uint32_t pos[NK][2];
    staged_search_pos<TILE, NK>(tau, span, Pm, T0, T1, R0, R1, R2, lds_stage, pos);
    const uint32_t stage_a = lds_addr(lds_stage);
#pragma unroll
    for (int k = 0; k < NK; ++k) { off[k][0] = (int)((pos[k][0] - stage_a) >> 3); off[k][1] = (int)((pos[k][1] - stage_a) >> 3); }
}

// ---------------------------------------------------------------------------------------
// The pieces of a multinomial selection against the exact integer cdf, in the order a kernel calls them:
// clamp_to_window, publish_ratios, StagedTiles::load, multinomial_targets, StagedTiles::store, staged_prefixes, (barrier),
// staged_ratios, staged_search -- or probe_ancestor per target when the tile's sources span more than kStageTiles tiles.
// Callers: k_filter_step, the Liu-West stages (lw_select) and, for probe_ancestor, the forecast's start draw (fc_draw_ancestor).
// A caller says where T'_j and A_j / A'_j live by passing accessors; the pieces know nothing else about it.
// ---------------------------------------------------------------------------------------
// Fixed-halo sharding: the source window this rank holds ([win_tile0, win_tile0 + win_tiles) of B tiles) was exchanged BEFORE
// anyone knew the plan.  If the sources [bb_min, bb_min + span) of this output tile leave it, say so in flag[0] (the host reruns
// the series on the exact path) and stay inside the buffer for this launch.  flag = null: unchecked.
__device__ __forceinline__ void clamp_to_window(int32_t* flag, int win_tile0, int win_tiles, int B, int& bb_min, int& span) {
    if (!flag) return;
    const int first = win_tile0 > 0 ? win_tile0 : 0, last = win_tile0 + win_tiles - 1 < B - 1 ? win_tile0 + win_tiles - 1 : B - 1;
    if (bb_min < first || bb_min + span - 1 > last) {
        if (threadIdx.x == 0) atomicOr(flag, 1);
        bb_min = bb_min < first ? first : (bb_min > last ? last : bb_min);
        span = 1;
    }
}

// In-LDS level-2: A_b / A'_b (maps a global target into its tile's fixed point) from the entries the threads hold (thread tid:
// j = e * NT + tid).  Only the staged tiles' ratios are needed, so the IEEE division runs in the one or two waves that hold those
// entries, off the path to the first barrier (R3[sl]: tile min(bb_min + sl, B - 1)); an output tile spanning more than
// kStageTiles source tiles (iid resampling, degenerate weights) publishes all of them in R_all and passes a barrier.  R3 is
// visible after the caller's next barrier.
template <int NT>
__device__ __forceinline__ void publish_ratios(const double (&A)[2048 / NT], const double (&Ap)[2048 / NT], int B, int Bpow2, int bb_min,
                                               int span, double* R3, double* R_all) {
    constexpr int NE = 2048 / NT;
    const int tid = threadIdx.x;
    if (span <= kStageTiles) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e * NT < Bpow2) {
                const int j = e * NT + tid;
#pragma unroll
                for (int sl = 0; sl < kStageTiles; ++sl) {
                    const int bs = bb_min + sl < B ? bb_min + sl : B - 1;
                    if (j == bs) R3[sl] = A[e] / Ap[e];
                }
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e * NT < Bpow2) {
                const int j = e * NT + tid;
                if (j < Bpow2) R_all[j] = (j < B) ? A[e] / Ap[e] : 0.0;
            }
        }
        __syncthreads();
    }
}

// The (at most) three source cdf tiles of an output tile on their way from memory to LDS, in registers in between so that the
// spacings' arithmetic hides the loads: thread tid holds pairs k * NT + tid of each tile.  Three explicitly named register
// tiles (a run-time indexed array would be placed in scratch memory).
template <int NT, int NK, int TILE>
struct StagedTiles {
    double2 stg0[NK], stg1[NK], stg2[NK];
    // src: the first staged tile (uniform).  Coalesced 16-byte loads at a uniform base (scalar registers) plus a 32-bit lane
    // offset: no 64-bit address arithmetic per lane.
    __device__ __forceinline__ void load(const double* src, int span) {
#pragma unroll
        for (int k = 0; k < NK; ++k) { stg0[k] = make_double2(0.0, 0.0); stg1[k] = stg0[k]; stg2[k] = stg0[k]; }
        if (span > kStageTiles) return;
        const unsigned char* base = reinterpret_cast<const unsigned char*>(src);
        const uint32_t lane_off = (uint32_t)threadIdx.x * 16u;
#pragma unroll
        for (int k = 0; k < NK; ++k) stg0[k] = *reinterpret_cast<const double2*>(base + (lane_off + (uint32_t)(k * NT * 16)));
        if (span >= 2) {
#pragma unroll
            for (int k = 0; k < NK; ++k) stg1[k] = *reinterpret_cast<const double2*>(base + (lane_off + (uint32_t)(TILE * 8 + k * NT * 16)));
        }
        if (span >= 3) {
#pragma unroll
            for (int k = 0; k < NK; ++k) stg2[k] = *reinterpret_cast<const double2*>(base + (lane_off + (uint32_t)(2 * TILE * 8 + k * NT * 16)));
        }
    }
    // span <= kStageTiles; visible after the caller's next barrier
    __device__ __forceinline__ void store(double* lds_stage, int span) const {
        double* dst = lds_stage + threadIdx.x * 2;
#pragma unroll
        for (int k = 0; k < NK; ++k) *reinterpret_cast<double2*>(dst + k * NT * 2) = stg0[k];
        if (span >= 2) {
#pragma unroll
            for (int k = 0; k < NK; ++k) *reinterpret_cast<double2*>(dst + TILE + k * NT * 2) = stg1[k];
        }
        if (span >= 3) {
#pragma unroll
            for (int k = 0; k < NK; ++k) *reinterpret_cast<double2*>(dst + 2 * TILE + k * NT * 2) = stg2[k];
        }
    }
};

// Integer resampling targets in [0, S'] of the multinomial draw (liu_west_filter.h:105-139): sorted uniforms by exponential
// spacings.  spacings(k, e0, e1): the spacings of particles i_first + (k * NT + tid) * 2 + {0, 1} from the pair's draw words;
// qE = rne(E 2^35), exact tile scan (one barrier, lds_seg: 16 doubles), target = ceil((pgam + Gamma_b E_cum / E_tile) S'/G) with
// t_scale = S'/G.  The caller's draw runs INSIDE the per-pair loop: a pair's Philox + log chain then ends at the ragged-tile
// branch of its own pair; all pairs' chains in one block interleave and cost k_filter_step two VGPRs and a wave per SIMD.
template <int NT, int NK, int TILE, class EF>
__device__ __forceinline__ void multinomial_targets(EF spacings, int i_first, int N, double gam, double pgam, double t_scale,
                                                    double* lds_seg, double (&tau)[NK][2]) {
    double qe[NK][2], le[NK][2], se;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        double e0, e1;
        spacings(k, e0, e1);
        qe[k][0] = __builtin_rint(e0 * 34359738368.0 /* 2^35 */);
        qe[k][1] = __builtin_rint(e1 * 34359738368.0);
        if (i_first + TILE > N) {         // only the last tile of a filter whose N is not a multiple of the tile: a uniform branch
            asm volatile("");             // (kept a branch: as selects these masks cost every tile 12 instructions per particle pair)
            const int i0 = i_first + (k * NT + (int)threadIdx.x) * 2;
            if (!(i0 < N)) qe[k][0] = 0.0;
            if (!(i0 + 1 < N)) qe[k][1] = 0.0;
        }
    }
    block_scan_f64<NT, NK>(qe, le, se, lds_seg);
    const double ratio = gam / se;        // per tile: Gamma_b * E_j / sum_tile(E)
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double t1 = ratio * le[k][c];
            const double t2 = pgam + t1;
            tau[k][c] = __builtin_ceil(t2 * t_scale);
        }
    }
}

// Operands of staged_search for the staged tiles bb_min .. : the prefixes Pm / T0 / T1 from Tof(j) = T'_j (read before the barrier
// that makes the staged tiles visible, so that their latency is hidden behind it) and the ratios R0..R2 from Rof(j) = A_j / A'_j,
// a table of the split level-2 (the in-LDS level-2 has them in publish_ratios' R3[0..2] already, read after that barrier).
template <class TF>
__device__ __forceinline__ void staged_prefixes(TF Tof, int bb_min, int B, double& Pm, double& T0, double& T1) {
    T0 = Tof(bb_min);
    T1 = (bb_min + 1 < B) ? Tof(bb_min + 1) : dinf();
    Pm = bb_min ? Tof(bb_min - 1) : 0.0;
}
template <class RF>
__device__ __forceinline__ void staged_ratios(RF Rof, int bb_min, int B, double& R0, double& R1, double& R2) {
    const int b1 = bb_min + 1 < B ? bb_min + 1 : B - 1, b2 = bb_min + 2 < B ? bb_min + 2 : B - 1;
    R0 = Rof(bb_min); R1 = Rof(b1); R2 = Rof(b2);
}

// The general search of one target (iid multinomial, an output tile spanning many cdf tiles, the forecast's start draw): source
// tile b = min(#{j < Bpow2 : Tof(j) < target}, B - 1) (Tof(j) = +inf for B <= j < Bpow2: the caller's accessor says so), tile-local target
// tloc = ceil((target - T'_{b-1}) A_b / A'_b), j = #{q : cdf_b[q] < tloc} (count_less_pow2: at most tile - 1); returns the
// ancestor min(b tile + j, N - 1).  cdf_row starts at tile win_tile0.  Probes go to L2.
template <class TF, class RF>
__device__ __forceinline__ int probe_ancestor(double target, TF Tof, RF Rof, const double* cdf_row, int B, int Bpow2, int tile,
                                              int win_tile0, int N) {
    int bb = count_less_pow2(Bpow2, target, Tof);
    bb = bb < B - 1 ? bb : B - 1;
    const double Pb = bb ? Tof(bb - 1) : 0.0;
    const double tloc = __builtin_ceil((target - Pb) * Rof(bb));
    const double* tl = cdf_row + (size_t)(bb - win_tile0) * tile;
    const int j = count_less_pow2(tile, tloc, [&](int q) { return tl[q]; });
    const int anc = bb * tile + j;
    return anc < N - 1 ? anc : N - 1;
}

// 16-byte store of a particle pair.  stream = 1: non-temporal, the lines leave the XCD's L2 as they are written.  A launch
// whose workgroups are all resident at once ends with every L2 full of dirty lines (2 MB per XCD at N = 2^20), and the
// write-back at the end of the kernel is then serial time: 15.9 -> 14.3 us per step at N = 2^20.  Grids of several
// residency waves overlap that write-back with the next workgroups' arithmetic and lose 3 % with streaming stores.
typedef double f64x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_pair(double* p, double v0, double v1, int stream) {
    if (stream) {
        f64x2_t v = {v0, v1};
        __builtin_nontemporal_store(v, reinterpret_cast<f64x2_t*>(p));
    } else *reinterpret_cast<double2*>(p) = make_double2(v0, v1);
}
template <int MODEL, int NT, bool BIG = false, int TILE = kTile, int RS = -1, bool WL2 = false, bool RESIDENT = false>
__global__ __launch_bounds__(NT) void k_filter_step(const StepArgs a) {
    constexpr int NK = TILE / 2 / NT;
    constexpr bool HOT = RS >= 0;
    static_assert(!RESIDENT || HOT, "the compiled-in schedule exists for the RS >= 0 kernels only");
    static_assert(NK >= 1 && NK * NT * 2 == TILE, "tile = 2 NT NK particles");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nT2 = (BIG || a.Bpow2 < 2) ? 2 : a.Bpow2;      // BIG: level-2 comes from k_level2_plan, no tables in LDS
    // the staged tiles come FIRST: their LDS address is then a compile-time constant and every search probe is a
    // ds_read_b64 with the level's offset in its immediate field (the level-2 tables behind them are indexed at run time anyway)
    double* lds_stage = reinterpret_cast<double*>(smem);         // [3][TILE] staged cdf tiles, 16-byte aligned
    double* lds_T = lds_stage + kStageTiles * TILE;              // [Bpow2] inclusive prefixes of A'
    double* lds_R = lds_T + nT2;                                 // [Bpow2] A_b / A'_b
    __shared__ double lds_seg_a[16];
    __shared__ double lds_seg_l2[64];
    __shared__ double lds_seg_c[16];
    __shared__ int lds_cnt[2];
    __shared__ double lds_R3[4];         // A_b / A'_b of the staged tiles
    __shared__ double lds_d1[16];
    __shared__ double lds_d2[16];
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];

    const int tid = threadIdx.x;
    load_log_table<NT>(&lds_dtab);        // visible after the first barrier below (every path has one before its first draw)
    load_exp_table<NT>(lds_etab);        // first used behind level2_scan's first barrier (block max)
    // (filter, tile) of this workgroup: the launch's tiles in filter-major order, a contiguous range per XCD
    const int gtile = xcd_tile_of_block((int)(blockIdx.x + gridDim.x * blockIdx.y), (int)(gridDim.x * gridDim.y));
    const int r = gtile / (int)gridDim.x, bloc = gtile - r * (int)gridDim.x;
    const int b = bloc + a.tile0;                       // global tile id (tile0 = 0 unless the filter is sharded over GPUs)
    const int out0 = a.tile0 * TILE, win0 = a.win_tile0 * TILE;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const uint32_t key0 = a.keyp[0], key1 = a.keyp[1];
    const size_t rowoff = (size_t)r * a.Npad;
    const ModelConst mc = a.mc[r];
    constexpr int DX = model_dx<MODEL>(), DY = model_dy<MODEL>();           // 1 unless a user model says otherwise (model_api.h)
    constexpr bool VEC = DX > 1 || DY > 1;
    const double y = a.by_value ? a.y_now : a.y[(size_t)a.yi * DY];
    const double zcov = a.by_value ? a.z_now : (a.z ? a.z[a.yi] : 0.0);
    constexpr int KC = model_kcov<MODEL>();                                 // covariates of a dim_cov user model, 0 otherwise
    CovVals<KC> zc;
    if constexpr (KC > 0) {
#pragma unroll
        for (int j = 0; j < KC; ++j)
            zc.v[j] = a.by_value ? (j ? a.z_now_v[j > 0 ? j - 1 : 0] : a.z_now) : (a.z ? a.z[(size_t)a.yi * KC + j] : 0.0);
    }
    const int rsm = HOT ? RS : a.resampler;
    const bool first_step = !HOT && a.t == 0;
    const bool resampled = HOT ? true : ((a.t > 0) && (a.t % a.resamp_sched == 0));
    const bool need_l2 = HOT ? true : ((a.t > 0) && (resampled || (!BIG && bloc == 0 && a.finalize_prev)));
    const bool sorted = rsm != RESAMP_MULTINOMIAL_IID;
    uint32_t* const anc_p = HOT ? nullptr : a.anc;
    double* const logw_p = HOT ? nullptr : a.logw;
    const int i_first = b * TILE;
    const int nvalid = (a.N - i_first) < TILE ? (a.N - i_first) : TILE;    // valid outputs in this tile (>= 1)
    const bool ragged = nvalid < TILE;                                     // uniform: this tile holds particles beyond N

    STAMP(a, 0);
    PRIO_AT(0);
    // --- issue the level-2 loads first: previous step's tile sums and maxima ---
    constexpr int NE = 2048 / NT;
    double A2[NE], M2[NE], ApL2[NE];
    // Filters of at most 128 tiles (512 filters x 2^14: eight tiles each; one filter of 2^16: 128): every WAVE holds all tile
    // sums, two per lane (entries lane and lane + 64), and takes the level-2 by itself -- wave max, wave scans, no LDS
    // hand-over and one barrier less.  Afterwards a thread keeps the entry the general layout gives it (j = tid: the low
    // half in wave 0, the high half in wave 1), so everything after the level-2 reads the same registers; the other waves'
    // copies fail every `j < B` test below.  Integer sums and a max: the same bits as the block-wide form.
    // (a template parameter, WL2 = the host's "B <= 128": as a run-time branch its mere presence cost the N = 2^20 kernel 2 %)
    const bool wave_l2 = WL2 && !BIG && need_l2;
    double Ahi = 0.0, Mhi = 0.0;
    if (wave_l2) {
        const int ln = tid & 63;
#pragma unroll
        for (int e = 0; e < NE; ++e) { A2[e] = 0.0; M2[e] = 0.0; }
        if (ln < a.B) { A2[0] = a.tsum_in[(size_t)r * a.Bs + ln]; M2[0] = a.tmax_in[(size_t)r * a.Bs + ln]; }
        if (a.B > 64 && ln + 64 < a.B) { Ahi = a.tsum_in[(size_t)r * a.Bs + ln + 64]; Mhi = a.tmax_in[(size_t)r * a.Bs + ln + 64]; }
    } else if (need_l2 && !BIG) level2_load<NT>(a.tsum_in + (size_t)r * a.Bs, a.tmax_in + (size_t)r * a.Bs, a.B, A2, M2);
    const double* l2T = a.l2_T + (size_t)r * a.Bs;
    const double* l2R = a.l2_R + (size_t)r * a.Bs;
    // T'_j of the split level-2 = l2_offs[j / 1024] + l2_tsrc[j]: a table plus zeros (k_level2_plan / k_l2_ranges), or block
    // offset + block-local scan (l2_inkernel) -- one expression, no branch at the reads
    const bool l2ink = BIG && a.l2_inkernel;
    const double* l2ts = a.l2_tsrc + (size_t)r * a.Bs;
    const double* l2of = a.l2_offs + (size_t)r * a.l2_offs_stride;
    auto l2Tg = [&](int j) -> double { return l2of[j >> 10] + l2ts[j]; };
    // l2_inkernel: wave 0 looks for this tile's source range itself; the 64 entries around its own tile id, requested now
    // (two loads; their sum is taken where it is needed, after the other loads of the head have been issued)
    const int l2w0 = (b - 32 < 0 || a.B <= 64) ? 0 : (b - 32 > a.B - 64 ? a.B - 64 : b - 32);
    double l2win_o = 0.0, l2win_t = dinf();
    if (l2ink && need_l2 && sorted && tid < 64 && l2w0 + tid < a.B) { l2win_o = l2of[(l2w0 + tid) >> 10]; l2win_t = l2ts[l2w0 + tid]; }
    if (tid == 0) { lds_cnt[0] = 0; lds_cnt[1] = 0; }
    double gam = 0.0, pgam = 0.0, pgam_next = 0.0, G = 1.0, u0 = 0.0;
    const bool multinomial = resampled && rsm == RESAMP_MULTINOMIAL;
    if (resampled) draw_consts(a, rsm, r, rep, G, u0);
    if (multinomial) {
        const size_t gidx = ((size_t)a.gi * a.R + r) * a.B + b;
        gam = a.gam[gidx]; pgam = a.pgam[gidx];
        pgam_next = (b + 1 < a.B) ? a.pgam[gidx + 1] : G;
    }

    STAMP(a, 1);
    PRIO_AT(1);
    // --- level-2: global max, rescaled tile sums A', inclusive prefixes T', total S'; tile range of my targets ---
    double S = 0.0;
    double t_scale = 0.0;
    if (need_l2 && BIG) {
        // split level-2: S', T', A/A' and this tile's source range were computed once per filter by k_level2_plan
        S = a.scal[r].S;
        double t_lo, t_hi;
        tile_target_bounds(rsm, S, a.N, i_first, nvalid, pgam, pgam_next, G, u0, t_scale, t_lo, t_hi);
        if (l2ink && sorted && tid < 64) {
            // lo = #{T'_j < t_lo}, hi = #{T'_j < t_hi}.  T' is nondecreasing, so the window [w0, w0 + 64) gives a count
            // exactly when it brackets the target: something below it inside (or w0 = 0) and something not below it inside (or
            // the window reaches B).  Weights that are not wildly uneven put the targets of tile b a few tiles from b; beyond
            // that a 64-ary descent (strides 256, 4, 1: three rounds for 16384 tiles) finds the same counts.
            const bool at_end = l2w0 + 64 >= a.B;
            const double l2win = l2win_o + l2win_t;
            int lo = __popcll(__ballot(l2win < t_lo)), hi = __popcll(__ballot(l2win < t_hi));
            const bool ok = (lo > 0 || l2w0 == 0) && (lo < 64 || at_end) && (hi > 0 || l2w0 == 0) && (hi < 64 || at_end);
            lo += l2w0; hi += l2w0;
            if (!ok) {
                lo = 0; hi = 0;
                auto round = [&](int stride) {
                    const int jl = lo + (tid + 1) * stride - 1, jh = hi + (tid + 1) * stride - 1;
                    const double vl = jl < a.B ? l2Tg(jl) : dinf(), vh = jh < a.B ? l2Tg(jh) : dinf();
                    lo += __popcll(__ballot(vl < t_lo)) * stride;
                    hi += __popcll(__ballot(vh < t_hi)) * stride;
                };
                round(256); round(4); round(1);
            }
            if (tid == 0) { lds_cnt[0] = lo; lds_cnt[1] = hi; }
        }
    }
    if (need_l2 && !BIG) {
        double Tinc[NE];
        double m;
#ifdef SSME_ABLATE
        if (a.stamps) { asm volatile("" :: "v"(A2[0]), "v"(M2[0])); }   // force the loads to have landed
        STAMP(a, 13);
#endif
        if (wave_l2) {
            __syncthreads();                               // the LDS tables and lds_cnt = 0 (level2_scan's first barrier otherwise)
            const int ln = tid & 63;
            const bool two = a.B > 64;                     // uniform: a second entry per lane
            const bool v0 = ln < a.B, v1 = two && (ln + 64 < a.B);
            const double mv = M2[0];
            bool nanv = v0 && (mv != mv);
            double mx = (v0 && !nanv) ? mv : -dinf();
            if (two) {
                const bool n1 = v1 && (Mhi != Mhi);
                if (v1 && !n1) mx = (Mhi > mx) ? Mhi : mx;
                nanv = nanv || n1;
            }
            const double mw = wave_max_f64(mx);
            m = __ballot(nanv) ? dnan() : mw;
#pragma unroll
            for (int e = 0; e < NE; ++e) { ApL2[e] = 0.0; Tinc[e] = 0.0; }
            if (v0) ApL2[0] = __builtin_rint(A2[0] * dexp_scaled_t(mv - m, a.rshift - kTileShift, lds_etab));
            Tinc[0] = wave_incl_scan_f64(ApL2[0]);
            S = readlane_f64(Tinc[0], 63);
            if (two) {
                double Ap1 = 0.0;
                if (v1) Ap1 = __builtin_rint(Ahi * dexp_scaled_t(Mhi - m, a.rshift - kTileShift, lds_etab));
                const double T1 = S + wave_incl_scan_f64(Ap1);
                S = readlane_f64(T1, 63);
                if ((tid >> 6) == 1) { A2[0] = Ahi; ApL2[0] = Ap1; Tinc[0] = T1; }       // the general layout: thread j = tid holds entry j
            }
        } else
        level2_scan<NT>(A2, M2, a.B, a.rshift, m, ApL2, Tinc, S, lds_d1, lds_seg_l2, lds_etab);
        STAMP(a, 14);
        // bounds [t_lo, t_hi] of this tile's targets, known to every thread without the spacings
        double t_lo = 0.0, t_hi = dinf();
        tile_target_bounds(rsm, S, a.N, i_first, nvalid, pgam, pgam_next, G, u0, t_scale, t_lo, t_hi);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e * NT < a.Bpow2) {
                const int j = e * NT + tid;
                if (j < a.Bpow2) lds_T[j] = (j < a.B) ? Tinc[e] : dinf();
                if (resampled && sorted) {
                    // #{T'_j < t_lo}, #{T'_j < t_hi}: wave popcounts, one LDS atomic per wave
                    const int w_lo = __popcll(__ballot(j < a.B && Tinc[e] < t_lo));
                    const int w_hi = __popcll(__ballot(j < a.B && Tinc[e] < t_hi));
                    if ((tid & 63) == 0) { if (w_lo) atomicAdd(&lds_cnt[0], w_lo); if (w_hi) atomicAdd(&lds_cnt[1], w_hi); }
                }
            }
        }
        STAMP(a, 15);
        if (bloc == 0 && tid == 0 && a.finalize_prev) {
            const double ll = account_step(a.scal + r, m, S, a.rshift, resampled, a.logN);
            if (a.per_step) a.per_step[(size_t)r * a.Tcap + (a.t - 1)] = ll;
        }
    }
    STAMP(a, 2);
    PRIO_AT(2);

    // --- request the cdf tiles my targets fall into (coalesced 16-byte loads into registers) ---
    int bb_min = 0, span = kStageTiles + 1;
    StagedTiles<NT, NK, TILE> stg;
    const double* cdf_r = a.cdf_in + rowoff;
    const double* xin_r = a.x_in + rowoff;
    if (resampled) {
        __syncthreads();          // lds_T, lds_cnt visible
        if (sorted) {
            int lo, hi;
            if (BIG && !l2ink) { lo = a.l2_lo[(size_t)r * a.Bs + b]; hi = a.l2_hi[(size_t)r * a.Bs + b]; }
            else { lo = lds_cnt[0]; hi = lds_cnt[1]; }
            lo = lo < a.B - 1 ? lo : a.B - 1;
            hi = hi < a.B - 1 ? hi : a.B - 1;
            bb_min = __builtin_amdgcn_readfirstlane(lo);
            span = __builtin_amdgcn_readfirstlane(hi) - bb_min + 1;
        }
        clamp_to_window(a.win_flag, a.win_tile0, a.win_tiles, a.B, bb_min, span);
        if (!BIG) publish_ratios<NT>(A2, ApL2, a.B, a.Bpow2, bb_min, span, lds_R3, lds_R);
        stg.load(cdf_r + (size_t)(bb_min - a.win_tile0) * TILE, span);
    }
    STAMP(a, 3);
    PRIO_AT(3);

    // --- exponential spacings of the multinomial resampler (liu_west_filter.h:105-139), exact tile scan;
    //     this arithmetic hides the latency of the tile loads ---
    double tau[NK][2];                    // integer resampling targets in [0, S']
    uint32_t nw0[NK], nw1[NK];            // words 0-1 of each pair's Philox output: the propagation normals (below)
    if (!resampled) __syncthreads();      // the log table is in LDS (the resampling path has passed a barrier already)
    auto pair_draw = [&](int k) {
        const u32x4 o = pair_words((uint32_t)(b * (TILE / 2) + k * NT + tid), (uint32_t)a.t, rep, key0, key1);
        nw0[k] = o.v0; nw1[k] = o.v1;
        return o;
    };
    if (multinomial) {
        multinomial_targets<NT, NK, TILE>([&](int k, double& e0, double& e1) {
            const u32x4 o = pair_draw(k);
            if (ABL(a, 1)) { e0 = 1.0 + 1e-6 * (double)((i_first + (k * NT + tid) * 2) & 1023); e1 = 1.0; }
            else pair_spacings(o, lds_dtab.log, &e0, &e1);
        }, i_first, a.N, gam, pgam, t_scale, lds_seg_a, tau);
    } else {
#pragma unroll
        for (int k = 0; k < NK; ++k) pair_draw(k);
    }
    STAMP(a, 4);
    PRIO_AT(4);

    double xin[NK][2], lw_old[NK][2];
    int srcv[NK][2];                      // vector states: where the other components of the source particle are
#pragma unroll
    for (int k = 0; k < NK; ++k) { srcv[k][0] = 0; srcv[k][1] = 0; }
    if (first_step) {
#pragma unroll
        for (int k = 0; k < NK; ++k) { xin[k][0] = 0.0; xin[k][1] = 0.0; lw_old[k][0] = 0.0; lw_old[k][1] = 0.0; }
    } else if (!resampled) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const size_t idx = rowoff + (size_t)(i_first - out0) + (k * NT + tid) * 2;
            const double2 xv = *reinterpret_cast<const double2*>(a.x_in + idx);
            const double2 lv = *reinterpret_cast<const double2*>(logw_p + idx);
            xin[k][0] = xv.x; xin[k][1] = xv.y; lw_old[k][0] = lv.x; lw_old[k][1] = lv.y;
            if constexpr (DX > 1) { srcv[k][0] = i_first + (k * NT + tid) * 2; srcv[k][1] = srcv[k][0] + 1; }
        }
    } else {
        // --- the other resamplers' targets ---
        if (rsm != RESAMP_MULTINOMIAL) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i0 = i_first + (k * NT + tid) * 2;
                if (rsm == RESAMP_SYSTEMATIC) {
                    tau[k][0] = __builtin_ceil(((double)i0 + u0) * t_scale);
                    tau[k][1] = __builtin_ceil(((double)(i0 + 1) + u0) * t_scale);
                } else {
                    const u32x4 o = philox4x32_10((uint32_t)(i0 >> 1), (uint32_t)a.t, rep, STREAM_RESAMP, key0, key1);
                    const double v0 = u01_co(o.v0, o.v1), v1 = u01_co(o.v2, o.v3);
                    if (rsm == RESAMP_STRATIFIED) {
                        tau[k][0] = __builtin_ceil(((double)i0 + v0) * t_scale);
                        tau[k][1] = __builtin_ceil(((double)(i0 + 1) + v1) * t_scale);
                    } else {
                        tau[k][0] = __builtin_ceil(v0 * S);
                        tau[k][1] = __builtin_ceil(v1 * S);
                    }
                }
            }
        }

        auto Tof = [&](int j) -> double { return BIG ? l2Tg(j) : lds_T[j]; };                              // j < B
        auto Tinf = [&](int j) -> double { return BIG ? (j < a.B ? l2Tg(j) : dinf()) : lds_T[j]; };        // lds_T holds +inf beyond B
        if (span <= kStageTiles) {
            // --- staged tiles -> LDS, then count-search in LDS ---
            stg.store(lds_stage, span);
            double Pm, T0, T1, R0, R1, R2;
            staged_prefixes(Tof, bb_min, a.B, Pm, T0, T1);
            __syncthreads();
            if (BIG) staged_ratios([&](int j) { return l2R[j]; }, bb_min, a.B, R0, R1, R2);
            else { R0 = lds_R3[0]; R1 = lds_R3[1]; R2 = lds_R3[2]; }
            STAMP(a, 5);
            PRIO_AT(5);
            // all 2 NK count-searches of the thread descend together (staged_search_pos): positions as absolute LDS byte addresses
            uint32_t spos[NK][2];
            if (ABL(a, 2)) {
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    for (int c = 0; c < 2; ++c) spos[k][c] = lds_addr(lds_stage) + (((uint32_t)(d2bits(tau[k][c]) >> 20) & 2047u) << 3);
            } else staged_search_pos<TILE, NK>(tau, span, Pm, T0, T1, R0, R1, R2, lds_stage, spos);
            // gather: the ancestor's state at a 32-bit byte offset from a uniform base (no 64-bit address arithmetic per lane).
            // ancestor = bb_min TILE + (position - stage) / 8, so its byte offset is the position plus a uniform: one add.  A count
            // is at most TILE - 1, so an ancestor can pass N - 1 only in the filter's last tile when that tile is ragged: the
            // clamp to N - 1 sits behind that uniform condition (kept a branch, as the ragged output tile's).
            const unsigned char* xbase = reinterpret_cast<const unsigned char*>(xin_r - win0);
            const uint32_t pos2byte = (uint32_t)bb_min * (uint32_t)(TILE * 8) - lds_addr(lds_stage);
            const bool last_src_ragged = bb_min + span >= a.B && a.B * TILE > a.N;
            uint32_t goff[NK][2];
#pragma unroll
            for (int k = 0; k < NK; ++k) { goff[k][0] = spos[k][0] + pos2byte; goff[k][1] = spos[k][1] + pos2byte; }
            if (last_src_ragged) {
                asm volatile("");
                const uint32_t top = (uint32_t)(a.N - 1) << 3;
#pragma unroll
                for (int k = 0; k < NK; ++k) { goff[k][0] = goff[k][0] < top ? goff[k][0] : top; goff[k][1] = goff[k][1] < top ? goff[k][1] : top; }
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int i = i_first + (k * NT + tid) * 2 + c;
                    if (anc_p && i < a.N) anc_p[rowoff + i - out0] = goff[k][c] >> 3;
                    xin[k][c] = *reinterpret_cast<const double*>(xbase + goff[k][c]);
                    if constexpr (DX > 1) srcv[k][c] = (int)(goff[k][c] >> 3);
                    lw_old[k][c] = 0.0;
                }
            }
        } else {
            // general path (iid multinomial, or an output tile spanning many cdf tiles): probes in L2
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int anc = probe_ancestor(tau[k][c], Tinf, [&](int j) { return BIG ? l2R[j] : lds_R[j]; }, cdf_r, a.B, a.Bpow2, TILE,
                                                   a.win_tile0, a.N);
                    const int i = i_first + (k * NT + tid) * 2 + c;
                    if (anc_p && i < a.N) anc_p[rowoff + i - out0] = (uint32_t)anc;
                    xin[k][c] = xin_r[anc - win0];
                    if constexpr (DX > 1) srcv[k][c] = anc;
                    lw_old[k][c] = 0.0;
                }
            }
        }
    }
    STAMP(a, 6);
    PRIO_AT(6);

    // --- standard normals (Box-Muller); this arithmetic hides the latency of the ancestor gather ---
    double zn[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (ABL(a, 0)) { zn[k][0] = 0.25 + 1e-9 * (double)nw0[k]; zn[k][1] = -0.25; }
        else pair_normals(nw0[k], nw1[k], &lds_dtab, &zn[k][0], &zn[k][1]);
    }
    STAMP(a, 7);
    PRIO_AT(7);

    // --- fSamp / q1Samp, logGEv, tile max ---
    double lg[NK][2];
    double mx = -dinf();
    bool nan = false;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i0 = i_first + (k * NT + tid) * 2;
        double xo[2];
        double xov[VEC ? kMaxDim : 1][2];  // components 1 .. of a vector state
        if constexpr (VEC) {
#if SSME_HAS_USER_MODEL
            // vector state / observation (user model with dim_x or dim_y > 1): component 0 travels the scalar path above (gather, the
            // pair's Box-Muller draw); components d >= 1 are gathered from their planes at the same source index and take their
            // normals from one more Philox call per pair each (counter stream STREAM_XDIM + d)
            double yv[kMaxDim];
            yv[0] = y;
#pragma unroll
            for (int d = 1; d < DY; ++d) yv[d] = a.by_value ? a.y_now_v[d - 1] : a.y[(size_t)a.yi * DY + d];
            double znd[kMaxDim][2];
            znd[0][0] = zn[k][0]; znd[0][1] = zn[k][1];
#pragma unroll
            for (int d = 1; d < DX; ++d) {
                const u32x4 o = xdim_words((uint32_t)(b * (TILE / 2) + k * NT + tid), (uint32_t)a.t, rep, d, key0, key1);
                pair_normals(o.v0, o.v1, &lds_dtab, &znd[d][0], &znd[d][1]);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                double xv[kMaxDim], zv[kMaxDim], xn[kMaxDim];
                xv[0] = xin[k][c];
#pragma unroll
                for (int d = 1; d < DX; ++d) xv[d] = first_step ? 0.0 : a.x_in[(size_t)d * a.xplane + rowoff + (size_t)srcv[k][c]];
#pragma unroll
                for (int d = 0; d < DX; ++d) zv[d] = znd[d][c];
                const double gv = vector_step<MODEL>(mc, first_step, xv, zv, yv, zcov, zc, xn, lds_etab);
                xo[c] = xn[0];
#pragma unroll
                for (int d = 1; d < DX; ++d) xov[d][c] = xn[d];
                lg[k][c] = lw_old[k][c] + gv;
            }
#endif
        } else {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double xn, gv;
            if (KC == 0 && ABL(a, 3)) {       // diagnostic build: the proposal alone and a stand-in for log g
                xn = first_step ? zn[k][c] * mc.a2 : model_prop<MODEL>(mc, xin[k][c], zn[k][c], zcov, lds_etab);
                gv = -0.5 * xn * xn;
            } else gv = scalar_step<MODEL>(mc, first_step, xin[k][c], zn[k][c], y, zcov, zc, &xn, lds_etab);
            xo[c] = xn;
            lg[k][c] = lw_old[k][c] + gv;
        }
        }
        if (ragged) {                     // particles beyond N: state 0, log-weight -inf (weight 0, no part in the maximum)
            asm volatile("");
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (!((i0 + c) < a.N)) {
                    xo[c] = 0.0; lg[k][c] = -dinf();
                    if constexpr (DX > 1) { for (int d = 1; d < DX; ++d) xov[d][c] = 0.0; }
                }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) { const double l = lg[k][c]; nan = nan || (l != l); mx = (l > mx) ? l : mx; }
        const size_t idx = rowoff + (size_t)(i0 - out0);
        store_pair(reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(a.x_out + rowoff + (size_t)(i_first - out0)) + (uint32_t)(k * NT + tid) * 16u),
                   xo[0], xo[1], RESIDENT ? 1 : a.stream_stores);
        if (logw_p) *reinterpret_cast<double2*>(logw_p + idx) = make_double2(lg[k][0], lg[k][1]);
        if constexpr (DX > 1) {
#pragma unroll
            for (int d = 1; d < DX; ++d) *reinterpret_cast<double2*>(a.x_out + (size_t)d * a.xplane + idx) = make_double2(xov[d][0], xov[d][1]);
        }
    }
    STAMP(a, 8);
    PRIO_AT(8);
    const double mb = block_max_nanprop<NT>(mx, nan, lds_d2);
    STAMP(a, 9);
    PRIO_AT(9);

    // --- tile-local fixed-point weights and their exact inclusive scan (the next step's cdf) ---
    double q[NK][2], inc[NK][2], total;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (ABL(a, 4)) { q[k][0] = (double)(d2bits(lg[k][0] - mb) >> 24); q[k][1] = (double)(d2bits(lg[k][1] - mb) >> 24); }
        else {
            // (a particle beyond N carries log-weight -inf: the clamped exp makes its q exactly 0, no mask needed)
            q[k][0] = __builtin_rint(dexp_scaled_t(lg[k][0] - mb, kTileShift, lds_etab));
            q[k][1] = __builtin_rint(dexp_scaled_t(lg[k][1] - mb, kTileShift, lds_etab));
        }
    }
    if (ABL(a, 5)) {
#pragma unroll
        for (int k = 0; k < NK; ++k) { inc[k][0] = q[k][0]; inc[k][1] = q[k][0] + q[k][1]; }
        total = inc[0][1] + 1048576.0;
    } else block_scan_f64<NT, NK>(q, inc, total, lds_seg_c);
    STAMP(a, 12);
    PRIO_AT(12);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        store_pair(reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(a.cdf_out + rowoff + (size_t)(i_first - out0)) + (uint32_t)(k * NT + tid) * 16u),
                   inc[k][0], inc[k][1], RESIDENT ? 1 : a.stream_stores);
    }
    STAMP(a, 10);
    PRIO_AT(10);
    bool fused_accounting = false;
    if constexpr (!HOT && !BIG) fused_accounting = a.ticket != nullptr;
    if (tid == 0) {
        double* ts = a.tsum_out + (size_t)r * a.Bs + (b - a.tile0);
        double* tm = a.tmax_out + (size_t)r * a.Bs + (b - a.tile0);
        if (fused_accounting) {      // device-coherent stores: another workgroup (another XCD, another L2) reads them in this launch
            __hip_atomic_store(ts, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(tm, mb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else { *ts = total; *tm = mb; }
    }
    if constexpr (!HOT && !BIG) {
        if (fused_accounting) {
            // Step API (mod.filter(y); mod.getLogCondLike()): the workgroup that arrives last at its filter's counter does
            // what kf_finalize does in a second launch -- level-2 of the weights just written, log p(y_t | y_{1:t-1}) --
            // so that a filter() call is ONE launch.  Only the tile sums / maxima cross workgroups: they are written and read
            // with device-scope accesses and ordered by the counter, so no cache write-back of the particle arrays is needed.
            // Ordering.  The formally ordered form -- an ACQ_REL read-modify-write of the counter at agent scope -- was measured
            // (round 3, tools/step_latency.cpp): the release half is a write-back of the XCD's whole L2 (buffer_wbl2 sc1) and the
            // acquire half an invalidate (buffer_inv sc1), i.e. the cache write-back of the particle arrays this design exists
            // to avoid: filter() 27.8 -> 40.0 us at N = 2^20, 41 -> 55 us for 64 filters x 2^14 (profiles/r03_step_api_handover.txt).
            // Kept instead: agent-scope RELAXED atomic stores of the two values (global_store_dwordx2 ... sc1: written through
            // to the memory side, past the non-coherent L2), an explicit s_waitcnt vmcnt(0) (both stores acknowledged before
            // the next instruction issues -- the compiler's workgroup-scope release fence emits NO wait outside tgsplit mode,
            // so round 2's form left the two stores and the counter's atomic free to reach their different L2 channels in any
            // order; seen in the ISA this round, profiles/r03_step_api_handover.txt), then the agent-scope relaxed atomic add;
            // the last arriver reads with agent-scope atomic loads (global_load_dwordx2 ... sc1: not served from its own L2),
            // issued only after the atomic's return value has arrived.  The C++ memory model gives relaxed atomics on different
            // addresses no inter-thread order; this form leans on the completion wait instead of a scope-wide fence.  Cost: one
            // thread per workgroup waits for two store acknowledgements at the end of the kernel (measured: none,
            // profiles/r03_step_api_handover.txt).
            __shared__ int lds_last;
            if (tid == 0) {
                int last = 1;
                if (gridDim.x > 1) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the two stores above have been acknowledged
                    last = __hip_atomic_fetch_add(a.ticket + r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
                }
                lds_last = last;
            }
            __syncthreads();
            if (lds_last) {
                constexpr int NE2 = 2048 / NT;
                double A2[NE2], M2[NE2], Ap2[NE2], Tinc2[NE2], S2, m2;
#pragma unroll
                for (int e = 0; e < NE2; ++e) {
                    const int j = e * NT + tid;
                    A2[e] = 0.0; M2[e] = 0.0;
                    if (j < a.B) {
                        A2[e] = __hip_atomic_load(a.tsum_out + (size_t)r * a.Bs + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        M2[e] = __hip_atomic_load(a.tmax_out + (size_t)r * a.Bs + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                level2_scan<NT>(A2, M2, a.B, a.rshift, m2, Ap2, Tinc2, S2, lds_d1, lds_seg_l2, lds_etab);
                if (tid == 0) {
                    const double ll = account_step(a.scal + r, m2, S2, a.rshift, (a.t + 1) % a.resamp_sched == 0, a.logN);
                    if (a.per_step) a.per_step[(size_t)r * a.Tcap + a.t] = ll;
                    if (gridDim.x > 1) __hip_atomic_store(a.ticket + r, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch (kernel boundary orders it)
                    if (a.ll_host) a.ll_host[r] = ll;
                }
            }
        }
    }
#ifdef SSME_ABLATE
    __syncthreads();
    STAMP(a, 11);
    PRIO_AT(11);
#endif
}

// ---------------------------------------------------------------------------------------
// KF: account the last step's log conditional likelihood.  grid = (R), block = 256.
// Reads the tile sums / maxima the last k_filter_step wrote (passed as tsum_in / tmax_in).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kf_finalize(const StepArgs a) {
    __shared__ double lds_seg[128];
    __shared__ double lds_d[16];
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    double A2[8], Ap[8], Tinc[8], M2[8], S, m;
    level2_load<kThreads>(a.tsum_in + (size_t)r * a.Bs, a.tmax_in + (size_t)r * a.Bs, a.B, A2, M2);
    level2_scan<kThreads>(A2, M2, a.B, a.rshift, m, Ap, Tinc, S, lds_d, lds_seg, kExpTable);
    if (tid == 0) {
        const double ll = account_step(a.scal + r, m, S, a.rshift, (a.t + 1) % a.resamp_sched == 0, a.logN);
        if (a.per_step) a.per_step[(size_t)r * a.Tcap + a.t] = ll;
        if (a.ll_host) a.ll_host[r] = ll;
    }
}

// ---------------------------------------------------------------------------------------
// Split level-2 for filters of more than 2048 tiles (N > 2^22; also selectable for tests): ONE workgroup per filter
// does what every workgroup of k_filter_step otherwise repeats -- global max, rescaled integer tile sums A', their exact
// inclusive scan T', the total S', A/A' -- and additionally the source-tile range [lo, hi] of every output tile
// (same tile_target_bounds, same counts), and accounts log p(y_{t-1} | .).  Same arithmetic as level2_scan: integer
// sums are exact and associative, so the results are those of the in-kernel level-2 to the bit.
// grid = (R), block = 1024, dynamic LDS = Bpow2 doubles.  a.t = the step about to run (its targets); plan_ranges = 0
// for the call that only accounts the last step's log-likelihood (the kf_finalize role).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_level2_plan(const StepArgs a, int plan_ranges) {
    constexpr int NT = 1024, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_l2[];
    double* lds_T = reinterpret_cast<double*>(smem_l2);          // [Bpow2]
    __shared__ double lds_d[16];
    __shared__ double lds_seg[16];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double* ts = a.tsum_in + (size_t)r * a.Bs;
    const double* tm = a.tmax_in + (size_t)r * a.Bs;
    double* Tp = a.l2_T + (size_t)r * a.Bs;
    double* Rp = a.l2_R + (size_t)r * a.Bs;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const bool resampled = (a.t % a.resamp_sched == 0);
    // This kernel is ONE workgroup per filter and bound by memory round trips, not by arithmetic: every tile sum and maximum
    // is therefore requested up front (tile j = k * 1024 + tid, k < 16: coalesced, all loads in flight at once) and the
    // max, the rescale and the scan run from registers.
    constexpr int KMAX = kMaxTilesSplit / NT;                    // 16
    double Areg[KMAX], Mreg[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int j = k * NT + tid;
        Areg[k] = 0.0; Mreg[k] = -dinf();
        if (j < a.B) { Areg[k] = ts[j]; Mreg[k] = tm[j]; }
    }
    // global max of the tile maxima, NaN propagating
    double mx;
    bool nan;
    reg_max_nanflag<NT, KMAX>(Mreg, a.B, mx, nan);
    const double m = block_max_nanprop<NT>(mx, nan, lds_d);
    // rescaled tile sums and their exact inclusive scan, 1024 tiles per round
    double carry = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k * NT < a.Bpow2) {
            const int j = k * NT + tid;
            double A = 0.0, Ap = 0.0;
            if (j < a.B) {
                A = Areg[k];
                const double ex = dexp_scaled_t(Mreg[k] - m, a.rshift - kTileShift, kExpTable);
                Ap = __builtin_rint(A * ex);
            }
            const double inc = wave_incl_scan_f64(Ap);
            __syncthreads();                                     // lds_seg of the previous round has been read
            if (lane == 63) lds_seg[wave] = inc;
            __syncthreads();
            const double sv = row16_incl_scan((lane & 15) < NW ? lds_seg[lane & 15] : 0.0);
            const double pre = wave ? readlane_f64(sv, wave - 1) : 0.0;
            const double T = (carry + pre) + inc;
            carry = carry + readlane_f64(sv, 15);
            if (j < a.Bpow2) lds_T[j] = (j < a.B) ? T : dinf();
            if (j < a.B) { Tp[j] = T; Rp[j] = A / Ap; }
        }
    }
    const double S = carry;
    __syncthreads();
    if (plan_ranges && resampled && a.resampler != RESAMP_MULTINOMIAL_IID) {
        double G, u0;
        draw_consts(a, a.resampler, r, rep, G, u0);
        const size_t g0 = ((size_t)a.gi * a.R + r) * a.B;
        // The source-tile range [lo, hi] of every output tile.  The bounds grow with the tile index (t_lo(b) <= t_hi(b),
        // t_lo(b) <= t_lo(b + 1)), so a thread takes CONSECUTIVE tiles and every count after its first starts where the
        // last one ended: a short gallop instead of a log2(B)-level descent (this phase is bound by the LDS traffic of one
        // CU: 2 x 14 probes per tile at B = 16384 before, 3-4 now).  The Gamma prefixes of a thread's tiles are all
        // requested before the first use (Areg / Mreg are dead by now).
        const int per = (a.B + NT - 1) / NT;                     // <= KMAX
        const int bb0 = tid * per;
        double pgreg[KMAX + 1];
#pragma unroll
        for (int k = 0; k <= KMAX; ++k) {
            const int b = bb0 + k;
            pgreg[k] = 0.0;
            if (a.resampler == RESAMP_MULTINOMIAL && k <= per && b <= a.B) pgreg[k] = (b < a.B) ? a.pgam[g0 + b] : G;
        }
        // #{ j : T'_j < t } given that every entry below `from` is < t (entries past B are +inf)
        auto count_from = [&](int from, double t) {
            int p = from, sz = 1;
            while (p + sz - 1 < a.Bpow2 && lds_T[p + sz - 1] < t) { p += sz; sz <<= 1; }
            for (sz >>= 1; sz >= 1; sz >>= 1)
                if (p + sz - 1 < a.Bpow2 && lds_T[p + sz - 1] < t) p += sz;
            return p;
        };
        int prev = 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int b = bb0 + k;
            if (k < per && b < a.B) {
                const int i_first = b * a.tile;
                const int nvalid = (a.N - i_first) < a.tile ? (a.N - i_first) : a.tile;
                double ts_, t_lo, t_hi;
                tile_target_bounds(a.resampler, S, a.N, i_first, nvalid, pgreg[k], pgreg[k + 1], G, u0, ts_, t_lo, t_hi);
                const int lo = (k == 0) ? count_less_pow2(a.Bpow2, t_lo, [&](int j) { return lds_T[j]; }) : count_from(prev, t_lo);
                const int hi = count_from(lo, t_hi);
                prev = lo;
                a.l2_lo[(size_t)r * a.Bs + b] = lo < a.B - 1 ? lo : a.B - 1;
                a.l2_hi[(size_t)r * a.Bs + b] = hi < a.B - 1 ? hi : a.B - 1;
            }
        }
    }
    if (tid == 0) {
        // (m, S) of the weights this step starts from: k_filter_step<.., true> and the forecast read them
        if (a.finalize_prev) {
            const double ll = account_step(a.scal + r, m, S, a.rshift, resampled, a.logN);
            if (a.per_step) a.per_step[(size_t)r * a.Tcap + (a.t - 1)] = ll;
            if (a.ll_host) a.ll_host[r] = ll;
        } else { a.scal[r].m = m; a.scal[r].S = S; }
    }
}

// ---------------------------------------------------------------------------------------
// The same split level-2 over SEVERAL workgroups, for filters of more than 1024 tiles.  k_level2_plan is one workgroup per
// filter and its time grows with the number of tiles (B = 4096: 15 us, 16384: 51 us per launch -- a sixth of the step at
// N >= 2^23, and every rank of a sharded filter plans ALL tiles); here workgroup g takes tiles [1024 g, 1024 g + 1024):
//   k_l2_scan_blocks  global max (every workgroup reads all maxima itself), rescaled sums A', A / A', the inclusive scan
//                     of its own 1024 tiles and their total
//   k_l2_ranges       offsets from the (at most 16) totals, T' = local scan + offset for all tiles into LDS and for its
//                     own tiles into l2_T, source ranges of its own tiles, and (workgroup 0) the accounting.
// Integer sums are exact, so T', S', the ranges and the log-likelihood are k_level2_plan's to the bit.
// grid = (ceil(B / 1024), R), block = 1024; k_l2_ranges: dynamic LDS = Bpow2 doubles.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_l2_scan_blocks(const StepArgs a) {
    constexpr int NT = 1024, NW = NT / 64, KMAX = kMaxTilesSplit / NT;
    __shared__ double lds_d[16];
    __shared__ double lds_seg[16];
    const int tid = threadIdx.x, blk = blockIdx.x, r = blockIdx.y;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double* ts = a.tsum_in + (size_t)r * a.Bs;
    const double* tm = a.tmax_in + (size_t)r * a.Bs;
    double Mreg[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int j = k * NT + tid;
        Mreg[k] = (j < a.B) ? tm[j] : -dinf();
    }
    const int jo = blk * NT + tid;
    const double A = (jo < a.B) ? ts[jo] : 0.0;
    const double Mo = (jo < a.B) ? tm[jo] : 0.0;
    double mx;
    bool nan;
    reg_max_nanflag<NT, KMAX>(Mreg, a.B, mx, nan);
    const double m = block_max_nanprop<NT>(mx, nan, lds_d);
    double Ap = 0.0;
    if (jo < a.B) Ap = __builtin_rint(A * dexp_scaled_t(Mo - m, a.rshift - kTileShift, kExpTable));
    const double inc = wave_incl_scan_f64(Ap);
    if (lane == 63) lds_seg[wave] = inc;
    __syncthreads();
    const double sv = row16_incl_scan((lane & 15) < NW ? lds_seg[lane & 15] : 0.0);
    const double pre = wave ? readlane_f64(sv, wave - 1) : 0.0;
    double* Tloc = a.l2_work + (size_t)r * a.Bs;
    double* blkv = a.l2_work + (size_t)a.R * a.Bs + (size_t)r * kL2Scratch;
    if (jo < a.B) {
        Tloc[jo] = pre + inc;
        a.l2_R[(size_t)r * a.Bs + jo] = A / Ap;
    }
    if (tid == 0 && !a.l2_inkernel) {
        blkv[blk] = readlane_f64(sv, 15);
        if (blk == 0) blkv[KMAX] = m;
    }
    if (wave == 0 && a.l2_inkernel) {
        // One launch: the workgroup that arrives last adds up the block totals.  The total goes out as an agent-scope store and
        // has left the CU (s_waitcnt) before the arrival is counted; the last arriver reads the totals with agent-scope loads
        // issued after its own count came back -- the hand-over of the step API's ticket (k_filter_step), at 16 workgroups.
        // Lane k of its first wave takes block k: one load, a 16-lane scan (integer sums: exact in any order).
        const int nblk = (int)gridDim.x;
        const double tot = readlane_f64(sv, 15);
        int arrived = 0;
        if (lane == 0) {
            __hip_atomic_store(&blkv[blk], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            arrived = __hip_atomic_fetch_add(a.l2_ticket + r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        if (arrived == nblk - 1) {
            const double v = (lane < nblk) ? __hip_atomic_load(&blkv[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            const double tinc = row16_incl_scan(v);
            const double S = readlane_f64(tinc, 15);
            double* off = blkv + kL2Offsets;
            if (lane <= KMAX) off[lane] = (lane < KMAX) ? tinc - v : S;       // exclusive offset of block k (k >= nblk: S')
            if (lane == 0) {
                __hip_atomic_store(a.l2_ticket + r, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool resampled = (a.t % a.resamp_sched == 0);
                // (m, S) of the weights this step starts from: k_filter_step<.., true> and the forecast read them
                if (a.finalize_prev) {
                    const double ll = account_step(a.scal + r, m, S, a.rshift, resampled, a.logN);
                    if (a.per_step) a.per_step[(size_t)r * a.Tcap + (a.t - 1)] = ll;
                    if (a.ll_host) a.ll_host[r] = ll;
                } else { a.scal[r].m = m; a.scal[r].S = S; }
            }
        }
    }
}

__global__ __launch_bounds__(1024) void k_l2_ranges(const StepArgs a, int plan_ranges) {
    constexpr int NT = 1024, KMAX = kMaxTilesSplit / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_l2r[];
    double* lds_T = reinterpret_cast<double*>(smem_l2r);         // [Bpow2]
    const int tid = threadIdx.x, blk = blockIdx.x, r = blockIdx.y;
    const double* Tloc = a.l2_work + (size_t)r * a.Bs;
    const double* blkv = a.l2_work + (size_t)a.R * a.Bs + (size_t)r * kL2Scratch;
    double* Tp = a.l2_T + (size_t)r * a.Bs;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const bool resampled = (a.t % a.resamp_sched == 0);
    const int nblk = (a.B + NT - 1) / NT;
    // local scans of all tiles, requested before anything else
    double Treg[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int j = k * NT + tid;
        Treg[k] = (j < a.B) ? Tloc[j] : 0.0;
    }
    double off[KMAX + 1];
    off[0] = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) off[k + 1] = off[k] + ((k < nblk) ? blkv[k] : 0.0);
    const double S = off[KMAX];
    const double m = blkv[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const int j = k * NT + tid;
        if (j < a.Bpow2) {
            const double T = off[k] + Treg[k];
            lds_T[j] = (j < a.B) ? T : dinf();
            if (k == blk && j < a.B) Tp[j] = T;
        }
    }
    __syncthreads();
    const int b = blk * NT + tid;
    if (plan_ranges && resampled && a.resampler != RESAMP_MULTINOMIAL_IID && b < a.B) {
        double G, u0, pg = 0.0, pgn = 0.0;
        draw_consts(a, a.resampler, r, rep, G, u0);
        const size_t g0 = ((size_t)a.gi * a.R + r) * a.B;
        if (a.resampler == RESAMP_MULTINOMIAL) { pg = a.pgam[g0 + b]; pgn = (b + 1 < a.B) ? a.pgam[g0 + b + 1] : G; }
        const int i_first = b * a.tile;
        const int nvalid = (a.N - i_first) < a.tile ? (a.N - i_first) : a.tile;
        double ts_, t_lo, t_hi;
        tile_target_bounds(a.resampler, S, a.N, i_first, nvalid, pg, pgn, G, u0, ts_, t_lo, t_hi);
        int lo = 0, hi = 0;
        for (int step = a.Bpow2 >> 1; step >= 1; step >>= 1) {       // the two counts descend together
            if (lds_T[lo + step - 1] < t_lo) lo += step;
            if (lds_T[hi + step - 1] < t_hi) hi += step;
        }
        a.l2_lo[(size_t)r * a.Bs + b] = lo < a.B - 1 ? lo : a.B - 1;
        a.l2_hi[(size_t)r * a.Bs + b] = hi < a.B - 1 ? hi : a.B - 1;
    }
    if (blk == 0 && tid == 0) {
        // (m, S) of the weights this step starts from: k_filter_step<.., true> and the forecast read them
        if (a.finalize_prev) {
            const double ll = account_step(a.scal + r, m, S, a.rshift, resampled, a.logN);
            if (a.per_step) a.per_step[(size_t)r * a.Tcap + (a.t - 1)] = ll;
            if (a.ll_host) a.ll_host[r] = ll;
        } else { a.scal[r].m = m; a.scal[r].S = S; }
    }
}

// ---------------------------------------------------------------------------------------
// Particle-sharded filter (one filter over `world` GPUs, B/world tiles each): the range of SOURCE tiles
// [lo, hi] that the output tiles of every rank touch at step a.t, from the gathered tile sums / maxima.
// Runs the same level-2 and the same target bounds as k_filter_step, so the ranges are exact.
// grid = 1, block = 512, dynamic LDS = max(Bpow2, 2) doubles.  lo_hi: [world][2] ints.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_shard_plan(const StepArgs a, int world, int Bl, int32_t* lo_hi, int margin = 0, int32_t* flag = nullptr) {
    constexpr int NT = 512, NE = 2048 / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_plan[];
    double* lds_T = reinterpret_cast<double*>(smem_plan);
    __shared__ double lds_seg[64];
    __shared__ double lds_d[16];
    const int tid = threadIdx.x;
    double A2[NE], M2[NE], Ap[NE], Tinc[NE], S, m;
    level2_load<NT>(a.tsum_in, a.tmax_in, a.B, A2, M2);
    level2_scan<NT>(A2, M2, a.B, a.rshift, m, Ap, Tinc, S, lds_d, lds_seg, kExpTable);
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int j = e * NT + tid;
        if (j < a.Bpow2) lds_T[j] = (j < a.B) ? Tinc[e] : dinf();
    }
    __syncthreads();
    if (tid < world) {
        const int bF = tid * Bl, bL = bF + Bl - 1 < a.B - 1 ? bF + Bl - 1 : a.B - 1;      // Bl = ceil(B / world): the last rank may own fewer
        int lo = 0, hi = a.B - 1;
        if (a.resampler != RESAMP_MULTINOMIAL_IID) {
            double G, u0, pgF = 0.0, pgFn = 0.0, pgL = 0.0, pgLn = 0.0;
            draw_consts(a, a.resampler, 0, a.first_filter, G, u0);          // R = 1
            if (a.resampler == RESAMP_MULTINOMIAL) {
                const size_t g0 = (size_t)a.gi * a.B;
                pgF = a.pgam[g0 + bF]; pgFn = (bF + 1 < a.B) ? a.pgam[g0 + bF + 1] : G;
                pgL = a.pgam[g0 + bL]; pgLn = (bL + 1 < a.B) ? a.pgam[g0 + bL + 1] : G;
            }
            const int iF = bF * a.tile, iL = bL * a.tile;
            const int nvF = (a.N - iF) < a.tile ? (a.N - iF) : a.tile, nvL = (a.N - iL) < a.tile ? (a.N - iL) : a.tile;
            double ts, t_lo, t_hi, unused;
            tile_target_bounds(a.resampler, S, a.N, iF, nvF, pgF, pgFn, G, u0, ts, t_lo, unused);
            tile_target_bounds(a.resampler, S, a.N, iL, nvL, pgL, pgLn, G, u0, ts, unused, t_hi);
            lo = count_less_pow2(a.Bpow2, t_lo, [&](int j) { return lds_T[j]; });
            hi = count_less_pow2(a.Bpow2, t_hi, [&](int j) { return lds_T[j]; });
            lo = lo < a.B - 1 ? lo : a.B - 1;
            hi = hi < a.B - 1 ? hi : a.B - 1;
        }
        lo_hi[2 * tid] = lo;
        lo_hi[2 * tid + 1] = hi;
        if (flag) {
            // C++ shard driver: does this rank's window stay inside its fixed halo?  flag[0]: some window left it;
            // flag[1] / flag[2]: widest reach left / right of the own tiles seen so far
            const int left = bF - lo, right = hi - bL;
            if (left > margin || right > margin) atomicOr(&flag[0], 1);
            if (left > 0) atomicMax(&flag[1], left);
            if (right > 0) atomicMax(&flag[2], right);
        }
    }
}

// ---------------------------------------------------------------------------------------
// Gamma tables for the multinomial resampler (data independent: seed, t, filter, tile only).
// k_gamma_draw: grid = (ceil(B/256), nT, R).  k_gamma_prefix: one workgroup per (ti, r).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_gamma_draw(double* gam, int N, int B, int R, int t0, const uint32_t* keyp,
                                                         uint32_t first_filter, uint32_t gamma_stream, int tile) {
    const uint32_t key0 = keyp[0], key1 = keyp[1];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    const int ti = blockIdx.y, r = blockIdx.z;
    if (b >= B) return;
    const int nb = (N - b * tile) < tile ? (N - b * tile) : tile;
    gam[((size_t)ti * R + r) * B + b] = gamma_draw((uint32_t)b, (uint32_t)(t0 + ti), first_filter + (uint32_t)r, key0, key1, (double)nb,
                                                   gamma_stream);
}

// One workgroup per (ti, r) row.  The exclusive prefix is the SEQUENTIAL sum run = run + g[b] (its rounding is part of
// the specification), so one lane adds; but the row is brought into LDS by all 256 threads first and the prefixes leave
// through LDS as well, in chunks of 2048 tiles: the adding lane then sees LDS latency instead of one dependent global
// load per tile (a single filter step of the step API spent ~100 us here at 512 tiles).
__global__ __launch_bounds__(kThreads) void k_gamma_prefix(const double* gam, double* pgam, double* gtot, int B, int R,
                                                           int nT, int t0, const uint32_t* keyp, uint32_t first_filter,
                                                           uint32_t extra_stream) {
    __shared__ double buf[2048];
    const int id = blockIdx.x, tid = threadIdx.x;
    const int ti = id / R, r = id % R;
    const double* g = gam + (size_t)id * B;
    double* p = pgam + (size_t)id * B;
    double run = 0.0;                                  // meaningful in thread 0 only
    for (int c0 = 0; c0 < B; c0 += 2048) {
        const int n = (B - c0) < 2048 ? (B - c0) : 2048;
        for (int j = tid; j < n; j += kThreads) buf[j] = g[c0 + j];
        __syncthreads();
        if (tid == 0) {
            for (int j = 0; j < n; ++j) { const double v = buf[j]; buf[j] = run; run = run + v; }
        }
        __syncthreads();
        for (int j = tid; j < n; j += kThreads) p[c0 + j] = buf[j];
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t key0 = keyp[0], key1 = keyp[1];
        const u32x4 ox = philox4x32_10(0u, (uint32_t)(t0 + ti), first_filter + (uint32_t)r, extra_stream, key0, key1);
        gtot[id] = run + (-dlog_pn(u01_oc(ox.v0, ox.v1)));
    }
}

// the same for short rows (few tiles per filter, many filters): one thread per (ti, r)
__global__ __launch_bounds__(kThreads) void k_gamma_prefix_rows(const double* gam, double* pgam, double* gtot, int B, int R,
                                                                int nT, int t0, const uint32_t* keyp, uint32_t first_filter,
                                                                uint32_t extra_stream) {
    const uint32_t key0 = keyp[0], key1 = keyp[1];
    const int id = blockIdx.x * kThreads + threadIdx.x;
    if (id >= nT * R) return;
    const int ti = id / R, r = id % R;
    const double* g = gam + (size_t)id * B;
    double* p = pgam + (size_t)id * B;
    double run = 0.0;
    for (int b = 0; b < B; ++b) { p[b] = run; run = run + g[b]; }
    const u32x4 ox = philox4x32_10(0u, (uint32_t)(t0 + ti), first_filter + (uint32_t)r, extra_stream, key0, key1);
    gtot[id] = run + (-dlog_pn(u01_oc(ox.v0, ox.v1)));
}

// ---------------------------------------------------------------------------------------
// Weighted expectations of built-in functionals with the last step's (pre-resampling) weights
// (getExpectations(); twin liu_west_filter.h:1662-1683; callers pswarm_filter.h:87-89,383-385).
// The weights are the fixed-point weights the resampler uses: w_j = q_j exp(m_tile - m), q_j = cdf_j - cdf_{j-1}.
//   k_expect_partials  grid (B tiles, R): per tile sum_j h_f(x_j) q_j for ALL requested functionals at once (the tile's
//                      denominator sum_j q_j is its exact integer tile sum A_b, already in memory); every CU takes part
//   k_expect_final     grid (R): E_f = sum_b num_{b,f} e^{m_b - m} / sum_b A_b e^{m_b - m}
//   k_expect_mean      grid (1): the swarm aggregate, the plain mean over the R members (pswarm_filter.h:103,136)
// Summation trees are fixed (per-thread strided, wave xor tree, waves in order), so results are reproducible.
// ---------------------------------------------------------------------------------------
constexpr int kMaxFunctionals = 4;
struct FunctionalIds { int32_t n; int32_t id[kMaxFunctionals]; };

__device__ __forceinline__ double builtin_h(int functional, double xv) {
    return functional == 0 ? xv : functional == 1 ? xv * xv : functional == 2 ? dexp(0.5 * xv) : 42.0;
}
__device__ __forceinline__ double wave_sum_xor(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, kWave);
    return v;
}

// The pieces of k_expect_partials' summation tree (shared with the smoothing sweep, smooth.h): one particle into a thread's
// numerators, the wave sums of a thread's numerators into lds[f][wave], and functional f's tile sum from them (after a barrier).
__device__ __forceinline__ void expect_add(double (&num)[kMaxFunctionals], const FunctionalIds& fs, double xv, double q) {
#pragma unroll
    for (int f = 0; f < kMaxFunctionals; ++f)
        if (f < fs.n) num[f] = num[f] + builtin_h(fs.id[f], xv) * q;
}
__device__ __forceinline__ void expect_wave_sums(double (&num)[kMaxFunctionals], double (*lds)[4], int tid) {
#pragma unroll
    for (int f = 0; f < kMaxFunctionals; ++f) {
        num[f] = wave_sum_xor(num[f]);
        if ((tid & 63) == 0) lds[f][tid >> 6] = num[f];
    }
}
__device__ __forceinline__ double expect_tile_sum(const double (*lds)[4], int f) { return ((lds[f][0] + lds[f][1]) + lds[f][2]) + lds[f][3]; }

__global__ __launch_bounds__(kThreads) void k_expect_partials(const double* x, const double* cdf, int N, int Npad, int Bs, int tile,
                                                              FunctionalIds fs, double* part /*[R][Bs][kMaxFunctionals]*/) {
    __shared__ double lds[kMaxFunctionals][4];
    const int tid = threadIdx.x, b = blockIdx.x, r = blockIdx.y;
    const double* xr = x + (size_t)r * Npad + (size_t)b * tile;
    const double* cr = cdf + (size_t)r * Npad + (size_t)b * tile;
    const int nvalid = (N - b * tile) < tile ? (N - b * tile) : tile;
    double num[kMaxFunctionals] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < nvalid; j += kThreads) {
        const double q = cr[j] - (j ? cr[j - 1] : 0.0);
        expect_add(num, fs, xr[j], q);
    }
    expect_wave_sums(num, lds, tid);
    __syncthreads();
    if (tid < kMaxFunctionals) part[((size_t)r * Bs + b) * kMaxFunctionals + tid] = expect_tile_sum(lds, tid);
}

// k_expect_final's work for filter r: E_f from the per-tile numerators part[(r Bs + b) 4 + f] and the tile sums / maxima, into
// out[f R + r].  Called by every thread of a kThreads workgroup (also by the smoothing rows, smooth.h).
__device__ __forceinline__ void expect_final_filter(const double* part, const double* tsum, const double* tmax, int B, int Bs, int R, int r,
                                                    const FunctionalIds& fs, double* out /*[n][R]*/) {
    __shared__ double lds[kMaxFunctionals + 1][4];
    __shared__ double lds_m[16];
    const int tid = threadIdx.x;
    double mx = -dinf();
    bool nan = false;
    for (int j = tid; j < B; j += kThreads) { const double v = tmax[(size_t)r * Bs + j]; nan = nan || (v != v); mx = (v > mx) ? v : mx; }
    const double m = block_max_nanprop<kThreads>(mx, nan, lds_m);
    double acc[kMaxFunctionals + 1] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < B; j += kThreads) {
        const double sc = dexp(tmax[(size_t)r * Bs + j] - m);
#pragma unroll
        for (int f = 0; f < kMaxFunctionals; ++f)
            if (f < fs.n) acc[f] = acc[f] + part[((size_t)r * Bs + j) * kMaxFunctionals + f] * sc;
        acc[kMaxFunctionals] = acc[kMaxFunctionals] + tsum[(size_t)r * Bs + j] * sc;
    }
#pragma unroll
    for (int f = 0; f <= kMaxFunctionals; ++f) {
        acc[f] = wave_sum_xor(acc[f]);
        if ((tid & 63) == 0) lds[f][tid >> 6] = acc[f];
    }
    __syncthreads();
    if (tid < fs.n) {
        const double n4 = ((lds[tid][0] + lds[tid][1]) + lds[tid][2]) + lds[tid][3];
        const double d4 = ((lds[kMaxFunctionals][0] + lds[kMaxFunctionals][1]) + lds[kMaxFunctionals][2]) + lds[kMaxFunctionals][3];
        out[(size_t)tid * R + r] = (m != m) ? dnan() : n4 / d4;
    }
}

__global__ __launch_bounds__(kThreads) void k_expect_final(const double* part, const double* tsum, const double* tmax, int B, int Bs,
                                                           int R, FunctionalIds fs, double* out /*[n][R]*/) {
    expect_final_filter(part, tsum, tmax, B, Bs, R, blockIdx.x, fs, out);
}

// Swarm aggregation in one launch: block f < n: mean over the R members of expectation row f ([n][R] in exp_rows);
// block n: mean of the members' last log conditional likelihoods.  out: n + 1 doubles at
// out[0..n) and out[slot_ll] (device-mapped host memory: the host polls it).  grid (n + 1), block 256.
// num_threads > 0: the reference's mean of per-thread means -- split_data_thread_pool deals member i to thread i % num_threads
// (thread_pool.h:443-447), every thread averages its own members (intra_agg_func, pswarm_filter.h:130-160) and the thread
// averages are averaged (inter_agg_func, :96-128).  That is a weighted mean with weight 1 / (num_threads * members of the
// thread), equal to the plain mean only when num_threads divides R.  num_threads <= 0: the plain mean.
__global__ __launch_bounds__(kThreads) void k_swarm_means(const double* exp_rows, const FilterScalars* scal, int R, int n, int slot_ll,
                                                          double* out, int num_threads) {
    __shared__ double lds[4];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int T = (num_threads > 0 && num_threads < R) ? num_threads : (num_threads >= R ? R : 0);
    double s = 0.0;
    for (int r = tid; r < R; r += kThreads) {
        const double v = (f < n) ? exp_rows[(size_t)f * R + r] : scal[r].last_ll;
        if (T > 0) {
            const int members = R / T + ((r % T) < (R % T) ? 1 : 0);
            s = s + v / (double)members;
        } else s = s + v;
    }
    s = wave_sum_xor(s);
    if ((tid & 63) == 0) lds[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[f < n ? f : slot_ll] = (((lds[0] + lds[1]) + lds[2]) + lds[3]) / (double)(T > 0 ? T : R);
}

// Normalisable weights of one filter for host-side functionals (arbitrary std::function h: pswarm_filter.h:44,87-89):
// w_j = q_j exp(m_tile - m) 2^-41  (= exp(logw_j - max logw) to 2^-41).  grid (B), block 256.
__global__ __launch_bounds__(kThreads) void k_weights(const double* cdf, const double* tmax, int N, int B, int tile, double* w) {
    __shared__ double lds_m[16];
    const int tid = threadIdx.x, b = blockIdx.x;
    double mx = -dinf();
    bool nan = false;
    for (int j = tid; j < B; j += kThreads) { const double v = tmax[j]; nan = nan || (v != v); mx = (v > mx) ? v : mx; }
    const double m = block_max_nanprop<kThreads>(mx, nan, lds_m);
    const double sc = (m != m) ? dnan() : dexp_scaled(tmax[b] - m, -kTileShift);
    const double* cr = cdf + (size_t)b * tile;
    for (int j = tid; j < tile; j += kThreads)
        if (b * tile + j < N) w[(size_t)b * tile + j] = (cr[j] - (j ? cr[j - 1] : 0.0)) * sc;
}

}  // namespace ssme
