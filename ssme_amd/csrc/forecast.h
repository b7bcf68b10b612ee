// forecast.h -- simulation of future observations from the filtered particle cloud, gfx950.
//
// Reference counterpart: sim_future_obs(num_future_steps) of the filters' *FutureSimulator add-ons, called on every member
// by Swarm::simFutureObs / SwarmWithCovs::simFutureObs (include/ssme/pswarm_filter.h:247-253, 547-553); the in-tree
// simulation is the Liu-West one (include/ssme/liu_west_filter.h:1315-1363): start from the unweighted (resampled) samples,
// then per future step propagate the state and draw an observation from it.
//
// Two kernels per call (bootstrap models; the Liu-West pair below adds the parameter records and their moments), both on buffers of
// the forecast's own (nothing a later filter step reads is written):
//   k_fc_start_vec<DX>  draws N ancestors per filter from the last step's weights -- an iid two-level search of the integer
//                  weight cdf, the search of k_filter_step's general path, on the level-2 tables k_level2_plan leaves
//                  (T'_b, A_b / A'_b, S') -- and gathers their states, one gather per state plane (DX = 1: the built-in models).
//                  grid = (tiles, R).
//   k_fc_horizon   all H horizons in ONE launch: two particles per lane, state / y_prev / model constants in registers across
//                  the run-time loop over the horizon, one Philox call per particle and horizon (words 0-1 -> the pair
//                  (z_state, z_obs) by pair_normals), one coalesced 16-byte store per lane and horizon into y[r][k][.]
//                  (and x[r][k][.] when asked).  Tables of log / sincos / exp in LDS, as in the step kernels.
// A user model that declares its observation draw (model_api.h: gsamp / gsamp_vec) runs the same pair on every state plane:
//   k_fc_start_vec<DX>, k_fc_horizon_user<M, DX, DY> (below the built-in kernels).
// What the three horizon kernels (k_fc_horizon, k_fc_horizon_user, k_fc_lw_horizon) share is in fc_load_tables, fc_lane and
// fc_store_row; what the two argument structs share is FcCommon.
#pragma once
#include "pf_kernels.h"
#include "lw_kernels.h"

namespace ssme {

// Counter streams of the forecast.  A counter is (particle, t0, filter id, stream + (k << 8)) with t0 = the origin (steps done
// so far) and k = the horizon (0 for the start draw).  The filters' streams are all below 144 (ssme_math.h, lw_kernels.h,
// model_api.h) and carry nothing above bit 7, so no forecast counter equals a filter counter; k < 2^16 keeps k << 8 inside the word.
// STREAM_FC_SIM2: the second call of a user model with more than two state or observation components (k_fc_horizon_user).
enum { STREAM_FC_START = 160, STREAM_FC_SIM = 161, STREAM_FC_LW_JIT = 162, STREAM_FC_LW_SIM = 163, STREAM_FC_SIM2 = 164 };
constexpr int kFcMaxSteps = 65535;
constexpr int kFcNT = 256;

// what the bootstrap and the Liu-West forecast both pass to their kernels
struct FcCommon {
    const double* x;           // [R][Npad] particles of the last step (pre-resampling); user models: [DX][R][Npad], as x0
    const double* cdf;         // [R][Npad] tile-local inclusive integer sums of their fixed-point weights (Liu-West: second stage)
    const double* l2_T;        // [R][Bs] inclusive prefixes T'_b of the rescaled tile sums   (k_level2_plan, forecast's own buffers)
    const double* l2_R;        // [R][Bs] A_b / A'_b
    const FilterScalars* scal; // [R] S' (forecast's own copy)
    const double* last_obs;    // [R] y_prev of the first horizon, or null (0)
    double* x0;                // [R][Npad] states of the start population
    uint32_t* start;           // [R][Npad] its ancestors
    double* y_out;             // [R][H][Ns]; user models: [R][H][DY][Ns]
    double* x_out;             // [R][H][Ns] or null; user models: [R][H][DX][Ns]
    const uint32_t* keyp;      // [2] Philox key
    uint32_t first_filter;
    int32_t N, Npad, Ns, B, Bs, Bpow2, t0, H;
};

struct FcArgs : FcCommon {
    const ModelConst* mc;      // [R]
    const double* gscale;      // [R] scale of the observation draw: beta (SVOL), 1 (leverage), tau (linear Gaussian)
    const double* z_future;    // [H][dim_cov] exogenous covariates of the horizons (user models with dim_cov), or null
    int32_t tile;
};

// The start draw of particle i: u = u01_mid40 of words 0-1 of Philox(i, t0, filter id, STREAM_FC_START), target = ceil(u S'),
// ancestor = the filters' general search of that target (probe_ancestor, pf_kernels.h).
// Shared by the bootstrap and the Liu-West start kernels.
__device__ __forceinline__ int fc_draw_ancestor(const double* T, const double* Rr, const double* cdf_r, double S, int B, int Bpow2,
                                                int tile, int N, int i, uint32_t t0, uint32_t rep, uint32_t key0, uint32_t key1) {
    const u32x4 o = philox4x32_10((uint32_t)i, t0, rep, STREAM_FC_START, key0, key1);
    const double target = __builtin_ceil(u01_mid40(o.v0, o.v1) * S);
    return probe_ancestor(target, [&](int j) { return j < B ? T[j] : dinf(); }, [&](int j) { return Rr[j]; }, cdf_r, B, Bpow2, tile, 0, N);
}

// ---------------------------------------------------------------------------------------
// Start population of the bootstrap models: every particle's ancestor by fc_draw_ancestor and its state, one gather per state plane
// at the ancestor's index: x and x0 are [DX][R][Npad] (xplane = R Npad doubles per plane), as the filter's own particles.  The
// built-in models and scalar user models are DX = 1.  A filter without weight (S' not > 0: all weights zero, -inf or NaN) gets NaN
// states.  grid = (B, R), block = kFcNT.
// ---------------------------------------------------------------------------------------
template <int DX>
__global__ __launch_bounds__(kFcNT) void k_fc_start_vec(const FcArgs a, const size_t xplane) {
    const int r = blockIdx.y, b = blockIdx.x;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const uint32_t key0 = a.keyp[0], key1 = a.keyp[1];
    const size_t rowoff = (size_t)r * a.Npad;
    const double* T = a.l2_T + (size_t)r * a.Bs;
    const double* Rr = a.l2_R + (size_t)r * a.Bs;
    const double* cdf_r = a.cdf + rowoff;
    const double S = a.scal[r].S;
    const bool alive = S > 0.0;
    for (int j0 = threadIdx.x; j0 < a.tile; j0 += kFcNT) {
        const int i = b * a.tile + j0;                       // < Npad
        uint32_t anc = 0u;
        double xv[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) xv[d] = 0.0;
        if (i < a.N) {
            const int an = fc_draw_ancestor(T, Rr, cdf_r, S, a.B, a.Bpow2, a.tile, a.N, i, (uint32_t)a.t0, rep, key0, key1);
            anc = (uint32_t)an;
#pragma unroll
            for (int d = 0; d < DX; ++d) xv[d] = alive ? a.x[(size_t)d * xplane + rowoff + an] : dnan();
        }
        a.start[rowoff + i] = anc;
#pragma unroll
        for (int d = 0; d < DX; ++d) a.x0[(size_t)d * xplane + rowoff + i] = xv[d];
    }
}

// observation draw gSamp(x, z): SVOL beta exp(x/2) z, leverage exp(x/2) z (test/test_pswarm.cpp:112-116), linear Gaussian x + tau z
template <int MODEL>
__device__ __forceinline__ double model_gsamp(double gs, double x, double z, const ExpTabEntry* etab) {
    if (MODEL == MODEL_LIN_GAUSS) return x + gs * z;
    const double e = dexp_scaled_t(0.5 * x, 0, etab);
    if (MODEL == MODEL_SVOL) return (gs * e) * z;
    return e * z;
}

// ---------------------------------------------------------------------------------------
// What the three horizon kernels share.  fc_load_tables: the draw and exp tables into LDS, then the barrier.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void fc_load_tables(DrawTabs* dtab, ExpTabEntry* etab) {
    load_log_table<kFcNT>(dtab);
    load_exp_table<kFcNT>(etab);
    __syncthreads();
}

// A lane's share of a horizon kernel: particles i0 and i0 + 1 of filter r (Philox filter id rep), the key, whether the filter has
// weight, y_prev of the first horizon, the doubles per output plane and where the lane's first double2 of y / x (null: not asked
// for) goes; a horizon is ny / nx planes of y / x.  False: the lane is past the row and has nothing to do.
struct FcLane {
    int r, i0;
    uint32_t rep, key0, key1;
    bool alive;
    double y0;
    size_t plane;
    double *yrow, *xrow;
};
__device__ __forceinline__ bool fc_lane(const FcCommon& a, int ny, int nx, FcLane* l) {
    l->r = blockIdx.y;
    l->i0 = ((int)blockIdx.x * kFcNT + (int)threadIdx.x) * 2;
    if (l->i0 >= a.Ns) return false;
    l->rep = a.first_filter + (uint32_t)l->r;
    l->key0 = a.keyp[0]; l->key1 = a.keyp[1];
    l->alive = a.scal[l->r].S > 0.0;
    l->y0 = a.last_obs ? a.last_obs[l->r] : 0.0;
    l->plane = (size_t)a.Ns;
    l->yrow = a.y_out + (size_t)l->r * a.H * ny * l->plane + l->i0;
    l->xrow = a.x_out ? a.x_out + (size_t)l->r * a.H * nx * l->plane + l->i0 : nullptr;
    return true;
}

// one horizon's D planes of a lane's pair: an aligned double2 per plane, then the row moves on to the next horizon
template <int D>
__device__ __forceinline__ void fc_store_row(double*& row, size_t plane, const double (*v)[2]) {
#pragma unroll
    for (int j = 0; j < D; ++j) *reinterpret_cast<double2*>(row + (size_t)j * plane) = make_double2(v[j][0], v[j][1]);
    row += (size_t)D * plane;
}

// ---------------------------------------------------------------------------------------
// All H horizons of lane pairs (2p, 2p + 1).  Per horizon k and particle i: (z_s, z_o) = pair_normals of words 0-1 of
// Philox(i, t0, filter id, STREAM_FC_SIM + (k << 8)); x <- model_prop(x, z_s, y_prev); y <- gSamp(x, z_o); y_prev <- y
// (propagate, then observe: liu_west_filter.h:1338-1356).  Rows of the outputs are Ns = N rounded up to even doubles long, so
// every store is an aligned double2; the pad column of an odd N is computed from a zero state and never copied out.
// grid = (ceil(Ns / 2 / kFcNT), R), block = kFcNT.
// ---------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kFcNT) void k_fc_horizon(const FcArgs a) {
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    fc_load_tables(&lds_dtab, lds_etab);
    FcLane l;
    if (!fc_lane(a, 1, 1, &l)) return;
    const ModelConst mc = a.mc[l.r];
    const double gs = a.gscale[l.r];
    const double2 xs = *reinterpret_cast<const double2*>(a.x0 + (size_t)l.r * a.Npad + l.i0);
    double x[2] = {xs.x, xs.y};
    double yp[2] = {l.y0, l.y0};
    for (int k = 0; k < a.H; ++k) {
        const uint32_t c3 = (uint32_t)STREAM_FC_SIM + ((uint32_t)k << 8);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const u32x4 o = philox4x32_10((uint32_t)(l.i0 + c), (uint32_t)a.t0, l.rep, c3, l.key0, l.key1);
            double zs, zo;
            pair_normals(o.v0, o.v1, &lds_dtab, &zs, &zo);
            x[c] = model_prop<MODEL>(mc, x[c], zs, yp[c], lds_etab);
            const double yv = model_gsamp<MODEL>(gs, x[c], zo, lds_etab);
            yp[c] = l.alive ? yv : dnan();
        }
        fc_store_row<1>(l.yrow, l.plane, &yp);
        if (l.xrow) fc_store_row<1>(l.xrow, l.plane, &x);
    }
}

// ---------------------------------------------------------------------------------------
// All H horizons of lane pairs (2p, 2p + 1) of a user model.  Per horizon k and particle i, call c in {0, 1} is
// Philox(i, t0, filter id, S_c + (k << 8)) with S_0 = STREAM_FC_SIM, S_1 = STREAM_FC_SIM2; words 0-1 of call c give
// (zs[2c], zo[2c]) and words 2-3 (zs[2c + 1], zo[2c + 1]) by pair_normals.  Only what max(DX, DY) components need is evaluated;
// members past DX (state) or DY (observation) are dropped, so a scalar model consumes what k_fc_horizon does.
//   x <- prop_vec(x, zs, y_prev[0]);  y <- gsamp_vec(x, zo);  y_prev <- y.
// A dim_cov model instead takes the K exogenous covariates of horizon k, z_future[k K + j] (uniform loads), into both calls:
//   x <- prop_vec(x, zs, z_k);  y <- gsamp_vec(x, zo, z_k);  y_prev is not read.
// Outputs: y[(r H + k) DY + j][Ns], x[(r H + k) DX + d][Ns], rows of Ns = N rounded up to even doubles, one aligned double2 store
// per lane, component and horizon; the pad column of an odd N is computed from a zero state and never copied out.  State, y_prev,
// the model constants and the key stay in registers across the run-time loop (constant indices only: nothing in scratch).
// grid = (ceil(Ns / 2 / kFcNT), R), block = kFcNT.
// ---------------------------------------------------------------------------------------
template <class M, int DX, int DY>
__global__ __launch_bounds__(kFcNT) void k_fc_horizon_user(const FcArgs a, const size_t xplane) {
    constexpr int DM = DX > DY ? DX : DY, KC = user_cov<M>::k;
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    fc_load_tables(&lds_dtab, lds_etab);
    FcLane l;
    if (!fc_lane(a, DY, DX, &l)) return;
    const ModelConst mc = a.mc[l.r];
    double x[DX][2];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        const double2 xs = *reinterpret_cast<const double2*>(a.x0 + (size_t)d * xplane + (size_t)l.r * a.Npad + l.i0);
        x[d][0] = xs.x; x[d][1] = xs.y;
    }
    double yp[2] = {l.y0, l.y0};                                   // component 0 of the previous observation
    for (int k = 0; k < a.H; ++k) {
        const uint32_t kk = (uint32_t)k << 8;
        double y[DY][2];
        CovVals<KC> zc;
        if constexpr (KC > 0) zc.load(a.z_future, (size_t)k);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double zs[4], zo[4];
            {
                const u32x4 o = philox4x32_10((uint32_t)(l.i0 + c), (uint32_t)a.t0, l.rep, (uint32_t)STREAM_FC_SIM + kk, l.key0, l.key1);
                pair_normals(o.v0, o.v1, &lds_dtab, &zs[0], &zo[0]);
                if constexpr (DM > 1) pair_normals(o.v2, o.v3, &lds_dtab, &zs[1], &zo[1]);
            }
            if constexpr (DM > 2) {
                const u32x4 o = philox4x32_10((uint32_t)(l.i0 + c), (uint32_t)a.t0, l.rep, (uint32_t)STREAM_FC_SIM2 + kk, l.key0, l.key1);
                pair_normals(o.v0, o.v1, &lds_dtab, &zs[2], &zo[2]);
                if constexpr (DM > 3) pair_normals(o.v2, o.v3, &lds_dtab, &zs[3], &zo[3]);
            }
            double xi[DX], xn[DX], yv[DY];
#pragma unroll
            for (int d = 0; d < DX; ++d) xi[d] = x[d][c];
            if constexpr (KC > 0) {
                user_calls<M>::prop_vec(mc, xi, zs, zc.v, xn, lds_etab);
                user_calls<M>::gsamp_vec(mc, xn, zo, zc.v, yv, lds_etab);
            } else {
                user_calls<M>::prop_vec(mc, xi, zs, yp[c], xn, lds_etab);
                user_calls<M>::gsamp_vec(mc, xn, zo, yv, lds_etab);
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) x[d][c] = xn[d];
#pragma unroll
            for (int j = 0; j < DY; ++j) y[j][c] = l.alive ? yv[j] : dnan();
            yp[c] = y[0][c];
        }
        fc_store_row<DY>(l.yrow, l.plane, y);
        if (l.xrow) fc_store_row<DX>(l.xrow, l.plane, x);
    }
}

// =======================================================================================
// Liu-West, both forms (liu_west_filter.h:1315-1363): the start population carries its parameters; theta-bar and the Cholesky
// factor L of (1 - a^2) V are taken ONCE over the transformed parameters of the start population (the reference recomputes them
// every horizon from the unchanged m_param_particles, so they are constant), by the filter's own moment tree (k_lw_stage1's tile
// partials, k_lw_mom_totals, lw_proposal_components).  Per horizon, in k_lw_stage2's operation order:
//   m = a theta + (1 - a) theta-bar;  theta <- m + L e;  tu = tr_inv(theta);
//   x <- mean(x, y_prev, tu) + z_s tu[2] sqrt(1 - tu[3]^2);  y <- z_o exp(x / 2);  y_prev <- y
// e: four normals of one Philox call (STREAM_FC_LW_JIT), (z_s, z_o): words 0-1 of a second one (STREAM_FC_LW_SIM).
// =======================================================================================
struct FcLwArgs : FcCommon {      // x, x0: [R][Npad]; cdf: of the second-stage weights; last_obs is never null
    const double* th;          // [R][Npad][4] transformed parameters of the particles of the last step
    double* th0;               // [R][Npad][4] those of the start population
    double* mom;               // [R][B][16] tile partials of the 14 moments
    const double* prop;        // [R][16] theta-bar[4], L[10]
    double a_shrink;
    int32_t trans[kDP];
};

// grid = (B, R), block = kLwNT, 2048-particle tiles: thread tid holds particles i_first + (k 512 + tid) 2 + c, as k_lw_stage1 does,
// so that the moment partials run through the same additions
__global__ __launch_bounds__(kLwNT) void k_fc_lw_start(const FcLwArgs a) {
    constexpr int NT = kLwNT, NK = 2;
    __shared__ double lds_mom[8][4][16];
    const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.x;
    const uint32_t rep = a.first_filter + (uint32_t)r;
    const uint32_t key0 = a.keyp[0], key1 = a.keyp[1];
    const size_t rowoff = (size_t)r * a.Npad;
    const double* T = a.l2_T + (size_t)r * a.Bs;
    const double* Rr = a.l2_R + (size_t)r * a.Bs;
    const double* cdf_r = a.cdf + rowoff;
    const double S = a.scal[r].S;
    const bool alive = S > 0.0;
    const int i_first = b * kTile;
    double fold[kNMom][2];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int i0 = i_first + (k * NT + tid) * 2;
        double xo[2], tt[kDP][2];
        uint32_t an[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int i = i0 + c;
            const bool valid = i < a.N;
            int anc = 0;
            if (valid) anc = fc_draw_ancestor(T, Rr, cdf_r, S, a.B, a.Bpow2, kTile, a.N, i, (uint32_t)a.t0, rep, key0, key1);
            an[c] = (uint32_t)anc;
            double trec[kDP];
            th_load(a.th, rowoff + (size_t)anc, trec);
            xo[c] = valid ? (alive ? a.x[rowoff + anc] : dnan()) : 0.0;
            int q = 0;
#pragma unroll
            for (int d = 0; d < kDP; ++d) { tt[d][c] = valid ? trec[d] : 0.0; const double v = tt[d][c]; fold[q][c] = (k == 0) ? v : fold[q][c] + v; ++q; }
#pragma unroll
            for (int d = 0; d < kDP; ++d) {
#pragma unroll
                for (int e = 0; e <= d; ++e) { const double v = valid ? tt[d][c] * tt[e][c] : 0.0; fold[q][c] = (k == 0) ? v : fold[q][c] + v; ++q; }
            }
        }
        *reinterpret_cast<double2*>(a.x0 + rowoff + i0) = make_double2(xo[0], xo[1]);
        *reinterpret_cast<uint2*>(a.start + rowoff + i0) = make_uint2(an[0], an[1]);
        th_store_pair(a.th0, rowoff + (size_t)i0, tt);
    }
    {
        double v[16];
#pragma unroll
        for (int q = 0; q < kNMom; ++q) v[q] = fold[q][0] + fold[q][1];
        v[14] = 0.0; v[15] = 0.0;
        const double rowtot = lw_row_tree14(v, tid);
        lds_mom[tid >> 6][(tid >> 4) & 3][lw_row_tree_index(tid & 15)] = rowtot;
    }
    __syncthreads();
    if (tid < kNMom) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 8; ++w) s = s + ((lds_mom[w][3][tid] + lds_mom[w][2][tid]) + (lds_mom[w][1][tid] + lds_mom[w][0][tid]));
        a.mom[((size_t)r * a.B + b) * 16 + tid] = s;
    }
}

// theta-bar and L of every filter from its 14 moment totals.  grid = (R), block = 64 (one thread works)
__global__ __launch_bounds__(64) void k_fc_lw_prop(const double* momtot, int N, double a_shrink, double* prop) {
    if (threadIdx.x == 0) lw_proposal_components(momtot + (size_t)blockIdx.x * 16, N, a_shrink, prop + (size_t)blockIdx.x * 16);
}

// grid = (ceil(Ns / 2 / kFcNT), R), block = kFcNT; layout and stores as k_fc_horizon
__global__ __launch_bounds__(kFcNT) void k_fc_lw_horizon(const FcLwArgs a) {
    __shared__ __attribute__((aligned(16))) DrawTabs lds_dtab;
    __shared__ __attribute__((aligned(16))) ExpTabEntry lds_etab[SSME_EXP_TABLE_SIZE];
    fc_load_tables(&lds_dtab, lds_etab);
    FcLane l;
    if (!fc_lane(a, 1, 1, &l)) return;
    double prop[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) prop[q] = a.prop[(size_t)l.r * 16 + q];     // uniform: scalar loads
    const size_t rowoff = (size_t)l.r * a.Npad;
    const double2 xs = *reinterpret_cast<const double2*>(a.x0 + rowoff + l.i0);
    double x[2] = {xs.x, xs.y};
    double th[kDP][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        double trec[kDP];
        th_load(a.th0, rowoff + (size_t)(l.i0 + c), trec);
#pragma unroll
        for (int d = 0; d < kDP; ++d) th[d][c] = trec[d];
    }
    double yp[2] = {l.y0, l.y0};
    const double om = 1.0 - a.a_shrink;
    for (int k = 0; k < a.H; ++k) {
        const uint32_t kk = (uint32_t)k << 8;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double e[kDP];
            const u32x4 o1 = philox4x32_10((uint32_t)(l.i0 + c), (uint32_t)a.t0, l.rep, (uint32_t)STREAM_FC_LW_JIT + kk, l.key0, l.key1);
            pair_normals(o1.v0, o1.v1, &lds_dtab, &e[0], &e[1]);
            pair_normals(o1.v2, o1.v3, &lds_dtab, &e[2], &e[3]);
            double tu[kDP];
            int q = kDP;
#pragma unroll
            for (int d = 0; d < kDP; ++d) {
                const double mm = a.a_shrink * th[d][c] + om * prop[d];
                double acc = 0.0;
#pragma unroll
                for (int w = 0; w <= d; ++w) { acc = acc + prop[q] * e[w]; ++q; }
                th[d][c] = mm + acc;
                tu[d] = tr_inv(a.trans[d], th[d][c], lds_etab);
            }
            const u32x4 o2 = philox4x32_10((uint32_t)(l.i0 + c), (uint32_t)a.t0, l.rep, (uint32_t)STREAM_FC_LW_SIM + kk, l.key0, l.key1);
            double zs, zo;
            pair_normals(o2.v0, o2.v1, &lds_dtab, &zs, &zo);
            const double xk = x[c];
            const double mean = (tu[1] + tu[0] * (xk - tu[1])) + ((yp[c] * tu[3]) * tu[2]) * dexp_scaled_t(-0.5 * xk, 0, lds_etab);
            x[c] = mean + zs * (tu[2] * dsqrt(1.0 - tu[3] * tu[3]));
            const double yv = zo * dexp_scaled_t(0.5 * x[c], 0, lds_etab);
            yp[c] = l.alive ? yv : dnan();
        }
        fc_store_row<1>(l.yrow, l.plane, &yp);
        if (l.xrow) fc_store_row<1>(l.xrow, l.plane, &x);
    }
}

}  // namespace ssme
