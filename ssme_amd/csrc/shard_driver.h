// shard_driver.h -- RCCL transport of the C++ host drivers of the particle-sharded filters (included by pf_api.hip:
// ssme_pf_shard_run_series, the bootstrap filter; ssme_lw_shard_run_series, the Liu-West filter).
//
// SURVEY.md section 8e row 2 / BASELINE.json north star: "C++ host code owns ... and calls HIP kernels through a thin
// extern-"C" ABI ... one RCCL [collective] over xGMI per time step for the global log-weight sum and an all-to-all for
// particle redistribution".  One process per GPU; rank g owns B/world consecutive 2048-particle tiles.  Per time step of
// the bootstrap driver, everything on ONE HIP stream and -- on the fast path -- without any host synchronisation:
//     two grouped ncclAllGather (tile sums, tile maxima: 16 bytes per tile), each straight into its final array (all_gather)
//     k_shard_plan (or k_level2_plan + k_shard_window_check above 1024 tiles): every rank's source-tile window [lo, hi] and
//         a device flag if a window leaves the fixed halo
//     grouped ncclSend / ncclRecv of the halo tiles (integer cdf + particles) with the two neighbouring ranks (halo_exchange)
//     k_filter_step on the rank's tiles, reading its window in place from the halo buffer
// A rank's flag says what ITS OWN workgroups saw (up to 1024 tiles no plan kernel runs, so nothing else knows), and the
// decision to run again must be the same on every rank -- otherwise one rank re-enters the collectives alone.  After the
// time loop the flags are therefore reduced over the ranks (one ncclAllReduce(max) of one int, still on the stream:
// reduce_flags), and the reduced flag is what the host reads: if a window ever left the halo on ANY rank (very unbalanced
// weights), EVERY rank runs the series again on the exact path (the plan is downloaded every step and exactly the planned
// tiles travel, any rank to any rank: planned_exchange).
// Results are bit-identical to the unsharded filter on both paths (RNG counters are global particle indices, the level-2
// is the same exact integer arithmetic on the gathered tile sums).
//
// RCCL is resolved at run time from what the process already has loaded (torch's librccl in the Python tests and
// bench.py; `librccl.so` from the loader path otherwise): the library itself does not link against it.
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and enums only

#include <initializer_list>

#include "handle_core.h"

namespace ssme {

struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};

static void* rccl_sym(void*& lib, const char* name) {
    void* p = dlsym(RTLD_DEFAULT, name);                  // the RCCL this process already uses, if any
    if (p) return p;
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    return lib ? dlsym(lib, name) : nullptr;
}
static const RcclApi& rccl() {
    static const RcclApi api = [] {
        RcclApi a;
        void* lib = nullptr;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(rccl_sym(lib, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(rccl_sym(lib, "ncclCommInitRank"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(rccl_sym(lib, "ncclCommDestroy"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(rccl_sym(lib, "ncclAllGather"));
        a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(rccl_sym(lib, "ncclAllReduce"));
        a.Send = reinterpret_cast<decltype(a.Send)>(rccl_sym(lib, "ncclSend"));
        a.Recv = reinterpret_cast<decltype(a.Recv)>(rccl_sym(lib, "ncclRecv"));
        a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(rccl_sym(lib, "ncclGroupStart"));
        a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(rccl_sym(lib, "ncclGroupEnd"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(rccl_sym(lib, "ncclGetErrorString"));
        a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.AllReduce && a.Send && a.Recv && a.GroupStart && a.GroupEnd;
        return a;
    }();
    return api;
}

#define NCCLCHK(call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) { \
    if (h) h->err = std::string(#call) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r_) : "RCCL error"); return SSME_ERR_HIP; } } while (0)

// ---- the transport of both drivers: collectives and copies on the handle's stream ---------------------------------------

// what a native series starts with (the driver has allocated its buffers): RCCL present, the caller's communicator, the flags and
// the count of received tiles cleared
static int native_begin(HandleCore* h, void* nccl_comm, ncclComm_t* comm) {
    if (!rccl().ok) { h->err = "RCCL (librccl.so) not found in this process"; return SSME_ERR_UNSUPPORTED; }
    *comm = reinterpret_cast<ncclComm_t>(nccl_comm);
    HIPCHK(hipMemsetAsync(h->sh_flag, 0, sizeof(int32_t) * 4, h->stream));
    h->sh_exchanged = 0;
    return SSME_OK;
}

// halo margin in tiles: a rank's resampling window normally reaches a tile or two into its neighbours (the cumulative tile
// weights wander like sqrt(tiles) around the uniform split); 4 tiles or 1/64 of the share, never more than the share
static int halo_margin(int Bl, int world) {
    if (world == 1) return 0;
    const int m = Bl / 64 > 4 ? Bl / 64 : 4;
    return m > Bl ? Bl : m;
}

// entries of a gathered per-tile array: world x Bl (rank g's at g Bl), the first B are tiles; at least Bs (level-2 kernels)
static size_t gathered_len(const HandleCore* h) {
    return (size_t)h->shard_world * h->sh_Bl > (size_t)h->Bs ? (size_t)h->shard_world * h->sh_Bl : (size_t)h->Bs;
}

// one grouped all-gather: every rank's `count` doubles at src, in rank order into dst
struct GatherPart { const double* src; double* dst; size_t count; };
static int all_gather(HandleCore* h, ncclComm_t comm, std::initializer_list<GatherPart> parts) {
    NCCLCHK(rccl().GroupStart());
    for (const GatherPart& p : parts) NCCLCHK(rccl().AllGather(p.src, p.dst, p.count, ncclDouble, comm, h->stream));
    NCCLCHK(rccl().GroupEnd());
    return SSME_OK;
}

// fixed halo of buffers [margin | Bl own | margin] x `width` doubles per tile: my first m own rows are the left neighbour's right
// margin, my last m own rows the right neighbour's left margin
struct HaloBuf { double* rows; size_t width; };
static int halo_exchange(HandleCore* h, ncclComm_t comm, std::initializer_list<HaloBuf> bufs) {
    const int world = h->shard_world, rank = h->shard_rank, Bl = h->sh_Bl, m = h->sh_margin;
    if (world == 1 || m == 0) return SSME_OK;
    NCCLCHK(rccl().GroupStart());
    for (const HaloBuf& b : bufs) {
        const size_t w = b.width;
        if (rank > 0) {
            NCCLCHK(rccl().Send(b.rows + (size_t)m * w, (size_t)m * w, ncclDouble, rank - 1, comm, h->stream));
            NCCLCHK(rccl().Recv(b.rows, (size_t)m * w, ncclDouble, rank - 1, comm, h->stream));
        }
        if (rank + 1 < world) {
            NCCLCHK(rccl().Send(b.rows + (size_t)Bl * w, (size_t)m * w, ncclDouble, rank + 1, comm, h->stream));
            NCCLCHK(rccl().Recv(b.rows + (size_t)(m + Bl) * w, (size_t)m * w, ncclDouble, rank + 1, comm, h->stream));
        }
    }
    NCCLCHK(rccl().GroupEnd());
    h->sh_exchanged += (long)m * ((rank > 0) + (rank + 1 < world));
    return SSME_OK;
}

// exact path: every rank's planned window (lo_hi: [world][2] global tiles) travels from the ranks that own it, any rank to any
// rank, into `win` (global tiles lo .. hi); `own`: this rank's Bl tiles.  The received tiles of the first buffer are counted.
struct WindowBuf { const double* own; double* win; size_t width; };
static int planned_exchange(HandleCore* h, ncclComm_t comm, const int32_t* lo_hi, std::initializer_list<WindowBuf> bufs) {
    const int world = h->shard_world, rank = h->shard_rank, Bl = h->sh_Bl, tile0 = rank * Bl;
    const int lo = lo_hi[2 * rank], hi = lo_hi[2 * rank + 1];
    NCCLCHK(rccl().GroupStart());
    for (const WindowBuf& b : bufs) {
        const size_t w = b.width;
        for (int p = 0; p < world; ++p) {
            // what I need from rank p: [lo, hi] x p's tiles
            const int a1 = lo > p * Bl ? lo : p * Bl, b1 = hi < (p + 1) * Bl - 1 ? hi : (p + 1) * Bl - 1;
            if (b1 >= a1) {
                if (p == rank) HIPCHK(hipMemcpyAsync(b.win + (size_t)(a1 - lo) * w, b.own + (size_t)(a1 - tile0) * w, sizeof(double) * (size_t)(b1 - a1 + 1) * w,
                                                     hipMemcpyDeviceToDevice, h->stream));
                else {
                    NCCLCHK(rccl().Recv(b.win + (size_t)(a1 - lo) * w, (size_t)(b1 - a1 + 1) * w, ncclDouble, p, comm, h->stream));
                    if (&b == bufs.begin()) h->sh_exchanged += b1 - a1 + 1;
                }
            }
            // what rank p needs from me: [lo_p, hi_p] x my tiles
            if (p != rank) {
                const int lp = lo_hi[2 * p], hp = lo_hi[2 * p + 1];
                const int a2 = lp > tile0 ? lp : tile0, b2 = hp < tile0 + Bl - 1 ? hp : tile0 + Bl - 1;
                if (b2 >= a2) NCCLCHK(rccl().Send(b.own + (size_t)(a2 - tile0) * w, (size_t)(b2 - a2 + 1) * w, ncclDouble, p, comm, h->stream));
            }
        }
    }
    NCCLCHK(rccl().GroupEnd());
    return SSME_OK;
}

// end of a fixed-halo series: the fallback decision must be the SAME on every rank, so every rank's flag [0] is reduced (max)
// into [3] before anyone reads it; then sh_stats = the flags and *overflow = the reduced one.  One int, once per series; synchronises.
static int reduce_flags(HandleCore* h, ncclComm_t comm, bool* overflow) {
    NCCLCHK(rccl().AllReduce(h->sh_flag, h->sh_flag + 3, 1, ncclInt32, ncclMax, comm, h->stream));
    HIPCHK(hipMemcpyAsync(h->sh_stats, h->sh_flag, sizeof(h->sh_stats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *overflow = h->sh_stats[3] != 0;
    return SSME_OK;
}

// Does every rank's window [lo, hi] stay inside [first own tile - margin, last own tile + margin]?  lo_hi: [world][2]
// (k_shard_plan), or null: the per-tile ranges of k_level2_plan (window = [lo of the rank's first tile, hi of its last]).
__global__ void k_shard_window_check(const int32_t* lo_hi, const int32_t* l2_lo, const int32_t* l2_hi, int world, int Bl, int B, int margin,
                                     int32_t* flag, int32_t* stats /*[2]: max tiles needed left / right of the own range*/) {
    const int g = threadIdx.x;
    if (g >= world) return;
    const int last = (g + 1) * Bl - 1 < B - 1 ? (g + 1) * Bl - 1 : B - 1;       // the last rank may own fewer than Bl tiles
    const int lo = lo_hi ? lo_hi[2 * g] : l2_lo[(size_t)g * Bl];
    const int hi = lo_hi ? lo_hi[2 * g + 1] : l2_hi[last];
    const int left = g * Bl - lo, right = hi - last;
    if (left > margin || right > margin) atomicOr(flag, 1);
    if (left > 0) atomicMax(&stats[0], left);
    if (right > 0) atomicMax(&stats[1], right);
}

}  // namespace ssme
