// What the stages that write one byte stream in message order share (ngz_flow_json.hip, ngz_wire.hip;
// included by those units only).  The whole output of such a stage is one stream in stream order; every
// byte belongs to a record or to glue (datagram head, set framing, datagram tail), and the unit of work is
// a tile: at most 64 consecutive records of one data set, which are consecutive rows of one slot's columns
// and consecutive bytes of the output.  Here are the tables of that bookkeeping (Layout), the passes that
// build them, and the host scaffold of the stage handle.  A stage states what is its own in a traits struct
// S of __device__ static functions over its args type S::Args (a Layout, its plan beside it; its slots
// carry n_rows):
//   sets_how(slot, how)       the `how` the set pass stores for a datagram with a set of this slot, below 0: none,
//   fill_tile(A, slot, n, t, first)  the fill pass's store of tile t's bytes, where they need no pass over rows
//                             (the tile: records from `first` of a set of n in this slot),
//   set_len(A, si, tiles)     a set's bytes: its framing around the sum of its tiles',
//   dgram_frame(A, h, n_sets) a datagram's bytes but for its sets': head, what stands between n_sets sets, tail,
//   counter(A, d, how)        which of the four stats counts datagram d (0..3); the last word on how[d].
// Header only.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_json.h"
#include "ngz/flow_wire.h"
#include "ngz_agg_rows.h"
#include "ngz_host.h"
#include "ngz_stage.h"

namespace ngzms {

constexpr uint32_t THREADS = 256;
constexpr uint32_t TILE = 64;
constexpr uint32_t ERR_SETS = 1, ERR_VLEN = 2, ERR_TILES = 4;
// counters: the error bits, then the stage's four stats in the order of its stats struct (bytes apart)
constexpr uint32_t C_ERR = 0, C_COUNT = 5;
// how[d]: both public headers number these alike; a stage's further values lie above them
enum : uint8_t { HOW_NONE = 0, HOW_WRITTEN = 1, HOW_HOST = 2 };
static_assert(NGZ_FLOW_JSON_NONE == HOW_NONE && NGZ_FLOW_JSON_LINE == HOW_WRITTEN && NGZ_FLOW_JSON_HOST == HOW_HOST, "");
static_assert(NGZ_WIRE_NONE == HOW_NONE && NGZ_WIRE_WIRE == HOW_WRITTEN && NGZ_WIRE_HOST == HOW_HOST, "");

struct Tile {
    uint32_t set, first;  // records [first, first + 64) of the set, as far as it has them
};
struct Layout {  // a stage's args derive from it and are passed by value
    const uint32_t *host_dgrams;  // the datagrams with (options) template sets, ascending
    const ngz_set_info *sets;
    const ngz_dgram_hdr *hdr;
    const uint8_t *in;  // the batch input
    unsigned long long in_size;
    uint32_t n_host, n_sets, n_dgrams, n_slots, tile_cap;
    uint8_t *how;
    uint32_t *dset0, *dset1;   // per datagram: its sets [dset0, dset1)
    uint32_t *ntiles, *tile0;  // per set, and one more: tile0[n_sets] is the number of tiles
    Tile *tiles;
    uint32_t *tile_bytes;
    unsigned long long *tile_off, *set_len, *set_off, *dlen, *offs;
    uint8_t *out;
    unsigned long long total;
    unsigned long long *counters;
};

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ld_cell(const uint8_t *p, uint32_t w) {  // p: aligned to w
    return w == 8 ? *(const uint64_t *)p : w == 4 ? *(const uint32_t *)p : w == 2 ? *(const uint16_t *)p : *p;
}

// A set inside the batch's tables
template <class Args>
__device__ __forceinline__ bool set_ok(const Args &A, const ngz_set_info &si) {
    return si.dgram < A.n_dgrams && si.slot < A.n_slots && (!si.n || (uint64_t)si.rec0 + si.n <= A.slots[si.slot].n_rows);
}

// Tile t: its set, the records it has of it, and the row of its first
struct TileRows {
    ngz_set_info si;
    uint32_t first, cnt, row0;
};
template <class Args>
__device__ __forceinline__ TileRows tile_rows(const Args &A, uint32_t t) {
    const Tile tl = A.tiles[t];
    const ngz_set_info si = A.sets[tl.set];
    return TileRows{si, tl.first, min(TILE, si.n - tl.first), si.rec0 + tl.first};
}

// Inclusive sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint32_t up = __shfl_up(v, k, 64);
        if (lane >= (uint32_t)k) v += up;
    }
    return v;
}

// One thread per datagram: written, not OK, or left to the host for its template sets
template <class S>
__global__ __launch_bounds__(THREADS) void k_dgrams(const typename S::Args A) {
    const uint32_t d = blockIdx.x * THREADS + threadIdx.x;
    if (d >= A.n_dgrams) return;
    uint8_t how = A.hdr[d].status == NGZ_DG_OK ? HOW_WRITTEN : HOW_NONE;
    uint32_t lo = 0, hi = A.n_host;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.host_dgrams[mid] < d) lo = mid + 1;
        else hi = mid;
    }
    if (how == HOW_WRITTEN && lo < A.n_host && A.host_dgrams[lo] == d) how = HOW_HOST;
    A.how[d] = how;
    A.dset0[d] = A.dset1[d] = 0;
}

// One thread per data set: its datagram's range of sets, and what its slot says about the datagram
template <class S>
__global__ __launch_bounds__(THREADS) void k_sets(const typename S::Args A) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const ngz_set_info si = A.sets[s];
    if (!set_ok(A, si)) {
        atomicOr((unsigned int *)&A.counters[C_ERR], ERR_SETS);
        return;
    }
    if (s == 0 || A.sets[s - 1].dgram != si.dgram) A.dset0[si.dgram] = s;  // the sets are in stream order
    if (s + 1 == A.n_sets || A.sets[s + 1].dgram != si.dgram) A.dset1[si.dgram] = s + 1;
    // several sets of a datagram may store the same value; k_dgrams ran before.  `how` goes by reference:
    // a stage that decides by the slot alone does not load it
    const int how = S::sets_how(A.slots[si.slot], A.how[si.dgram]);
    if (how >= 0) A.how[si.dgram] = (uint8_t)how;
}

// One thread per data set: its tiles, ceil(n / 64), if its datagram is written
template <class S>
__global__ __launch_bounds__(THREADS) void k_tiles(const typename S::Args A) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s > A.n_sets) return;
    uint32_t n = 0;
    if (s < A.n_sets) {
        const ngz_set_info si = A.sets[s];
        if (set_ok(A, si) && A.how[si.dgram] == HOW_WRITTEN) n = (si.n + TILE - 1) / TILE;
    }
    A.ntiles[s] = n;  // ntiles[n_sets] = 0: the scan's last item
}

// One thread per data set, after the scan of ntiles into tile0: the tile table (set, first record)
template <class S>
__global__ __launch_bounds__(THREADS) void k_fill(const typename S::Args A) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const uint32_t t0 = A.tile0[s], n = A.ntiles[s];
    if (!n) return;
    const ngz_set_info si = A.sets[s];
    const auto slot = A.slots[si.slot];  // a copy: what fill_tile reads of it is loaded once, before the stores
    for (uint32_t t = 0; t < n; ++t) {
        if (t0 + t >= A.tile_cap || t0 + t < t0) {
            atomicOr((unsigned int *)&A.counters[C_ERR], ERR_TILES);
            break;
        }
        A.tiles[t0 + t] = Tile{s, t * TILE};
        S::fill_tile(A, slot, si.n, t0 + t, t * TILE);
    }
}

// One thread per set: its framing and its tiles
template <class S>
__global__ __launch_bounds__(THREADS) void k_set_len(const typename S::Args A) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const ngz_set_info si = A.sets[s];
    unsigned long long len = 0;
    if (set_ok(A, si) && A.how[si.dgram] == HOW_WRITTEN) {
        const uint32_t t1 = min(A.tile0[s + 1], A.tile_cap);
        for (uint32_t t = A.tile0[s]; t < t1; ++t) len += A.tile_bytes[t];
        len = S::set_len(A, si, len);
    }
    A.set_len[s] = len;
}

// One thread per datagram: its head, sets and tail; the stats
template <class S>
__global__ __launch_bounds__(THREADS) void k_dgram_len(const typename S::Args A) {
    __shared__ unsigned long long acc[4];
    const uint32_t d = blockIdx.x * THREADS + threadIdx.x;
    uint64_t c[4] = {0, 0, 0, 0};
    if (d < A.n_dgrams) {
        unsigned long long len = 0;
        const uint8_t how = A.how[d];
        if (how == HOW_WRITTEN) {
            const uint32_t s0 = A.dset0[d], s1 = min(A.dset1[d], A.n_sets);
            len = S::dgram_frame(A, A.hdr[d], s1 > s0 ? s1 - s0 : 0u);
            for (uint32_t s = s0; s < s1; ++s) len += A.set_len[s];
        }
        c[S::counter(A, d, how)] = 1;
        A.dlen[d] = len;
        if (d == 0) A.dlen[A.n_dgrams] = 0;  // the scan's last item
    }
    unsigned long long *const dst[4] = {&A.counters[1], &A.counters[2], &A.counters[3], &A.counters[4]};
    ngzs::block_add<4>(acc, c, dst);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// What both stage handles are.  `what` names the stage in its out-of-memory errors.
struct MsgStage : ngzs::Stage {
    explicit MsgStage(const char *what_) : Stage(4), what(what_) {}
    const char *const what;
    float size_ms = 0, offsets_ms = 0, pack_ms = 0;
    int launches = 0;
    uint64_t n_dgrams = 0, n_bytes = 0;  // the last encode
    bool have = false;
    hipStream_t st = nullptr;                                // the encode under way: its stream,
    uint64_t in_bytes = 0;                                   // the bytes of d_in it uploads,
    size_t scan_a = 0, scan_b = 0;                           // and the temp bytes of its two scans
    ngzh::DevBuf<uint8_t> d_in, d_how, d_bytes, d_scan_tmp;  // d_in: the stage's plan, then the template datagrams
    ngzh::DevBuf<uint32_t> d_u32;                            // dset0, dset1, ntiles, tile0, tile_bytes
    ngzh::DevBuf<Tile> d_tiles;
    ngzh::DevBuf<unsigned long long> d_u64, d_offs, d_counters;  // d_u64: tile_off, set_len, set_off, dlen
    ngzs::PinnedBuf<uint8_t> h_in;
    ngzs::PinnedBuf<unsigned long long> h_back;  // the counters, the total, the tiles

    void release_device() {  // the destroy functions select the device first
        d_in.release();
        d_how.release();
        d_bytes.release();
        d_scan_tmp.release();
        d_u32.release();
        d_tiles.release();
        d_u64.release();
        d_offs.release();
        d_counters.release();
    }
    template <class K, class... Args>
    hipError_t launch(K kernel, uint32_t nb, uint32_t threads, Args... args) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(threads), 0, st, args...);
        ++launches;
        return hipGetLastError();
    }
};

inline uint32_t blocks(uint64_t items) { return (uint32_t)((items + THREADS - 1) / THREADS); }

inline int fail_vlen(MsgStage *o) { return ngzs::fail(o, NGZ_E_INVALID, "a variable-length cell outside the batch input"); }

// The opening of an encode (o, ctx, out: not null): the last result forgotten, `out` the context's last decode
inline int begin(MsgStage *o, const ngz_ctx *ctx, const ngz_batch_out *out) {
    o->have = false;
    o->n_dgrams = o->n_bytes = 0;
    o->launches = 0;
    o->size_ms = o->offsets_ms = o->pack_ms = 0;
    if (int rc = ngzs::check_ctx(o, ctx)) return rc;
    if (!ngzs::slot_table_ok(out) || out->n_slots != ctx->slot_version.size() || out->n_dgrams != ctx->last_in.n)
        return ngzs::fail(o, NGZ_E_INVALID, "slot table: `out` is not the context's last decode");
    if (out->n_sets && !out->sets) return ngzs::fail(o, NGZ_E_INVALID, "no set table");
    return NGZ_OK;
}

// Slot s of `out`: its template version with a column layout, its columns where a lane may load its row's cells
inline int slot_version(MsgStage *o, const ngz_ctx *ctx, const ngz_batch_out *out, uint32_t s, const ngzh::Version **ver) {
    const ngz_slot_info &si = out->slots[s];
    const int32_t vi = ctx->slot_version[s];
    if (vi < 0 || (size_t)vi >= ctx->versions.size()) return ngzs::fail(o, NGZ_E_INVALID, "slot table: `out` is not the context's last decode");
    *ver = &ctx->versions[vi];
    if ((*ver)->specs.size() > (*ver)->fields.size()) return ngzs::fail(o, NGZ_E_INVALID, "a template without its column layout");
    // every column starts at a multiple of 16 bytes: a cell is aligned to its width
    if (si.n_records && (!si.columns || ((uintptr_t)si.columns & 15) || (si.capacity & 15) || si.capacity < si.n_records))
        return ngzs::fail(o, NGZ_E_LIMIT, "unexpected column block alignment");
    return NGZ_OK;
}

inline std::vector<uint32_t> host_dgrams(const ngz_ctx *ctx) {
    std::vector<uint32_t> v;  // (datagram, set position) order: ascending
    for (const ngzh::TemplateSetJson &t : ctx->tmpl_sets)
        if (v.empty() || v.back() != t.dgram) v.push_back(t.dgram);
    return v;
}

// The buffers of an encode whose plan takes plan_bytes (a multiple of 256) at the start of d_in and whose slots
// hold n_records rows, and the tables in them into L.  h_in is zero but for the template datagrams after the plan.
inline int carve(MsgStage *o, ngz_ctx *ctx, const ngz_batch_out *out, void *hip_stream, uint64_t plan_bytes, uint64_t n_records, Layout *L) {
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    const std::vector<uint32_t> host = host_dgrams(ctx);
    const uint64_t tile_cap = n_records / TILE + NS + 1;  // a set's last tile may be short
    if (tile_cap >> 31) return ngzs::fail(o, NGZ_E_LIMIT, "batch too large");
    o->in_bytes = plan_bytes + ngzrow::align256(host.size() * sizeof(uint32_t)) + 256;
    if (int rc = ngzs::device_init(o)) return rc;
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    o->st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, o->scan_a, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(NS + 1), o->st) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, o->scan_b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(D + 1),
                                         o->st) != hipSuccess)
        return ngzs::fail(o, NGZ_E_DEVICE, "scan temp size");
    const uint64_t n_u32 = 2ull * D + 2ull * (NS + 1) + tile_cap, n_u64 = tile_cap + 2ull * NS + D + 1;
    if (o->h_in.reserve(o->in_bytes) || o->d_in.ensure(o->in_bytes) || o->d_how.ensure(D) || o->d_u32.ensure(n_u32) ||
        o->d_tiles.ensure(tile_cap) || o->d_u64.ensure(n_u64) || o->d_offs.ensure(D + 1) || o->d_counters.ensure(C_COUNT) ||
        o->d_scan_tmp.ensure(std::max(o->scan_a, o->scan_b) + 1) || o->h_back.reserve(C_COUNT + 2))
        return ngzs::fail(o, NGZ_E_NOMEM, std::string(o->what) + " buffers");
    memset(o->h_in.p, 0, o->in_bytes);
    if (!host.empty()) memcpy(o->h_in.p + plan_bytes, host.data(), host.size() * sizeof(uint32_t));

    L->host_dgrams = (const uint32_t *)(o->d_in.p + plan_bytes);
    L->n_host = (uint32_t)host.size();
    L->sets = out->sets;
    L->hdr = out->dgrams;
    L->in = ctx->last_in.bytes;
    L->in_size = ctx->last_in.bytes_size;
    L->n_sets = NS;
    L->n_dgrams = D;
    L->n_slots = S;
    L->tile_cap = (uint32_t)tile_cap;
    L->how = o->d_how.p;
    L->dset0 = o->d_u32.p;
    L->dset1 = L->dset0 + D;
    L->ntiles = L->dset1 + D;
    L->tile0 = L->ntiles + NS + 1;
    L->tile_bytes = L->tile0 + NS + 1;
    L->tiles = o->d_tiles.p;
    L->tile_off = o->d_u64.p;
    L->set_len = L->tile_off + tile_cap;
    L->set_off = L->set_len + NS;
    L->dlen = L->set_off + NS;
    L->offs = o->d_offs.p;
    L->counters = o->d_counters.p;
    return NGZ_OK;
}

// The plan up, the counters zero, then the passes up to the tile table.  The stage's size pass follows, if
// there are sets.
template <class S>
int run_tiles(MsgStage *o, const typename S::Args &A) {
    const uint32_t D = A.n_dgrams, NS = A.n_sets;
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->d_in.p, o->h_in.p, o->in_bytes, hipMemcpyHostToDevice, o->st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_counters.p, 0, C_COUNT * sizeof(unsigned long long), o->st));
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], o->st));
    NGZ_STAGE_HIP(o, o->launch(k_dgrams<S>, blocks(D), THREADS, A));
    if (NS) {
        NGZ_STAGE_HIP(o, o->launch(k_sets<S>, blocks(NS), THREADS, A));
        NGZ_STAGE_HIP(o, o->launch(k_tiles<S>, blocks((uint64_t)NS + 1), THREADS, A));
        NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, o->scan_a, (const uint32_t *)A.ntiles, A.tile0, (int)(NS + 1), o->st));
        ++o->launches;
        NGZ_STAGE_HIP(o, o->launch(k_fill<S>, blocks(NS), THREADS, A));
    }
    return NGZ_OK;
}

// After the size pass: the lengths and the offsets scan, read back with the counters (left in h_back) and the
// number of tiles; size_ms and offsets_ms; the output buffer, into A with the total.
template <class S>
int run_offsets(MsgStage *o, typename S::Args &A, uint32_t *n_tiles) {
    const uint32_t D = A.n_dgrams, NS = A.n_sets;
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], o->st));
    if (NS) NGZ_STAGE_HIP(o, o->launch(k_set_len<S>, blocks(NS), THREADS, A));
    NGZ_STAGE_HIP(o, o->launch(k_dgram_len<S>, blocks(D), THREADS, A));
    NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, o->scan_b, (const unsigned long long *)A.dlen, A.offs, (int)(D + 1), o->st));
    ++o->launches;
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[2], o->st));
    unsigned long long *hb = o->h_back.p;
    hb[C_COUNT + 1] = 0;
    NGZ_STAGE_HIP(o, hipMemcpyAsync(hb, o->d_counters.p, C_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, o->st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(hb + C_COUNT, A.offs + D, sizeof(unsigned long long), hipMemcpyDeviceToHost, o->st));
    if (NS) NGZ_STAGE_HIP(o, hipMemcpyAsync(hb + C_COUNT + 1, A.tile0 + NS, sizeof(uint32_t), hipMemcpyDeviceToHost, o->st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(o->st));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->size_ms, o->ev[0], o->ev[1]));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->offsets_ms, o->ev[1], o->ev[2]));
    if (hb[C_ERR] & (ERR_SETS | ERR_TILES)) return ngzs::fail_sets(o);
    if (hb[C_ERR] & ERR_VLEN) return fail_vlen(o);
    *n_tiles = (uint32_t)hb[C_COUNT + 1];
    if (*n_tiles > A.tile_cap) return ngzs::fail_sets(o);
    if (o->d_bytes.ensure(hb[C_COUNT] + NGZ_OUTPUT_GUARD + 16)) return ngzs::fail(o, NGZ_E_NOMEM, std::string(o->what) + " bytes");
    A.out = o->d_bytes.p;
    A.total = hb[C_COUNT];
    return NGZ_OK;
}

// After the pack passes: the error word into h_back[C_COUNT], and the stream drained
inline int read_errors(MsgStage *o) {
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p + C_COUNT, o->d_counters.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, o->st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(o->st));
    return NGZ_OK;
}
// ... and what it says: the encode of n_dgrams datagrams into n_bytes is there to read, or failed
inline int finish(MsgStage *o, uint64_t n_dgrams, uint64_t n_bytes) {
    if (o->h_back.p[C_COUNT] & ERR_VLEN) return fail_vlen(o);
    o->have = true;
    o->n_dgrams = n_dgrams;
    o->n_bytes = n_bytes;
    return NGZ_OK;
}

inline int result(MsgStage *o, const uint8_t **bytes, const uint64_t **offsets, const uint8_t **how, uint64_t *n_dgrams, uint64_t *n_bytes) {
    if (!o) return NGZ_E_INVALID;
    if (!o->have) return ngzs::fail(o, NGZ_E_INVALID, "no encode to read");
    if (bytes) *bytes = o->n_dgrams ? o->d_bytes.p : nullptr;
    if (offsets) *offsets = o->n_dgrams ? (const uint64_t *)o->d_offs.p : nullptr;
    if (how) *how = o->n_dgrams ? o->d_how.p : nullptr;
    if (n_dgrams) *n_dgrams = o->n_dgrams;
    if (n_bytes) *n_bytes = o->n_bytes;
    return NGZ_OK;
}

inline int to_host(MsgStage *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap, uint8_t *how, uint64_t how_cap) {
    if (!o) return NGZ_E_INVALID;
    if (!o->have) return ngzs::fail(o, NGZ_E_INVALID, "no encode to read");
    if ((bytes && bytes_cap < o->n_bytes) || (offsets && offsets_cap < o->n_dgrams + 1) || (how && how_cap < o->n_dgrams))
        return ngzs::fail(o, NGZ_E_INVALID, "a buffer smaller than the result");
    if (!o->n_dgrams) {
        if (offsets && offsets_cap) offsets[0] = 0;
        return NGZ_OK;
    }
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    if (bytes) {
        const uint64_t n = bytes_cap >= o->n_bytes + NGZ_OUTPUT_GUARD ? o->n_bytes + NGZ_OUTPUT_GUARD : o->n_bytes;
        if (n) NGZ_STAGE_HIP(o, hipMemcpy(bytes, o->d_bytes.p, n, hipMemcpyDeviceToHost));
    }
    if (offsets) NGZ_STAGE_HIP(o, hipMemcpy(offsets, o->d_offs.p, (o->n_dgrams + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (how) NGZ_STAGE_HIP(o, hipMemcpy(how, o->d_how.p, o->n_dgrams, hipMemcpyDeviceToHost));
    return NGZ_OK;
}

}  // namespace ngzms
