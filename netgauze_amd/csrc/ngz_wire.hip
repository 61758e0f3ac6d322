// The Encoder half of the codec (include/ngz/flow_wire.h): the IPFIX / NetFlow v9 message of every OK
// datagram of a batch, written again from the decoded columns.  The mirror of the staged decode: host-endian
// SoA columns in, big-endian AoS records out, interleaved with message and set headers in stream order.
// The bookkeeping is ngz_flow_json.hip's: the whole output is one byte stream, every byte a record's or
// glue (message head, set header, NFv9 set padding), and the unit of work is a tile, at most 64 consecutive
// records of one data set: consecutive rows of one slot's columns and consecutive bytes of the output.
// Per encode the host lists every slot's fields as items (column, operation, wire length, offset in the
// record), uploads the plan in one copy, and runs, whatever the number of slots,
//   k_w_dgrams      one thread per datagram: written, not OK, or left to the host for its template sets,
//   k_w_sets        one thread per data set: its datagram's range of sets; an unwritable template's datagram,
//   k_w_tiles       one thread per data set: its tiles, ceil(n / 64), if its datagram is written,
//   a hipcub exclusive scan and k_w_fill: the tile table, and every tile's bytes where the slot's records
//                   have one length (records x rec_len: no pass over rows),
//   k_w_size        only with records of variable-length templates: a wave per such tile, a lane per record
//                   through the counting writer,
//   k_w_set_len, k_w_dgram_len, a hipcub exclusive scan: the u64 offsets and the stats,
//   k_w_glue_dgrams / k_w_glue_sets  message heads, set headers and padding by bytes; every set's and
//                   tile's output offset,
//   k_w_pack_fixed  the transpose: a wave per tile of a fixed-length slot.  Lane l loads row l's cell of
//                   each column (consecutive rows: a coalesced load per column), reverses and narrows it in
//                   registers and stores it into an LDS image of the tile's records at
//                   l * rec_len + field offset, with dword stores where the address allows; the image is
//                   laid out like its output range and leaves in 16-byte stores, ragged ends by bytes,
//   k_w_pack_rows   only with variable-length (or longer-than-image) records: pack_tile (ngz_output_enc.h)
//                   with a lane rendering its record through the byte writer.
// put_field below is the one statement of the field bytes: the host specification (ngz_dgram_wire), the
// counting pass and k_w_pack_rows run it; k_w_pack_fixed is written apart from it and checked against it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_wire.h"
#include "ngz_host.h"
#include "ngz_output_enc.h"
#include "ngz_stage.h"

namespace {

constexpr uint32_t W_THREADS = 256;
constexpr uint32_t W_TILE = 64;
// A wave's record image: 64 records of 256 bytes, and 16 of slack for the output's misalignment
constexpr uint32_t W_IMG = 16384;
constexpr uint32_t ERR_SETS = 1, ERR_VLEN = 2, ERR_TILES = 4;
constexpr uint32_t C_ERR = 0, C_WIRE = 1, C_TEMPLATE = 2, C_UNWRITABLE = 3, C_NOT_OK = 4, C_COUNT = 5;

enum : uint8_t {
    OP_INT,     // the low `len` bytes of the cell's integer, big-endian (len may exceed the column: tcpControlBits)
    OP_BYTES,   // the cell's first `len` bytes
    OP_STRZ,    // the cell's bytes before its first NUL, zero-filled to len
    OP_DTFRAC,  // {u32 secs, u32 nanos}: secs, then nanos * (2^32 - 1) / 10^9
    OP_VLEN,    // {u64 offset, u32 length} into the batch input: length prefix, value
    OP_VRAW,    // the same cell: the value alone (the list types)
    OP_PBYTES,  // a length prefix, then the cell's `width` bytes (IE::Unknown of length 65535)
};
enum : uint32_t { SK_FIXED, SK_ROWS_FIXED, SK_ROWS_VLEN };  // transposed; through the writer, one length; counted

struct WItem {
    const uint8_t *col;  // the field's column: row r at col + r * width
    uint32_t off;        // SK_FIXED / SK_ROWS_FIXED: where the field starts in its record
    uint16_t width, len;
    uint8_t op, reserved[3];
    uint32_t col_off;  // host: the column's bytes per row before it
};
struct WSlot {
    uint32_t item0, n_items;
    uint32_t n_rows, kind;
    uint32_t rec_len, tid;
    uint32_t unwritable, proto;
};
struct WTile {
    uint32_t set, first;
};
struct WArgs {  // passed by value
    const WSlot *slots;
    const WItem *items;
    const uint32_t *host_dgrams;  // the datagrams with (options) template sets, ascending
    const ngz_set_info *sets;
    const ngz_dgram_hdr *hdr;
    const uint8_t *in;  // the batch input
    unsigned long long in_size;
    uint32_t n_host, n_sets, n_dgrams, n_slots, tile_cap, align4;
    uint8_t *how;
    uint32_t *dset0, *dset1;
    uint32_t *ntiles, *tile0;  // per set, and one more: tile0[n_sets] is the number of tiles
    WTile *tiles;
    uint32_t *tile_bytes;
    unsigned long long *tile_off, *set_len, *set_off, *dlen, *offs;
    uint8_t *out;
    unsigned long long total;
    unsigned long long *counters;
};

// The writers: counting and storing (nothing is stored at or past `end`)
struct WCount {
    uint32_t n = 0;
    __host__ __device__ void put(uint32_t) { ++n; }
};
struct WPut {
    uint8_t *p, *end;
    __host__ __device__ void put(uint32_t b) {
        if (p < end) *p = (uint8_t)b;
        ++p;
    }
};

__host__ __device__ inline uint64_t ld_cell(const uint8_t *p, uint32_t w) {  // device: p aligned to w
#ifdef __HIP_DEVICE_COMPILE__
    return w == 8 ? *(const uint64_t *)p : w == 4 ? *(const uint32_t *)p : w == 2 ? *(const uint16_t *)p : *p;
#else
    uint64_t v = 0;
    for (uint32_t i = 0; i < w; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
#endif
}

template <class W>
__host__ __device__ inline void put_be(W &w, uint64_t v, uint32_t len) {
    for (uint32_t i = len; i-- > 0;) w.put(i < 8 ? (uint32_t)(v >> (8 * i)) & 255u : 0u);
}
template <class W>
__host__ __device__ inline void put_prefix(W &w, uint32_t n) {  // generator.rs:3022-3028
    if (n < 255) {
        w.put(n);
    } else {
        w.put(255);
        put_be(w, n, 3);
    }
}
__host__ __device__ inline uint32_t ntp_fraction(uint32_t nanos) { return (uint32_t)(((uint64_t)nanos * 0xFFFFFFFFull) / 1000000000ull); }

// One field of one record: Field::write with the template's length (generator.rs:3010-3361)
template <class W>
__host__ __device__ inline void put_field(W &w, const WItem &it, const uint8_t *cell, const uint8_t *in, unsigned long long in_size,
                                          uint32_t *err) {
    switch (it.op) {
    case OP_INT: put_be(w, ld_cell(cell, it.width), it.len); break;
    case OP_BYTES:
        for (uint32_t i = 0; i < it.len; ++i) w.put(cell[i]);
        break;
    case OP_STRZ: {
        uint32_t n = 0;
        while (n < it.len && cell[n]) w.put(cell[n++]);
        for (; n < it.len; ++n) w.put(0);
        break;
    }
    case OP_DTFRAC: {
        const uint64_t v = ld_cell(cell, 8);
        put_be(w, (uint32_t)v, 4);
        put_be(w, ntp_fraction((uint32_t)(v >> 32)), 4);
        break;
    }
    case OP_VLEN:
    case OP_VRAW: {  // outside the batch input: empty, and the encode fails
        const uint64_t off = ld_cell(cell, 8);
        uint32_t len = (uint32_t)ld_cell(cell + 8, 4);
        if (off > in_size || len > in_size - off) {
            *err |= ERR_VLEN;
            len = 0;
        }
        if (it.op == OP_VLEN) put_prefix(w, len);
        for (uint32_t i = 0; i < len; ++i) w.put(in[off + i]);
        break;
    }
    case OP_PBYTES:
        put_prefix(w, it.width);
        for (uint32_t i = 0; i < it.width; ++i) w.put(cell[i]);
        break;
    }
}

// The 16 (IPFIX) or 20 (NFv9) bytes of a message head; `count`: the NFv9 records of all its sets
template <class W>
__host__ __device__ inline void put_head(W &w, const ngz_dgram_hdr &h, unsigned long long length, unsigned long long count) {
    if (h.version == 10) {
        put_be(w, 10, 2);
        put_be(w, length & 0xFFFFu, 2);
    } else {
        put_be(w, 9, 2);
        put_be(w, count & 0xFFFFu, 2);
        put_be(w, h.sys_up_time, 4);
    }
    put_be(w, h.time, 4);
    put_be(w, h.sequence, 4);
    put_be(w, h.domain, 4);
}
__host__ __device__ inline uint32_t head_len(const ngz_dgram_hdr &h) { return h.version == 10 ? 16u : 20u; }
// The bytes after an NFv9 set of `len` bytes (header included): netflow.rs:133-134 as written
__host__ __device__ inline uint32_t set_pad(uint32_t proto, uint32_t align4, unsigned long long len) {
    return proto == 9 && align4 ? (uint32_t)(len % 4) : 0u;
}

__device__ __forceinline__ bool set_ok(const WArgs &A, const ngz_set_info &si) {
    return si.dgram < A.n_dgrams && si.slot < A.n_slots && (!si.n || (uint64_t)si.rec0 + si.n <= A.slots[si.slot].n_rows);
}

// Row `row` of slot S as a record
template <class W>
__device__ __forceinline__ void put_record(const WArgs &A, const WSlot &S, uint32_t row, W &w, uint32_t *err) {
    for (uint32_t i = 0; i < S.n_items; ++i) {
        const WItem &it = A.items[S.item0 + i];
        put_field(w, it, it.col + (uint64_t)row * it.width, A.in, A.in_size, err);
    }
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(W_THREADS) void k_w_dgrams(const WArgs A) {
    const uint32_t d = blockIdx.x * W_THREADS + threadIdx.x;
    if (d >= A.n_dgrams) return;
    uint8_t how = A.hdr[d].status == NGZ_DG_OK ? NGZ_WIRE_WIRE : NGZ_WIRE_NONE;
    uint32_t lo = 0, hi = A.n_host;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.host_dgrams[mid] < d) lo = mid + 1;
        else hi = mid;
    }
    if (how == NGZ_WIRE_WIRE && lo < A.n_host && A.host_dgrams[lo] == d) how = NGZ_WIRE_HOST;
    A.how[d] = how;
    A.dset0[d] = A.dset1[d] = 0;
}

__global__ __launch_bounds__(W_THREADS) void k_w_sets(const WArgs A) {
    const uint32_t s = blockIdx.x * W_THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const ngz_set_info si = A.sets[s];
    if (!set_ok(A, si)) {
        atomicOr((unsigned int *)&A.counters[C_ERR], ERR_SETS);
        return;
    }
    if (s == 0 || A.sets[s - 1].dgram != si.dgram) A.dset0[si.dgram] = s;  // the sets are in stream order
    if (s + 1 == A.n_sets || A.sets[s + 1].dgram != si.dgram) A.dset1[si.dgram] = s + 1;
    // several sets of a datagram may store the same value; k_w_dgrams ran before
    if (A.slots[si.slot].unwritable && A.how[si.dgram] != NGZ_WIRE_NONE) A.how[si.dgram] = NGZ_WIRE_UNWRITABLE;
}

__global__ __launch_bounds__(W_THREADS) void k_w_tiles(const WArgs A) {
    const uint32_t s = blockIdx.x * W_THREADS + threadIdx.x;
    if (s > A.n_sets) return;
    uint32_t n = 0;
    if (s < A.n_sets) {
        const ngz_set_info si = A.sets[s];
        if (set_ok(A, si) && A.how[si.dgram] == NGZ_WIRE_WIRE) n = (si.n + W_TILE - 1) / W_TILE;
    }
    A.ntiles[s] = n;  // ntiles[n_sets] = 0: the scan's last item
}

__global__ __launch_bounds__(W_THREADS) void k_w_fill(const WArgs A) {
    const uint32_t s = blockIdx.x * W_THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const uint32_t t0 = A.tile0[s], n = A.ntiles[s];
    if (!n) return;
    const ngz_set_info si = A.sets[s];
    const uint32_t rec_len = A.slots[si.slot].rec_len;  // SK_ROWS_VLEN: k_w_size stores the bytes after this
    for (uint32_t t = 0; t < n; ++t) {
        if (t0 + t >= A.tile_cap || t0 + t < t0) {
            atomicOr((unsigned int *)&A.counters[C_ERR], ERR_TILES);
            break;
        }
        A.tiles[t0 + t] = WTile{s, t * W_TILE};
        A.tile_bytes[t0 + t] = min(W_TILE, si.n - t * W_TILE) * rec_len;
    }
}

__global__ __launch_bounds__(W_THREADS) void k_w_size(const WArgs A) {
    const uint32_t lane = threadIdx.x & 63u, n_tiles = min(A.tile0[A.n_sets], A.tile_cap);
    uint32_t err = 0;
    for (uint32_t t = blockIdx.x * (W_THREADS / 64u) + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * (W_THREADS / 64u)) {
        const WTile tl = A.tiles[t];
        const ngz_set_info si = A.sets[tl.set];
        const WSlot &S = A.slots[si.slot];
        if (S.kind != SK_ROWS_VLEN) continue;
        const uint32_t cnt = min(W_TILE, si.n - tl.first);
        WCount w;
        if (lane < cnt) put_record(A, S, si.rec0 + tl.first + lane, w, &err);
        const uint64_t sum = ngzs::wave_sum(w.n);
        if (lane == 0) A.tile_bytes[t] = (uint32_t)sum;
    }
    if (err) atomicOr((unsigned int *)&A.counters[C_ERR], err);
}

// Header, tiles, padding: the padding is part of the length the header carries
__global__ __launch_bounds__(W_THREADS) void k_w_set_len(const WArgs A) {
    const uint32_t s = blockIdx.x * W_THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const ngz_set_info si = A.sets[s];
    unsigned long long len = 0;
    if (set_ok(A, si) && A.how[si.dgram] == NGZ_WIRE_WIRE) {
        len = 4;
        const uint32_t t1 = min(A.tile0[s + 1], A.tile_cap);
        for (uint32_t t = A.tile0[s]; t < t1; ++t) len += A.tile_bytes[t];
        len += set_pad(A.slots[si.slot].proto, A.align4, len);
    }
    A.set_len[s] = len;
}

__global__ __launch_bounds__(W_THREADS) void k_w_dgram_len(const WArgs A) {
    __shared__ unsigned long long acc[4];
    const uint32_t d = blockIdx.x * W_THREADS + threadIdx.x;
    uint64_t c[4] = {0, 0, 0, 0};  // written, left for templates, unwritable, not OK
    if (d < A.n_dgrams) {
        unsigned long long len = 0;
        const uint8_t how = A.how[d];
        if (how == NGZ_WIRE_WIRE) {
            len = head_len(A.hdr[d]);
            const uint32_t s0 = A.dset0[d], s1 = min(A.dset1[d], A.n_sets);
            for (uint32_t s = s0; s < s1; ++s) len += A.set_len[s];
        }
        c[how == NGZ_WIRE_WIRE ? 0 : how == NGZ_WIRE_HOST ? 1 : how == NGZ_WIRE_UNWRITABLE ? 2 : 3] = 1;
        A.dlen[d] = len;
        if (d == 0) A.dlen[A.n_dgrams] = 0;  // the scan's last item
    }
    unsigned long long *const dst[4] = {&A.counters[C_WIRE], &A.counters[C_TEMPLATE], &A.counters[C_UNWRITABLE], &A.counters[C_NOT_OK]};
    ngzs::block_add<4>(acc, c, dst);
}

// The message head; where each of the datagram's sets starts
__global__ __launch_bounds__(W_THREADS) void k_w_glue_dgrams(const WArgs A) {
    const uint32_t d = blockIdx.x * W_THREADS + threadIdx.x;
    if (d >= A.n_dgrams || A.how[d] != NGZ_WIRE_WIRE) return;
    const unsigned long long o0 = A.offs[d], o1 = min(A.offs[d + 1], A.total);
    const uint32_t s0 = A.dset0[d], s1 = min(A.dset1[d], A.n_sets);
    unsigned long long count = 0, o = o0 + head_len(A.hdr[d]);
    for (uint32_t s = s0; s < s1; ++s) {
        count += A.sets[s].n;
        A.set_off[s] = o;
        o += A.set_len[s];
    }
    WPut w{A.out + o0, A.out + o1};
    put_head(w, A.hdr[d], o - o0, count);
}

// The set's header and padding; where each of its tiles starts
__global__ __launch_bounds__(W_THREADS) void k_w_glue_sets(const WArgs A) {
    const uint32_t s = blockIdx.x * W_THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const ngz_set_info si = A.sets[s];
    if (!set_ok(A, si) || A.how[si.dgram] != NGZ_WIRE_WIRE) return;
    const unsigned long long o0 = A.set_off[s], len = A.set_len[s], o1 = min(o0 + len, A.total);
    WPut w{A.out + o0, A.out + o1};
    put_be(w, A.slots[si.slot].tid, 2);
    put_be(w, len & 0xFFFFu, 2);
    const uint32_t t1 = min(A.tile0[s + 1], A.tile_cap);
    for (uint32_t t = A.tile0[s]; t < t1; ++t) {
        A.tile_off[t] = (unsigned long long)(w.p - A.out);
        w.p += A.tile_bytes[t];
    }
    while (w.p < A.out + o0 + len) w.put(0);
}

// `len` bytes of v, big-endian, at image byte `pos`: one store of len bytes where pos is a multiple of it
__device__ __forceinline__ void st_be(uint8_t *img, uint32_t pos, uint64_t v, uint32_t len) {
    if (len == 4 && !(pos & 3u)) {
        *(uint32_t *)(img + pos) = __builtin_bswap32((uint32_t)v);
    } else if (len == 8 && !(pos & 3u)) {
        const uint64_t r = __builtin_bswap64(v);
        *(uint32_t *)(img + pos) = (uint32_t)r;
        *(uint32_t *)(img + pos + 4) = (uint32_t)(r >> 32);
    } else if (len == 2 && !(pos & 1u)) {
        *(uint16_t *)(img + pos) = __builtin_bswap16((uint16_t)v);
    } else {
        for (uint32_t i = 0; i < len; ++i) img[pos + i] = len - 1 - i < 8 ? (uint8_t)(v >> (8 * (len - 1 - i))) : 0;
    }
}

// The transpose.  One wave per block: LDS, not threads, bounds what a CU holds
__global__ __launch_bounds__(64) void k_w_pack_fixed(const WArgs A, const uint32_t n_tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t img[W_IMG + 16];
    const uint32_t lane = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const WTile tl = A.tiles[t];
        const ngz_set_info si = A.sets[tl.set];
        const WSlot &S = A.slots[si.slot];
        if (S.kind != SK_FIXED) continue;
        const uint32_t cnt = min(W_TILE, si.n - tl.first), rl = S.rec_len;
        const uint32_t rpg = min(W_TILE, W_IMG / rl);  // records an image holds: rl <= W_IMG
        for (uint32_t g0 = 0; g0 < cnt; g0 += rpg) {
            const uint32_t gc = min(rpg, cnt - g0), len = gc * rl;
            const unsigned long long o = A.tile_off[t] + (unsigned long long)g0 * rl;
            uint8_t *const dst = A.out + o;
            const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
            if (lane < gc) {
                const uint64_t row = (uint64_t)si.rec0 + tl.first + g0 + lane;
                const uint32_t r0 = mis + lane * rl;
                for (uint32_t i = 0; i < S.n_items; ++i) {
                    const WItem &it = A.items[S.item0 + i];
                    const uint8_t *cell = it.col + row * it.width;
                    const uint32_t pos = r0 + it.off;
                    switch (it.op) {
                    case OP_INT: st_be(img, pos, ld_cell(cell, it.width), it.len); break;
                    case OP_DTFRAC: {
                        const uint64_t v = *(const uint64_t *)cell;
                        st_be(img, pos, (uint32_t)v, 4);
                        st_be(img, pos + 4, ntp_fraction((uint32_t)(v >> 32)), 4);
                        break;
                    }
                    case OP_STRZ: {
                        uint32_t n = 0;
                        for (; n < it.len && cell[n]; ++n) img[pos + n] = cell[n];
                        for (; n < it.len; ++n) img[pos + n] = 0;
                        break;
                    }
                    default:  // OP_BYTES: a column as wide as a multiple of a dword has its cells on dwords
                        if (!((it.width | it.len | pos) & 3u)) {
                            for (uint32_t k = 0; k < it.len; k += 4) *(uint32_t *)(img + pos + k) = *(const uint32_t *)(cell + k);
                        } else {
                            for (uint32_t k = 0; k < it.len; ++k) img[pos + k] = cell[k];
                        }
                        break;
                    }
                }
            }
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            if (o + len <= A.total) {  // ragged head, then tail, then the aligned middle: pack_tile's copy-out
                const uint32_t head = min(len, (16u - mis) & 15u);
                const uint32_t n16 = (len - head) / 16u, tail0 = head + 16u * n16;
                if (lane < head) dst[lane] = img[mis + lane];
                if (lane < len - tail0) dst[tail0 + lane] = img[mis + tail0 + lane];
                for (uint32_t i = lane; i < n16; i += 64u) *(uint4 *)(dst + head + 16u * i) = *(const uint4 *)(img + mis + head + 16u * i);
            }
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Records through the byte writer: variable-length ones, and fixed ones an image cannot hold
__global__ __launch_bounds__(64) void k_w_pack_rows(const WArgs A, const uint32_t n_tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t img[W_IMG + 16];  // pack_tile's
    const uint32_t lane = threadIdx.x;
    uint32_t err = 0;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const WTile tl = A.tiles[t];
        const ngz_set_info si = A.sets[tl.set];
        const WSlot &S = A.slots[si.slot];
        if (S.kind == SK_FIXED) continue;
        const uint32_t cnt = min(W_TILE, si.n - tl.first), row = si.rec0 + tl.first + lane;
        uint32_t mine = 0;
        if (lane < cnt) {
            if (S.kind == SK_ROWS_VLEN) {
                WCount c;
                put_record(A, S, row, c, &err);
                mine = c.n;
            } else {
                mine = S.rec_len;
            }
        }
        uint32_t incl = mine;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const uint32_t up = __shfl_up(incl, k, 64);
            if (lane >= (uint32_t)k) incl += up;
        }
        ngzenc::pack_tile<W_IMG, WPut, WPut>(lane, cnt, A.tile_off[t], incl - mine, incl, A.out, A.total, img,
                                             [&](auto &w) { put_record(A, S, row, w, &err); });
    }
    if (err) atomicOr((unsigned int *)&A.counters[C_ERR], err);
}

__global__ __launch_bounds__(W_THREADS) void k_w_guard(uint8_t *p, uint32_t n) {
    if (threadIdx.x < n) p[threadIdx.x] = 0xA5;
}

}  // namespace

struct ngz_wire : ngzs::Stage {
    ngz_wire() : Stage(4) {}
    float size_ms = 0, offsets_ms = 0, glue_ms = 0, pack_ms = 0;
    int launches = 0;
    int align4 = 0;
    uint64_t n_dgrams = 0, n_bytes = 0;  // the last encode
    bool have = false;
    ngzh::DevBuf<uint8_t> d_in, d_how, d_bytes, d_scan_tmp;  // d_in: slots, items, template datagrams
    ngzh::DevBuf<uint32_t> d_u32;                            // dset0, dset1, ntiles, tile0, tile_bytes
    ngzh::DevBuf<WTile> d_tiles;
    ngzh::DevBuf<unsigned long long> d_u64, d_offs, d_counters;  // d_u64: tile_off, set_len, set_off, dlen
    ngzs::PinnedBuf<uint8_t> h_in;
    ngzs::PinnedBuf<unsigned long long> h_back;  // the counters, the total, the tiles
};

namespace {

using ngzh::Spec;

// Field::write's choice for the fields of one template version: its items, and what the slot is.
// false: a column the loaders cannot read.
bool plan_version(const ngzh::Version &ver, std::vector<WItem> &items, WSlot &ws, std::string *why) {
    ws = WSlot{};
    ws.item0 = (uint32_t)items.size();
    ws.n_items = (uint32_t)ver.specs.size();
    ws.tid = ver.tid;
    ws.proto = ver.proto;
    uint32_t off = 0;
    bool vlen = false;
    for (uint32_t f = 0; f < ws.n_items; ++f) {
        const Spec &sp = ver.specs[f];
        const DevField &fd = ver.plan.f[f];
        WItem it{};
        it.off = off;
        it.width = fd.width;
        it.len = sp.length;
        it.col_off = fd.col_off;
        const bool int_w = fd.width == 1 || fd.width == 2 || fd.width == 4 || fd.width == 8;
        const bool known = sp.kind == ngzh::IK_IANA || sp.kind == ngzh::IK_VENDOR;
        bool ok = true;
        switch (fd.kind) {
        case NGZ_K_UINT:
        case NGZ_K_SINT:
        case NGZ_K_TCPFLAGS:
        case NGZ_K_BOOL:
        case NGZ_K_SCOPE32:
        case NGZ_K_DTMS: it.op = OP_INT; ok = int_w && sp.length <= 8; break;
        case NGZ_K_DTFRAC: it.op = OP_DTFRAC; ok = fd.width == 8 && sp.length == 8; break;
        case NGZ_K_STR: it.op = OP_STRZ; break;
        case NGZ_K_U256: it.op = OP_BYTES; ok = sp.length <= fd.width; break;
        case NGZ_K_BYTES:
            it.op = OP_BYTES;
            if (sp.length == 0xFFFF) {  // IE::Unknown reads 65535 fixed bytes; its writer prefixes them
                if (ver.proto == 9) ws.unwritable = 1;
                else it.op = OP_PBYTES, vlen = true;
            }
            break;
        case NGZ_K_VLEN: {
            const bool list = known && (sp.dtype == ngzh::DT_basicList || sp.dtype == ngzh::DT_subTemplateList ||
                                        sp.dtype == ngzh::DT_subTemplateMultiList);
            it.op = list ? OP_VRAW : OP_VLEN;
            ok = fd.width == 16;
            vlen = true;
            if (ver.proto == 9) ws.unwritable = 1;  // 65535 is a literal length there
            break;
        }
        default:  // NGZ_K_FAIL, a length the decode refuses: no record of this template ever decodes, and the
                  // reference's writer has no consistent set for it; the slot is planned as never written
            it.op = OP_BYTES;
            it.width = it.len = 0;
            ws.unwritable = 1;
            break;
        }
        if (!ok) {
            if (why) *why = "field " + std::to_string(f) + " of template " + std::to_string(ver.tid) + ": a column the writers cannot read";
            return false;
        }
        off += sp.length;
        items.push_back(it);
    }
    ws.rec_len = vlen ? 0 : off;
    ws.kind = vlen ? SK_ROWS_VLEN : off && off <= W_IMG ? SK_FIXED : SK_ROWS_FIXED;
    return true;
}

uint32_t blocks(uint64_t items) { return (uint32_t)((items + W_THREADS - 1) / W_THREADS); }

void push_be(std::vector<uint8_t> &o, uint64_t v, uint32_t len) {
    for (uint32_t i = len; i-- > 0;) o.push_back((uint8_t)(v >> (8 * i)));
}

// One field specifier at p[pos, end) again (serializer/mod.rs:49-69); false: it does not parse
bool rewrite_spec(const uint8_t *p, uint32_t &pos, uint32_t end, std::vector<uint8_t> &o) {
    if (end - pos < 4) return false;
    const uint32_t id = ngzh::rd16(p + pos), len = ngzh::rd16(p + pos + 2);
    uint32_t pen = 0;
    pos += 4;
    if (id & 0x8000u) {
        if (end - pos < 4) return false;
        pen = ngzh::rd32(p + pos);
        pos += 4;
    }
    push_be(o, pen ? id | 0x8000u : id & 0x7FFFu, 2);
    push_be(o, len, 2);
    if (pen) push_be(o, pen, 4);
    return true;
}

// The records of the (options) template set at p[pos, end) again, without its padding
// (serializer/ipfix.rs:84-150, netflow.rs:200-280); their number, or -1
int rewrite_template_set(uint32_t proto, uint32_t id, const uint8_t *p, uint32_t pos, uint32_t end, std::vector<uint8_t> &o) {
    int n = 0;
    const bool options = id == (proto == 10 ? 3u : 1u);
    while (end - pos > 3) {  // fewer than four bytes are padding, in both kinds of set
        if (options && end - pos < 6) return -1;
        const uint32_t tid = ngzh::rd16(p + pos), a = ngzh::rd16(p + pos + 2);
        push_be(o, tid, 2);
        push_be(o, a, 2);
        pos += 4;
        if (!options || proto == 10) {
            if (options) {
                push_be(o, ngzh::rd16(p + pos), 2);  // the scope field count
                pos += 2;
            }
            for (uint32_t f = 0; f < a; ++f)
                if (!rewrite_spec(p, pos, end, o)) return -1;
        } else {  // NFv9: scope bytes, option bytes
            const uint32_t b = ngzh::rd16(p + pos);
            push_be(o, b, 2);
            pos += 2;
            if (end - pos < a + b) return -1;
            o.insert(o.end(), p + pos, p + pos + a);  // scope specifiers: {type, length}
            pos += a;
            const size_t at = o.size();
            for (const uint32_t opt_end = pos + b; pos < opt_end;)
                if (!rewrite_spec(p, pos, opt_end, o)) return -1;
            const size_t wrote = o.size() - at;  // the option length is the written specifiers'
            o[at - a - 2] = (uint8_t)(wrote >> 8);
            o[at - a - 1] = (uint8_t)wrote;
        }
        ++n;
    }
    return n;
}

struct HostPlan {
    std::vector<WItem> items;
    WSlot slot;
    bool ok;
};
struct WVec {  // the host function's writer
    std::vector<uint8_t> *v;
    void put(uint32_t b) { v->push_back((uint8_t)b); }
};

int64_t dgram_wire(ngz_ctx *ctx, uint32_t d, int align4, uint8_t *buf, size_t cap) {
    if (!ctx || d >= ctx->last_in.n) return NGZ_E_INVALID;
    if (ctx->async.pending.load()) return NGZ_E_INVALID;
    if (hipSetDevice(ctx->device)) return NGZ_E_DEVICE;
    if (!ctx->json_view || ctx->json_view->serial != ctx->batch_serial) {
        auto v = std::make_shared<ngzh::JsonView>();
        const int rc = ngzh::json_view_load(ctx, nullptr, *v);
        if (rc) return rc;
        ctx->json_view = v;
    }
    const ngzh::JsonView &v = *ctx->json_view;
    const ngz_dgram_hdr &h = v.hdr[d];
    if (h.status != NGZ_DG_OK) return NGZ_E_INVALID;
    const uint8_t *p = v.bytes + v.offs[d];
    const uint32_t dl = v.lens[d];
    std::vector<uint8_t> body;  // the sets
    std::map<int32_t, HostPlan> plans;
    uint64_t count = 0;
    uint32_t ds = v.set_first[d], de = v.set_first[d + 1], ts = v.tset_first[d], te = v.tset_first[d + 1];
    while (ds < de || ts < te) {
        const bool take_t = ts < te && (ds >= de || ctx->tmpl_sets[ts].set_pos < v.sets[ds].set_pos);
        const size_t at = body.size();
        body.resize(at + 4);
        uint32_t id;
        if (take_t) {
            const uint32_t sp = ctx->tmpl_sets[ts++].set_pos;
            if (sp + 4u > dl) return NGZ_E_INVALID;
            id = ngzh::rd16(p + sp);
            const uint32_t sl = ngzh::rd16(p + sp + 2);
            if (sl < 4 || sp + sl > dl) return NGZ_E_INVALID;
            const int n = rewrite_template_set(h.version, id, p, sp + 4, sp + sl, body);
            if (n < 0) return NGZ_E_INVALID;
            count += (uint64_t)n;
        } else {
            const ngz_set_info &si = v.sets[ds++];
            const ngzh::Version &ver = ctx->versions[ctx->slot_version[si.slot]];
            auto pl = plans.find(ctx->slot_version[si.slot]);  // one plan per template version and call
            if (pl == plans.end()) {
                pl = plans.emplace(ctx->slot_version[si.slot], HostPlan{}).first;
                pl->second.ok = plan_version(ver, pl->second.items, pl->second.slot, nullptr);
            }
            if (!pl->second.ok || pl->second.slot.unwritable) return NGZ_E_INVALID;
            const std::vector<WItem> &items = pl->second.items;
            id = ver.tid;
            count += si.n;
            const uint32_t rows = ctx->slot_rt[si.slot].cap;
            const uint8_t *cols = v.cols[si.slot].data();
            auto cell = [&](const WItem &it, uint32_t r) { return cols + (uint64_t)rows * it.col_off + ((uint64_t)si.rec0 + r) * it.width; };
            uint32_t err = 0;
            WVec st{&body};  // one walk: the device's put_field into a growing buffer
            for (uint32_t r = 0; r < si.n; ++r)
                for (const WItem &it : items) put_field(st, it, cell(it, r), v.bytes, ctx->last_in.bytes_size, &err);
            if (err) return NGZ_E_INVALID;
        }
        uint64_t len = body.size() - at;
        const uint32_t pad = set_pad(h.version, (uint32_t)align4, len);
        body.resize(body.size() + pad, 0);
        len += pad;
        body[at] = (uint8_t)(id >> 8);
        body[at + 1] = (uint8_t)id;
        body[at + 2] = (uint8_t)(len >> 8);
        body[at + 3] = (uint8_t)len;
    }
    uint8_t head[20];
    WPut w{head, head + sizeof head};
    put_head(w, h, head_len(h) + body.size(), count);
    const size_t hl = head_len(h), total = hl + body.size();
    if (buf && cap) {
        const size_t a = std::min(cap, hl);
        memcpy(buf, head, a);
        if (cap > hl) memcpy(buf + hl, body.data(), std::min(cap - hl, body.size()));
    }
    return (int64_t)total;
}

}  // namespace

extern "C" {

int ngz_wire_abi_version(void) { return NGZ_WIRE_ABI_VERSION; }

int64_t ngz_dgram_wire(ngz_ctx *ctx, uint32_t dgram, uint8_t *buf, size_t cap) { return dgram_wire(ctx, dgram, 0, buf, cap); }
int64_t ngz_dgram_wire_aligned(ngz_ctx *ctx, uint32_t dgram, uint8_t *buf, size_t cap) { return dgram_wire(ctx, dgram, 1, buf, cap); }

int ngz_wire_create(int device, ngz_wire **out) {
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0) return NGZ_E_INVALID;
    ngz_wire *w = new ngz_wire;
    w->device = device;
    *out = w;
    return NGZ_OK;
}

void ngz_wire_destroy(ngz_wire *w) {
    if (!w) return;
    if (w->device_ready) {
        hipSetDevice(w->device);
        w->d_in.release();
        w->d_how.release();
        w->d_bytes.release();
        w->d_scan_tmp.release();
        w->d_u32.release();
        w->d_tiles.release();
        w->d_u64.release();
        w->d_offs.release();
        w->d_counters.release();
    }
    delete w;
}

const char *ngz_wire_last_error(ngz_wire *w) { return w ? w->last_error.c_str() : "null wire stage"; }

int ngz_wire_set_option(ngz_wire *w, int option, int64_t value) {
    if (!w) return NGZ_E_INVALID;
    if (option != NGZ_WIRE_OPT_ALIGN4 || (value != 0 && value != 1)) return ngzs::fail(w, NGZ_E_INVALID, "unknown option or value");
    w->align4 = (int)value;
    return NGZ_OK;
}

int ngz_wire_encode(ngz_wire *o, ngz_ctx *ctx, const ngz_batch_out *out, ngz_wire_stats *stats, void *hip_stream) {
    if (!o || !ctx || !out) return NGZ_E_INVALID;
    if (stats) memset(stats, 0, sizeof *stats);
    o->have = false;
    o->n_dgrams = o->n_bytes = 0;
    o->launches = 0;
    o->size_ms = o->offsets_ms = o->glue_ms = o->pack_ms = 0;
    if (int rc = ngzs::check_ctx(o, ctx)) return rc;
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    if (!ngzs::slot_table_ok(out) || S != ctx->slot_version.size() || D != ctx->last_in.n)
        return ngzs::fail(o, NGZ_E_INVALID, "slot table: `out` is not the context's last decode");
    if (NS && !out->sets) return ngzs::fail(o, NGZ_E_INVALID, "no set table");
    if (!D) {  // no datagram: no kernel
        o->have = true;
        return NGZ_OK;
    }

    // the plan: every slot's record as items
    std::vector<WSlot> slots(S);
    std::vector<WItem> items;
    uint64_t n_records = 0;
    bool any_fixed = false, any_rows = false, any_vlen = false;
    for (uint32_t s = 0; s < S; ++s) {
        const ngz_slot_info &si = out->slots[s];
        const int32_t vi = ctx->slot_version[s];
        if (vi < 0 || (size_t)vi >= ctx->versions.size()) return ngzs::fail(o, NGZ_E_INVALID, "slot table: `out` is not the context's last decode");
        const ngzh::Version &ver = ctx->versions[vi];
        if (ver.specs.size() > ver.fields.size()) return ngzs::fail(o, NGZ_E_INVALID, "a template without its column layout");
        // every column starts at a multiple of 16 bytes: a cell is aligned to its width
        if (si.n_records && (!si.columns || ((uintptr_t)si.columns & 15) || (si.capacity & 15) || si.capacity < si.n_records))
            return ngzs::fail(o, NGZ_E_LIMIT, "unexpected column block alignment");
        std::string why;
        if (!plan_version(ver, items, slots[s], &why)) return ngzs::fail(o, NGZ_E_LIMIT, why);
        WSlot &ws = slots[s];
        ws.n_rows = si.n_records;
        for (uint32_t i = 0; i < ws.n_items; ++i)
            items[ws.item0 + i].col = si.columns ? si.columns + (uint64_t)si.capacity * items[ws.item0 + i].col_off : nullptr;
        n_records += si.n_records;
        if (si.n_records && !ws.unwritable) {
            any_fixed = any_fixed || ws.kind == SK_FIXED;
            any_rows = any_rows || ws.kind != SK_FIXED;
            any_vlen = any_vlen || ws.kind == SK_ROWS_VLEN;
        }
    }
    std::vector<uint32_t> host_dgrams;  // (datagram, set position) order: ascending
    for (const ngzh::TemplateSetJson &t : ctx->tmpl_sets)
        if (host_dgrams.empty() || host_dgrams.back() != t.dgram) host_dgrams.push_back(t.dgram);
    const uint64_t tile_cap = n_records / W_TILE + NS + 1;  // a set's last tile may be short
    if (tile_cap >> 31) return ngzs::fail(o, NGZ_E_LIMIT, "batch too large");

    auto align256 = [](uint64_t n) { return (n + 255) & ~255ull; };
    const uint64_t items_at = align256(slots.size() * sizeof(WSlot)), host_at = items_at + align256(items.size() * sizeof(WItem));
    const uint64_t in_bytes = host_at + align256(host_dgrams.size() * sizeof(uint32_t)) + 256;
    if (int rc = ngzs::device_init(o)) return rc;
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    size_t scan_a = 0, scan_b = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_a, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)(NS + 1), st) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(D + 1), st) !=
            hipSuccess)
        return ngzs::fail(o, NGZ_E_DEVICE, "scan temp size");
    const size_t scan_bytes = std::max(scan_a, scan_b);
    const uint64_t n_u32 = 2ull * D + 2ull * (NS + 1) + tile_cap, n_u64 = tile_cap + 2ull * NS + D + 1;
    if (o->h_in.reserve(in_bytes) || o->d_in.ensure(in_bytes) || o->d_how.ensure(D) || o->d_u32.ensure(n_u32) || o->d_tiles.ensure(tile_cap) ||
        o->d_u64.ensure(n_u64) || o->d_offs.ensure(D + 1) || o->d_counters.ensure(C_COUNT) || o->d_scan_tmp.ensure(scan_bytes + 1) ||
        o->h_back.reserve(C_COUNT + 2))
        return ngzs::fail(o, NGZ_E_NOMEM, "wire buffers");
    uint8_t *h = o->h_in.p;
    memset(h, 0, in_bytes);
    if (S) memcpy(h, slots.data(), slots.size() * sizeof(WSlot));
    if (!items.empty()) memcpy(h + items_at, items.data(), items.size() * sizeof(WItem));
    if (!host_dgrams.empty()) memcpy(h + host_at, host_dgrams.data(), host_dgrams.size() * sizeof(uint32_t));

    WArgs A{};
    A.slots = (const WSlot *)o->d_in.p;
    A.items = (const WItem *)(o->d_in.p + items_at);
    A.host_dgrams = (const uint32_t *)(o->d_in.p + host_at);
    A.n_host = (uint32_t)host_dgrams.size();
    A.sets = out->sets;
    A.hdr = out->dgrams;
    A.in = ctx->last_in.bytes;
    A.in_size = ctx->last_in.bytes_size;
    A.n_sets = NS;
    A.n_dgrams = D;
    A.n_slots = S;
    A.tile_cap = (uint32_t)tile_cap;
    A.align4 = (uint32_t)o->align4;
    A.how = o->d_how.p;
    A.dset0 = o->d_u32.p;
    A.dset1 = A.dset0 + D;
    A.ntiles = A.dset1 + D;
    A.tile0 = A.ntiles + NS + 1;
    A.tile_bytes = A.tile0 + NS + 1;
    A.tiles = o->d_tiles.p;
    A.tile_off = o->d_u64.p;
    A.set_len = A.tile_off + tile_cap;
    A.set_off = A.set_len + NS;
    A.dlen = A.set_off + NS;
    A.offs = o->d_offs.p;
    A.counters = o->d_counters.p;

    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->d_in.p, h, in_bytes, hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_counters.p, 0, C_COUNT * sizeof(unsigned long long), st));
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
    auto launch = [&](auto kernel, uint32_t nb, uint32_t threads, auto... args) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(threads), 0, st, args...);
        ++o->launches;
        return hipGetLastError();
    };
    NGZ_STAGE_HIP(o, launch(k_w_dgrams, blocks(D), W_THREADS, A));
    if (NS) {
        NGZ_STAGE_HIP(o, launch(k_w_sets, blocks(NS), W_THREADS, A));
        NGZ_STAGE_HIP(o, launch(k_w_tiles, blocks((uint64_t)NS + 1), W_THREADS, A));
        NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, scan_a, (const uint32_t *)A.ntiles, A.tile0, (int)(NS + 1), st));
        ++o->launches;
        NGZ_STAGE_HIP(o, launch(k_w_fill, blocks(NS), W_THREADS, A));
        if (any_vlen) {
            const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((tile_cap + 3) / 4, (uint64_t)o->n_cus * 16));
            NGZ_STAGE_HIP(o, launch(k_w_size, nb, W_THREADS, A));
        }
    }
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
    if (NS) NGZ_STAGE_HIP(o, launch(k_w_set_len, blocks(NS), W_THREADS, A));
    NGZ_STAGE_HIP(o, launch(k_w_dgram_len, blocks(D), W_THREADS, A));
    NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, scan_b, (const unsigned long long *)A.dlen, A.offs, (int)(D + 1), st));
    ++o->launches;
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[2], st));
    unsigned long long *hb = o->h_back.p;
    hb[C_COUNT + 1] = 0;
    NGZ_STAGE_HIP(o, hipMemcpyAsync(hb, o->d_counters.p, C_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(hb + C_COUNT, A.offs + D, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (NS) NGZ_STAGE_HIP(o, hipMemcpyAsync(hb + C_COUNT + 1, A.tile0 + NS, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->size_ms, o->ev[0], o->ev[1]));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->offsets_ms, o->ev[1], o->ev[2]));
    if (hb[C_ERR] & (ERR_SETS | ERR_TILES)) return ngzs::fail_sets(o);
    if (hb[C_ERR] & ERR_VLEN) return ngzs::fail(o, NGZ_E_INVALID, "a variable-length cell outside the batch input");
    const unsigned long long total = hb[C_COUNT];
    const uint32_t n_tiles = (uint32_t)hb[C_COUNT + 1];
    if (n_tiles > tile_cap) return ngzs::fail_sets(o);
    if (o->d_bytes.ensure(total + NGZ_OUTPUT_GUARD + 16)) return ngzs::fail(o, NGZ_E_NOMEM, "wire bytes");
    A.out = o->d_bytes.p;
    A.total = total;
    NGZ_STAGE_HIP(o, launch(k_w_guard, 1u, W_THREADS, A.out + total, (uint32_t)NGZ_OUTPUT_GUARD));
    if (total) {
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
        NGZ_STAGE_HIP(o, launch(k_w_glue_dgrams, blocks(D), W_THREADS, A));
        if (NS) NGZ_STAGE_HIP(o, launch(k_w_glue_sets, blocks(NS), W_THREADS, A));
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
        if (n_tiles) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)o->n_cus * 32);
            if (any_fixed) NGZ_STAGE_HIP(o, launch(k_w_pack_fixed, nb, 64u, A, n_tiles));
            if (any_rows) NGZ_STAGE_HIP(o, launch(k_w_pack_rows, nb, 64u, A, n_tiles));
        }
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[3], st));
    }
    NGZ_STAGE_HIP(o, hipMemcpyAsync(hb + C_COUNT, o->d_counters.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    if (total) {
        NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->glue_ms, o->ev[0], o->ev[1]));
        NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->pack_ms, o->ev[1], o->ev[3]));
    }
    if (hb[C_COUNT] & ERR_VLEN) return ngzs::fail(o, NGZ_E_INVALID, "a variable-length cell outside the batch input");
    o->have = true;
    o->n_dgrams = D;
    o->n_bytes = total;
    if (stats) *stats = ngz_wire_stats{hb[C_WIRE], total, hb[C_TEMPLATE], hb[C_UNWRITABLE], hb[C_NOT_OK]};
    return NGZ_OK;
}

int ngz_wire_result(ngz_wire *o, const uint8_t **bytes, const uint64_t **offsets, const uint8_t **how, uint64_t *n_dgrams, uint64_t *n_bytes) {
    if (!o) return NGZ_E_INVALID;
    if (!o->have) return ngzs::fail(o, NGZ_E_INVALID, "no encode to read");
    if (bytes) *bytes = o->n_dgrams ? o->d_bytes.p : nullptr;
    if (offsets) *offsets = o->n_dgrams ? (const uint64_t *)o->d_offs.p : nullptr;
    if (how) *how = o->n_dgrams ? o->d_how.p : nullptr;
    if (n_dgrams) *n_dgrams = o->n_dgrams;
    if (n_bytes) *n_bytes = o->n_bytes;
    return NGZ_OK;
}

int ngz_wire_to_host(ngz_wire *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap, uint8_t *how, uint64_t how_cap) {
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

int ngz_wire_last_timing(ngz_wire *o, float *size_ms, float *offsets_ms, float *glue_ms, float *pack_ms) {
    if (!o || !size_ms || !offsets_ms || !glue_ms || !pack_ms) return NGZ_E_INVALID;
    *size_ms = o->size_ms;
    *offsets_ms = o->offsets_ms;
    *glue_ms = o->glue_ms;
    *pack_ms = o->pack_ms;
    return NGZ_OK;
}

int ngz_wire_last_launches(ngz_wire *o) { return o ? o->launches : NGZ_E_INVALID; }

}  // extern "C"
