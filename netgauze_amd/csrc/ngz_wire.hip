// The Encoder half of the codec (include/ngz/flow_wire.h): the IPFIX / NetFlow v9 message of every OK
// datagram of a batch, written again from the decoded columns.  The mirror of the staged decode: host-endian
// SoA columns in, big-endian AoS records out, interleaved with message and set headers in stream order.
// The bookkeeping is ngz_msg_stream.h's, shared with ngz_flow_json.hip: the whole output is one byte stream,
// every byte a record's or glue (message head, set header, NFv9 set padding), and the unit of work is a tile,
// at most 64 consecutive records of one data set: consecutive rows of one slot's columns and consecutive
// bytes of the output.  Per encode the host lists every slot's fields as items (column, operation, wire
// length, offset in the record), uploads the plan in one copy, and runs, whatever the number of slots, the
// shared passes (WStream below says what is this stage's in them) around its own, the k_w_ ones:
//   k_dgrams        one thread per datagram: written, not OK, or left to the host for its template sets,
//   k_sets          one thread per data set: its datagram's range of sets; an unwritable template's datagram,
//   k_tiles         one thread per data set: its tiles, ceil(n / 64), if its datagram is written,
//   a hipcub exclusive scan and k_fill: the tile table, and every tile's bytes where the slot's records
//                   have one length (records x rec_len: no pass over rows),
//   k_w_size        only with records of variable-length templates: a wave per such tile, a lane per record
//                   through the counting writer,
//   k_set_len, k_dgram_len, a hipcub exclusive scan: the u64 offsets and the stats,
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

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_wire.h"
#include "ngz_host.h"
#include "ngz_msg_stream.h"
#include "ngz_output_enc.h"

namespace {

using namespace ngzms;
using ngzrow::align256;

constexpr uint32_t W_THREADS = THREADS;
// A wave's record image: 64 records of 256 bytes, and 16 of slack for the output's misalignment
constexpr uint32_t W_IMG = 16384;
constexpr uint32_t C_WIRE = 1, C_TEMPLATE = 2, C_UNWRITABLE = 3, C_NOT_OK = 4;  // ngz_wire_stats' order

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
struct WArgs : Layout {  // passed by value
    const WSlot *slots;
    const WItem *items;
    uint32_t align4;
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
    return ngzms::ld_cell(p, w);
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
// What is this stage's in the shared passes (ngz_msg_stream.h)
struct WStream {
    using Args = WArgs;
    static __device__ __forceinline__ int sets_how(const WSlot &S, const uint8_t &how) { return S.unwritable && how != HOW_NONE ? NGZ_WIRE_UNWRITABLE : -1; }
    // SK_ROWS_VLEN (rec_len 0): k_w_size stores the bytes after this
    static __device__ __forceinline__ void fill_tile(const WArgs &A, const WSlot &S, uint32_t n, uint32_t t, uint32_t first) {
        A.tile_bytes[t] = min(TILE, n - first) * S.rec_len;
    }
    // Header, tiles, padding: the padding is part of the length the header carries
    static __device__ __forceinline__ unsigned long long set_len(const WArgs &A, const ngz_set_info &si, unsigned long long tiles) {
        const unsigned long long len = 4 + tiles;
        return len + set_pad(A.slots[si.slot].proto, A.align4, len);
    }
    static __device__ __forceinline__ unsigned long long dgram_frame(const WArgs &, const ngz_dgram_hdr &h, uint32_t) { return head_len(h); }
    static __device__ __forceinline__ uint32_t counter(const WArgs &, uint32_t, uint8_t how) {  // C_WIRE + this
        return how == HOW_WRITTEN ? 0u : how == HOW_HOST ? 1u : how == NGZ_WIRE_UNWRITABLE ? 2u : 3u;
    }
};

__global__ __launch_bounds__(W_THREADS) void k_w_size(const WArgs A) {
    const uint32_t lane = threadIdx.x & 63u, n_tiles = min(A.tile0[A.n_sets], A.tile_cap);
    uint32_t err = 0;
    for (uint32_t t = blockIdx.x * (W_THREADS / 64u) + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * (W_THREADS / 64u)) {
        const TileRows tr = tile_rows(A, t);
        const WSlot &S = A.slots[tr.si.slot];
        if (S.kind != SK_ROWS_VLEN) continue;
        WCount w;
        if (lane < tr.cnt) put_record(A, S, tr.row0 + lane, w, &err);
        const uint64_t sum = ngzs::wave_sum(w.n);
        if (lane == 0) A.tile_bytes[t] = (uint32_t)sum;
    }
    if (err) atomicOr((unsigned int *)&A.counters[C_ERR], err);
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
        const TileRows tr = tile_rows(A, t);
        const WSlot &S = A.slots[tr.si.slot];
        if (S.kind != SK_FIXED) continue;
        const uint32_t cnt = tr.cnt, rl = S.rec_len;
        const uint32_t rpg = min(TILE, W_IMG / rl);  // records an image holds: rl <= W_IMG
        for (uint32_t g0 = 0; g0 < cnt; g0 += rpg) {
            const uint32_t gc = min(rpg, cnt - g0), len = gc * rl;
            const unsigned long long o = A.tile_off[t] + (unsigned long long)g0 * rl;
            uint8_t *const dst = A.out + o;
            const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
            if (lane < gc) {
                const uint64_t row = (uint64_t)tr.si.rec0 + tr.first + g0 + lane;
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
            if (o + len <= A.total) ngzenc::copy_out(img, mis, dst, len, lane);
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
        const TileRows tr = tile_rows(A, t);
        const WSlot &S = A.slots[tr.si.slot];
        if (S.kind == SK_FIXED) continue;
        const uint32_t row = tr.row0 + lane;
        uint32_t mine = 0;
        if (lane < tr.cnt) {
            if (S.kind == SK_ROWS_VLEN) {
                WCount c;
                put_record(A, S, row, c, &err);
                mine = c.n;
            } else {
                mine = S.rec_len;
            }
        }
        const uint32_t incl = wave_incl_scan(mine);
        ngzenc::pack_tile<W_IMG, WPut, WPut>(lane, tr.cnt, A.tile_off[t], incl - mine, incl, A.out, A.total, img,
                                             [&](auto &w) { put_record(A, S, row, w, &err); });
    }
    if (err) atomicOr((unsigned int *)&A.counters[C_ERR], err);
}

__global__ __launch_bounds__(W_THREADS) void k_w_guard(uint8_t *p, uint32_t n) {
    if (threadIdx.x < n) p[threadIdx.x] = 0xA5;
}

}  // namespace

struct ngz_wire : ngzms::MsgStage {  // its plan in d_in: slots, items
    ngz_wire() : MsgStage("wire") {}
    float glue_ms = 0;
    int align4 = 0;
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
        w->release_device();
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
    o->glue_ms = 0;
    if (int rc = ngzms::begin(o, ctx, out)) return rc;
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
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
        const ngzh::Version *ver;
        if (int rc = ngzms::slot_version(o, ctx, out, s, &ver)) return rc;
        std::string why;
        if (!plan_version(*ver, items, slots[s], &why)) return ngzs::fail(o, NGZ_E_LIMIT, why);
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
    const uint64_t items_at = align256(slots.size() * sizeof(WSlot)), plan_bytes = items_at + align256(items.size() * sizeof(WItem));
    WArgs A{};
    if (int rc = carve(o, ctx, out, hip_stream, plan_bytes, n_records, &A)) return rc;
    uint8_t *h = o->h_in.p;
    if (S) memcpy(h, slots.data(), slots.size() * sizeof(WSlot));
    if (!items.empty()) memcpy(h + items_at, items.data(), items.size() * sizeof(WItem));
    A.slots = (const WSlot *)o->d_in.p;
    A.items = (const WItem *)(o->d_in.p + items_at);
    A.align4 = (uint32_t)o->align4;

    if (int rc = run_tiles<WStream>(o, A)) return rc;
    if (NS && any_vlen) {
        const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)A.tile_cap + 3) / 4, (uint64_t)o->n_cus * 16));
        NGZ_STAGE_HIP(o, o->launch(k_w_size, nb, W_THREADS, A));
    }
    uint32_t n_tiles = 0;
    if (int rc = run_offsets<WStream>(o, A, &n_tiles)) return rc;
    const unsigned long long total = A.total;
    hipStream_t st = o->st;
    NGZ_STAGE_HIP(o, o->launch(k_w_guard, 1u, W_THREADS, A.out + total, (uint32_t)NGZ_OUTPUT_GUARD));
    if (total) {
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
        NGZ_STAGE_HIP(o, o->launch(k_w_glue_dgrams, blocks(D), W_THREADS, A));
        if (NS) NGZ_STAGE_HIP(o, o->launch(k_w_glue_sets, blocks(NS), W_THREADS, A));
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
        if (n_tiles) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)o->n_cus * 32);
            if (any_fixed) NGZ_STAGE_HIP(o, o->launch(k_w_pack_fixed, nb, 64u, A, n_tiles));
            if (any_rows) NGZ_STAGE_HIP(o, o->launch(k_w_pack_rows, nb, 64u, A, n_tiles));
        }
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[3], st));
    }
    if (int rc = read_errors(o)) return rc;
    if (total) {
        NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->glue_ms, o->ev[0], o->ev[1]));
        NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->pack_ms, o->ev[1], o->ev[3]));
    }
    if (int rc = finish(o, D, total)) return rc;
    const unsigned long long *hb = o->h_back.p;
    if (stats) *stats = ngz_wire_stats{hb[C_WIRE], total, hb[C_TEMPLATE], hb[C_UNWRITABLE], hb[C_NOT_OK]};
    return NGZ_OK;
}

int ngz_wire_result(ngz_wire *o, const uint8_t **bytes, const uint64_t **offsets, const uint8_t **how, uint64_t *n_dgrams, uint64_t *n_bytes) {
    return ngzms::result(o, bytes, offsets, how, n_dgrams, n_bytes);
}

int ngz_wire_to_host(ngz_wire *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap, uint8_t *how, uint64_t how_cap) {
    return ngzms::to_host(o, bytes, bytes_cap, offsets, offsets_cap, how, how_cap);
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
