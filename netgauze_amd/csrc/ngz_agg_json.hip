// serde JSON of aggregated flow groups (include/ngz/flow_agg_json.h): the text ngz_agg_flowinfo_json
// (ngz_json.cpp, the specification) gives for each row of a flush / emit, rendered on the device.  Per
// encode and on the host this unit lists the group's fields as items (presence test, loader by row
// storage, renderer, constant prefix and suffix text in a dword-padded pool), uploads plan, rows, tails
// and peers in one copy, and runs
//   k_agg_json_size  a wave stages its tile of consecutive rows into LDS (coalesced 16-byte loads), each
//                    lane renders its own row through a counting writer; four lengths per 16-byte store,
//   a hipcub exclusive scan: the u64 offsets,
//   k_agg_json_pack  the same staging, then each lane renders its row into the wave's LDS image through
//                    JAcc: a 64-bit accumulator that takes rendered characters up to four at a time and
//                    constant text a dword at a time, funnel-shifted by the writer's byte phase, and
//                    stores aligned dwords; only a row's first and last partial dword, which it shares
//                    with its neighbours, are stored by bytes.  The image is laid out like the output
//                    range and goes out in 16-byte stores (pack_tile, ngz_output_enc.h); a line longer
//                    than the image goes straight out through the byte writer.
// One set of renderers, templated on the writer, serves both passes: the sizes are the packed bytes by
// construction.  Both kernels have a second instantiation (FLT) whose renderer knows float64 (put_f64,
// ngz_f64_dev.h), launched in their place when the plan has a float item (NGZ_AGG_JSON_OPT_FLOATS): a layout
// without floats runs the kernels it ran before.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_agg_json.h"
#include "ngz_agg_rows.h"
#include "ngz_host.h"
#include "ngz_f64_dev.h"
#include "ngz_json_dev.h"
#include "ngz_output_enc.h"
#include "ngz_stage.h"

namespace {

using namespace ngzrow;
using namespace ngzjson;  // the writers and value renderers, shared with ngz_flow_json.hip

constexpr uint32_t JS_THREADS = 64;  // one wave per block: LDS, not threads, bounds what a CU holds
constexpr uint32_t JS_STAGE_SMALL = 64 * (128 + AO_PAD), JS_STAGE_LARGE = 64 * (256 + AO_PAD);
// A wave's image, and 16 of slack for the output's misalignment.  A line is several hundred bytes, so
// the image is what decides how many lanes render at once: 30 KB holds some thirty lines of 1 KB; with
// the 8.25 KB stage a block takes 38.25 KB and four blocks fit the CU's 160 KB.
constexpr uint32_t JS_IMG = 30704;
constexpr uint32_t JS_MAX_ITEMS = 64;  // 16 keys, 32 values, 11 extras
constexpr uint32_t ERR_PEER = 1, ERR_TAIL = 2;

enum : uint8_t { P_KEY, P_VAL, P_ALWAYS, P_PEER4, P_PEER6, P_PORTS, P_DOMAINS, P_TEMPLATES };  // an item's presence test
enum : uint8_t { L_INT, L_PTR, L_STRZ, L_BVAL, L_WSTART, L_WEND, L_PEER4, L_PEER6, L_MEMBER };  // how its value is read
enum : uint8_t {  // put_value of ngz_json.cpp, case by case
    RD_NULL, RD_U64, RD_I64, RD_BOOL, RD_IP4, RD_IP6, RD_LIST, RD_STR, RD_DT_SECS, RD_DT_MS, RD_DT_FRAC_KEY, RD_DT_FRAC_VAL,
    RD_TCP, RD_SUBREG, RD_SUBREG_NESTED, RD_F64
};
enum { T_V10_A, T_V10_B, T_V9_A, T_V9_B, T_V9_C, T_TAIL, T_UNASSIGNED, T_COUNT };

struct JItem {
    uint8_t pres, bit, load, rend;
    uint16_t off, width;  // row offset; bytes of an integer or of fixed bytes
    JText pre, suf;       // the field's tag around its value
    JSub sub;             // RD_SUBREG*: its variants in the name table; RD_SUBREG_NESTED: its groups
};
// One encode's plan, in device memory (uploaded with the rows): every lane reads it uniformly
struct JPlan {
    JItem items[JS_MAX_ITEMS];
    JText fixed[T_COUNT];
    SetEntry ports[NGZ_AGG_SET_BITS], templates[NGZ_AGG_SET_BITS], domains[2 * NGZ_AGG_SET_BITS];  // ascending by value
    uint32_t n_ports, n_templates, n_domains;
    uint32_t n_items;
    unsigned long long window_ms;
};
struct JArgs {  // passed by value
    const JPlan *plan;
    const JName *names;
    const uint32_t *pool;
    const uint8_t *rows;   // n_rows x row_bytes, 16-byte aligned
    const uint8_t *arena;  // the byte values longer than a row holds, whole, at 8-byte offsets
    unsigned long long arena_size;
    const ngz_peer *peers;
    uint32_t n_peers, n_rows, row_bytes, tile, seq0;
    uint32_t *lens;
    const unsigned long long *offs;
    uint8_t *out;
    unsigned long long total;
    unsigned int *err;
};

struct JCell {
    uint64_t v;        // an integer, zero-extended
    const uint8_t *p;  // any other value's bytes
    uint32_t n;
};

// The value of item `it` (member m of a set) of row R
__device__ __forceinline__ void load_value(const JPlan &P, const JArgs &A, const uint8_t *R, const JItem &it, uint32_t member, JCell &c,
                                           uint32_t *err) {
    c = JCell{0, R, 0};
    const uint8_t *p = R + it.off;
    switch (it.load) {
    case L_INT: c.v = ld_le(p, it.width); break;
    case L_PTR:
        c.p = p;
        c.n = it.width;
        break;
    case L_STRZ: {  // a fixed string ends at its first NUL
        uint32_t n = 0;
        while (n < it.width && p[n]) ++n;
        c.p = p;
        c.n = n;
        break;
    }
    case L_BVAL: {  // {u32 length, u32 offset / 8 into the arena, the first 32 bytes}
        const uint32_t len = *(const uint32_t *)p;
        const uint64_t at = (uint64_t) * (const uint32_t *)(p + 4) << 3;
        if (len <= BVAL_INLINE) {
            c.p = p + 8;
            c.n = len;
        } else if (at + len <= A.arena_size) {
            c.p = A.arena + at;
            c.n = len;
        } else {
            *err |= ERR_TAIL;
        }
        break;
    }
    case L_WSTART: c.v = ld_le(R + R_WINDOW, 4) * 1000ull; break;
    case L_WEND: c.v = ld_le(R + R_WINDOW, 4) * 1000ull + P.window_ms; break;  // actor.rs:222-240
    case L_PEER4: {
        const uint8_t *a = A.peers[ld_le(R + R_PEER, 2)].addr;  // the index was checked by peer_family
        c.v = ((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3];
        break;
    }
    case L_PEER6:
        c.p = A.peers[ld_le(R + R_PEER, 2)].addr;
        c.n = 16;
        break;
    default: c.v = member; break;  // L_MEMBER
    }
}

template <bool FLT, class W>
__device__ __forceinline__ void render_value(W &w, const JPlan &P, const JArgs &A, const JItem &it, const JCell &c) {
    if constexpr (FLT) {  // outside the switch: without FLT this function is what it was
        if (it.rend == RD_F64) {  // the aggregator's f64 value class and a float64 key cell: the bits, L_INT at 8 bytes
            put_f64(w, c.v);
            return;
        }
    }
    switch (it.rend) {
    case RD_U64: put_dec(w, c.v); break;
    case RD_I64: {
        const int shift = 64 - 8 * (int)it.width;
        const int64_t sv = (int64_t)(c.v << shift) >> shift;
        if (sv < 0) w.push('-', 1);
        put_dec(w, sv < 0 ? 0ull - (uint64_t)sv : (uint64_t)sv);
        break;
    }
    case RD_BOOL: put_bool(w, (c.v & 255u) != 0); break;
    case RD_IP4: put_ip4_str(w, c.v); break;
    case RD_IP6: put_ip6_str(w, c.p); break;
    case RD_LIST: put_list(w, c.p, c.n); break;
    case RD_STR: put_str(w, c.p, c.n); break;
    case RD_DT_SECS: put_datetime(w, (int64_t)c.v, 0); break;
    case RD_DT_MS: {
        const int64_t ms = (int64_t)c.v, secs = floor_div(ms, 1000);
        put_datetime(w, secs, (uint32_t)(ms - secs * 1000) * 1000000u);
        break;
    }
    case RD_DT_FRAC_KEY: put_datetime(w, (int64_t)(uint32_t)c.v, (uint32_t)(c.v >> 32)); break;  // {u32 secs, u32 nanos}
    case RD_DT_FRAC_VAL: put_datetime(w, (int64_t)(c.v >> 32), (uint32_t)c.v); break;            // secs << 32 | nanos
    case RD_TCP: put_tcp(w, (uint32_t)c.v & 255u); break;
    case RD_SUBREG:
    case RD_SUBREG_NESTED: put_subreg(w, A.names, A.pool, P.fixed[T_UNASSIGNED], it.sub, it.rend == RD_SUBREG_NESTED, c.v); break;
    default: w.push('n' | ('u' << 8) | ('l' << 16) | ('l' << 24), 4); break;
    }
}

// The peer's address family, 0 for an index outside the peers (sets ERR_PEER)
__device__ __forceinline__ uint32_t peer_family(const JArgs &A, const uint8_t *R, uint32_t *err) {
    const uint32_t pi = (uint32_t)ld_le(R + R_PEER, 2);
    if (pi >= A.n_peers) {
        *err |= ERR_PEER;
        return 0;
    }
    return A.peers[pi].family;
}

// Row g's line: the head by the flow type, the present items, the closing text
template <bool FLT, class W>
__device__ __forceinline__ void render_row(const JPlan &P, const JArgs &A, const uint8_t *R, uint32_t g, W &w, uint32_t *err) {
    auto fixed = [&](int t) { w.text(A.pool + P.fixed[t].off / 4u, P.fixed[t].len); };
    if (R[R_FLOW_TYPE] == 10) {
        fixed(T_V10_A);
        put_dec(w, (uint32_t)(A.seq0 + g));
        fixed(T_V10_B);
    } else {
        fixed(T_V9_A);
        put_dec(w, (uint32_t)ld_le(R + R_SYS_UP, 4));
        fixed(T_V9_B);
        put_dec(w, (uint32_t)(A.seq0 + g));
        fixed(T_V9_C);
    }
    bool first = true;
    JCell c;
    auto field = [&](const JItem &it, uint32_t member) {
        load_value(P, A, R, it, member, c, err);
        if (!first) w.push(',', 1);
        first = false;
        w.text(A.pool + it.pre.off / 4u, it.pre.len);
        render_value<FLT>(w, P, A, it, c);
        w.text(A.pool + it.suf.off / 4u, it.suf.len);
    };
    for (uint32_t i = 0; i < P.n_items; ++i) {
        const JItem &it = P.items[i];
        if (it.pres == P_PORTS || it.pres == P_DOMAINS || it.pres == P_TEMPLATES) {
            const SetEntry *e = it.pres == P_PORTS ? P.ports : it.pres == P_DOMAINS ? P.domains : P.templates;
            const uint32_t n = it.pres == P_PORTS ? P.n_ports : it.pres == P_DOMAINS ? P.n_domains : P.n_templates;
            const uint8_t *bits = R + (it.pres == P_PORTS ? R_PORTS : it.pres == P_DOMAINS ? R_DOMAINS : R_TEMPLATES);
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t b = e[j].bit;
                if ((*(const uint32_t *)(bits + 4u * (b >> 5)) >> (b & 31u)) & 1u) field(it, e[j].value);
            }
            continue;
        }
        bool present = true;
        if (it.pres == P_KEY) present = (ld_le(R + R_KEYP, 4) >> it.bit) & 1u;
        else if (it.pres == P_VAL) present = (ld_le(R + R_VALP, 4) >> it.bit) & 1u;
        else if (it.pres == P_PEER4) present = peer_family(A, R, err) == 4;
        else if (it.pres == P_PEER6) present = peer_family(A, R, err) == 6;
        if (present) field(it, 0);
    }
    fixed(T_TAIL);
    w.finish();
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
template <uint32_t STAGE, bool FLT>
__global__ __launch_bounds__(JS_THREADS) void k_agg_json_size(const JArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    const uint32_t lane = threadIdx.x, T = A.tile;
    const uint32_t tiles = (A.n_rows + T - 1) / T;
    const JPlan &P = *A.plan;
    uint32_t err = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.lens[(A.n_rows + 3u) & ~3u] = 0;  // the scan's last item
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row0 = tile * T, nt = min(T, A.n_rows - row0);
        stage_rows(A.rows, A.row_bytes, row0, nt, stage, lane);
        JCount w;
        if (lane < nt) render_row<FLT>(P, A, stage + lane * (A.row_bytes + AO_PAD), row0 + lane, w, &err);
        // four lengths per 16-byte store: T and row0 are multiples of four, rows past n_rows count 0
        const uint32_t n1 = __shfl_down(w.n, 1, 64), n2 = __shfl_down(w.n, 2, 64), n3 = __shfl_down(w.n, 3, 64);
        if (!(lane & 3u) && lane < nt) *(uint4 *)(A.lens + row0 + lane) = make_uint4(w.n, n1, n2, n3);
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();  // the stage is rewritten by the next tile
    }
    if (err) atomicOr(A.err, err);
}

template <uint32_t STAGE, class WImg, bool FLT>
__global__ __launch_bounds__(JS_THREADS) void k_agg_json_pack(const JArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t img[JS_IMG + 16];  // pack_tile's
    const uint32_t lane = threadIdx.x, T = A.tile;
    const uint32_t tiles = (A.n_rows + T - 1) / T;
    const JPlan &P = *A.plan;
    uint32_t err = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row0 = tile * T, nt = min(T, A.n_rows - row0);
        stage_rows(A.rows, A.row_bytes, row0, nt, stage, lane);
        const uint8_t *const R = stage + lane * (A.row_bytes + AO_PAD);
        const unsigned long long a = A.offs[lane < nt ? row0 + lane : A.n_rows], b = lane < nt ? A.offs[row0 + lane + 1] : a;
        const unsigned long long base = __shfl(a, 0, 64);
        const uint32_t rel0 = (uint32_t)(a - base), rel1 = (uint32_t)(b - base);
        ngzenc::pack_tile<JS_IMG, WImg, JByte>(lane, nt, base, rel0, rel1, A.out, A.total, img,
                                               [&](auto &w) { render_row<FLT>(P, A, R, row0 + lane, w, &err); });
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();  // the stage is rewritten by the next tile
    }
    if (err) atomicOr(A.err, err);
}

struct ToU64 {
    __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t v) const { return v; }
};
using LenIter = hipcub::TransformInputIterator<unsigned long long, ToU64, const uint32_t *>;

// The two kernels of a row size, a writer and a renderer set
template <bool FLT>
void (*size_kernel(bool small))(const JArgs) {
    return small ? k_agg_json_size<JS_STAGE_SMALL, FLT> : k_agg_json_size<JS_STAGE_LARGE, FLT>;
}
template <bool FLT>
void (*pack_kernel(bool small, bool bytes))(const JArgs) {
    return bytes ? (small ? k_agg_json_pack<JS_STAGE_SMALL, JByte, FLT> : k_agg_json_pack<JS_STAGE_LARGE, JByte, FLT>)
                 : (small ? k_agg_json_pack<JS_STAGE_SMALL, JAcc, FLT> : k_agg_json_pack<JS_STAGE_LARGE, JAcc, FLT>);
}

}  // namespace

struct ngz_agg_json : ngzs::Stage {
    ngz_agg_json() : Stage(4) {}
    int writer = 0;       // NGZ_AGG_JSON_OPT_WRITER
    bool floats = false;  // NGZ_AGG_JSON_OPT_FLOATS
    float upload_ms = 0, size_ms = 0, pack_ms = 0;
    int launches = 0;
    uint64_t n_rows = 0, n_bytes = 0;  // the last encode
    bool have = false;
    ngzh::DevBuf<uint8_t> d_in, d_bytes, d_scan_tmp;  // d_in: plan, names, pool, rows, arena, peers
    ngzh::DevBuf<uint32_t> d_lens, d_err;
    ngzh::DevBuf<unsigned long long> d_offs;
    ngzs::PinnedBuf<uint8_t> h_in;
    ngzs::PinnedBuf<unsigned long long> h_back;  // error bits, the total
};

namespace {

using ngzh::Spec;

Spec spec_of(uint32_t pen, uint16_t id) {  // as ngz_json.cpp's
    Spec s{};
    s.pen = pen;
    s.id = id;
    s.kind = ngzh::IK_UNKNOWN;
    s.dtype = ngzh::DT_octetArray;
    const ngzh::IeRow *r = ngzh::ie_find(pen, id);
    s.vendor = pen ? ngzh::vendor_name(pen) : nullptr;
    if (pen && !s.vendor) return s;
    if (r) {
        s.kind = pen ? ngzh::IK_VENDOR : ngzh::IK_IANA;
        s.dtype = r->dtype;
        s.flags = r->flags;
        s.name = r->name;
    } else if (pen) {
        s.kind = ngzh::IK_VENDOR_UNKNOWN;
    }
    return s;
}

std::string ie_label(const Spec &s) {
    return s.name ? std::string(s.name) : "pen " + std::to_string(s.pen) + " id " + std::to_string(s.id);
}

void tag_text(const Spec &s, Pool &pool, JItem *it) {
    std::string pre, suf;
    ngzjson::tag_text(s, &pre, &suf);
    it->pre = pool.add(pre);
    it->suf = pool.add(suf);
}

// put_value's choice for a cell of column kind `kind`, `width` bytes wide; false: an integer storage the
// loader cannot read
bool pick(const Spec &s, uint8_t kind, uint16_t width, Pool &pool, std::vector<JName> &names, JItem *it) {
    const bool known = s.kind == ngzh::IK_IANA || s.kind == ngzh::IK_VENDOR;
    const bool int_w = width == 1 || width == 2 || width == 4 || width == 8;
    it->load = L_INT;
    it->width = width;
    it->rend = RD_NULL;
    switch (kind) {
    case NGZ_K_UINT:
        it->rend = RD_U64;
        if (known && (s.flags & 4)) {
            if (const int sk = add_subreg(s.pen, s.id, pool, names, &it->sub)) {
                it->rend = sk == 2 ? RD_SUBREG_NESTED : RD_SUBREG;
                return int_w;
            }
        }
        if (known && s.dtype == ngzh::DT_ipv4Address) it->rend = RD_IP4;
        if (known && s.dtype == ngzh::DT_dateTimeSeconds) it->rend = RD_DT_SECS;
        return int_w;
    case NGZ_K_SCOPE32:
        it->rend = RD_U64;
        it->width = 4;
        return true;
    case NGZ_K_TCPFLAGS: it->rend = RD_TCP; it->width = 1; return true;
    case NGZ_K_SINT: it->rend = RD_I64; return int_w;
    case NGZ_K_BOOL: it->rend = RD_BOOL; it->width = 1; return true;
    case NGZ_K_BYTES:
        it->load = L_PTR;
        it->rend = known && s.dtype == ngzh::DT_ipv6Address && width == 16 ? RD_IP6 : RD_LIST;
        return true;
    case NGZ_K_U256:
        it->load = L_PTR;
        it->width = 32;
        it->rend = RD_LIST;
        return true;
    case NGZ_K_DTMS: it->rend = RD_DT_MS; it->width = 8; return true;
    case NGZ_K_DTFRAC: it->rend = RD_DT_FRAC_KEY; it->width = 8; return true;
    case NGZ_K_STR:
        it->load = L_STRZ;
        it->rend = RD_STR;
        return true;
    }
    return true;  // a kind no record has given yet (no row has the bit), or one put_value prints as null
}

}  // namespace

extern "C" {

int ngz_agg_json_abi_version(void) { return NGZ_AGG_JSON_ABI_VERSION; }

int ngz_agg_json_create(int device, ngz_agg_json **out) {
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0) return NGZ_E_INVALID;
    ngz_agg_json *j = new ngz_agg_json;
    j->device = device;
    *out = j;
    return NGZ_OK;
}

void ngz_agg_json_destroy(ngz_agg_json *j) {
    if (!j) return;
    if (j->device_ready) {
        hipSetDevice(j->device);
        j->d_in.release();
        j->d_bytes.release();
        j->d_scan_tmp.release();
        j->d_lens.release();
        j->d_err.release();
        j->d_offs.release();
    }
    delete j;
}

const char *ngz_agg_json_last_error(ngz_agg_json *j) { return j ? j->last_error.c_str() : "null aggregated JSON stage"; }

int ngz_agg_json_set_option(ngz_agg_json *j, int opt, int64_t value) {
    if (!j) return NGZ_E_INVALID;
    if ((opt != NGZ_AGG_JSON_OPT_WRITER && opt != NGZ_AGG_JSON_OPT_FLOATS) || (value != 0 && value != 1))
        return ngzs::fail(j, NGZ_E_INVALID, "unknown option or value");
    if (opt == NGZ_AGG_JSON_OPT_WRITER) j->writer = (int)value;
    else j->floats = value != 0;
    return NGZ_OK;
}

int ngz_agg_json_encode(ngz_agg_json *o, ngz_agg *agg, const void *rows, uint64_t n_rows, uint32_t shard_id, uint32_t seq0,
                        int64_t export_time_ms, ngz_agg_json_stats *stats, void *hip_stream) {
    if (!o || !agg || (n_rows && !rows)) return NGZ_E_INVALID;
    if (stats) memset(stats, 0, sizeof *stats);
    o->have = false;
    o->n_rows = o->n_bytes = 0;
    o->launches = 0;
    o->upload_ms = o->size_ms = o->pack_ms = 0;
    if (n_rows >> 31) return ngzs::fail(o, NGZ_E_LIMIT, "more than 2^31 rows");

    // the row layout, through the aggregator's ABI
    const std::vector<ngz_agg_field> &keys = ngzh::agg_keys(agg), &vals = ngzh::agg_vals(agg);
    const uint32_t nk = (uint32_t)keys.size(), nv = (uint32_t)vals.size();
    uint32_t rb = 0;
    std::vector<uint32_t> ko(nk + 1), vo(nv + 1);
    std::vector<uint16_t> kw(nk + 1), vw(nv + 1);
    if (ngz_agg_layout(agg, &rb, ko.data(), kw.data(), vo.data(), vw.data())) return ngzs::fail(o, NGZ_E_INVALID, "ngz_agg_layout");
    if (!rb || rb % 128 || rb > 0xFFFF) return ngzs::fail(o, NGZ_E_LIMIT, "unexpected row size");
    std::vector<ngz_agg_key_desc> kd(nk);
    std::vector<ngz_agg_value_desc> vd(nv);
    for (uint32_t k = 0; k < nk; ++k) ngz_agg_key_info(agg, k, &kd[k]);
    for (uint32_t v = 0; v < nv; ++v) ngz_agg_value_info(agg, v, &vd[v]);

    // the plan: the group's field list as items (ngz_json.cpp:656-762)
    std::vector<uint8_t> plan_mem(sizeof(JPlan), 0);
    JPlan &P = *(JPlan *)plan_mem.data();
    Pool pool;
    std::vector<JName> names;
    uint32_t ni = 0;
    bool use_float = false;  // the plan has a float item: the kernels' float instantiation
    auto item = [&](uint32_t pen, uint16_t ie, uint8_t pres, uint32_t bit, uint32_t off, uint8_t kind, uint16_t width, int bval,
                    int load) -> int {
        if (ni == JS_MAX_ITEMS) return ngzs::fail(o, NGZ_E_LIMIT, "more than 64 fields in a group's record");
        const Spec s = spec_of(pen, ie);
        const bool known = s.kind == ngzh::IK_IANA || s.kind == ngzh::IK_VENDOR;
        const bool is_float = (pres == P_KEY || pres == P_VAL) && known && (s.dtype == ngzh::DT_float32 || s.dtype == ngzh::DT_float64);
        const bool f64 = is_float && o->floats && s.dtype == ngzh::DT_float64;
        if (is_float && !f64)
            return ngzs::fail(o, NGZ_OUTPUT_E_UNSUPPORTED,
                              "field " + ie_label(s) + ": float text is not rendered on the device (ngz_agg_flowinfo_json renders it)");
        JItem it{};
        it.pres = pres;
        it.bit = (uint8_t)bit;
        it.off = (uint16_t)off;
        if (bval) {  // put_bytes: a byte value of any length, string text or the bytes as a list
            it.load = L_BVAL;
            it.rend = s.dtype == ngzh::DT_string ? RD_STR : RD_LIST;
        } else if (!pick(s, kind, width, pool, names, &it)) {
            return ngzs::fail(o, NGZ_E_LIMIT, "field " + ie_label(s) + ": an integer storage that is not 1, 2, 4 or 8 bytes wide");
        }
        if (load >= 0) it.load = (uint8_t)load;
        if (f64) {  // the bits as the row stores them: the f64 value class, or a key's 8-byte column cell
            if (it.load != L_INT || it.width != 8)
                return ngzs::fail(o, NGZ_E_LIMIT, "field " + ie_label(s) + ": a float64 storage that is not 8 bytes wide");
            it.rend = RD_F64;
            use_float = true;
        }
        tag_text(s, pool, &it);
        P.items[ni++] = it;
        return NGZ_OK;
    };
    for (uint32_t k = 0; k < nk; ++k)
        if (int rc = item(keys[k].pen, keys[k].ie_id, P_KEY, k, ko[k], kd[k].kind, kd[k].width, kd[k].kkind == 3, -1)) return rc;
    for (uint32_t v = 0; v < nv; ++v) {
        int rc;
        switch (vd[v].vclass) {
        case 2:  // secs << 32 | nanos
            rc = item(vals[v].pen, vals[v].ie_id, P_VAL, v, vo[v], NGZ_K_DTFRAC, 8, 0, -1);
            if (!rc) P.items[ni - 1].rend = RD_DT_FRAC_VAL;
            break;
        case 5: rc = item(vals[v].pen, vals[v].ie_id, P_VAL, v, vo[v], NGZ_K_UINT, 4, 0, -1); break;
        case 6: rc = item(vals[v].pen, vals[v].ie_id, P_VAL, v, vo[v], NGZ_K_UINT, 8, 0, -1); break;
        case 7: rc = item(vals[v].pen, vals[v].ie_id, P_VAL, v, vo[v], NGZ_K_BYTES, 16, 0, -1); break;
        case 8: case 9: rc = item(vals[v].pen, vals[v].ie_id, P_VAL, v, vo[v], 0, 0, 1, -1); break;
        default: rc = item(vals[v].pen, vals[v].ie_id, P_VAL, v, vo[v], vd[v].kind, vd[v].width, 0, -1); break;
        }
        if (rc) return rc;
    }
    {
        int rc = item(0, 375, P_ALWAYS, 0, R_COUNT, NGZ_K_UINT, 8, 0, -1);                               // originalFlowsPresent
        if (!rc) rc = item(0, 264, P_ALWAYS, 0, R_MIN_EXPORT, NGZ_K_UINT, 4, 0, -1);                     // minExportSeconds
        if (!rc) rc = item(0, 260, P_ALWAYS, 0, R_MAX_EXPORT, NGZ_K_UINT, 4, 0, -1);                     // maxExportSeconds
        if (!rc) rc = item(0, 258, P_ALWAYS, 0, R_MAX_COLL, NGZ_K_DTMS, 8, 0, -1);                       // collectionTimeMilliseconds
        if (!rc) rc = item(3746, 1, P_ALWAYS, 0, R_WINDOW, NGZ_K_DTMS, 8, 0, L_WSTART);                  // NetGauze windowStart
        if (!rc) rc = item(3746, 2, P_ALWAYS, 0, R_WINDOW, NGZ_K_DTMS, 8, 0, L_WEND);                    // NetGauze windowEnd
        if (!rc) rc = item(0, 403, P_PEER4, 0, 0, NGZ_K_UINT, 4, 0, L_PEER4);                            // originalExporterIPv4Address
        if (!rc) rc = item(0, 404, P_PEER6, 0, 0, NGZ_K_BYTES, 16, 0, L_PEER6);                          // originalExporterIPv6Address
        if (!rc) rc = item(3746, 4, P_PORTS, 0, 0, NGZ_K_UINT, 2, 0, L_MEMBER);                          // NetGauze originalExporterTransportPort
        if (!rc) rc = item(0, 405, P_DOMAINS, 0, 0, NGZ_K_UINT, 4, 0, L_MEMBER);                         // originalObservationDomainId
        if (!rc) rc = item(3746, 3, P_TEMPLATES, 0, 0, NGZ_K_UINT, 2, 0, L_MEMBER);                      // NetGauze originalTemplateId
        if (rc) return rc;
    }
    if (names.size() > NGZ_AGG_JSON_MAX_NAMES) return ngzs::fail(o, NGZ_E_LIMIT, "more sub-registry variants than NGZ_AGG_JSON_MAX_NAMES");
    P.n_items = ni;
    P.window_ms = ngzh::agg_window_ms(agg);
    {  // the head and tail texts of both flow types, the export time rendered once
        JHost t;
        const int64_t es = floor_div(export_time_ms, 1000);
        put_datetime(t, es, (uint32_t)(export_time_ms - es * 1000) * 1000000u);
        const std::string sets = ",\"sets\":[{\"Data\":{\"id\":65535,\"records\":[{\"scope_fields\":[],\"fields\":[";
        P.fixed[T_V10_A] = pool.add("{\"IPFIX\":{\"version\":10,\"export_time\":" + t.s + ",\"sequence_number\":");
        P.fixed[T_V10_B] = pool.add(",\"observation_domain_id\":" + std::to_string(shard_id) + sets);
        P.fixed[T_V9_A] = pool.add("{\"NetFlowV9\":{\"version\":9,\"sys_up_time\":");
        P.fixed[T_V9_B] = pool.add(",\"unix_time\":" + t.s + ",\"sequence_number\":");
        P.fixed[T_V9_C] = pool.add(",\"source_id\":" + std::to_string(shard_id) + sets);
        P.fixed[T_TAIL] = pool.add("]}]}}]}}");
        P.fixed[T_UNASSIGNED] = pool.add("{\"Unassigned\":");
        pool.b.resize(pool.b.size() + 4, 0);
    }
    {  // the dictionaries of the last flush / emit (entry i <-> bit i, -1 free), each sorted once
        const std::vector<int64_t> *dt, *dp, *dd;
        ngzh::agg_out_dicts(agg, &dt, &dp, &dd);
        P.n_templates = sorted_set(*dt, 0xFFFFu, P.templates, NGZ_AGG_SET_BITS);
        P.n_ports = sorted_set(*dp, 0xFFFFu, P.ports, NGZ_AGG_SET_BITS);
        P.n_domains = sorted_set(*dd, 0xFFFFFFFFu, P.domains, 2 * NGZ_AGG_SET_BITS);
    }
    if (!n_rows) {  // no row: no kernel
        o->have = true;
        return NGZ_OK;
    }
    std::vector<ngz_peer> peers;
    {
        ngz_peer pe;
        const int np = ngz_agg_peer(agg, 0, &pe);
        for (int i = 0; i < np; ++i) {
            ngz_agg_peer(agg, (uint32_t)i, &pe);
            peers.push_back(pe);
        }
    }

    // rows: one take, known peers; the byte values longer than a row holds fetched whole
    struct ByteField {
        int is_value;
        uint32_t index, off, bit_off;
    };
    std::vector<ByteField> bf;
    for (uint32_t k = 0; k < nk; ++k)
        if (kd[k].kkind == 3) bf.push_back(ByteField{0, k, ko[k], R_KEYP});
    for (uint32_t v = 0; v < nv; ++v)
        if (vd[v].vclass == 8 || vd[v].vclass == 9) bf.push_back(ByteField{1, v, vo[v], R_VALP});
    const uint8_t *src = (const uint8_t *)rows;
    uint32_t take0;
    memcpy(&take0, src + R_TAKE, 4);
    if (!take0 || (!bf.empty() && ngz_agg_row_bytes(agg, src, bf[0].is_value, bf[0].index, nullptr, 0) < 0))
        return ngzs::fail(o, NGZ_E_INVALID, "rows of an earlier flush / emit");
    uint64_t arena_bytes = 0;
    for (uint64_t g = 0; g < n_rows; ++g) {
        const uint8_t *R = src + g * rb;
        uint32_t take;
        uint16_t pi;
        memcpy(&take, R + R_TAKE, 4);
        memcpy(&pi, R + R_PEER, 2);
        if (take != take0) return ngzs::fail(o, NGZ_E_INVALID, "rows of different flush / emit calls");
        if (pi >= peers.size()) return ngzs::fail(o, NGZ_E_INVALID, "a row whose peer the aggregator's last flush / emit does not know");
        for (const ByteField &b : bf) {
            uint32_t present, len;
            memcpy(&present, R + b.bit_off, 4);
            memcpy(&len, R + b.off, 4);
            if (((present >> b.index) & 1u) && len > BVAL_INLINE) arena_bytes += ((uint64_t)len + 7) & ~7ull;
        }
    }
    if (arena_bytes >> 34) return ngzs::fail(o, NGZ_E_LIMIT, "more than 16 GiB of long byte values");
    const uint64_t rows_bytes = n_rows * rb;
    const uint64_t names_at = align256(sizeof(JPlan)), pool_at = names_at + align256(names.size() * sizeof(JName));
    const uint64_t rows_at = pool_at + align256(pool.b.size()), arena_at = rows_at + align256(rows_bytes);
    const uint64_t peers_at = arena_at + align256(arena_bytes), in_bytes = peers_at + align256(peers.size() * sizeof(ngz_peer));
    if (int rc = ngzs::device_init(o)) return rc;
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    if (o->h_in.reserve(in_bytes)) return ngzs::fail(o, NGZ_E_NOMEM, "aggregated JSON staging");
    uint8_t *h = o->h_in.p;
    memcpy(h, plan_mem.data(), sizeof(JPlan));
    if (!names.empty()) memcpy(h + names_at, names.data(), names.size() * sizeof(JName));
    memcpy(h + pool_at, pool.b.data(), pool.b.size());
    memcpy(h + rows_at, src, rows_bytes);
    memcpy(h + peers_at, peers.data(), peers.size() * sizeof(ngz_peer));
    if (arena_bytes) {
        uint64_t at = 0;
        for (uint64_t g = 0; g < n_rows; ++g) {
            const uint8_t *R = src + g * rb;
            for (const ByteField &b : bf) {
                uint32_t present, len;
                memcpy(&present, R + b.bit_off, 4);
                memcpy(&len, R + b.off, 4);
                if (!((present >> b.index) & 1u) || len <= BVAL_INLINE) continue;
                if (ngz_agg_row_bytes(agg, R, b.is_value, b.index, h + arena_at + at, len) != (int64_t)len)
                    return ngzs::fail(o, NGZ_E_INVALID, "rows of an earlier flush / emit");
                const uint32_t at8 = (uint32_t)(at >> 3);
                memcpy(h + rows_at + g * rb + b.off + 4, &at8, 4);  // the uploaded row points into the arena
                at += ((uint64_t)len + 7) & ~7ull;
            }
        }
    }

    hipStream_t st = (hipStream_t)hip_stream;
    const uint32_t tile = rb <= 256 ? 64u : (JS_STAGE_LARGE / (rb + AO_PAD)) & ~3u;
    if (!tile) return ngzs::fail(o, NGZ_E_LIMIT, "rows too long to stage");
    const uint64_t n_lens = ((n_rows + 3) & ~3ull) + 4;
    size_t scan_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, LenIter((const uint32_t *)nullptr, ToU64()), (unsigned long long *)nullptr,
                                         (int)(n_rows + 1), st) != hipSuccess)
        return ngzs::fail(o, NGZ_E_DEVICE, "scan temp size");
    if (o->d_in.ensure(in_bytes) || o->d_lens.ensure(n_lens) || o->d_offs.ensure(n_rows + 2) || o->d_err.ensure(4) ||
        o->d_scan_tmp.ensure(scan_bytes + 1) || o->h_back.reserve(2))
        return ngzs::fail(o, NGZ_E_NOMEM, "aggregated JSON buffers");
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->d_in.p, h, in_bytes, hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_err.p, 0, sizeof(uint32_t), st));
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
    JArgs A{};
    A.plan = (const JPlan *)o->d_in.p;
    A.names = (const JName *)(o->d_in.p + names_at);
    A.pool = (const uint32_t *)(o->d_in.p + pool_at);
    A.rows = o->d_in.p + rows_at;
    A.arena = o->d_in.p + arena_at;
    A.arena_size = arena_bytes;
    A.peers = (const ngz_peer *)(o->d_in.p + peers_at);
    A.n_peers = (uint32_t)peers.size();
    A.n_rows = (uint32_t)n_rows;
    A.row_bytes = rb;
    A.tile = tile;
    A.seq0 = seq0;
    A.lens = o->d_lens.p;
    A.offs = o->d_offs.p;
    A.err = o->d_err.p;
    const uint64_t tiles = (n_rows + tile - 1) / tile;
    const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)o->n_cus * 16));
    const bool small = rb == 128;
    hipLaunchKernelGGL(use_float ? size_kernel<true>(small) : size_kernel<false>(small), dim3(nb), dim3(JS_THREADS), 0, st, A);
    NGZ_STAGE_HIP(o, hipGetLastError());
    NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, scan_bytes, LenIter(A.lens, ToU64()), o->d_offs.p, (int)(n_rows + 1), st));
    o->launches += 2;
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[2], st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p, o->d_err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p + 1, o->d_offs.p + n_rows, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->upload_ms, o->ev[0], o->ev[1]));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->size_ms, o->ev[1], o->ev[2]));
    if ((uint32_t)o->h_back.p[0]) return ngzs::fail(o, NGZ_E_INVALID, "a row whose peer or byte value lies outside what was uploaded");
    const unsigned long long total = o->h_back.p[1];
    if (o->d_bytes.ensure(total + NGZ_OUTPUT_GUARD + 16)) return ngzs::fail(o, NGZ_E_NOMEM, "aggregated JSON bytes");
    A.out = o->d_bytes.p;
    A.total = total;
    NGZ_STAGE_HIP(o, hipMemsetAsync(A.out + total, 0xA5, NGZ_OUTPUT_GUARD, st));
    if (total) {
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
        hipLaunchKernelGGL(use_float ? pack_kernel<true>(small, o->writer != 0) : pack_kernel<false>(small, o->writer != 0), dim3(nb),
                           dim3(JS_THREADS), 0, st, A);
        NGZ_STAGE_HIP(o, hipGetLastError());
        ++o->launches;
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[3], st));
    }
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p, o->d_err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    if (total) NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->pack_ms, o->ev[0], o->ev[3]));
    if ((uint32_t)o->h_back.p[0]) return ngzs::fail(o, NGZ_E_INVALID, "a row whose peer or byte value lies outside what was uploaded");
    o->have = true;
    o->n_rows = n_rows;
    o->n_bytes = total;
    if (stats) *stats = ngz_agg_json_stats{n_rows, total, arena_bytes};
    return NGZ_OK;
}

int ngz_agg_json_result(ngz_agg_json *o, const uint8_t **bytes, const uint64_t **offsets, uint64_t *n_rows, uint64_t *n_bytes) {
    if (!o) return NGZ_E_INVALID;
    if (!o->have) return ngzs::fail(o, NGZ_E_INVALID, "no encode to read");
    if (bytes) *bytes = o->n_rows ? o->d_bytes.p : nullptr;
    if (offsets) *offsets = o->n_rows ? (const uint64_t *)o->d_offs.p : nullptr;
    if (n_rows) *n_rows = o->n_rows;
    if (n_bytes) *n_bytes = o->n_bytes;
    return NGZ_OK;
}

int ngz_agg_json_to_host(ngz_agg_json *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap) {
    if (!o) return NGZ_E_INVALID;
    if (!o->have) return ngzs::fail(o, NGZ_E_INVALID, "no encode to read");
    if ((bytes && bytes_cap < o->n_bytes) || (offsets && offsets_cap < o->n_rows + 1))
        return ngzs::fail(o, NGZ_E_INVALID, "a buffer smaller than the result");
    if (!o->n_rows) {
        if (offsets && offsets_cap) offsets[0] = 0;
        return NGZ_OK;
    }
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    if (bytes) {
        const uint64_t n = bytes_cap >= o->n_bytes + NGZ_OUTPUT_GUARD ? o->n_bytes + NGZ_OUTPUT_GUARD : o->n_bytes;
        if (n) NGZ_STAGE_HIP(o, hipMemcpy(bytes, o->d_bytes.p, n, hipMemcpyDeviceToHost));
    }
    if (offsets) NGZ_STAGE_HIP(o, hipMemcpy(offsets, o->d_offs.p, (o->n_rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return NGZ_OK;
}

int ngz_agg_json_last_timing(ngz_agg_json *o, float *upload_ms, float *size_ms, float *pack_ms) {
    if (!o || !upload_ms || !size_ms || !pack_ms) return NGZ_E_INVALID;
    *upload_ms = o->upload_ms;
    *size_ms = o->size_ms;
    *pack_ms = o->pack_ms;
    return NGZ_OK;
}

int ngz_agg_json_last_launches(ngz_agg_json *o) { return o ? o->launches : NGZ_E_INVALID; }

}  // extern "C"
