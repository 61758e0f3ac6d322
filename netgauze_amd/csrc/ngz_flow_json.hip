// serde JSON of decoded messages (include/ngz/flow_json.h): the line ngz_dgram_json (ngz_json.cpp, the
// specification) gives for each OK datagram of a batch, rendered on the device from the decoded columns.
// The whole output is one byte stream in stream order; every byte belongs either to a record (with the
// comma after it inside its set) or to glue: datagram head, set head, set tail, commas between sets,
// datagram tail.  The unit of work is a tile: at most 64 consecutive records of one data set.  They are
// consecutive rows of the slot's columns, so a lane-per-row load coalesces, and consecutive in the output,
// so a wave's LDS image (pack_tile, ngz_output_enc.h) holds them.  Per encode the host lists every slot's
// fields as items (column, renderer, separator and tag as constant text in a dword-padded pool), uploads
// the plan in one copy, and runs, whatever the number of slots, the passes of ngz_msg_stream.h (shared with
// ngz_wire.hip; FStream below says what is this stage's in them) around its own, the k_fj_ ones:
//   k_dgrams        one thread per datagram: rendered, not OK, or left to the host for its template sets,
//   k_sets          one thread per data set: its datagram's range of sets; the datagram of a template with
//                   a float the plan did not take (NGZ_FLOW_JSON_OPT_FLOATS 0, float32) is left to the host,
//   k_tiles         one thread per data set: its tiles, ceil(n / 64), if its datagram is rendered,
//   a hipcub exclusive scan and k_fill: the tile table (set, first record),
//   k_fj_size       a wave per tile, a lane per record through the counting writer, a wave sum per tile,
//   k_set_len       one thread per set: head, its tiles, tail,
//   k_dgram_len     one thread per datagram: head, sets, commas, tail; the stats,
//   a hipcub exclusive scan: the u64 offsets,
//   k_fj_glue_dgrams / k_fj_glue_sets  the same two walks downwards: every set's and tile's output offset,
//                   and the glue itself, written straight out by bytes,
//   k_fj_pack       a wave per tile: lane l sizes record l again, a wave scan places it, JAcc renders it
//                   into the wave's LDS image, which goes out in 16-byte stores; a record longer than the
//                   image goes straight out through the byte writer.
// pack_tile stores its ragged ends by bytes, so the glue and pack passes write disjoint bytes.
// k_fj_size and k_fj_pack have a second instantiation (FLT) whose renderer knows float64 (put_f64,
// ngz_f64_dev.h); it is launched in their place only when a slot with rows carries a float item, so a batch
// without one runs the kernels it ran before there was a float renderer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_json.h"
#include "ngz_host.h"
#include "ngz_f64_dev.h"
#include "ngz_json_dev.h"
#include "ngz_msg_stream.h"
#include "ngz_output_enc.h"

namespace {

using namespace ngzjson;
using namespace ngzms;
using ngzrow::align256;

constexpr uint32_t FJ_THREADS = THREADS;
// A wave's image, and 16 of slack for the output's misalignment: §2i's.  Nothing is staged here (a lane
// loads its own row's cells from the columns), so a block's LDS is the image: 30 KB, five blocks per CU.
constexpr uint32_t FJ_IMG = 30704;
constexpr uint32_t C_LINES = 1, C_TEMPLATE = 2, C_FLOAT = 3, C_NOT_OK = 4;  // ngz_flow_json_stats' order
constexpr uint8_t HOW_FLOAT = 3;  // between k_sets and k_dgram_len: NGZ_FLOW_JSON_HOST for a float field

enum : uint8_t {  // put_value / put_field of ngz_json.cpp, case by case
    RD_NULL, RD_U64, RD_I64, RD_BOOL, RD_IP4, RD_IP6, RD_LIST, RD_STRZ, RD_DT_SECS, RD_DT_MS, RD_DT_FRAC, RD_TCP, RD_SUBREG,
    RD_SUBREG_NESTED, RD_VSTR, RD_VLIST, RD_F64
};
enum { T_V10_A, T_SEQ, T_V10_DOMAIN, T_V9_A, T_V9_TIME, T_V9_SOURCE, T_SETS, T_DGRAM_TAIL, T_SET_TAIL, T_UNASSIGNED, T_COUNT };

struct FItem {
    const uint8_t *col;  // the field's column: row r at col + r * width
    JText pre, suf;      // the separator before the field and its tag, around its value
    uint16_t width;
    uint8_t rend, reserved;
    JSub sub;
};
struct FSlot {
    uint32_t item0, n_items;  // its fields in template order, scope fields first
    uint32_t n_rows, has_float;
    JText rec_head, rec_tail, set_head;  // {"scope_fields":[  |  ]}  |  {"Data":{"id":<template id>,"records":[
};
struct FArgs : Layout {  // passed by value
    const FSlot *slots;
    const FItem *items;
    const JName *names;
    const uint32_t *pool;
    JText fixed[T_COUNT];
};

template <bool FLT, class W>
__device__ __forceinline__ void render_value(W &w, const FArgs &A, const FItem &it, uint32_t row, uint32_t *err) {
    const uint8_t *cell = it.col + (uint64_t)row * it.width;
    if constexpr (FLT) {  // outside the switch: without FLT this function is what it was
        if (it.rend == RD_F64) {
            put_f64(w, ld_cell(cell, 8));
            return;
        }
    }
    switch (it.rend) {
    case RD_U64: put_dec(w, ld_cell(cell, it.width)); break;
    case RD_I64: {
        const int shift = 64 - 8 * (int)it.width;
        const int64_t sv = (int64_t)(ld_cell(cell, it.width) << shift) >> shift;
        if (sv < 0) w.push('-', 1);
        put_dec(w, sv < 0 ? 0ull - (uint64_t)sv : (uint64_t)sv);
        break;
    }
    case RD_BOOL: put_bool(w, cell[0] != 0); break;
    case RD_IP4: put_ip4_str(w, ld_cell(cell, it.width) & 0xFFFFFFFFu); break;
    case RD_IP6: put_ip6_str(w, cell); break;
    case RD_LIST: put_list(w, cell, it.width); break;
    case RD_STRZ: {  // a fixed string ends at its first NUL
        uint32_t n = 0;
        while (n < it.width && cell[n]) ++n;
        put_str(w, cell, n);
        break;
    }
    case RD_DT_SECS: put_datetime(w, (int64_t)ld_cell(cell, it.width), 0); break;
    case RD_DT_MS: {
        const int64_t ms = (int64_t)ld_cell(cell, 8), secs = floor_div(ms, 1000);
        put_datetime(w, secs, (uint32_t)(ms - secs * 1000) * 1000000u);
        break;
    }
    case RD_DT_FRAC: {  // {u32 secs, u32 nanos}
        const uint64_t v = ld_cell(cell, 8);
        put_datetime(w, (int64_t)(uint32_t)v, (uint32_t)(v >> 32));
        break;
    }
    case RD_TCP: put_tcp(w, cell[0]); break;
    case RD_SUBREG:
    case RD_SUBREG_NESTED:
        put_subreg(w, A.names, A.pool, A.fixed[T_UNASSIGNED], it.sub, it.rend == RD_SUBREG_NESTED, ld_cell(cell, it.width));
        break;
    case RD_VSTR:
    case RD_VLIST: {  // {u64 offset into the batch input, u32 length}; outside it: empty, and the encode fails
        const uint64_t off = *(const uint64_t *)cell;
        uint32_t len = *(const uint32_t *)(cell + 8);
        const uint8_t *p = A.in;
        if (off > A.in_size || len > A.in_size - off) {
            *err |= ERR_VLEN;
            len = 0;
        } else {
            p += off;
        }
        if (it.rend == RD_VSTR) put_str(w, p, len);
        else put_list(w, p, len);
        break;
    }
    default: w.push('n' | ('u' << 8) | ('l' << 16) | ('l' << 24), 4); break;
    }
}

// Row `row` of slot S as a record of its set, and the comma after it unless it is the set's last
template <bool FLT, class W>
__device__ __forceinline__ void render_record(const FArgs &A, const FSlot &S, uint32_t row, bool last, W &w, uint32_t *err) {
    w.text(A.pool + S.rec_head.off / 4u, S.rec_head.len);
    for (uint32_t i = 0; i < S.n_items; ++i) {
        const FItem &it = A.items[S.item0 + i];
        w.text(A.pool + it.pre.off / 4u, it.pre.len);
        render_value<FLT>(w, A, it, row, err);
        w.text(A.pool + it.suf.off / 4u, it.suf.len);
    }
    w.text(A.pool + S.rec_tail.off / 4u, S.rec_tail.len);
    if (!last) w.push(',', 1);
    w.finish();
}

// The datagram's text up to its first set
template <class W>
__device__ __forceinline__ void render_head(const FArgs &A, const ngz_dgram_hdr &h, W &w) {
    auto fixed = [&](int t) { w.text(A.pool + A.fixed[t].off / 4u, A.fixed[t].len); };
    if (h.version == 10) {
        fixed(T_V10_A);
        put_datetime(w, (int64_t)h.time, 0);
        fixed(T_SEQ);
        put_dec(w, h.sequence);
        fixed(T_V10_DOMAIN);
        put_dec(w, h.domain);
    } else {
        fixed(T_V9_A);
        put_dec(w, h.sys_up_time);
        fixed(T_V9_TIME);
        put_datetime(w, (int64_t)h.time, 0);
        fixed(T_SEQ);
        put_dec(w, h.sequence);
        fixed(T_V9_SOURCE);
        put_dec(w, h.domain);
    }
    fixed(T_SETS);
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// What is this stage's in the shared passes (ngz_msg_stream.h)
struct FStream {
    using Args = FArgs;
    static __device__ __forceinline__ int sets_how(const FSlot &S, const uint8_t &how) { return S.has_float && how == HOW_WRITTEN ? HOW_FLOAT : -1; }
    static __device__ __forceinline__ void fill_tile(const FArgs &, const FSlot &, uint32_t, uint32_t, uint32_t) {}  // k_fj_size sizes every tile
    static __device__ __forceinline__ unsigned long long set_len(const FArgs &A, const ngz_set_info &si, unsigned long long tiles) {
        return A.slots[si.slot].set_head.len + A.fixed[T_SET_TAIL].len + tiles;
    }
    static __device__ __forceinline__ unsigned long long dgram_frame(const FArgs &A, const ngz_dgram_hdr &h, uint32_t n_sets) {
        JCount w;
        render_head(A, h, w);
        return w.n + A.fixed[T_DGRAM_TAIL].len + (n_sets ? n_sets - 1u : 0u);  // a comma between two sets
    }
    static __device__ __forceinline__ uint32_t counter(const FArgs &A, uint32_t d, uint8_t how) {  // C_LINES + this
        if (how == HOW_FLOAT) A.how[d] = HOW_HOST;
        return how == HOW_WRITTEN ? 0u : how == HOW_HOST ? 1u : how == HOW_FLOAT ? 2u : 3u;
    }
};

template <bool FLT>
__global__ __launch_bounds__(FJ_THREADS) void k_fj_size(const FArgs A) {
    const uint32_t lane = threadIdx.x & 63u, n_tiles = min(A.tile0[A.n_sets], A.tile_cap);
    uint32_t err = 0;
    for (uint32_t t = blockIdx.x * (FJ_THREADS / 64u) + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * (FJ_THREADS / 64u)) {
        const TileRows tr = tile_rows(A, t);
        JCount w;
        if (lane < tr.cnt) render_record<FLT>(A, A.slots[tr.si.slot], tr.row0 + lane, tr.first + lane + 1u == tr.si.n, w, &err);
        const uint64_t sum = ngzs::wave_sum(w.n);
        if (lane == 0) A.tile_bytes[t] = (uint32_t)sum;
    }
    if (err) atomicOr((unsigned int *)&A.counters[C_ERR], err);
}

// The datagram's head, the commas between its sets and its closing text; where each of its sets starts
__global__ __launch_bounds__(FJ_THREADS) void k_fj_glue_dgrams(const FArgs A) {
    const uint32_t d = blockIdx.x * FJ_THREADS + threadIdx.x;
    if (d >= A.n_dgrams || A.how[d] != NGZ_FLOW_JSON_LINE) return;
    const unsigned long long o1 = min(A.offs[d + 1], A.total);
    JByte w{A.out + A.offs[d], A.out + o1};
    render_head(A, A.hdr[d], w);
    const uint32_t s0 = A.dset0[d], s1 = min(A.dset1[d], A.n_sets);
    for (uint32_t s = s0; s < s1; ++s) {
        if (s > s0) w.put(',');
        A.set_off[s] = (unsigned long long)(w.p - A.out);
        w.p += A.set_len[s];
    }
    w.text(A.pool + A.fixed[T_DGRAM_TAIL].off / 4u, A.fixed[T_DGRAM_TAIL].len);
}

// The set's head and tail; where each of its tiles starts
__global__ __launch_bounds__(FJ_THREADS) void k_fj_glue_sets(const FArgs A) {
    const uint32_t s = blockIdx.x * FJ_THREADS + threadIdx.x;
    if (s >= A.n_sets) return;
    const ngz_set_info si = A.sets[s];
    if (!set_ok(A, si) || A.how[si.dgram] != NGZ_FLOW_JSON_LINE) return;
    const JText head = A.slots[si.slot].set_head;
    const unsigned long long o0 = A.set_off[s], o1 = min(o0 + A.set_len[s], A.total);
    JByte w{A.out + o0, A.out + o1};
    w.text(A.pool + head.off / 4u, head.len);
    const uint32_t t1 = min(A.tile0[s + 1], A.tile_cap);
    for (uint32_t t = A.tile0[s]; t < t1; ++t) {
        A.tile_off[t] = (unsigned long long)(w.p - A.out);
        w.p += A.tile_bytes[t];
    }
    w.text(A.pool + A.fixed[T_SET_TAIL].off / 4u, A.fixed[T_SET_TAIL].len);
}

// One wave per block: LDS, not threads, bounds what a CU holds
template <class WImg, bool FLT>
__global__ __launch_bounds__(64) void k_fj_pack(const FArgs A, const uint32_t n_tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t img[FJ_IMG + 16];  // pack_tile's
    const uint32_t lane = threadIdx.x;
    uint32_t err = 0;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const TileRows tr = tile_rows(A, t);
        const FSlot &S = A.slots[tr.si.slot];
        const uint32_t row = tr.row0 + lane;
        const bool last = tr.first + lane + 1u == tr.si.n;
        JCount c;
        if (lane < tr.cnt) render_record<FLT>(A, S, row, last, c, &err);
        const uint32_t incl = wave_incl_scan(c.n);
        ngzenc::pack_tile<FJ_IMG, WImg, JByte>(lane, tr.cnt, A.tile_off[t], incl - c.n, incl, A.out, A.total, img,
                                               [&](auto &w) { render_record<FLT>(A, S, row, last, w, &err); });
    }
    if (err) atomicOr((unsigned int *)&A.counters[C_ERR], err);
}

}  // namespace

struct ngz_flow_json : ngzms::MsgStage {  // its plan in d_in: slots, items, names, pool
    ngz_flow_json() : MsgStage("flow JSON") {}
    bool floats = false;  // NGZ_FLOW_JSON_OPT_FLOATS
};

namespace {

using ngzh::Spec;

std::string ie_label(const Spec &s) {
    return s.name ? std::string(s.name) : "pen " + std::to_string(s.pen) + " id " + std::to_string(s.id);
}

const char *const kScopeNames[] = {nullptr, "System", "Interface", "LineCard", "Cache", "Template"};

// put_field / put_value's choice for field `sp` of column layout `fd`.  *is_float: serde_json's float text
// where the plan leaves it to the host (float32 always, float64 unless `floats`).  false: a column the
// loaders cannot read.
bool pick(const Spec &sp, const DevField &fd, bool floats, Pool &pool, std::vector<JName> &names, FItem *it, std::string *pre,
          std::string *suf, bool *is_float) {
    const bool int_w = fd.width == 1 || fd.width == 2 || fd.width == 4 || fd.width == 8;
    it->width = fd.width;
    it->rend = RD_NULL;
    if (sp.kind == ngzh::IK_SCOPE) {  // NFv9 ScopeField: a known scope's u32 or bytes, an unknown one's bytes
        const char *nm = sp.pen == 0 && sp.id >= 1 && sp.id <= 5 ? kScopeNames[sp.id] : nullptr;
        if (nm) {
            *pre = std::string("{\"") + nm + "\":";
            *suf = "}";
        } else {
            *pre = "{\"Unknown\":{\"pen\":" + std::to_string(sp.pen) + ",\"id\":" + std::to_string(sp.id) + ",\"value\":";
            *suf = "}}";
        }
        it->rend = nm && fd.kind == NGZ_K_SCOPE32 ? RD_U64 : RD_LIST;
        return it->rend == RD_LIST || fd.width == 4;
    }
    tag_text(sp, pre, suf);
    const bool known = sp.kind == ngzh::IK_IANA || sp.kind == ngzh::IK_VENDOR;
    switch (fd.kind) {
    case NGZ_K_UINT:
        it->rend = RD_U64;
        if (known && (sp.flags & 4)) {
            if (const int sk = add_subreg(sp.pen, sp.id, pool, names, &it->sub)) {
                it->rend = sk == 2 ? RD_SUBREG_NESTED : RD_SUBREG;
                return int_w;
            }
        }
        if (known && sp.dtype == ngzh::DT_float64 && floats) {
            it->rend = RD_F64;
            return fd.width == 8;
        }
        if (known && (sp.dtype == ngzh::DT_float32 || sp.dtype == ngzh::DT_float64)) *is_float = true;
        if (known && sp.dtype == ngzh::DT_ipv4Address) it->rend = RD_IP4;
        if (known && sp.dtype == ngzh::DT_dateTimeSeconds) it->rend = RD_DT_SECS;
        return int_w;
    case NGZ_K_SCOPE32: it->rend = RD_U64; return fd.width == 4;
    case NGZ_K_TCPFLAGS: it->rend = RD_TCP; return true;
    case NGZ_K_SINT: it->rend = RD_I64; return int_w;
    case NGZ_K_BOOL: it->rend = RD_BOOL; return true;
    case NGZ_K_BYTES: it->rend = known && sp.dtype == ngzh::DT_ipv6Address && fd.width == 16 ? RD_IP6 : RD_LIST; return true;
    case NGZ_K_U256: it->rend = RD_LIST; return fd.width == 32;
    case NGZ_K_DTMS: it->rend = RD_DT_MS; return fd.width == 8;
    case NGZ_K_DTFRAC: it->rend = RD_DT_FRAC; return fd.width == 8;
    case NGZ_K_STR: it->rend = RD_STRZ; return true;
    case NGZ_K_VLEN: it->rend = (fd.flags & 0x80) ? RD_VSTR : RD_VLIST; return fd.width == 16;
    }
    return true;  // a kind put_value prints as null
}

}  // namespace

extern "C" {

int ngz_flow_json_abi_version(void) { return NGZ_FLOW_JSON_ABI_VERSION; }

int ngz_flow_json_create(int device, ngz_flow_json **out) {
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0) return NGZ_E_INVALID;
    ngz_flow_json *j = new ngz_flow_json;
    j->device = device;
    *out = j;
    return NGZ_OK;
}

void ngz_flow_json_destroy(ngz_flow_json *j) {
    if (!j) return;
    if (j->device_ready) {
        hipSetDevice(j->device);
        j->release_device();
    }
    delete j;
}

const char *ngz_flow_json_last_error(ngz_flow_json *j) { return j ? j->last_error.c_str() : "null flow JSON stage"; }

int ngz_flow_json_set_option(ngz_flow_json *j, int opt, int64_t value) {
    if (!j) return NGZ_E_INVALID;
    if (opt != NGZ_FLOW_JSON_OPT_FLOATS || (value != 0 && value != 1)) return ngzs::fail(j, NGZ_E_INVALID, "unknown option or value");
    j->floats = value != 0;
    return NGZ_OK;
}

int ngz_flow_json_f64_text(uint64_t bits, char *buf, size_t cap) {
    uint8_t text[32];  // put_f64 writes at most 24 characters
    JByte w{text, text + sizeof text};
    put_f64(w, bits);
    const size_t n = (size_t)(w.p - text);
    if (!buf || cap < n) return NGZ_E_INVALID;
    memcpy(buf, text, n);
    return (int)n;
}

int ngz_flow_json_encode(ngz_flow_json *o, ngz_ctx *ctx, const ngz_batch_out *out, ngz_flow_json_stats *stats, void *hip_stream) {
    if (!o || !ctx || !out) return NGZ_E_INVALID;
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = ngzms::begin(o, ctx, out)) return rc;
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    if (!D) {  // no datagram: no kernel
        o->have = true;
        return NGZ_OK;
    }

    // the plan: every slot's record as items, as json_render_mode walks it (ngz_json.cpp)
    std::vector<FSlot> slots(S);
    std::vector<FItem> items;
    std::vector<JName> names;
    Pool pool;
    uint64_t n_records = 0;
    bool use_float = false;  // a slot with rows has a float item: the renderer kernels' float instantiation
    for (uint32_t s = 0; s < S; ++s) {
        const ngz_slot_info &si = out->slots[s];
        const ngzh::Version *pv;
        if (int rc = ngzms::slot_version(o, ctx, out, s, &pv)) return rc;
        const ngzh::Version &ver = *pv;
        const uint32_t nf = (uint32_t)ver.specs.size();
        FSlot &fs = slots[s];
        fs = FSlot{};
        fs.item0 = (uint32_t)items.size();
        fs.n_items = nf;
        fs.n_rows = si.n_records;
        n_records += si.n_records;
        for (uint32_t f = 0; f < nf; ++f) {
            const Spec &sp = ver.specs[f];
            const DevField &fd = ver.plan.f[f];
            FItem it{};
            std::string pre, suf;
            bool is_float = false;
            if (!pick(sp, fd, o->floats, pool, names, &it, &pre, &suf, &is_float))
                return ngzs::fail(o, NGZ_E_LIMIT, "field " + ie_label(sp) + ": a column of a width the renderers cannot read");
            if (is_float) fs.has_float = 1;
            if (it.rend == RD_F64 && si.n_records) use_float = true;
            it.col = si.columns ? si.columns + (uint64_t)si.capacity * fd.col_off : nullptr;
            it.pre = pool.add((f == ver.n_scope ? "],\"fields\":[" : f ? "," : "") + pre);
            it.suf = pool.add(suf);
            items.push_back(it);
        }
        fs.rec_head = pool.add("{\"scope_fields\":[");
        fs.rec_tail = pool.add(ver.n_scope == nf ? "],\"fields\":[]}" : "]}");
        fs.set_head = pool.add("{\"Data\":{\"id\":" + std::to_string(ver.tid) + ",\"records\":[");
    }
    if (names.size() > NGZ_FLOW_JSON_MAX_NAMES) return ngzs::fail(o, NGZ_E_LIMIT, "more sub-registry variants than NGZ_FLOW_JSON_MAX_NAMES");
    FArgs A{};
    A.fixed[T_V10_A] = pool.add("{\"IPFIX\":{\"version\":10,\"export_time\":");
    A.fixed[T_SEQ] = pool.add(",\"sequence_number\":");
    A.fixed[T_V10_DOMAIN] = pool.add(",\"observation_domain_id\":");
    A.fixed[T_V9_A] = pool.add("{\"NetFlowV9\":{\"version\":9,\"sys_up_time\":");
    A.fixed[T_V9_TIME] = pool.add(",\"unix_time\":");
    A.fixed[T_V9_SOURCE] = pool.add(",\"source_id\":");
    A.fixed[T_SETS] = pool.add(",\"sets\":[");
    A.fixed[T_DGRAM_TAIL] = pool.add("]}}");
    A.fixed[T_SET_TAIL] = pool.add("]}}");
    A.fixed[T_UNASSIGNED] = pool.add("{\"Unassigned\":");
    pool.b.resize(pool.b.size() + 4, 0);
    if (pool.b.size() >> 31) return ngzs::fail(o, NGZ_E_LIMIT, "batch too large");

    const uint64_t items_at = align256(slots.size() * sizeof(FSlot)), names_at = items_at + align256(items.size() * sizeof(FItem));
    const uint64_t pool_at = names_at + align256(names.size() * sizeof(JName)), plan_bytes = pool_at + align256(pool.b.size());
    if (int rc = carve(o, ctx, out, hip_stream, plan_bytes, n_records, &A)) return rc;
    uint8_t *h = o->h_in.p;
    if (S) memcpy(h, slots.data(), slots.size() * sizeof(FSlot));
    if (!items.empty()) memcpy(h + items_at, items.data(), items.size() * sizeof(FItem));
    if (!names.empty()) memcpy(h + names_at, names.data(), names.size() * sizeof(JName));
    memcpy(h + pool_at, pool.b.data(), pool.b.size());
    A.slots = (const FSlot *)o->d_in.p;
    A.items = (const FItem *)(o->d_in.p + items_at);
    A.names = (const JName *)(o->d_in.p + names_at);
    A.pool = (const uint32_t *)(o->d_in.p + pool_at);

    if (int rc = run_tiles<FStream>(o, A)) return rc;
    if (NS) {
        const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)A.tile_cap + 3) / 4, (uint64_t)o->n_cus * 16));
        NGZ_STAGE_HIP(o, o->launch(use_float ? k_fj_size<true> : k_fj_size<false>, nb, FJ_THREADS, A));
    }
    uint32_t n_tiles = 0;
    if (int rc = run_offsets<FStream>(o, A, &n_tiles)) return rc;
    const unsigned long long total = A.total;
    hipStream_t st = o->st;
    NGZ_STAGE_HIP(o, hipMemsetAsync(A.out + total, 0xA5, NGZ_OUTPUT_GUARD, st));
    if (total) {
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
        NGZ_STAGE_HIP(o, o->launch(k_fj_glue_dgrams, blocks(D), FJ_THREADS, A));
        if (NS) NGZ_STAGE_HIP(o, o->launch(k_fj_glue_sets, blocks(NS), FJ_THREADS, A));
        if (n_tiles) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)o->n_cus * 16);
            NGZ_STAGE_HIP(o, o->launch(use_float ? k_fj_pack<JAcc, true> : k_fj_pack<JAcc, false>, nb, 64u, A, n_tiles));
        }
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[3], st));
    }
    if (int rc = read_errors(o)) return rc;
    if (total) NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->pack_ms, o->ev[0], o->ev[3]));
    if (int rc = finish(o, D, total)) return rc;
    const unsigned long long *hb = o->h_back.p;
    if (stats) *stats = ngz_flow_json_stats{hb[C_LINES], total, hb[C_TEMPLATE], hb[C_FLOAT], hb[C_NOT_OK]};
    return NGZ_OK;
}

int ngz_flow_json_result(ngz_flow_json *o, const uint8_t **bytes, const uint64_t **offsets, const uint8_t **how, uint64_t *n_dgrams,
                         uint64_t *n_bytes) {
    return ngzms::result(o, bytes, offsets, how, n_dgrams, n_bytes);
}

int ngz_flow_json_to_host(ngz_flow_json *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap, uint8_t *how,
                          uint64_t how_cap) {
    return ngzms::to_host(o, bytes, bytes_cap, offsets, offsets_cap, how, how_cap);
}

int ngz_flow_json_last_timing(ngz_flow_json *o, float *size_ms, float *offsets_ms, float *pack_ms) {
    if (!o || !size_ms || !offsets_ms || !pack_ms) return NGZ_E_INVALID;
    *size_ms = o->size_ms;
    *offsets_ms = o->offsets_ms;
    *pack_ms = o->pack_ms;
    return NGZ_OK;
}

int ngz_flow_json_last_launches(ngz_flow_json *o) { return o ? o->launches : NGZ_E_INVALID; }

}  // extern "C"
