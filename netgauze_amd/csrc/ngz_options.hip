// The flow-options input (include/ngz/flow_options.h): the reference's FlowOptionsActor loop
// (crates/collector/src/inputs/flow_options/actor.rs:217-326) over the decoded columns of a batch.
// The per-template plan is built on the host (ngz_options_plan.cpp); the device finds the live
// rows of the options slots, applies the one per-record test (the id equality), sizes, scans and
// packs each row's operations, copying variable-length values out of the batch input, so the host
// reads back the few bytes the operations hold and never the columns.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_options.h"
#include "ngz_host.h"
#include "ngz_options_plan.h"
#include "ngz_stage.h"

namespace {

constexpr uint32_t OP_THREADS = 256;
constexpr uint32_t OP_MAX_VALUES = 2 * NGZ_OPTIONS_MAX_REFS;  // scope fields then fields of one operation
constexpr uint32_t OP_HEADER_WORDS = 5;  // bytes, set index, record in set, domain, slot | op << 16
constexpr uint64_t SLOT_NOT_OPTIONS = ~0ull;      // slot_off: a slot without scope fields
constexpr uint64_t SLOT_COUNT_ONLY = ~0ull - 1;   // an options slot whose live rows are only counted
// device counters
constexpr uint32_t C_OK_DGRAMS = 0, C_OPS = 1, C_ID_ERRORS = 2, C_ERR = 3, C_SLOT0 = 4;
constexpr uint32_t ERR_SETS = 1, ERR_VLEN = 2;  // ERR_SETS: the bit ngzs::for_each_set sets

enum : uint32_t { V_FIXED = 0, V_STR = 1, V_VLEN = 2 };
struct OpValue {
    const uint8_t *col;  // the column the value is read from
    uint32_t width;      // column bytes per row
    uint32_t mode;       // V_FIXED the cell; V_STR the cell up to its first NUL; V_VLEN {u64 offset, u32 len, u32 0}
};

// What the row and pack kernels need of one slot, passed by value
struct OpPlan {
    OpValue v[2][OP_MAX_VALUES];
    uint32_t nv[2];
    uint32_t n_ops;
    uint32_t id_equal;
    const uint8_t *id_col[2];
    uint32_t id_w[2];
    uint32_t n_rows;
    uint32_t slot;
    const uint32_t *rowset;            // per row of the slot: its set index + 1, 0 = a failed message's row
    unsigned long long *size;          // per row: bytes of its packed operations (row pass)
    const unsigned long long *offs;    // the scanned sizes, n_rows + 1 readable (pack pass)
    uint8_t *packed;
    unsigned long long total;          // bytes of the packed buffer
    const ngz_set_info *sets;
    const ngz_dgram_hdr *hdr;
    const uint8_t *bytes;              // the batch input
    unsigned long long bytes_size;
    unsigned long long *counters;
};

// Columns start at capacity * col_off: only their cells' own alignment is known, so cells are read
// bytewise (this path carries a few bytes per options row)
__device__ __forceinline__ uint64_t op_load_le(const uint8_t *p, uint32_t n) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < n; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// Length and source of one value of `row`; a variable-length cell outside the input reads as empty
__device__ __forceinline__ uint32_t op_value(const OpValue &v, uint32_t row, const uint8_t *bytes, unsigned long long bytes_size,
                                             const uint8_t **src, uint32_t *err) {
    const uint8_t *cell = v.col + (uint64_t)v.width * row;
    if (v.mode == V_FIXED) {
        *src = cell;
        return v.width;
    }
    if (v.mode == V_STR) {
        uint32_t n = 0;
        while (n < v.width && cell[n]) ++n;
        *src = cell;
        return n;
    }
    const uint64_t off = op_load_le(cell, 8);
    const uint32_t len = (uint32_t)op_load_le(cell + 8, 4);
    if (off > bytes_size || len > bytes_size - off) {
        *err |= ERR_VLEN;
        *src = bytes;
        return 0;
    }
    *src = bytes + off;
    return len;
}

// One thread per data set (ngzs::for_each_set): the rows of an options slot's set whose message
// decoded get the set's index + 1 and count as live rows of the slot; the other rows keep the 0
// the buffer was cleared to.  Then the batch's NGZ_DG_OK messages are counted.
__global__ __launch_bounds__(OP_THREADS) void k_options_sets(const ngz_set_info *__restrict__ sets, uint32_t n_sets,
                                                             const ngz_dgram_hdr *__restrict__ hdr, uint32_t n_dgrams, uint32_t n_slots,
                                                             const uint32_t *__restrict__ slot_rows, const uint64_t *__restrict__ slot_off,
                                                             uint32_t *__restrict__ rowset, unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long acc[1];
    const uint32_t stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
    ngzs::for_each_set(sets, n_sets, hdr, n_dgrams, n_slots, slot_rows, (unsigned int *)&counters[C_ERR],
                       [&](uint32_t s, const ngz_set_info &si, const ngz_dgram_hdr &h) {
        const uint64_t off = slot_off[si.slot];
        if (off == SLOT_NOT_OPTIONS || h.status != NGZ_DG_OK) return;
        atomicAdd(&counters[C_SLOT0 + si.slot], (unsigned long long)si.n);
        if (off == SLOT_COUNT_ONLY) return;
        uint32_t *p = rowset + off + si.rec0;
        for (uint32_t r = 0; r < si.n; ++r) p[r] = s + 1u;
    });
    uint64_t ok[1] = {0};
    for (uint32_t d = t0; d < n_dgrams; d += stride) ok[0] += hdr[d].status == NGZ_DG_OK ? 1u : 0u;
    unsigned long long *const dst[1] = {&counters[C_OK_DGRAMS]};
    ngzs::block_add<1>(acc, ok, dst);
}

// One thread per row of an options slot: the id test and the bytes of the row's packed operations
__global__ __launch_bounds__(OP_THREADS) void k_options_rows(const OpPlan P) {
    __shared__ unsigned long long acc[2];
    uint64_t cnt[2] = {0, 0};  // operations, id errors
    uint32_t err = 0;
    for (uint32_t r = blockIdx.x * OP_THREADS + threadIdx.x; r < P.n_rows; r += gridDim.x * OP_THREADS) {
        unsigned long long bytes = 0;
        if (P.rowset[r]) {
            bool ok = true;
            if (P.id_equal)
                ok = op_load_le(P.id_col[0] + (uint64_t)P.id_w[0] * r, P.id_w[0]) ==
                     op_load_le(P.id_col[1] + (uint64_t)P.id_w[1] * r, P.id_w[1]);
            if (!ok) {
                ++cnt[1];
            } else {
                cnt[0] += P.n_ops;
                for (uint32_t op = 0; op < P.n_ops; ++op) {
                    uint32_t vb = 0;
                    for (uint32_t i = 0; i < P.nv[op]; ++i) {
                        const uint8_t *src;
                        vb += op_value(P.v[op][i], r, P.bytes, P.bytes_size, &src, &err);
                    }
                    bytes += 4ull * (OP_HEADER_WORDS + P.nv[op]) + ((vb + 3u) & ~3u);
                }
            }
        }
        P.size[r] = bytes;
    }
    if (err) atomicOr((unsigned int *)&P.counters[C_ERR], err);
    unsigned long long *const dst[2] = {&P.counters[C_OPS], &P.counters[C_ID_ERRORS]};
    ngzs::block_add<2>(acc, cnt, dst);
}

// One thread per row: the row's operations at its scanned offset.  Per operation: the header words
// (bytes, set index, record in the set, observation domain, slot | op << 16), one length word per
// value, the values back to back, zero-padded to a word.  Nothing is written past P.total.
__global__ __launch_bounds__(OP_THREADS) void k_options_pack(const OpPlan P) {
    for (uint32_t r = blockIdx.x * OP_THREADS + threadIdx.x; r < P.n_rows; r += gridDim.x * OP_THREADS) {
        const unsigned long long at = P.offs[r], size = P.offs[r + 1] - at;
        const uint32_t set1 = P.rowset[r];
        if (!size || !set1 || at > P.total || size > P.total - at) continue;
        const ngz_set_info si = P.sets[set1 - 1u];
        const uint32_t domain = P.hdr[si.dgram].domain;
        uint8_t *w = P.packed + at;
        uint8_t *const row_end = w + size;
        uint32_t err = 0;
        for (uint32_t op = 0; op < P.n_ops; ++op) {
            const uint32_t nv = P.nv[op];
            uint32_t *head = (uint32_t *)w;  // offsets and sizes are multiples of 4, the buffer is 256-byte aligned
            uint8_t *val = w + 4ull * (OP_HEADER_WORDS + nv);
            if (val > row_end) break;
            uint32_t vb = 0;
            for (uint32_t i = 0; i < nv; ++i) {
                const uint8_t *src;
                const uint32_t n = op_value(P.v[op][i], r, P.bytes, P.bytes_size, &src, &err);
                if (val + vb + n > row_end) break;  // cannot happen: the sizes come from the same rule
                head[OP_HEADER_WORDS + i] = n;
                for (uint32_t b = 0; b < n; ++b) val[vb + b] = src[b];
                vb += n;
            }
            const uint32_t padded = (vb + 3u) & ~3u;
            for (uint32_t b = vb; b < padded && val + b < row_end; ++b) val[b] = 0;
            head[0] = 4u * (OP_HEADER_WORDS + nv) + padded;
            head[1] = set1 - 1u;
            head[2] = r - si.rec0;
            head[3] = domain;
            head[4] = P.slot | (op << 16);
            w = val + padded;
        }
    }
}

struct HostValue {  // what the host needs to name one value of an operation
    uint32_t pen;
    uint16_t ie;
    uint8_t kind;
};
struct HostSlotPlan {
    uint32_t n_ops = 0;
    uint32_t n_scope[2] = {0, 0};
    std::vector<HostValue> v[2];
};

}  // namespace

struct ngz_options : ngzs::Stage {
    ngz_options() : Stage(4) {}
    uint8_t weight = 0;
    ngz_options_stats totals{};
    float harvest_ms = 0;
    int launches = 0;
    ngzh::DevBuf<uint32_t> d_rowset;
    ngzh::DevBuf<unsigned long long> d_size, d_offs, d_counters;
    ngzh::DevBuf<uint64_t> d_meta;  // slot_off[S], then slot_rows[S] as uint32_t
    ngzh::DevBuf<uint8_t> d_scan_tmp, d_packed;
    // the last harvest's operations: the packed records and what points into them
    std::vector<uint8_t> h_packed;
    std::vector<ngz_enrich_field> op_fields;
    std::vector<ngz_enrich_operation> ops;
};

namespace {

// The canonical kind an operation's value has, and how the kernels read it from its column
bool value_rule(const ngz_field_info &fi, uint32_t pen, uint16_t ie, uint8_t *kind, uint32_t *mode) {
    switch (fi.kind) {
    case NGZ_K_SCOPE32:
        *kind = NGZ_K_UINT;
        *mode = V_FIXED;
        return fi.width == 4;
    case NGZ_K_STR:
        *kind = NGZ_K_STR;
        *mode = V_STR;
        return true;
    case NGZ_K_VLEN: {
        const ngzh::IeRow *row = ngzh::ie_find(pen, ie);
        *kind = row && row->dtype == ngzh::DT_string ? NGZ_K_STR : NGZ_K_BYTES;
        *mode = V_VLEN;
        return fi.width == 16;
    }
    case NGZ_K_UINT: case NGZ_K_TCPFLAGS: case NGZ_K_SINT: case NGZ_K_BOOL: case NGZ_K_BYTES: case NGZ_K_U256: case NGZ_K_DTMS:
    case NGZ_K_DTFRAC:
        *kind = fi.kind;
        *mode = V_FIXED;
        return fi.width > 0;
    }
    return false;
}

void add_stats(ngz_options_stats &t, const ngz_options_stats &b) {
    t.received_flows += b.received_flows;
    t.processed_options_records += b.processed_options_records;
    t.operations_generated += b.operations_generated;
    t.normalization_errors += b.normalization_errors;
    t.netflow_v9_conversion_errors += b.netflow_v9_conversion_errors;
    t.ops_refused += b.ops_refused;
}

}  // namespace

extern "C" {

int ngz_options_abi_version(void) { return NGZ_OPTIONS_ABI_VERSION; }

int ngz_options_create(int device, uint8_t weight, ngz_options **out) {
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0) return NGZ_E_INVALID;
    ngz_options *o = new ngz_options;
    o->device = device;
    o->weight = weight;
    *out = o;
    return NGZ_OK;
}

void ngz_options_destroy(ngz_options *o) {
    if (!o) return;
    if (o->device_ready) {
        hipSetDevice(o->device);
        o->d_rowset.release();
        o->d_size.release();
        o->d_offs.release();
        o->d_counters.release();
        o->d_meta.release();
        o->d_scan_tmp.release();
        o->d_packed.release();
    }
    delete o;
}

const char *ngz_options_last_error(ngz_options *o) { return o ? o->last_error.c_str() : "null harvester"; }

int ngz_options_harvest(ngz_options *o, ngz_ctx *ctx, const ngz_batch_out *out, const ngz_enrich_peer *peer,
                        ngz_options_stats *batch_stats, void *hip_stream) {
    if (!o || !ctx || !out || !peer) return NGZ_E_INVALID;
    if (batch_stats) memset(batch_stats, 0, sizeof *batch_stats);
    if (peer->family != 4 && peer->family != 6) return ngzs::fail(o, NGZ_E_INVALID, "peer address family");
    if (int rc = ngzs::check_ctx(o, ctx)) return rc;
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    if (!ngzs::slot_table_ok(out) || S != ctx->slot_version.size() || D != ctx->last_in.n)
        return ngzs::fail(o, NGZ_E_INVALID, "slot table: `out` is not the context's last decode");
    o->ops.clear();
    o->op_fields.clear();
    o->h_packed.clear();
    o->launches = 0;
    o->harvest_ms = 0;

    // per-slot plans; nothing touches the device before every slot checked out
    struct SlotWork {
        OpPlan k;
        bool packs = false;
        uint8_t outcome = NGZ_OPTIONS_OUT_NOT_OPTIONS;
        uint64_t row0 = 0;
    };
    std::vector<SlotWork> work(S);
    std::vector<HostSlotPlan> hplan(S);
    std::vector<uint64_t> slot_off(S, SLOT_NOT_OPTIONS);
    std::vector<uint32_t> slot_rows(S, 0);
    std::vector<ngz_field_info> fi;
    std::vector<ngzo::PlanField> pf;
    uint64_t n_rows = 0;
    bool any_options = false;
    for (uint32_t s = 0; s < S; ++s) {
        const ngz_slot_info &si = out->slots[s];
        SlotWork &w = work[s];
        memset(&w.k, 0, sizeof w.k);
        slot_rows[s] = si.n_records;
        if (!si.n_records) continue;
        const int nf = ngzs::slot_fields(o, ctx, s, fi);
        if (nf < 0) return nf;
        pf.resize(nf);
        for (int i = 0; i < nf; ++i) {
            pf[i].pen = fi[i].pen;
            pf[i].ie = fi[i].ie_id;
            pf[i].scope = fi[i].is_scope != 0;
        }
        ngz_options_plan plan;
        if (ngzo::plan_fields(pf, si.proto, &plan))
            return ngzs::fail(o, NGZ_E_LIMIT, "an options template with more than 24 scope fields or fields per operation");
        w.outcome = plan.outcome;
        if (plan.outcome == NGZ_OPTIONS_OUT_NOT_OPTIONS) continue;
        any_options = true;
        slot_off[s] = SLOT_COUNT_ONLY;
        if (plan.outcome != NGZ_OPTIONS_OUT_OPS || !plan.n_ops) continue;
        if (!si.columns || si.capacity < si.n_records) return ngzs::fail(o, NGZ_E_LIMIT, "unexpected column block");
        auto column = [&](uint32_t f) { return (const uint8_t *)si.columns + (uint64_t)si.capacity * fi[f].col_off; };
        HostSlotPlan &hp = hplan[s];
        hp.n_ops = plan.n_ops;
        w.k.n_ops = plan.n_ops;
        for (uint32_t op = 0; op < plan.n_ops; ++op) {
            hp.n_scope[op] = plan.n_scope[op];
            const uint32_t nv = (uint32_t)plan.n_scope[op] + plan.n_fields[op];
            w.k.nv[op] = nv;
            for (uint32_t i = 0; i < nv; ++i) {
                const bool sc = i < plan.n_scope[op];
                const ngz_options_ref &ref = sc ? plan.scope[op][i] : plan.fields[op][i - plan.n_scope[op]];
                const uint32_t src = sc ? plan.scope_src[op][i] : plan.fields_src[op][i - plan.n_scope[op]];
                if (src >= (uint32_t)nf) return ngzs::fail(o, NGZ_E_INVALID, "plan source field");
                HostValue hv{ref.pen, ref.ie_id, 0};
                OpValue &kv = w.k.v[op][i];
                // a re-tagged name keeps the string-ness of the IE it was read as
                if (!value_rule(fi[src], fi[src].pen, fi[src].ie_id, &hv.kind, &kv.mode))
                    return ngzs::fail(o, NGZ_E_LIMIT, "an options field of a kind the harvest cannot carry");
                kv.col = column(src);
                kv.width = fi[src].width;
                hp.v[op].push_back(hv);
            }
        }
        w.k.id_equal = plan.id_equal;
        if (plan.id_equal) {
            for (int d = 0; d < 2; ++d) {
                const ngz_field_info &f = fi[plan.id_src[d]];
                if ((f.kind != NGZ_K_UINT && f.kind != NGZ_K_SCOPE32) || f.width < 1 || f.width > 8)
                    return ngzs::fail(o, NGZ_E_LIMIT, "an interface or VRF id that is no unsigned integer");
                w.k.id_col[d] = column(plan.id_src[d]);
                w.k.id_w[d] = f.width;
            }
        }
        w.k.n_rows = si.n_records;
        w.k.slot = s;
        w.packs = true;
        w.row0 = n_rows;
        slot_off[s] = n_rows;
        n_rows += si.n_records;
    }
    ngz_options_stats bs{};
    if (int rc = ngzs::device_init(o)) return rc;
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    if (!any_options) {
        // no options row: no kernel.  received_flows still counts the messages that decoded: their
        // headers (32 bytes per datagram) are all that is read
        if (D) {
            std::vector<ngz_dgram_hdr> hdr(D);
            NGZ_STAGE_HIP(o, hipMemcpyAsync(hdr.data(), out->dgrams, (size_t)D * sizeof(ngz_dgram_hdr), hipMemcpyDeviceToHost, st));
            NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
            for (const ngz_dgram_hdr &h : hdr) bs.received_flows += h.status == NGZ_DG_OK;
        }
        add_stats(o->totals, bs);
        if (batch_stats) *batch_stats = bs;
        return NGZ_OK;
    }
    if (n_rows >> 31) return ngzs::fail(o, NGZ_E_LIMIT, "batch too large");

    const size_t n_counters = C_SLOT0 + S, n_meta = 2ull * S + 2;
    size_t scan_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                         (int)(n_rows + 1), st) != hipSuccess)
        return ngzs::fail(o, NGZ_E_DEVICE, "scan temp size");
    if (o->d_rowset.ensure(n_rows + 1) || o->d_size.ensure(n_rows + 1) || o->d_offs.ensure(n_rows + 2) ||
        o->d_counters.ensure(n_counters) || o->d_meta.ensure(n_meta) || o->d_scan_tmp.ensure(scan_bytes + 1))
        return ngzs::fail(o, NGZ_E_NOMEM, "harvester buffers");
    std::vector<uint64_t> h_meta(n_meta, 0);
    uint32_t *h_rows = (uint32_t *)(h_meta.data() + S);
    for (uint32_t s = 0; s < S; ++s) {
        h_meta[s] = slot_off[s];
        h_rows[s] = slot_rows[s];
    }
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->d_meta.p, h_meta.data(), n_meta * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_counters.p, 0, n_counters * sizeof(unsigned long long), st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_rowset.p, 0, (n_rows + 1) * sizeof(uint32_t), st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_size.p, 0, (n_rows + 1) * sizeof(unsigned long long), st));
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
    {
        const uint64_t items = std::max<uint64_t>(NS, D);
        const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + OP_THREADS - 1) / OP_THREADS, (uint64_t)o->n_cus * 8));
        hipLaunchKernelGGL(k_options_sets, dim3(nb), dim3(OP_THREADS), 0, st, out->sets, NS, out->dgrams, D, S,
                           (const uint32_t *)(o->d_meta.p + S), (const uint64_t *)o->d_meta.p, o->d_rowset.p, o->d_counters.p);
        NGZ_STAGE_HIP(o, hipGetLastError());
        ++o->launches;
    }
    auto grid = [&](uint32_t rows) {
        return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)rows + OP_THREADS - 1) / OP_THREADS, (uint64_t)o->n_cus * 16));
    };
    for (uint32_t s = 0; s < S; ++s) {
        SlotWork &w = work[s];
        if (!w.packs) continue;
        w.k.rowset = o->d_rowset.p + w.row0;
        w.k.size = o->d_size.p + w.row0;
        w.k.offs = o->d_offs.p + w.row0;
        w.k.sets = out->sets;
        w.k.hdr = out->dgrams;
        w.k.bytes = ctx->last_in.bytes;
        w.k.bytes_size = ctx->last_in.bytes_size;
        w.k.counters = o->d_counters.p;
        hipLaunchKernelGGL(k_options_rows, dim3(grid(w.k.n_rows)), dim3(OP_THREADS), 0, st, w.k);
        NGZ_STAGE_HIP(o, hipGetLastError());
        ++o->launches;
    }
    if (n_rows) {
        NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, scan_bytes, o->d_size.p, o->d_offs.p, (int)(n_rows + 1), st));
        ++o->launches;
    }
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
    std::vector<unsigned long long> h_counters(n_counters, 0);
    unsigned long long total = 0;
    NGZ_STAGE_HIP(o, hipMemcpyAsync(h_counters.data(), o->d_counters.p, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (n_rows) NGZ_STAGE_HIP(o, hipMemcpyAsync(&total, o->d_offs.p + n_rows, sizeof total, hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    float ms = 0;
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&ms, o->ev[0], o->ev[1]));
    o->harvest_ms = ms;
    if (h_counters[C_ERR] & ERR_SETS) return ngzs::fail_sets(o);
    if (h_counters[C_ERR] & ERR_VLEN) return ngzs::fail(o, NGZ_E_INVALID, "a variable-length cell outside the batch input");
    if (total >> 32) return ngzs::fail(o, NGZ_E_LIMIT, "more than 4 GiB of operations in one batch");

    bs.received_flows = h_counters[C_OK_DGRAMS];
    bs.operations_generated = h_counters[C_OPS];
    bs.normalization_errors = h_counters[C_ID_ERRORS];
    for (uint32_t s = 0; s < S; ++s) {
        if (slot_off[s] == SLOT_NOT_OPTIONS) continue;
        const uint64_t live = h_counters[C_SLOT0 + s];
        bs.processed_options_records += live;
        if (work[s].outcome == NGZ_OPTIONS_OUT_CONVERSION) bs.netflow_v9_conversion_errors += live;
        if (work[s].outcome == NGZ_OPTIONS_OUT_MISSING) bs.normalization_errors += live;
    }

    if (total) {
        if (o->d_packed.ensure(total + 4)) return ngzs::fail(o, NGZ_E_NOMEM, "packed operations");
        o->h_packed.resize(total);
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[2], st));
        for (uint32_t s = 0; s < S; ++s) {
            SlotWork &w = work[s];
            if (!w.packs) continue;
            w.k.packed = o->d_packed.p;
            w.k.total = total;
            hipLaunchKernelGGL(k_options_pack, dim3(grid(w.k.n_rows)), dim3(OP_THREADS), 0, st, w.k);
            NGZ_STAGE_HIP(o, hipGetLastError());
            ++o->launches;
        }
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[3], st));
        NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_packed.data(), o->d_packed.p, total, hipMemcpyDeviceToHost, st));
        NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
        NGZ_STAGE_HIP(o, hipEventElapsedTime(&ms, o->ev[2], o->ev[3]));
        o->harvest_ms += ms;

        // the records of all slots, then stream order: set index, record in the set, operation
        struct Rec {
            uint64_t ord;
            uint32_t op;
            uint64_t at;
        };
        std::vector<Rec> recs;
        size_t n_values = 0;
        for (uint64_t at = 0; at < total;) {
            uint32_t head[OP_HEADER_WORDS];
            if (total - at < sizeof head) return ngzs::fail(o, NGZ_E_DEVICE, "packed operations: a truncated record");
            memcpy(head, o->h_packed.data() + at, sizeof head);
            const uint32_t s = head[4] & 0xFFFFu, op = head[4] >> 16;
            if (s >= S || op >= hplan[s].n_ops || head[0] < 4u * (OP_HEADER_WORDS + hplan[s].v[op].size()) || head[0] > total - at ||
                (head[0] & 3u))
                return ngzs::fail(o, NGZ_E_DEVICE, "packed operations: a malformed record");
            recs.push_back(Rec{((uint64_t)head[1] << 32) | head[2], op, at});
            n_values += hplan[s].v[op].size();
            at += head[0];
        }
        if (recs.size() != bs.operations_generated) return ngzs::fail(o, NGZ_E_DEVICE, "packed operations: count mismatch");
        std::sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.ord != b.ord ? a.ord < b.ord : a.op < b.op; });
        o->op_fields.assign(n_values + 1, ngz_enrich_field{});
        o->ops.reserve(recs.size());
        size_t fpos = 0;
        for (const Rec &r : recs) {
            const uint8_t *p = o->h_packed.data() + r.at;
            uint32_t head[OP_HEADER_WORDS];
            memcpy(head, p, sizeof head);
            const HostSlotPlan &hp = hplan[head[4] & 0xFFFFu];
            const std::vector<HostValue> &hv = hp.v[r.op];
            const uint8_t *val = p + 4ull * (OP_HEADER_WORDS + hv.size());
            const uint8_t *const end = p + head[0];
            ngz_enrich_field *f0 = o->op_fields.data() + fpos;
            for (size_t i = 0; i < hv.size(); ++i) {
                uint32_t len;
                memcpy(&len, p + 4ull * (OP_HEADER_WORDS + i), 4);
                if (len > (size_t)(end - val)) return ngzs::fail(o, NGZ_E_DEVICE, "packed operations: a value past its record");
                ngz_enrich_field &f = f0[i];
                f.pen = hv[i].pen;
                f.ie_id = hv[i].ie;
                f.kind = hv[i].kind;
                f.len = len;
                f.value = val;
                val += len;
            }
            fpos += hv.size();
            ngz_enrich_operation op{};
            op.kind = NGZ_ENRICH_UPSERT;
            op.weight = o->weight;
            op.peer = *peer;
            op.obs_domain_id = head[3];
            op.n_scope = hp.n_scope[r.op];
            op.n_fields = (uint32_t)hv.size() - op.n_scope;
            op.scope = f0;
            op.fields = f0 + op.n_scope;
            o->ops.push_back(op);
        }
    }
    add_stats(o->totals, bs);
    if (batch_stats) *batch_stats = bs;
    return NGZ_OK;
}

uint64_t ngz_options_op_count(ngz_options *o) { return o ? o->ops.size() : 0; }

int ngz_options_op(ngz_options *o, uint64_t i, ngz_enrich_operation *op) {
    if (!o || !op) return NGZ_E_INVALID;
    if (i >= o->ops.size()) return ngzs::fail(o, NGZ_E_INVALID, "no such operation");
    *op = o->ops[i];
    return NGZ_OK;
}

int ngz_options_feed(ngz_options *o, ngz_enrich *enricher, uint64_t *n_applied) {
    if (n_applied) *n_applied = 0;
    if (!o || !enricher) return NGZ_E_INVALID;
    uint64_t applied = 0;
    for (const ngz_enrich_operation &op : o->ops) {
        const int rc = ngz_enrich_op(enricher, &op);
        if (rc == NGZ_E_LIMIT) {
            ++o->totals.ops_refused;
            continue;
        }
        if (rc) return ngzs::fail(o, rc, std::string("ngz_enrich_op: ") + ngz_enrich_last_error(enricher));
        ++applied;
        if (n_applied) *n_applied = applied;
    }
    return NGZ_OK;
}

int ngz_options_totals(ngz_options *o, ngz_options_stats *totals, int reset) {
    if (!o || !totals) return NGZ_E_INVALID;
    *totals = o->totals;
    if (reset) o->totals = ngz_options_stats{};
    return NGZ_OK;
}

int ngz_options_last_timing(ngz_options *o, float *harvest_ms) {
    if (!o || !harvest_ms) return NGZ_E_INVALID;
    *harvest_ms = o->harvest_ms;
    return NGZ_OK;
}

int ngz_options_last_launches(ngz_options *o) { return o ? o->launches : NGZ_E_INVALID; }

}  // extern "C"
