// Flow renormalization (include/ngz/flow_renormalize.h): the reference's renormalize()
// (crates/collector/src/flow/renormalization/logic.rs:381-524) applied in place to the decoded
// columns of a batch.  One plan-driven streaming kernel per template slot that carries a
// sampling IE: lanes map to consecutive rows (four per lane), every column access is a
// coalesced vector load / store; the per-record arithmetic is ngz_renorm_math.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ngz/flow_renormalize.h"
#include "ngz_enrich_internal.h"
#include "ngz_host.h"
#include "ngz_renorm_internal.h"
#include "ngz_renorm_math.h"
#include "ngz_stage.h"
#include "ngz_template_record.h"

namespace {

constexpr uint32_t RN_THREADS = 256;
constexpr uint32_t RN_ROWS_PER_LANE = 4;
constexpr uint32_t RN_MAX_OV = 16;  // added sampling columns of an enrichment one slot may carry
constexpr uint32_t RN_STATS = 3;  // device counters: renormalized, missing_or_invalid, inferred

// What the kernel needs of one slot, passed by value
struct RnPlan {
    const uint8_t *param[NGZ_RN_NPARAMS];  // column of the parameter's last occurrence, or null
    uint64_t *count[NGZ_RENORM_MAX_COUNTS];
    uint32_t n_counts;
    uint32_t present;            // bit i: parameter i is in the template
    uint32_t n_rows;             // the slot's n_records
    uint32_t reserved;
    uint8_t *flags;              // one byte per row (room for a whole last quad)
    const uint32_t *bad;         // one bit per row: row of a message that did not decode
    unsigned long long *stats;   // [RN_STATS]
    // ngz_renorm_apply_enriched: the enrichment's added columns of sampling IEs, in ascending
    // FieldRef (appended fields come last, so a later one overrides: logic.rs:327-341)
    uint32_t n_ov;
    uint32_t reserved2;
    const uint32_t *ov_mask;     // the enrichment's presence word per row
    const uint8_t *ov_col[RN_MAX_OV];
    uint8_t ov_param[RN_MAX_OV];
    uint8_t ov_bit[RN_MAX_OV];
};

// IE -> parameter index, its column width (field_rule's for the IE's data type), or -1
int param_index(uint16_t ie, uint16_t *width) {
    static const struct { uint16_t ie, w; } T[NGZ_RN_NPARAMS] = {{34, 4}, {35, 1}, {49, 1}, {50, 4}, {304, 2},
                                                                 {305, 4}, {306, 4}, {309, 4}, {310, 4}, {311, 8}};
    for (int i = 0; i < NGZ_RN_NPARAMS; ++i)
        if (T[i].ie == ie) { *width = T[i].w; return i; }
    return -1;
}
bool is_count_ie(uint16_t ie) { return ie == 1 || ie == 2 || ie == 85 || ie == 86; }

// Bit masks of the parameters by column width
constexpr uint32_t RN_W1 = (1u << NGZ_RN_P35) | (1u << NGZ_RN_P49);
constexpr uint32_t RN_W2 = 1u << NGZ_RN_P304;

__global__ __launch_bounds__(RN_THREADS) void k_renorm(const RnPlan P) {
    __shared__ unsigned long long acc[RN_STATS];
    uint32_t n_renorm = 0, n_invalid = 0, n_inferred = 0;
    const uint32_t quads = (P.n_rows + RN_ROWS_PER_LANE - 1) / RN_ROWS_PER_LANE;
    for (uint32_t q = blockIdx.x * RN_THREADS + threadIdx.x; q < quads; q += gridDim.x * RN_THREADS) {
        const uint32_t r0 = q * RN_ROWS_PER_LANE;
        // rows of this quad that are records of a decoded message (r0 % 4 == 0: one bitmap word)
        uint32_t live = ~(P.bad[r0 >> 5] >> (r0 & 31)) & 0xFu;
        if (P.n_rows - r0 < RN_ROWS_PER_LANE) live &= (1u << (P.n_rows - r0)) - 1u;
        NgzRenormParams prm[RN_ROWS_PER_LANE];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            prm[j] = NgzRenormParams{};
            prm[j].present = P.present;
        }
        // a quad's loads stay inside the column: the capacity is a multiple of 4 rows
#define RN_PARAM(IDX, MEMBER)                                                                       \
    if (P.present & (1u << (IDX))) {                                                                \
        uint32_t v[4];                                                                              \
        ngzs::load4(P.param[IDX], ((1u << (IDX)) & RN_W1) ? 1u : ((1u << (IDX)) & RN_W2) ? 2u : 4u, r0, v); \
        prm[0].MEMBER = v[0]; prm[1].MEMBER = v[1]; prm[2].MEMBER = v[2]; prm[3].MEMBER = v[3];      \
    }
        RN_PARAM(NGZ_RN_P34, interval34)
        RN_PARAM(NGZ_RN_P35, algorithm35)
        RN_PARAM(NGZ_RN_P49, mode49)
        RN_PARAM(NGZ_RN_P50, interval50)
        RN_PARAM(NGZ_RN_P304, selector304)
        RN_PARAM(NGZ_RN_P305, interval305)
        RN_PARAM(NGZ_RN_P306, space306)
        RN_PARAM(NGZ_RN_P309, size309)
        RN_PARAM(NGZ_RN_P310, population310)
#undef RN_PARAM
        if (P.present & (1u << NGZ_RN_P311)) {
            const double2 a = *(const double2 *)(P.param[NGZ_RN_P311] + 8ull * r0);
            const double2 b = *(const double2 *)(P.param[NGZ_RN_P311] + 8ull * r0 + 16);
            prm[0].probability311 = a.x; prm[1].probability311 = a.y;
            prm[2].probability311 = b.x; prm[3].probability311 = b.y;
        }
        if (P.n_ov) {  // a row's value is the added column's where its presence bit is set
            const uint4 mk = *(const uint4 *)(P.ov_mask + r0);  // the mask buffer is padded to a quad
            const uint32_t mk4[4] = {mk.x, mk.y, mk.z, mk.w};
            for (uint32_t o = 0; o < P.n_ov; ++o) {
                const uint32_t pi = P.ov_param[o], bit = P.ov_bit[o];
                uint32_t v[4] = {0, 0, 0, 0};
                double dv[4] = {0, 0, 0, 0};
                if (pi == NGZ_RN_P311) {
                    const double2 a = *(const double2 *)(P.ov_col[o] + 8ull * r0);
                    const double2 b = *(const double2 *)(P.ov_col[o] + 8ull * r0 + 16);
                    dv[0] = a.x; dv[1] = a.y; dv[2] = b.x; dv[3] = b.y;
                } else {
                    ngzs::load4(P.ov_col[o], ((1u << pi) & RN_W1) ? 1u : ((1u << pi) & RN_W2) ? 2u : 4u, r0, v);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!((mk4[j] >> bit) & 1u)) continue;
                    prm[j].present |= 1u << pi;
                    switch (pi) {
                    case NGZ_RN_P34: prm[j].interval34 = v[j]; break;
                    case NGZ_RN_P35: prm[j].algorithm35 = v[j]; break;
                    case NGZ_RN_P49: prm[j].mode49 = v[j]; break;
                    case NGZ_RN_P50: prm[j].interval50 = v[j]; break;
                    case NGZ_RN_P304: prm[j].selector304 = v[j]; break;
                    case NGZ_RN_P305: prm[j].interval305 = v[j]; break;
                    case NGZ_RN_P306: prm[j].space306 = v[j]; break;
                    case NGZ_RN_P309: prm[j].size309 = v[j]; break;
                    case NGZ_RN_P310: prm[j].population310 = v[j]; break;
                    default: prm[j].probability311 = dv[j]; break;
                    }
                }
            }
        }
        double k[RN_ROWS_PER_LANE];
        uint32_t scale = 0;  // rows with a factor
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const NgzRenormFactor f = ngz_renorm_factor(prm[j]);
            k[j] = f.k;
            if ((live >> j) & 1u) {
                n_invalid += f.invalid;
                n_inferred += f.inferred;
                if (f.has_k) scale |= 1u << j;
            }
        }
        const bool whole = P.n_rows - r0 >= RN_ROWS_PER_LANE;
        if (scale) {
            for (uint32_t c = 0; c < P.n_counts; ++c) {
                uint64_t *col = P.count[c] + r0;
                if (whole) {
                    ulonglong2 a = *(const ulonglong2 *)col, b = *(const ulonglong2 *)(col + 2);
                    if (scale & 1u) a.x = ngz_renorm_scale(a.x, k[0]);
                    if (scale & 2u) a.y = ngz_renorm_scale(a.y, k[1]);
                    if (scale & 4u) b.x = ngz_renorm_scale(b.x, k[2]);
                    if (scale & 8u) b.y = ngz_renorm_scale(b.y, k[3]);
                    *(ulonglong2 *)col = a;
                    *(ulonglong2 *)(col + 2) = b;
                } else {  // the slot's last rows: nothing past n_rows is written
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if ((scale >> j) & 1u) col[j] = ngz_renorm_scale(col[j], k[j]);
                }
            }
        }
        const uint32_t flagged = P.n_counts ? scale : 0u;
        n_renorm += __popc(flagged);
        // the flags of four rows in one dword store
        *(uint32_t *)(P.flags + r0) = (flagged & 1u) | ((flagged & 2u) << 7) | ((flagged & 4u) << 14) | ((flagged & 8u) << 21);
    }
    const uint64_t cnt[RN_STATS] = {n_renorm, n_invalid, n_inferred};
    unsigned long long *const dst[RN_STATS] = {&P.stats[0], &P.stats[1], &P.stats[2]};
    ngzs::block_add<RN_STATS>(acc, cnt, dst);
}

// Rows of messages that did not decode (the final status is on the device after decode, k_counts;
// the aggregation push selects rows by datagram the same way): one thread per data set marks its
// rows in the slot's bitmap and counts them.  err bit 0: a set outside the batch's tables.
__global__ void k_renorm_sets(const ngz_set_info *__restrict__ sets, uint32_t n_sets, const ngz_dgram_hdr *__restrict__ hdr,
                              uint32_t n_dgrams, uint32_t n_slots, const uint32_t *__restrict__ slot_rows,
                              const uint32_t *__restrict__ bm_off, uint32_t *__restrict__ bitmap,
                              unsigned long long *__restrict__ bad_rows, unsigned int *__restrict__ err) {
    ngzs::for_each_set(sets, n_sets, hdr, n_dgrams, n_slots, slot_rows, err, [&](uint32_t, const ngz_set_info &si, const ngz_dgram_hdr &h) {
        if (h.status == NGZ_DG_OK) return;
        atomicAdd(&bad_rows[si.slot], (unsigned long long)si.n);
        uint32_t *bm = bitmap + bm_off[si.slot];
        uint32_t r = si.rec0;
        const uint32_t e = si.rec0 + si.n;
        while (r < e) {
            const uint32_t w = r >> 5, lo = r & 31u;
            const uint32_t hi = (e - (w << 5)) < 32u ? e - (w << 5) : 32u;
            const uint32_t mask = (hi == 32u ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
            atomicOr(&bm[w], mask);
            r = (w + 1u) << 5;
        }
    });
}

// One field of a template as the plan builder sees it
struct PlanField {
    uint32_t pen;
    uint16_t ie;
    bool scope;
    bool usable;  // decodes into the column the kernel expects (the IE's width, NGZ_K_UINT)
};

// ngz_renorm_plan of a template's fields (scope first); false: more count fields than the plan holds
bool build_plan(const std::vector<PlanField> &fields, ngz_renorm_plan *out) {
    memset(out, 0, sizeof *out);
    for (int i = 0; i < NGZ_RN_NPARAMS; ++i) out->param_field[i] = -1;
    bool any_param = false, fits = true;
    for (size_t i = 0; i < fields.size(); ++i) {
        const PlanField &f = fields[i];
        if (f.scope) { out->dropped = 1; continue; }
        if (f.pen != 0 || !f.usable) continue;
        uint16_t w;
        const int pi = param_index(f.ie, &w);
        if (pi >= 0) {  // the last occurrence wins (logic.rs:327-341)
            out->param_field[pi] = (int16_t)i;
            any_param = true;
        } else if (is_count_ie(f.ie)) {
            if (out->n_counts < NGZ_RENORM_MAX_COUNTS) out->count_field[out->n_counts++] = (uint16_t)i;
            else fits = false;
        }
    }
    out->launches = (!out->dropped && any_param) ? 1 : 0;
    return fits || out->dropped || !any_param;
}

}  // namespace

struct ngz_renorm : ngzs::Stage {
    ngz_renorm() : Stage(2) {}
    ngz_renorm_stats totals{};
    std::map<const ngz_ctx *, uint64_t> applied;  // context -> batch serial last applied
    // the batch last applied
    const ngz_ctx *last_ctx = nullptr;
    uint64_t last_serial = 0;
    std::vector<uint64_t> flag_off;   // per slot: offset of its flags in d_flags
    std::vector<uint32_t> slot_rows;  // per slot: n_records
    ngzh::DevBuf<uint8_t> d_flags;
    ngzh::DevBuf<uint32_t> d_bitmap;
    ngzh::DevBuf<uint32_t> d_meta;               // slot_rows[S], bm_off[S]
    ngzh::DevBuf<unsigned long long> d_counters;  // stats[RN_STATS], err, bad_rows[S]
    ngzs::PinnedBuf<uint32_t> h_meta;
    ngzs::PinnedBuf<unsigned long long> h_counters;
    float apply_ms = 0;
};

extern "C" {

int ngz_renorm_abi_version(void) { return NGZ_RENORM_ABI_VERSION; }

int ngz_renorm_create(int device, ngz_renorm **out) {
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    ngz_renorm *r = new ngz_renorm;
    r->device = device;
    if (ngzs::device_init(r)) {  // a renormalizer takes its device at creation
        delete r;
        return NGZ_E_DEVICE;
    }
    *out = r;
    return NGZ_OK;
}

void ngz_renorm_destroy(ngz_renorm *r) {
    if (!r) return;
    hipSetDevice(r->device);
    r->d_flags.release();
    r->d_bitmap.release();
    r->d_meta.release();
    r->d_counters.release();
    delete r;
}

const char *ngz_renorm_last_error(ngz_renorm *r) { return r ? r->last_error.c_str() : "null renormalizer"; }

}  // extern "C"

// ngz_renorm_apply, and with `enriched` (an enricher's results for this batch) ngz_renorm_apply_enriched
static int renorm_apply(ngz_renorm *r, const std::vector<ngze::SlotResult> *enriched, ngz_ctx *ctx, const ngz_batch_out *out,
                        ngz_renorm_stats *batch_stats, void *hip_stream) {
    if (!r || !ctx || !out) return NGZ_E_INVALID;
    if (batch_stats) memset(batch_stats, 0, sizeof *batch_stats);
    if (int rc = ngzs::check_ctx(r, ctx)) return rc;
    {
        auto it = r->applied.find(ctx);
        if (it != r->applied.end() && it->second == ctx->batch_serial)
            return ngzs::fail(r, NGZ_E_INVALID, "this batch was already renormalized");
    }
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    if (!ngzs::slot_table_ok(out)) return ngzs::fail(r, NGZ_E_INVALID, "slot table");
    NGZ_STAGE_HIP(r, hipSetDevice(r->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;

    // per-slot plans from the slot's column layout; nothing is launched before every slot checked out
    struct SlotWork {
        ngz_renorm_plan plan;
        RnPlan k;
    };
    std::vector<SlotWork> work(S);
    std::vector<ngz_field_info> fi;
    std::vector<PlanField> pf;
    std::vector<uint64_t> flag_off(S, 0);
    std::vector<uint32_t> slot_rows(S, 0), bm_off(S, 0);
    uint64_t flag_bytes = 0, bm_words = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const ngz_slot_info &si = out->slots[s];
        SlotWork &w = work[s];
        memset(&w, 0, sizeof w);
        slot_rows[s] = si.n_records;
        flag_off[s] = flag_bytes;
        bm_off[s] = (uint32_t)bm_words;
        flag_bytes += ((uint64_t)si.n_records + 15) & ~15ull;  // 16-byte aligned, room for a last quad
        bm_words += ((uint64_t)si.n_records + 31) / 32 + 1;
        if (!si.n_records) continue;
        const int nf = ngzs::slot_fields(r, ctx, s, fi);
        if (nf < 0) return nf;
        pf.resize(nf);
        for (int i = 0; i < nf; ++i) {
            uint16_t pw = 0;
            const int pi = fi[i].pen == 0 ? param_index(fi[i].ie_id, &pw) : -1;
            const uint16_t want = pi >= 0 ? pw : 8;
            pf[i] = PlanField{fi[i].pen, fi[i].ie_id, fi[i].is_scope != 0, fi[i].kind == NGZ_K_UINT && fi[i].width == want};
        }
        if (!build_plan(pf, &w.plan))
            return ngzs::fail(r, NGZ_E_LIMIT, "a template with more than 64 count fields");
        // the enrichment's added columns of sampling IEs (canonical encoding: NGZ_K_UINT of the IE's width)
        if (enriched && !w.plan.dropped && s < enriched->size() && (*enriched)[s].rows == si.n_records) {
            const ngze::SlotResult &er = (*enriched)[s];
            for (size_t c = 0; c < er.cols.size(); ++c) {
                uint16_t pw = 0;
                const int pi = er.cols[c].pen == 0 ? param_index(er.cols[c].ie_id, &pw) : -1;
                if (pi < 0 || er.cols[c].kind != NGZ_K_UINT || er.cols[c].width != pw || !er.cols[c].data) continue;
                if (w.k.n_ov == RN_MAX_OV) return ngzs::fail(r, NGZ_E_LIMIT, "more than 16 added sampling columns in one slot");
                w.k.ov_col[w.k.n_ov] = er.cols[c].data;
                w.k.ov_param[w.k.n_ov] = (uint8_t)pi;
                w.k.ov_bit[w.k.n_ov] = (uint8_t)c;
                ++w.k.n_ov;
            }
            if (w.k.n_ov) {
                size_t n_count_fields = 0;
                for (const PlanField &f : pf) n_count_fields += !f.scope && f.pen == 0 && f.usable && is_count_ie(f.ie);
                if (n_count_fields > NGZ_RENORM_MAX_COUNTS) return ngzs::fail(r, NGZ_E_LIMIT, "a template with more than 64 count fields");
                w.k.ov_mask = er.mask;
                w.plan.launches = 1;
            }
        }
        if (!w.plan.launches) continue;
        if (!si.columns || ((uintptr_t)si.columns & 15) || (si.capacity & 3) || si.capacity < si.n_records)
            return ngzs::fail(r, NGZ_E_LIMIT, "unexpected column block alignment");
        for (int i = 0; i < NGZ_RN_NPARAMS; ++i) {
            if (w.plan.param_field[i] < 0) continue;
            w.k.param[i] = si.columns + (uint64_t)si.capacity * fi[w.plan.param_field[i]].col_off;
            w.k.present |= 1u << i;
        }
        for (uint32_t c = 0; c < w.plan.n_counts; ++c)
            w.k.count[c] = (uint64_t *)(si.columns + (uint64_t)si.capacity * fi[w.plan.count_field[c]].col_off);
        w.k.n_counts = w.plan.n_counts;
        w.k.n_rows = si.n_records;
    }
    if (flag_bytes >> 32 || bm_words >> 32) return ngzs::fail(r, NGZ_E_LIMIT, "batch too large");
    const size_t n_counters = RN_STATS + 1 + S;
    if (r->d_flags.ensure(flag_bytes + 16) || r->d_bitmap.ensure(bm_words + 1) || r->d_meta.ensure(2ull * S + 2) ||
        r->d_counters.ensure(n_counters) || r->h_meta.reserve(2ull * S + 2) || r->h_counters.reserve(n_counters))
        return ngzs::fail(r, NGZ_E_NOMEM, "renormalizer buffers");
    // from here on the batch counts as applied: the columns may change
    r->applied[ctx] = ctx->batch_serial;
    r->last_ctx = ctx;
    r->last_serial = ctx->batch_serial;
    r->flag_off = flag_off;
    r->slot_rows = slot_rows;
    r->apply_ms = 0;
    ctx->json_view.reset();

    for (uint32_t s = 0; s < S; ++s) {
        r->h_meta.p[s] = slot_rows[s];
        r->h_meta.p[S + s] = bm_off[s];
    }
    NGZ_STAGE_HIP(r, hipEventRecord(r->ev[0], st));
    if (S) NGZ_STAGE_HIP(r, hipMemcpyAsync(r->d_meta.p, r->h_meta.p, 2ull * S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(r, hipMemsetAsync(r->d_counters.p, 0, n_counters * sizeof(unsigned long long), st));
    NGZ_STAGE_HIP(r, hipMemsetAsync(r->d_bitmap.p, 0, (bm_words + 1) * sizeof(uint32_t), st));
    unsigned long long *d_stats = r->d_counters.p, *d_bad = r->d_counters.p + RN_STATS + 1;
    unsigned int *d_err = (unsigned int *)(r->d_counters.p + RN_STATS);
    if (NS && D && S) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(((uint64_t)NS + 255) / 256, (uint64_t)r->n_cus * 8);
        hipLaunchKernelGGL(k_renorm_sets, dim3(nb), dim3(256), 0, st, out->sets, NS, out->dgrams, D, S, r->d_meta.p,
                           r->d_meta.p + S, r->d_bitmap.p, d_bad, d_err);
        NGZ_STAGE_HIP(r, hipGetLastError());
    }
    uint32_t launches = 0;
    for (uint32_t s = 0; s < S; ++s) {
        SlotWork &w = work[s];
        if (!slot_rows[s]) continue;
        uint8_t *flags = r->d_flags.p + flag_off[s];
        if (!w.plan.launches) {  // its flags read 0
            NGZ_STAGE_HIP(r, hipMemsetAsync(flags, 0, ((uint64_t)slot_rows[s] + 15) & ~15ull, st));
            continue;
        }
        w.k.flags = flags;
        w.k.bad = r->d_bitmap.p + bm_off[s];
        w.k.stats = d_stats;
        const uint64_t quads = ((uint64_t)slot_rows[s] + RN_ROWS_PER_LANE - 1) / RN_ROWS_PER_LANE;
        const uint32_t nb = (uint32_t)std::min<uint64_t>((quads + RN_THREADS - 1) / RN_THREADS, (uint64_t)r->n_cus * 16);
        hipLaunchKernelGGL(k_renorm, dim3(nb), dim3(RN_THREADS), 0, st, w.k);
        NGZ_STAGE_HIP(r, hipGetLastError());
        ++launches;
    }
    NGZ_STAGE_HIP(r, hipEventRecord(r->ev[1], st));
    NGZ_STAGE_HIP(r, hipMemcpyAsync(r->h_counters.p, r->d_counters.p, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(r, hipStreamSynchronize(st));
    if (launches) NGZ_STAGE_HIP(r, hipEventElapsedTime(&r->apply_ms, r->ev[0], r->ev[1]));
    const unsigned long long *hc = r->h_counters.p;
    if (hc[RN_STATS] & 1) return ngzs::fail_sets(r);
    ngz_renorm_stats bs{};
    bs.flows_renormalized = hc[0];
    bs.ie_missing_or_invalid = hc[1];
    bs.sampling_algorithm_inferred = hc[2];
    for (uint32_t s = 0; s < S; ++s) {
        if (!slot_rows[s]) continue;
        const uint64_t ok_rows = ngzs::ok_rows(slot_rows[s], hc[RN_STATS + 1 + s]);
        if (work[s].plan.dropped) bs.records_dropped += ok_rows;
        else bs.flows_processed += ok_rows;
    }
    r->totals.flows_processed += bs.flows_processed;
    r->totals.flows_renormalized += bs.flows_renormalized;
    r->totals.ie_missing_or_invalid += bs.ie_missing_or_invalid;
    r->totals.sampling_algorithm_inferred += bs.sampling_algorithm_inferred;
    r->totals.records_dropped += bs.records_dropped;
    if (batch_stats) *batch_stats = bs;
    return NGZ_OK;
}

extern "C" {

int ngz_renorm_apply(ngz_renorm *r, ngz_ctx *ctx, const ngz_batch_out *out, ngz_renorm_stats *batch_stats,
                     void *hip_stream) {
    return renorm_apply(r, nullptr, ctx, out, batch_stats, hip_stream);
}

int ngz_renorm_apply_enriched(ngz_renorm *r, ngz_enrich *e, ngz_ctx *ctx, const ngz_batch_out *out,
                              ngz_renorm_stats *batch_stats, void *hip_stream) {
    if (!r || !e || !ctx || !out) return NGZ_E_INVALID;
    if (batch_stats) memset(batch_stats, 0, sizeof *batch_stats);
    const std::vector<ngze::SlotResult> *res = ngze::results_for(e, ctx);
    if (ngze::enrich_device(e) != r->device) return ngzs::fail(r, NGZ_E_INVALID, "the enricher is on another device");
    if (!res) return ngzs::fail(r, NGZ_E_INVALID, "the enricher has not applied the context's last batch");
    return renorm_apply(r, res, ctx, out, batch_stats, hip_stream);
}

int ngz_renorm_totals(ngz_renorm *r, ngz_renorm_stats *totals, int reset) {
    if (!r || !totals) return NGZ_E_INVALID;
    *totals = r->totals;
    if (reset) r->totals = ngz_renorm_stats{};
    return NGZ_OK;
}

int ngz_renorm_flags(ngz_renorm *r, uint32_t slot, const uint8_t **dev_flags, uint32_t *n) {
    if (!r || !dev_flags || !n) return NGZ_E_INVALID;
    if (!r->last_ctx || slot >= r->slot_rows.size()) return ngzs::fail(r, NGZ_E_INVALID, "no such slot in the batch last applied");
    *dev_flags = r->d_flags.p + r->flag_off[slot];
    *n = r->slot_rows[slot];
    return NGZ_OK;
}

}  // extern "C"

int ngzh::renorm_flags_host(ngz_renorm *r, ngz_ctx *ctx, std::vector<uint8_t> &flags, std::vector<const uint8_t *> &slot_flags) {
    if (r->last_ctx != ctx || r->last_serial != ctx->batch_serial || ctx->async.pending.load())
        return ngzs::fail(r, NGZ_E_INVALID, "the context's last batch is not the batch last applied");
    NGZ_STAGE_HIP(r, hipSetDevice(r->device));
    const size_t S = r->slot_rows.size();
    if (S != ctx->slot_infos.size()) return ngzs::fail(r, NGZ_E_INVALID, "slot table");
    const uint64_t total = S ? r->flag_off[S - 1] + (((uint64_t)r->slot_rows[S - 1] + 15) & ~15ull) : 0;
    flags.assign(total + 1, 0);
    if (total) NGZ_STAGE_HIP(r, hipMemcpy(flags.data(), r->d_flags.p, total, hipMemcpyDeviceToHost));
    slot_flags.assign(S, nullptr);
    for (size_t s = 0; s < S; ++s)
        if (r->slot_rows[s]) slot_flags[s] = flags.data() + r->flag_off[s];
    return NGZ_OK;
}

extern "C" {

int64_t ngz_renorm_batch_json(ngz_renorm *r, ngz_ctx *ctx, const uint8_t *host_bytes, ngz_json_line_fn fn, void *user) {
    if (!r || !ctx || !fn) return NGZ_E_INVALID;
    std::vector<uint8_t> flags;
    ngzh::RenormJson mode;
    if (const int frc = ngzh::renorm_flags_host(r, ctx, flags, mode.slot_flags)) return frc;
    ngzh::JsonView v;
    const int rc = ngzh::json_view_load(ctx, host_bytes, v);
    if (rc) return ngzs::fail(r, rc, "json_view_load");
    int64_t lines = 0;
    std::string s;
    for (uint32_t d = 0; d < ctx->last_in.n; ++d) {
        s.clear();
        uint32_t consumed = 0;
        const int st = ngzh::json_render_mode(ctx, v, d, s, &consumed, &mode);
        if (st < 0) return st;
        if (st != NGZ_DG_OK && st != NGZ_DG_ERROR) continue;
        if (fn(user, d, st, s.data(), s.size(), consumed)) break;
        ++lines;
    }
    return lines;
}

int ngz_renorm_last_timing(ngz_renorm *r, float *apply_ms) {
    if (!r || !apply_ms) return NGZ_E_INVALID;
    *apply_ms = r->apply_ms;
    return NGZ_OK;
}

int ngz_renorm_template_plan(const uint8_t *tmpl, size_t len, int proto, ngz_renorm_plan *out) {
    if (!tmpl || !out) return NGZ_E_INVALID;
    const bool options = (proto & NGZ_RENORM_OPTIONS) != 0;
    proto &= ~NGZ_RENORM_OPTIONS;
    if (proto != 10 && proto != 9) return NGZ_E_INVALID;
    std::vector<PlanField> pf;
    const int rc = ngzt::walk_template_record(tmpl, len, proto, options, [&](const ngzt::FieldSpec &f) {
        const uint32_t L = f.length;
        uint16_t pw = 0;
        const int pi = f.pen == 0 ? param_index(f.ie, &pw) : -1;
        // the lengths field_rule decodes into the IE's full-width column (reduced-size encoding)
        bool usable = false;
        if (pi >= 0) usable = pw == 8 ? L == 8 : pw == 1 ? L == 1 : (L >= 1 && L <= pw);
        else if (f.pen == 0 && is_count_ie(f.ie)) usable = L >= 1 && L <= 8;
        pf.push_back(PlanField{f.pen, f.ie, f.scope, usable});
    });
    if (rc) return rc;
    build_plan(pf, out);
    return NGZ_OK;
}

}  // extern "C"
