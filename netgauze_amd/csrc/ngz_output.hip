// The flow output (include/ngz/flow_output.h): FlowOutputConfig::get_avro_values
// (crates/collector/src/flow/config.rs:105-215) over the decoded columns of a batch, each record's
// datum in the Avro binary encoding.  The config, the schema and the per-template plan are host code
// (ngz_output_plan.cpp); this unit turns a slot's plan into column pointers, passed by value, and runs
//   k_output_sets  one thread per data set: the rows of messages that did not decode,
//   k_output_size  four rows per lane: each row's datum length (vector column loads, one 16-byte store),
//   a hipcub exclusive scan: the u64 offsets,
//   k_output_pack  a wave encodes its 64 consecutive rows into an LDS image laid out like the output
//                  range they fill, and copies the image out in 16-byte stores.
// One set of encoders (templated on a counting or a storing writer, ngz_output_enc.h, shared with
// ngz_agg_output.hip) serves both passes, so the sizes are the packed bytes by construction.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_output.h"
#include "ngz_host.h"
#include "ngz_output_enc.h"
#include "ngz_output_plan.h"
#include "ngz_stage.h"

namespace {

using namespace ngzenc;
using ngzout::Enc;

constexpr uint32_t OUT_THREADS = 256;
constexpr uint32_t OUT_WAVES = OUT_THREADS / 64;
constexpr uint32_t OUT_ROWS_PER_LANE = 4;  // size pass
// A wave's LDS image is IMG bytes and 16 of slack for the output's misalignment.  8176 + 16 per wave is
// 32 KB per block of 4 waves, so five blocks (20 of a CU's 32 waves) fit its 160 KB, and 127 bytes per
// row of a full wave, above the 87.5 of the benchmark's ten-field datum: a wave's rows usually leave
// as one group.  4080 + 16 (16 KB per block) lets the pack kernel's 92 VGPRs decide, five blocks again, but cuts
// every such wave in two.  Measured both (profiles/output/summary.txt): NGZ_OUTPUT_OPT_IMAGE.
constexpr uint32_t OUT_IMG_LARGE = 8176, OUT_IMG_SMALL = 4080;
constexpr uint32_t OUT_DEFAULT_POOL = 1024;  // encoded defaults of one config, in all
constexpr uint32_t C_ERR = 0, C_SLOT0 = 1;   // device counters: error bits, then the failed rows per slot
constexpr uint32_t ERR_SETS = 1, ERR_VLEN = 2;  // ERR_SETS: the bit ngzs::for_each_set sets

enum : uint8_t { M_CELL = 0, M_STR = 1, M_VLEN = 2 };  // OutSource::mode
enum : uint8_t { F_NULLABLE = 1, F_L2 = 2, F_ARRAY = 4, F_MASK40 = 8 };

struct OutSource {
    const uint8_t *col;
    uint16_t width;  // column bytes per row
    uint8_t enc;     // ngzout::Enc
    uint8_t aux;     // ENC_MPLS_ITEM: n
    uint8_t mode;    // M_CELL the cell; M_STR the cell up to its first NUL; M_VLEN {u64 offset, u32 length, u32 0}
    uint8_t reserved[3];
};

struct OutField {
    uint8_t first, n;  // its present sources: src[first, first + n)
    uint8_t flags;
    uint8_t l2_encap;
    uint16_t def_off;  // the default's Avro bytes in defaults[]
    uint8_t def_len;
    uint8_t reserved;
};

// What the size and pack kernels need of one slot, passed by value (3.3 KB of the 4 KB a launch takes)
struct OutPlan {
    OutSource src[NGZ_OUTPUT_MAX_SOURCES];
    OutField f[NGZ_OUTPUT_MAX_FIELDS];
    uint8_t defaults[OUT_DEFAULT_POOL];
    uint32_t n_fields;
    uint32_t n_rows;
    const uint32_t *bad;             // one bit per row: row of a message that did not decode
    uint32_t *lens;                  // per row: its datum's bytes (size pass; whole quads, and one 0 after them)
    const unsigned long long *offs;  // the scanned lengths, n_rows + 1 (pack pass)
    uint8_t *out;                    // the slot's datums
    unsigned long long total;        // their bytes
    const uint8_t *bytes;            // the batch input
    unsigned long long bytes_size;
    unsigned long long *counters;
};

// The cells of rows r0 .. r0 + R - 1 of one source.  R == 4 (r0 a multiple of 4): an integer column
// loads as one dword / 8 / 16 / 2 x 16 bytes that stay inside the column and are aligned: its capacity
// is a multiple of 16 rows (checked by the encode).  Other cells are read for the rows of `live` only; a variable-length cell
// outside the batch input reads as empty and sets ERR_VLEN.
template <int R>
__device__ __forceinline__ void load_cells(const OutPlan &P, const OutSource &S, uint32_t r0, uint32_t live, Cell (&c)[R], uint32_t *err) {
#pragma unroll
    for (int j = 0; j < R; ++j) c[j] = Cell{0, P.bytes, 0};
    if (S.mode == M_CELL && enc_numeric(S.enc)) {
        if constexpr (R == 4) {
            if (S.width == 8) {
                const ulonglong2 a = *(const ulonglong2 *)(S.col + 8ull * r0), b = *(const ulonglong2 *)(S.col + 8ull * r0 + 16);
                c[0].v = a.x; c[1].v = a.y; c[2].v = b.x; c[3].v = b.y;
            } else {
                uint32_t v[4];
                ngzs::load4(S.col, S.width, r0, v);
                c[0].v = v[0]; c[1].v = v[1]; c[2].v = v[2]; c[3].v = v[3];
            }
        } else {
            const uint8_t *cell = S.col + (uint64_t)S.width * r0;
            c[0].v = S.width == 8 ? *(const uint64_t *)cell : S.width == 4 ? *(const uint32_t *)cell
                   : S.width == 2 ? *(const uint16_t *)cell : *cell;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (!((live >> j) & 1u)) continue;
        const uint8_t *cell = S.col + (uint64_t)S.width * (r0 + j);
        if (S.mode == M_CELL) {
            c[j].p = cell;
            c[j].n = S.width;
        } else if (S.mode == M_STR) {
            uint32_t n = 0;
            while (n < S.width && cell[n]) ++n;
            c[j].p = cell;
            c[j].n = n;
        } else {
            const uint64_t off = *(const uint64_t *)cell;
            const uint32_t len = *(const uint32_t *)(cell + 8);
            if (off > P.bytes_size || len > P.bytes_size - off) {
                *err |= ERR_VLEN;
            } else {
                c[j].p = P.bytes + off;
                c[j].n = len;
            }
        }
    }
}

// The datums of rows r0 .. r0 + R - 1 (those of `live`) into w[]: per field select, transform, default
// as FieldConfig::avro_value (config.rs:532-543), then the union branch of a nullable field
template <int R, class W>
__device__ __forceinline__ void encode_rows(const OutPlan &P, uint32_t r0, uint32_t live, W (&w)[R], uint32_t *err) {
    for (uint32_t fi = 0; fi < P.n_fields; ++fi) {
        const OutField F = P.f[fi];
        uint32_t some = F.n ? live : 0u;
        for (uint32_t s = 0; s < (F.n ? F.n : 1u); ++s) {
            Cell c[R];
            if (F.n) load_cells<R>(P, P.src[F.first + s], r0, live, c, err);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (!((live >> j) & 1u)) continue;
                if (s == 0) {
                    if ((F.flags & F_L2) && F.n) {  // Layer2SegmentIdFieldSelect::apply (:746-762)
                        if ((uint8_t)(c[j].v >> 56) != F.l2_encap) some &= ~(1u << j);
                        c[j].v &= (F.flags & F_MASK40) ? 0xFFFFFFFFFFull : 0xFFFFFFull;
                    }
                    if (!((some >> j) & 1u)) {
                        if (F.flags & F_NULLABLE) w[j].put(0);
                        else w[j].bytes(P.defaults + F.def_off, F.def_len);
                        continue;
                    }
                    if (F.flags & F_NULLABLE) w[j].put(2);  // branch 1
                    if (F.flags & F_ARRAY) put_varint(w[j], (uint64_t)F.n << 1);
                }
                if ((some >> j) & 1u) encode_value(w[j], P.src[F.first + s], c[j]);
            }
        }
        if (F.flags & F_ARRAY)
#pragma unroll
            for (int j = 0; j < R; ++j)
                if ((some >> j) & 1u) w[j].put(0);
    }
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// One thread per data set: the rows of a set whose message did not decode, in the slot's bitmap
// and counted per slot
__global__ __launch_bounds__(OUT_THREADS) void k_output_sets(const ngz_set_info *__restrict__ sets, uint32_t n_sets,
                                                            const ngz_dgram_hdr *__restrict__ hdr, uint32_t n_dgrams, uint32_t n_slots,
                                                            const uint32_t *__restrict__ slot_rows, const uint32_t *__restrict__ bm_off,
                                                            uint32_t *__restrict__ bitmap, unsigned long long *__restrict__ counters) {
    ngzs::for_each_set(sets, n_sets, hdr, n_dgrams, n_slots, slot_rows, (unsigned int *)&counters[C_ERR],
                       [&](uint32_t, const ngz_set_info &si, const ngz_dgram_hdr &h) {
        if (h.status == NGZ_DG_OK) return;
        atomicAdd(&counters[C_SLOT0 + si.slot], (unsigned long long)si.n);
        uint32_t *bm = bitmap + bm_off[si.slot];
        const uint32_t e = si.rec0 + si.n;
        for (uint32_t r = si.rec0; r < e;) {
            const uint32_t wd = r >> 5, lo = r & 31u;
            const uint32_t hi = (e - (wd << 5)) < 32u ? e - (wd << 5) : 32u;
            atomicOr(&bm[wd], (hi == 32u ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u));
            r = (wd + 1u) << 5;
        }
    });
}

__global__ __launch_bounds__(OUT_THREADS) void k_output_size(const OutPlan P) {
    const uint32_t quads = (P.n_rows + OUT_ROWS_PER_LANE - 1) / OUT_ROWS_PER_LANE;
    uint32_t err = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) P.lens[quads * OUT_ROWS_PER_LANE] = 0;  // the scan's last item
    for (uint32_t q = blockIdx.x * OUT_THREADS + threadIdx.x; q < quads; q += gridDim.x * OUT_THREADS) {
        const uint32_t r0 = q * OUT_ROWS_PER_LANE;
        uint32_t live = ~(P.bad[r0 >> 5] >> (r0 & 31u)) & 0xFu;  // r0 % 4 == 0: one bitmap word
        if (P.n_rows - r0 < OUT_ROWS_PER_LANE) live &= (1u << (P.n_rows - r0)) - 1u;
        CountW w[OUT_ROWS_PER_LANE];
        encode_rows<OUT_ROWS_PER_LANE>(P, r0, live, w, &err);
        *(uint4 *)(P.lens + r0) = make_uint4(w[0].n, w[1].n, w[2].n, w[3].n);  // 0 for the rows that are not live
    }
    if (err) atomicOr((unsigned int *)&P.counters[C_ERR], err);
}

// IMG: the image's bytes.  RECOMPUTE: a lane sizes its row again and a wave scan places it after the
// tile's first offset, instead of reading the row's two scanned offsets back.
template <uint32_t IMG, bool RECOMPUTE>
__global__ __launch_bounds__(OUT_THREADS) void k_output_pack(const OutPlan P) {
    __shared__ __attribute__((aligned(16))) uint8_t images[OUT_WAVES][IMG + 16];  // pack_tile's, one per wave
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t *const img = images[threadIdx.x >> 6];
    const uint32_t tiles = (P.n_rows + 63u) / 64u;
    uint32_t err = 0;
    for (uint32_t tile = blockIdx.x * OUT_WAVES + (threadIdx.x >> 6); tile < tiles; tile += gridDim.x * OUT_WAVES) {
        const uint32_t row = tile * 64u + lane, nt = min(64u, P.n_rows - tile * 64u);
        unsigned long long base;
        uint32_t rel0, rel1;
        if constexpr (RECOMPUTE) {
            CountW c[1];
            if (lane < nt && !((P.bad[row >> 5] >> (row & 31u)) & 1u)) encode_rows<1>(P, row, 1u, c, &err);
            uint32_t incl = c[0].n;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if (lane >= (uint32_t)d) incl += up;
            }
            base = P.offs[tile * 64u];
            rel1 = incl;
            rel0 = incl - c[0].n;
        } else {
            const unsigned long long a = P.offs[lane < nt ? row : P.n_rows], b = lane < nt ? P.offs[row + 1] : a;
            base = __shfl(a, 0, 64);
            rel0 = (uint32_t)(a - base);
            rel1 = (uint32_t)(b - base);
        }
        pack_tile<IMG>(lane, nt, base, rel0, rel1, P.out, P.total, img, [&](PutW &pw) {
            PutW w[1] = {pw};
            encode_rows<1>(P, row, 1u, w, &err);
        });
    }
    if (err) atomicOr((unsigned int *)&P.counters[C_ERR], err);
}

struct ToU64 {
    __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t v) const { return v; }
};
using LenIter = hipcub::TransformInputIterator<unsigned long long, ToU64, const uint32_t *>;

struct SlotOut {
    const uint8_t *bytes = nullptr;
    const uint64_t *offs = nullptr;
    uint64_t n_rows = 0, n_bytes = 0;
};

}  // namespace

struct ngz_output : ngzs::Stage {
    ngz_output() : Stage(4) {}
    ngzout::Config cfg;
    std::string schema;
    ngz_output_stats totals{};
    float size_ms = 0, pack_ms = 0;
    int launches = 0;
    bool recompute = false;     // NGZ_OUTPUT_OPT_RECOMPUTE
    bool small_image = false;   // NGZ_OUTPUT_OPT_IMAGE 4096
    std::vector<SlotOut> slots;  // the last encode
    ngzh::DevBuf<uint32_t> d_lens, d_bitmap, d_meta;  // d_meta: slot_rows[S], bm_off[S]
    ngzh::DevBuf<unsigned long long> d_offs, d_counters;
    ngzh::DevBuf<uint8_t> d_scan_tmp, d_bytes;
    ngzs::PinnedBuf<unsigned long long> h_back;  // counters, then the slots' totals
};

namespace {

// The column a source of encoding `enc` reads, as the decode laid it out; false: not the column the
// encoders expect
bool source_rule(const ngz_field_info &fi, uint8_t enc, uint8_t *mode) {
    *mode = M_CELL;
    const bool int_w = fi.width == 1 || fi.width == 2 || fi.width == 4 || fi.width == 8;
    switch (enc) {
    case ngzout::ENC_INT_U: case ngzout::ENC_DEC_U: return fi.kind == NGZ_K_UINT && int_w;
    case ngzout::ENC_INT_S: case ngzout::ENC_DEC_S: return fi.kind == NGZ_K_SINT && int_w;
    case ngzout::ENC_RAW: return fi.kind == NGZ_K_UINT && (fi.width == 4 || fi.width == 8);
    case ngzout::ENC_BOOL: case ngzout::ENC_BOOLSTR: return fi.kind == NGZ_K_BOOL && fi.width == 1;
    case ngzout::ENC_IP4: return fi.kind == NGZ_K_UINT && fi.width == 4;
    case ngzout::ENC_MAC: return fi.kind == NGZ_K_BYTES && fi.width == 6;
    case ngzout::ENC_IP6: return fi.kind == NGZ_K_BYTES && fi.width == 16;
    case ngzout::ENC_MPLS_ITEM: return fi.kind == NGZ_K_BYTES && fi.width == 3;
    case ngzout::ENC_STR:
        *mode = fi.kind == NGZ_K_VLEN ? M_VLEN : M_STR;
        return (fi.kind == NGZ_K_VLEN && fi.width == 16) || fi.kind == NGZ_K_STR;
    case ngzout::ENC_BYTES:
        *mode = fi.kind == NGZ_K_VLEN ? M_VLEN : M_CELL;
        return (fi.kind == NGZ_K_VLEN && fi.width == 16) || fi.kind == NGZ_K_BYTES || (fi.kind == NGZ_K_U256 && fi.width == 32);
    }
    return false;
}

}  // namespace

extern "C" {

int ngz_output_abi_version(void) { return NGZ_OUTPUT_ABI_VERSION; }

int ngz_output_create(int device, const ngz_output_field *fields, uint32_t n, ngz_output **out, char *err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0) return NGZ_E_INVALID;
    ngz_output *o = new ngz_output;
    o->device = device;
    std::string why;
    int rc = ngzout::build_config(fields, n, &o->cfg, &why);
    size_t pool = 0;
    for (const ngzout::CfgField &f : o->cfg.fields) pool += f.def.size();
    if (!rc && pool > OUT_DEFAULT_POOL) {
        rc = NGZ_E_LIMIT;
        why = "more than 1024 bytes of encoded defaults";
    }
    if (rc) {
        if (err && err_cap) snprintf(err, err_cap, "%s", why.c_str());
        delete o;
        return rc;
    }
    o->schema = ngzout::schema_text(o->cfg);
    *out = o;
    return NGZ_OK;
}

void ngz_output_destroy(ngz_output *o) {
    if (!o) return;
    if (o->device_ready) {
        hipSetDevice(o->device);
        o->d_lens.release();
        o->d_bitmap.release();
        o->d_meta.release();
        o->d_offs.release();
        o->d_counters.release();
        o->d_scan_tmp.release();
        o->d_bytes.release();
    }
    delete o;
}

const char *ngz_output_last_error(ngz_output *o) { return o ? o->last_error.c_str() : "null output stage"; }

int64_t ngz_output_schema(ngz_output *o, char *buf, size_t cap) {
    if (!o) return NGZ_E_INVALID;
    if (buf && cap) snprintf(buf, cap, "%s", o->schema.c_str());
    return (int64_t)o->schema.size();
}

int ngz_output_set_option(ngz_output *o, int opt, int64_t value) {
    if (!o) return NGZ_E_INVALID;
    if (opt == NGZ_OUTPUT_OPT_RECOMPUTE && (value == 0 || value == 1)) o->recompute = value != 0;
    else if (opt == NGZ_OUTPUT_OPT_IMAGE && (value == 4096 || value == 8192)) o->small_image = value == 4096;
    else return ngzs::fail(o, NGZ_E_INVALID, "no such option or value");
    return NGZ_OK;
}

int ngz_output_template_plan(ngz_output *o, const uint8_t *tmpl, size_t len, int proto, ngz_output_plan *plan) {
    if (!o) return NGZ_E_INVALID;
    return ngzout::template_plan(o->cfg, tmpl, len, proto, plan);
}

int ngz_output_encode(ngz_output *o, ngz_ctx *ctx, const ngz_batch_out *out, ngz_output_stats *batch_stats, void *hip_stream) {
    if (!o || !ctx || !out) return NGZ_E_INVALID;
    if (batch_stats) memset(batch_stats, 0, sizeof *batch_stats);
    if (int rc = ngzs::check_ctx(o, ctx)) return rc;
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    if (!ngzs::slot_table_ok(out) || S != ctx->slot_version.size() || D != ctx->last_in.n)
        return ngzs::fail(o, NGZ_E_INVALID, "slot table: `out` is not the context's last decode");
    o->slots.assign(S, SlotOut{});
    o->launches = 0;
    o->size_ms = o->pack_ms = 0;

    // per-slot plans; nothing touches the device before every slot checked out
    struct SlotWork {
        OutPlan k;
        uint64_t len0 = 0, off0 = 0;  // the slot's lengths in d_lens, offsets in d_offs
        uint32_t bm0 = 0;
    };
    std::vector<SlotWork> work(S);
    std::vector<uint32_t> slot_rows(S, 0);
    std::vector<ngz_field_info> fi;
    std::vector<ngzout::TField> tf;
    std::vector<std::vector<uint8_t>> ref_of;
    uint64_t n_lens = 0, n_offs = 0, bm_words = 0, n_rows = 0, max_rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const ngz_slot_info &si = out->slots[s];
        SlotWork &w = work[s];
        memset(&w.k, 0, sizeof w.k);
        slot_rows[s] = si.n_records;
        w.bm0 = (uint32_t)bm_words;
        bm_words += ((uint64_t)si.n_records + 31) / 32 + 1;
        if (!si.n_records) continue;
        const int nf = ngzs::slot_fields(o, ctx, s, fi);
        if (nf < 0) return nf;
        tf.resize(nf);
        for (int i = 0; i < nf; ++i) tf[i] = ngzout::TField{fi[i].pen, fi[i].ie_id, fi[i].is_scope != 0};
        ngz_output_plan plan;
        if (ngzout::plan_fields(o->cfg, tf, &plan, &ref_of))
            return ngzs::fail(o, NGZ_E_LIMIT, "a template of which the config reads more than 96 columns");
        // every column starts at a multiple of 16 bytes: the size pass's vector loads are aligned
        if (!si.columns || ((uintptr_t)si.columns & 15) || (si.capacity & 15) || si.capacity < si.n_records)
            return ngzs::fail(o, NGZ_E_LIMIT, "unexpected column block alignment");
        uint32_t n_src = 0, def_off = 0;
        for (uint32_t f = 0; f < plan.n_fields; ++f) {
            const ngzout::CfgField &cf = o->cfg.fields[f];
            OutField &df = w.k.f[f];
            df.first = (uint8_t)n_src;
            df.flags = (cf.nullable ? F_NULLABLE : 0) | (cf.select == NGZ_OUT_SEL_L2SEGMENT ? F_L2 : 0) |
                       (cf.avro == NGZ_OUT_T_ARRAY ? F_ARRAY : 0) | (cf.l2_mask > 0xFFFFFFull ? F_MASK40 : 0);
            df.l2_encap = cf.l2_encap;
            df.def_off = (uint16_t)def_off;
            df.def_len = (uint8_t)cf.def.size();
            memcpy(w.k.defaults + def_off, cf.def.data(), cf.def.size());
            def_off += (uint32_t)cf.def.size();
            for (uint32_t i = 0; i < plan.f[f].n_present; ++i) {
                const ngz_field_info &src = fi[plan.f[f].src[i]];
                const ngzout::CfgRef &ref = cf.refs[ref_of[f][i]];
                if (src.kind == NGZ_K_FAIL) continue;  // no record of this template ever decodes
                OutSource &ds = w.k.src[n_src];
                if (!source_rule(src, ref.enc, &ds.mode))
                    return ngzs::fail(o, NGZ_E_LIMIT, "field " + cf.name + ": a column of a kind the output cannot read");
                ds.col = si.columns + (uint64_t)si.capacity * src.col_off;
                ds.width = src.width;
                ds.enc = ref.enc;
                ds.aux = ref.mpls_n;
                ++n_src;
            }
            df.n = (uint8_t)(n_src - df.first);
        }
        w.k.n_fields = plan.n_fields;
        w.k.n_rows = si.n_records;
        const uint64_t quads = ((uint64_t)si.n_records + OUT_ROWS_PER_LANE - 1) / OUT_ROWS_PER_LANE;
        w.len0 = n_lens;
        w.off0 = n_offs;
        n_lens += quads * OUT_ROWS_PER_LANE + 4;  // whole quads and the scan's last item, 16-byte aligned
        n_offs += (uint64_t)si.n_records + 2;
        n_rows += si.n_records;
        max_rows = std::max<uint64_t>(max_rows, si.n_records);
    }
    ngz_output_stats bs{};
    if (!n_rows) {  // no row: no kernel
        if (batch_stats) *batch_stats = bs;
        return NGZ_OK;
    }
    if (max_rows >> 31 || bm_words >> 32) return ngzs::fail(o, NGZ_E_LIMIT, "batch too large");
    if (int rc = ngzs::device_init(o)) return rc;
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;

    const size_t n_counters = C_SLOT0 + S, n_back = n_counters + S;
    size_t scan_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, LenIter((const uint32_t *)nullptr, ToU64()), (unsigned long long *)nullptr,
                                         (int)(max_rows + 1), st) != hipSuccess)
        return ngzs::fail(o, NGZ_E_DEVICE, "scan temp size");
    if (o->d_lens.ensure(n_lens + 4) || o->d_offs.ensure(n_offs + 2) || o->d_bitmap.ensure(bm_words + 1) || o->d_meta.ensure(2ull * S + 2) ||
        o->d_counters.ensure(n_counters) || o->d_scan_tmp.ensure(scan_bytes + 1) || o->h_back.reserve(n_back))
        return ngzs::fail(o, NGZ_E_NOMEM, "output stage buffers");
    std::vector<uint32_t> h_meta(2ull * S);
    for (uint32_t s = 0; s < S; ++s) {
        h_meta[s] = slot_rows[s];
        h_meta[S + s] = work[s].bm0;
    }
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->d_meta.p, h_meta.data(), h_meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_counters.p, 0, n_counters * sizeof(unsigned long long), st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_bitmap.p, 0, (bm_words + 1) * sizeof(uint32_t), st));
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
    if (NS && D) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(((uint64_t)NS + OUT_THREADS - 1) / OUT_THREADS, (uint64_t)o->n_cus * 8);
        hipLaunchKernelGGL(k_output_sets, dim3(nb), dim3(OUT_THREADS), 0, st, out->sets, NS, out->dgrams, D, S, o->d_meta.p,
                           o->d_meta.p + S, o->d_bitmap.p, o->d_counters.p);
        NGZ_STAGE_HIP(o, hipGetLastError());
        ++o->launches;
    }
    auto grid = [&](uint64_t items) {
        return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + OUT_THREADS - 1) / OUT_THREADS, (uint64_t)o->n_cus * 16));
    };
    for (uint32_t s = 0; s < S; ++s) {
        SlotWork &w = work[s];
        if (!slot_rows[s]) continue;
        w.k.bad = o->d_bitmap.p + w.bm0;
        w.k.lens = o->d_lens.p + w.len0;
        w.k.offs = o->d_offs.p + w.off0;
        w.k.bytes = ctx->last_in.bytes;
        w.k.bytes_size = ctx->last_in.bytes_size;
        w.k.counters = o->d_counters.p;
        hipLaunchKernelGGL(k_output_size, dim3(grid(((uint64_t)slot_rows[s] + 3) / 4)), dim3(OUT_THREADS), 0, st, w.k);
        NGZ_STAGE_HIP(o, hipGetLastError());
        NGZ_STAGE_HIP(o, hipcub::DeviceScan::ExclusiveSum(o->d_scan_tmp.p, scan_bytes, LenIter(w.k.lens, ToU64()), o->d_offs.p + w.off0,
                                                          (int)(slot_rows[s] + 1), st));
        o->launches += 2;
    }
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
    // the counters and each slot's total, read back at the size passes' completion
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p, o->d_counters.p, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    for (uint32_t s = 0; s < S; ++s) {
        o->h_back.p[n_counters + s] = 0;
        if (slot_rows[s])
            NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p + n_counters + s, o->d_offs.p + work[s].off0 + slot_rows[s], sizeof(unsigned long long),
                                            hipMemcpyDeviceToHost, st));
    }
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->size_ms, o->ev[0], o->ev[1]));
    const unsigned long long *hc = o->h_back.p;
    if (hc[C_ERR] & ERR_SETS) return ngzs::fail_sets(o);
    if (hc[C_ERR] & ERR_VLEN) return ngzs::fail(o, NGZ_E_INVALID, "a variable-length cell outside the batch input");

    // the slots' datums: each at a multiple of 16 bytes, its guard after it
    uint64_t n_bytes = 0;
    std::vector<uint64_t> base(S, 0);
    for (uint32_t s = 0; s < S; ++s) {
        base[s] = n_bytes;
        if (slot_rows[s]) n_bytes += (hc[n_counters + s] + NGZ_OUTPUT_GUARD + 15) & ~15ull;
    }
    if (o->d_bytes.ensure(n_bytes + 16)) return ngzs::fail(o, NGZ_E_NOMEM, "output bytes");
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[2], st));
    bool packed = false;
    for (uint32_t s = 0; s < S; ++s) {
        if (!slot_rows[s]) continue;
        SlotWork &w = work[s];
        const unsigned long long total = hc[n_counters + s];
        w.k.out = o->d_bytes.p + base[s];
        w.k.total = total;
        NGZ_STAGE_HIP(o, hipMemsetAsync(w.k.out + total, 0xA5, NGZ_OUTPUT_GUARD, st));
        o->slots[s] = SlotOut{w.k.out, (const uint64_t *)w.k.offs, slot_rows[s], total};
        bs.rows += slot_rows[s];
        bs.rows_failed += std::min<uint64_t>(slot_rows[s], hc[C_SLOT0 + s]);
        bs.bytes += total;
        if (!total) continue;
        const uint64_t tiles = ((uint64_t)slot_rows[s] + 63) / 64;
        const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((tiles + OUT_WAVES - 1) / OUT_WAVES, (uint64_t)o->n_cus * 16));
        auto *pack = o->small_image ? (o->recompute ? k_output_pack<OUT_IMG_SMALL, true> : k_output_pack<OUT_IMG_SMALL, false>)
                                    : (o->recompute ? k_output_pack<OUT_IMG_LARGE, true> : k_output_pack<OUT_IMG_LARGE, false>);
        hipLaunchKernelGGL(pack, dim3(nb), dim3(OUT_THREADS), 0, st, w.k);
        NGZ_STAGE_HIP(o, hipGetLastError());
        ++o->launches;
        packed = true;
    }
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[3], st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->h_back.p, o->d_counters.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(o, hipStreamSynchronize(st));
    if (packed) NGZ_STAGE_HIP(o, hipEventElapsedTime(&o->pack_ms, o->ev[2], o->ev[3]));
    if (o->h_back.p[C_ERR] & ERR_VLEN) return ngzs::fail(o, NGZ_E_INVALID, "a variable-length cell outside the batch input");
    o->totals.rows += bs.rows;
    o->totals.rows_failed += bs.rows_failed;
    o->totals.bytes += bs.bytes;
    if (batch_stats) *batch_stats = bs;
    return NGZ_OK;
}

int ngz_output_slot(ngz_output *o, uint32_t slot, const uint8_t **bytes, const uint64_t **offsets, uint64_t *n_rows, uint64_t *n_bytes) {
    if (!o) return NGZ_E_INVALID;
    if (slot >= o->slots.size()) return ngzs::fail(o, NGZ_E_INVALID, "no such slot in the last encode");
    const SlotOut &so = o->slots[slot];
    if (bytes) *bytes = so.bytes;
    if (offsets) *offsets = so.offs;
    if (n_rows) *n_rows = so.n_rows;
    if (n_bytes) *n_bytes = so.n_bytes;
    return NGZ_OK;
}

int ngz_output_to_host(ngz_output *o, uint32_t slot, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap) {
    if (!o) return NGZ_E_INVALID;
    if (slot >= o->slots.size()) return ngzs::fail(o, NGZ_E_INVALID, "no such slot in the last encode");
    const SlotOut &so = o->slots[slot];
    if ((bytes && bytes_cap < so.n_bytes) || (offsets && offsets_cap < so.n_rows + 1))
        return ngzs::fail(o, NGZ_E_INVALID, "a buffer smaller than the slot");
    if (!so.n_rows) {
        if (offsets && offsets_cap) offsets[0] = 0;
        return NGZ_OK;
    }
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    if (bytes) {
        const uint64_t n = bytes_cap >= so.n_bytes + NGZ_OUTPUT_GUARD ? so.n_bytes + NGZ_OUTPUT_GUARD : so.n_bytes;
        if (n) NGZ_STAGE_HIP(o, hipMemcpy(bytes, so.bytes, n, hipMemcpyDeviceToHost));
    }
    if (offsets) NGZ_STAGE_HIP(o, hipMemcpy(offsets, so.offs, (so.n_rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return NGZ_OK;
}

int ngz_output_totals(ngz_output *o, ngz_output_stats *totals, int reset) {
    if (!o || !totals) return NGZ_E_INVALID;
    *totals = o->totals;
    if (reset) o->totals = ngz_output_stats{};
    return NGZ_OK;
}

int ngz_output_last_timing(ngz_output *o, float *size_ms, float *pack_ms) {
    if (!o || !size_ms || !pack_ms) return NGZ_E_INVALID;
    *size_ms = o->size_ms;
    *pack_ms = o->pack_ms;
    return NGZ_OK;
}

int ngz_output_last_launches(ngz_output *o) { return o ? o->launches : NGZ_E_INVALID; }

}  // extern "C"
