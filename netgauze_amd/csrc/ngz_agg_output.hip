// Avro datums of aggregated flow groups (include/ngz/flow_agg_output.h): get_avro_value_from_fields
// (crates/collector/src/flow/config.rs:105-145) over the one-record FlowInfo of each group
// (aggregation/aggregator.rs:203-277, aggregation/actor.rs:222-240), read from the rows ngz_agg_flush /
// ngz_agg_emit hand out.  The config and the schema are ngz_output_plan.cpp's; this unit lists, per
// encode and on the host, each ref's candidates in the group's field order, uploads rows, tails and
// plan, and runs
//   k_agg_output_size  a wave stages its tile of consecutive rows into LDS (coalesced 16-byte loads),
//                      each lane sizes its own row there; four lengths per 16-byte store,
//   a hipcub exclusive scan: the u64 offsets,
//   k_agg_output_pack  the same staging, then the wave encodes into an LDS image laid out like its
//                      output range and copies it out in 16-byte stores.
// The writers and encoders are ngz_output_enc.h's, shared with ngz_output.hip.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ngz/flow_agg_output.h"
#include "ngz_agg_rows.h"
#include "ngz_host.h"
#include "ngz_output_enc.h"
#include "ngz_output_plan.h"
#include "ngz_stage.h"

namespace {

using namespace ngzenc;
using namespace ngzrow;

constexpr uint32_t AO_THREADS = 128;
constexpr uint32_t AO_WAVES = AO_THREADS / 64;
// A tile is the rows a wave stages at once (ngz_agg_rows.h: a row takes row_bytes + AO_PAD there): 64
// of 128-byte rows in AO_STAGE_SMALL, 64 of 256-byte rows in AO_STAGE_LARGE, fewer (a multiple of
// four) of longer rows.
constexpr uint32_t AO_STAGE_SMALL = 64 * (128 + AO_PAD), AO_STAGE_LARGE = 64 * (256 + AO_PAD);
constexpr uint32_t AO_IMG = 8176;  // a wave's image, and 16 of slack for the output's misalignment
constexpr uint32_t AO_DEFAULT_POOL = 1024;
constexpr uint32_t AO_MAX_REFS = NGZ_OUTPUT_MAX_FIELDS * NGZ_OUTPUT_MAX_REFS;
constexpr uint32_t ERR_PEER = 1, ERR_TAIL = 2;

enum : uint8_t { A_KEY, A_VAL, A_ALWAYS, A_PEER4, A_PEER6, A_PORTS, A_DOMAINS, A_TEMPLATES };  // where a candidate lives
enum : uint8_t { LD_INT, LD_PTR, LD_STRZ, LD_BVAL, LD_WEND };  // how its value is read
enum : uint8_t { TS_NONE, TS_SECS, TS_MS, TS_FRAC_KEY, TS_FRAC_VAL };  // ENC_TS_SECS: the dateTime storage
enum : uint8_t { F_NULLABLE = 1, F_L2 = 2, F_ARRAY = 4, F_MASK40 = 8 };

struct ASource {  // one candidate of a ref
    uint8_t kind;
    uint8_t bit;    // A_KEY / A_VAL: its presence bit
    uint8_t load;
    uint8_t enc;    // ngzout::Enc
    uint16_t off;   // row offset
    uint16_t width;
    uint8_t aux;    // ENC_MPLS_ITEM: n
    uint8_t ts;
    uint8_t reserved[2];
};
struct ARef {
    uint16_t first, n;  // its candidates, in the order of the group's field list
    uint16_t index;     // FieldRef index: the occurrence wanted among the present ones
    uint16_t reserved;
};
struct AField {
    uint16_t ref0;
    uint8_t n_refs;
    uint8_t flags;
    uint16_t def_off;
    uint8_t def_len;
    uint8_t l2_encap;
};
using ASetEntry = ngzrow::SetEntry;
// One encode's plan, in device memory (uploaded with the rows): every lane reads it uniformly
struct APlan {
    ASource src[NGZ_AGG_OUTPUT_MAX_SOURCES];
    ARef refs[AO_MAX_REFS];
    AField f[NGZ_OUTPUT_MAX_FIELDS];
    uint8_t defaults[AO_DEFAULT_POOL];
    ASetEntry ports[NGZ_AGG_SET_BITS], templates[NGZ_AGG_SET_BITS], domains[2 * NGZ_AGG_SET_BITS];  // ascending by value
    uint32_t n_ports, n_templates, n_domains;
    uint32_t n_fields;
    unsigned long long window_ms;
};
struct AArgs {  // passed by value
    const APlan *plan;
    const uint8_t *rows;   // n_rows x row_bytes, 16-byte aligned
    const uint8_t *arena;  // the byte values longer than a row holds, whole, at 8-byte offsets
    unsigned long long arena_size;
    const ngz_peer *peers;
    uint32_t n_peers, n_rows, row_bytes, tile;
    uint32_t *lens;
    const unsigned long long *offs;
    uint8_t *out;
    unsigned long long total;
    unsigned int *err;
};

// The value of candidate S (member m of a set) of row R into c; S.enc / S.width as the encoders want them
__device__ __forceinline__ void load_value(const APlan &P, const AArgs &A, const uint8_t *R, ASource &S, uint32_t member, Cell &c, uint32_t *err) {
    c = Cell{0, R, 0};
    const uint8_t *p = R + S.off;
    if (S.kind == A_PORTS || S.kind == A_DOMAINS || S.kind == A_TEMPLATES) {
        c.v = member;
    } else if (S.kind == A_PEER4 || S.kind == A_PEER6) {
        const uint8_t *a = A.peers[ld_le(R + R_PEER, 2)].addr;  // the index was checked by peer_family
        c.p = a;
        c.n = 16;
        c.v = ((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3];
    } else if (S.load == LD_INT) {
        c.v = ld_le(p, S.width);
    } else if (S.load == LD_WEND) {  // windowEnd = windowStart + window duration (actor.rs:222-240), milliseconds
        c.v = ld_le(R + R_WINDOW, 4) * 1000ull + P.window_ms;
    } else if (S.load == LD_PTR) {
        c.p = p;
        c.n = S.width;
    } else if (S.load == LD_STRZ) {
        uint32_t n = 0;
        while (n < S.width && p[n]) ++n;
        c.p = p;
        c.n = n;
    } else {  // LD_BVAL: {u32 length, u32 offset / 8 into the arena, the first 32 bytes}
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
    }
    if (S.ts != TS_NONE) {  // ts.timestamp().to_string() (config.rs:934-940): the whole seconds, floored
        int64_t secs;
        if (S.ts == TS_MS) secs = floor_div((int64_t)c.v, 1000);
        else if (S.ts == TS_FRAC_VAL) secs = (int64_t)(c.v >> 32);
        else secs = (int64_t)(uint32_t)c.v;  // TS_SECS, TS_FRAC_KEY {u32 secs, u32 nanos}
        c.v = (uint64_t)secs;
        S.width = 8;  // S.enc is ENC_DEC_S already; its width was the storage's
    }
}

// The peer's address family, 0 for an index outside the peers (sets ERR_PEER)
__device__ __forceinline__ uint32_t peer_family(const AArgs &A, const uint8_t *R, uint32_t *err) {
    const uint32_t pi = (uint32_t)ld_le(R + R_PEER, 2);
    if (pi >= A.n_peers) {
        *err |= ERR_PEER;
        return 0;
    }
    return A.peers[pi].family;
}

// FieldRef lookup in the row's own list (config.rs:194-213): the ref's index-th present candidate
__device__ __forceinline__ bool resolve(const APlan &P, const AArgs &A, const uint8_t *R, const ARef &ref, ASource &S, Cell &c, bool load,
                                        uint32_t *err) {
    uint32_t rem = ref.index;
    for (uint32_t s = ref.first; s < (uint32_t)ref.first + ref.n; ++s) {
        S = P.src[s];
        uint32_t member = 0;
        bool hit = false;
        if (S.kind == A_PORTS || S.kind == A_DOMAINS || S.kind == A_TEMPLATES) {
            const ASetEntry *e = S.kind == A_PORTS ? P.ports : S.kind == A_DOMAINS ? P.domains : P.templates;
            const uint32_t n = S.kind == A_PORTS ? P.n_ports : S.kind == A_DOMAINS ? P.n_domains : P.n_templates;
            const uint8_t *bits = R + (S.kind == A_PORTS ? R_PORTS : S.kind == A_DOMAINS ? R_DOMAINS : R_TEMPLATES);
            for (uint32_t j = 0; j < n && !hit; ++j) {
                const uint32_t b = e[j].bit;
                if (!((*(const uint32_t *)(bits + 4u * (b >> 5)) >> (b & 31u)) & 1u)) continue;
                if (rem == 0) {
                    hit = true;
                    member = e[j].value;
                } else {
                    --rem;
                }
            }
        } else {
            bool present = true;
            if (S.kind == A_KEY) present = (ld_le(R + R_KEYP, 4) >> S.bit) & 1u;
            else if (S.kind == A_VAL) present = (ld_le(R + R_VALP, 4) >> S.bit) & 1u;
            else if (S.kind == A_PEER4) present = peer_family(A, R, err) == 4;
            else if (S.kind == A_PEER6) present = peer_family(A, R, err) == 6;
            if (present) {
                if (rem == 0) hit = true;
                else --rem;
            }
        }
        if (hit) {
            if (load) load_value(P, A, R, S, member, c, err);
            return true;
        }
    }
    return false;
}

// One group's datum: per field select, transform, default as FieldConfig::avro_value (config.rs:532-543),
// then the union branch of a nullable field
template <class W>
__device__ __forceinline__ void encode_row(const APlan &P, const AArgs &A, const uint8_t *R, W &w, uint32_t *err) {
    for (uint32_t fi = 0; fi < P.n_fields; ++fi) {
        const AField F = P.f[fi];
        ASource S;
        Cell c;
        uint32_t n_some = 0;
        if (F.flags & F_ARRAY) {  // Multi under MplsIndex: the present ones in select order (:964-996)
            for (uint32_t r = 0; r < F.n_refs; ++r) n_some += resolve(P, A, R, P.refs[F.ref0 + r], S, c, false, err) ? 1u : 0u;
        } else {  // Single, Coalesce: the first one present; Layer2SegmentIdFieldSelect::apply (:746-762)
            for (uint32_t r = 0; r < F.n_refs && !n_some; ++r) n_some = resolve(P, A, R, P.refs[F.ref0 + r], S, c, true, err) ? 1u : 0u;
            if ((F.flags & F_L2) && n_some) {
                if ((uint8_t)(c.v >> 56) != F.l2_encap) n_some = 0;
                c.v &= (F.flags & F_MASK40) ? 0xFFFFFFFFFFull : 0xFFFFFFull;
            }
        }
        if (!n_some) {
            if (F.flags & F_NULLABLE) w.put(0);
            else w.bytes(P.defaults + F.def_off, F.def_len);
            continue;
        }
        if (F.flags & F_NULLABLE) w.put(2);  // branch 1
        if (!(F.flags & F_ARRAY)) {
            encode_value(w, S, c);
            continue;
        }
        put_varint(w, (uint64_t)n_some << 1);
        for (uint32_t r = 0; r < F.n_refs; ++r)
            if (resolve(P, A, R, P.refs[F.ref0 + r], S, c, true, err)) encode_value(w, S, c);
        w.put(0);
    }
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
template <uint32_t STAGE>
__global__ __launch_bounds__(AO_THREADS) void k_agg_output_size(const AArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t stages[AO_WAVES][STAGE];
    const uint32_t lane = threadIdx.x & 63u, T = A.tile;
    uint8_t *const stage = stages[threadIdx.x >> 6];
    const uint32_t tiles = (A.n_rows + T - 1) / T;
    const APlan &P = *A.plan;
    uint32_t err = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.lens[(A.n_rows + 3u) & ~3u] = 0;  // the scan's last item
    for (uint32_t tile = blockIdx.x * AO_WAVES + (threadIdx.x >> 6); tile < tiles; tile += gridDim.x * AO_WAVES) {
        const uint32_t row0 = tile * T, nt = min(T, A.n_rows - row0);
        stage_rows(A.rows, A.row_bytes, row0, nt, stage, lane);
        CountW w;
        if (lane < nt) encode_row(P, A, stage + lane * (A.row_bytes + AO_PAD), w, &err);
        // four lengths per 16-byte store: T and row0 are multiples of four, rows past n_rows count 0
        const uint32_t n1 = __shfl_down(w.n, 1, 64), n2 = __shfl_down(w.n, 2, 64), n3 = __shfl_down(w.n, 3, 64);
        if (!(lane & 3u) && lane < nt) *(uint4 *)(A.lens + row0 + lane) = make_uint4(w.n, n1, n2, n3);
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();  // the stage is rewritten by the next tile
    }
    if (err) atomicOr(A.err, err);
}

template <uint32_t STAGE>
__global__ __launch_bounds__(AO_THREADS) void k_agg_output_pack(const AArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t stages[AO_WAVES][STAGE];
    __shared__ __attribute__((aligned(16))) uint8_t images[AO_WAVES][AO_IMG + 16];  // pack_tile's, one per wave
    const uint32_t lane = threadIdx.x & 63u, T = A.tile;
    uint8_t *const stage = stages[threadIdx.x >> 6];
    uint8_t *const img = images[threadIdx.x >> 6];
    const uint32_t tiles = (A.n_rows + T - 1) / T;
    const APlan &P = *A.plan;
    uint32_t err = 0;
    for (uint32_t tile = blockIdx.x * AO_WAVES + (threadIdx.x >> 6); tile < tiles; tile += gridDim.x * AO_WAVES) {
        const uint32_t row0 = tile * T, nt = min(T, A.n_rows - row0);
        stage_rows(A.rows, A.row_bytes, row0, nt, stage, lane);
        const uint8_t *const R = stage + lane * (A.row_bytes + AO_PAD);
        const unsigned long long a = A.offs[lane < nt ? row0 + lane : A.n_rows], b = lane < nt ? A.offs[row0 + lane + 1] : a;
        const unsigned long long base = __shfl(a, 0, 64);
        const uint32_t rel0 = (uint32_t)(a - base), rel1 = (uint32_t)(b - base);
        pack_tile<AO_IMG>(lane, nt, base, rel0, rel1, A.out, A.total, img, [&](PutW &w) { encode_row(P, A, R, w, &err); });
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();  // the stage is rewritten by the next tile
    }
    if (err) atomicOr(A.err, err);
}

struct ToU64 {
    __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t v) const { return v; }
};
using LenIter = hipcub::TransformInputIterator<unsigned long long, ToU64, const uint32_t *>;

}  // namespace

struct ngz_agg_output : ngzs::Stage {
    ngz_agg_output() : Stage(4) {}
    ngzout::Config cfg;
    std::string schema;
    float upload_ms = 0, size_ms = 0, pack_ms = 0;
    int launches = 0;
    uint64_t n_rows = 0, n_bytes = 0;  // the last encode
    bool have = false;
    ngzh::DevBuf<uint8_t> d_in, d_bytes, d_scan_tmp;  // d_in: plan, rows, arena, peers
    ngzh::DevBuf<uint32_t> d_lens, d_err;
    ngzh::DevBuf<unsigned long long> d_offs;
    ngzs::PinnedBuf<uint8_t> h_in;
    ngzs::PinnedBuf<unsigned long long> h_back;  // error bits, the total
};

namespace {

struct Item {  // one entry of the group's field list (aggregator.rs:219-242)
    uint32_t pen;
    uint16_t ie;
    uint8_t kind;
    uint32_t index;  // A_KEY / A_VAL: which
    uint16_t off, width;
    uint8_t load, ts;
};

// How a candidate of encoding `enc` is read from key k's storage; false: a storage the encoders cannot read
bool key_rule(const ngz_agg_key_desc &d, uint8_t enc, ASource *s) {
    using namespace ngzout;
    if (d.kkind == 3) {
        s->load = LD_BVAL;
        return enc == ENC_STR || enc == ENC_BYTES;
    }
    const bool int_w = d.width == 1 || d.width == 2 || d.width == 4 || d.width == 8;
    s->load = LD_INT;
    s->width = d.width;
    switch (enc) {
    case ENC_INT_U: case ENC_DEC_U: return d.kind == NGZ_K_UINT && int_w;
    case ENC_INT_S: case ENC_DEC_S: return d.kind == NGZ_K_SINT && int_w;
    case ENC_RAW: return d.kind == NGZ_K_UINT && (d.width == 4 || d.width == 8);
    case ENC_BOOL: case ENC_BOOLSTR: return d.kind == NGZ_K_BOOL && d.width == 1;
    case ENC_IP4: return d.kind == NGZ_K_UINT && d.width == 4;
    case ENC_TS_SECS:
        s->ts = d.kind == NGZ_K_DTMS ? TS_MS : d.kind == NGZ_K_DTFRAC ? TS_FRAC_KEY : TS_SECS;
        return (d.kind == NGZ_K_UINT && d.width == 4) || ((d.kind == NGZ_K_DTMS || d.kind == NGZ_K_DTFRAC) && d.width == 8);
    }
    s->load = LD_PTR;
    switch (enc) {
    case ENC_MAC: return d.kind == NGZ_K_BYTES && d.width == 6;
    case ENC_IP6: return d.kind == NGZ_K_BYTES && d.width == 16;
    case ENC_MPLS_ITEM: return d.kind == NGZ_K_BYTES && d.width == 3;
    case ENC_BYTES: return d.kind == NGZ_K_BYTES || (d.kind == NGZ_K_U256 && d.width == 32);
    case ENC_STR:
        s->load = LD_STRZ;
        return d.kind == NGZ_K_STR;
    }
    return false;
}

// The same for aggregated field v: integers are 8 bytes, extended from the IE's Rust width
bool value_rule(const ngz_agg_value_desc &d, uint16_t bytes_width, uint8_t enc, ASource *s) {
    using namespace ngzout;
    s->load = LD_INT;
    s->width = 8;
    switch (d.vclass) {
    case 0:
        if (enc == ENC_TS_SECS) {
            s->ts = d.kind == NGZ_K_DTMS ? TS_MS : TS_SECS;
            return d.kind == NGZ_K_DTMS || d.kind == NGZ_K_UINT;
        }
        return enc == ENC_INT_U || enc == ENC_DEC_U || enc == ENC_IP4 || enc == ENC_BOOL || enc == ENC_BOOLSTR;
    case 1:
        if (enc == ENC_TS_SECS) {
            s->ts = TS_MS;
            return d.kind == NGZ_K_DTMS;
        }
        return enc == ENC_INT_S || enc == ENC_DEC_S;
    case 2:
        s->ts = TS_FRAC_VAL;
        return enc == ENC_TS_SECS;
    case 5: s->width = 4; return enc == ENC_RAW;
    case 6: return enc == ENC_RAW;
    case 3:
        s->load = LD_PTR;
        s->width = bytes_width;
        return (enc == ENC_MAC && bytes_width == 6) || (enc == ENC_IP6 && bytes_width == 16) || (enc == ENC_MPLS_ITEM && bytes_width == 3) ||
               enc == ENC_BYTES;
    case 7:
        s->load = LD_PTR;
        s->width = 16;
        return enc == ENC_IP6;
    case 8: case 9:
        s->load = LD_BVAL;
        return enc == ENC_STR || enc == ENC_BYTES;
    }
    return false;  // vclass 4: reachable through no accepted transform
}

// The extra fields of the group's record: always present, the peer's family or set members aside
bool extra_rule(const Item &it, uint8_t enc, ASource *s) {
    using namespace ngzout;
    s->load = it.load;
    s->width = it.width;
    s->ts = it.ts;
    switch (it.kind) {
    case A_PEER4: return enc == ENC_IP4;
    case A_PEER6: return enc == ENC_IP6;
    case A_ALWAYS: return it.ts != TS_NONE ? enc == ENC_TS_SECS : enc == ENC_INT_U || enc == ENC_DEC_U;
    }
    s->ts = TS_NONE;
    return enc == ENC_INT_U || enc == ENC_DEC_U;  // the sets: u16 ports and template ids, u32 domains
}

}  // namespace

extern "C" {

int ngz_agg_output_abi_version(void) { return NGZ_AGG_OUTPUT_ABI_VERSION; }

int ngz_agg_output_create(int device, const ngz_output_field *fields, uint32_t n, ngz_agg_output **out, char *err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0) return NGZ_E_INVALID;
    ngz_agg_output *o = new ngz_agg_output;
    o->device = device;
    std::string why;
    int rc = ngzout::build_config(fields, n, &o->cfg, &why, true);
    size_t pool = 0;
    for (const ngzout::CfgField &f : o->cfg.fields) pool += f.def.size();
    if (!rc && pool > AO_DEFAULT_POOL) {
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

void ngz_agg_output_destroy(ngz_agg_output *o) {
    if (!o) return;
    if (o->device_ready) {
        hipSetDevice(o->device);
        o->d_in.release();
        o->d_bytes.release();
        o->d_scan_tmp.release();
        o->d_lens.release();
        o->d_err.release();
        o->d_offs.release();
    }
    delete o;
}

const char *ngz_agg_output_last_error(ngz_agg_output *o) { return o ? o->last_error.c_str() : "null aggregated output stage"; }

int64_t ngz_agg_output_schema(ngz_agg_output *o, char *buf, size_t cap) {
    if (!o) return NGZ_E_INVALID;
    if (buf && cap) snprintf(buf, cap, "%s", o->schema.c_str());
    return (int64_t)o->schema.size();
}

int ngz_agg_output_encode(ngz_agg_output *o, ngz_agg *agg, const void *rows, uint64_t n_rows, ngz_agg_output_stats *stats, void *hip_stream) {
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

    // the group's field list (aggregator.rs:219-242, actor.rs:222-240)
    std::vector<Item> list;
    for (uint32_t k = 0; k < nk; ++k) list.push_back(Item{keys[k].pen, keys[k].ie_id, A_KEY, k, (uint16_t)ko[k], 0, 0, 0});
    for (uint32_t v = 0; v < nv; ++v) list.push_back(Item{vals[v].pen, vals[v].ie_id, A_VAL, v, (uint16_t)vo[v], 0, 0, 0});
    list.push_back(Item{0, 375, A_ALWAYS, 0, (uint16_t)R_COUNT, 8, LD_INT, TS_NONE});       // originalFlowsPresent
    list.push_back(Item{0, 264, A_ALWAYS, 0, (uint16_t)R_MIN_EXPORT, 4, LD_INT, TS_SECS});  // minExportSeconds
    list.push_back(Item{0, 260, A_ALWAYS, 0, (uint16_t)R_MAX_EXPORT, 4, LD_INT, TS_SECS});  // maxExportSeconds
    list.push_back(Item{0, 258, A_ALWAYS, 0, (uint16_t)R_MAX_COLL, 8, LD_INT, TS_MS});      // collectionTimeMilliseconds
    list.push_back(Item{3746, 1, A_ALWAYS, 0, (uint16_t)R_WINDOW, 4, LD_INT, TS_SECS});     // NetGauze windowStart
    list.push_back(Item{3746, 2, A_ALWAYS, 0, (uint16_t)R_WINDOW, 8, LD_WEND, TS_MS});      // NetGauze windowEnd
    list.push_back(Item{0, 403, A_PEER4, 0, 0, 4, LD_INT, TS_NONE});                        // originalExporterIPv4Address
    list.push_back(Item{0, 404, A_PEER6, 0, 0, 16, LD_PTR, TS_NONE});                       // originalExporterIPv6Address
    list.push_back(Item{3746, 4, A_PORTS, 0, 0, 2, LD_INT, TS_NONE});                       // NetGauze originalExporterTransportPort
    list.push_back(Item{0, 405, A_DOMAINS, 0, 0, 4, LD_INT, TS_NONE});                      // originalObservationDomainId
    list.push_back(Item{3746, 3, A_TEMPLATES, 0, 0, 2, LD_INT, TS_NONE});                   // NetGauze originalTemplateId

    // the plan: each ref's candidates in list order, each with its presence test and its reader
    const uint64_t plan_bytes = align256(sizeof(APlan));
    std::vector<uint8_t> plan_mem(sizeof(APlan), 0);
    APlan &P = *(APlan *)plan_mem.data();
    uint32_t n_src = 0, n_refs = 0, def_off = 0;
    for (size_t f = 0; f < o->cfg.fields.size(); ++f) {
        const ngzout::CfgField &cf = o->cfg.fields[f];
        AField &df = P.f[f];
        df.ref0 = (uint16_t)n_refs;
        df.n_refs = (uint8_t)cf.refs.size();
        df.flags = (cf.nullable ? F_NULLABLE : 0) | (cf.select == NGZ_OUT_SEL_L2SEGMENT ? F_L2 : 0) | (cf.avro == NGZ_OUT_T_ARRAY ? F_ARRAY : 0) |
                   (cf.l2_mask > 0xFFFFFFull ? F_MASK40 : 0);
        df.l2_encap = cf.l2_encap;
        df.def_off = (uint16_t)def_off;
        df.def_len = (uint8_t)cf.def.size();
        memcpy(P.defaults + def_off, cf.def.data(), cf.def.size());
        def_off += (uint32_t)cf.def.size();
        for (const ngzout::CfgRef &ref : cf.refs) {
            ARef &dr = P.refs[n_refs++];
            dr.first = (uint16_t)n_src;
            dr.index = ref.index;
            for (const Item &it : list) {
                if (it.pen != ref.pen || it.ie != ref.ie) continue;
                // a key or value no record has carried yet has no kind: its presence bit is set in no row
                if (it.kind == A_KEY && kd[it.index].kkind != 3 && !kd[it.index].kind) continue;
                if (it.kind == A_VAL && !vd[it.index].kind) continue;
                if (n_src == NGZ_AGG_OUTPUT_MAX_SOURCES) return ngzs::fail(o, NGZ_E_LIMIT, "more than 256 candidates over all refs");
                ASource s{};
                s.kind = it.kind;
                s.bit = (uint8_t)it.index;
                s.off = it.off;
                s.enc = ref.enc;
                s.aux = ref.mpls_n;
                const bool ok = it.kind == A_KEY ? key_rule(kd[it.index], ref.enc, &s)
                              : it.kind == A_VAL ? value_rule(vd[it.index], vw[it.index], ref.enc, &s) : extra_rule(it, ref.enc, &s);
                if (!ok) return ngzs::fail(o, NGZ_E_LIMIT, "field " + cf.name + ": a row storage the output cannot read in this encoding");
                if (s.enc == ngzout::ENC_TS_SECS) s.enc = ngzout::ENC_DEC_S;  // load_value hands the seconds on
                P.src[n_src++] = s;
            }
            dr.n = (uint16_t)(n_src - dr.first);
        }
    }
    P.n_fields = (uint32_t)o->cfg.fields.size();
    P.window_ms = ngzh::agg_window_ms(agg);
    {  // the dictionaries of the last flush / emit (entry i <-> bit i, -1 free), each sorted once: bit
       // order is not value order
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
    const uint64_t rows_at = plan_bytes, arena_at = rows_at + align256(rows_bytes), peers_at = arena_at + align256(arena_bytes);
    const uint64_t in_bytes = peers_at + align256(peers.size() * sizeof(ngz_peer));
    if (int rc = ngzs::device_init(o)) return rc;
    NGZ_STAGE_HIP(o, hipSetDevice(o->device));
    if (o->h_in.reserve(in_bytes)) return ngzs::fail(o, NGZ_E_NOMEM, "aggregated output staging");
    uint8_t *h = o->h_in.p;
    memcpy(h, plan_mem.data(), sizeof(APlan));
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
    const uint32_t tile = rb <= 256 ? 64u : (AO_STAGE_LARGE / (rb + AO_PAD)) & ~3u;
    if (!tile) return ngzs::fail(o, NGZ_E_LIMIT, "rows too long to stage");
    const uint64_t n_lens = ((n_rows + 3) & ~3ull) + 4;
    size_t scan_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, LenIter((const uint32_t *)nullptr, ToU64()), (unsigned long long *)nullptr,
                                         (int)(n_rows + 1), st) != hipSuccess)
        return ngzs::fail(o, NGZ_E_DEVICE, "scan temp size");
    if (o->d_in.ensure(in_bytes) || o->d_lens.ensure(n_lens) || o->d_offs.ensure(n_rows + 2) || o->d_err.ensure(4) ||
        o->d_scan_tmp.ensure(scan_bytes + 1) || o->h_back.reserve(2))
        return ngzs::fail(o, NGZ_E_NOMEM, "aggregated output buffers");
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
    NGZ_STAGE_HIP(o, hipMemcpyAsync(o->d_in.p, h, in_bytes, hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(o, hipMemsetAsync(o->d_err.p, 0, sizeof(uint32_t), st));
    NGZ_STAGE_HIP(o, hipEventRecord(o->ev[1], st));
    AArgs A{};
    A.plan = (const APlan *)o->d_in.p;
    A.rows = o->d_in.p + rows_at;
    A.arena = o->d_in.p + arena_at;
    A.arena_size = arena_bytes;
    A.peers = (const ngz_peer *)(o->d_in.p + peers_at);
    A.n_peers = (uint32_t)peers.size();
    A.n_rows = (uint32_t)n_rows;
    A.row_bytes = rb;
    A.tile = tile;
    A.lens = o->d_lens.p;
    A.offs = o->d_offs.p;
    A.err = o->d_err.p;
    const uint64_t tiles = (n_rows + tile - 1) / tile;
    const uint32_t nb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((tiles + AO_WAVES - 1) / AO_WAVES, (uint64_t)o->n_cus * 16));
    const bool small = rb == 128;
    hipLaunchKernelGGL(small ? k_agg_output_size<AO_STAGE_SMALL> : k_agg_output_size<AO_STAGE_LARGE>, dim3(nb), dim3(AO_THREADS), 0, st, A);
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
    if (o->d_bytes.ensure(total + NGZ_OUTPUT_GUARD + 16)) return ngzs::fail(o, NGZ_E_NOMEM, "aggregated output bytes");
    A.out = o->d_bytes.p;
    A.total = total;
    NGZ_STAGE_HIP(o, hipMemsetAsync(A.out + total, 0xA5, NGZ_OUTPUT_GUARD, st));
    if (total) {
        NGZ_STAGE_HIP(o, hipEventRecord(o->ev[0], st));
        hipLaunchKernelGGL(small ? k_agg_output_pack<AO_STAGE_SMALL> : k_agg_output_pack<AO_STAGE_LARGE>, dim3(nb), dim3(AO_THREADS), 0, st, A);
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
    if (stats) *stats = ngz_agg_output_stats{n_rows, total, arena_bytes};
    return NGZ_OK;
}

int ngz_agg_output_result(ngz_agg_output *o, const uint8_t **bytes, const uint64_t **offsets, uint64_t *n_rows, uint64_t *n_bytes) {
    if (!o) return NGZ_E_INVALID;
    if (!o->have) return ngzs::fail(o, NGZ_E_INVALID, "no encode to read");
    if (bytes) *bytes = o->n_rows ? o->d_bytes.p : nullptr;
    if (offsets) *offsets = o->n_rows ? (const uint64_t *)o->d_offs.p : nullptr;
    if (n_rows) *n_rows = o->n_rows;
    if (n_bytes) *n_bytes = o->n_bytes;
    return NGZ_OK;
}

int ngz_agg_output_to_host(ngz_agg_output *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap) {
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

int ngz_agg_output_last_timing(ngz_agg_output *o, float *upload_ms, float *size_ms, float *pack_ms) {
    if (!o || !upload_ms || !size_ms || !pack_ms) return NGZ_E_INVALID;
    *upload_ms = o->upload_ms;
    *size_ms = o->size_ms;
    *pack_ms = o->pack_ms;
    return NGZ_OK;
}

int ngz_agg_output_last_launches(ngz_agg_output *o) { return o ? o->launches : NGZ_E_INVALID; }

}  // extern "C"
