// Flow enrichment (include/ngz/flow_enrich.h): the reference's EnrichmentActor::enrich
// (crates/collector/src/flow/enrichment/actor.rs:122-271) over the decoded columns of a batch.
// The cache lives on the host (ngz_enrich_cache.cpp); a peer's scopes are uploaded as read-only
// open-addressing tables, one per scope shape, and one plan-driven row kernel per template slot
// resolves every record against them: lanes map to consecutive rows (four per lane), key columns
// load and added columns store as coalesced vectors.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "ngz/flow_enrich.h"
#include "ngz_enrich_cache.h"
#include "ngz_enrich_internal.h"
#include "ngz_host.h"
#include "ngz_renorm_internal.h"
#include "ngz_stage.h"
#include "ngz_template_record.h"

namespace {

constexpr uint32_t EN_THREADS = 256;
constexpr uint32_t EN_ROWS_PER_LANE = 4;
constexpr uint32_t EN_STATS = 2;  // device counters: records matched, fields added
constexpr uint32_t EN_NONE = 0xFFFFFFFFu;
constexpr uint32_t EN_MAX_RANK = (1u << 23) - 2;  // scopes of one map (the priority word below)

// One scope of the peer: its key (scope values, each zero-padded to 16 bytes), the map it is in
// (0 global, 1 + i the peer's i-th domain) and its fields
struct EnEntry {
    uint4 key[NGZ_ENRICH_MAX_SCOPE_FIELDS];
    uint32_t map;
    uint32_t field0, n_fields;
    uint32_t reserved;
};
// One field of a scope: the peer column it adds, its priority ((weight << 24 | domain << 23 | order
// rank in the map) + 1: the maximum over the matched scopes is the reference's visiting-order
// winner, cache.rs:500-528) and the cell (the value, or the value arena descriptor)
struct EnField {
    uint32_t pcol;
    uint32_t prio;
    uint32_t reserved[2];
    uint4 cell;
};
static_assert(sizeof(EnEntry) == 80 && sizeof(EnField) == 32, "device table layout");

struct EnShape {
    const uint32_t *slots;  // 1 << bits words: entry index + 1, 0 = empty
    uint32_t bits;
    uint32_t n;             // scope fields
    const uint8_t *col[NGZ_ENRICH_MAX_SCOPE_FIELDS];
    uint32_t w[NGZ_ENRICH_MAX_SCOPE_FIELDS];
};

// What the row kernel needs of one slot, passed by value
struct EnPlan {
    EnShape shape[NGZ_ENRICH_MAX_SHAPES];
    uint32_t n_shapes;
    uint32_t n_cols;
    uint8_t *out[NGZ_ENRICH_MAX_COLUMNS];
    uint16_t pcol[NGZ_ENRICH_MAX_COLUMNS];  // the peer column of each added column
    uint8_t w[NGZ_ENRICH_MAX_COLUMNS];
    uint32_t *mask;
    const uint8_t *rowdom;  // per row: 0 a failed message's row, 1 no domain map, 2 + i the i-th domain
    const EnEntry *entries;
    const EnField *fields;
    uint32_t n_rows;
    uint32_t reserved;
    unsigned long long *stats;  // [EN_STATS]
};

__host__ __device__ inline uint32_t en_hash(uint32_t map, const uint4 *key, uint32_t n) {
    uint32_t h = map * 0x9E3779B1u + 0x85EBCA6Bu;
#pragma unroll
    for (uint32_t i = 0; i < NGZ_ENRICH_MAX_SCOPE_FIELDS; ++i) {
        if (i >= n) break;
        const uint32_t w[4] = {key[i].x, key[i].y, key[i].z, key[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h ^= w[j];
            h *= 0x01000193u;
            h ^= h >> 15;
        }
    }
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    return h;
}

__device__ __forceinline__ uint32_t en_word(const uint4 &v, uint32_t i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
__device__ __forceinline__ uint32_t en_byte(const uint4 &v, uint32_t b) { return (en_word(v, b >> 2) >> ((b & 3u) * 8u)) & 0xFFu; }

// The cells of four consecutive rows of a w-byte column (r0 a multiple of 4), each zero-extended to
// 16 bytes.  Whole-quad vector loads stay inside the column: its capacity is a multiple of 4 rows.
__device__ __forceinline__ void en_load4(const uint8_t *col, uint32_t w, uint32_t r0, uint4 v[4]) {
    const uint8_t *p = col + (uint64_t)w * r0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = make_uint4(0, 0, 0, 0);
    if (w == 4 || w == 2 || w == 1) {
        uint32_t x[4];
        ngzs::load4(col, w, r0, x);
        v[0].x = x[0]; v[1].x = x[1]; v[2].x = x[2]; v[3].x = x[3];
    } else if (w == 8) {
        const uint4 a = *(const uint4 *)p, b = *(const uint4 *)(p + 16);
        v[0].x = a.x; v[0].y = a.y; v[1].x = a.z; v[1].y = a.w;
        v[2].x = b.x; v[2].y = b.y; v[3].x = b.z; v[3].y = b.w;
    } else if (w == 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *(const uint4 *)(p + 16 * j);
    } else {  // 3, 5, 6, ... bytes (MAC, MPLS, short octets): w <= 16
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t x[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; b < w; ++b) x[b >> 2] |= (uint32_t)p[j * w + b] << ((b & 3u) * 8u);
            v[j] = make_uint4(x[0], x[1], x[2], x[3]);
        }
    }
}

// Four consecutive cells of a w-byte column; `live` rows (1..4) exist: nothing past them is written
__device__ __forceinline__ void en_store4(uint8_t *col, uint32_t w, uint32_t r0, const uint4 v[4], uint32_t live) {
    uint8_t *p = col + (uint64_t)w * r0;
    if (live == 4 && w == 4) {
        *(uint4 *)p = make_uint4(v[0].x, v[1].x, v[2].x, v[3].x);
    } else if (live == 4 && w == 2) {
        *(uint2 *)p = make_uint2((v[0].x & 0xFFFFu) | (v[1].x << 16), (v[2].x & 0xFFFFu) | (v[3].x << 16));
    } else if (live == 4 && w == 1) {
        *(uint32_t *)p = (v[0].x & 0xFFu) | ((v[1].x & 0xFFu) << 8) | ((v[2].x & 0xFFu) << 16) | (v[3].x << 24);
    } else if (live == 4 && w == 8) {
        *(uint4 *)p = make_uint4(v[0].x, v[0].y, v[1].x, v[1].y);
        *(uint4 *)(p + 16) = make_uint4(v[2].x, v[2].y, v[3].x, v[3].y);
    } else if (live == 4 && w == 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *(uint4 *)(p + 16 * j) = v[j];
    } else {  // other widths, and the slot's last rows
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((uint32_t)j >= live) break;
            for (uint32_t b = 0; b < w; ++b) p[j * w + b] = (uint8_t)en_byte(v[j], b);
        }
    }
}

// The entry of `map` whose key equals `key` in the shape's table, or EN_NONE.  The table has at
// least one empty slot, so the probe ends.
__device__ __forceinline__ uint32_t en_probe(const EnShape &S, const EnEntry *__restrict__ entries, uint32_t map,
                                             const uint4 key[NGZ_ENRICH_MAX_SCOPE_FIELDS]) {
    const uint32_t m = (1u << S.bits) - 1u;
    uint32_t i = en_hash(map, key, S.n) & m;
    for (uint32_t step = 0; step <= m; ++step, i = (i + 1u) & m) {
        const uint32_t s = S.slots[i];
        if (!s) return EN_NONE;
        const EnEntry &e = entries[s - 1u];
        bool eq = e.map == map;
#pragma unroll
        for (uint32_t f = 0; f < NGZ_ENRICH_MAX_SCOPE_FIELDS; ++f) {
            if (!eq || f >= S.n) break;
            const uint4 k = e.key[f];
            eq = k.x == key[f].x && k.y == key[f].y && k.z == key[f].z && k.w == key[f].w;
        }
        if (eq) return s - 1u;
    }
    return EN_NONE;
}

__global__ __launch_bounds__(EN_THREADS) void k_enrich(const EnPlan P) {
    __shared__ unsigned long long acc[EN_STATS];
    uint32_t n_matched = 0, n_added = 0;
    const uint32_t quads = (P.n_rows + EN_ROWS_PER_LANE - 1) / EN_ROWS_PER_LANE;
    for (uint32_t q = blockIdx.x * EN_THREADS + threadIdx.x; q < quads; q += gridDim.x * EN_THREADS) {
        const uint32_t r0 = q * EN_ROWS_PER_LANE;
        const uint32_t live = P.n_rows - r0 < EN_ROWS_PER_LANE ? P.n_rows - r0 : EN_ROWS_PER_LANE;
        const uint32_t rd = *(const uint32_t *)(P.rowdom + r0);  // four row bytes (the buffer is padded to a quad)
        uint32_t dom[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) dom[j] = (uint32_t)j < live ? (rd >> (8 * j)) & 0xFFu : 0u;
        // the matched scope of each (shape, global | domain), per row
        uint32_t hit[4][2 * NGZ_ENRICH_MAX_SHAPES];
#pragma unroll
        for (int s = 0; s < NGZ_ENRICH_MAX_SHAPES; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) hit[j][2 * s] = hit[j][2 * s + 1] = EN_NONE;
            if ((uint32_t)s >= P.n_shapes) continue;
            const EnShape &S = P.shape[s];
            uint4 key[4][NGZ_ENRICH_MAX_SCOPE_FIELDS];
#pragma unroll
            for (int f = 0; f < NGZ_ENRICH_MAX_SCOPE_FIELDS; ++f) {
                uint4 v[4];
                if ((uint32_t)f < S.n) en_load4(S.col[f], S.w[f], r0, v);
                else v[0] = v[1] = v[2] = v[3] = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) key[j][f] = v[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!dom[j]) continue;
                hit[j][2 * s] = en_probe(S, P.entries, 0u, key[j]);
                if (dom[j] >= 2u) hit[j][2 * s + 1] = en_probe(S, P.entries, dom[j] - 1u, key[j]);
            }
        }
        uint32_t mask[4] = {0, 0, 0, 0};
        for (uint32_t c = 0; c < P.n_cols; ++c) {
            const uint32_t pc = P.pcol[c];
            uint4 cell[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cell[j] = make_uint4(0, 0, 0, 0);
                uint32_t best = 0;
#pragma unroll
                for (int k = 0; k < 2 * NGZ_ENRICH_MAX_SHAPES; ++k) {
                    const uint32_t e = hit[j][k];
                    if (e == EN_NONE) continue;
                    const uint32_t f0 = P.entries[e].field0, nf = P.entries[e].n_fields;
                    for (uint32_t f = f0; f < f0 + nf; ++f) {
                        const EnField &fl = P.fields[f];
                        if (fl.pcol == pc && fl.prio > best) {  // priorities of one row's candidates are distinct
                            best = fl.prio;
                            cell[j] = fl.cell;
                        }
                    }
                }
                if (best) mask[j] |= 1u << c;
            }
            en_store4(P.out[c], P.w[c], r0, cell, live);
        }
        if (live == 4) {
            *(uint4 *)(P.mask + r0) = make_uint4(mask[0], mask[1], mask[2], mask[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if ((uint32_t)j < live) P.mask[r0 + j] = mask[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            n_matched += mask[j] ? 1u : 0u;
            n_added += __popc(mask[j]);
        }
    }
    const uint64_t cnt[EN_STATS] = {n_matched, n_added};
    unsigned long long *const dst[EN_STATS] = {&P.stats[0], &P.stats[1]};
    ngzs::block_add<EN_STATS>(acc, cnt, dst);
}

// One thread per data set (ngzs::for_each_set): the rows of a set whose message decoded get the byte
// 1 (the peer has no map for the message's observation domain) or 2 + i (its i-th domain, sorted);
// rows of failed messages keep the 0 the buffer was cleared to and are counted per slot.  err bit
// 0: a set outside the batch's tables.
__global__ void k_enrich_sets(const ngz_set_info *__restrict__ sets, uint32_t n_sets, const ngz_dgram_hdr *__restrict__ hdr,
                              uint32_t n_dgrams, uint32_t n_slots, const uint32_t *__restrict__ slot_rows,
                              const uint64_t *__restrict__ row_off, uint8_t *__restrict__ rowdom,
                              const uint32_t *__restrict__ domains, uint32_t n_domains,
                              unsigned long long *__restrict__ bad_rows, unsigned int *__restrict__ err) {
    ngzs::for_each_set(sets, n_sets, hdr, n_dgrams, n_slots, slot_rows, err, [&](uint32_t, const ngz_set_info &si, const ngz_dgram_hdr &dh) {
        const ngz_dgram_hdr h = dh;
        if (h.status != NGZ_DG_OK) {
            atomicAdd(&bad_rows[si.slot], (unsigned long long)si.n);
            return;
        }
        uint32_t v = 1;
        uint32_t lo = 0, hi = n_domains;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint32_t d = domains[mid];
            if (d == h.domain) { v = 2u + mid; break; }
            if (d < h.domain) lo = mid + 1; else hi = mid;
        }
        uint8_t *p = rowdom + row_off[si.slot] + si.rec0;
        uint8_t *const end = p + si.n;
        while (p < end && ((uintptr_t)p & 15)) *p++ = (uint8_t)v;
        const uint32_t v4 = v * 0x01010101u;
        for (; p + 16 <= end; p += 16) *(uint4 *)p = make_uint4(v4, v4, v4, v4);
        while (p < end) *p++ = (uint8_t)v;
    });
}

// ---------------------------------------------------------------------------------------------
// host: a peer's device tables
// ---------------------------------------------------------------------------------------------
struct ShapeKeyField {
    ngze::FieldRef ref;
    uint8_t kind;
    uint32_t len;
    bool operator<(const ShapeKeyField &o) const {
        if (!(ref == o.ref)) return ref < o.ref;
        return kind != o.kind ? kind < o.kind : len < o.len;
    }
};
using ShapeKey = std::vector<ShapeKeyField>;

struct PeerColumn {
    ngze::FieldRef ref;
    uint8_t kind = 0;     // NGZ_K_VLEN: descriptors into the value arena
    uint8_t is_string = 0;
    uint16_t width = 0;
    uint8_t value_kind = 0;  // the kind every value of the column has, 0 when they differ
};

struct PeerDev {
    uint64_t generation = ~0ull;  // the peer's cache generation the tables were built from
    int64_t table_bits = -1;
    std::vector<uint32_t> domains;  // sorted
    std::vector<ShapeKey> shapes;
    std::vector<std::set<uint32_t>> shape_cols;  // peer columns the scopes of a shape add
    std::vector<uint32_t> shape_bits;
    std::vector<uint64_t> shape_slot0;  // offset of the shape's table in d_slots
    std::vector<PeerColumn> cols;       // ascending FieldRef
    ngzh::DevBuf<EnEntry> d_entries;
    ngzh::DevBuf<EnField> d_fields;
    ngzh::DevBuf<uint32_t> d_slots;
    ngzh::DevBuf<uint32_t> d_domains;
    void release() {
        d_entries.release();
        d_fields.release();
        d_slots.release();
        d_domains.release();
    }
};

bool fixed_cell(uint8_t kind, size_t len) {
    switch (kind) {
    case NGZ_K_UINT: case NGZ_K_SINT: case NGZ_K_BOOL: case NGZ_K_TCPFLAGS: case NGZ_K_DTMS: case NGZ_K_DTFRAC:
    case NGZ_K_BYTES:
        return len >= 1 && len <= 16;
    }
    return false;
}

uint4 pad16(const std::string &b) {
    uint32_t w[4] = {0, 0, 0, 0};
    memcpy(w, b.data(), std::min<size_t>(b.size(), 16));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

struct ngz_enrich : ngzs::Stage {
    ngz_enrich() : Stage(2) {}
    std::string writer_id;
    ngze::Cache cache;
    ngz_enrich_stats totals{};
    int64_t table_bits = 0;  // NGZ_ENRICH_OPT_TABLE_BITS
    float apply_ms = 0;
    std::map<ngze::PeerIp, std::unique_ptr<PeerDev>> peers;
    // value arena: the bytes of variable-length values, interned (offsets stay valid as it grows)
    std::vector<uint8_t> h_arena;
    std::map<std::string, uint64_t> interned;
    ngzh::DevBuf<uint8_t> d_arena;
    uint64_t arena_uploaded = 0;
    // per context (by address, as a renormalizer remembers them): the batch last applied on it
    struct CtxResult {
        uint64_t serial = 0;
        bool valid = false;
        std::vector<ngze::SlotResult> results;
        std::vector<uint64_t> row_off;    // per slot: offset of its row bytes in d_rowdom
        ngzh::DevBuf<uint8_t> d_out;      // masks and added columns
        ngzh::DevBuf<uint8_t> d_rowdom;
        uint64_t out_bytes = 0, rowdom_bytes = 0;
        std::vector<uint8_t> h_out, h_rowdom;  // host copies for ngz_enrich_row_fields, made on first use
    };
    std::map<const ngz_ctx *, std::unique_ptr<CtxResult>> by_ctx;
    ngzh::DevBuf<uint64_t> d_meta;    // row_off[S], then slot_rows[S] as uint32_t
    ngzh::DevBuf<unsigned long long> d_counters;  // stats[EN_STATS], err, bad_rows[S]
    ngzs::PinnedBuf<uint64_t> h_meta;
    ngzs::PinnedBuf<unsigned long long> h_counters;
    std::vector<ngz_enrich_resolved> lookup_tmp;
};

namespace {

// Is the IE of a scope field one whose canonical encoding compares as the reference's Field does
bool scope_ie_ok(const ngz_enrich_field &f) {
    const ngzh::IeRow *row = ngzh::ie_find(f.pen, f.ie_id);
    if (!row) return false;
    switch (row->dtype) {
    case ngzh::DT_unsigned8: case ngzh::DT_unsigned16: case ngzh::DT_unsigned32: case ngzh::DT_unsigned64:
    case ngzh::DT_signed8: case ngzh::DT_signed16: case ngzh::DT_signed32: case ngzh::DT_signed64: case ngzh::DT_boolean:
    case ngzh::DT_macAddress: case ngzh::DT_dateTimeSeconds: case ngzh::DT_dateTimeMilliseconds:
    case ngzh::DT_ipv4Address: case ngzh::DT_ipv6Address:
        return true;
    }
    return false;
}

uint64_t intern(ngz_enrich *e, const std::string &bytes) {
    auto it = e->interned.find(bytes);
    if (it != e->interned.end()) return it->second;
    const uint64_t off = e->h_arena.size();
    e->h_arena.insert(e->h_arena.end(), bytes.begin(), bytes.end());
    e->interned.emplace(bytes, off);
    return off;
}

// Peer columns: every FieldRef a scope of the peer adds; fixed-width when all its values agree on
// one fixed kind and length, else descriptors into the value arena
void peer_columns(const ngze::PeerMetadata &pm, std::map<ngze::FieldRef, PeerColumn> &colmap) {
    auto scan_cols = [&](const ngze::ScopeMap &m) {
        for (const auto &sc : m)
            for (const auto &fw : sc.second) {
                const ngze::Value &v = fw.second.value;
                const bool fixed = fixed_cell(v.kind, v.bytes.size());
                auto it = colmap.find(fw.first);
                if (it == colmap.end()) {
                    PeerColumn pc;
                    pc.ref = fw.first;
                    pc.kind = fixed ? v.kind : (uint8_t)NGZ_K_VLEN;
                    pc.width = fixed ? (uint16_t)v.bytes.size() : 16;
                    pc.is_string = v.kind == NGZ_K_STR;
                    pc.value_kind = v.kind;
                    colmap.emplace(fw.first, pc);
                    continue;
                }
                PeerColumn &pc = it->second;
                if (pc.value_kind != v.kind) pc.value_kind = 0;
                if (pc.kind != NGZ_K_VLEN && (!fixed || pc.kind != v.kind || pc.width != v.bytes.size())) {
                    pc.kind = NGZ_K_VLEN;
                    pc.width = 16;
                }
                if (v.kind != NGZ_K_STR) pc.is_string = 0;
            }
    };
    scan_cols(pm.global);
    for (const auto &d : pm.domain_scoped) scan_cols(d.second);
}

// The shape of a scope: its ordered FieldRefs with the kind and length of each value
ShapeKey shape_of(const ngze::ScopeKey &sc) {
    ShapeKey sk;
    for (const ngze::ScopeField &f : sc) sk.push_back(ShapeKeyField{f.ref, f.value.kind, (uint32_t)f.value.bytes.size()});
    return sk;
}

// Build and upload the lookup tables of one peer (copies are synchronous: the host vectors are
// temporaries)
int upload_peer(ngz_enrich *e, const ngze::PeerMetadata &pm, PeerDev &pd) {
    pd.domains.clear();
    pd.shapes.clear();
    pd.shape_cols.clear();
    pd.cols.clear();
    if (pm.domain_scoped.size() > NGZ_ENRICH_MAX_DOMAINS)
        return ngzs::fail(e, NGZ_E_LIMIT, "a peer with more than 253 observation domains");
    for (const auto &d : pm.domain_scoped) pd.domains.push_back(d.first);
    std::map<ngze::FieldRef, PeerColumn> colmap;
    peer_columns(pm, colmap);
    std::map<ngze::FieldRef, uint32_t> col_index;
    for (const auto &c : colmap) {
        col_index[c.first] = (uint32_t)pd.cols.size();
        pd.cols.push_back(c.second);
    }
    if (pd.cols.size() > 0xFFFF) return ngzs::fail(e, NGZ_E_LIMIT, "a peer with more than 65535 distinct added fields");
    // entries in visiting order, by map
    std::vector<EnEntry> entries;
    std::vector<EnField> fields;
    std::vector<uint32_t> entry_shape;
    std::map<ShapeKey, uint32_t> shape_index;
    auto scan_map = [&](const ngze::ScopeMap &m, uint32_t map) -> int {
        if (m.size() > EN_MAX_RANK) return NGZ_E_LIMIT;
        uint32_t rank = 0;
        for (const auto &sc : m) {
            ShapeKey sk;
            EnEntry en{};
            for (size_t i = 0; i < sc.first.size(); ++i) {
                sk.push_back(ShapeKeyField{sc.first[i].ref, sc.first[i].value.kind, (uint32_t)sc.first[i].value.bytes.size()});
                en.key[i] = pad16(sc.first[i].value.bytes);
            }
            auto si = shape_index.find(sk);
            if (si == shape_index.end()) {
                si = shape_index.emplace(sk, (uint32_t)pd.shapes.size()).first;
                pd.shapes.push_back(sk);
                pd.shape_cols.emplace_back();
            }
            en.map = map;
            en.field0 = (uint32_t)fields.size();
            en.n_fields = (uint32_t)sc.second.size();
            for (const auto &fw : sc.second) {
                EnField f{};
                f.pcol = col_index[fw.first];
                f.prio = (((uint32_t)fw.second.weight << 24) | ((map ? 1u : 0u) << 23) | rank) + 1u;
                const PeerColumn &pc = pd.cols[f.pcol];
                if (pc.kind == NGZ_K_VLEN) {
                    const uint64_t off = intern(e, fw.second.value.bytes);
                    f.cell = make_uint4((uint32_t)off, (uint32_t)(off >> 32), (uint32_t)fw.second.value.bytes.size(), 0);
                } else {
                    f.cell = pad16(fw.second.value.bytes);
                }
                fields.push_back(f);
                pd.shape_cols[si->second].insert(f.pcol);
            }
            entry_shape.push_back(si->second);
            entries.push_back(en);
            ++rank;
        }
        return NGZ_OK;
    };
    if (scan_map(pm.global, 0)) return ngzs::fail(e, NGZ_E_LIMIT, "too many scopes in one map");
    uint32_t di = 0;
    for (const auto &d : pm.domain_scoped)
        if (scan_map(d.second, 1 + di++)) return ngzs::fail(e, NGZ_E_LIMIT, "too many scopes in one map");
    if (fields.size() >> 31 || entries.size() >> 31) return ngzs::fail(e, NGZ_E_LIMIT, "peer cache too large");
    // one open-addressing table per shape
    const size_t NSH = pd.shapes.size();
    std::vector<uint64_t> count(NSH, 0);
    for (uint32_t s : entry_shape) ++count[s];
    pd.shape_bits.assign(NSH, 0);
    pd.shape_slot0.assign(NSH, 0);
    uint64_t total_slots = 0;
    for (size_t s = 0; s < NSH; ++s) {
        uint32_t bits = e->table_bits ? (uint32_t)e->table_bits : 3;
        while (bits < 31 && (1ull << bits) < (e->table_bits ? count[s] + 1 : 2 * count[s] + 1)) ++bits;
        if (bits >= 31) return ngzs::fail(e, NGZ_E_LIMIT, "peer cache too large");
        pd.shape_bits[s] = bits;
        pd.shape_slot0[s] = total_slots;
        total_slots += 1ull << bits;
    }
    std::vector<uint32_t> slots(total_slots, 0);
    for (size_t i = 0; i < entries.size(); ++i) {
        const uint32_t s = entry_shape[i];
        const uint32_t m = (1u << pd.shape_bits[s]) - 1u;
        uint32_t h = en_hash(entries[i].map, entries[i].key, (uint32_t)pd.shapes[s].size()) & m;
        uint32_t *t = slots.data() + pd.shape_slot0[s];
        while (t[h]) h = (h + 1u) & m;
        t[h] = (uint32_t)i + 1u;
    }
    if (pd.d_entries.ensure(entries.size() + 1) || pd.d_fields.ensure(fields.size() + 1) ||
        pd.d_slots.ensure(total_slots + 1) || pd.d_domains.ensure(pd.domains.size() + 1))
        return ngzs::fail(e, NGZ_E_NOMEM, "enrichment tables");
    if (!entries.empty()) NGZ_STAGE_HIP(e, hipMemcpy(pd.d_entries.p, entries.data(), entries.size() * sizeof(EnEntry), hipMemcpyHostToDevice));
    if (!fields.empty()) NGZ_STAGE_HIP(e, hipMemcpy(pd.d_fields.p, fields.data(), fields.size() * sizeof(EnField), hipMemcpyHostToDevice));
    if (total_slots) NGZ_STAGE_HIP(e, hipMemcpy(pd.d_slots.p, slots.data(), total_slots * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!pd.domains.empty())
        NGZ_STAGE_HIP(e, hipMemcpy(pd.d_domains.p, pd.domains.data(), pd.domains.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (e->h_arena.size() > e->arena_uploaded) {
        if (e->d_arena.ensure(e->h_arena.size() + 1)) return ngzs::fail(e, NGZ_E_NOMEM, "value arena");
        NGZ_STAGE_HIP(e, hipMemcpy(e->d_arena.p, e->h_arena.data(), e->h_arena.size(), hipMemcpyHostToDevice));
        e->arena_uploaded = e->h_arena.size();
    }
    pd.generation = pm.generation;
    pd.table_bits = e->table_bits;
    return NGZ_OK;
}

}  // namespace

namespace ngze {
const std::vector<SlotResult> *results_for(const ngz_enrich *e, const ngz_ctx *ctx) {
    if (!e || !ctx) return nullptr;
    auto it = e->by_ctx.find(ctx);
    if (it == e->by_ctx.end() || !it->second->valid || it->second->serial != ctx->batch_serial) return nullptr;
    return &it->second->results;
}
int enrich_device(const ngz_enrich *e) { return e->device; }
}  // namespace ngze

extern "C" {

int ngz_enrich_abi_version(void) { return NGZ_ENRICH_ABI_VERSION; }

int ngz_enrich_create(int device, const char *writer_id, ngz_enrich **out) {
    if (!out) return NGZ_E_INVALID;
    *out = nullptr;
    if (device < 0 || !writer_id) return NGZ_E_INVALID;
    ngz_enrich *e = new ngz_enrich;
    e->device = device;
    e->writer_id = writer_id;
    *out = e;
    return NGZ_OK;
}

void ngz_enrich_destroy(ngz_enrich *e) {
    if (!e) return;
    if (e->device_ready) {
        hipSetDevice(e->device);
        for (auto &p : e->peers) p.second->release();
        e->d_arena.release();
        for (auto &c : e->by_ctx) {
            c.second->d_out.release();
            c.second->d_rowdom.release();
        }
        e->d_meta.release();
        e->d_counters.release();
    }
    delete e;
}

const char *ngz_enrich_last_error(ngz_enrich *e) { return e ? e->last_error.c_str() : "null enricher"; }
const char *ngz_enrich_writer_id(ngz_enrich *e) { return e ? e->writer_id.c_str() : ""; }

int ngz_enrich_set_option(ngz_enrich *e, int opt, int64_t value) {
    if (!e) return NGZ_E_INVALID;
    if (opt == NGZ_ENRICH_OPT_TABLE_BITS && (value == 0 || (value >= 3 && value <= 24))) {
        e->table_bits = value;
        return NGZ_OK;
    }
    return ngzs::fail(e, NGZ_E_INVALID, "option");
}

int ngz_enrich_op(ngz_enrich *e, const ngz_enrich_operation *op) {
    if (!e || !op) return NGZ_E_INVALID;
    if (op->n_scope && op->scope && op->n_scope <= NGZ_ENRICH_MAX_SCOPE_FIELDS)
        for (uint32_t i = 0; i < op->n_scope; ++i)
            if (!scope_ie_ok(op->scope[i]))
                return ngzs::fail(e, NGZ_E_LIMIT, "a scope field of a float, string, octet, list or unknown IE");
    std::string why;
    const int rc = e->cache.apply(*op, &why);
    if (rc) return ngzs::fail(e, rc, why);
    return NGZ_OK;
}

uint64_t ngz_enrich_peer_count(ngz_enrich *e) { return e ? e->cache.peer_count() : 0; }
uint64_t ngz_enrich_generation(ngz_enrich *e) { return e ? e->cache.generation() : 0; }

int ngz_enrich_lookup(ngz_enrich *e, const ngz_enrich_peer *peer, uint32_t obs_domain_id, const ngz_enrich_field *record,
                      uint32_t n_record, ngz_enrich_resolved *out, uint32_t cap) {
    if (!e || !peer || (n_record && !record) || (cap && !out)) return NGZ_E_INVALID;
    ngze::PeerIp ip;
    if (!ngze::peer_ip(peer, &ip)) return ngzs::fail(e, NGZ_E_INVALID, "peer address family");
    for (uint32_t i = 0; i < n_record; ++i)
        if (record[i].len && !record[i].value) return ngzs::fail(e, NGZ_E_INVALID, "record field without a value");
    const std::vector<ngze::Resolved> r = e->cache.lookup(ip, obs_domain_id, record, n_record);
    for (size_t i = 0; i < r.size() && i < cap; ++i) {
        ngz_enrich_resolved &o = out[i];
        memset(&o, 0, sizeof o);
        o.pen = r[i].ref.pen;
        o.ie_id = r[i].ref.ie;
        o.index = r[i].ref.index;
        o.kind = r[i].field->value.kind;
        o.weight = r[i].field->weight;
        o.len = (uint32_t)r[i].field->value.bytes.size();
        o.value = (const uint8_t *)r[i].field->value.bytes.data();
    }
    return (int)r.size();
}

int ngz_enrich_apply(ngz_enrich *e, ngz_ctx *ctx, const ngz_batch_out *out, const ngz_enrich_peer *peer,
                     ngz_enrich_stats *batch_stats, void *hip_stream) {
    if (!e || !ctx || !out || !peer) return NGZ_E_INVALID;
    if (batch_stats) memset(batch_stats, 0, sizeof *batch_stats);
    ngze::PeerIp ip;
    if (!ngze::peer_ip(peer, &ip)) return ngzs::fail(e, NGZ_E_INVALID, "peer address family");
    if (int rc = ngzs::check_ctx(e, ctx)) return rc;
    const uint32_t S = out->n_slots, D = out->n_dgrams, NS = out->n_sets;
    if (!ngzs::slot_table_ok(out)) return ngzs::fail(e, NGZ_E_INVALID, "slot table");
    if (int rc = ngzs::device_init(e)) return rc;
    NGZ_STAGE_HIP(e, hipSetDevice(e->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    // the results of an earlier apply for this context are void from here on
    std::unique_ptr<ngz_enrich::CtxResult> &cslot = e->by_ctx[ctx];
    if (!cslot) cslot.reset(new ngz_enrich::CtxResult);
    ngz_enrich::CtxResult &cr = *cslot;
    cr.valid = false;
    cr.results.clear();
    cr.h_out.clear();
    cr.h_rowdom.clear();
    e->apply_ms = 0;

    // the peer's tables
    const ngze::PeerMetadata *pm = e->cache.peer(ip);
    PeerDev *pd = nullptr;
    if (pm) {
        std::unique_ptr<PeerDev> &slot = e->peers[ip];
        if (!slot) slot.reset(new PeerDev);
        pd = slot.get();
        if (pd->generation != pm->generation || pd->table_bits != e->table_bits) {
            pd->generation = ~0ull;
            if (int rc = upload_peer(e, *pm, *pd)) return rc;
        }
    } else {
        auto it = e->peers.find(ip);
        if (it != e->peers.end()) {
            it->second->release();
            e->peers.erase(it);
        }
    }

    // per-slot plans from the slot's column layout; nothing is launched before every slot checked out
    struct SlotWork {
        EnPlan k;
        bool launches;
        std::vector<uint64_t> col_off;  // of each added column in d_out
        uint64_t mask_off;
    };
    std::vector<SlotWork> work(S);
    std::vector<ngze::SlotResult> results(S);
    std::vector<ngz_field_info> fi;
    std::vector<uint64_t> row_off(S, 0);
    std::vector<uint32_t> slot_rows(S, 0);
    uint64_t rowdom_bytes = 0, out_bytes = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t off = out_bytes;
        out_bytes += (bytes + 255) & ~255ull;
        return off;
    };
    for (uint32_t s = 0; s < S; ++s) {
        const ngz_slot_info &si = out->slots[s];
        SlotWork &w = work[s];
        memset(&w.k, 0, sizeof w.k);
        w.launches = false;
        slot_rows[s] = si.n_records;
        results[s].rows = si.n_records;
        row_off[s] = rowdom_bytes;
        const uint64_t rows4 = ((uint64_t)si.n_records + 3) & ~3ull;
        rowdom_bytes += ((uint64_t)si.n_records + 15) & ~15ull;  // 16-byte aligned, room for a last quad
        w.mask_off = take(rows4 * 4);
        if (!si.n_records) continue;
        const int nf = ngzs::slot_fields(e, ctx, s, fi);
        if (nf < 0) return nf;
        // FieldRef -> field of the template's non-scope fields (occurrence index per IE, cache.rs:452-453)
        std::map<ngze::FieldRef, int> by_ref;
        std::map<std::pair<uint32_t, uint16_t>, uint16_t> seen;
        for (int i = 0; i < nf; ++i) {
            if (fi[i].is_scope) { results[s].dropped = true; continue; }
            ngze::FieldRef r;
            r.pen = fi[i].pen;
            r.ie = fi[i].ie_id;
            r.index = seen[{fi[i].pen, fi[i].ie_id}]++;
            by_ref[r] = i;
        }
        if (results[s].dropped || !pd) continue;
        std::set<uint32_t> pcols;
        for (size_t sh = 0; sh < pd->shapes.size(); ++sh) {
            const ShapeKey &sk = pd->shapes[sh];
            bool candidate = true;
            int field_of[NGZ_ENRICH_MAX_SCOPE_FIELDS] = {0, 0, 0, 0};
            for (size_t f = 0; candidate && f < sk.size(); ++f) {
                auto it = by_ref.find(sk[f].ref);
                candidate = it != by_ref.end() && fi[it->second].kind == sk[f].kind && fi[it->second].width == sk[f].len;
                if (candidate) field_of[f] = it->second;
            }
            if (!candidate) continue;
            if (w.k.n_shapes == NGZ_ENRICH_MAX_SHAPES) return ngzs::fail(e, NGZ_E_LIMIT, "a slot plan with more than 8 scope shapes");
            EnShape &ks = w.k.shape[w.k.n_shapes++];
            ks.slots = pd->d_slots.p + pd->shape_slot0[sh];
            ks.bits = pd->shape_bits[sh];
            ks.n = (uint32_t)sk.size();
            for (size_t f = 0; f < sk.size(); ++f) {
                ks.col[f] = si.columns + (uint64_t)si.capacity * fi[field_of[f]].col_off;
                ks.w[f] = sk[f].len;
            }
            pcols.insert(pd->shape_cols[sh].begin(), pd->shape_cols[sh].end());
        }
        if (!w.k.n_shapes) continue;
        if (pcols.size() > NGZ_ENRICH_MAX_COLUMNS) return ngzs::fail(e, NGZ_E_LIMIT, "a slot plan with more than 32 added columns");
        if (!si.columns || ((uintptr_t)si.columns & 15) || (si.capacity & 3) || si.capacity < si.n_records)
            return ngzs::fail(e, NGZ_E_LIMIT, "unexpected column block alignment");
        w.launches = true;
        for (uint32_t pc : pcols) {  // ascending peer column = ascending FieldRef
            const PeerColumn &c = pd->cols[pc];
            const uint32_t k = w.k.n_cols++;
            w.k.pcol[k] = (uint16_t)pc;
            w.k.w[k] = (uint8_t)c.width;
            w.col_off.push_back(take(rows4 * c.width));
            ngz_enrich_column rc{};
            rc.pen = c.ref.pen;
            rc.ie_id = c.ref.ie;
            rc.index = c.ref.index;
            rc.kind = c.kind;
            rc.is_string = c.is_string;
            rc.value_kind = c.value_kind;
            rc.width = c.width;
            results[s].cols.push_back(rc);
        }
        w.k.n_rows = si.n_records;
        w.k.entries = pd->d_entries.p;
        w.k.fields = pd->d_fields.p;
    }
    if (rowdom_bytes >> 40 || out_bytes >> 44) return ngzs::fail(e, NGZ_E_LIMIT, "batch too large");
    const size_t n_counters = EN_STATS + 1 + S;
    const size_t n_meta = 2ull * S + 2;
    if (cr.d_out.ensure(out_bytes + 256) || cr.d_rowdom.ensure(rowdom_bytes + 16) || e->d_meta.ensure(n_meta) ||
        e->d_counters.ensure(n_counters) || e->h_meta.reserve(n_meta) || e->h_counters.reserve(n_counters))
        return ngzs::fail(e, NGZ_E_NOMEM, "enricher buffers");
    uint32_t *h_rows = (uint32_t *)(e->h_meta.p + S);
    for (uint32_t s = 0; s < S; ++s) {
        e->h_meta.p[s] = row_off[s];
        h_rows[s] = slot_rows[s];
    }
    NGZ_STAGE_HIP(e, hipEventRecord(e->ev[0], st));
    if (S) NGZ_STAGE_HIP(e, hipMemcpyAsync(e->d_meta.p, e->h_meta.p, n_meta * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    NGZ_STAGE_HIP(e, hipMemsetAsync(e->d_counters.p, 0, n_counters * sizeof(unsigned long long), st));
    NGZ_STAGE_HIP(e, hipMemsetAsync(cr.d_rowdom.p, 0, rowdom_bytes + 16, st));
    unsigned long long *d_stats = e->d_counters.p, *d_bad = e->d_counters.p + EN_STATS + 1;
    unsigned int *d_err = (unsigned int *)(e->d_counters.p + EN_STATS);
    if (NS && D && S) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(((uint64_t)NS + 255) / 256, (uint64_t)e->n_cus * 8);
        hipLaunchKernelGGL(k_enrich_sets, dim3(nb), dim3(256), 0, st, out->sets, NS, out->dgrams, D, S,
                           (const uint32_t *)(e->d_meta.p + S), (const uint64_t *)e->d_meta.p, cr.d_rowdom.p,
                           pd ? (const uint32_t *)pd->d_domains.p : nullptr, pd ? (uint32_t)pd->domains.size() : 0u, d_bad, d_err);
        NGZ_STAGE_HIP(e, hipGetLastError());
    }
    uint32_t launches = 0;
    for (uint32_t s = 0; s < S; ++s) {
        SlotWork &w = work[s];
        if (!slot_rows[s]) continue;
        uint32_t *mask = (uint32_t *)(cr.d_out.p + w.mask_off);
        results[s].mask = mask;
        if (!w.launches) {  // its masks read 0
            NGZ_STAGE_HIP(e, hipMemsetAsync(mask, 0, (((uint64_t)slot_rows[s] + 3) & ~3ull) * 4, st));
            continue;
        }
        for (uint32_t c = 0; c < w.k.n_cols; ++c) {
            w.k.out[c] = cr.d_out.p + w.col_off[c];
            results[s].cols[c].data = w.k.out[c];
        }
        w.k.mask = mask;
        w.k.rowdom = cr.d_rowdom.p + row_off[s];
        w.k.stats = d_stats;
        const uint64_t quads = ((uint64_t)slot_rows[s] + EN_ROWS_PER_LANE - 1) / EN_ROWS_PER_LANE;
        const uint32_t nb = (uint32_t)std::min<uint64_t>((quads + EN_THREADS - 1) / EN_THREADS, (uint64_t)e->n_cus * 16);
        hipLaunchKernelGGL(k_enrich, dim3(nb), dim3(EN_THREADS), 0, st, w.k);
        NGZ_STAGE_HIP(e, hipGetLastError());
        ++launches;
    }
    NGZ_STAGE_HIP(e, hipEventRecord(e->ev[1], st));
    NGZ_STAGE_HIP(e, hipMemcpyAsync(e->h_counters.p, e->d_counters.p, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    NGZ_STAGE_HIP(e, hipStreamSynchronize(st));
    NGZ_STAGE_HIP(e, hipEventElapsedTime(&e->apply_ms, e->ev[0], e->ev[1]));
    const unsigned long long *hc = e->h_counters.p;
    if (hc[EN_STATS] & 1) return ngzs::fail_sets(e);
    ngz_enrich_stats bs{};
    bs.records_matched = hc[0];
    bs.fields_added = hc[1];
    for (uint32_t s = 0; s < S; ++s) {
        if (!slot_rows[s]) continue;
        const uint64_t ok_rows = ngzs::ok_rows(slot_rows[s], hc[EN_STATS + 1 + s]);
        if (results[s].dropped) bs.records_dropped += ok_rows;
        else bs.records_processed += ok_rows;
    }
    e->totals.records_processed += bs.records_processed;
    e->totals.records_matched += bs.records_matched;
    e->totals.fields_added += bs.fields_added;
    e->totals.records_dropped += bs.records_dropped;
    if (batch_stats) *batch_stats = bs;
    cr.results = std::move(results);
    cr.row_off = row_off;
    cr.out_bytes = out_bytes;
    cr.rowdom_bytes = rowdom_bytes;
    cr.serial = ctx->batch_serial;
    cr.valid = true;
    return NGZ_OK;
}

int ngz_enrich_totals(ngz_enrich *e, ngz_enrich_stats *totals, int reset) {
    if (!e || !totals) return NGZ_E_INVALID;
    *totals = e->totals;
    if (reset) e->totals = ngz_enrich_stats{};
    return NGZ_OK;
}

int ngz_enrich_slot_columns(ngz_enrich *e, ngz_ctx *ctx, uint32_t slot, ngz_enrich_column *cols, uint32_t cap,
                            const uint32_t **dev_mask, uint32_t *n) {
    if (!e || !ctx || (cap && !cols)) return NGZ_E_INVALID;
    const std::vector<ngze::SlotResult> *res = ngze::results_for(e, ctx);
    if (!res) return ngzs::fail(e, NGZ_E_INVALID, "the context's last batch is not the batch last applied on it");
    if (slot >= res->size()) return ngzs::fail(e, NGZ_E_INVALID, "no such slot in the batch last applied");
    const ngze::SlotResult &r = (*res)[slot];
    for (size_t i = 0; i < r.cols.size() && i < cap; ++i) cols[i] = r.cols[i];
    if (dev_mask) *dev_mask = r.mask;
    if (n) *n = r.rows;
    return (int)r.cols.size();
}

int ngz_enrich_row_fields(ngz_enrich *e, ngz_ctx *ctx, uint32_t slot, uint32_t row, ngz_field_value *out, uint32_t cap) {
    if (!e || !ctx || (cap && !out)) return NGZ_E_INVALID;
    if (!ngze::results_for(e, ctx)) return ngzs::fail(e, NGZ_E_INVALID, "the context's last batch is not the batch last applied on it");
    ngz_enrich::CtxResult &cr = *e->by_ctx[ctx];
    if (slot >= cr.results.size() || row >= cr.results[slot].rows) return ngzs::fail(e, NGZ_E_INVALID, "no such row");
    if (cr.h_out.empty()) {  // one D2H of the masks, the added columns and the row bytes
        NGZ_STAGE_HIP(e, hipSetDevice(e->device));
        cr.h_out.resize(cr.out_bytes + 1);
        cr.h_rowdom.resize(cr.rowdom_bytes + 1);
        if (cr.out_bytes) NGZ_STAGE_HIP(e, hipMemcpy(cr.h_out.data(), cr.d_out.p, cr.out_bytes, hipMemcpyDeviceToHost));
        if (cr.rowdom_bytes) NGZ_STAGE_HIP(e, hipMemcpy(cr.h_rowdom.data(), cr.d_rowdom.p, cr.rowdom_bytes, hipMemcpyDeviceToHost));
    }
    const ngze::SlotResult &r = cr.results[slot];
    // a record the reference never enriches: one with scope fields, or of a message that did not decode
    if (r.dropped || !cr.h_rowdom[cr.row_off[slot] + row]) return ngzs::fail(e, NGZ_E_INVALID, "the row is not an enriched record");
    uint32_t mask;
    memcpy(&mask, cr.h_out.data() + ((const uint8_t *)r.mask - cr.d_out.p) + 4ull * row, 4);
    uint32_t n = 0;
    auto put = [&](const ngz_field_value &fv) {
        if (n < cap) out[n] = fv;
        ++n;
    };
    for (size_t c = 0; c < r.cols.size(); ++c) {
        if (!((mask >> c) & 1u)) continue;
        const ngz_enrich_column &col = r.cols[c];
        const uint8_t *cell = cr.h_out.data() + (col.data - cr.d_out.p) + (uint64_t)col.width * row;
        const ngzh::IeRow *ie = ngzh::ie_find(col.pen, col.ie_id);
        ngz_field_value fv{};
        fv.pen = col.pen;
        fv.ie_id = col.ie_id;
        fv.kind = col.kind;
        fv.dtype = ie ? ie->dtype : (uint8_t)NGZ_DT_OCTET_ARRAY;
        fv.width = col.width;
        fv.flags = (col.is_string ? NGZ_FV_STRING : 0u) | (col.pen ? NGZ_FV_VENDOR : 0u) | (ie ? 0u : NGZ_FV_UNKNOWN) |
                   (ie && (ie->flags & 4) ? NGZ_FV_SUBREG : 0u);
        if (col.kind == NGZ_K_VLEN) {  // {u64 offset into the value arena, u32 length, u32 0}
            uint64_t off;
            uint32_t len;
            memcpy(&off, cell, 8);
            memcpy(&len, cell + 8, 4);
            fv.wire_length = 0xFFFF;
            fv.len = len;
            fv.value = e->h_arena.data() + off;
            if (col.value_kind && col.value_kind != NGZ_K_STR) {  // a long fixed value: its own kind
                fv.kind = col.value_kind;
                fv.width = (uint16_t)len;
                fv.wire_length = (uint16_t)len;
            }
        } else {
            fv.wire_length = col.width;
            fv.len = col.width;
            fv.value = cell;
        }
        put(fv);
    }
    ngz_field_value w{};  // Field::NetGauze(dataCollectionManifestName(writer_id)), last (actor.rs:122-271)
    w.pen = 3746;
    w.ie_id = 7;
    w.kind = NGZ_K_VLEN;
    w.dtype = NGZ_DT_STRING;
    w.wire_length = 0xFFFF;
    w.width = 16;
    w.len = (uint32_t)e->writer_id.size();
    w.flags = NGZ_FV_STRING | NGZ_FV_VENDOR;
    w.value = (const uint8_t *)e->writer_id.data();
    put(w);
    return (int)n;
}

int ngz_enrich_forget(ngz_enrich *e, ngz_ctx *ctx) {
    if (!e || !ctx) return NGZ_E_INVALID;
    auto it = e->by_ctx.find(ctx);
    if (it == e->by_ctx.end()) return NGZ_OK;
    if (e->device_ready) {
        hipSetDevice(e->device);
        it->second->d_out.release();
        it->second->d_rowdom.release();
    }
    e->by_ctx.erase(it);
    return NGZ_OK;
}

int64_t ngz_enrich_batch_json(ngz_enrich *e, ngz_renorm *renorm, ngz_ctx *ctx, const uint8_t *host_bytes, ngz_json_line_fn fn,
                              void *user) {
    if (!e || !ctx || !fn) return NGZ_E_INVALID;
    if (!ngze::results_for(e, ctx) || ctx->async.pending.load())
        return ngzs::fail(e, NGZ_E_INVALID, "the context's last batch is not the batch last applied on it");
    ngz_enrich::CtxResult &cr = *e->by_ctx[ctx];
    const size_t S = cr.results.size();
    if (S != ctx->slot_infos.size()) return ngzs::fail(e, NGZ_E_INVALID, "slot table");
    NGZ_STAGE_HIP(e, hipSetDevice(e->device));
    if (cr.h_out.empty()) {
        cr.h_out.resize(cr.out_bytes + 1);
        cr.h_rowdom.resize(cr.rowdom_bytes + 1);
        if (cr.out_bytes) NGZ_STAGE_HIP(e, hipMemcpy(cr.h_out.data(), cr.d_out.p, cr.out_bytes, hipMemcpyDeviceToHost));
        if (cr.rowdom_bytes) NGZ_STAGE_HIP(e, hipMemcpy(cr.h_rowdom.data(), cr.d_rowdom.p, cr.rowdom_bytes, hipMemcpyDeviceToHost));
    }
    ngzh::RenormJson mode;
    std::vector<uint8_t> flags;
    mode.slot_flags.assign(S, nullptr);
    if (renorm) {
        if (const int rc = ngzh::renorm_flags_host(renorm, ctx, flags, mode.slot_flags))
            return ngzs::fail(e, rc, "the renormalizer has not applied the context's last batch");
        if (mode.slot_flags.size() != S) return ngzs::fail(e, NGZ_E_INVALID, "slot table");
    }
    mode.enrich.resize(S);
    for (size_t s = 0; s < S; ++s) {
        const ngze::SlotResult &r = cr.results[s];
        if (!r.rows) continue;
        mode.enrich[s].mask = (const uint32_t *)(cr.h_out.data() + ((const uint8_t *)r.mask - cr.d_out.p));
        for (const ngz_enrich_column &c : r.cols)
            mode.enrich[s].cols.push_back(ngzh::EnrichJsonCol{c.pen, c.ie_id, c.kind, c.is_string, c.width,
                                                              cr.h_out.data() + (c.data - cr.d_out.p)});
    }
    mode.arena = e->h_arena.data();
    {  // Field::NetGauze(dataCollectionManifestName(writer_id)), rendered once
        uint8_t cell[16] = {};
        const uint32_t n = (uint32_t)e->writer_id.size();
        memcpy(cell + 8, &n, 4);
        ngzh::json_put_added(mode.writer_field, ngzh::EnrichJsonCol{3746, 7, NGZ_K_VLEN, 1, 16, nullptr}, cell,
                             (const uint8_t *)e->writer_id.data());
    }
    ngzh::JsonView v;
    const int rc = ngzh::json_view_load(ctx, host_bytes, v);
    if (rc) return ngzs::fail(e, rc, "json_view_load");
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

// The decode rule of one template field where a scope can key on it (the kinds of
// ngze::scope_kind_ok): kind and column width by the IE's data type, as the decoder's field rule
// (generator.rs:1439-1807); 0: a column no scope matches
static void plan_rule(uint32_t pen, uint16_t ie, uint32_t L, uint8_t *kind, uint16_t *width) {
    *kind = 0;
    *width = 0;
    const ngzh::IeRow *row = ngzh::ie_find(pen, ie);
    if (!row) return;
    auto set = [&](bool ok, uint8_t k, uint16_t w) {
        if (ok) { *kind = k; *width = w; }
    };
    switch (row->dtype) {
    case ngzh::DT_unsigned8: set(L == 1, NGZ_K_UINT, 1); break;
    case ngzh::DT_unsigned16:
        if (row->flags & 2) set(L == 1 || L == 2, NGZ_K_TCPFLAGS, 1);
        else set(L == 1 || L == 2, NGZ_K_UINT, 2);
        break;
    case ngzh::DT_unsigned32: set(L >= 1 && L <= 4, NGZ_K_UINT, 4); break;
    case ngzh::DT_unsigned64: set(L >= 1 && L <= 8, NGZ_K_UINT, 8); break;
    case ngzh::DT_signed8: set(L == 1, NGZ_K_SINT, 1); break;
    case ngzh::DT_signed16: set(L == 1 || L == 2, NGZ_K_SINT, 2); break;
    case ngzh::DT_signed32: set(L >= 1 && L <= 4, NGZ_K_SINT, 4); break;
    case ngzh::DT_signed64: set(L >= 1 && L <= 8, NGZ_K_SINT, 8); break;
    case ngzh::DT_boolean: set(L == 1, NGZ_K_BOOL, 1); break;
    case ngzh::DT_macAddress: set(L == 6, NGZ_K_BYTES, 6); break;
    case ngzh::DT_ipv4Address: set(L == 4, NGZ_K_UINT, 4); break;
    case ngzh::DT_ipv6Address: set(L == 16, NGZ_K_BYTES, 16); break;
    case ngzh::DT_dateTimeSeconds: set(L == 4, NGZ_K_UINT, 4); break;
    case ngzh::DT_dateTimeMilliseconds: set(L == 8, NGZ_K_DTMS, 8); break;
    default: break;
    }
}

int ngz_enrich_template_plan(ngz_enrich *e, const ngz_enrich_peer *peer, const uint8_t *tmpl, size_t len, int proto,
                             ngz_enrich_plan *out) {
    if (!e || !peer || !tmpl || !out) return NGZ_E_INVALID;
    memset(out, 0, sizeof *out);
    ngze::PeerIp ip;
    if (!ngze::peer_ip(peer, &ip)) return ngzs::fail(e, NGZ_E_INVALID, "peer address family");
    const bool options = (proto & NGZ_ENRICH_OPTIONS) != 0;
    proto &= ~NGZ_ENRICH_OPTIONS;
    if (proto != 10 && proto != 9) return ngzs::fail(e, NGZ_E_INVALID, "protocol");
    std::map<ngze::FieldRef, std::pair<uint8_t, uint16_t>> by_ref;  // non-scope FieldRef -> column kind, width
    std::map<std::pair<uint32_t, uint16_t>, uint16_t> seen;
    const int rc = ngzt::walk_template_record(tmpl, len, proto, options, [&](const ngzt::FieldSpec &f) {
        if (f.scope) { out->dropped = 1; return; }
        ngze::FieldRef r;
        r.pen = f.pen;
        r.ie = f.ie;
        r.index = seen[{f.pen, f.ie}]++;
        uint8_t kind;
        uint16_t width;
        plan_rule(f.pen, f.ie, f.length, &kind, &width);
        by_ref[r] = {kind, width};
    });
    if (rc) return ngzs::fail(e, rc, "template record");
    const ngze::PeerMetadata *pm = e->cache.peer(ip);
    if (out->dropped || !pm) return NGZ_OK;
    std::map<ngze::FieldRef, PeerColumn> colmap;
    peer_columns(*pm, colmap);
    std::map<ShapeKey, std::set<ngze::FieldRef>> shapes;  // every shape of the peer -> the FieldRefs its scopes add
    auto scan = [&](const ngze::ScopeMap &m) {
        for (const auto &sc : m) {
            std::set<ngze::FieldRef> &adds = shapes[shape_of(sc.first)];
            for (const auto &fw : sc.second) adds.insert(fw.first);
        }
    };
    scan(pm->global);
    for (const auto &d : pm->domain_scoped) scan(d.second);
    std::set<ngze::FieldRef> cols;
    std::vector<const ShapeKey *> cand;
    for (const auto &sh : shapes) {
        bool ok = true;
        for (const ShapeKeyField &f : sh.first) {
            auto it = by_ref.find(f.ref);
            ok = ok && it != by_ref.end() && it->second.first == f.kind && it->second.second == f.len;
        }
        if (!ok) continue;
        cand.push_back(&sh.first);
        cols.insert(sh.second.begin(), sh.second.end());
    }
    if (cand.size() > NGZ_ENRICH_MAX_SHAPES) return ngzs::fail(e, NGZ_E_LIMIT, "a slot plan with more than 8 scope shapes");
    if (cols.size() > NGZ_ENRICH_MAX_COLUMNS) return ngzs::fail(e, NGZ_E_LIMIT, "a slot plan with more than 32 added columns");
    out->n_shapes = (uint8_t)cand.size();
    for (size_t s = 0; s < cand.size(); ++s) {
        out->shape_len[s] = (uint8_t)cand[s]->size();
        for (size_t f = 0; f < cand[s]->size(); ++f)
            out->shape[s][f] = ngz_enrich_ref{(*cand[s])[f].ref.pen, (*cand[s])[f].ref.ie, (*cand[s])[f].ref.index};
    }
    out->launches = cand.empty() ? 0 : 1;
    for (const ngze::FieldRef &r : cols) {
        const PeerColumn &pc = colmap[r];
        const uint32_t c = out->n_columns++;
        out->column[c] = ngz_enrich_ref{r.pen, r.ie, r.index};
        out->column_kind[c] = pc.kind;
        out->column_width[c] = pc.width;
    }
    return NGZ_OK;
}

int ngz_enrich_value_arena(ngz_enrich *e, const uint8_t **dev, const uint8_t **host, uint64_t *size) {
    if (!e) return NGZ_E_INVALID;
    if (dev) *dev = e->arena_uploaded ? e->d_arena.p : nullptr;
    if (host) *host = e->h_arena.data();
    if (size) *size = e->arena_uploaded;
    return NGZ_OK;
}

int ngz_enrich_last_timing(ngz_enrich *e, float *apply_ms) {
    if (!e || !apply_ms) return NGZ_E_INVALID;
    *apply_ms = e->apply_ms;
    return NGZ_OK;
}

}  // extern "C"
