// The enrichment cache on the host (include/ngz/flow_enrich.h): the reference's EnrichmentCache
// (crates/collector/src/flow/enrichment/cache.rs:60-529), its three operations and the
// per-record lookup.  No HIP: builds with a plain C++17 compiler (tests/native/enrich_cache_check.cpp).
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "ngz/flow_enrich.h"

namespace ngze {

struct FieldRef {  // FieldRef(IE, occurrence index); ordered by (PEN, IE id, index)
    uint32_t pen = 0;
    uint16_t ie = 0;
    uint16_t index = 0;
    bool operator<(const FieldRef &o) const {
        return pen != o.pen ? pen < o.pen : ie != o.ie ? ie < o.ie : index < o.index;
    }
    bool operator==(const FieldRef &o) const { return pen == o.pen && ie == o.ie && index == o.index; }
};

struct Value {  // a Field's value in the canonical column encoding
    uint8_t kind = 0;
    std::string bytes;
    bool operator==(const Value &o) const { return kind == o.kind && bytes == o.bytes; }
};

// -1 / 0 / 1: the order of two values of one IE (unsigned and signed integers by value, else bytewise)
int value_cmp(const Value &a, const Value &b);

struct ScopeField {
    FieldRef ref;
    Value value;
};
using ScopeKey = std::vector<ScopeField>;  // IndexedScopeFields (cache.rs:338-361)
struct ScopeLess {                         // Ord of Box<[(FieldRef, Field)]>: lexicographic, a prefix first
    bool operator()(const ScopeKey &a, const ScopeKey &b) const;
};

struct Weighted {  // WeightedField (cache.rs:380-395)
    uint8_t weight = 0;
    Value value;
};
using Metadata = std::map<FieldRef, Weighted>;           // IndexedMetadata
using ScopeMap = std::map<ScopeKey, Metadata, ScopeLess>;

struct PeerMetadata {  // cache.rs:406-410
    ScopeMap global;
    std::map<uint32_t, ScopeMap> domain_scoped;
    uint64_t generation = 0;  // the cache generation that last changed this peer
};

using PeerIp = std::array<uint8_t, 17>;  // family, 16 address bytes
// false: the family is neither 4 nor 6
bool peer_ip(const ngz_enrich_peer *p, PeerIp *out);

struct Resolved {
    FieldRef ref;
    const Weighted *field;
};

// FieldRef of each field of a list: the occurrence index counted per IE (FieldRef::map_fields)
std::vector<FieldRef> index_fields(const ngz_enrich_field *f, uint32_t n);
// is `kind` with `len` bytes a scope value the device tables can key on
bool scope_kind_ok(uint8_t kind, uint32_t len);

class Cache {
  public:
    // EnrichmentCache::apply_enrichment (cache.rs:96-120).  NGZ_OK, NGZ_E_INVALID or NGZ_E_LIMIT;
    // *why names the refusal.  Only NGZ_OK can have changed the cache.
    int apply(const ngz_enrich_operation &op, std::string *why);
    // get_enrichment_fields (cache.rs:84-93, 437-528) in ascending FieldRef
    std::vector<Resolved> lookup(const PeerIp &ip, uint32_t obs_domain_id, const ngz_enrich_field *record,
                                 uint32_t n_record) const;
    const PeerMetadata *peer(const PeerIp &ip) const;
    uint64_t peer_count() const { return peers_.size(); }
    uint64_t generation() const { return generation_; }

  private:
    bool upsert(const PeerIp &ip, uint32_t domain, const ScopeKey &scope, uint8_t weight, const ngz_enrich_operation &op);
    bool remove(const PeerIp &ip, uint32_t domain, const ScopeKey &scope, uint8_t weight, const ngz_enrich_operation &op,
                bool all);
    std::map<PeerIp, PeerMetadata> peers_;
    uint64_t generation_ = 0;
};

}  // namespace ngze
