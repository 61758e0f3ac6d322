// The enrichment cache on the host: see ngz_enrich_cache.h.  No HIP in this unit.
#include "ngz_enrich_cache.h"

#include <algorithm>
#include <cstring>

namespace ngze {

namespace {

// little-endian integer of up to 16 bytes as (hi, lo)
void le128(const std::string &b, bool is_signed, uint64_t *hi, uint64_t *lo) {
    uint8_t v[16];
    const size_t n = std::min<size_t>(b.size(), 16);
    const uint8_t fill = (is_signed && n && (uint8_t)b[n - 1] & 0x80) ? 0xFF : 0;
    memset(v, fill, sizeof v);
    memcpy(v, b.data(), n);
    *lo = *hi = 0;
    for (int i = 7; i >= 0; --i) {
        *lo = (*lo << 8) | v[i];
        *hi = (*hi << 8) | v[8 + i];
    }
    if (is_signed) *hi ^= 0x8000000000000000ull;  // order as unsigned
}

bool value_kind_ok(uint8_t kind) {
    switch (kind) {
    case NGZ_K_UINT: case NGZ_K_TCPFLAGS: case NGZ_K_SINT: case NGZ_K_BOOL: case NGZ_K_BYTES: case NGZ_K_U256:
    case NGZ_K_DTMS: case NGZ_K_DTFRAC: case NGZ_K_STR:
        return true;
    }
    return false;
}

Value value_of(const ngz_enrich_field &f) {
    Value v;
    v.kind = f.kind;
    if (f.len) v.bytes.assign((const char *)f.value, f.len);
    return v;
}

bool fields_ok(const ngz_enrich_field *f, uint32_t n) {
    if (n && !f) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (!value_kind_ok(f[i].kind) || (f[i].len && !f[i].value)) return false;
    return true;
}

}  // namespace

int value_cmp(const Value &a, const Value &b) {
    if (a.kind != b.kind) return a.kind < b.kind ? -1 : 1;
    const bool is_signed = a.kind == NGZ_K_SINT || a.kind == NGZ_K_DTMS;
    if ((a.kind == NGZ_K_UINT || a.kind == NGZ_K_BOOL || a.kind == NGZ_K_TCPFLAGS || is_signed) && a.bytes.size() <= 16 &&
        b.bytes.size() <= 16) {
        uint64_t ah, al, bh, bl;
        le128(a.bytes, is_signed, &ah, &al);
        le128(b.bytes, is_signed, &bh, &bl);
        if (ah != bh) return ah < bh ? -1 : 1;
        if (al != bl) return al < bl ? -1 : 1;
        // one IE has one width; values given with another stay scopes of their own
        if (a.bytes.size() != b.bytes.size()) return a.bytes.size() < b.bytes.size() ? -1 : 1;
        return 0;
    }
    const int c = a.bytes.compare(b.bytes);
    return c < 0 ? -1 : c > 0 ? 1 : 0;
}

bool ScopeLess::operator()(const ScopeKey &a, const ScopeKey &b) const {
    const size_t n = std::min(a.size(), b.size());
    // the generated IE enum declares Unknown, then every vendor's IEs, then the IANA IEs
    // (ipfix-code-generator/src/generator.rs:1160-1164): a vendor IE orders before an IANA one
    auto ref_less = [](const FieldRef &x, const FieldRef &y) {
        if ((x.pen == 0) != (y.pen == 0)) return y.pen == 0;
        return x < y;
    };
    for (size_t i = 0; i < n; ++i) {
        if (ref_less(a[i].ref, b[i].ref)) return true;
        if (ref_less(b[i].ref, a[i].ref)) return false;
        const int c = value_cmp(a[i].value, b[i].value);
        if (c) return c < 0;
    }
    return a.size() < b.size();
}

bool peer_ip(const ngz_enrich_peer *p, PeerIp *out) {
    if (!p || (p->family != 4 && p->family != 6)) return false;
    out->fill(0);
    (*out)[0] = p->family;
    memcpy(out->data() + 1, p->addr, p->family == 4 ? 4 : 16);
    return true;
}

std::vector<FieldRef> index_fields(const ngz_enrich_field *f, uint32_t n) {
    std::vector<FieldRef> out(n);
    std::map<std::pair<uint32_t, uint16_t>, uint16_t> seen;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].pen = f[i].pen;
        out[i].ie = f[i].ie_id;
        out[i].index = seen[{f[i].pen, f[i].ie_id}]++;
    }
    return out;
}

bool scope_kind_ok(uint8_t kind, uint32_t len) {
    if (len < 1 || len > NGZ_ENRICH_MAX_KEY_BYTES) return false;
    switch (kind) {
    case NGZ_K_UINT: case NGZ_K_SINT: return len == 1 || len == 2 || len == 4 || len == 8;
    case NGZ_K_BOOL: case NGZ_K_TCPFLAGS: return len == 1;
    case NGZ_K_DTMS: return len == 8;
    case NGZ_K_BYTES: return true;
    }
    return false;
}

const PeerMetadata *Cache::peer(const PeerIp &ip) const {
    auto it = peers_.find(ip);
    return it == peers_.end() ? nullptr : &it->second;
}

int Cache::apply(const ngz_enrich_operation &op, std::string *why) {
    auto refuse = [&](int rc, const char *msg) {
        if (why) *why = msg;
        return rc;
    };
    if (op.kind != NGZ_ENRICH_UPSERT && op.kind != NGZ_ENRICH_DELETE && op.kind != NGZ_ENRICH_DELETE_ALL)
        return refuse(NGZ_E_INVALID, "operation kind");
    PeerIp ip;
    if (!peer_ip(&op.peer, &ip)) return refuse(NGZ_E_INVALID, "peer address family");
    if (!fields_ok(op.scope, op.n_scope)) return refuse(NGZ_E_INVALID, "scope fields");
    if (op.kind == NGZ_ENRICH_UPSERT && !fields_ok(op.fields, op.n_fields)) return refuse(NGZ_E_INVALID, "fields");
    if (op.kind == NGZ_ENRICH_DELETE && op.n_ies && !op.ies) return refuse(NGZ_E_INVALID, "ies");
    if (op.n_scope > NGZ_ENRICH_MAX_SCOPE_FIELDS) return refuse(NGZ_E_LIMIT, "more than 4 scope fields");
    for (uint32_t i = 0; i < op.n_scope; ++i)
        if (!scope_kind_ok(op.scope[i].kind, op.scope[i].len))
            return refuse(NGZ_E_LIMIT, "a scope field of a kind or length the lookup tables cannot key on");
    const std::vector<FieldRef> refs = index_fields(op.scope, op.n_scope);
    ScopeKey scope(op.n_scope);
    for (uint32_t i = 0; i < op.n_scope; ++i) scope[i] = ScopeField{refs[i], value_of(op.scope[i])};
    bool changed;
    if (op.kind == NGZ_ENRICH_UPSERT) changed = upsert(ip, op.obs_domain_id, scope, op.weight, op);
    else changed = remove(ip, op.obs_domain_id, scope, op.weight, op, op.kind == NGZ_ENRICH_DELETE_ALL);
    if (changed) {
        ++generation_;
        auto it = peers_.find(ip);
        if (it != peers_.end()) it->second.generation = generation_;
    }
    return NGZ_OK;
}

// cache.rs:128-232
bool Cache::upsert(const PeerIp &ip, uint32_t domain, const ScopeKey &scope, uint8_t weight, const ngz_enrich_operation &op) {
    if (!op.n_fields) return false;  // :136-152
    const std::vector<FieldRef> refs = index_fields(op.fields, op.n_fields);
    PeerMetadata &pm = peers_[ip];
    ScopeMap &target = domain == 0 ? pm.global : pm.domain_scoped[domain];
    Metadata &md = target[scope];
    bool changed = false;
    for (uint32_t i = 0; i < op.n_fields; ++i) {
        Weighted w{weight, value_of(op.fields[i])};
        auto it = md.find(refs[i]);
        if (it == md.end()) {
            md.emplace(refs[i], std::move(w));
            changed = true;
        } else if (weight >= it->second.weight) {  // :188
            if (it->second.weight != weight || !(it->second.value == w.value)) changed = true;
            it->second = std::move(w);
        }
    }
    return changed;
}

// cache.rs:239-325
bool Cache::remove(const PeerIp &ip, uint32_t domain, const ScopeKey &scope, uint8_t weight, const ngz_enrich_operation &op,
                   bool all) {
    if (!all && !op.n_ies) return false;  // :242-249
    auto pit = peers_.find(ip);
    if (pit == peers_.end()) return false;
    PeerMetadata &pm = pit->second;
    ScopeMap *target = &pm.global;
    if (domain != 0) {
        auto dit = pm.domain_scoped.find(domain);
        if (dit == pm.domain_scoped.end()) return false;
        target = &dit->second;
    }
    auto sit = target->find(scope);
    if (sit == target->end()) return false;
    Metadata &md = sit->second;
    bool changed = false;
    for (auto it = md.begin(); it != md.end();) {
        bool listed = all;
        for (uint32_t i = 0; !listed && i < op.n_ies; ++i)
            listed = op.ies[i].pen == it->first.pen && op.ies[i].ie_id == it->first.ie;
        if (it->second.weight <= weight && listed) {  // :279-280
            it = md.erase(it);
            changed = true;
        } else {
            ++it;
        }
    }
    if (md.empty()) {  // :292-311
        target->erase(sit);
        if (domain != 0 && target->empty()) pm.domain_scoped.erase(domain);
        if (pm.global.empty() && pm.domain_scoped.empty()) peers_.erase(pit);
    }
    return changed;
}

std::vector<Resolved> Cache::lookup(const PeerIp &ip, uint32_t obs_domain_id, const ngz_enrich_field *record,
                                    uint32_t n_record) const {
    std::vector<Resolved> out;
    const PeerMetadata *pm = peer(ip);
    if (!pm) return out;
    const std::vector<FieldRef> refs = index_fields(record, n_record);
    std::map<FieldRef, uint32_t> by_ref;
    for (uint32_t i = 0; i < n_record; ++i) by_ref[refs[i]] = i;
    std::map<FieldRef, const Weighted *> best;
    auto visit = [&](const ScopeMap &m) {
        for (const auto &kv : m) {
            bool match = true;  // IndexedScopeFields::matches (:345-351)
            for (const ScopeField &sf : kv.first) {
                auto it = by_ref.find(sf.ref);
                if (it == by_ref.end()) { match = false; break; }
                const ngz_enrich_field &rf = record[it->second];
                if (rf.kind != sf.value.kind || rf.len != sf.value.bytes.size() ||
                    (rf.len && memcmp(rf.value, sf.value.bytes.data(), rf.len))) {
                    match = false;
                    break;
                }
            }
            if (!match) continue;
            for (const auto &fw : kv.second) {  // merge_fields (:500-528)
                auto b = best.find(fw.first);
                if (b == best.end()) best[fw.first] = &fw.second;
                else if (fw.second.weight >= b->second->weight) b->second = &fw.second;
            }
        }
    };
    visit(pm->global);
    auto dit = pm->domain_scoped.find(obs_domain_id);
    if (dit != pm->domain_scoped.end()) visit(dit->second);
    for (const auto &b : best) out.push_back(Resolved{b.first, b.second});
    return out;
}

}  // namespace ngze
