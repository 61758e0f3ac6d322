// The one walk over a template record's field specifiers that the per-template planners share
// (ngz_renorm_template_plan, ngz_enrich_template_plan, ngz_options_template_plan).  The record is
// untrusted wire data: every bound is checked here and nowhere else.  Host only, no HIP and no
// ngz_host.h: builds with a plain C++17 compiler (tests/native/template_record_check.cpp).
// The decoder's own template reader (ngz_host.cpp, with its error rendering) is not this one: it
// belongs to the decode sources, whose hash the committed profiles carry.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ngz/flow_decode.h"

namespace ngzt {

struct FieldSpec {  // one field specifier, scope fields first
    uint32_t pen;
    uint16_t ie;      // enterprise bit cleared; NetFlow v9 scope fields: the raw scope code
    uint16_t length;  // on the wire
    bool scope;
};

inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
inline uint32_t be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// Calls field(FieldSpec) for each specifier of one template record (proto 10 or 9; `options`: an
// options template record), in order, as it is read.  NGZ_OK, or NGZ_E_INVALID at the first
// specifier that does not fit; no byte at or past `len` is read.
//   template:       id, field count                        (ipfix.rs:384-413, netflow.rs:324-353)
//   IPFIX options:  id, field count (scope included), scope field count
//   NFv9 options:   id, scope bytes, option bytes; a specifier that begins before their end is read
//                   whole where the record still holds it
template <class F>
int walk_template_record(const uint8_t *tmpl, size_t len, int proto, bool options, F &&field) {
    uint32_t n_fields = 0, n_scope = 0, seen = 0;
    size_t pos, scope_end = 0, end = len;
    if (!options) {
        if (len < 4) return NGZ_E_INVALID;
        n_fields = be16(tmpl + 2);
        pos = 4;
    } else {
        if (len < 6) return NGZ_E_INVALID;
        pos = 6;
        if (proto == 10) {
            n_fields = be16(tmpl + 2);
            n_scope = be16(tmpl + 4);
            if (n_scope > n_fields) return NGZ_E_INVALID;
        } else {
            scope_end = pos + be16(tmpl + 2);
            end = scope_end + be16(tmpl + 4);
            if (end > len) return NGZ_E_INVALID;
        }
    }
    const bool by_bytes = options && proto == 9;
    while (by_bytes ? pos < end : seen < n_fields) {
        if (pos + 4 > len) return NGZ_E_INVALID;
        FieldSpec f;
        uint32_t code = be16(tmpl + pos);
        f.length = (uint16_t)be16(tmpl + pos + 2);
        f.scope = by_bytes ? pos < scope_end : seen < n_scope;
        f.pen = 0;
        pos += 4;
        if (!(by_bytes && f.scope) && (code & 0x8000)) {  // NetFlow v9 scope codes carry no enterprise bit
            if (pos + 4 > len) return NGZ_E_INVALID;
            f.pen = be32(tmpl + pos);
            pos += 4;
            code &= 0x7FFF;
        }
        f.ie = (uint16_t)code;
        if (++seen > 0x7FFF) return NGZ_E_INVALID;
        field(f);
    }
    return NGZ_OK;
}

}  // namespace ngzt
