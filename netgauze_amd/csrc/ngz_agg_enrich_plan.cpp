// The plan of the aggregation over enriched records (ngz_agg_enrich_plan.h).  The record the
// aggregation sees is the record's own non-scope fields, then the cache fields resolved for it in
// ascending (PEN, IE id, cache index), then dataCollectionManifestName(writer_id)
// (enrichment/actor.rs:141-153, :176-187); FieldRef::map_fields (flow/types.rs:82-100) numbers the
// occurrences of an IE over that whole list, so an index past the template's own occurrences counts
// the added fields PRESENT in the row, whatever their cache index.
#include "ngz_agg_enrich_plan.h"

#include <cstring>

namespace ngza {

bool slot_dropped(const ngz_agg_slot_field *fields, uint32_t n_fields) {
    for (uint32_t i = 0; i < n_fields; ++i)
        if (fields[i].is_scope) return true;
    return false;
}

int resolve_field(const ngz_agg_slot_field *fields, uint32_t n_fields, const ngz_agg_ref *cols, uint32_t n_cols,
                  uint32_t pen, uint16_t ie, uint16_t index, ngz_agg_enrich_resolution *out) {
    memset(out, 0, sizeof *out);
    out->kind = NGZ_AGG_RES_NONE;
    if (n_cols > NGZ_AGG_ENRICH_MAX_COLUMNS) return NGZ_E_LIMIT;
    if (slot_dropped(fields, n_fields)) {
        out->dropped = 1;
        return NGZ_OK;
    }
    uint32_t own = 0;  // the template's occurrences of the IE
    for (uint32_t i = 0; i < n_fields; ++i) {
        if (fields[i].pen != pen || fields[i].ie_id != ie) continue;
        if (own == index) {
            out->kind = NGZ_AGG_RES_OWN;
            out->own_field = i;
            return NGZ_OK;
        }
        ++own;
    }
    const uint32_t ordinal = (uint32_t)index - own;
    uint32_t n = 0;
    for (uint32_t c = 0; c < n_cols; ++c)
        if (cols[c].pen == pen && cols[c].ie_id == ie) out->candidates[n++] = (uint8_t)c;
    const bool writer = pen == WRITER_PEN && ie == WRITER_IE;
    // a row has at most n of them: ordinals past that (past n + 1 with the writer id) never exist
    if (ordinal >= n + (writer ? 1u : 0u)) {
        memset(out->candidates, 0, sizeof out->candidates);
        return NGZ_OK;
    }
    if (n == 0) {  // the writer id alone
        out->kind = NGZ_AGG_RES_WRITER;
        return NGZ_OK;
    }
    out->kind = NGZ_AGG_RES_ADDED;
    out->n_candidates = (uint8_t)n;
    out->ordinal = (uint8_t)ordinal;
    out->writer_after = writer ? 1 : 0;
    return NGZ_OK;
}

}  // namespace ngza

extern "C" int ngz_agg_enrich_field_plan(const ngz_agg_slot_field *fields, uint32_t n_fields, const ngz_agg_ref *cols,
                                         uint32_t n_cols, uint32_t pen, uint16_t ie_id, uint16_t index,
                                         ngz_agg_enrich_resolution *out) {
    if (!out || (n_fields && !fields) || (n_cols && !cols)) return NGZ_E_INVALID;
    return ngza::resolve_field(fields, n_fields, cols, n_cols, pen, ie_id, index, out);
}
