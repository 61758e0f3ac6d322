// The resolve pass of ngz_agg_push_enriched (ngz_agg_enrich.hip): per row of a slot, which key
// and aggregated fields are Some once the enrichment's added columns and the writer id count as
// fields of the record.  Not part of the C ABI.
#pragma once
#include <cstdint>

#include "ngz/flow_aggregate.h"

namespace ngza {

constexpr uint32_t RS_MAX_SEL = NGZ_AGG_MAX_KEYS + NGZ_AGG_MAX_VALUES;
constexpr uint32_t CELL_WRITER = 1;  // word 3 of a resolved variable-length cell: the bytes are the writer id's

struct ResolveSel {       // one selected field that resolves past the template's own columns
    uint32_t cand;        // bits of the enrichment mask: the added columns of the field's IE
    uint8_t ordinal;      // the wanted rank among those present in a row (ascending column = ascending bit)
    uint8_t writer_after; // dataCollectionManifestName: the writer id when exactly `ordinal` are present
    uint8_t bit;          // key k / value v
    uint8_t is_value;
    uint32_t width;       // resolved: bytes per cell (16: a variable-length cell)
    uint32_t wid_len;     // length of the writer id
    uint8_t *resolved;    // null: one candidate column, read in place
};

struct ResolvePlan {
    const uint32_t *mask;  // the enrichment's presence word per row, padded to a quad
    uint32_t n_rows, n_sel;
    uint32_t own_keys, own_vals;  // fields on the template's own columns: present in every row
    uint32_t *kpres, *vpres;      // out: one word per row each
    const uint8_t *col[NGZ_AGG_ENRICH_MAX_COLUMNS];  // the slot's added columns
    ResolveSel sel[RS_MAX_SEL];
};

// One launch of the resolve kernel on `stream` (a hipStream_t); 0 or the hipError_t
int resolve_launch(const ResolvePlan &p, void *stream);

}  // namespace ngza
