// The per-slot plan of the aggregation over enriched records (include/ngz/flow_aggregate.h,
// ngz_agg_push_enriched): where one FieldRef of the aggregation config lands in the record the
// enrichment actor leaves (crates/collector/src/flow/enrichment/actor.rs:141-153, :176-187) under
// FieldRef::map_fields (crates/collector/src/flow/types.rs:82-100).
// No HIP: builds with a plain C++17 compiler (tests/native/agg_enrich_plan_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "ngz/flow_aggregate.h"

namespace ngza {

constexpr uint32_t WRITER_PEN = 3746;  // NetGauze dataCollectionManifestName
constexpr uint16_t WRITER_IE = 7;

// Whether a slot with these template fields is dropped (records with scope fields, actor.rs:178)
bool slot_dropped(const ngz_agg_slot_field *fields, uint32_t n_fields);

// The resolution of FieldRef (pen, ie, index) in a slot: fields in template order, cols the
// slot's added columns in ascending (PEN, IE id, index).  NGZ_OK, or NGZ_E_LIMIT past
// NGZ_AGG_ENRICH_MAX_COLUMNS added columns
int resolve_field(const ngz_agg_slot_field *fields, uint32_t n_fields, const ngz_agg_ref *cols, uint32_t n_cols,
                  uint32_t pen, uint16_t ie, uint16_t index, ngz_agg_enrich_resolution *out);

}  // namespace ngza
