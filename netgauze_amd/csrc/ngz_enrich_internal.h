// What the renormalization unit reads of an enricher's last apply (ngz_enrich.hip).  Not part of
// the C ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "ngz/flow_enrich.h"

struct ngz_ctx;

namespace ngze {

struct SlotResult {
    std::vector<ngz_enrich_column> cols;  // the slot's added columns (device pointers)
    const uint32_t *mask = nullptr;       // device, one word per row
    uint32_t rows = 0;
    bool dropped = false;                 // the template has scope fields
};

// The per-slot results of the enricher's last apply when that was ctx's current batch, else null
const std::vector<SlotResult> *results_for(const ngz_enrich *e, const ngz_ctx *ctx);
int enrich_device(const ngz_enrich *e);

}  // namespace ngze
