// The per-template plan of the flow-options input (include/ngz/flow_options.h): everything of the
// reference's OptionsDataRecord conversion, classification and normalization
// (crates/collector/src/inputs/flow_options/normalize.rs:56-496) that the template alone decides.
// No HIP: builds with a plain C++17 compiler (tests/native/options_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ngz/flow_options.h"

namespace ngzo {

struct PlanField {  // one field specifier of a template, scope fields first
    uint32_t pen = 0;
    uint16_t ie = 0;  // NetFlow v9 scope fields: the raw scope code
    bool scope = false;
};

// The plan of a template's records; proto 10 or 9.  NGZ_OK, or NGZ_E_LIMIT past NGZ_OPTIONS_MAX_REFS
int plan_fields(const std::vector<PlanField> &fields, int proto, ngz_options_plan *out);

}  // namespace ngzo
