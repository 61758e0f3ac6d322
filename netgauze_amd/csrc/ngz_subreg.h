// The sub-registry tables of ngz_json.cpp (subreg_table.inc), for the unit that renders them on the
// device (ngz_agg_json.hip).  Beside ngzh::subreg_kind; kept out of ngz_host.h, which the decode and
// aggregation units are built from.
#pragma once
#include <cstdint>
#include <vector>

namespace ngzh {

struct SubregName {
    uint32_t value;
    const char *name;
};
// The variants of the IE's sub-registry enum ascending by value; for a nested one (forwardingStatus)
// every group's reasons, and `groups`: the name of the group of the values 64 g .. 64 g + 63.
// Returns subreg_kind: 0 none, 1 flat, 2 nested.
int subreg_names(uint32_t pen, uint16_t id, std::vector<SubregName> *values, std::vector<const char *> *groups);

}  // namespace ngzh
