// Internals shared by ngz_renorm.hip and ngz_json.cpp.  Not part of the C ABI.
#pragma once
#include <string>
#include <vector>

#include "ngz_host.h"

namespace ngzh {
// json_render's renormalized mode (flow_renormalize.h ngz_renorm_batch_json): the flag bytes of
// each slot of the batch in host memory (null: a slot without records)
struct RenormJson {
    std::vector<const uint8_t *> slot_flags;
};
// json_render with mode == null; otherwise the reference's renormalize() output shape
// (renormalization/logic.rs:381-524): template sets and records with scope fields removed,
// isRenormalized(true) appended to flagged records
int json_render_mode(ngz_ctx *ctx, const JsonView &v, uint32_t d, std::string &out, uint32_t *consumed,
                     const RenormJson *mode);
}  // namespace ngzh
