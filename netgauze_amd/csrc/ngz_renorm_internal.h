// Internals shared by ngz_renorm.hip and ngz_json.cpp.  Not part of the C ABI.
#pragma once
#include <string>
#include <vector>

#include "ngz_host.h"

namespace ngzh {
// json_render's renormalized mode (flow_renormalize.h ngz_renorm_batch_json): the flag bytes of
// each slot of the batch in host memory (null: a slot without records)
struct EnrichJsonCol {  // one added column of a slot, in host memory
    uint32_t pen;
    uint16_t ie;
    uint8_t kind, is_string;
    uint16_t width;
    const uint8_t *data;
};
struct EnrichJsonSlot {
    std::vector<EnrichJsonCol> cols;
    const uint32_t *mask = nullptr;  // host, one word per row (null: a slot without records)
};
struct RenormJson {
    std::vector<const uint8_t *> slot_flags;  // null entries: no flags (no renormalizer)
    // the enriched view (flow_enrich.h ngz_enrich_batch_json): per slot the added columns, the value
    // arena their descriptors point into, and the writer id field appended last; empty: none
    std::vector<EnrichJsonSlot> enrich;
    const uint8_t *arena = nullptr;
    std::string writer_field;
};
// one appended Field of an added column cell (ngz_json.cpp)
void json_put_added(std::string &o, const EnrichJsonCol &c, const uint8_t *cell, const uint8_t *arena);
// json_render with mode == null; otherwise the reference's renormalize() output shape
// (renormalization/logic.rs:381-524): template sets and records with scope fields removed,
// isRenormalized(true) appended to flagged records
int json_render_mode(ngz_ctx *ctx, const JsonView &v, uint32_t d, std::string &out, uint32_t *consumed,
                     const RenormJson *mode);
}  // namespace ngzh
struct ngz_renorm;
namespace ngzh {
// The flag bytes of the batch `r` last applied when that is ctx's current batch: host copy into
// `store`, per-slot pointers into `slot_flags`.  NGZ_OK, or NGZ_E_* (ngz_renorm.hip)
int renorm_flags_host(ngz_renorm *r, ngz_ctx *ctx, std::vector<uint8_t> &store, std::vector<const uint8_t *> &slot_flags);
}  // namespace ngzh
