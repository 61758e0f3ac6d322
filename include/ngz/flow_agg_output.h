/*
 * netgauze_amd — Avro datums of aggregated flow groups, encoded on the device: what the reference
 * collector's Kafka Avro publisher sends.  It subscribes to the aggregation actor
 * (crates/collector/src/lib.rs:139-181), so FlowOutputConfig::get_avro_values (flow/config.rs:189-215)
 * only ever sees the one-record FlowInfo AggFlowInfo::into_flowinfo_with_extra_fields builds per group
 * (aggregation/aggregator.rs:203-277) with the actor's extra fields (aggregation/actor.rs:222-240).
 * flow_output.h is the same config over the decoded records of a batch; this header is that config
 * over the rows ngz_agg_flush / ngz_agg_emit hand out (flow_aggregate.h).
 *
 *   ngz_agg_output         ≙ one validated FlowOutputConfig (config.rs:56-69).
 *   ngz_agg_output_schema  ≙ get_avro_schema (:149-169, get_record_schema :454-522), byte for byte.
 *   ngz_agg_output_encode  ≙ get_avro_value_from_fields (:105-145) of each group's record.
 *
 * The group's record, in this order (aggregator.rs:219-242): the present key fields in config order
 * (key_present), the present aggregated fields (val_present), originalFlowsPresent, minExportSeconds,
 * maxExportSeconds, collectionTimeMilliseconds (the max), NetGauze windowStart and windowEnd (start +
 * the aggregator's window duration), originalExporterIPv4Address or originalExporterIPv6Address by the
 * peer's family, one NetGauze originalExporterTransportPort per peer port, one
 * originalObservationDomainId per domain, one NetGauze originalTemplateId per template id.  Set members
 * are ascending by value, as ngz_agg_flowinfo_json pins (the reference iterates HashSets: parity
 * unpinned).
 *
 * A FieldRef (IE, index) counts occurrences in that row's list (FieldRef::map_fields_into_fxhashmap,
 * config.rs:194-213): the same IE may be a key twice, or a key and an aggregated field, or a key and a
 * set member, so the occurrence a ref lands on depends on the row's presence bits.  Per encode the host
 * lists each ref's candidates in list order; the kernel takes the index-th present one.  An index past
 * the present ones is None: null, or the default.
 *
 * Config: exactly flow_output.h's accepted subset, with the same refusals and codes through the same
 * validation code, and one addition: TimestampMillisString on the four dateTime types
 * (validate_ie_compatibility :371-385, NGZ_OUTPUT_E_CONFIG on any other IE), the decimal text of
 * ts.timestamp() (:934-940): the whole seconds, floored, negative values included.  All four dateTime
 * types hold a DateTime<Utc> in their Field (ipfix-code-generator generator.rs:2736-2739), so the
 * conversion is the same for each and none is refused.  windowStart / windowEnd (dateTimeSeconds),
 * minExportSeconds / maxExportSeconds and collectionTimeMilliseconds leave no other way: Identity and
 * String on them stay NGZ_OUTPUT_E_UNSUPPORTED, as on every dateTime in flow_output.h (their RawValue is
 * the String fallback, whose text nothing pins); originalFlowsPresent, an unsigned64, takes both.
 * A selected key or aggregated field that no record has carried yet is None in every row.
 *
 * Values are read by their row storage (ngz_agg_key_info / ngz_agg_value_info): kkind 0 keys as the
 * decoded cell; kkind 3 keys and vclass 8 / 9 values as byte values of any length (the ones longer than
 * the 32 bytes a row holds are fetched through ngz_agg_row_bytes and uploaded with the rows: nothing is
 * truncated); vclass 0 / 1 integers (a u64 goes out `as i64`); 5 / 6 floats; 2 micro / nano dateTimes;
 * 3 / 7 fixed bytes and IPv6.  vclass 4 (sub-registry, TCP flags) is reachable through no accepted
 * transform: such a config is refused at create.  A selected field whose storage the encoding cannot
 * read is NGZ_E_LIMIT at encode (a column kind the decode never produces for the IE).
 *
 * Rows.  `rows` is what the LAST ngz_agg_flush / ngz_agg_emit of `agg` copied to the host: the set
 * dictionaries, the peers and the byte tails are that call's.  Rows that carry different take_ids, or
 * whose take_id is not the aggregator's last as far as the aggregator's ABI tells (ngz_agg_row_bytes:
 * layouts with a byte-valued key or value, as for ngz_agg_flowinfo_json), are NGZ_E_INVALID.  The encode
 * uploads the rows (n_rows x row_bytes): groups are few next to records.
 *
 * Output, in device memory the stage owns until its next encode: `bytes`, the datums back to back in
 * row order, NGZ_OUTPUT_GUARD bytes of 0xA5 after them, and `offsets[n_rows + 1]` (u64).
 *
 * Device path (ngz_agg_output.hip): a wave stages its consecutive rows (64 of up to 256 bytes, fewer of
 * longer ones) into LDS with coalesced 16-byte loads, each lane then reads its own row there; one size
 * launch (lengths stored four at a time), one exclusive scan, one pack launch (a wave encodes into an
 * LDS image of its output range and copies it out in 16-byte stores).  n_rows == 0 launches nothing.
 *
 * Limits (NGZ_E_LIMIT): those of flow_output.h, and NGZ_AGG_OUTPUT_MAX_SOURCES candidates over all
 * refs.  Return codes as flow_output.h.  A stage object is not thread-safe; the aggregator is only read.
 */
#ifndef NGZ_FLOW_AGG_OUTPUT_H
#define NGZ_FLOW_AGG_OUTPUT_H

#include "ngz/flow_aggregate.h"
#include "ngz/flow_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_AGG_OUTPUT_ABI_VERSION 1
#define NGZ_AGG_OUTPUT_MAX_SOURCES 256 /* candidates of all refs of one config in one aggregator's list */

typedef struct ngz_agg_output ngz_agg_output;

typedef struct {        /* of the last encode */
    uint64_t rows;        /* datums written */
    uint64_t bytes;       /* bytes of all datums */
    uint64_t tail_bytes;  /* bytes of the byte values longer than a row holds, uploaded with the rows */
} ngz_agg_output_stats;

int ngz_agg_output_abi_version(void);

/* One FlowOutputConfig of n fields for `device`, from the same array as ngz_output_create.  Makes no HIP
 * call.  On a refused config the reason, naming the field, goes to err[0, err_cap). */
int ngz_agg_output_create(int device, const ngz_output_field *fields, uint32_t n, ngz_agg_output **out, char *err, size_t err_cap);
void ngz_agg_output_destroy(ngz_agg_output *o);
const char *ngz_agg_output_last_error(ngz_agg_output *o);

/* As ngz_output_schema. */
int64_t ngz_agg_output_schema(ngz_agg_output *o, char *buf, size_t cap);

/* The datums of n_rows rows of the last flush / emit of `agg` (row_bytes each, ngz_agg_layout).
 * Synchronous; hip_stream NULL: the device's default stream. */
int ngz_agg_output_encode(ngz_agg_output *o, ngz_agg *agg, const void *rows, uint64_t n_rows, ngz_agg_output_stats *stats /* may be NULL */,
                          void *hip_stream);

/* The last encode: device pointers valid until the next encode (NULL after an encode of no rows). */
int ngz_agg_output_result(ngz_agg_output *o, const uint8_t **bytes, const uint64_t **offsets, uint64_t *n_rows, uint64_t *n_bytes);

/* As ngz_output_to_host: the datums into bytes[0, bytes_cap) and the n_rows + 1 offsets into
 * offsets[0, offsets_cap) (either may be NULL); with room for them the guard bytes follow the datums. */
int ngz_agg_output_to_host(ngz_agg_output *o, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap);

/* Device milliseconds of the last encode: the upload (rows, tails, plan), the size pass with its scan,
 * the pack pass. */
int ngz_agg_output_last_timing(ngz_agg_output *o, float *upload_ms, float *size_ms, float *pack_ms);
/* Kernels the last encode launched (the scan counts as one); 0 for no rows. */
int ngz_agg_output_last_launches(ngz_agg_output *o);

#ifdef __cplusplus
}
#endif
#endif
