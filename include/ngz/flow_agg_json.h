/*
 * netgauze_amd — serde JSON of aggregated flow groups, rendered on the device: what the reference
 * collector's Kafka JSON publisher sends.  FlowKafkaJson subscribes to the aggregation actor
 * (crates/collector/src/lib.rs:237-281) and sends serde_json of each FlowInfo (serialize_flow :963-971,
 * publishers/kafka_json.rs:201-229): the one-record FlowInfo AggFlowInfo::into_flowinfo_with_extra_fields
 * builds per group (aggregation/aggregator.rs:203-277) with the actor's extra fields (actor.rs:222-240).
 * flow_agg_output.h is the Avro publisher over the same rows; this header closes the publisher layer.
 *
 * Specification: line g is byte for byte what ngz_agg_flowinfo_json(agg, rows, n, shard_id, seq0,
 * export_time_ms, ...) (flow_aggregate.h) hands its callback for row g.  That host function stays; it is
 * what the tests compare against.
 *
 * A line: the IPFIX or NetFlow v9 head by the row's flow type (the export time is the call's, the
 * sequence number (u32)(seq0 + g), NetFlow v9 carries the row's max_sys_up_time), then the fields: the
 * present key fields in config order, the present aggregated fields, originalFlowsPresent,
 * minExportSeconds, maxExportSeconds, collectionTimeMilliseconds, NetGauze windowStart and windowEnd, the
 * exporter address by the peer's family, one field per port, domain and template id of the row's set
 * bits ascending by value (template ids masked to 16 bits and sorted again, duplicates kept), and the
 * closing text.
 *
 * Rendered on the device: u64 decimals up to 2^64 - 1, signed integers, booleans, IPv4 and Ipv6Addr
 * Display text, byte lists (macAddress, fixed bytes, unsigned256, octetArray, list-typed and unknown IEs,
 * byte values of any length), strings with serde_json's escapes (fixed ones cut at the first NUL), the
 * three dateTime storages as chrono's RFC 3339 text (floored negative milliseconds, 0 / 3 / 6 / 9
 * fraction digits, nanos >= 10^9 as second 60, years outside 0..9999 signed), TCPHeaderFlags,
 * sub-registry enums flat and nested, and the four tag shapes (IANA, vendor, vendor-unknown, Unknown).
 *
 * Floats: serde_json's text for them is ryu's shortest round trip.  By default a key or aggregated field
 * whose IE is float32 or float64 makes the encode fail with NGZ_OUTPUT_E_UNSUPPORTED and a message naming
 * the IE, before any launch, and ngz_agg_flowinfo_json remains the way for such layouts.  With
 * NGZ_AGG_JSON_OPT_FLOATS 1 a float64 key or aggregated value (the aggregator's f64 value class: sums in
 * record order, Min / Max in its float order) is rendered on the device, null for NaN and the infinities;
 * float32 is still refused: no IE of the registry has that type, and its text would need the 32-bit variant
 * of the routine.  Nothing is approximated.
 *
 * Rows: as flow_agg_output.h.  `rows` is what the LAST ngz_agg_flush / ngz_agg_emit of `agg` copied to
 * the host.  Rows that carry different take_ids, or whose take_id is not the aggregator's last as far as
 * ngz_agg_row_bytes tells (layouts with a byte-valued key or value), are NGZ_E_INVALID.  Byte values
 * longer than the 32 bytes a row holds are fetched whole through ngz_agg_row_bytes and uploaded with the
 * rows: nothing is truncated.
 *
 * Output, in device memory the stage owns until its next encode: `bytes`, the lines back to back in row
 * order with no separator, NGZ_OUTPUT_GUARD bytes of 0xA5 after them, and `offsets[n_rows + 1]` (u64).
 *
 * Device path (ngz_agg_json.hip): per encode the host lists the group's fields as items (presence test,
 * loader, renderer, constant prefix and suffix text in a dword-padded pool) and uploads plan, rows, tails
 * and peers in one copy; three launches: a size pass (the renderers through a counting writer), one
 * exclusive scan, a pack pass (each lane renders its row into the wave's LDS image through a 64-bit
 * accumulator that stores aligned dwords, constant text a dword at a time; the image goes out in 16-byte
 * stores; a line longer than the image goes straight out).  n_rows == 0 launches nothing.
 *
 * Limits (NGZ_E_LIMIT): 2^31 rows, 16 GiB of long byte values, NGZ_AGG_JSON_MAX_NAMES sub-registry
 * variants over the fields in use, an integer storage that is not 1, 2, 4 or 8 bytes wide.  Return codes
 * as flow_output.h.  A stage object is not thread-safe; the aggregator is only read.
 */
#ifndef NGZ_FLOW_AGG_JSON_H
#define NGZ_FLOW_AGG_JSON_H

#include "ngz/flow_aggregate.h"
#include "ngz/flow_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_AGG_JSON_ABI_VERSION 1
#define NGZ_AGG_JSON_MAX_NAMES 2048 /* sub-registry variants of all fields of one aggregator */

/* A diagnostic option (tools/bench_agg_json.py); a host has no reason to set it.  How the pack pass runs,
 * never what it writes.  NGZ_AGG_JSON_OPT_WRITER 0 (default): the accumulating dword writer; 1: the plain
 * byte writer of the Avro stages.  Default as measured, profiles/agg_json/summary.txt. */
#define NGZ_AGG_JSON_OPT_WRITER 1
/* Unlike NGZ_AGG_JSON_OPT_WRITER this option changes what an encode accepts, never a byte of a line it
 * accepted before.  NGZ_AGG_JSON_OPT_FLOATS 0 (default): a float key or aggregated field is refused as
 * above.  1: a float64 one is rendered; float32 is still refused.  A layout without floats launches the same
 * kernels under both values. */
#define NGZ_AGG_JSON_OPT_FLOATS 2

typedef struct ngz_agg_json ngz_agg_json;

typedef struct {        /* of the last encode */
    uint64_t rows;        /* lines written */
    uint64_t bytes;       /* bytes of all lines */
    uint64_t tail_bytes;  /* bytes of the byte values longer than a row holds, uploaded with the rows */
} ngz_agg_json_stats;

int ngz_agg_json_abi_version(void);

/* A stage for `device`.  Makes no HIP call. */
int ngz_agg_json_create(int device, ngz_agg_json **out);
void ngz_agg_json_destroy(ngz_agg_json *j);
const char *ngz_agg_json_last_error(ngz_agg_json *j);
int ngz_agg_json_set_option(ngz_agg_json *j, int opt, int64_t value);

/* The lines of n_rows rows of the last flush / emit of `agg` (row_bytes each, ngz_agg_layout), with the
 * packet header of ngz_agg_flowinfo_json.  Synchronous; hip_stream NULL: the device's default stream. */
int ngz_agg_json_encode(ngz_agg_json *j, ngz_agg *agg, const void *rows, uint64_t n_rows, uint32_t shard_id, uint32_t seq0,
                        int64_t export_time_ms, ngz_agg_json_stats *stats /* may be NULL */, void *hip_stream);

/* The last encode: device pointers valid until the next encode (NULL after an encode of no rows). */
int ngz_agg_json_result(ngz_agg_json *j, const uint8_t **bytes, const uint64_t **offsets, uint64_t *n_rows, uint64_t *n_bytes);

/* The lines into bytes[0, bytes_cap) and the n_rows + 1 offsets into offsets[0, offsets_cap) (either may
 * be NULL); with room for them the guard bytes follow the lines. */
int ngz_agg_json_to_host(ngz_agg_json *j, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap);

/* Device milliseconds of the last encode: the upload (rows, tails, plan), the size pass with its scan,
 * the pack pass. */
int ngz_agg_json_last_timing(ngz_agg_json *j, float *upload_ms, float *size_ms, float *pack_ms);
/* Kernels the last encode launched (the scan counts as one); 0 for no rows. */
int ngz_agg_json_last_launches(ngz_agg_json *j);

#ifdef __cplusplus
}
#endif
#endif
