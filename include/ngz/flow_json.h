/*
 * netgauze_amd — serde JSON of decoded messages, rendered on the device: the line of every datagram's
 * FlowInfo, what the reference's KafkaJson flow publisher and its HTTP publisher send (serialize_flow_req,
 * crates/collector/src/lib.rs:953-961) and what pcap-decoder prints.  flow_output.h is the Avro publisher
 * over the same decoded records; flow_agg_output.h and flow_agg_json.h are the two publishers over
 * aggregated groups.
 *
 * Specification: for every datagram d with how[d] == NGZ_FLOW_JSON_LINE, bytes[offsets[d], offsets[d+1])
 * is byte for byte what ngz_dgram_json(ctx, d) (flow_decode.h) returns.  That host function stays; it is
 * what the tests compare against.  Every other datagram has a zero-length line.
 *
 *   NGZ_FLOW_JSON_LINE  rendered.
 *   NGZ_FLOW_JSON_NONE  the datagram's status is not NGZ_DG_OK: no FlowInfo.  The text of an error stays
 *                       with ngz_dgram_error_json.
 *   NGZ_FLOW_JSON_HOST  an OK datagram the device leaves to ngz_dgram_json: it carries a template or
 *                       options-template set (their texts live on the host with the template state; the
 *                       host uploads the indices of such datagrams, which are rare), or a data set of a
 *                       template with a float field the device does not render: a float64 field while
 *                       NGZ_FLOW_JSON_OPT_FLOATS is 0, the default, and a float32 field always.  It costs
 *                       those datagrams only, never the batch.
 * Nothing is refused and nothing approximated.
 *
 * Floats: serde_json's text of a float is ryu's shortest round trip.  With NGZ_FLOW_JSON_OPT_FLOATS 1 a
 * float64 field (samplingProbability, absoluteError, relativeError, the confidence-interval bounds and
 * confidenceLevel: every float IE of the registry) is rendered on the device like any other field, null for
 * NaN and the infinities, and its datagrams are NGZ_FLOW_JSON_LINE.  float32 stays with the host: no IE of
 * the registry has that type, so no template can reach it, and its text would need the 32-bit variant of the
 * routine.  Template-set datagrams stay with the host under either value.
 *
 * Scope: the plain decoded FlowInfo only.  The renormalized and the enriched renderer modes
 * (ngz_renorm_batch_json, ngz_enrich_batch_json) and the line callback's `consumed` are not rendered here.
 *
 * A line: the IPFIX head (export_time as RFC 3339 text, sequence number, observation domain) or the
 * NetFlow v9 head (sys_up_time, unix_time, sequence number, source_id), then the data sets in stream
 * order, each with its template id and its records, each record its scope fields and fields in template
 * order.  Rendered: everything ngz_dgram_json renders (floats as above): unsigned and signed integers, booleans,
 * IPv4 and Ipv6Addr Display text, byte lists (macAddress, fixed bytes, unsigned256, octetArray, list-typed
 * and unknown IEs), strings with serde_json's escapes (fixed ones cut at the first NUL), the dateTime
 * storages as chrono's RFC 3339 text, TCPHeaderFlags, sub-registry enums flat and nested, the four tag
 * shapes (IANA, vendor, vendor-unknown, Unknown) and the NetFlow v9 scope fields.  Variable-length values
 * are read from the batch input through the column's {offset, length}: the input of the decode must
 * still be valid during the encode.
 *
 * Output, in device memory the stage owns until its next encode: `bytes`, the lines back to back in
 * datagram order with no separator, NGZ_OUTPUT_GUARD bytes of 0xA5 after them, `offsets[n_dgrams + 1]`
 * (u64) and `how[n_dgrams]` (u8).
 *
 * Device path (ngz_flow_json.hip): per encode the host lists every slot's fields as items
 * (column, renderer, tag text in a dword-padded pool) and uploads the plan in one copy.  A set pass cuts
 * the data sets into tiles of at most 64 consecutive records; a size pass renders each tile's records
 * through a counting writer; two walks and one scan turn the tile sizes into the datagram offsets and
 * back into every set's and tile's output offset; a glue pass writes heads, tails and commas; a pack pass
 * renders each tile into a wave's LDS image and copies it out in 16-byte stores.  The number of launches
 * does not depend on the number of templates.  A batch with no datagram launches nothing.
 *
 * Limits (NGZ_E_LIMIT): NGZ_FLOW_JSON_MAX_NAMES sub-registry variants over the fields in use, an integer
 * column that is not 1, 2, 4 or 8 bytes wide.  Return codes as flow_output.h.  A stage object is not
 * thread-safe; the context is only read.
 */
#ifndef NGZ_FLOW_JSON_H
#define NGZ_FLOW_JSON_H

#include "ngz/flow_decode.h"
#include "ngz/flow_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_FLOW_JSON_ABI_VERSION 1
#define NGZ_FLOW_JSON_MAX_NAMES 65536 /* sub-registry variants of all fields of one batch's templates */

#define NGZ_FLOW_JSON_NONE 0
#define NGZ_FLOW_JSON_LINE 1
#define NGZ_FLOW_JSON_HOST 2

typedef struct ngz_flow_json ngz_flow_json;

typedef struct {          /* of the last encode */
    uint64_t lines;         /* datagrams rendered (NGZ_FLOW_JSON_LINE) */
    uint64_t bytes;         /* bytes of all lines */
    uint64_t left_template; /* OK datagrams left to the host for their (options) template sets */
    uint64_t left_float;    /* OK datagrams left to the host for a float field, and for that alone */
    uint64_t not_ok;        /* datagrams whose status is not NGZ_DG_OK */
} ngz_flow_json_stats;

int ngz_flow_json_abi_version(void);

/* A stage for `device`.  Makes no HIP call. */
int ngz_flow_json_create(int device, ngz_flow_json **out);
void ngz_flow_json_destroy(ngz_flow_json *j);
const char *ngz_flow_json_last_error(ngz_flow_json *j);

/* NGZ_FLOW_JSON_OPT_FLOATS 0 (default): a data set of a template with a float64 field leaves its datagram
 * to the host (NGZ_FLOW_JSON_HOST, counted in left_float).  1: such a template is planned like any other and
 * its datagrams are rendered; left_float then counts float32 templates only.  The option changes which
 * datagrams are rendered, never a rendered byte; a batch without float fields launches the same kernels
 * under both values.  NGZ_E_INVALID: an unknown option or value. */
#define NGZ_FLOW_JSON_OPT_FLOATS 1
int ngz_flow_json_set_option(ngz_flow_json *j, int opt, int64_t value);

/* serde_json's text of the float64 with bit pattern `bits`, through the routine the device kernels run,
 * compiled for the host: so that it can be checked where there is no device.  Makes no HIP call.  Returns
 * the length (at most 24; no terminator is written), or NGZ_E_INVALID when buf is NULL or cap is smaller. */
int ngz_flow_json_f64_text(uint64_t bits, char *buf, size_t cap);

/* The stage over the batch last decoded on ctx (`out` is that decode's result).  Synchronous.  Reads the
 * decoded columns, the set table, the datagram headers and the batch input; writes nothing into the
 * context's arena.  NGZ_E_INVALID: a decode pending on ctx, ctx on another device, `out` not the
 * context's last decode, a variable-length cell outside the batch input. */
int ngz_flow_json_encode(ngz_flow_json *j, ngz_ctx *ctx, const ngz_batch_out *out, ngz_flow_json_stats *stats /* may be NULL */,
                         void *hip_stream);

/* The last encode: device pointers valid until the next encode (NULL after an encode of no datagram). */
int ngz_flow_json_result(ngz_flow_json *j, const uint8_t **bytes, const uint64_t **offsets, const uint8_t **how, uint64_t *n_dgrams,
                         uint64_t *n_bytes);

/* The lines into bytes[0, bytes_cap), the n_dgrams + 1 offsets into offsets[0, offsets_cap) and `how` into
 * how[0, how_cap) (each may be NULL); with room for them the guard bytes follow the lines. */
int ngz_flow_json_to_host(ngz_flow_json *j, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap, uint8_t *how,
                          uint64_t how_cap);

/* Device milliseconds of the last encode: the size pass (set pass, tile table and the counting
 * renderers), the offsets (the two sums and the scan), the glue and pack passes. */
int ngz_flow_json_last_timing(ngz_flow_json *j, float *size_ms, float *offsets_ms, float *pack_ms);
/* Kernels the last encode launched (a scan counts as one); 0 for no datagram. */
int ngz_flow_json_last_launches(ngz_flow_json *j);

#ifdef __cplusplus
}
#endif
#endif
