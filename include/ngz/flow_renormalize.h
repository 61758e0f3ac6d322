/*
 * netgauze_amd — flow renormalization on the device: the stage of the reference collector's flow
 * pipeline between decode and aggregation,
 *
 *   decode -> (enrichment) -> RenormalizationActor -> AggregationActor -> publisher
 *             crates/collector/src/lib.rs:140-163
 *
 *   ngz_renorm              ≙ one RenormalizationActor shard
 *                             (crates/collector/src/flow/renormalization/actor.rs); serves any
 *                             number of contexts (exporter peers) on one device.
 *   ngz_renorm_apply        ≙ renormalize() applied to every FlowInfo of a decoded batch
 *                             (renormalization/logic.rs:381-524), in place in the batch's columns:
 *                             one streaming read-modify-write pass in HBM, so ngz_agg_push on the
 *                             same batch sums renormalized counts.
 *   ngz_renorm_stats        ≙ RenormalizationStats (actor.rs), plus records_dropped.
 *
 * Semantics (logic.rs:30-379), per data record of a message that decoded (NGZ_DG_OK):
 *   - a record with scope fields is filtered out (logic.rs:415, 484): it counts in records_dropped
 *     only, and its columns are left as decoded (ngz_renorm_batch_json omits it);
 *   - every other record counts in flows_processed (logic.rs:324);
 *   - the sampling parameters are the non-scope PEN-0 fields 34, 35, 49, 50, 304, 305, 306, 309,
 *     310, 311; the LAST occurrence of each in the record wins (logic.rs:327-341 overwrites);
 *   - the factor k, in f64 (calculate_renormalization_factor, logic.rs:107-261):
 *       1. IE 304 present: 1 -> (306 + 305) / 305, no factor if 305 == 0 (:30-48);
 *                          3 -> 310 / 309, no factor if 309 == 0 (:50-68);
 *                          4 -> 1 / 311, no factor unless 0 < p <= 1 (NaN: no factor, :70-88);
 *          a missing parameter, or any other value of 304 (Unassigned included), gives no factor;
 *       2. else IE 49 present: modes 1 | 2 with IE 50 -> k = IE 50 (:177-204);
 *       3. else IE 35 present: algorithms 1 | 2 with IE 34 -> k = IE 34 (:205-233);
 *       4. else inferred, in this order: 305 + 306, 309 + 310, 311, 50, 34 (:236-256); each counts
 *          sampling_algorithm_inferred;
 *     every "no factor" above counts ie_missing_or_invalid.  IE 50 or 34 equal to 0 gives
 *     k = 0.0: the counts become 0 and the record is flagged;
 *   - with a factor, EVERY occurrence of octetDeltaCount (1), packetDeltaCount (2),
 *     octetTotalCount (85), packetTotalCount (86) becomes `(count as f64 * k) as u64`
 *     (:346-370): u64 -> f64 rounds to nearest even, f64 -> u64 truncates toward zero and
 *     saturates at 0 and u64::MAX, NaN -> 0;
 *   - a record with a factor and at least one count field gets isRenormalized(true) (PEN 3746,
 *     id 16) appended (:371-374) and counts in flows_renormalized: bit 0 of its flag byte here.  A
 *     record with a factor but no count field is unchanged and unflagged; its other statistics
 *     still count.
 * Rows of messages whose status is not NGZ_DG_OK are left byte-identical and count in nothing
 * (they yield no FlowInfo).  Template and options-template sets carry no records here; the JSON
 * view drops them (logic.rs:434-449, 497-512).
 *
 * Out of scope:
 *   - the reference's warn! / trace! logs are not reproduced;
 *   - ngz_record_fields does not append the extra field: a host reads ngz_renorm_flags;
 *   - ngz_agg_push still explodes options records after an apply (the reference would have
 *     dropped them before aggregation);
 *   - an aggregation config that names isRenormalized sees None;
 *   - ngz_renorm_apply reads only sampling IEs carried in the record itself; the ones an enrichment
 *     resolved (flow_enrich.h) act through ngz_renorm_apply_enriched.
 *
 * Return codes as flow_decode.h (0 = ok, NGZ_E_*).  A renormalizer is not thread-safe.
 */
#ifndef NGZ_FLOW_RENORMALIZE_H
#define NGZ_FLOW_RENORMALIZE_H

#include "ngz/flow_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_RENORM_ABI_VERSION 1
#define NGZ_RENORM_MAX_COUNTS 64  /* count fields (IE 1, 2, 85, 86 occurrences) one template may carry */

typedef struct ngz_renorm ngz_renorm;

typedef struct {                      /* RenormalizationStats (actor.rs), per call or running total */
    uint64_t flows_processed;         /* every record with no scope fields, of NGZ_DG_OK messages */
    uint64_t flows_renormalized;      /* records that got isRenormalized */
    uint64_t ie_missing_or_invalid;
    uint64_t sampling_algorithm_inferred;
    uint64_t records_dropped;         /* records with scope fields (the reference filters them out) */
} ngz_renorm_stats;

int ngz_renorm_abi_version(void);
int ngz_renorm_create(int device, ngz_renorm **out);
void ngz_renorm_destroy(ngz_renorm *r);
const char *ngz_renorm_last_error(ngz_renorm *r);

/* renormalize() applied to every FlowInfo of the batch last decoded on ctx (`out` is that decode's
 * result), in place in its columns.  One kernel launch per template slot that carries a sampling
 * IE, on the context's stream (or hip_stream); synchronous: on return the columns, the flags and
 * *batch_stats are complete.  The context's cached host view is dropped, so ngz_dgram_json,
 * ngz_batch_json, ngz_record_fields and ngz_columns_to_host show the scaled counts.
 * NGZ_E_INVALID, with nothing changed: the same batch (ctx and its batch serial) applied twice, a
 * decode pending on ctx (ngz_decode_batch_submit), ctx on another device than the renormalizer.
 * NGZ_E_LIMIT: a template with more than NGZ_RENORM_MAX_COUNTS count fields.  A renormalizer
 * remembers the last batch of each context by the context's address: destroy it, or decode a new
 * batch, before a context created at a destroyed one's address is applied. */
int ngz_renorm_apply(ngz_renorm *r, ngz_ctx *ctx, const ngz_batch_out *out, ngz_renorm_stats *batch_stats /* may be NULL */,
                     void *hip_stream);
/* ngz_renorm_apply over enriched records: `e` must have applied this batch of ctx last
 * (ngz_enrich_apply; NGZ_E_INVALID otherwise).  For each sampling parameter a row's value is the
 * enrichment's added column of that IE where the row's presence bit is set (of several occurrence
 * indexes the highest present: appended fields come last and logic.rs:327-341 keeps the last),
 * otherwise the record's own last occurrence.  An added column takes part when it is in the IE's
 * canonical encoding (NGZ_K_UINT of the IE's width).  A slot with no sampling IE in its template
 * but one among its added columns launches.  Counts, flags, the five counters, the refusals and
 * the cached-view invalidation are ngz_renorm_apply's.  NGZ_E_LIMIT also for more than 16 added
 * sampling columns in one slot.  An addition to ABI version 1: no existing signature changed. */
struct ngz_enrich;
int ngz_renorm_apply_enriched(ngz_renorm *r, struct ngz_enrich *e, ngz_ctx *ctx, const ngz_batch_out *out,
                              ngz_renorm_stats *batch_stats /* may be NULL */, void *hip_stream);
int ngz_renorm_totals(ngz_renorm *r, ngz_renorm_stats *totals, int reset);

/* Per row of a slot of the batch last applied: bit 0 = isRenormalized(true) was appended.
 * Device pointer, n = the slot's n_records; valid until the next apply or the context's next decode. */
int ngz_renorm_flags(ngz_renorm *r, uint32_t slot, const uint8_t **dev_flags, uint32_t *n);

/* serde JSON of the renormalized FlowInfos of the batch last applied, which must still be ctx's
 * last decode (ngz_batch_json's contract and callback): template and options-template sets
 * removed, records with scope fields removed (a data set left empty stays "records":[]),
 * {"NetGauze":{"isRenormalized":true}} appended as the last field of each flagged record, headers
 * unchanged, error datagrams as ngz_batch_json renders them. */
int64_t ngz_renorm_batch_json(ngz_renorm *r, ngz_ctx *ctx, const uint8_t *host_bytes, ngz_json_line_fn fn, void *user);

/* Device milliseconds of the last apply's kernels (HIP events round them); 0 when it launched none. */
int ngz_renorm_last_timing(ngz_renorm *r, float *apply_ms);

/* Introspection, no device: the plan for one IPFIX (proto 10) / NetFlow v9 (proto 9) template
 * record (template id u16, field count u16, field specifiers: ipfix.rs:384-413, netflow.rs:324-353).
 * proto | NGZ_RENORM_OPTIONS: an options template record instead (IPFIX: id, field count, scope
 * field count, specifiers, ipfix.rs:276-327; NetFlow v9: id, scope bytes, option bytes,
 * specifiers, netflow.rs:265-310). */
#define NGZ_RENORM_OPTIONS 0x100
typedef struct {
    int16_t param_field[10];  /* template field index (scope first) the value of IE
                                 34,35,49,50,304,305,306,309,310,311 is taken from; -1 = absent */
    uint16_t n_counts;        /* occurrences of IE 1, 2, 85, 86 among the non-scope fields */
    uint16_t count_field[64];
    uint8_t dropped;          /* the template has scope fields: its records are dropped */
    uint8_t launches;         /* 0: no kernel is needed for this template */
} ngz_renorm_plan;
int ngz_renorm_template_plan(const uint8_t *tmpl, size_t len, int proto, ngz_renorm_plan *out);

#ifdef __cplusplus
}
#endif
#endif
