/*
 * netgauze_amd — the flow-options input on the device: options data records of a decoded batch
 * turned into enrichment operations, the stage of the reference collector that feeds the
 * enrichment cache from the exporters themselves,
 *
 *   decode -> FlowOptionsActor -> EnrichmentOperation::Upsert -> EnrichmentActor's cache
 *             crates/collector/src/inputs/flow_options/{actor,normalize,handlers}.rs
 *
 *   ngz_options               ≙ one FlowOptionsActor with its FlowEnrichmentOptionsHandler(weight)
 *                               (actor.rs:217-326, handlers.rs:40-51).
 *   ngz_options_template_plan ≙ everything of OptionsDataRecord::try_from, classify and
 *                               into_normalized_records (normalize.rs:56-496) that depends on the
 *                               template alone, over IndexedDataRecord / FieldRefLookup
 *                               (flow/types.rs:138-234).
 *   ngz_options_harvest       ≙ the actor's loop over the FlowInfos of a batch (actor.rs:217-326)
 *                               with handle_option_record (handlers.rs:53-95).
 *   ngz_options_feed          ≙ send_enrichment_operations into EnrichmentCache::apply_enrichment
 *                               (ngz_enrich_op).
 *
 * Input (actor.rs:217-246, 275-288).  The batch last decoded on a context.  Only records of
 * messages with status NGZ_DG_OK count (the reference only ever sees a parsed FlowInfo), and of
 * those only records of slots whose template has scope fields (ngz_field_info.is_scope).  A
 * record's observation domain is its message's (ngz_dgram_hdr.domain: IPFIX observation domain id,
 * NetFlow v9 source id, actor.rs:221); the peer is the caller's, as in ngz_enrich_apply.
 *
 * NetFlow v9 scope conversion (normalize.rs:91-141; the raw scope code is ngz_field_info.ie_id,
 * the value a NGZ_K_SCOPE32 cell that becomes a canonical u32):
 *   System (1)                    dropped (:102-105)
 *   Interface (2)                 ingressInterface(v), egressInterface(v), in that order (:106-115)
 *   LineCard (3)                  lineCardId(v) (:116-118)
 *   Cache (4), Template (5), any  a conversion error, counted, no operation (:119-133)
 *   other code
 *
 * Classification (normalize.rs:156-169), in this order: sampling (:172-189: samplingInterval,
 * samplerRandomInterval, samplingProbability, or both of samplingPacketInterval/-Space,
 * samplingTimeInterval/-Space, samplingSize/-Population), interface (:218-226: an ingress or egress
 * interface with interfaceName or interfaceDescription), VRF (:347-354: ingressVRFID or egressVRFID
 * with VRFname or mplsVpnRouteDistinguisher), else unclassified.  contains_ie looks in the scope,
 * then in the non-scope fields (types.rs:219-221); get_by_ie prefers occurrence index 0, scope
 * before non-scope (types.rs:164-174, 229-233).
 * Normalization:
 *   - sampling, unclassified (:192-215, 463-483): paddingOctets dropped everywhere,
 *     exportingProcessId dropped from the scope; one record.
 *   - interface, VRF (:283-344, 407-460): split into an ingress and an egress record.  The id
 *     (get_by_ie over scope then fields) is the first scope field, the remaining scope fields minus
 *     the ingress/egress ids, paddingOctets and exportingProcessId follow (:291-304, 415-428).  The
 *     name and description / VRFname and route distinguisher come from the NON-scope fields only
 *     (:288-289, 412-413) and are re-tagged as NetGauze IEs (PEN 3746: 8/9 ingress/egress-
 *     InterfaceName, 10/11 -InterfaceDescription, 12/13 -VRFname, 14/15 -MplsVpnRouteDistinguisher;
 *     :230-273, 357-400).  With both directions present their ids must be equal, else
 *     UnsupportedInterfaceType / UnsupportedVrfType (:307-335, 431-451): the one test that depends
 *     on the record, made on the device.  A split that yields no field is MissingRequiredFields
 *     (:337-341, 453-457).
 *   - every normalized record becomes one Upsert {peer, Scope(obs_domain_id, scope fields), weight,
 *     fields} (handlers.rs:80-95); upserts without fields are dropped (handlers.rs:71-74,
 *     enrichment/mod.rs:118-120).
 *
 * Order.  Operations come in stream order: datagram, then set position in the datagram, then record
 * position in the set, the ingress record before the egress record (actor.rs:234-272,
 * normalize.rs:313-318); later upserts win ties in the cache, so the order is part of the contract.
 * Scope and field order inside an operation is template order, occurrence indices counted in that
 * order.  The reference collects both from an FxHashMap (types.rs:183-185, handlers.rs:88-93), whose
 * order is unspecified, and re-indexes in that order (IndexedDataRecord::new): PARITY UNPINNED
 * where a scope (or the fields) repeats an IE, and for the order of fields inside one operation.
 *
 * Counters (FlowOptionsActorStats, actor.rs:230, 248, 256, 263, 297): received_flows (NGZ_DG_OK
 * messages of the batch), processed_options_records, operations_generated, normalization_errors,
 * netflow_v9_conversion_errors; and ops_refused (ngz_options_feed).
 *
 * Device path (ngz_options.hip).  No kernel and no column copy for a batch whose options slots
 * hold no row.  Otherwise: one set pass over the set table (liveness, and the set a row belongs
 * to, which is its stream order and its domain); one row pass per options slot with a non-error
 * plan, the plan by value (the id test, the byte size of the row's packed operations: a variable-
 * length field's size is the length in its {offset, len} cell, a fixed NGZ_K_STR is NUL-truncated);
 * an exclusive scan of the sizes (hipcub); one pack pass per such slot, which copies the values out
 * of the columns and variable-length bytes out of the batch input on the device.  The host reads
 * the counters and the scanned total, then the packed buffer, merges the slots' streams by stream
 * order and materialises ngz_enrich_operations.  Work scales with the set table, the options slots
 * and their rows, never with the batch's data records; nothing is written into the context's
 * arena.
 *
 * Limits (NGZ_E_LIMIT): NGZ_OPTIONS_MAX_REFS scope fields or fields per operation.
 *
 * Out of scope: the actor's channels, back-off and logs (actor.rs:90-210, 340-420); the file and
 * Kafka inputs (inputs/files, inputs/kafka); the serde JSON of an operation.
 *
 * Return codes as flow_decode.h.  A harvester is not thread-safe.
 */
#ifndef NGZ_FLOW_OPTIONS_H
#define NGZ_FLOW_OPTIONS_H

#include "ngz/flow_enrich.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_OPTIONS_ABI_VERSION 1
#define NGZ_OPTIONS_MAX_REFS 24 /* scope fields, or fields, of one operation */

typedef struct ngz_options ngz_options;

typedef struct {                       /* per call or running total */
    uint64_t received_flows;           /* NGZ_DG_OK messages of the batch */
    uint64_t processed_options_records;
    uint64_t operations_generated;
    uint64_t normalization_errors;
    uint64_t netflow_v9_conversion_errors;
    uint64_t ops_refused;              /* operations the enricher refused with NGZ_E_LIMIT (feed) */
} ngz_options_stats;

/* class of a template's records (OptionsDataRecord) */
#define NGZ_OPTIONS_NONE 0          /* no scope fields: not an options template */
#define NGZ_OPTIONS_SAMPLING 1
#define NGZ_OPTIONS_INTERFACE 2
#define NGZ_OPTIONS_VRF 3
#define NGZ_OPTIONS_UNCLASSIFIED 4
/* template-level outcome */
#define NGZ_OPTIONS_OUT_OPS 0         /* n_ops operations per record (0: every upsert had no fields) */
#define NGZ_OPTIONS_OUT_NOT_OPTIONS 1 /* records are not options data records: nothing counted */
#define NGZ_OPTIONS_OUT_CONVERSION 2  /* UnsupportedNetFlowV9ScopeFieldType: a conversion error per record */
#define NGZ_OPTIONS_OUT_MISSING 3     /* MissingRequiredFields (or Unsupported*Type where the ids differ):
                                         a normalization error per record */

typedef struct {
    uint32_t pen;
    uint16_t ie_id;
    uint16_t index;  /* occurrence index among the operation's scope fields / fields */
} ngz_options_ref;

typedef struct {
    uint8_t klass;     /* NGZ_OPTIONS_* class */
    uint8_t outcome;   /* NGZ_OPTIONS_OUT_* */
    uint8_t n_ops;     /* operations per record: 0, 1 or 2 (ingress, then egress) */
    uint8_t id_equal;  /* the record's two ids (id_src) must be equal, else a normalization error */
    uint16_t id_src[2];                        /* template field index (scope first) of the ingress / egress id */
    uint8_t n_scope[2], n_fields[2];           /* per operation */
    ngz_options_ref scope[2][NGZ_OPTIONS_MAX_REFS];
    ngz_options_ref fields[2][NGZ_OPTIONS_MAX_REFS];
    uint16_t scope_src[2][NGZ_OPTIONS_MAX_REFS];   /* template field index each value is read from */
    uint16_t fields_src[2][NGZ_OPTIONS_MAX_REFS];
} ngz_options_plan;

int ngz_options_abi_version(void);

/* One FlowOptionsActor for contexts on `device`; `weight` is every upsert's.  Makes no HIP call:
 * the device is first touched by a harvest that has options rows. */
int ngz_options_create(int device, uint8_t weight, ngz_options **out);
void ngz_options_destroy(ngz_options *o);
const char *ngz_options_last_error(ngz_options *o);

/* No device: the plan of one IPFIX (proto 10) / NetFlow v9 (proto 9) template record
 * (proto | NGZ_OPTIONS_OPTIONS: an options template record; layouts as ngz_renorm_template_plan).
 * NGZ_E_INVALID: a record that does not parse; NGZ_E_LIMIT past NGZ_OPTIONS_MAX_REFS. */
#define NGZ_OPTIONS_OPTIONS 0x100
int ngz_options_template_plan(const uint8_t *tmpl, size_t len, int proto, ngz_options_plan *out);

/* The stage over the batch last decoded on ctx (`out` is that decode's result) for the exporter
 * `peer`.  Synchronous.  Reads the decoded columns, the set table, the datagram headers and the
 * batch input; writes nothing into the context's arena.  The operations live in the harvester
 * until its next harvest.  NGZ_E_INVALID: a decode pending on ctx (ngz_decode_batch_submit), ctx on
 * another device, `out` not the context's last decode. */
int ngz_options_harvest(ngz_options *o, ngz_ctx *ctx, const ngz_batch_out *out, const ngz_enrich_peer *peer,
                        ngz_options_stats *batch_stats /* may be NULL */, void *hip_stream);

/* The harvested operations, in order.  The scope / fields / value pointers lead into host memory
 * the harvester keeps until its next harvest; values are in the canonical column encodings, so an
 * operation goes to ngz_enrich_op unchanged. */
uint64_t ngz_options_op_count(ngz_options *o);
int ngz_options_op(ngz_options *o, uint64_t i, ngz_enrich_operation *op);

/* ngz_enrich_op for each harvested operation, in order.  One the enricher refuses with NGZ_E_LIMIT
 * (more than NGZ_ENRICH_MAX_SCOPE_FIELDS scope fields, a string or octet scope field such as a
 * VRFname scope) is counted in ops_refused and skipped; any other error stops and is returned.
 * *n_applied (may be NULL): the operations the enricher took. */
int ngz_options_feed(ngz_options *o, ngz_enrich *enricher, uint64_t *n_applied);

int ngz_options_totals(ngz_options *o, ngz_options_stats *totals, int reset);
/* Device milliseconds of the last harvest's kernels (HIP events round them; 0 without kernels). */
int ngz_options_last_timing(ngz_options *o, float *harvest_ms);
/* Kernels the last harvest launched (the scan counts as one); 0 for a batch without options rows. */
int ngz_options_last_launches(ngz_options *o);

#ifdef __cplusplus
}
#endif
#endif
