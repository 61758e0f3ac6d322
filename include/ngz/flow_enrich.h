/*
 * netgauze_amd — flow enrichment on the device: the stage of the reference collector's flow
 * pipeline between decode and renormalization,
 *
 *   decode -> FlowEnrichmentActor -> RenormalizationActor -> AggregationActor -> publisher
 *             crates/collector/src/lib.rs:140-163
 *
 *   ngz_enrich              ≙ one EnrichmentActor shard (crates/collector/src/flow/enrichment/
 *                             actor.rs) with its EnrichmentCache (enrichment/cache.rs:60-529);
 *                             serves any number of contexts (exporter peers) on one device.
 *   ngz_enrich_op           ≙ EnrichmentCache::apply_enrichment (cache.rs:96-120) of one
 *                             EnrichmentOperation (enrichment/mod.rs:48-215).
 *   ngz_enrich_lookup       ≙ EnrichmentCache::get_enrichment_fields for one record, on the host
 *                             (cache.rs:84-93, 437-528).
 *   ngz_enrich_apply        ≙ EnrichmentActor::enrich (actor.rs:122-271) over every FlowInfo of a
 *                             decoded batch: the fields the reference appends to each record land
 *                             in added columns beside the batch's own, with one presence mask per
 *                             row.  Nothing is written into the context's arena.
 *   ngz_enrich_stats        ≙ the actor's counters, per call and running.
 *
 * Cache (cache.rs:60-326).  peer IP -> { global scopes (obs_domain_id 0), scopes per observation
 * domain }; a scope is its fields in the order given, each tagged FieldRef(IE, occurrence index
 * among the scope's fields), and maps FieldRef(IE, occurrence index among the upserted fields) ->
 * (weight, value).
 *   - upsert: no fields is a no-op (:136-152); an incoming field replaces the one at its FieldRef
 *     when weight >= the current weight (:183-219);
 *   - delete / delete-all: an empty IE list is a no-op (:242-252); fields with weight <= the
 *     operation's are removed, delete only those whose IE is listed (:278-290); a scope, a domain
 *     map and a peer left empty are removed (:292-311).
 * Lookup (cache.rs:437-528).  The record's non-scope fields are indexed by FieldRef (occurrence
 * index per IE over the record's fields).  A scope matches when every scope field equals the
 * record's field at the same FieldRef (:345-351).  Global scopes are visited first, then the
 * scopes of the message's observation domain (IPFIX observation_domain_id, NetFlow v9 source_id),
 * each map in its order; a field of a later scope replaces an earlier one at the same FieldRef
 * when weight >= the current weight (:500-528): the higher weight wins, on equal weight the later
 * scope.
 * Scope visiting order inside one map: the Rust Ord of Box<[(FieldRef, Field)]> -- the empty scope
 * first, then lexicographic over (FieldRef, value) pairs.  The generated IE enum declares the
 * vendors' IEs before the IANA ones (ipfix-code-generator/src/generator.rs:1160-1164), so here a
 * FieldRef orders by (IANA last, PEN, IE id, index) and a value by its kind's order (unsigned,
 * signed, else bytewise); the order among vendors and the registry's declaration order inside one
 * package were not established (ascending PEN and IE id are assumed).  The two tie-breaks the
 * reference tests pin (cache/tests.rs:629-814: global before domain, no-scope-field before scoped)
 * hold exactly; between two scopes on DIFFERENT IEs that match one record, give one FieldRef and
 * have equal weight, the order rests on that assumption: parity unpinned for that case.
 * Apply (actor.rs:122-271).  Records with scope fields are dropped (counted, mask 0); every other
 * record of a message that decoded (NGZ_DG_OK) gets the resolved fields appended after its own and
 * NetGauze dataCollectionManifestName(writer_id) (PEN 3746, id 7) last.  The reference appends in
 * FxHashMap order (unspecified; its tests compare sets); here the order is ascending (PEN, IE id,
 * occurrence index), which is also the order of a slot's added columns.  Rows of messages that
 * did not decode have mask 0 and count in nothing.
 * Downstream: renormalize() reads the LAST occurrence of each sampling IE (logic.rs:327-341), so
 * an added sampling IE overrides the record's own: ngz_renorm_apply_enriched (flow_renormalize.h).
 *
 * Values are in the canonical column encodings, where byte equality is Field
 * equality.  Scope fields are restricted to the fixed-width kinds where that holds: NGZ_K_UINT of
 * an unsigned / sub-registry / IPv4 / dateTimeSeconds IE, NGZ_K_SINT, NGZ_K_BOOL, NGZ_K_TCPFLAGS,
 * NGZ_K_DTMS, NGZ_K_BYTES (IPv6, MAC), at most NGZ_ENRICH_MAX_KEY_BYTES bytes.  An operation whose
 * scope carries a float, string, octetArray, list or unknown IE, or a longer value, returns
 * NGZ_E_LIMIT and leaves the cache unchanged.  Added fields may be of any kind and length
 * (NGZ_K_STR: a string, NGZ_K_BYTES: octets).
 *
 * Limits (each a design condition, NGZ_E_LIMIT): NGZ_ENRICH_MAX_SCOPE_FIELDS scope fields per
 * scope (ngz_enrich_op), NGZ_ENRICH_MAX_SHAPES scope shapes and NGZ_ENRICH_MAX_COLUMNS added
 * columns per slot plan, NGZ_ENRICH_MAX_DOMAINS observation domains per peer (ngz_enrich_apply).
 *
 * Out of scope:
 *   - the file and Kafka inputs, the serde JSON of EnrichmentOperation: operations come through
 *     ngz_enrich_op (the flow-options input, inputs/flow_options/normalize.rs: options data records
 *     turned into operations, is include/ngz/flow_options.h and feeds ngz_enrich_op);
 *   - the debug! logs;
 *   - scope fields of float, string, octet, list or unknown kinds;
 *
 * The value arena interns every variable-length value an upload met and is released only by
 * ngz_enrich_destroy: its size is bounded by the distinct values ever upserted, not by the live
 * cache.  An enricher remembers a context by its address, with its device buffers, until
 * ngz_enrich_forget or ngz_enrich_destroy: call ngz_enrich_forget before destroying a context, or a
 * context created at the same address whose batch serial happens to match would be handed the
 * destroyed one's results.  A column whose values differ in kind or are fixed values longer than 16
 * bytes (NGZ_K_U256) is a NGZ_K_VLEN column; value_kind keeps the common kind, and
 * ngz_enrich_row_fields reports it.
 *
 * Return codes as flow_decode.h (0 = ok, NGZ_E_*).  An enricher is not thread-safe.
 */
#ifndef NGZ_FLOW_ENRICH_H
#define NGZ_FLOW_ENRICH_H

#include "ngz/flow_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_ENRICH_ABI_VERSION 1
#define NGZ_ENRICH_MAX_SCOPE_FIELDS 4  /* scope fields per scope */
#define NGZ_ENRICH_MAX_SHAPES 8        /* scope shapes (ordered FieldRef lists) one slot plan holds */
#define NGZ_ENRICH_MAX_COLUMNS 32      /* added columns per slot: the mask is a uint32_t */
#define NGZ_ENRICH_MAX_KEY_BYTES 16    /* bytes of one scope field's value */
#define NGZ_ENRICH_MAX_DOMAINS 253     /* observation domains of one peer (one byte per row) */

typedef struct ngz_enrich ngz_enrich;

typedef struct {       /* an exporter's IpAddr */
    uint8_t family;    /* 4 or 6 */
    uint8_t reserved[3];
    uint8_t addr[16];  /* IPv4 in the first 4 bytes, the rest 0 */
} ngz_enrich_peer;

typedef struct {           /* one Field: its IE and its value in the canonical column encoding */
    uint32_t pen;
    uint16_t ie_id;
    uint8_t kind;          /* NGZ_K_* of the encoding (never NGZ_K_VLEN / NGZ_K_FAIL / NGZ_K_SCOPE32) */
    uint8_t reserved;
    uint32_t len;          /* bytes at `value` */
    uint32_t reserved2;
    const uint8_t *value;
} ngz_enrich_field;

typedef struct {
    uint32_t pen;
    uint16_t ie_id;
    uint16_t reserved;
} ngz_enrich_ie;

#define NGZ_ENRICH_UPSERT 1
#define NGZ_ENRICH_DELETE 2
#define NGZ_ENRICH_DELETE_ALL 3
typedef struct {                     /* EnrichmentOperation (enrichment/mod.rs:48-215) */
    uint8_t kind;                    /* NGZ_ENRICH_UPSERT / _DELETE / _DELETE_ALL */
    uint8_t weight;
    uint8_t reserved[2];
    ngz_enrich_peer peer;
    uint32_t obs_domain_id;          /* 0: a global scope */
    uint32_t n_scope, n_fields, n_ies;
    const ngz_enrich_field *scope;   /* the scope's fields, in order */
    const ngz_enrich_field *fields;  /* upsert: the fields to add */
    const ngz_enrich_ie *ies;        /* delete: the IEs to remove */
} ngz_enrich_operation;

typedef struct {           /* one resolved field (ngz_enrich_lookup) */
    uint32_t pen;
    uint16_t ie_id;
    uint16_t index;        /* occurrence index of the FieldRef */
    uint8_t kind;
    uint8_t weight;
    uint16_t reserved;
    uint32_t len;
    const uint8_t *value;  /* in the cache: valid until the next ngz_enrich_op */
} ngz_enrich_resolved;

typedef struct {                 /* per call or running total */
    uint64_t records_processed;  /* records with no scope fields, of NGZ_DG_OK messages */
    uint64_t records_matched;    /* records that got at least one cache field */
    uint64_t fields_added;       /* cache fields added, the writer id not counted */
    uint64_t records_dropped;    /* records with scope fields */
} ngz_enrich_stats;

typedef struct {          /* one added column of a slot (ngz_enrich_slot_columns) */
    uint32_t pen;
    uint16_t ie_id;
    uint16_t index;       /* occurrence index of the FieldRef */
    uint8_t kind;         /* NGZ_K_*; NGZ_K_VLEN: {u64 offset into the value arena, u32 length, u32 0} */
    uint8_t is_string;    /* NGZ_K_VLEN: 1 a string, 0 octets */
    uint16_t width;       /* bytes per row */
    uint8_t value_kind;   /* the NGZ_K_* every value of the column was given with; 0: they differ (a
                             NGZ_K_VLEN column then reads as octets, whatever each value was) */
    uint8_t reserved[3];
    const uint8_t *data;  /* device, n rows; a cell whose mask bit is clear holds zero bytes */
} ngz_enrich_column;

int ngz_enrich_abi_version(void);

/* One EnrichmentActor shard for contexts on `device`; writer_id is the value of
 * dataCollectionManifestName appended to every record.  Makes no HIP call: the device is first
 * touched by ngz_enrich_apply, so the cache and lookup entry points run without a GPU. */
int ngz_enrich_create(int device, const char *writer_id, ngz_enrich **out);
void ngz_enrich_destroy(ngz_enrich *e);
const char *ngz_enrich_last_error(ngz_enrich *e);
const char *ngz_enrich_writer_id(ngz_enrich *e);

/* Options: NGZ_ENRICH_OPT_TABLE_BITS forces every device lookup table to 2^value slots (3..24;
 * 0 = sized by its entries, at most half full); a table always has more slots than entries (a
 * forced size too small for a table is raised to the next that holds it), so tests reach long
 * probe chains with it.  Changes how an apply runs, never its results. */
#define NGZ_ENRICH_OPT_TABLE_BITS 1
int ngz_enrich_set_option(ngz_enrich *e, int opt, int64_t value);

/* NGZ_E_INVALID: a malformed operation (kind, peer family, a null array, a value kind that is not
 * a column encoding).  NGZ_E_LIMIT: more than NGZ_ENRICH_MAX_SCOPE_FIELDS scope fields, or a scope
 * field of a kind or length outside the list above.  Either leaves the cache and its generation
 * unchanged. */
int ngz_enrich_op(ngz_enrich *e, const ngz_enrich_operation *op);
uint64_t ngz_enrich_peer_count(ngz_enrich *e);
/* Bumped by every operation that changed the cache. */
uint64_t ngz_enrich_generation(ngz_enrich *e);

/* get_enrichment_fields for one record on the host: `record` are its non-scope fields in record
 * order.  The resolved fields in ascending (PEN, IE id, index) into out[0, cap); returns their
 * number (> cap: only cap written; 0: the reference's None). */
int ngz_enrich_lookup(ngz_enrich *e, const ngz_enrich_peer *peer, uint32_t obs_domain_id, const ngz_enrich_field *record,
                      uint32_t n_record, ngz_enrich_resolved *out, uint32_t cap);

/* The stage over the batch last decoded on ctx (`out` is that decode's result), for the exporter
 * `peer`.  Synchronous.  Reads the decoded columns and writes nothing into the context's arena;
 * the results live in the enricher until the next apply for ctx or ctx's next decode.  Applying
 * the same batch again replaces them (the cache may have changed).  The peer's lookup tables are
 * uploaded when its part of the cache changed since the last upload.  One launch of the row kernel
 * per slot whose plan has a candidate scope, on the context's stream (or hip_stream).
 * NGZ_E_INVALID: a decode pending on ctx (ngz_decode_batch_submit), ctx on another device.
 * NGZ_E_LIMIT: a slot plan past NGZ_ENRICH_MAX_SHAPES or NGZ_ENRICH_MAX_COLUMNS, a peer with more
 * than NGZ_ENRICH_MAX_DOMAINS domains. */
int ngz_enrich_apply(ngz_enrich *e, ngz_ctx *ctx, const ngz_batch_out *out, const ngz_enrich_peer *peer,
                     ngz_enrich_stats *batch_stats /* may be NULL */, void *hip_stream);
int ngz_enrich_totals(ngz_enrich *e, ngz_enrich_stats *totals, int reset);

/* The added columns of a slot of the batch last applied on ctx, which must still be ctx's last
 * decode (NGZ_E_INVALID otherwise): one per distinct FieldRef that a candidate scope of the peer can
 * add, in ascending (PEN, IE id, index), into cols[0, cap).  A candidate scope is one whose every
 * FieldRef the template has as a non-scope column of the scope value's kind and width.  *dev_mask:
 * one uint32_t per row, bit c = column c is present; rows of failed messages and of dropped
 * templates have mask 0.  *n = the slot's n_records.  Returns the number of columns (> cap: only
 * cap written).  Each context's results are its own: an apply for another context leaves them. */
int ngz_enrich_slot_columns(ngz_enrich *e, ngz_ctx *ctx, uint32_t slot, ngz_enrich_column *cols, uint32_t cap,
                            const uint32_t **dev_mask, uint32_t *n);

/* The fields the reference appends to the record at `row` of `slot`, as ngz_field_values in the
 * canonical order, dataCollectionManifestName(writer_id) (PEN 3746, id 7) last, into out[0, cap): a
 * Rust host extends Box<[Field]> with them.  `value` points into host copies the
 * enricher keeps until the next apply for ctx (one D2H on the first call), into the value arena for
 * NGZ_K_VLEN.  Returns the field count (> cap: only cap written); NGZ_E_INVALID for a row that is
 * not an enriched record (scope fields, a message that did not decode) or a stale batch. */
int ngz_enrich_row_fields(ngz_enrich *e, ngz_ctx *ctx, uint32_t slot, uint32_t row, ngz_field_value *out, uint32_t cap);

/* Drop what the enricher keeps for ctx (results, device buffers): before ngz_ctx_destroy. */
int ngz_enrich_forget(ngz_enrich *e, ngz_ctx *ctx);

/* serde JSON of the enriched FlowInfos of the batch last applied on ctx, which must still be its
 * last decode (ngz_batch_json's contract and callback): template and options-template sets removed,
 * records with scope fields removed, each record's appended fields after its own in the canonical
 * order, {"NetGauze":{"dataCollectionManifestName":..}} last; with `renorm` (may be NULL), which
 * must have applied this batch (ngz_renorm_apply_enriched or ngz_renorm_apply),
 * {"NetGauze":{"isRenormalized":true}} after that for flagged rows.  A mode of the renderer behind
 * ngz_renorm_batch_json. */
struct ngz_renorm;
int64_t ngz_enrich_batch_json(ngz_enrich *e, struct ngz_renorm *renorm, ngz_ctx *ctx, const uint8_t *host_bytes,
                              ngz_json_line_fn fn, void *user);

/* Introspection, no device: the plan for one IPFIX (proto 10) / NetFlow v9 (proto 9) template
 * record of `peer` (proto | NGZ_ENRICH_OPTIONS: an options template record; layouts as
 * ngz_renorm_template_plan): whether its records are dropped, the scope shapes of the peer the
 * template can satisfy (a shape naming a FieldRef the template lacks, or one whose column decodes
 * with another kind or width than the scope's value, is left out), and the added columns.
 * NGZ_E_LIMIT past NGZ_ENRICH_MAX_SHAPES / NGZ_ENRICH_MAX_COLUMNS. */
#define NGZ_ENRICH_OPTIONS 0x100
typedef struct {
    uint32_t pen;
    uint16_t ie_id;
    uint16_t index;
} ngz_enrich_ref;
typedef struct {
    uint8_t dropped;    /* the template has scope fields: its records are dropped */
    uint8_t launches;   /* 0: no candidate scope, no kernel for this template */
    uint8_t n_shapes;
    uint8_t n_columns;
    uint8_t shape_len[NGZ_ENRICH_MAX_SHAPES];
    ngz_enrich_ref shape[NGZ_ENRICH_MAX_SHAPES][NGZ_ENRICH_MAX_SCOPE_FIELDS];
    ngz_enrich_ref column[NGZ_ENRICH_MAX_COLUMNS];  /* ascending (PEN, IE id, index) */
    uint8_t column_kind[NGZ_ENRICH_MAX_COLUMNS];
    uint16_t column_width[NGZ_ENRICH_MAX_COLUMNS];
} ngz_enrich_plan;
int ngz_enrich_template_plan(ngz_enrich *e, const ngz_enrich_peer *peer, const uint8_t *tmpl, size_t len, int proto,
                             ngz_enrich_plan *out);

/* The bytes NGZ_K_VLEN added columns point into: device and host copies, and their size. */
int ngz_enrich_value_arena(ngz_enrich *e, const uint8_t **dev, const uint8_t **host, uint64_t *size);

/* Device milliseconds of the last apply's kernels (HIP events round them). */
int ngz_enrich_last_timing(ngz_enrich *e, float *apply_ms);

#ifdef __cplusplus
}
#endif
#endif
