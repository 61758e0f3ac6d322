/*
 * netgauze_amd — flow output on the device: the decoded records of a batch turned into the flat
 * Avro datums both flow publishers of the reference collector send,
 *
 *   decode -> FlowOutputConfig::get_avro_values -> encode_value -> Kafka
 *             crates/collector/src/flow/config.rs:56-216, publishers/kafka_avro.rs:335-337
 *
 *   ngz_output               ≙ one validated FlowOutputConfig (config.rs:56-69).
 *   ngz_output_schema        ≙ get_avro_schema (:149-169, get_record_schema :454-522), byte for byte.
 *   ngz_output_template_plan ≙ FieldRef::map_fields_into_fxhashmap (:113, :194-213) and every select
 *                              (:576-763) as far as the template alone decides them.
 *   ngz_output_encode        ≙ get_avro_values (:189-215): get_avro_value_from_fields (:105-145) per
 *                              data record, each value written in the Avro binary encoding.
 *
 * Semantics.  A field is (name, select, transform, optional default) as FieldConfig (:238-557), evaluated
 * per record as avro_value (:532-543): select, transform, then the default where the result is None.  A
 * field without a default is nullable (:524-526) and written as the union ["null", T]: branch 0, or
 * branch 1 and the value; a field with a default is a bare T.  The datum is the fields in config order:
 * long / int zigzag varints, string / bytes a long length and the bytes, float / double little-endian,
 * boolean one byte, array one block (count, items, 0).  The 5-byte schema-registry prefix encode_value
 * adds is the caller's.  A FieldRef (IE, index) counts occurrences among the template's non-scope fields
 * only (record.fields()).
 *
 * Accepted (everything else is refused by ngz_output_create, never approximated):
 *   selects     Single; Coalesce of up to NGZ_OUTPUT_MAX_COALESCE refs (the first one the template holds);
 *               Layer2SegmentId (top byte == encapsulation type, then masked, :746-762); Multi under
 *               MplsIndex only.
 *   Identity    on IEs whose Field converts natively (generator.rs:2628-2636, flow/mod.rs:133-183):
 *               unsigned8/16, signed8/16/32 -> int; unsigned32/64 (as i64), signed64 -> long; float32/64;
 *               boolean; string; macAddress, ipv4Address, ipv6Address -> their text; octetArray, the
 *               list types, unsigned256 -> bytes.  A Coalesce needs one Avro type (:644-659).
 *   String      on integers (decimal), boolean, string, ipv4Address, ipv6Address (Rust's Ipv6Addr
 *               Display) and macAddress (aa:bb:.., generator.rs:2645-2647).  The MPLS label IEs have
 *               a String conversion (:2650-2651), but they are octetArrays, so validate rejects
 *               String on them as on any bytes type (config.rs:425): refused, as there.
 *   MplsIndex   over Multi of mplsLabelStackSection 1..10: an array of "{n}-{label}" over the present
 *               ones in select order, None if none is (:964-996).
 *   defaults    the scalar, string and bytes kinds of RawValue, of the field's Avro type (:441-452).
 * Refused with NGZ_OUTPUT_E_UNSUPPORTED (the message names the field):
 *   Identity on IEs with a sub-registry, tcpControlBits, the MPLS label IEs and the four dateTime types:
 *   their From<Field> for RawValue falls through to the String fallback (flow/mod.rs:179-182,
 *   generator.rs:2631-2634), which contradicts the schema's own type;
 *   String on floats, dateTimes, sub-registry IEs, tcpControlBits and the route distinguisher, whose
 *   Display text nothing here pins; TrimmedString, LowercaseString, TimestampMillisString, Rename,
 *   StringArray, StringArrayAgg, StringMapAgg; "custom_primitives." names; TimestampMillis, StringArray
 *   and StringMap defaults; IEs the registry does not know.
 * Refused with NGZ_OUTPUT_E_CONFIG: what FieldConfig::validate rejects (:254-452): an empty Coalesce or
 *   Multi, Multi without an aggregating transform, MplsIndex without Multi or on other IEs, a mixed-type
 *   Coalesce under Identity, Layer2SegmentId on another IE, String on a bytes type, a default of another
 *   Avro type.
 *
 * Rows.  One datum per row of every slot, in the slot's stream order (pair rows with (datagram, set,
 * record) through the set table, as ngz_record_fields does).  Rows of a datagram whose status is not
 * NGZ_DG_OK give a zero-length datum and are counted (rows_failed).  A slot none of whose fields can be
 * present still gives its rows: nulls and defaults.  The plan reads a slot's own columns only: no
 * enrichment columns; aggregated rows, what the Avro publisher sends, are flow_agg_output.h's.
 *
 * Output, per batch slot, in device memory the stage owns until its next encode: `bytes`, the datums
 * back to back in row order, and `offsets[n_rows + 1]` (u64): row r is bytes[offsets[r], offsets[r+1]).
 * Variable-length values are read from the batch input through the column's {offset, length}: the input
 * of the decode must still be valid during the encode, as for the variable-length columns themselves.
 *
 * Device path (ngz_output.hip): no kernel for a batch without rows.  One set pass marks the rows of
 * failed messages; per slot with rows one size launch (four rows per lane, vector column loads, four
 * lengths in one 16-byte store), one exclusive scan (u64 offsets), and one pack launch (a wave encodes
 * its 64 consecutive rows into an LDS image and copies it out in 16-byte stores).
 *
 * Limits (NGZ_E_LIMIT): NGZ_OUTPUT_MAX_FIELDS fields, NGZ_OUTPUT_MAX_SOURCES present sources per slot
 * over all fields, NGZ_OUTPUT_MAX_DEFAULT encoded bytes per default, NGZ_OUTPUT_MAX_NAME per name.
 *
 * Return codes as flow_decode.h plus the two below.  A stage object is not thread-safe.
 */
#ifndef NGZ_FLOW_OUTPUT_H
#define NGZ_FLOW_OUTPUT_H

#include "ngz/flow_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_OUTPUT_ABI_VERSION 1
#define NGZ_OUTPUT_MAX_FIELDS 64
#define NGZ_OUTPUT_MAX_COALESCE 8
#define NGZ_OUTPUT_MAX_REFS 10     /* refs of one select (Multi of the ten MPLS label IEs) */
#define NGZ_OUTPUT_MAX_SOURCES 96  /* columns one slot's plan reads, over all fields */
#define NGZ_OUTPUT_MAX_DEFAULT 64
#define NGZ_OUTPUT_MAX_NAME 128
#define NGZ_OUTPUT_GUARD 64        /* bytes of 0xA5 the stage keeps after each slot's `bytes` */

#define NGZ_OUTPUT_E_UNSUPPORTED (-20) /* a config outside the accepted subset */
#define NGZ_OUTPUT_E_CONFIG (-21)      /* a config FieldConfig::validate rejects */

/* FieldSelectFunction */
#define NGZ_OUT_SEL_SINGLE 0
#define NGZ_OUT_SEL_COALESCE 1
#define NGZ_OUT_SEL_MULTI 2
#define NGZ_OUT_SEL_L2SEGMENT 3
/* FieldTransformFunction (3..9 are named so that they can be refused) */
#define NGZ_OUT_TR_IDENTITY 0
#define NGZ_OUT_TR_STRING 1
#define NGZ_OUT_TR_MPLS_INDEX 2
#define NGZ_OUT_TR_TRIMMED_STRING 3
#define NGZ_OUT_TR_LOWERCASE_STRING 4
#define NGZ_OUT_TR_TIMESTAMP_MILLIS_STRING 5
#define NGZ_OUT_TR_RENAME 6
#define NGZ_OUT_TR_STRING_ARRAY 7
#define NGZ_OUT_TR_STRING_ARRAY_AGG 8
#define NGZ_OUT_TR_STRING_MAP_AGG 9
/* RawValue kind of a default (14..16 are named so that they can be refused) */
#define NGZ_OUT_DEF_NONE 0
#define NGZ_OUT_DEF_BYTES 1
#define NGZ_OUT_DEF_U8 2
#define NGZ_OUT_DEF_U16 3
#define NGZ_OUT_DEF_U32 4
#define NGZ_OUT_DEF_U64 5
#define NGZ_OUT_DEF_I8 6
#define NGZ_OUT_DEF_I16 7
#define NGZ_OUT_DEF_I32 8
#define NGZ_OUT_DEF_I64 9
#define NGZ_OUT_DEF_F32 10
#define NGZ_OUT_DEF_F64 11
#define NGZ_OUT_DEF_BOOLEAN 12
#define NGZ_OUT_DEF_STRING 13
#define NGZ_OUT_DEF_TIMESTAMP_MILLIS 14
#define NGZ_OUT_DEF_STRING_ARRAY 15
#define NGZ_OUT_DEF_STRING_MAP 16
/* AvroValueKind of a field */
#define NGZ_OUT_T_INT 1
#define NGZ_OUT_T_LONG 2
#define NGZ_OUT_T_FLOAT 3
#define NGZ_OUT_T_DOUBLE 4
#define NGZ_OUT_T_BOOLEAN 5
#define NGZ_OUT_T_STRING 6
#define NGZ_OUT_T_BYTES 7
#define NGZ_OUT_T_ARRAY 8

typedef struct ngz_output ngz_output;

typedef struct {
    uint32_t pen;
    uint16_t ie_id;
    uint16_t index; /* occurrence index among the record's non-scope fields */
} ngz_output_ref;

typedef struct {
    const char *name;
    uint8_t select;           /* NGZ_OUT_SEL_* */
    uint8_t transform;        /* NGZ_OUT_TR_* */
    uint8_t default_kind;     /* NGZ_OUT_DEF_* */
    uint8_t encap_type;       /* Layer2SegmentId: the encapsulation type (1 VxLAN, 2 NVGRE) */
    uint8_t encap_unassigned; /* Layer2SegmentId::Unassigned(encap_type): the 40-bit mask */
    uint8_t reserved[3];
    uint32_t n_refs;
    const ngz_output_ref *refs;
    uint64_t default_scalar;  /* integer kinds: the value (signed ones sign-extended); F32 / F64: the
                                 IEEE bits; BOOLEAN: 0 / 1 */
    const uint8_t *default_bytes; /* BYTES / STRING */
    uint32_t default_len;
    uint32_t reserved2;
} ngz_output_field;

typedef struct {
    uint8_t avro_type;  /* NGZ_OUT_T_* */
    uint8_t nullable;
    uint8_t n_present;  /* refs the template holds that the record's value is built from: 0 (null or
                           the default), 1, or up to 10 under MplsIndex */
    uint8_t reserved;
    int16_t src[NGZ_OUTPUT_MAX_REFS]; /* their template field indices (scope fields first), select order */
} ngz_output_field_plan;

typedef struct {
    uint32_t n_fields;
    uint32_t reserved;
    ngz_output_field_plan f[NGZ_OUTPUT_MAX_FIELDS];
} ngz_output_plan;

typedef struct {        /* per call or running total */
    uint64_t rows;        /* datums written, the zero-length ones included */
    uint64_t rows_failed; /* rows of messages that did not decode: zero-length datums */
    uint64_t bytes;       /* bytes of all datums */
} ngz_output_stats;

int ngz_output_abi_version(void);

/* One FlowOutputConfig of n fields for contexts on `device`.  Makes no HIP call.  On a refused config
 * the reason, naming the field, goes to err[0, err_cap) (NUL-terminated; may be NULL). */
int ngz_output_create(int device, const ngz_output_field *fields, uint32_t n, ngz_output **out, char *err, size_t err_cap);
void ngz_output_destroy(ngz_output *o);
const char *ngz_output_last_error(ngz_output *o);

/* Diagnostic switches, kept so that the two design choices below can be measured again
 * (tools/bench_output.py); a host has no reason to set them.  How the pack pass runs, never what it writes.  NGZ_OUTPUT_OPT_RECOMPUTE 0 (default): a lane reads its
 * row's two scanned offsets back; 1: it sizes the row again and a wave scan places it after the tile's
 * first offset.  NGZ_OUTPUT_OPT_IMAGE: bytes of LDS per wave image, 8192 (default) or 4096.  Defaults as
 * measured, profiles/output/summary.txt. */
#define NGZ_OUTPUT_OPT_RECOMPUTE 1
#define NGZ_OUTPUT_OPT_IMAGE 2
int ngz_output_set_option(ngz_output *o, int opt, int64_t value);

/* The text of get_avro_schema into buf (truncated to cap, NUL-terminated); its length.  Host only.  As in
 * the reference a name goes into the text unescaped: a name with a quote or a backslash gives a schema
 * that is no JSON, there and here; ngz_output_create does not refuse it. */
int64_t ngz_output_schema(ngz_output *o, char *buf, size_t cap);

/* No device: the plan of one IPFIX (proto 10) / NetFlow v9 (proto 9) template record
 * (proto | NGZ_OUTPUT_OPTIONS: an options template record; layouts as ngz_renorm_template_plan).
 * NGZ_E_INVALID: a record that does not parse; NGZ_E_LIMIT past NGZ_OUTPUT_MAX_SOURCES. */
#define NGZ_OUTPUT_OPTIONS 0x100
int ngz_output_template_plan(ngz_output *o, const uint8_t *tmpl, size_t len, int proto, ngz_output_plan *plan);

/* The stage over the batch last decoded on ctx (`out` is that decode's result).  Synchronous.  Reads the
 * decoded columns, the set table, the datagram headers and the batch input; writes nothing into the
 * context's arena.  NGZ_E_INVALID: a decode pending on ctx, ctx on another device, `out` not the
 * context's last decode, a variable-length cell outside the batch input. */
int ngz_output_encode(ngz_output *o, ngz_ctx *ctx, const ngz_batch_out *out, ngz_output_stats *batch_stats /* may be NULL */,
                      void *hip_stream);

/* Slot `slot` of the last encode: device pointers valid until the next encode (NULL for a slot without
 * rows), its rows and the bytes of its datums. */
int ngz_output_slot(ngz_output *o, uint32_t slot, const uint8_t **bytes, const uint64_t **offsets, uint64_t *n_rows,
                    uint64_t *n_bytes);

/* Copies one slot to the host: its datums into bytes[0, bytes_cap) and its n_rows + 1 offsets into
 * offsets[0, offsets_cap) (either may be NULL).  With room for them the NGZ_OUTPUT_GUARD bytes after the
 * datums follow them.  NGZ_E_INVALID when a buffer is too small. */
int ngz_output_to_host(ngz_output *o, uint32_t slot, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap);

int ngz_output_totals(ngz_output *o, ngz_output_stats *totals, int reset);
/* Device milliseconds of the last encode's size passes (with their scans) and pack passes. */
int ngz_output_last_timing(ngz_output *o, float *size_ms, float *pack_ms);
/* Kernels the last encode launched (a scan counts as one); 0 for a batch without rows. */
int ngz_output_last_launches(ngz_output *o);

#ifdef __cplusplus
}
#endif
#endif
