/*
 * netgauze_amd — the Encoder half of FlowInfoCodec on the device: the IPFIX / NetFlow v9 message of every
 * decoded datagram, written again from the decoded columns (Encoder for FlowInfoCodec, codec.rs:100-140,
 * over wire/serializer/{ipfix,netflow,ie}.rs).  flow_json.h and flow_output.h are the JSON and Avro
 * publishers over the same decoded records.
 *
 * Specification: ngz_dgram_wire(ctx, d) returns the bytes IpfixPacket::write / NetFlowV9Packet::write give
 * for the packet datagram d decoded to, with the context's templates as the TemplatesMap, template and
 * options-template sets included (serializer/ipfix.rs:47-71,84-150,162-339, serializer/netflow.rs).  For
 * every datagram d with how[d] == NGZ_WIRE_WIRE, bytes[offsets[d], offsets[d+1]) of the device stage is
 * that, byte for byte.  Every other datagram has a zero-length message on the device.
 *
 *   NGZ_WIRE_NONE        the datagram's status is not NGZ_DG_OK: there is no packet.
 *   NGZ_WIRE_WIRE        written on the device.
 *   NGZ_WIRE_HOST        an OK datagram with a template or options-template set, and no unwritable data
 *                        set: ngz_dgram_wire writes it (the specifiers live on the host).
 *   NGZ_WIRE_UNWRITABLE  an OK datagram with a data set of an unwritable template (below):
 *                        ngz_dgram_wire returns NGZ_E_INVALID for it.
 *
 * The columns are read as they are at the time of the call: an encode after ngz_renorm_apply carries the
 * scaled counts, and a message is the normal form of its input, not a copy: set padding is gone, a short
 * variable-length value has a one-byte prefix, a fixed string is zero after its first NUL.
 *
 * Field bytes (generator.rs:2982-3560, the vendor packages' :1863-2410 are the same), by the column
 * encodings of DESIGN.md §3, L the template's length:
 *   unsigned / signed / float / boolean, sub-registry enums (through their numeric value), tcpControlBits
 *     (as u16), ipv4Address, dateTimeSeconds, the NFv9 System / Interface / LineCard scopes: the low L
 *     bytes of the Rust width, big-endian;
 *   dateTimeMilliseconds: u64; dateTimeMicro- / Nanoseconds: u32 seconds, then u32
 *     nanos * (2^32 - 1) / 10^9 in integer arithmetic (a fraction does not round-trip exactly);
 *   ipv6Address, macAddress, MPLS labels, fixed octetArray, lists, unknown IEs, other NFv9 scopes: their
 *     bytes; unsigned256: the first L of its 32;
 *   fixed string: the bytes before the first NUL, zero-filled to L;
 *   L = 65535 (IPFIX) on octetArray, string and a vendor's unknown IE: a length prefix, one byte below
 *     255 bytes, 0xFF and three bytes otherwise, then the value; on basicList, subTemplateList and
 *     subTemplateMultiList the value with no prefix, as the reference writes them; on IE::Unknown the
 *     prefix and its 65535 bytes.
 * Messages: IPFIX sets carry no padding; the IPFIX length and every set length are `as u16`.  The NFv9
 * header count is the number of records of all sets (netflow.rs:60-70).  NGZ_WIRE_OPT_ALIGN4 (default 0)
 * is the NFv9 writer's align_to_4_bytes, exactly as calculate_set_size_with_padding (:116-134) has it:
 * length % 4 zero bytes after the set, counted in its length.
 *
 * Unwritable templates.  The reference writer ignores the template's length for the single-byte types
 * and the types it writes at their natural width, while DataRecord::len trusts the template, so the
 * set length it writes disagrees with its bytes for these (type, length) pairs:
 *   unsigned8, signed8, boolean with L != 1;  macAddress with L != 6;  ipv4Address, dateTimeSeconds with
 *   L != 4;  ipv6Address with L != 16;  dateTimeMilli- / Micro- / Nanoseconds with L != 8;
 *   and under NetFlow v9, where 65535 is a literal length (netflow.rs:298-328 sums the template's
 *   lengths), octetArray, string, the list types and unknown IEs with L = 65535, whose writers emit the
 *   value's bytes (with or without a prefix).
 * The decode refuses every pair of the first line (InvalidLength: the datagram is not OK), so the
 * NetFlow v9 pairs are the ones a decoded batch can hold records of.  A template with a refused pair (or
 * any other length the decode refuses) still has a slot in every batch of its context: the stage plans
 * that slot as never written and goes on, so such a template disables nothing.  An OK datagram with a
 * data set of an unwritable template, records or not, is NGZ_WIRE_UNWRITABLE; one whose records the
 * decode refused is not OK and NGZ_WIRE_NONE.
 *
 * Output, in device memory the stage owns until its next encode: `bytes`, the messages back to back in
 * datagram order, NGZ_OUTPUT_GUARD bytes of 0xA5 after them, `offsets[n_dgrams + 1]` (u64) and
 * `how[n_dgrams]` (u8).  Nothing is written into the context's arena.
 *
 * Device path (ngz_wire.hip): flow_json.h's set and tile bookkeeping (a tile is at most 64
 * consecutive records of one data set); tile sizes of fixed-length templates come from record counts, a
 * counting pass runs over the tiles of variable-length templates only; heads and set headers are written
 * by bytes; a transpose kernel packs fixed-length tiles (column loads, byte reversal in registers, a
 * record image in LDS, 16-byte stores out), a writer kernel the variable-length ones.  The number of
 * launches does not depend on the number of templates.  A batch with no datagram launches nothing.
 *
 * Limits (NGZ_E_LIMIT): an integer column that is not 1, 2, 4 or 8 bytes wide.  Return codes as
 * flow_output.h.  A stage object is not thread-safe; the context is only read.
 */
#ifndef NGZ_FLOW_WIRE_H
#define NGZ_FLOW_WIRE_H

#include "ngz/flow_decode.h"
#include "ngz/flow_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NGZ_WIRE_ABI_VERSION 1

#define NGZ_WIRE_NONE 0
#define NGZ_WIRE_WIRE 1
#define NGZ_WIRE_HOST 2
#define NGZ_WIRE_UNWRITABLE 3

#define NGZ_WIRE_OPT_ALIGN4 1 /* NetFlow v9 align_to_4_bytes: 0 (default) or 1 */

typedef struct ngz_wire ngz_wire;

typedef struct {          /* of the last encode */
    uint64_t wire;          /* datagrams written on the device (NGZ_WIRE_WIRE) */
    uint64_t bytes;         /* bytes of all messages */
    uint64_t left_template; /* OK datagrams left to ngz_dgram_wire for their (options) template sets */
    uint64_t unwritable;    /* OK datagrams with a data set of an unwritable template */
    uint64_t not_ok;        /* datagrams whose status is not NGZ_DG_OK */
} ngz_wire_stats;

int ngz_wire_abi_version(void);

/* The message of datagram `dgram` of the batch last decoded on ctx into buf[0, cap) (as much of it as
 * fits; buf may be NULL); ngz_dgram_wire_aligned: with the NetFlow v9 align_to_4_bytes option on.
 * Returns its length, or NGZ_E_INVALID: no such datagram, its status is not NGZ_DG_OK, or it holds a
 * data set of an unwritable template.  The first call after a decode copies the batch to the host. */
int64_t ngz_dgram_wire(ngz_ctx *ctx, uint32_t dgram, uint8_t *buf, size_t cap);
int64_t ngz_dgram_wire_aligned(ngz_ctx *ctx, uint32_t dgram, uint8_t *buf, size_t cap);

/* A stage for `device`.  Makes no HIP call. */
int ngz_wire_create(int device, ngz_wire **out);
void ngz_wire_destroy(ngz_wire *w);
const char *ngz_wire_last_error(ngz_wire *w);
/* NGZ_WIRE_OPT_*; NGZ_E_INVALID for an unknown option or value. */
int ngz_wire_set_option(ngz_wire *w, int option, int64_t value);

/* The stage over the batch last decoded on ctx (`out` is that decode's result).  Synchronous.  Reads the
 * decoded columns, the set table, the datagram headers and the batch input (variable-length values:
 * the input of the decode must still be valid).  NGZ_E_INVALID: a decode pending on ctx, ctx on another
 * device, `out` not the context's last decode, a variable-length cell outside the batch input. */
int ngz_wire_encode(ngz_wire *w, ngz_ctx *ctx, const ngz_batch_out *out, ngz_wire_stats *stats /* may be NULL */, void *hip_stream);

/* The last encode: device pointers valid until the next encode (NULL after an encode of no datagram). */
int ngz_wire_result(ngz_wire *w, const uint8_t **bytes, const uint64_t **offsets, const uint8_t **how, uint64_t *n_dgrams,
                    uint64_t *n_bytes);

/* The messages into bytes[0, bytes_cap), the n_dgrams + 1 offsets into offsets[0, offsets_cap) and `how`
 * into how[0, how_cap) (each may be NULL); with room for them the guard bytes follow the messages. */
int ngz_wire_to_host(ngz_wire *w, uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets, uint64_t offsets_cap, uint8_t *how,
                     uint64_t how_cap);

/* Device milliseconds of the last encode: the size pass (set pass, tile table, the counting pass over
 * variable-length tiles), the offsets (the two sums and the scan), the glue passes, the pack passes. */
int ngz_wire_last_timing(ngz_wire *w, float *size_ms, float *offsets_ms, float *glue_ms, float *pack_ms);
/* Kernels the last encode launched (a scan counts as one); 0 for no datagram. */
int ngz_wire_last_launches(ngz_wire *w);

#ifdef __cplusplus
}
#endif
#endif
