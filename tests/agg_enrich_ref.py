"""The aggregation over enriched records, composed from the restatements (TEST INFRASTRUCTURE ONLY):
the checker of ngz_agg_push_enriched (include/ngz/flow_aggregate.h).

The reference collector chains enrichment into aggregation (crates/collector/src/lib.rs:140-163):
the aggregation's explode runs FieldRef::map_fields over each record as the enrichment actor left it
(crates/collector/src/flow/enrichment/actor.rs:141-153, :176-187):
  - the record's own non-scope fields in template order,
  - the cache fields resolved for it (tests/enrich_ref.py's lookup), here in ascending
    (PEN, IE id, cache index) -- the reference appends them in FxHashMap order,
  - dataCollectionManifestName(writer_id) last;
records with scope fields are removed (actor.rs:178, :237).  The packets then go to
oracle/ngz_agg_oracle.FlowAggregatorOracle unchanged: its explode already runs map_fields over
whatever fields a record has, and a packet left with no record explodes to no item, so it neither
advances the event time nor counts as late (analytics/src/aggregation.rs:124-172).
"""
import struct

import enrich_ref as E
import ngz_agg_oracle as A
import ngz_oracle as O
import renorm_ref as R

_UINT = {"unsigned8": 1, "unsigned16": 2, "unsigned32": 4, "unsigned64": 8}


def restated(fields):
    """The oracle's [Field] of a record as enrich_ref fields (pen, ie_id, kind, value): unsigned IEs
    at their IE's width (the canonical column encoding), strings and octets as they are; a field of
    another type is no scope candidate (kind 0 matches no scope value)."""
    out = []
    for f in fields:
        pen, ie, v = f.ie.pen, f.ie.id, f.value
        if f.ie.dtype in _UINT and isinstance(v, int) and not isinstance(v, bool):
            out.append((pen, ie, E.K_UINT, v.to_bytes(_UINT[f.ie.dtype], "little")))
        elif isinstance(v, str):
            out.append((pen, ie, E.K_STR, v.encode("utf-8")))
        elif isinstance(v, (bytes, bytearray)):
            out.append((pen, ie, E.K_BYTES, bytes(v)))
        else:
            out.append((pen, ie, 0, b""))
    return out


def enrich_packet(pkt, cache, ip, writer_id):
    """EnrichmentActor::enrich of one decoded packet, in place."""
    domain = pkt.observation_domain_id if isinstance(pkt, O.IpfixPacket) else pkt.source_id
    writer = O.Field(O.REGISTRY.lookup(*E.WRITER_ID_IE), writer_id)
    sets = []
    for kind, sid, recs in pkt.sets:
        if kind == "Data":
            recs = [(scope, list(fields) + [E.oracle_field(g) for g in cache.lookup(ip, domain, restated(fields))] + [writer])
                    for scope, fields in recs if not len(scope)]
        sets.append((kind, sid, recs))
    pkt.sets = sets
    return pkt


class EnrichCodec(O.FlowInfoCodec):
    """A peer's codec whose packets leave as the enrichment actor (and, with renormalize, the
    renormalization actor after it) would pass them on."""

    def __init__(self, cache, ip, writer_id, renormalize=False):
        super().__init__()
        self.cache, self.ip, self.writer_id, self.renormalize = cache, ip, writer_id, renormalize

    def decode(self, buf):
        pkt = super().decode(buf)
        if pkt is not None:
            enrich_packet(pkt, self.cache, self.ip, self.writer_id)
            if self.renormalize:
                R.renormalize_packet(pkt, R.new_stats())
        return pkt


def aggregate(fields, datagrams, cache, ip=A.DEFAULT_PEER, writer_id="w", agg=None, codec=None, renormalize=False, **kw):
    """ngz_agg_oracle.aggregate_datagrams over the enriched packets; returns (aggregator, codec)."""
    codec = codec if codec is not None else EnrichCodec(cache, ip, writer_id, renormalize)
    return A.aggregate_datagrams(fields, datagrams, peer_ip=ip, agg=agg, codec=codec, **kw), codec


def group_tuple(g):
    """Everything the tests compare of one output group, hashable and sortable."""
    return (g["peer"], g["window_start"], g["flow_type"], repr(g["key"]), repr(g["vals"]), g["record_count"], g["min_export"],
            g["max_export"], g["max_sysup"], g["min_coll"], g["max_coll"], tuple(sorted(g["templates"])),
            tuple(sorted(g["ports"])), tuple(sorted(g["domains"])))


# ----------------------------------------------------------------------------------------------
# wire messages
# ----------------------------------------------------------------------------------------------
T0 = 1_700_000_040  # a minute boundary + 0: windows start at multiples of 60
V = 0xFFFF


def spec(fields):
    return b"".join(struct.pack(">HH", i, n) if not p else struct.pack(">HHI", i | 0x8000, n, p)
                    for (p, i), n in [((f[0] if isinstance(f[0], tuple) else (0, f[0])), f[1]) for f in fields])


def ipfix_msg(sets, t=T0, seq=0, domain=1):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIII", 10, 16 + len(body), t, seq, domain) + body


def nf9_msg(sets, count, t=T0, seq=0, source=1, sysup=1000):
    body = b""
    for sid, b in sets:
        pad = (-len(b)) % 4
        body += struct.pack(">HH", sid, 4 + len(b) + pad) + b + b"\0" * pad
    return struct.pack(">HHIIII", 9, count, sysup, t, seq, source) + body


def template_msg(proto, templates, **kw):
    body = b"".join(struct.pack(">HH", tid, len(f)) + spec(f) for tid, f in templates)
    return ipfix_msg([(2, body)], **kw) if proto == 10 else nf9_msg([(0, body)], len(templates), **kw)


def options_template_msg(tid, scope, fields, **kw):
    """IPFIX options template: `scope` scope fields, then `fields`."""
    return ipfix_msg([(3, struct.pack(">HHH", tid, len(scope) + len(fields), len(scope)) + spec(scope + fields))], **kw)


def record(fields, values):
    out = b""
    for (_ie, n), v in zip(fields, values):
        if n == V:
            out += (bytes([len(v)]) if len(v) < 255 else b"\xff" + len(v).to_bytes(2, "big")) + v
        elif isinstance(v, bytes):
            out += v
        else:
            out += (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
    return out


def data_msg(proto, tid, recs, **kw):
    return ipfix_msg([(tid, b"".join(recs))], **kw) if proto == 10 else nf9_msg([(tid, b"".join(recs))], len(recs), **kw)


def u(ie, v, w=4, pen=0):
    return (pen, ie, E.K_UINT, int(v).to_bytes(w, "little"))


def s(ie, text, pen=0):
    return (pen, ie, E.K_STR, text if isinstance(text, bytes) else text.encode("utf-8"))


def upsert(cache, ip, scope, fields, domain=0, weight=64, enricher=None):
    """One upsert into the restatement's cache and, when given, the product enricher."""
    cache.apply({"op": "upsert", "ip": ip, "domain": domain, "weight": weight, "scope": scope, "fields": fields})
    if enricher is not None:
        enricher.upsert(ip, domain, weight, scope, fields)
