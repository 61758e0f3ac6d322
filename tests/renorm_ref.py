"""Python restatement of the reference collector's flow renormalization
(crates/collector/src/flow/renormalization/logic.rs:30-524), over the oracle's decoded FlowInfo
objects (oracle ngz_oracle: IpfixPacket / NetFlowV9Packet, records as (scope, [Field])) and
their serde JSON.  The checker of include/ngz/flow_renormalize.h.

Arithmetic: Python's int -> float conversion is correctly rounded (nearest even), the product is
an IEEE f64 product, and rust_u64() is Rust's saturating `as u64`.
"""
import math
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import ngz_oracle as O  # noqa: E402

PARAM_IES = (34, 35, 49, 50, 304, 305, 306, 309, 310, 311)
COUNT_IES = (1, 2, 85, 86)  # octetDeltaCount, packetDeltaCount, octetTotalCount, packetTotalCount
U64_MAX = (1 << 64) - 1
STAT_KEYS = ("flows_processed", "flows_renormalized", "ie_missing_or_invalid", "sampling_algorithm_inferred",
             "records_dropped")
IS_RENORMALIZED = O.REGISTRY.lookup(3746, 16)  # NetGauze::isRenormalized


def new_stats():
    return dict.fromkeys(STAT_KEYS, 0)


def f64_from_bits(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def rust_u64(x):
    """`x as u64`: truncate toward zero, saturate at 0 and u64::MAX, NaN -> 0."""
    if math.isnan(x) or x <= 0.0:
        return 0
    if x >= 18446744073709551616.0:
        return U64_MAX
    return int(x)


def scale(count, k):
    """`(count as f64 * k) as u64` (logic.rs:353-365)."""
    return rust_u64(float(count) * k)


def _div(a, b):
    """IEEE f64 division with b != 0 (Python raises where the quotient overflows: 1 / subnormal)."""
    try:
        return a / b
    except OverflowError:
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def factor(params, stats):
    """calculate_renormalization_factor (logic.rs:107-261).  params: {IE id: value} of the record's
    sampling parameters (311 as a float).  Returns k or None; counts into stats."""
    p = params

    def invalid():
        stats["ie_missing_or_invalid"] += 1
        return None

    def count_based():  # :30-48
        if p[305] == 0:
            return invalid()
        return _div(float(p[306]) + float(p[305]), float(p[305]))

    def n_out_of_n():  # :50-68
        if p[309] == 0:
            return invalid()
        return _div(float(p[310]), float(p[309]))

    def probabilistic():  # :70-88
        pr = p[311]
        if pr > 0.0 and pr <= 1.0:
            return _div(1.0, pr)
        return invalid()

    if 304 in p:
        alg = p[304]
        if alg == 1:
            return count_based() if 305 in p and 306 in p else invalid()
        if alg == 3:
            return n_out_of_n() if 309 in p and 310 in p else invalid()
        if alg == 4:
            return probabilistic() if 311 in p else invalid()
        return invalid()
    if 49 in p:
        return float(p[50]) if p[49] in (1, 2) and 50 in p else invalid()
    if 35 in p:
        return float(p[34]) if p[35] in (1, 2) and 34 in p else invalid()
    if 305 in p and 306 in p:
        stats["sampling_algorithm_inferred"] += 1
        return count_based()
    if 309 in p and 310 in p:
        stats["sampling_algorithm_inferred"] += 1
        return n_out_of_n()
    if 311 in p:
        stats["sampling_algorithm_inferred"] += 1
        return probabilistic()
    if 50 in p:
        stats["sampling_algorithm_inferred"] += 1
        return float(p[50])
    if 34 in p:
        stats["sampling_algorithm_inferred"] += 1
        return float(p[34])
    return None


def renormalize_pairs(pairs, stats):
    """renormalize_fields (logic.rs:263-379) over [(IE id, value)] of PEN-0 fields (311 as a float).
    Returns (k or None, new pairs, flagged)."""
    stats["flows_processed"] += 1
    params = {}
    for ie, v in pairs:
        if ie in PARAM_IES:
            params[ie] = v  # the last occurrence wins (:327-341)
    k = factor(params, stats)
    if k is None:
        return None, list(pairs), False
    out, flagged = [], False
    for ie, v in pairs:
        if ie in COUNT_IES:
            v = scale(v, k)
            flagged = True
        out.append((ie, v))
    if flagged:
        stats["flows_renormalized"] += 1
    return k, out, flagged


def _pairs(fields):
    out = []
    for i, f in enumerate(fields):
        if f.ie.kind == "iana" and f.ie.pen == 0 and (f.ie.id in PARAM_IES or f.ie.id in COUNT_IES):
            v = f.value
            if f.ie.id == 311:
                v = f64_from_bits(v[1])
            out.append((i, f.ie.id, v))
    return out


def renormalize_fields(fields, stats):
    """The same over the oracle's [Field]: scales the count fields in place; True if the record
    gets isRenormalized(true)."""
    idx = _pairs(fields)
    _k, new, flagged = renormalize_pairs([(ie, v) for _, ie, v in idx], stats)
    for (i, ie, _), (_, v) in zip(idx, new):
        if ie in COUNT_IES:
            fields[i] = O.Field(fields[i].ie, v)
    return flagged


def renormalize_packet(pkt, stats):
    """renormalize() (logic.rs:381-524) over one decoded packet.  The packet's count fields are
    scaled in place (records with scope fields untouched, counted as dropped); returns the flags
    {(data set index, record index): True} of the records that get isRenormalized(true)."""
    flags = {}
    si = 0
    for kind, _sid, recs in pkt.sets:
        if kind != "Data":
            continue
        for ri, (scope, fields) in enumerate(recs):
            if len(scope):
                stats["records_dropped"] += 1
                continue
            if renormalize_fields(fields, stats):
                flags[(si, ri)] = True
        si += 1
    return flags


def renormalize_batch(oracle, stats=None):
    """Every ("ok", packet) of parity.oracle_datagrams' list, in place.  Returns (stats, per-datagram
    flags)."""
    stats = stats if stats is not None else new_stats()
    flags = []
    for kind, val in oracle:
        flags.append(renormalize_packet(val, stats) if kind == "ok" else {})
    return stats, flags


def packet_json(pkt, flags):
    """serde JSON text of the renormalized FlowInfo: template sets and records with scope fields
    removed, isRenormalized(true) appended to the flagged records."""
    netflow = isinstance(pkt, O.NetFlowV9Packet)
    sets = []
    si = 0
    for kind, sid, recs in pkt.sets:
        if kind != "Data":
            continue
        out = []
        for ri, (scope, fields) in enumerate(recs):
            if len(scope):
                continue
            fj = [O.field_json(x) for x in fields]
            if flags.get((si, ri)):
                fj.append(O.field_json(O.Field(IS_RENORMALIZED, True)))
            out.append({"scope_fields": [], "fields": fj})
        sets.append({"Data": {"id": sid, "records": out}})
        si += 1
    if netflow:
        body = {"NetFlowV9": {"version": 9, "sys_up_time": pkt.sys_up_time, "unix_time": pkt.unix_time.to_json(),
                              "sequence_number": pkt.sequence_number, "source_id": pkt.source_id, "sets": sets}}
    else:
        body = {"IPFIX": {"version": 10, "export_time": pkt.export_time.to_json(),
                          "sequence_number": pkt.sequence_number,
                          "observation_domain_id": pkt.observation_domain_id, "sets": sets}}
    return O.dumps(body)
