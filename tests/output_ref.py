"""Python restatement of the reference collector's flow output for the subset include/ngz/flow_output.h
accepts (crates/collector/src/flow/config.rs:105-145, 532-543, 576-763, 888-996; flow/mod.rs:78-183):
per record a dict FieldRef -> the oracle's Field, then select, transform and default, then the Avro
binary writer.  A config field is the dict netgauze_amd.output.FlowOutput takes.
"""
import struct

import ngz_oracle as O

INTS = ("unsigned8", "unsigned16", "unsigned32", "unsigned64", "signed8", "signed16", "signed32", "signed64")
DEFAULT_KINDS = {"Bytes": "bytes", "F32": "float", "F64": "double", "Boolean": "boolean", "String": "string"}


def w_long(v):
    """Avro long / int: the zigzag varint of a signed 64-bit value."""
    z = ((v << 1) ^ (v >> 63)) & ((1 << 64) - 1)
    out = bytearray()
    while z >= 0x80:
        out.append((z & 0x7F) | 0x80)
        z >>= 7
    out.append(z)
    return bytes(out)


def w_value(kind, v):
    if kind == "long":
        return w_long(v)
    if kind == "float":
        return struct.pack("<I", v)  # the IEEE bits
    if kind == "double":
        return struct.pack("<Q", v)
    if kind == "boolean":
        return bytes([1 if v else 0])
    if kind == "string":
        v = v.encode("utf-8")
    if kind in ("string", "bytes"):
        return w_long(len(v)) + bytes(v)
    assert kind == "array"
    return (w_long(len(v)) + b"".join(w_value("string", s) for s in v) if v else b"") + w_long(0)


def w_field(value, nullable):
    """A nullable field is the union ["null", T]; `value` is (kind, v) or None."""
    if value is None:
        assert nullable
        return w_long(0)
    return (w_long(1) if nullable else b"") + w_value(*value)


def _text(dt, v):
    if dt == "macAddress":
        return ":".join("%02x" % b for b in v)
    if dt == "ipv4Address":
        return O._ipv4_str(v[1])
    if dt == "ipv6Address":
        return O.ipv6_str(v[1])
    return v


def raw_value(f):
    """From<ie::Field> for RawValue (flow/mod.rs:133-183) and into_avro_value (:78-103)."""
    dt, v = f.ie.dtype, f.value
    if dt in INTS:
        return "long", v - (1 << 64) if v >= 1 << 63 else v  # a u64 goes out `as i64`
    if dt in ("float32", "float64"):
        return ("float" if dt == "float32" else "double"), v[1]
    if dt == "boolean":
        return "boolean", v
    if dt in ("string", "macAddress", "ipv4Address", "ipv6Address"):
        return "string", _text(dt, v)
    return "bytes", bytes(v)


def string_value(f):
    """TryInto<String> for Field (generator.rs:2637-2651) of the accepted IEs."""
    dt, v = f.ie.dtype, f.value
    if dt in INTS:
        return "string", str(v)
    if dt == "boolean":
        return "string", "true" if v else "false"
    return "string", _text(dt, v)


def field_value(cfg, fmap):
    """FieldConfig::avro_value (config.rs:532-543): (kind, value) or None."""
    sel, refs, tr = cfg.get("select", "Single"), [tuple(r) for r in cfg["refs"]], cfg.get("transform", "Identity")
    if sel == "Layer2SegmentId":
        encap = cfg["encap"]
        code, mask = (encap[1], 0xFFFFFFFFFF) if isinstance(encap, tuple) else (encap, 0xFFFFFF if encap in (1, 2) else 0xFFFFFFFFFF)
        f = fmap.get(refs[0])
        picked = [O.Field(f.ie, f.value & mask)] if f is not None and f.value >> 56 == code else None
    elif sel == "Multi":
        picked = [fmap[r] for r in refs if r in fmap] or None
    else:  # Single, Coalesce: the first present
        picked = next(([fmap[r]] for r in refs if r in fmap), None)
    if picked is None:
        value = None
    elif tr == "MplsIndex":
        n = lambda ie: 1 if ie.id == 316 else ie.id - 69  # noqa: E731
        value = "array", ["%d-%d" % (n(f.ie), int.from_bytes(f.value, "big")) for f in picked]
    else:
        value = raw_value(picked[-1]) if tr == "Identity" else string_value(picked[-1])
    if value is None and cfg.get("default") is not None:
        kind, v = cfg["default"]
        if kind in ("F32", "F64"):
            v = struct.unpack("<I", struct.pack("<f", v))[0] if kind == "F32" else struct.unpack("<Q", struct.pack("<d", v))[0]
        if kind == "U64" and v >= 1 << 63:
            v -= 1 << 64
        value = DEFAULT_KINDS.get(kind, "long"), v
    return value


def datum(config, fields):
    """get_avro_value_from_fields (config.rs:105-145) of one record's non-scope fields, encoded."""
    fmap, seen = {}, {}
    for f in fields:  # FieldRef::map_fields_into_fxhashmap (:194-213)
        key = (f.ie.pen, f.ie.id)
        fmap[key + (seen.get(key, 0),)] = f
        seen[key] = seen.get(key, 0) + 1
    return b"".join(w_field(field_value(c, fmap), c.get("default") is None) for c in config)


def encode_batch(config, batch, oracle):
    """Per batch slot the datums of its rows in stream order, b"" for rows of failed messages:
    `oracle` is parity.oracle_datagrams' list, laid out by the product batch's sets."""
    rows = [[b""] * int(sl.n_records) for sl in batch.slots]
    by_dg = {}
    for gs in batch.sets():
        by_dg.setdefault(int(gs["dgram"]), []).append(gs)
    for d, (kind, pkt) in enumerate(oracle):
        if kind != "ok":
            continue
        for (_, _sid, recs), gs in zip([s for s in pkt.sets if s[0] == "Data"], by_dg.get(d, [])):
            for i, (_scope, fields) in enumerate(recs):
                rows[int(gs["slot"])][int(gs["rec0"]) + i] = datum(config, fields)
    return rows
