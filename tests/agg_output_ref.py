"""Python restatement of the Avro datum of one aggregated group (include/ngz/flow_agg_output.h): the
record AggFlowInfo::into_flowinfo_with_extra_fields builds (aggregator.rs:219-242, actor.rs:222-240,
as FlowAggregatorOracle.flowinfo lists it) run through output_ref's select / transform / default and
Avro writer, plus TimestampMillisString (config.rs:934-940).  Helper only: no test logic.
"""
import ipaddress

import ngz_agg_oracle as A
import ngz_oracle as O
import output_ref as R


def group_fields(oracle, g):
    """The group's fields as oracle Fields, in FlowAggregatorOracle.flowinfo's order."""
    reg, F = O.REGISTRY, O.Field
    refs = oracle.keys + [ref for ref, _op in oracle.vals]
    fields = [F(reg.lookup(p, i), A.to_field_value(reg.lookup(p, i), v))
              for (p, i, _x), v in zip(refs, g["key"] + g["vals"]) if v is not None]
    ms, we = g["max_coll"], g["window_start"] * 1000 + int(round(oracle.window_s * 1000))
    fields += [F(reg.lookup(0, 375), g["record_count"]), F(reg.lookup(0, 264), O.DateTime(g["min_export"], 0)),
               F(reg.lookup(0, 260), O.DateTime(g["max_export"], 0)),
               F(reg.lookup(0, 258), O.DateTime(ms // 1000, (ms % 1000) * 1_000_000)),
               F(reg.lookup(3746, 1), O.DateTime(g["window_start"], 0)),
               F(reg.lookup(3746, 2), O.DateTime(we // 1000, (we % 1000) * 1_000_000))]
    ip = ipaddress.ip_address(g["peer"])
    fields.append(F(reg.lookup(0, 403), ("v4", int(ip))) if ip.version == 4 else F(reg.lookup(0, 404), ("v6", int(ip))))
    fields += [F(reg.lookup(3746, 4), p) for p in sorted(g["ports"])]
    fields += [F(reg.lookup(0, 405), d) for d in sorted(g["domains"])]
    return fields + [F(reg.lookup(3746, 3), t) for t in sorted(t for _ft, t in g["templates"])]


def field_value(cfg, fmap):
    if cfg.get("transform") != "TimestampMillisString":
        return R.field_value(cfg, fmap)
    f = next((fmap[tuple(r)] for r in cfg["refs"] if tuple(r) in fmap), None)
    if f is not None:
        return "string", str(f.value.secs)  # ts.timestamp().to_string(): the whole seconds, floored
    return R.field_value(dict(cfg, transform="String", refs=[]), {})  # None, or the default


def datum(config, oracle, g):
    fmap, seen = {}, {}
    for f in group_fields(oracle, g):  # FieldRef::map_fields_into_fxhashmap (config.rs:194-213)
        key = (f.ie.pen, f.ie.id)
        fmap[key + (seen.get(key, 0),)] = f
        seen[key] = seen.get(key, 0) + 1
    return b"".join(R.w_field(field_value(c, fmap), c.get("default") is None) for c in config)
