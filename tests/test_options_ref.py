"""The restatement of the flow-options input (tests/options_ref.py) against the reference's own
test cases, transcribed as data (tests/golden/options_kats.json: every case of
inputs/flow_options/normalize/tests.rs and the three of handlers.rs:103-172).  Records are compared
as the reference compares them: IndexedDataRecords, i.e. the scope fields and the fields with
their occurrence indices."""
import json
import os
import struct

import pytest

import enrich_ref as E
import ngz_oracle as O
import options_ref as OR

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "options_kats.json")) as f:
    KATS = json.load(f)
NF9_SCOPES = {"System": 1, "Interface": 2, "LineCard": 3, "Cache": 4, "Template": 5}


def _names():
    out = {}
    for pen, top in ((0, 512), (OR.PEN_NETGAUZE, 32)):
        for i in range(1, top):
            try:
                ie = O.REGISTRY.lookup(pen, i)
            except O.ParseFail:  # an id the registry does not define
                continue
            if getattr(ie, "name", None):
                out[("NetGauze:" if pen else "") + ie.name] = (pen, i)
    return out


NAMES = _names()


def value(v):
    if isinstance(v, int):
        return E.K_UINT, int(v).to_bytes(8, "little")
    if "s" in v:
        return E.K_STR, v["s"].encode("utf-8")
    if "f" in v:
        return E.K_BYTES, struct.pack("<d", v["f"])
    return E.K_BYTES, bytes(v["b"])


def field(f):
    return NAMES[f[0]] + value(f[1])


def nf9_scope(f):
    name, v = f
    if name == "Unknown":
        return (v["id"], bytes(v["b"]), v["pen"])
    return (NF9_SCOPES[name], v if isinstance(v, int) else bytes(v["b"]), 0)


def indexed(scope, fields):
    """IndexedDataRecord: its two maps FieldRef -> Field."""
    return (dict(zip(E.index_fields(scope), scope)), dict(zip(E.index_fields(fields), fields)))


def canon32(fields):
    """A NetFlow v9 conversion yields u32 fields; the cases' integers are widened alike."""
    return [f[:3] + (f[3].ljust(8, b"\0"),) if f[2] == E.K_UINT else f for f in fields]


def test_the_fixture_holds_every_case():
    assert len(KATS["normalize"]) == 36 and len(KATS["handlers"]) == 3
    assert len({c["name"] for c in KATS["normalize"]}) == 36
    assert {NAMES["ingressInterface"], NAMES["selectorId"], NAMES["NetGauze:egressVRFname"]} == {(0, 10), (0, 302), (3746, 13)}


@pytest.mark.parametrize("case", KATS["normalize"], ids=lambda c: c["name"])
def test_normalize_case(case):
    netflow = case.get("netflow", False)
    scope = [nf9_scope(f) for f in case["scope"]] if netflow else [field(f) for f in case["scope"]]
    fields = [field(f) for f in case["fields"]]
    exp, check = case["expect"], case["check"]
    if check.startswith("is_"):
        assert bool(getattr(OR, check)(scope, fields)) is exp
        return
    try:
        if check == "try_from":
            got = OR.try_from(scope, fields, netflow)
        else:
            got = getattr(OR, check)(scope, fields)
    except OR.NoScopeFields:
        assert exp == {"error": "NoScopeFields"}
        return
    except OR.ConversionError as e:
        assert exp == {"error": "UnsupportedNetFlowV9ScopeFieldType", "scope_field": e.scope_field}
        return
    except OR.NormalizationError as e:
        assert exp == {"error": e.kind}
        return
    assert "error" not in exp, got
    if check == "try_from":
        if "class" in exp:
            klass, sc, fl = got
            assert klass == exp["class"]
            assert indexed(canon32(sc), fl) == indexed([field(f) for f in exp["scope"]], [field(f) for f in exp["fields"]])
        return
    want = [indexed([field(f) for f in r["scope"]], [field(f) for f in r["fields"]]) for r in exp["records"]]
    assert [indexed(sc, fl) for sc, fl in got] == want


@pytest.mark.parametrize("case", KATS["handlers"], ids=lambda c: c["name"])
def test_handler_case(case):
    ops = OR.handle([field(f) for f in case["scope"]], [field(f) for f in case["fields"]], case["ip"], case["obs_id"], case["weight"])
    exp = case["expect"]
    assert len(ops) == exp["n_ops"]
    assert all(op["op"] == "upsert" and op["ip"] == case["ip"] and op["weight"] == exp["weight"] and op["domain"] == exp["domain"]
               for op in ops)
