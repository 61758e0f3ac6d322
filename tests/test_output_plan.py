"""CPU, no device: the flow output's config checks, schema text and per-template plan
(include/ngz/flow_output.h) against FieldConfig::validate, get_avro_schema and the FieldRef map of
crates/collector/src/flow/config.rs."""
import json
import os
import struct

import pytest

from netgauze_amd import _lib
from netgauze_amd.output import FlowOutput, OutputError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "output", "schema_fragments.json")
UNSUPPORTED, CONFIG = _lib.NGZ_OUTPUT_E_UNSUPPORTED, _lib.NGZ_OUTPUT_E_CONFIG
one = lambda ie, **kw: dict({"name": "f", "refs": [(0, ie, 0)]}, **kw)  # noqa: E731

REFUSED = [
    # Identity where From<Field> for RawValue is the String fallback
    (one(4), UNSUPPORTED), (one(6), UNSUPPORTED), (one(70), UNSUPPORTED), (one(150), UNSUPPORTED), (one(152), UNSUPPORTED),
    (one(154), UNSUPPORTED), (one(156), UNSUPPORTED),
    # String where the Display text is not pinned
    (one(311, transform="String"), UNSUPPORTED), (one(152, transform="String"), UNSUPPORTED), (one(4, transform="String"), UNSUPPORTED),
    (one(6, transform="String"), UNSUPPORTED), (one(90, transform="String"), UNSUPPORTED),
    # transforms, names, defaults and IEs outside the subset
    *[(one(1, transform=t), UNSUPPORTED) for t in ("TrimmedString", "LowercaseString", "TimestampMillisString", "Rename",
                                                    "StringArray", "StringArrayAgg", "StringMapAgg")],
    (one(1, name="custom_primitives.x", transform="String"), UNSUPPORTED), (one(1, default=("TimestampMillis", 1)), UNSUPPORTED),
    (one(1, default=("StringArray", [])), UNSUPPORTED), (one(1, default=("StringMap", {})), UNSUPPORTED),
    ({"name": "f", "refs": [(9, 9, 0)]}, UNSUPPORTED),
    # what FieldConfig::validate rejects
    ({"name": "f", "select": "Coalesce", "refs": []}, CONFIG), ({"name": "f", "select": "Multi", "refs": [], "transform": "MplsIndex"}, CONFIG),
    ({"name": "f", "select": "Multi", "refs": [(0, 71, 0)], "transform": "String"}, CONFIG), (one(71, transform="MplsIndex"), CONFIG),
    ({"name": "f", "select": "Multi", "refs": [(0, 70, 0)], "transform": "MplsIndex"}, CONFIG),
    ({"name": "f", "select": "Coalesce", "refs": [(0, 1, 0), (0, 8, 0)]}, CONFIG),
    (one(1, select="Layer2SegmentId", encap=1), CONFIG), (one(313, transform="String"), CONFIG), (one(71, transform="String"), CONFIG),
    (one(1, default=("U16", 1)), CONFIG), (one(8, default=("U32", 1)), CONFIG),
]


@pytest.mark.parametrize("field,code", REFUSED, ids=lambda v: None if isinstance(v, int) else
                         "%s-%s-%s" % (v["refs"][:1], v.get("transform"), (v.get("default") or [v.get("select")])[0]))
def test_refused_configs_name_the_field(field, code):
    with pytest.raises(OutputError) as e:
        FlowOutput([{"name": "ok", "refs": [(0, 1, 0)]}, field])
    assert e.value.code == code and ("Invalid FieldConfig for %s, reason: " % field["name"]) in str(e.value)


CONFIG_OK = [
    {"name": "src_ip", "refs": [(0, 8, 0)]},
    {"name": "dst_ip", "refs": [(0, 12, 0)], "default": ("String", "0.0.0.0")},
    {"name": "mpls", "select": "Multi", "refs": [(0, 316, 0), (0, 71, 0), (0, 72, 0)], "transform": "MplsIndex"},
    {"name": "Bytes2", "refs": [(0, 1, 1)], "default": ("U64", 0)},
    {"name": "port", "select": "Coalesce", "refs": [(0, 11, 0), (0, 7, 0)]},
    {"name": "vni", "select": "Layer2SegmentId", "refs": [(0, 351, 0)], "encap": 1, "transform": "String"},
    {"name": "f64", "refs": [(0, 320, 0)]}, {"name": "ok", "refs": [(0, 276, 0)]}, {"name": "raw", "refs": [(0, 313, 0)]},
]


def test_schema_text_is_get_avro_schema():
    schema = FlowOutput(CONFIG_OK).schema
    typ = ['["null", "string"]', '"string"', '["null", {"type": "array", "items": "string"}]', '"long"', '["null", "int"]',
           '["null", "string"]', '["null", "double"]', '["null", "boolean"]', '["null", "bytes"]']
    want = "{\n  \"type\": \"record\",\n  \"name\": \"acct_data\",\n  \"fields\": [\n" + ",\n".join(
        '    { "name": "%s", "type": %s }' % (c["name"], t) for c, t in zip(CONFIG_OK, typ)) + "\n  ]\n}"
    assert schema == want and json.loads(schema)["fields"][3]["name"] == "Bytes2"
    for frag in json.load(open(GOLDEN))["fragments"]:  # what the reference's own test expects of these fields
        assert frag in schema, frag


def spec(fields):
    return b"".join(struct.pack(">HH", ie, n) for ie, n in fields)


@pytest.mark.parametrize("tmpl,options,want", [
    # a repeated IE: the second octetDeltaCount is index 1; Coalesce takes 7 for the absent 11; 72 absent from the Multi
    (struct.pack(">HH", 300, 6) + spec([(1, 8), (7, 2), (71, 3), (1, 8), (316, 3), (8, 4)]), False,
     [[5], [], [4, 2], [3], [1], [], [], [], []]),
    # scope fields are no FieldRefs: the scope's octetDeltaCount and sourceIPv4Address do not count
    (struct.pack(">HHH", 301, 5, 2) + spec([(1, 8), (8, 4), (1, 8), (351, 8), (12, 4)]), True,
     [[], [4], [], [], [], [3], [], [], []]),
])
def test_template_plan(tmpl, options, want):
    plan = FlowOutput(CONFIG_OK).template_plan(tmpl, 10, options)
    assert [p["src"] for p in plan] == want
    assert [p["nullable"] for p in plan] == [c.get("default") is None for c in CONFIG_OK]
    assert [p["type"] for p in plan] == ["string", "string", "array", "long", "int", "string", "double", "boolean", "bytes"]
    with pytest.raises(OutputError):
        FlowOutput(CONFIG_OK).template_plan(tmpl[:-1], 10, options)
