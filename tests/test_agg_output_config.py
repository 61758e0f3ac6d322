"""CPU, no device: the config side of include/ngz/flow_agg_output.h.  ngz_agg_output_create validates through
the column stage's code, so every refusal there is a refusal here with the same code; the one addition is
TimestampMillisString on the dateTime IEs (config.rs:371-385, :934-940), which ngz_output_create keeps refusing."""
import ctypes
import os
import re

import pytest

from netgauze_amd import _lib
from netgauze_amd.output import AggFlowOutput, FlowOutput, OutputError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, C = _lib.NGZ_OUTPUT_E_UNSUPPORTED, _lib.NGZ_OUTPUT_E_CONFIG


def f(name, *refs, **kw):
    return dict(name=name, refs=list(refs), **kw)


def code(cls, field):
    try:
        cls([field]).close()
        return 0
    except OutputError as e:
        return e.code


# (field, the column stage's code): flow_output.h's refusals, one of each kind
REFUSALS = [
    (f("a", (0, 6, 0)), U), (f("a", (0, 152, 0)), U), (f("a", (0, 1, 0), transform="Rename"), U),
    (f("a", (0, 320, 0), transform="String"), U), (f("a", (0, 264, 0), transform="String"), U), (f("a", (0, 9999, 0)), U),
    (f("a", (0, 1, 0), default=("StringArray", [])), U), (f("custom_primitives.x", (0, 1, 0)), U),
    (f("a", select="Coalesce"), C), (f("a", (0, 70, 0), select="Multi"), C), (f("a", (0, 1, 0), transform="MplsIndex"), C),
    (f("a", (0, 1, 0), (0, 82, 0), select="Coalesce"), C), (f("a", (0, 1, 0), select="Layer2SegmentId", encap=1), C),
    (f("a", (0, 313, 0), transform="String"), C), (f("a", (0, 1, 0), default=("String", "x")), C),
    (f("a", (0, 1, 0)), 0), (f("a", (0, 316, 0), (0, 71, 0), select="Multi", transform="MplsIndex"), 0),
]


@pytest.mark.parametrize("field,rc", REFUSALS, ids=lambda x: None if isinstance(x, int) else "%s-%s" % (x.get("transform", "Identity"), x["refs"][:1]))
def test_refusals_match_the_column_stage(field, rc):
    assert code(FlowOutput, field) == rc == code(AggFlowOutput, field)


@pytest.mark.parametrize("ie", [(0, 264), (0, 152), (0, 154), (0, 156), (3746, 1), (3746, 2)])
def test_timestamp_millis_string_on_datetimes_only(ie):
    ts = f("t", ie + (0,), transform="TimestampMillisString")
    assert code(AggFlowOutput, ts) == 0 and code(FlowOutput, ts) == U  # the column stage still refuses it
    assert code(AggFlowOutput, f("t", (0, 1, 0), transform="TimestampMillisString")) == C  # an integer IE
    assert code(AggFlowOutput, f("t", ie + (0,), (0, 1, 0), select="Coalesce", transform="TimestampMillisString")) == C
    assert code(AggFlowOutput, f("t", ie + (0,), select="Multi", transform="TimestampMillisString")) == C
    assert code(AggFlowOutput, dict(ts, default=("U32", 1))) == C and code(AggFlowOutput, dict(ts, default=("String", "0"))) == 0


def test_schema_text_and_abi():
    """get_record_schema's rules (config.rs:454-522): a nullable field is ["null", T], one with a default a bare
    T; TimestampMillisString gives a string.  The header's functions are the binding's, with the same arity."""
    cfg = [f("ws", (3746, 1, 0), transform="TimestampMillisString"), f("we", (3746, 2, 0), transform="TimestampMillisString", default=("String", "")),
           f("flows", (0, 375, 0)), f("labels", (0, 71, 0), select="Multi", transform="MplsIndex")]
    types = ['["null", "string"]', '"string"', '["null", "long"]', '["null", {"type": "array", "items": "string"}]']
    want = '{\n  "type": "record",\n  "name": "acct_data",\n  "fields": [\n' + ",\n".join(
        '    { "name": "%s", "type": %s }' % (c["name"], t) for c, t in zip(cfg, types)) + "\n  ]\n}"
    out = AggFlowOutput(cfg)
    assert out.schema() == want
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngz", "flow_agg_output.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2).count(",") + 1 if m.group(2).strip() not in ("", "void") else 0
            for m in re.finditer(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(ngz_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S)}
    lib = _lib.load()
    assert sorted(decl) == sorted(_lib.AGG_OUTPUT_FUNCTIONS) and all(len(getattr(lib, n).argtypes) == k for n, k in decl.items())
    assert lib.ngz_agg_output_abi_version() == _lib.NGZ_AGG_OUTPUT_ABI_VERSION == int(re.search(r"ABI_VERSION (\d+)", text).group(1))
    assert lib.ngz_agg_output_encode(out._h, None, None, 0, None, None) == _lib.NGZ_E_INVALID == lib.ngz_agg_output_result(out._h, None, None, None, None)
    assert lib.ngz_agg_output_last_launches(out._h) == 0 and ctypes.sizeof(_lib.AggOutputStats) == 24
