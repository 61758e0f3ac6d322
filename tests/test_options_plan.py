"""ngz_options_template_plan (include/ngz/flow_options.h, no device) against the restatement's plan
(tests/options_ref.py): class, template-level outcome, the id-equality flag and, per operation, the
(pen, ie_id, index) lists with the template fields their values come from."""
import struct

import pytest

import golden_io
import options_ref as OR
import parity


def spec(ies):
    return b"".join(struct.pack(">HH", ie | (0x8000 if pen else 0), 4) + (struct.pack(">I", pen) if pen else b"")
                    for pen, ie in ies)


def ipfix_options(scope, fields, tid=256):
    return struct.pack(">HHH", tid, len(scope) + len(fields), len(scope)) + spec(scope + fields)


def nf9_options(scope, fields, tid=256):
    return struct.pack(">HHH", tid, len(spec(scope)), len(spec(fields))) + spec(scope + fields)


def iana(*ies):
    return [(0, i) for i in ies]


def both(scope, fields, proto=10):
    from netgauze_amd.options import template_plan
    rec = ipfix_options(scope, fields) if proto == 10 else nf9_options(scope, fields)
    got, ref = template_plan(rec, proto), OR.plan(scope, fields, proto)
    assert got == ref, (scope, fields, got, ref)
    return got


SHAPES = [
    (iana(302), iana(34)), (iana(138), iana(50)), (iana(302), iana(305, 306)), (iana(302), iana(305)),
    (iana(302), iana(307, 308)), (iana(302), iana(309, 310)), (iana(302), iana(311)), (iana(302), iana(82)),
    (iana(302), iana(34, 210)), (iana(302, 144, 210), iana(34, 210, 84)),             # padding / exportingProcessId
    (iana(10, 14), iana(82)), (iana(10, 14), iana(82, 83)), (iana(10), iana(82)), (iana(14), iana(83)),
    (iana(10, 14, 141, 144, 210), iana(82, 83, 1)),                                  # extra scope carried into both halves
    (iana(10, 82), iana(1)), (iana(10, 14, 83), iana(2)),                            # the name only in the scope
    (iana(302), iana(10, 14, 82)), (iana(302, 14), iana(10, 83)),                    # ids among the non-scope fields
    (iana(234, 235), iana(236)), (iana(234), iana(236, 90)), (iana(235), iana(90)), (iana(234, 236), iana(1)),
    (iana(234, 235, 143), iana(236, 90)), (iana(302), iana(1)), (iana(302), iana(210)), (iana(302), []),
    (iana(10, 10, 14), iana(82, 82, 83)), (iana(302, 302, 143, 302), iana(34, 34, 1, 34)),  # repeated IEs
    (iana(10, 14), iana(34, 82)),                                                    # sampling wins over interface
    ([(9, 10)], [(9, 82)]), ([(0, 10)], [(3746, 8), (0, 82)]),                       # vendor IEs are not the IANA ones
]


@pytest.mark.parametrize("scope,fields", SHAPES)
def test_ipfix_shapes(scope, fields):
    both(scope, fields)


def test_outcomes_of_the_shapes():
    assert both(iana(302), iana(34)) == {"class": "sampling", "outcome": "ops", "id_equal": False, "ops": [
        {"scope": [(0, 302, 0)], "fields": [(0, 34, 0)], "scope_src": [0], "fields_src": [1]}]}
    p = both(iana(10, 14, 141, 144, 210), iana(82, 83, 1))
    assert p["class"] == "interface" and p["id_equal"] and [o["scope"] for o in p["ops"]] == [
        [(0, 10, 0), (0, 141, 0)], [(0, 14, 0), (0, 141, 0)]]
    assert [o["fields"] for o in p["ops"]] == [[(3746, 8, 0), (3746, 10, 0)], [(3746, 9, 0), (3746, 11, 0)]]
    assert both(iana(10, 82), iana(1))["outcome"] == "missing_required_fields"
    assert both(iana(302), iana(210)) == {"class": "unclassified", "outcome": "ops", "id_equal": False, "ops": []}
    p = both(iana(302, 302, 143, 302), iana(34, 34, 1, 34))
    assert p["ops"][0]["scope"] == [(0, 302, 0), (0, 302, 1), (0, 143, 0), (0, 302, 2)]
    assert p["ops"][0]["fields"] == [(0, 34, 0), (0, 34, 1), (0, 1, 0), (0, 34, 2)]
    p = both(iana(234, 235), iana(236, 90))
    assert [o["fields"] for o in p["ops"]] == [[(3746, 12, 0), (3746, 14, 0)], [(3746, 13, 0), (3746, 15, 0)]]


@pytest.mark.parametrize("code", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("fields", [iana(34), iana(82), iana(1)])
def test_netflow_v9_scope_codes(code, fields):
    p = both(iana(code), fields, proto=9)
    assert (p["outcome"] == "conversion_error") == (code not in (1, 2, 3))
    if code == 2 and fields == iana(82):  # one column read twice: no equality test
        assert not p["id_equal"] and [o["scope"] for o in p["ops"]] == [[(0, 10, 0)], [(0, 14, 0)]]
    if code == 1 and fields == iana(34):
        assert p["ops"][0]["scope"] == []
    both(iana(1, code), fields, proto=9)
    both(iana(code, 2, 3), fields, proto=9)


def test_a_template_without_scope_fields_and_bad_records():
    from netgauze_amd import _lib
    from netgauze_amd.options import OptionsError, template_plan
    rec = struct.pack(">HH", 300, 2) + spec(iana(302, 34))
    assert template_plan(rec, 10, options=False) == {"class": "none", "outcome": "not_options", "id_equal": False, "ops": []}
    for bad in (b"", b"\1\0\0", ipfix_options(iana(302), iana(34))[:-1], struct.pack(">HHH", 256, 1, 2) + spec(iana(302))):
        with pytest.raises(OptionsError) as e:
            template_plan(bad, 10)
        assert e.value.code == _lib.NGZ_E_INVALID
    with pytest.raises(OptionsError) as e:
        template_plan(ipfix_options(iana(*range(400, 425)), iana(34)), 10)
    assert e.value.code == _lib.NGZ_E_LIMIT


def golden_options_templates():
    out = []
    for name, _kind, _n in golden_io.cases():
        peers = {}
        for src, sp, _dst, _dp, payload in golden_io.datagrams(name):
            peers.setdefault((src, sp), []).append(payload)
        for dgrams in peers.values():
            _res, codec = parity.oracle_datagrams(dgrams)
            for proto, tmap in ((10, codec.ipfix_templates), (9, codec.netflow_templates)):
                for t in tmap.values():
                    if t.scope:
                        out.append((proto, tuple((s.ie.pen, s.ie.id) for s in t.scope), tuple((f.ie.pen, f.ie.id) for f in t.fields)))
    return sorted(set(out))


def test_every_options_template_of_the_goldens():
    found = golden_options_templates()
    assert found, "the goldens hold no options template"
    for proto, scope, fields in found:
        both(list(scope), list(fields), proto)
