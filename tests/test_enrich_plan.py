"""CPU checks of ngz_enrich_template_plan (include/ngz/flow_enrich.h): the plan of one template
record for a peer, with no device."""
import ctypes
import struct

import pytest

import enrich_ref as E

PEER = "10.0.0.1"


def u(ie, v, w):
    return (0, ie, E.K_UINT, int(v).to_bytes(w, "little"))


def template(tid, fields):
    return struct.pack(">HH", tid, len(fields)) + b"".join(struct.pack(">HH", i, n) for i, n in fields)


@pytest.fixture()
def enricher():
    from netgauze_amd.enrich import FlowEnricher
    en = FlowEnricher(0, "w")
    en.upsert(PEER, 0, 64, [], [u(34, 100, 4)])                                   # unconditional
    en.upsert(PEER, 0, 64, [u(10, 5, 4)], [(0, 82, E.K_STR, b"eth5")])            # ingressInterface
    en.upsert(PEER, 1000, 64, [u(10, 5, 4), u(14, 6, 4)], [u(138, 7, 8)])         # ingress, egress
    en.upsert(PEER, 2000, 64, [u(10, 1, 4), u(10, 2, 4)], [(0, 84, E.K_STR, b"two")])  # a second occurrence
    en.upsert(PEER, 0, 64, [u(302, 1, 8)], [u(50, 9, 4)])                         # selectorId
    en.upsert(PEER, 0, 64, [u(7, 80, 2)], [u(35, 1, 1)])                          # sourceTransportPort
    yield en
    en.close()


def test_struct_size():
    from netgauze_amd import _lib
    assert ctypes.sizeof(_lib.EnrichRef) == 8
    assert ctypes.sizeof(_lib.EnrichPlan) == 4 + 8 + 8 * 4 * 8 + 32 * 8 + 32 + 32 * 2


@pytest.mark.parametrize("proto", [10, 9])
def test_plan_with_the_scope_ies(enricher, proto):
    p = enricher.template_plan(PEER, template(300, [(8, 4), (10, 4), (14, 4), (1, 8)]), proto)
    assert not p["dropped"] and p["launches"] == 1
    assert p["shapes"] == [[], [(0, 10, 0)], [(0, 10, 0), (0, 14, 0)]]
    assert p["columns"] == [(0, 34, 0, E.K_UINT, 4), (0, 82, 0, E.K_VLEN, 16), (0, 138, 0, E.K_UINT, 8)]


def test_plan_without_the_scope_ies_keeps_the_unconditional_scope(enricher):
    p = enricher.template_plan(PEER, template(301, [(4, 1), (1, 8), (2, 8)]))
    assert p == {"dropped": False, "launches": 1, "shapes": [[]], "columns": [(0, 34, 0, E.K_UINT, 4)]}
    # another peer has no scope at all: nothing to launch
    q = enricher.template_plan("10.0.0.2", template(301, [(4, 1), (1, 8), (2, 8)]))
    assert q == {"dropped": False, "launches": 0, "shapes": [], "columns": []}


def test_plan_with_a_second_occurrence_and_reduced_size_selector(enricher):
    p = enricher.template_plan(PEER, template(302, [(10, 4), (302, 4), (10, 2)]))  # selectorId on 4 wire bytes
    assert p["shapes"] == [[], [(0, 10, 0)], [(0, 10, 0), (0, 10, 1)], [(0, 302, 0)]]
    assert [c[:3] for c in p["columns"]] == [(0, 34, 0), (0, 50, 0), (0, 82, 0), (0, 84, 0)]


def test_plan_leaves_out_a_scope_on_a_column_of_another_kind_or_width(enricher):
    enricher.upsert(PEER, 0, 64, [u(10, 5, 2)], [u(306, 1, 4)])       # a 2-byte value for a 4-byte column
    enricher.upsert(PEER, 0, 64, [(0, 7, E.K_SINT, b"\x50\x00")], [u(309, 1, 4)])  # signed against unsigned
    p = enricher.template_plan(PEER, template(303, [(10, 4), (7, 2)]))
    assert p["shapes"] == [[], [(0, 7, 0)], [(0, 10, 0)]]
    assert [c[1] for c in p["columns"]] == [34, 35, 82]
    # a field length the decoder refuses for the IE gives no column to key on
    p = enricher.template_plan(PEER, template(304, [(10, 8), (7, 2)]))
    assert p["shapes"] == [[], [(0, 7, 0)]]


def test_plan_of_templates_with_scope_fields_is_dropped(enricher):
    ipfix = struct.pack(">HHH", 400, 3, 1) + struct.pack(">HH", 143, 4) + struct.pack(">HH", 10, 4) + struct.pack(">HH", 1, 8)
    p = enricher.template_plan(PEER, ipfix, 10, options=True)
    assert p == {"dropped": True, "launches": 0, "shapes": [], "columns": []}
    nf = struct.pack(">HHH", 400, 4, 8) + struct.pack(">HH", 1, 4) + struct.pack(">HH", 10, 4) + struct.pack(">HH", 34, 4)
    assert enricher.template_plan(PEER, nf, 9, options=True)["dropped"]


def test_plan_refusals(enricher):
    from netgauze_amd import _lib
    from netgauze_amd.enrich import EnrichError
    t = template(300, [(10, 4), (14, 4)])
    with pytest.raises(EnrichError):
        enricher.template_plan(PEER, t[:-2])
    with pytest.raises(EnrichError):
        enricher.template_plan(PEER, t, 5)
    for i in range(33):
        enricher.upsert(PEER, 0, 1, [], [u(34, i, 4)] * (i + 1))
    with pytest.raises(EnrichError) as ei:
        enricher.template_plan(PEER, t)
    assert ei.value.code == _lib.NGZ_E_LIMIT
