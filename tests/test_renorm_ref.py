"""The Python restatement of the reference's flow renormalization (tests/renorm_ref.py) reproduces
every known-answer case of the reference's own unit tests (tests/golden/renorm_kats.json, the cases
of crates/collector/src/flow/renormalization/logic/tests.rs as data) and the derived edge cases."""
import json
import os

import pytest

import ngz_oracle as O
import renorm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "renorm_kats.json")) as f:
    KATS = json.load(f)
NAME = KATS["ie_ids"]


def value_of(v):
    return R.f64_from_bits(int(v["f64_bits"], 16)) if isinstance(v, dict) else v


def pairs_of(fields):
    return [(NAME[n], value_of(v)) for n, v in fields if n != "isRenormalized"]


def run_fields(inp):
    st = R.new_stats()
    k, new, flagged = R.renormalize_pairs(pairs_of(inp), st)
    got = [[n, v if isinstance(v, dict) else nv] for (n, v), (_, nv) in zip(inp, new)]
    if flagged:
        got.append(["isRenormalized", True])
    return k, got, st


@pytest.mark.parametrize("case", KATS["kats"], ids=lambda c: c["name"])
def test_reference_kat(case):
    _k, got, _st = run_fields(case["input"])
    assert got == case["expected"]


@pytest.mark.parametrize("case", KATS["edges"], ids=lambda c: c["name"])
def test_edge(case):
    assert case["derived"] is True
    k, got, st = run_fields(case["input"])
    assert got == case["expected"]
    assert (None if k is None else "0x%016x" % R.f64_bits(k)) == case["k_bits"]
    assert {x: st[x] for x in case["stats"]} == case["stats"]


def test_edge_table_is_complete():
    names = {c["name"] for c in KATS["edges"]}
    assert len(KATS["kats"]) + len(KATS["packets"]) >= 24 and len(names) >= 16
    by = {c["name"]: c for c in KATS["edges"]}
    # the values the edge table pins, worked out by hand from the arithmetic's definition
    assert by["count_2p53_plus_1_k1"]["expected"][0][1] == 1 << 53  # ties to even
    assert by["count_u64_max_k1_saturates"]["expected"][0][1] == (1 << 64) - 1
    assert by["count_2p63_k4_saturates"]["expected"][0][1] == (1 << 64) - 1
    assert by["k_4_thirds_truncates"]["expected"][:2] == [["octetDeltaCount", 133], ["packetDeltaCount", 9]]
    assert by["k_10_thirds_truncates"]["expected"][:2] == [["octetDeltaCount", 333], ["packetDeltaCount", 23]]
    assert by["probability_min_subnormal_count_0"]["expected"][0][1] == 0  # 0 * inf = NaN -> 0
    assert by["probability_min_subnormal_count_1"]["expected"][0][1] == (1 << 64) - 1
    for n in ("probability_negative_zero", "probability_zero", "probability_nan", "probability_next_after_one"):
        assert by[n]["k_bits"] is None and by[n]["stats"]["ie_missing_or_invalid"] == 1
    assert by["sampler_random_interval_zero_mode_1"]["k_bits"] == "0x0000000000000000"
    assert by["factor_without_count_field_no_flag"]["expected"][-1][0] != "isRenormalized"


def ie(name):
    return next(x for x in O.REGISTRY.by_key.values() if x.pen == 0 and x.name == name)


def build_packet(case):
    sets = []
    for s in case["sets"]:
        if s["kind"] != "Data":
            sets.append((s["kind"], 2 if s["kind"] == "Template" else 3, []))
            continue
        recs = [([], [O.Field(ie(n), v) for n, v in r["fields"]]) for r in s["records"]]
        sets.append(("Data", s["id"], recs))
    t = O.timestamp_opt(1735725600, 0)  # 2025-01-01T10:00:00Z
    assert t.to_json() == case.get("export_time", case.get("unix_time"))
    if case["proto"] == "IPFIX":
        return O.IpfixPacket(t, case["sequence_number"], case["observation_domain_id"], sets)
    return O.NetFlowV9Packet(case["sys_up_time"], t, case["sequence_number"], case["source_id"], sets)


@pytest.mark.parametrize("case", KATS["packets"], ids=lambda c: c["name"])
def test_reference_packet_kat(case):
    pkt = build_packet(case)
    st = R.new_stats()
    flags = R.renormalize_packet(pkt, st)
    got = json.loads(R.packet_json(pkt, flags))
    body = got["IPFIX" if case["proto"] == "IPFIX" else "NetFlowV9"]
    exp = [{"Data": {"id": s["id"], "records": [
        {"scope_fields": [], "fields": [{"NetGauze": {n: v}} if n == "isRenormalized" else {n: v} for n, v in r["fields"]]}
        for r in s["records"]]}} for s in case["expected_sets"]]
    assert body["sets"] == exp
    assert body["sequence_number"] == case["sequence_number"]


def test_records_with_scope_fields_are_dropped():
    pkt = O.IpfixPacket(O.timestamp_opt(0, 0), 0, 0, [("Data", 300, [
        ([O.Field(ie("samplingInterval"), 9)], [O.Field(ie("octetDeltaCount"), 5), O.Field(ie("samplingInterval"), 2)]),
        ([], [O.Field(ie("octetDeltaCount"), 5), O.Field(ie("samplingInterval"), 2)])])])
    st = R.new_stats()
    flags = R.renormalize_packet(pkt, st)
    assert st == dict(flows_processed=1, flows_renormalized=1, ie_missing_or_invalid=0, sampling_algorithm_inferred=1,
                      records_dropped=1)
    assert flags == {(0, 1): True}
    assert pkt.sets[0][2][0][1][0].value == 5 and pkt.sets[0][2][1][1][0].value == 10
    assert R.packet_json(pkt, flags).count('"scope_fields"') == 1
