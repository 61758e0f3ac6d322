"""The composition tests/agg_enrich_ref.py (enrichment restatement -> aggregation oracle) against
hand-worked cases (tests/agg_enrich_cases.py): what ngz_agg_push_enriched is checked against must
itself say what FieldRef::map_fields says over the enriched record (types.rs:82-100,
actor.rs:141-153, :176-187).  CPU only."""
import pytest

import agg_enrich_ref as AE
import enrich_ref as E
from agg_enrich_cases import ADD, CASES, KEY, OCT, cache_of

IP = "192.0.2.1"


def run(case, proto=10):
    tpl = case["template"]
    dgrams = [AE.template_msg(proto, [(300, tpl)]),
              AE.data_msg(proto, 300, [AE.record(tpl, r) for r in case["records"]], seq=1)]
    agg, _ = AE.aggregate(case["fields"], dgrams, cache_of(case), IP, "w")
    assert agg.late == 0
    return {g["key"]: (g["record_count"], g["vals"]) for g in agg.flush()}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("proto", [10, 9])
def test_hand_worked_case(name, proto):
    assert run(CASES[name], proto) == CASES[name]["groups"]


def test_options_only_message_leaves_event_time_and_late_count_alone():
    """Records with scope fields are removed before the aggregation (actor.rs:178, :237): a message
    holding only options records explodes to no item, so its export time, far ahead, neither closes a
    window nor makes the next data message late (aggregation.rs:124-172)."""
    tpl = [(10, 4), (OCT, 8)]
    dgrams = [AE.template_msg(10, [(300, tpl)]),
              AE.options_template_msg(400, [(302, 8)], [(34, 4)]),
              AE.data_msg(10, 300, [AE.record(tpl, (1, 10))], t=AE.T0 + 5),
              AE.data_msg(10, 400, [AE.record([(302, 8), (34, 4)], (7, 1000))], t=AE.T0 + 100_000),
              AE.data_msg(10, 300, [AE.record(tpl, (1, 20))], t=AE.T0 + 6)]
    fields = [(0, 10, 0, KEY), (0, OCT, 0, ADD)]
    agg, _ = AE.aggregate(fields, dgrams, E.Cache(), IP, "w")
    assert agg.late == 0 and agg.emit() == []
    assert agg.current_time[IP] == AE.T0 + 6
    groups = agg.flush()
    assert [(g["key"], g["record_count"], g["vals"], g["templates"], g["max_export"]) for g in groups] == \
        [((1,), 2, (30,), {(10, 300)}, AE.T0 + 6)]
    # the plain aggregation of the same datagrams does take the options record: an item without the
    # key, whose export time makes the last message late -- the difference the enriched push closes
    import ngz_agg_oracle as A
    plain = A.aggregate_datagrams(fields, dgrams, peer_ip=IP)
    assert plain.late == 1 and plain.current_time[IP] == AE.T0 + 100_000


def test_renormalized_counts_grouped_by_an_added_key():
    """With renormalize, the sums are the restatement's scaled counts (the added samplingInterval is
    the record's last sampling IE, logic.rs:327-341), grouped by the added VRF."""
    tpl = [(10, 4), (OCT, 8)]
    cache = E.Cache()
    AE.upsert(cache, IP, [AE.u(10, 1)], [AE.u(234, 7), AE.u(34, 100)])
    dgrams = [AE.template_msg(10, [(300, tpl)]),
              AE.data_msg(10, 300, [AE.record(tpl, r) for r in [(1, 3), (1, 4), (2, 5)]], seq=1)]
    fields = [(0, 234, 0, KEY), (0, OCT, 0, ADD)]
    agg, _ = AE.aggregate(fields, dgrams, cache, IP, "w", renormalize=True)
    assert {g["key"]: g["vals"] for g in agg.flush()} == {(7,): (700,), (None,): (5,)}
