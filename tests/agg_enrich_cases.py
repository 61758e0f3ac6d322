"""Hand-worked cases of the aggregation over enriched records, as data: shared by the composition's
own test (tests/test_agg_enrich_ref.py), the plan entry's (tests/test_agg_enrich_plan.py) and the
device tests.

A case: the template's fields [(ie, length)], the cache as {scope: {(pen, ie, cache index): value}}
(written as state, not as operations: no operation sequence leaves a scope with (X, 1) but without
(X, 0) -- an upsert that brings index 1 brings index 0 at the same weight, and a delete that removes
index 0 removes the lighter index 1 too -- yet FieldRef::map_fields is defined for such a record), the
records, the aggregation fields (pen, ie, index, op), and the expected groups
{key: (record_count, values)}.  Writer id "w", peer 192.0.2.1, all records in one window.
"""
import enrich_ref as E
from agg_enrich_ref import s, u

IN, EG, OCT, VRF, NAME = 10, 14, 1, 234, 82  # ingressInterface, egressInterface, octetDeltaCount, ingressVRFID, interfaceName
KEY, ADD = 0, 1

CASES = {
    "added_ie_the_template_lacks": dict(
        template=[(IN, 4), (OCT, 8)],
        cache={(u(IN, 1),): {(0, VRF, 0): u(VRF, 7)}},
        records=[(1, 100), (2, 50), (1, 5)],
        fields=[(0, VRF, 0, KEY), (0, OCT, 0, ADD)],
        groups={(7,): (2, (105,)), (None,): (1, (50,))}),
    "own_at_0_added_at_1": dict(
        template=[(IN, 4), (VRF, 4), (OCT, 8)],
        cache={(u(IN, 1),): {(0, VRF, 0): u(VRF, 9)}},
        records=[(1, 3, 10), (2, 3, 20), (1, 4, 1)],
        fields=[(0, VRF, 0, KEY), (0, VRF, 1, KEY), (0, OCT, 0, ADD)],
        groups={(3, 9): (1, (10,)), (3, None): (1, (20,)), (4, 9): (1, (1,))}),
    "lone_cache_field_index_1_is_ordinal_0": dict(
        template=[(IN, 4), (OCT, 8)],
        cache={(u(IN, 1),): {(0, NAME, 1): s(NAME, "eth1")}},
        records=[(1, 10), (2, 20)],
        fields=[(0, NAME, 0, KEY), (0, NAME, 1, KEY), (0, OCT, 0, ADD)],
        groups={("eth1", None): (1, (10,)), (None, None): (1, (20,))}),
    "two_added_of_one_ie_only_the_second_present": dict(
        template=[(IN, 4), (EG, 4), (OCT, 8)],
        cache={(u(IN, 1),): {(0, NAME, 0): s(NAME, "a0")}, (u(EG, 2),): {(0, NAME, 1): s(NAME, "b1")}},
        records=[(1, 2, 1), (9, 2, 2), (1, 9, 4), (9, 9, 8)],
        fields=[(0, NAME, 0, KEY), (0, NAME, 1, KEY), (0, OCT, 0, ADD)],
        groups={("a0", "b1"): (1, (1,)), ("b1", None): (1, (2,)), ("a0", None): (1, (4,)), (None, None): (1, (8,))}),
    "writer_id_as_a_key": dict(
        template=[(IN, 4), (OCT, 8)],
        cache={(u(IN, 1),): {(0, VRF, 0): u(VRF, 7)}},
        records=[(1, 100), (2, 50)],
        fields=[(3746, 7, 0, KEY), (3746, 7, 1, KEY), (0, OCT, 0, ADD)],
        groups={("w", None): (2, (150,))}),
}


def cache_of(case, ip="192.0.2.1"):
    """The case's cache state in the restatement's Cache."""
    c = E.Cache()
    c.peers[ip] = {"global": {E.Cache.scope_key(list(scope)): {ref: (64, f[2], bytes(f[3])) for ref, f in added.items()}
                              for scope, added in case["cache"].items()}, "domains": {}}
    return c


def plan_inputs(case):
    """(template fields [(pen, ie, is_scope)], added columns [(pen, ie, index)] ascending) of the case's slot."""
    cols = sorted({ref for added in case["cache"].values() for ref in added})
    return [(0, ie, 0) for ie, _n in case["template"]], cols
