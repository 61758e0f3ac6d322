"""ngz_agg_enrich_field_plan (include/ngz/flow_aggregate.h; netgauze_amd/csrc/ngz_agg_enrich_plan.cpp),
the host-only plan of ngz_agg_push_enriched, against the hand-worked cases: no device.  The plan says
per slot what the composition says per record: for every row mask the plan's resolution picks the
field FieldRef::map_fields picks (types.rs:82-100)."""
import ctypes
import itertools

import pytest

from agg_enrich_cases import CASES, KEY, plan_inputs
from netgauze_amd import _lib
from netgauze_amd.aggregate import enrich_field_plan

WRITER = (3746, 7)


def expect(fields, cols, ref):
    """The resolution restated: occurrence index over own fields, then the added columns, then the writer id."""
    if any(sc for _p, _i, sc in fields):
        return dict(kind=_lib.NGZ_AGG_RES_NONE, dropped=True)
    own = [i for i, (p, ie, _sc) in enumerate(fields) if (p, ie) == ref[:2]]
    if ref[2] < len(own):
        return dict(kind=_lib.NGZ_AGG_RES_OWN, dropped=False, own_field=own[ref[2]])
    cand = [c for c, (p, ie, _x) in enumerate(cols) if (p, ie) == ref[:2]]
    j, writer = ref[2] - len(own), ref[:2] == WRITER
    if j >= len(cand) + writer:
        return dict(kind=_lib.NGZ_AGG_RES_NONE, dropped=False)
    if not cand:
        return dict(kind=_lib.NGZ_AGG_RES_WRITER, dropped=False)
    return dict(kind=_lib.NGZ_AGG_RES_ADDED, dropped=False, candidates=cand, ordinal=j, writer_after=writer)


def pick(res, mask):
    """What a row with presence `mask` gets under a resolution: ("own", i) / ("col", c) / "writer" / None."""
    if res["kind"] == _lib.NGZ_AGG_RES_OWN:
        return ("own", res["own_field"])
    if res["kind"] == _lib.NGZ_AGG_RES_WRITER:
        return "writer"
    if res["kind"] == _lib.NGZ_AGG_RES_ADDED:
        present = [c for c in res["candidates"] if (mask >> c) & 1]
        if res["ordinal"] < len(present):
            return ("col", present[res["ordinal"]])
        if res["writer_after"] and res["ordinal"] == len(present):
            return "writer"
    return None


def map_fields_pick(fields, cols, ref, mask):
    """FieldRef::map_fields over own fields + present added columns + the writer id."""
    rec = [(("own", i), (p, ie)) for i, (p, ie, _sc) in enumerate(fields)]
    rec += [(("col", c), (p, ie)) for c, (p, ie, _x) in enumerate(cols) if (mask >> c) & 1]
    rec.append(("writer", WRITER))
    seen = 0
    for what, ie in rec:
        if ie == ref[:2]:
            if seen == ref[2]:
                return what
            seen += 1
    return None


def test_symbols_exist_with_their_signatures():
    lib = _lib.load()
    assert lib.ngz_agg_push_enriched.argtypes[:3] == [ctypes.c_void_p] * 3 and len(lib.ngz_agg_push_enriched.argtypes) == 8
    assert len(lib.ngz_agg_enrich_field_plan.argtypes) == 8
    assert ctypes.sizeof(_lib.AggEnrichResolution) == 44 and ctypes.sizeof(_lib.AggSlotField) == 8
    assert lib.ngz_agg_enrich_field_plan(None, 0, None, 0, 0, 1, 0, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_agg_push_enriched(None, None, None, None, None, 0, None, None) == _lib.NGZ_E_INVALID


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_of_the_hand_worked_cases(name):
    fields, cols = plan_inputs(CASES[name])
    for pen, ie, index, _op in CASES[name]["fields"]:
        got = enrich_field_plan(fields, cols, (pen, ie, index))
        want = expect(fields, cols, (pen, ie, index))
        assert {k: got[k] for k in want} == want, (name, (pen, ie, index), got)
        for mask in range(1 << len(cols)):
            assert pick(got, mask) == map_fields_pick(fields, cols, (pen, ie, index), mask), (name, index, mask)


def test_plan_by_hand():
    f2 = [(0, 10, 0), (0, 82, 0), (0, 1, 0)]
    cols = [(0, 82, 0), (0, 82, 3), (0, 234, 1), (3746, 7, 0)]
    assert enrich_field_plan(f2, cols, (0, 82, 0))["kind"] == _lib.NGZ_AGG_RES_OWN
    r = enrich_field_plan(f2, cols, (0, 82, 2))  # own at 0, then the second present of columns 0 and 1
    assert (r["kind"], r["candidates"], r["ordinal"], r["writer_after"]) == (_lib.NGZ_AGG_RES_ADDED, [0, 1], 1, False)
    assert enrich_field_plan(f2, cols, (0, 82, 3))["kind"] == _lib.NGZ_AGG_RES_NONE
    r = enrich_field_plan(f2, cols, (0, 234, 0))  # a lone cache index 1 is occurrence 0
    assert (r["kind"], r["candidates"], r["ordinal"]) == (_lib.NGZ_AGG_RES_ADDED, [2], 0)
    r = enrich_field_plan(f2, cols, (3746, 7, 1))  # after the added column of the writer's IE when present
    assert (r["kind"], r["candidates"], r["ordinal"], r["writer_after"]) == (_lib.NGZ_AGG_RES_ADDED, [3], 1, True)
    assert enrich_field_plan(f2, cols, (3746, 7, 2))["kind"] == _lib.NGZ_AGG_RES_NONE
    assert enrich_field_plan(f2, [], (3746, 7, 0))["kind"] == _lib.NGZ_AGG_RES_WRITER
    d = enrich_field_plan([(0, 302, 1)] + f2, cols, (0, 82, 0))
    assert d["dropped"] and d["kind"] == _lib.NGZ_AGG_RES_NONE


def test_every_mask_and_index_agrees_with_map_fields():
    fields = [(0, 82, 0), (0, 10, 0), (0, 82, 0), (3746, 7, 0)]
    cols = [(0, 10, 0), (0, 82, 0), (0, 82, 1), (0, 82, 5), (3746, 7, 0), (3746, 7, 2)]
    for (pen, ie), index in itertools.product([(0, 82), (0, 10), (3746, 7), (0, 1)], range(7)):
        got = enrich_field_plan(fields, cols, (pen, ie, index))
        for mask in range(1 << len(cols)):
            assert pick(got, mask) == map_fields_pick(fields, cols, (pen, ie, index), mask), (pen, ie, index, mask)
    assert KEY == _lib.NGZ_AGG_KEY
