"""The enrichment restatement (tests/enrich_ref.py) pinned to the reference's unit cases and the
derived edges in tests/golden/enrich_kats.json, compared as sets."""
import json
import os

import pytest

import enrich_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "enrich_kats.json")) as f:
    KATS = json.load(f)


def field(f):
    return (f[0], f[1], f[2], bytes.fromhex(f[3]))


def operation(step):
    op = dict(step)
    op["scope"] = [field(f) for f in step["scope"]]
    op["fields"] = [field(f) for f in step.get("fields", [])]
    op["ies"] = [tuple(x) for x in step.get("ies", [])]
    return op


def replay(case, apply, lookup, peer_count):
    for i, step in enumerate(case["steps"]):
        if "op" in step:
            apply(operation(step))
        elif "lookup" in step:
            q = step["lookup"]
            got = lookup(q["ip"], q["domain"], [field(f) for f in q["record"]])
            exp = {(e[0], e[1], e[2], e[3], bytes.fromhex(e[4])) for e in q["expect"]}
            assert {g[:5] for g in got} == exp and len(got) == len(exp), (case["name"], i, got, exp)
        else:
            assert peer_count() == step["peer_count"], (case["name"], i)


@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_restatement_matches_the_kats(case):
    c = E.Cache()
    replay(case, c.apply, c.lookup, lambda: len(c.peers))


def test_scope_order_puts_the_empty_scope_first_and_orders_integers_by_value():
    k = E.Cache.scope_key
    keys = [k([(0, 302, E.K_UINT, (256).to_bytes(8, "little"))]), k([]), k([(0, 302, E.K_UINT, (2).to_bytes(8, "little"))]),
            k([(0, 10, E.K_UINT, (9).to_bytes(4, "little")), (0, 14, E.K_UINT, (1).to_bytes(4, "little"))]),
            k([(0, 10, E.K_UINT, (9).to_bytes(4, "little"))])]
    order = sorted(range(5), key=lambda i: E.scope_order(keys[i]))
    assert order == [1, 4, 3, 2, 0]
