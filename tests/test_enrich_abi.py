"""CPU checks of the enrichment ABI (include/ngz/flow_enrich.h): exports, arity, version, struct
sizes, and the cache and lookup entry points -- none of which touches a device -- against the
restatement (tests/enrich_ref.py)."""
import ctypes
import os
import random
import re

import pytest

import enrich_ref as E
from test_enrich_ref import KATS, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngz", "flow_enrich.h")


def declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(ngz_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_functions_are_declared_in_the_binding_with_the_same_arity():
    from netgauze_amd import _lib
    decl = declarations()
    assert sorted(decl) == sorted(_lib.ENRICH_FUNCTIONS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name, n in decl.items():
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == n, name


def test_abi_versions_and_limits():
    from netgauze_amd import _lib
    text = open(HEADER).read()
    assert int(re.search(r"#define NGZ_ENRICH_ABI_VERSION (\d+)", text).group(1)) == 1 == _lib.NGZ_ENRICH_ABI_VERSION
    assert _lib.load().ngz_enrich_abi_version() == 1
    for name in ("MAX_SCOPE_FIELDS", "MAX_SHAPES", "MAX_COLUMNS", "MAX_KEY_BYTES", "MAX_DOMAINS"):
        m = re.search(r"#define NGZ_ENRICH_%s (\d+)" % name, text)
        assert int(m.group(1)) == getattr(_lib, "NGZ_ENRICH_" + name), name
    assert (_lib.NGZ_ENRICH_MAX_SCOPE_FIELDS, _lib.NGZ_ENRICH_MAX_SHAPES, _lib.NGZ_ENRICH_MAX_COLUMNS) == (4, 8, 32)


def test_struct_sizes_match_the_header():
    from netgauze_amd import _lib
    assert ctypes.sizeof(_lib.EnrichPeer) == 1 + 3 + 16
    assert ctypes.sizeof(_lib.EnrichField) == 4 + 2 + 1 + 1 + 4 + 4 + 8
    assert ctypes.sizeof(_lib.EnrichIe) == 8
    assert ctypes.sizeof(_lib.EnrichOperation) == 4 + 20 + 4 + 12 + 3 * 8
    assert ctypes.sizeof(_lib.EnrichResolved) == 4 + 2 + 2 + 1 + 1 + 2 + 4 + 8
    assert ctypes.sizeof(_lib.EnrichStats) == 4 * 8
    assert ctypes.sizeof(_lib.EnrichColumn) == 4 + 2 + 2 + 1 + 1 + 2 + 4 + 8


def test_binding_does_not_import_the_oracle():
    text = open(os.path.join(ROOT, "netgauze_amd", "enrich.py")).read()
    assert "oracle" not in text and "enrich_ref" not in text


def test_null_arguments_are_invalid():
    from netgauze_amd import _lib
    lib = _lib.load()
    st = _lib.EnrichStats()
    assert lib.ngz_enrich_create(0, None, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_enrich_op(None, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_enrich_apply(None, None, None, None, ctypes.byref(st), None) == _lib.NGZ_E_INVALID
    assert lib.ngz_enrich_totals(None, ctypes.byref(st), 0) == _lib.NGZ_E_INVALID
    lib.ngz_enrich_destroy(None)


@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_kats_through_the_c_abi(case):
    from netgauze_amd.enrich import FlowEnricher
    en = FlowEnricher(0, "w")

    def apply(op):
        if op["op"] == "upsert":
            en.upsert(op["ip"], op["domain"], op["weight"], op["scope"], op["fields"])
        elif op["op"] == "delete":
            en.delete(op["ip"], op["domain"], op["weight"], op["scope"], op["ies"])
        else:
            en.delete_all(op["ip"], op["domain"], op["weight"], op["scope"])

    replay(case, apply, en.lookup, lambda: en.peer_count)
    en.close()


def run_sequence(en, ref, seq):
    for step in seq:
        if "lookup" in step:
            ip, dom, rec = step["lookup"]
            assert en.lookup(ip, dom, rec) == ref.lookup(ip, dom, rec), step  # exact order
            continue
        ref.apply(step)
        if step["op"] == "upsert":
            en.upsert(step["ip"], step["domain"], step["weight"], step["scope"], step["fields"])
        elif step["op"] == "delete":
            en.delete(step["ip"], step["domain"], step["weight"], step["scope"], step["ies"])
        else:
            en.delete_all(step["ip"], step["domain"], step["weight"], step["scope"])
        assert en.peer_count == len(ref.peers), step


def test_random_operation_sequences_match_the_restatement_exactly():
    from netgauze_amd.enrich import FlowEnricher
    rng = random.Random(0x4E475A45)
    matched = 0
    for _ in range(2000):
        en, ref = FlowEnricher(0, "w"), E.Cache()
        seq = E.random_sequence(rng)
        run_sequence(en, ref, seq)
        matched += sum(1 for s in seq if "lookup" in s and ref.lookup(*s["lookup"]))
        en.close()
    assert matched > 500  # the sequences do reach matches


U32 = lambda ie, v: (0, ie, E.K_UINT, int(v).to_bytes(4, "little"))  # noqa: E731


def test_refused_operations_leave_the_cache_and_its_generation_unchanged():
    from netgauze_amd import _lib
    from netgauze_amd.enrich import EnrichError, FlowEnricher
    en = FlowEnricher(0, "w")
    ip = "10.0.0.1"
    en.upsert(ip, 0, 10, [U32(10, 5)], [U32(34, 100)])
    gen = en.generation
    assert gen == 1 and en.peer_count == 1
    add = [U32(34, 7)]
    refused = [
        [U32(10, 1), U32(14, 2), U32(10, 3), U32(14, 4), U32(252, 5)],   # five scope fields
        [(0, 82, E.K_STR, b"eth0")],                                    # a string
        [(0, 95, E.K_BYTES, b"\xf4")],                                  # octetArray (applicationId)
        [(0, 311, E.K_UINT, bytes(8))],                                 # float64 (samplingProbability)
        [(0, 291, E.K_BYTES, b"\0")],                                   # basicList
        [(0, 40000, E.K_UINT, bytes(4))],                               # unknown IE
        [(0, 154, E.K_DTFRAC, bytes(8))],                               # dateTimeMicroseconds
        [(0, 27, E.K_BYTES, bytes(17))],                                # longer than 16 bytes
        [(0, 10, E.K_UINT, bytes(3))],                                  # not a column width
    ]
    for scope in refused:
        for call in (lambda: en.upsert(ip, 0, 200, scope, add), lambda: en.delete_all(ip, 0, 200, scope),
                     lambda: en.delete(ip, 0, 200, scope, [(0, 34)])):
            with pytest.raises(EnrichError) as ei:
                call()
            assert ei.value.code == _lib.NGZ_E_LIMIT, scope
    with pytest.raises(EnrichError) as ei:
        en.upsert(ip, 0, 1, [(0, 10, 11, bytes(16))], add)  # NGZ_K_VLEN is not a value encoding
    assert ei.value.code == _lib.NGZ_E_INVALID
    with pytest.raises(EnrichError):
        en.set_table_bits(2)
    assert en.generation == gen and en.peer_count == 1
    assert en.lookup(ip, 1, [U32(10, 5)]) == [(0, 34, 0, E.K_UINT, (100).to_bytes(4, "little"), 10)]
    # operations that change nothing do not bump the generation; ones that do, do
    en.upsert(ip, 0, 10, [U32(10, 5)], [])
    en.upsert(ip, 0, 9, [U32(10, 5)], [U32(34, 1)])
    en.delete(ip, 0, 200, [U32(10, 5)], [])
    en.delete(ip, 0, 9, [U32(10, 5)], [(0, 34)])
    assert en.generation == gen
    en.upsert(ip, 0, 10, [U32(10, 5)], [U32(34, 101)])
    assert en.generation == gen + 1
    en.delete_all(ip, 0, 10, [U32(10, 5)])
    assert en.generation == gen + 2 and en.peer_count == 0
    en.close()


def test_create_needs_no_device():
    from netgauze_amd.enrich import FlowEnricher
    en = FlowEnricher(7, "writer-7")  # no such device here: only ngz_enrich_apply touches it
    en.upsert("10.0.0.1", 0, 1, [], [U32(34, 5)])
    assert en.lookup("10.0.0.1", 9, []) == [(0, 34, 0, E.K_UINT, (5).to_bytes(4, "little"), 1)]
    assert en.totals() == dict.fromkeys(E.STAT_KEYS, 0) and en.last_ms == 0
    en.close()
