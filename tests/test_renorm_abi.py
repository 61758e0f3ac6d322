"""CPU checks of the renormalization ABI (include/ngz/flow_renormalize.h): exports, arity, version,
and the no-device plan introspection."""
import ctypes
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngz", "flow_renormalize.h")


def declarations():
    """{function: number of parameters} of the header's prototypes."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(ngz_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_functions_are_declared_in_the_binding_with_the_same_arity():
    from netgauze_amd import _lib
    decl = declarations()
    assert sorted(decl) == sorted(_lib.RENORM_FUNCTIONS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name, n in decl.items():
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == n, name


def test_abi_version():
    from netgauze_amd import _lib
    m = re.search(r"#define NGZ_RENORM_ABI_VERSION (\d+)", open(HEADER).read())
    assert int(m.group(1)) == 1 == _lib.NGZ_RENORM_ABI_VERSION == _lib.load().ngz_renorm_abi_version()


def test_struct_sizes_match_the_header():
    from netgauze_amd import _lib
    assert ctypes.sizeof(_lib.RenormStats) == 5 * 8
    assert ctypes.sizeof(_lib.RenormPlan) == 10 * 2 + 2 + 64 * 2 + 2


def test_binding_does_not_import_the_oracle():
    text = open(os.path.join(ROOT, "netgauze_amd", "renormalize.py")).read()
    assert "oracle" not in text and "renorm_ref" not in text


def test_null_arguments_are_invalid_without_a_device():
    from netgauze_amd import _lib
    lib = _lib.load()
    st = _lib.RenormStats()
    assert lib.ngz_renorm_apply(None, None, None, ctypes.byref(st), None) == _lib.NGZ_E_INVALID
    assert lib.ngz_renorm_totals(None, ctypes.byref(st), 0) == _lib.NGZ_E_INVALID
    assert lib.ngz_renorm_template_plan(None, 0, 10, None) == _lib.NGZ_E_INVALID
    lib.ngz_renorm_destroy(None)


def template(tid, fields):
    return struct.pack(">HH", tid, len(fields)) + b"".join(struct.pack(">HH", i, n) for i, n in fields)


@pytest.mark.parametrize("proto", [10, 9])
def test_plan_duplicated_parameters_and_counts(proto):
    from netgauze_amd.renormalize import template_plan
    #          0        1       2        3        4       5         6         7        8
    fields = [(34, 4), (1, 8), (8, 4), (34, 2), (2, 4), (1, 8), (305, 4), (35, 1), (86, 8)]
    p = template_plan(template(300, fields), proto)
    assert p == {"param_field": {34: 3, 35: 7, 305: 6}, "count_field": [1, 4, 5, 8], "dropped": False, "launches": 1}


@pytest.mark.parametrize("proto", [10, 9])
def test_plan_without_sampling_ies_needs_no_launch(proto):
    from netgauze_amd import synth
    from netgauze_amd.renormalize import template_plan
    p = template_plan(template(synth.T20_ID, synth.T20), proto)
    assert p["launches"] == 0 and not p["dropped"] and p["param_field"] == {}
    assert p["count_field"] == [i for i, (ie, _) in enumerate(synth.T20) if ie in (1, 2, 85, 86)]


def test_plan_options_templates_are_dropped():
    from netgauze_amd.renormalize import template_plan
    # IPFIX options template: id, field count, scope field count, specifiers (scope first)
    ipfix = struct.pack(">HHH", 400, 3, 1) + struct.pack(">HH", 149, 4) + struct.pack(">HH", 34, 4) + struct.pack(">HH", 1, 8)
    p = template_plan(ipfix, 10, options=True)
    assert p["dropped"] and p["launches"] == 0
    # only non-scope fields feed the plan
    assert p["param_field"] == {34: 1} and p["count_field"] == [2]
    # NetFlow v9 options template: id, scope bytes, option bytes, specifiers
    nf = struct.pack(">HHH", 400, 4, 8) + struct.pack(">HH", 1, 4) + struct.pack(">HH", 34, 4) + struct.pack(">HH", 35, 1)
    p = template_plan(nf, 9, options=True)
    assert p["dropped"] and p["launches"] == 0 and p["param_field"] == {34: 1, 35: 2} and p["count_field"] == []


def test_plan_ignores_enterprise_fields_and_rejects_truncated_records():
    from netgauze_amd.renormalize import RenormError, template_plan
    t = struct.pack(">HH", 300, 2) + struct.pack(">HHI", 0x8000 | 34, 4, 3746) + struct.pack(">HH", 2, 8)
    assert template_plan(t, 10) == {"param_field": {}, "count_field": [1], "dropped": False, "launches": 0}
    with pytest.raises(RenormError):
        template_plan(t[:-2], 10)
    with pytest.raises(RenormError):
        template_plan(t, 5)
