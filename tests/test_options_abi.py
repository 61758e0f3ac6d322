"""CPU checks of the flow-options ABI (include/ngz/flow_options.h): exports, arity, version, struct
sizes, and argument checking -- none of which touches a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngz", "flow_options.h")


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
    assert sorted(decl) == sorted(_lib.OPTIONS_FUNCTIONS) and len(decl) == 12
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name, n in decl.items():
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == n, name


def test_abi_version_limits_and_struct_sizes():
    from netgauze_amd import _lib
    text = open(HEADER).read()
    assert int(re.search(r"#define NGZ_OPTIONS_ABI_VERSION (\d+)", text).group(1)) == 1 == _lib.NGZ_OPTIONS_ABI_VERSION
    assert _lib.load().ngz_options_abi_version() == 1
    assert int(re.search(r"#define NGZ_OPTIONS_MAX_REFS (\d+)", text).group(1)) == _lib.NGZ_OPTIONS_MAX_REFS == 24
    assert int(re.search(r"#define NGZ_OPTIONS_OPTIONS (0x[0-9a-f]+)", text).group(1), 16) == _lib.NGZ_OPTIONS_OPTIONS
    assert ctypes.sizeof(_lib.OptionsStats) == 6 * 8
    assert ctypes.sizeof(_lib.OptionsPlan) == 4 + 4 + 4 + 2 * (2 * 24 * 8) + 2 * (2 * 24 * 2)
    for value, name in _lib.OPTIONS_CLASSES.items():
        assert re.search(r"#define NGZ_OPTIONS_%s %d\b" % (name.upper(), value), text), name


def test_create_and_the_host_entry_points_touch_no_device():
    """On a machine without a GPU every call below still answers: the device is first touched by a
    harvest."""
    from netgauze_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ngz_options_create(0, 16, ctypes.byref(h)) == 0 and h.value
    assert lib.ngz_options_create(7, 255, ctypes.byref(ctypes.c_void_p())) == 0  # no such device: not looked at
    assert lib.ngz_options_create(-1, 16, ctypes.byref(ctypes.c_void_p())) == _lib.NGZ_E_INVALID
    assert lib.ngz_options_create(0, 16, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_options_op_count(h) == 0 and lib.ngz_options_last_launches(h) == 0
    op = _lib.EnrichOperation()
    assert lib.ngz_options_op(h, 0, ctypes.byref(op)) == _lib.NGZ_E_INVALID
    assert b"no such operation" in lib.ngz_options_last_error(h)
    st = _lib.OptionsStats()
    assert lib.ngz_options_totals(h, ctypes.byref(st), 1) == 0 and st.as_dict() == dict.fromkeys(st.as_dict(), 0)
    assert lib.ngz_options_totals(h, None, 0) == _lib.NGZ_E_INVALID
    ms = ctypes.c_float(-1)
    assert lib.ngz_options_last_timing(h, ctypes.byref(ms)) == 0 and ms.value == 0
    assert lib.ngz_options_last_timing(h, None) == _lib.NGZ_E_INVALID
    peer = _lib.EnrichPeer.of("10.0.0.1")
    out = _lib.BatchOut()
    assert lib.ngz_options_harvest(h, None, ctypes.byref(out), ctypes.byref(peer), None, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_options_harvest(None, None, None, None, None, None) == _lib.NGZ_E_INVALID
    # feeding no operations into an enricher: nothing applied, nothing refused
    e = ctypes.c_void_p()
    assert lib.ngz_enrich_create(0, b"w", ctypes.byref(e)) == 0
    n = ctypes.c_uint64(9)
    assert lib.ngz_options_feed(h, e, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.ngz_options_feed(h, None, None) == _lib.NGZ_E_INVALID
    plan = _lib.OptionsPlan()
    assert lib.ngz_options_template_plan(None, 0, 10, ctypes.byref(plan)) == _lib.NGZ_E_INVALID
    buf = (ctypes.c_uint8 * 8)()
    assert lib.ngz_options_template_plan(buf, 8, 11, ctypes.byref(plan)) == _lib.NGZ_E_INVALID
    lib.ngz_enrich_destroy(e)
    lib.ngz_options_destroy(h)
    lib.ngz_options_destroy(None)
