"""CPU checks of the flow-output ABI (include/ngz/flow_output.h): exports, arity, version, struct sizes
and argument checking -- none of which touches a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngz", "flow_output.h")


def test_header_functions_are_declared_in_the_binding_with_the_same_arity():
    from netgauze_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): 0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1 for m in
            re.finditer(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(ngz_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S)}
    assert sorted(decl) == sorted(_lib.OUTPUT_FUNCTIONS) and len(decl) == 13
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, n in decl.items():
        assert hasattr(raw, name) and len(getattr(lib, name).argtypes) == n, name


def test_abi_version_limits_and_struct_sizes():
    from netgauze_amd import _lib
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define %s \(?(-?\w+)\)?" % name, text).group(1), 0)  # noqa: E731
    assert define("NGZ_OUTPUT_ABI_VERSION") == 1 == _lib.NGZ_OUTPUT_ABI_VERSION == _lib.load().ngz_output_abi_version()
    assert (define("NGZ_OUTPUT_MAX_FIELDS"), define("NGZ_OUTPUT_MAX_REFS"), define("NGZ_OUTPUT_GUARD")) == (
        _lib.NGZ_OUTPUT_MAX_FIELDS, _lib.NGZ_OUTPUT_MAX_REFS, _lib.NGZ_OUTPUT_GUARD)
    assert (define("NGZ_OUTPUT_E_UNSUPPORTED"), define("NGZ_OUTPUT_E_CONFIG"), define("NGZ_OUTPUT_OPTIONS")) == (
        _lib.NGZ_OUTPUT_E_UNSUPPORTED, _lib.NGZ_OUTPUT_E_CONFIG, _lib.NGZ_OUTPUT_OPTIONS)
    assert (define("NGZ_OUTPUT_OPT_RECOMPUTE"), define("NGZ_OUTPUT_OPT_IMAGE")) == (_lib.NGZ_OUTPUT_OPT_RECOMPUTE, _lib.NGZ_OUTPUT_OPT_IMAGE)
    snake = lambda s: re.sub(r"(?<!^)(?=[A-Z])", "_", s).upper().replace("LAYER2_SEGMENT_ID", "L2SEGMENT")  # noqa: E731
    for table, prefix in ((_lib.OUTPUT_SELECTS, "SEL"), (_lib.OUTPUT_TRANSFORMS, "TR"), (_lib.OUTPUT_DEFAULTS, "DEF")):
        for name, value in table.items():
            assert define("NGZ_OUT_%s_%s" % (prefix, snake(name))) == value, name
    assert ctypes.sizeof(_lib.OutputField) == 56 and ctypes.sizeof(_lib.OutputStats) == 24
    assert ctypes.sizeof(_lib.OutputPlan) == 8 + 64 * (4 + 2 * 10)


def test_create_and_the_host_entry_points_touch_no_device():
    from netgauze_amd import _lib
    from netgauze_amd.output import _c_fields
    lib = _lib.load()
    arr, _keep = _c_fields([{"name": "a", "refs": [(0, 1, 0)]}])
    h, err = ctypes.c_void_p(), ctypes.create_string_buffer(64)
    assert lib.ngz_output_create(7, arr, 1, ctypes.byref(h), err, 64) == 0 and h.value  # no such device: not looked at
    assert lib.ngz_output_create(-1, arr, 1, ctypes.byref(ctypes.c_void_p()), None, 0) == _lib.NGZ_E_INVALID
    assert lib.ngz_output_create(0, arr, 1, None, None, 0) == _lib.NGZ_E_INVALID
    assert lib.ngz_output_create(0, None, 1, ctypes.byref(ctypes.c_void_p()), None, 0) == _lib.NGZ_E_INVALID
    many, _k = _c_fields([{"name": "f%d" % i, "refs": [(0, 1, 0)]} for i in range(65)])
    assert lib.ngz_output_create(0, many, 65, ctypes.byref(ctypes.c_void_p()), err, 64) == _lib.NGZ_E_LIMIT and b"64" in err.value
    twice, _k = _c_fields([{"name": "a", "refs": [(0, 1, 0)]}] * 2)
    assert lib.ngz_output_create(0, twice, 2, ctypes.byref(ctypes.c_void_p()), err, 64) == _lib.NGZ_E_INVALID
    empty = ctypes.c_void_p()
    assert lib.ngz_output_create(0, None, 0, ctypes.byref(empty), None, 0) == 0
    assert lib.ngz_output_schema(empty, None, 0) == len('{\n  "type": "record",\n  "name": "acct_data",\n  "fields": [\n\n  ]\n}')
    assert lib.ngz_output_last_launches(h) == 0 and lib.ngz_output_last_launches(None) == _lib.NGZ_E_INVALID
    assert lib.ngz_output_slot(h, 0, None, None, None, None) == _lib.NGZ_E_INVALID
    assert b"no such slot" in lib.ngz_output_last_error(h)
    assert lib.ngz_output_to_host(h, 0, None, 0, None, 0) == _lib.NGZ_E_INVALID
    st = _lib.OutputStats()
    assert lib.ngz_output_totals(h, ctypes.byref(st), 1) == 0 and st.as_dict() == {"rows": 0, "rows_failed": 0, "bytes": 0}
    assert lib.ngz_output_totals(h, None, 0) == _lib.NGZ_E_INVALID
    a, b = ctypes.c_float(-1), ctypes.c_float(-1)
    assert lib.ngz_output_last_timing(h, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert lib.ngz_output_last_timing(h, None, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_output_set_option(h, _lib.NGZ_OUTPUT_OPT_RECOMPUTE, 1) == 0 == lib.ngz_output_set_option(h, _lib.NGZ_OUTPUT_OPT_IMAGE, 4096)
    assert lib.ngz_output_set_option(h, _lib.NGZ_OUTPUT_OPT_IMAGE, 100) == _lib.NGZ_E_INVALID == lib.ngz_output_set_option(h, 3, 0)
    out = _lib.BatchOut()
    assert lib.ngz_output_encode(h, None, ctypes.byref(out), None, None) == _lib.NGZ_E_INVALID
    assert lib.ngz_output_encode(None, None, None, None, None) == _lib.NGZ_E_INVALID
    plan = _lib.OutputPlan()
    assert lib.ngz_output_template_plan(h, None, 0, 10, ctypes.byref(plan)) == _lib.NGZ_E_INVALID
    assert lib.ngz_output_template_plan(h, (ctypes.c_uint8 * 8)(), 8, 11, ctypes.byref(plan)) == _lib.NGZ_E_INVALID
    for x in (h, empty, None):
        lib.ngz_output_destroy(x)
