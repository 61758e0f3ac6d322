"""CPU checks of the two message-stream stages' handles (include/ngz/flow_json.h, include/ngz/flow_wire.h): what
create, the read-back functions, the options and the argument checks of encode answer before any encode --
none of which touches a device.  Both stages are held to the same table."""
import ctypes
import struct

import pytest

STAGES = {  # prefix: (its option, last_error(NULL), floats ngz_*_last_timing fills)
    "ngz_flow_json": ("NGZ_FLOW_JSON_OPT_FLOATS", b"null flow JSON stage", 3),
    "ngz_wire": ("NGZ_WIRE_OPT_ALIGN4", b"null wire stage", 4),
}


@pytest.mark.parametrize("prefix", sorted(STAGES))
def test_handle_before_any_encode_touches_no_device(prefix):
    from netgauze_amd import _lib
    lib = _lib.load()
    fn = lambda name: getattr(lib, prefix + "_" + name)  # noqa: E731
    option, null_error, n_times = STAGES[prefix]
    option, invalid = getattr(_lib, option), _lib.NGZ_E_INVALID

    h = ctypes.c_void_p()
    assert fn("create")(0, None) == invalid
    assert fn("create")(-1, ctypes.byref(h)) == invalid and not h.value
    assert fn("create")(7, ctypes.byref(h)) == 0 and h.value  # no such device: not looked at

    n, nb = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert fn("result")(h, None, None, None, ctypes.byref(n), ctypes.byref(nb)) == invalid and fn("last_error")(h) == b"no encode to read"
    assert (n.value, nb.value) == (5, 5)
    assert fn("set_option")(h, option, 1) == 0  # overwrites nothing: last_error keeps the last failure
    offs = (ctypes.c_uint64 * 1)(9)
    assert fn("to_host")(h, None, 0, offs, 1, None, 0) == invalid and fn("last_error")(h) == b"no encode to read" and offs[0] == 9
    assert fn("result")(None, None, None, None, None, None) == invalid == fn("to_host")(None, None, 0, None, 0, None, 0)

    assert fn("set_option")(h, option, 0) == 0
    assert fn("set_option")(h, option, 2) == invalid and fn("last_error")(h) == b"unknown option or value"
    assert fn("set_option")(h, option + 1, 1) == invalid == fn("set_option")(h, 0, 1)
    assert fn("set_option")(None, option, 1) == invalid

    out, somewhere = _lib.BatchOut(), ctypes.c_void_p(8)  # a context that is never looked at: the null beside it is refused first
    assert fn("encode")(None, somewhere, ctypes.byref(out), None, None) == invalid
    assert fn("encode")(h, None, ctypes.byref(out), None, None) == invalid
    assert fn("encode")(h, somewhere, None, None, None) == invalid

    t = [ctypes.c_float(-1) for _ in range(n_times)]
    assert fn("last_timing")(h, *[ctypes.byref(x) for x in t]) == 0 and [x.value for x in t] == [0] * n_times
    assert fn("last_timing")(h, *[None] * n_times) == invalid
    assert fn("last_timing")(h, *([ctypes.byref(x) for x in t[:-1]] + [None])) == invalid
    assert fn("last_timing")(None, *[ctypes.byref(x) for x in t]) == invalid
    assert fn("last_launches")(None) == invalid and fn("last_launches")(h) == 0
    assert fn("last_error")(None) == null_error
    for x in (h, None):
        fn("destroy")(x)


def test_f64_text_needs_room_for_the_whole_text():
    from netgauze_amd import _lib
    lib = _lib.load()
    bits = struct.unpack("<Q", struct.pack("<d", -1234.5625))[0]
    text = b"-1234.5625"
    buf = ctypes.create_string_buffer(b"#" * 32, 32)
    assert lib.ngz_flow_json_f64_text(bits, buf, len(text) - 1) == _lib.NGZ_E_INVALID and buf.raw == b"#" * 32
    assert lib.ngz_flow_json_f64_text(bits, None, 32) == _lib.NGZ_E_INVALID
    assert lib.ngz_flow_json_f64_text(bits, buf, len(text)) == len(text) and buf.raw[:len(text) + 1] == text + b"#"
