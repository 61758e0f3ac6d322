"""GPU: the JSON lines of aggregated groups rendered on the device (include/ngz/flow_agg_json.h) against
FlowAggregator.flowinfo_json over the same rows (ngz_agg_flowinfo_json, the specification, which
tests/test_gpu_agg.py pins to the oracle): line for line in row order, through the offsets array, with the
guard bytes intact."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kats_agg as K  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, ADD, MN, MX, OR = K.OP_KEY, K.OP_ADD, K.OP_MIN, K.OP_MAX, K.OP_OR
T0, V4, V6 = 1_700_000_000, "192.0.2.1", "2001:db8::1"
HEAD = dict(shard_id=3, seq0=2 ** 32 - 2, export_time_ms=1_760_000_000_123)  # the sequence number wraps


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.output import AggFlowJson  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def msg(sets, t=T0, domain=7):
    body = b"".join(sets)
    return struct.pack(">HHIII", 10, 16 + len(body), t, 1, domain) + body


def tset(tid, fields):  # a field: (id, length) or (id, length, pen)
    body = struct.pack(">HH", tid, len(fields)) + b"".join(
        struct.pack(">HH", f[0], f[1]) if len(f) == 2 else struct.pack(">HHI", 0x8000 | f[0], f[1], f[2]) for f in fields)
    return struct.pack(">HH", 2, 4 + len(body)) + body


def dset(tid, recs):
    return struct.pack(">HH", tid, 4 + sum(map(len, recs))) + b"".join(recs)


def vl(b):
    return (bytes([len(b)]) if len(b) < 255 else b"\xff" + len(b).to_bytes(3, "big")) + b  # as tests/test_gpu_agg.py


def check(out, agg, raw, head=HEAD):
    from netgauze_amd import _lib
    st = out.encode(agg, raw, **head)
    data, offs = out.result(guard=True)
    offs = offs.tolist()
    assert data[offs[-1]:] == b"\xA5" * _lib.NGZ_OUTPUT_GUARD and offs[0] == 0 and offs == sorted(offs)
    assert st["rows"] == len(raw) == len(offs) - 1 and st["bytes"] == offs[-1]
    assert [data[a:b].decode() for a, b in zip(offs, offs[1:])] == agg.flowinfo_json(raw, **head)
    assert out.last_launches == 3
    return st


def run(fields, pushes, writer=0, window_s=60):
    """pushes: [(datagrams, peer ip, peer port)].  The flush's lines against the host function's."""
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import AggFlowJson
    agg, codecs = FlowAggregator(fields, window_s=window_s, lateness_s=window_s), {}
    for dgrams, ip, port in pushes:
        agg.push(codecs.setdefault(ip, FlowInfoCodec()).decode_datagrams(dgrams), port, 1_700_000_000_123, ip)
    _hdr, raw = agg.flush_raw()
    out = AggFlowJson()
    out.set_option(_lib.NGZ_AGG_JSON_OPT_WRITER, writer)
    check(out, agg, raw)
    return agg, out, raw


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_group_counts(dev, n):
    d = [msg([tset(300, [(11, 2), (1, 8)]), dset(300, [struct.pack(">HQ", 1000 + i % n, i) for i in range(n + 7)])])]
    agg, out, raw = run([(0, 11, 0, OK), (0, 1, 0, ADD)], [(d, V4, 4739)])
    assert raw.shape == (n, 128)
    assert out.encode(agg, raw[:0])["rows"] == 0 and out.last_launches == 0  # no row: no launch, an empty result
    assert out.result()[0] == b"" and out.result()[1].tolist() == [0]


@pytest.mark.parametrize("with_list", [False, True], ids=["rows256", "rows384"])
def test_byte_keys_and_values(dev, with_list):
    """String and octetArray keys of 0, 32, 33 and 300 bytes, an octetArray BoolMapOr; with a list Max the
    rows outgrow 256 bytes and a wave stages fewer than 64.  Long and short lines share a wave."""
    names = [b"", b"n" * 32, b"m" * 33, b"x" * 300]
    recs = [vl(names[i % 4]) + vl(bytes(range(1, 1 + len(names[(i // 4) % 4]) % 251)) if (i // 4) % 4 != 3 else b"\7" * 300) +
            struct.pack(">H", i % 5) + vl(bytes([i % 7, 1, 2])) + vl(bytes([i % 3]) * (40 if i % 2 else 3)) for i in range(80)]
    d = [msg([tset(320, [(82, 0xFFFF), (313, 0xFFFF), (11, 2), (95, 0xFFFF), (291, 0xFFFF)]), dset(320, recs)])]
    fields = [(0, 82, 0, OK), (0, 313, 0, OK), (0, 11, 0, OK), (0, 95, 0, OR)] + ([(0, 291, 0, MX)] if with_list else [])
    _agg, _out, raw = run(fields, [(d, V4, 4739)])
    assert raw.shape[1] == (384 if with_list else 256)


@pytest.mark.parametrize("writer", [0, 1], ids=["accumulating", "bytes"])
def test_line_longer_than_the_image(dev, writer):
    """An octetArray key of 9 000 bytes, each >= 100 and so four characters, is a line of 36 KB, longer
    than a wave's 30 KB image: it goes straight out, between short lines of the same wave."""
    recs = [vl((b"\xc8" * 9000, b"s", b"")[i % 3]) + struct.pack(">HQ", i % 2, i) for i in range(6)]
    d = [msg([tset(330, [(313, 0xFFFF), (11, 2), (1, 8)]), dset(330, recs)])]
    _agg, out, _raw = run([(0, 313, 0, OK), (0, 11, 0, OK), (0, 1, 0, ADD)], [(d, V4, 4739)], writer)
    assert max(np.diff(out.result()[1])) > 36000


def test_value_renderers(dev):
    """One template: a u64 Add that ends at 2^64 - 1, a signed Min of -2^31, a boolean, IPv6 Max (::1,
    2001:db8::2, v4-mapped, two equal zero runs), macAddress and u256 OR, dateTimeMilliseconds Min of -1500 and
    Max in year 10000, a dateTimeMicroseconds key, a dateTimeNanoseconds Max with a fraction, tcpControlBits OR,
    protocolIdentifier 6 and unassigned, forwardingStatus in a registered reason, an unassigned one and >= 256,
    flowDirection, a Huawei unknown-id key and an unknown-PEN key; an IPv4 and an IPv6 peer; an NFv9 group."""
    tpl = [(11, 2), (276, 1), (154, 8), (4, 1), (89, 4), (61, 1), (9999, 2, 2011), (1234, 3, 99999), (1, 8), (434, 4), (27, 16),
           (56, 6), (515, 32), (152, 8), (153, 8), (156, 8), (6, 2)]
    ntp = lambda unix, frac: struct.pack(">II", unix + 2208988800, frac)  # noqa: E731
    ip6 = [bytes(15) + b"\1", b"\x20\1\x0d\xb8" + bytes(11) + b"\2", bytes(10) + b"\xff\xff\1\2\3\4", b"\x20\1\0\0\0\0\0\1\0\0\0\0\0\1\0\2"]
    rec = lambda i, n, s, ms: (struct.pack(">HB", 80 + i, 1 + i % 2) + ntp(T0 - 7, 0x40000800) +  # noqa: E731
                               struct.pack(">BIBH", (6, 200, 17, 6)[i], (66, 70, 300, 129)[i], i % 2, 7 + i) + bytes([1, 2, 200 + i]) +
                               struct.pack(">Qi", n, s) + ip6[i] + bytes([i, 2, 3, 4, 5, 0xfe]) + bytes(31) + bytes([1 << i]) +
                               struct.pack(">qq", ms, ms) + ntp(T0 + i, 0x80000000 + i) + struct.pack(">H", 0x12 << i))
    recs = [rec(0, 2 ** 64 - 2, -5, -1500), rec(0, 1, -2 ** 31, 5000), rec(1, 9, 7, 253_402_300_800_000), rec(2, 3, 0, 0), rec(3, 4, 1, -1)]
    d = [msg([tset(340, tpl), dset(340, recs)])]
    fields = [(0, 11, 0, OK), (0, 276, 0, OK), (0, 154, 0, OK), (0, 4, 0, OK), (0, 89, 0, OK), (0, 61, 0, OK), (2011, 9999, 0, OK),
              (99999, 1234, 0, OK), (0, 8, 0, OK), (0, 12, 0, OK), (0, 7, 0, OK), (0, 1, 0, ADD), (0, 2, 0, ADD), (0, 434, 0, MN),
              (0, 27, 0, MX), (0, 56, 0, OR), (0, 515, 0, OR), (0, 152, 0, MN), (0, 153, 0, MX), (0, 156, 0, MX), (0, 6, 0, OR)]
    _agg, _out, raw = run(fields, [(d, V4, 4739), (d, V6, 4740), ([K.nf_packet()], V4, 9995)])
    assert len(raw) == 9


def test_strings(dev):
    """A string key with a quote, a backslash, a newline, 0x01 and a multi-byte UTF-8 character; a fixed
    string with an embedded NUL."""
    texts = ['q"b\\n\nc\x01é€'.encode(), b"\b\f\r\t\x1f ~", b""]
    recs = [vl(t) + fixed + struct.pack(">Q", 1) for t in texts for fixed in (b"ab\0cd\0\0\0", b"abcdefgh")]
    d = [msg([tset(345, [(82, 0xFFFF), (83, 8), (1, 8)]), dset(345, recs)])]
    _agg, _out, raw = run([(0, 82, 0, OK), (0, 83, 0, OK), (0, 1, 0, ADD)], [(d, V4, 4739)])
    assert len(raw) == 6


def test_shifting_presence_and_sets(dev):
    """IE 1 as key 1, which template 301 lacks; three template ids, three domains and two ports pushed in
    descending order: dictionary (bit) order is the reverse of value order."""
    pushes = [([msg([tset(310 - i, [(11, 2), (1, 8)] + [(1, 8)] * (i % 2)),
                     dset(310 - i, [struct.pack(">HQ", 80 + j % 2, 1) + struct.pack(">Q", j % 3) * (i % 2) for j in range(6 - i)])],
                    domain=90 - i)], V4, 5000 - 1000 * (i % 2)) for i in range(3)]
    run([(0, 11, 0, OK), (0, 1, 1, OK), (0, 1, 0, ADD)], pushes)


def test_stale_rows_and_emit(dev):
    """Rows of an earlier take are NGZ_E_INVALID; an encode after an emit reads that emit's rows and
    dictionaries, not an earlier flush's."""
    from netgauze_amd import _lib
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import OutputError
    tpl = [(82, 0xFFFF), (1, 8)]
    d1 = [msg([tset(350, tpl), dset(350, [vl(b"a" * 40) + struct.pack(">Q", 1)])], domain=1)]
    agg, out, raw1 = run([(0, 82, 0, OK), (0, 1, 0, ADD)], [(d1, V4, 4739)], window_s=60)
    codec = FlowInfoCodec()
    for t, tid, dom in ((T0, 351, 9), (T0 + 600, 352, 3)):  # the second push closes the first one's window
        agg.push(codec.decode_datagrams([msg([tset(tid, tpl), dset(tid, [vl(b"b" * 50) + struct.pack(">Q", 2)])], t, dom)]), 4739, 0, V4)
    _hdr, raw2 = agg.emit_raw()
    assert len(raw2) == 1
    with pytest.raises(OutputError) as e:
        out.encode(agg, raw1)
    assert e.value.code == _lib.NGZ_E_INVALID
    with pytest.raises(OutputError) as e:
        out.encode(agg, np.concatenate([raw1, raw2]))  # two takes in one call
    assert e.value.code == _lib.NGZ_E_INVALID
    check(out, agg, raw2)


def test_floats_are_refused(dev):
    """An f64 Add: NGZ_OUTPUT_E_UNSUPPORTED naming the IE and no launch; the host function still renders."""
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import AggFlowJson, OutputError
    agg = FlowAggregator([(0, 11, 0, OK), (0, 320, 0, ADD)])
    agg.push(FlowInfoCodec().decode_datagrams([msg([tset(360, [(11, 2), (320, 8)]), dset(360, [struct.pack(">Hd", 80, 1.5)])])]), 4739, 0, V4)
    _hdr, raw = agg.flush_raw()
    out = AggFlowJson()
    with pytest.raises(OutputError, match="absoluteError") as e:
        out.encode(agg, raw)
    assert e.value.code == _lib.NGZ_OUTPUT_E_UNSUPPORTED and out.last_launches == 0
    assert len(agg.flowinfo_json(raw)) == len(raw) == 1
