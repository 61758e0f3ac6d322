"""GPU: the JSON lines of decoded messages rendered on the device (include/ngz/flow_json.h) against
DecodedBatch.json(d) (ngz_dgram_json, the specification, which tests/test_gpu_jsonl.py pins to the reference's
goldens and the oracle): byte for byte through the offsets array, with the guard bytes intact and `how` of
every datagram as the case constructs it."""
import struct

import pytest

import golden_io as G
from test_gpu_parity import ipfix_msg, ipfix_set, nf_msg, tmpl, vl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE, LINE, HOST = 0, 1, 2
A, B = [(8, 4), (7, 2)], [(12, 4)]  # templates 300 and 302
rec_a = lambda i: struct.pack(">IH", 0x0A000000 + i, i & 0xFFFF)  # noqa: E731
rec_b = lambda i: struct.pack(">I", 0xC0000200 + i)  # noqa: E731
TEMPLATES = ipfix_msg([ipfix_set(2, tmpl(300, A) + tmpl(302, B))])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.output import FlowJson  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def check(dgrams, how, stats=None):
    """Decode `dgrams` as one batch and encode it: guard, offsets, stats and `how` as constructed (None: by the
    decode's status and the specification's own text), every line against batch.json(d)."""
    from netgauze_amd import _lib
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import FlowJson
    batch, fj = FlowInfoCodec(0).decode_datagrams(dgrams), FlowJson()
    st = fj.encode(batch)
    data, offs, got_how = fj.result(guard=True)
    offs, got_how = offs.tolist(), got_how.tolist()
    assert data[offs[-1]:] == b"\xA5" * _lib.NGZ_OUTPUT_GUARD and offs[0] == 0 and offs == sorted(offs) and st["bytes"] == offs[-1]
    spec = [batch.json(d) if s == 0 else None for d, s in enumerate(batch.dgram_headers()["status"].tolist())]
    if how is None:
        how = [NONE if js is None else HOST if '{"Template":[' in js or '{"OptionsTemplate":[' in js else LINE for js in spec]
    assert got_how == how
    for d, h in enumerate(how):
        assert data[offs[d]:offs[d + 1]] == (spec[d].encode() if h == LINE else b""), d
    assert (st["lines"], st["not_ok"], st["left_template"] + st["left_float"]) == (how.count(LINE), how.count(NONE), how.count(HOST))
    for k, v in (stats or {}).items():
        assert st[k] == v, (k, st)
    return batch, fj


def tile_edge_dgrams(n):
    a, b = [rec_a(i) for i in range(n)], [rec_b(i) for i in range(n)]
    return a, [TEMPLATES, ipfix_msg([ipfix_set(300, b"".join(a))]), ipfix_msg([ipfix_set(300, b"".join(a)), ipfix_set(300, a[0])]),
               ipfix_msg([ipfix_set(300, b"".join(a)), ipfix_set(302, b"".join(b)), ipfix_set(300, a[-1]), ipfix_set(302, b"".join(b))]),
               ipfix_msg([])]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges(dev, n):
    """Sets of n records around the 64-record tile; two sets of one template; sets alternating between two
    templates; a message of a header alone.  Three templates launch what one template launches."""
    a, dgrams = tile_edge_dgrams(n)
    _batch, fj = check(dgrams, [HOST, LINE, LINE, LINE, LINE])
    one = [ipfix_msg([ipfix_set(2, tmpl(300, A))])] + dgrams[1:3]
    three = [ipfix_msg([ipfix_set(2, tmpl(300, A) + tmpl(302, B) + tmpl(303, A))])] + dgrams[1:4] + [ipfix_msg([ipfix_set(303, a[0])])]
    assert check(one, [HOST, LINE, LINE])[1].last_launches == check(three, [HOST] + [LINE] * 4)[1].last_launches == fj.last_launches


def test_one_handle_across_batches(dev):
    """One codec and one stage handle over batches of different shape, large, small, large again: after each
    encode the bytes with their guard, the offsets, `how`, the stats and the launches are those of a fresh
    handle on the same batch, whatever the handle's buffers held before."""
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import FlowJson
    codec, fj = FlowInfoCodec(0), FlowJson()
    for n in (129, 1, 129):
        batch = codec.decode_datagrams(tile_edge_dgrams(n)[1])
        got, fresh = [], FlowJson()
        for h in (fj, fresh):
            st = h.encode(batch)
            data, offs, how = h.result(guard=True)
            got.append((data, offs.tolist(), how.tolist(), st, h.last_launches))
        assert got[0] == got[1], n
        assert got[0][2] == [HOST, LINE, LINE, LINE, LINE] and got[0][3]["lines"] == 4 and got[0][3]["bytes"] == got[0][1][-1] > 0


def fixed_kinds():
    """Every fixed-length decode rule but floats: unsigned 1 / 2 / 4 / 8, signed32, boolean, IPv4, IPv6, MAC, u256,
    dateTimeSeconds / Milliseconds (negative) / Microseconds / Nanoseconds (nanos >= 10^9 in a leap second), a fixed
    string with a NUL, protocolIdentifier, forwardingStatus and flowDirection (registered, nested, unassigned),
    tcpControlBits, a VMware IE, a Huawei unknown id, an unknown PEN."""
    fields = [(5, 1), (7, 2), (10, 4), (1, 8), (434, 4), (276, 1), (8, 4), (27, 16), (56, 6), (515, 32), (150, 4), (152, 8), (154, 8),
              (156, 8), (83, 8), (4, 1), (89, 4), (61, 1), (6, 2), (880, 1, 6876), (9999, 2, 2011), (1234, 3, 99999)]
    ip6 = [bytes(15) + b"\1", b"\x20\1\x0d\xb8" + bytes(11) + b"\2", bytes(10) + b"\xff\xff\1\2\3\4", b"\x20\1\0\0\0\0\0\1\0\0\0\0\0\1\0\2"]
    rec = lambda i: (struct.pack(">BHIQiBI", 255 - i, 65535 - i, 2 ** 32 - 1 - i, 2 ** 64 - 1 - i, (-2 ** 31, -1, 0, 7)[i], 1 + i % 2,  # noqa: E731
                                 0xC0A80000 + i) + ip6[i] + bytes([i, 2, 3, 4, 5, 0xFE]) + bytes(31) + bytes([1 << i]) +
                     struct.pack(">Iq", 1_700_000_000 + i, (-1500, -1, 0, 253_402_300_800_000)[i]) +
                     struct.pack(">IIII", 1_700_000_039, (0xFFFFFFFF, 12345, 0, 1 << 31)[i], 1_700_000_039, (0xFFFFFFFF, 0x80000000, 1, 0)[i]) +
                     (b"ab\0cd\0\0\0", b"abcdefgh", b"\0" * 8, b'q"\\\x01\x1f\x7f\0\0')[i] +
                     struct.pack(">BIBHB", (6, 200, 17, 1)[i], (66, 70, 300, 129)[i], i % 2, 0x12 << i, 7 + i) + bytes([i, 200 + i]) + bytes([1, 2, 200 + i]))
    return [ipfix_msg([ipfix_set(2, tmpl(400, fields))]), ipfix_msg([ipfix_set(400, b"".join(rec(i) for i in range(4)))])]


def variable_kinds():
    """Variable-length strings with a quote, a backslash, controls and multi-byte characters; variable-length
    octets of 0, 254, 255 and 300 bytes; a vendor-unknown variable-length IE."""
    texts = ['q"b\\n\nc\x01é€'.encode(), b"\b\f\r\t\x1f ~", b"", "ü".encode() * 200]
    octets = [b"", bytes(range(254)), b"\xc8" * 255, bytes(i % 251 for i in range(300))]
    recs = [vl(texts[i]) + struct.pack(">H", i) + vl(octets[i]) + vl(bytes([i]) * i) for i in range(4)]
    return [ipfix_msg([ipfix_set(2, tmpl(410, [(82, 65535), (7, 2), (313, 65535), (1000, 65535, 2011)]))]), ipfix_msg([ipfix_set(410, b"".join(recs))])]


@pytest.mark.parametrize("dgrams", [fixed_kinds, variable_kinds], ids=["fixed", "variable"])
def test_value_kinds(dev, dgrams):
    check(dgrams(), [HOST, LINE])


def test_netflow_v9(dev):
    """A data template and an options template (scopes System, Interface and an unknown one) whose data records
    come in later datagrams than the templates."""
    tset = struct.pack(">HH", 0, 4 + 4 + 16) + struct.pack(">HH", 260, 4) + struct.pack(">HHHHHHHH", 8, 4, 1, 4, 7, 2, 6, 1)
    oset = struct.pack(">HH", 1, 4 + 6 + 12 + 4 + 2) + struct.pack(">HHH", 270, 12, 4) + struct.pack(">HHHHHH", 1, 4, 2, 2, 9, 2) + \
        struct.pack(">HH", 34, 4) + b"\0\0"
    rec, orec = struct.pack(">IIHB", 0x0A000001, 1500, 80, 0x12), struct.pack(">IHHI", 77, 3, 0xABCD, 1000)
    data, odata = struct.pack(">HH", 260, 4 + 11 * 3 + 3) + rec * 3 + b"\0\0\0", struct.pack(">HH", 270, 4 + 12 * 2) + orec * 2
    check([nf_msg([tset, oset], count=2), nf_msg([data], count=3), nf_msg([odata], count=2), nf_msg([odata, data], count=5)],
          [HOST, LINE, LINE, LINE])


def test_long_output(dev):
    """A 9 000-byte octetArray of bytes >= 100 is a record of 36 KB, longer than a wave's image: it goes straight
    out between short records of its tile.  The second set's 64 records exceed the image together: groups."""
    long_set = [vl(b"s") + b"\0\1", vl(b"\xc8" * 9000) + b"\0\2", vl(b"") + b"\0\3"]
    wide_set = [vl(bytes([100 + i]) * 150) + struct.pack(">H", i) for i in range(64)]
    dgrams = [ipfix_msg([ipfix_set(2, tmpl(420, [(313, 65535), (7, 2)]))]), ipfix_msg([ipfix_set(420, b"".join(long_set)), ipfix_set(420, b"".join(wide_set))])]
    _batch, fj = check(dgrams, [HOST, LINE])
    assert fj.result()[1][2] > 36000 + 64 * 600


def test_hand_over(dev):
    """Template-set datagrams, an error, an Ok(None) and a float field's data set among ordinary datagrams.  The
    registry's float IEs are all float64 (absoluteError here)."""
    from netgauze_amd.output import FlowJson
    a = ipfix_set(300, rec_a(1) + rec_a(2))
    dgrams = [ipfix_msg([ipfix_set(2, tmpl(300, A) + tmpl(301, [(7, 2), (320, 8)]) + tmpl(302, B))]), ipfix_msg([a]),
              ipfix_msg([ipfix_set(999, b"\0" * 8)]), ipfix_msg([ipfix_set(302, rec_b(1))]),
              ipfix_msg([a, ipfix_set(301, struct.pack(">Hd", 80, 1.5)), a]), ipfix_msg([a, a]), ipfix_msg([ipfix_set(2, tmpl(300, A)), a]),
              b"\x00\x0a\x00", ipfix_msg([ipfix_set(302, rec_b(2))])]
    batch, _fj = check(dgrams, [HOST, LINE, NONE, LINE, HOST, LINE, HOST, NONE, LINE],
                       dict(lines=4, left_template=2, left_float=1, not_ok=2))
    assert FlowJson().lines(batch) == [(d, js) for d, st, js, _ in batch.json_lines() if st == 0]


@pytest.mark.parametrize("name", [c[0] for c in G.cases()])
def test_goldens(dev, name):
    """Every reference capture, one batch per peer: no float IE in them, and the datagrams left to the host are
    the decode's own count of datagrams with template sets."""
    peers = {}
    for src, sp, _dst, _dp, payload in G.datagrams(name):
        peers.setdefault((src, sp), []).append(payload)
    for dgrams in peers.values():
        batch, fj = check(dgrams, None, dict(left_float=0))
        assert fj.encode(batch)["left_template"] == batch.n_template_dgrams
