"""GPU: the Avro datums of aggregated groups (include/ngz/flow_agg_output.h) against the restatement
(tests/agg_output_ref.py over the aggregation oracle's groups).  Every config selects all key fields, so
a datum identifies its group: the sorted datums of a flush are compared with the sorted reference datums,
through the offsets array, with the guard bytes intact."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_output_ref as REF  # noqa: E402
import kats_agg as K  # noqa: E402
import ngz_agg_oracle as A  # noqa: E402
import ngz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, ADD, MN, MX, OR = K.OP_KEY, K.OP_ADD, K.OP_MIN, K.OP_MAX, K.OP_OR
T0, V4, V6 = 1_700_000_000, "192.0.2.1", "2001:db8::1"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.output import AggFlowOutput  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def msg(sets, t=T0, domain=7):
    body = b"".join(sets)
    return struct.pack(">HHIII", 10, 16 + len(body), t, 1, domain) + body


def tset(tid, fields):
    body = struct.pack(">HH", tid, len(fields)) + b"".join(struct.pack(">HH", i, n) for i, n in fields)
    return struct.pack(">HH", 2, 4 + len(body)) + body


def dset(tid, recs):
    return struct.pack(">HH", tid, 4 + sum(map(len, recs))) + b"".join(recs)


def vl(b):
    return (bytes([len(b)]) if len(b) < 255 else b"\xff" + len(b).to_bytes(3, "big")) + b  # as tests/test_gpu_agg.py


def f(name, *refs, **kw):
    return dict(name=name, refs=list(refs), **kw)


def extras(ts="TimestampMillisString"):
    """The fields only a group's record has (actor.rs:222-240), under the transforms they can take."""
    return [f("flows", (0, 375, 0)), f("flows_s", (0, 375, 0), transform="String"), f("min_exp", (0, 264, 0), transform=ts),
            f("max_exp", (0, 260, 0), transform=ts), f("coll", (0, 258, 0), transform=ts), f("ws", (3746, 1, 0), transform=ts),
            f("we", (3746, 2, 0), transform=ts), f("peer", (0, 403, 0), (0, 404, 0), select="Coalesce", transform="String"),
            f("peer6", (0, 404, 0), default=("String", "none"))]


def sets(n):
    return [f("%s%d" % (nm, i), (pen, ie, i), **({"default": ("U32", 99)} if nm == "dom" else {}))
            for nm, pen, ie in (("port", 3746, 4), ("dom", 0, 405), ("tid", 3746, 3)) for i in range(n)]


def run(fields, config, pushes, window_s=60):
    """pushes: [(datagrams, peer ip, peer port)].  The flush's datums against the oracle's; the rows."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import AggFlowOutput
    agg, oracle = FlowAggregator(fields, window_s=window_s, lateness_s=window_s), A.FlowAggregatorOracle(fields, window_s, window_s)
    codecs = {}
    for dgrams, ip, port in pushes:
        c, oc = codecs.setdefault(ip, (FlowInfoCodec(), O.FlowInfoCodec()))
        agg.push(c.decode_datagrams(dgrams), port, 1_700_000_000_123, ip)
        A.aggregate_datagrams(fields, dgrams, port, 1_700_000_000_123, peer_ip=ip, agg=oracle, codec=oc)
    _hdr, raw = agg.flush_raw()
    out = AggFlowOutput(config)
    check(out, agg, raw, [REF.datum(config, oracle, g) for g in oracle.emit() + oracle.flush()])  # a flush hands out closed windows too
    return agg, out, raw


def check(out, agg, raw, ref):
    from netgauze_amd import _lib
    st = out.encode(agg, raw)
    data, offs = out.result(guard=True)
    offs = offs.tolist()
    assert data[offs[-1]:] == b"\xA5" * _lib.NGZ_OUTPUT_GUARD and offs[0] == 0 and offs == sorted(offs)
    assert st["rows"] == len(raw) == len(offs) - 1 and st["bytes"] == offs[-1]
    assert sorted(data[a:b] for a, b in zip(offs, offs[1:])) == sorted(ref)
    assert out.last_launches == 3


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_group_counts(dev, n):
    d = [msg([tset(300, [(11, 2), (1, 8)]), dset(300, [struct.pack(">HQ", 1000 + i % n, i) for i in range(n + 7)])])]
    cfg = [f("port", (0, 11, 0)), f("bytes", (0, 1, 0)), f("bytes_s", (0, 1, 0), transform="String", default=("String", ""))]
    agg, out, raw = run([(0, 11, 0, OK), (0, 1, 0, ADD)], cfg + extras() + sets(2), [(d, V4, 4739)])
    assert raw.shape == (n, 128)
    assert out.encode(agg, raw[:0])["rows"] == 0 and out.last_launches == 0  # no row: no launch, an empty result
    assert out.result()[0] == b"" and out.result()[1].tolist() == [0]


def test_shifting_presence(dev):
    """IE 1 as key 0, as key 1 (which template 301 lacks) and as the Add value: where a ref lands depends on
    the row's presence bits; refs at index 0..2 and one past the end, nullable and with a default.  A Min over
    flowStartMilliseconds, which no record carries, is null or its default in every row."""
    d = [msg([tset(300, [(1, 8), (1, 8), (11, 2)]), tset(301, [(1, 8), (11, 2)]),
              dset(300, [struct.pack(">QQH", 5, 6 + i % 2, 80 + i % 3) for i in range(12)]),
              dset(301, [struct.pack(">QH", 5, 80 + i % 3) for i in range(12)])])]
    cfg = [f("port", (0, 11, 0))] + [f("a%d" % i, (0, 1, i)) for i in range(4)] + \
          [f("d%d" % i, (0, 1, i), default=("U64", 77)) for i in range(4)] + \
          [f("c", (0, 1, 3), (0, 1, 2), (0, 1, 1), select="Coalesce", transform="String"),
           f("t", (0, 152, 0), transform="TimestampMillisString"), f("td", (0, 152, 0), transform="TimestampMillisString", default=("String", "-"))]
    run([(0, 11, 0, OK), (0, 1, 0, OK), (0, 1, 1, OK), (0, 1, 0, ADD), (0, 152, 0, MN)], cfg + extras(), [(d, V4, 4739)])


def test_set_members_ascend_by_value(dev):
    """Three template ids, three domains and two ports pushed in descending order: dictionary (bit)
    order is the reverse of value order; refs at index 0..2 and one beyond."""
    pushes = [([msg([tset(310 - i, [(11, 2), (1, 8)]), dset(310 - i, [struct.pack(">HQ", 80 + j % 2, 1) for j in range(6 - i)])],
                    domain=90 - i)], V4, 5000 - 1000 * (i % 2)) for i in range(3)]
    run([(0, 11, 0, OK), (0, 1, 0, ADD)], [f("port", (0, 11, 0))] + sets(4), pushes)


@pytest.mark.parametrize("with_list", [False, True], ids=["rows256", "rows384"])
def test_byte_keys_and_values(dev, with_list):
    """String and octetArray keys of 0, 32, 33 and 300 bytes, an octetArray BoolMapOr; with a list Max the
    rows outgrow 256 bytes and a wave stages fewer than 64.  Long and short datums share a wave."""
    names = [b"", b"n" * 32, b"m" * 33, b"x" * 300]
    recs = [vl(names[i % 4]) + vl(bytes(range(1, 1 + len(names[(i // 4) % 4]) % 251)) if (i // 4) % 4 != 3 else b"\7" * 300) +
            struct.pack(">H", i % 5) + vl(bytes([i % 7, 1, 2])) + vl(bytes([i % 3]) * (40 if i % 2 else 3)) for i in range(80)]
    d = [msg([tset(320, [(82, 0xFFFF), (313, 0xFFFF), (11, 2), (95, 0xFFFF), (291, 0xFFFF)]), dset(320, recs)])]
    fields = [(0, 82, 0, OK), (0, 313, 0, OK), (0, 11, 0, OK), (0, 95, 0, OR)] + ([(0, 291, 0, MX)] if with_list else [])
    cfg = [f("name", (0, 82, 0)), f("name_s", (0, 82, 0), transform="String"), f("blob", (0, 313, 0)), f("port", (0, 11, 0)),
           f("app", (0, 95, 0)), f("list", (0, 291, 0), default=("Bytes", b"\1\2"))]
    _agg, _out, raw = run(fields, cfg + extras(), [(d, V4, 4739)])
    assert raw.shape[1] == (384 if with_list else 256)


def test_datum_longer_than_the_image(dev):
    """A 300-byte key selected thirty times is a datum of 9 KB, longer than a wave's LDS image: it goes
    straight out, between short datums of the same wave."""
    recs = [vl((b"k" * 300, b"s", b"")[i % 3]) + struct.pack(">HQ", i % 4, i) for i in range(24)]
    d = [msg([tset(330, [(82, 0xFFFF), (11, 2), (1, 8)]), dset(330, recs)])]
    cfg = [f("port", (0, 11, 0))] + [f("name%d" % i, (0, 82, 0)) for i in range(30)]
    run([(0, 82, 0, OK), (0, 11, 0, OK), (0, 1, 0, ADD)], cfg, [(d, V4, 4739)])


def test_value_classes_peers_and_netflow9(dev):
    """A u64 Add that passes 2^63 (out `as i64`), signed Min, f64 Add, IPv6 Max, macAddress OR, a
    dateTimeMilliseconds Min before 1970, a dateTimeMicroseconds key and a dateTimeNanoseconds Max (NTP seconds and
    fraction) under TimestampMillisString; an IPv4 and an IPv6 peer; an NFv9 group."""
    tpl = [(11, 2), (1, 8), (434, 4), (320, 8), (27, 16), (56, 6), (152, 8), (154, 8), (156, 8)]
    ntp = lambda unix, frac: struct.pack(">II", unix + 2208988800, frac)  # noqa: E731
    rec = lambda p, n, s, x, ip, mac, ms: (struct.pack(">HQid", p, n, s, x) + ip + mac + struct.pack(">q", ms) +  # noqa: E731
                                           ntp(T0 - 7 + p, 0xC0000000) + ntp(T0 + n % 100, 0x80000000 + p))
    recs = [rec(80, (1 << 63) - 1, -5, 1.5, bytes(15) + b"\1", b"\1\2\3\4\5\6", -1500),
            rec(80, 9, 7, 2.25, b"\x20\1" + bytes(13) + b"\2", b"\x10\0\0\0\0\x60", 5000),
            rec(81, 3, -2 ** 31, -0.0, b"\0" * 10 + b"\xff\xff\1\2\3\4", b"\0" * 6, -1000)]
    d = [msg([tset(340, tpl), dset(340, recs)])]
    fields = [(0, 11, 0, OK), (0, 1, 0, ADD), (0, 434, 0, MN), (0, 320, 0, ADD), (0, 27, 0, MX), (0, 56, 0, OR), (0, 152, 0, MN),
              (0, 154, 0, OK), (0, 156, 0, MX)]
    cfg = [f("us", (0, 154, 0), transform="TimestampMillisString"), f("ns", (0, 156, 0), transform="TimestampMillisString"),
           f("port", (0, 11, 0), default=("U16", 0)), f("bytes", (0, 1, 0)), f("bytes_s", (0, 1, 0), transform="String"),
           f("smin", (0, 434, 0)), f("smin_s", (0, 434, 0), transform="String"), f("err", (0, 320, 0)), f("ip6", (0, 27, 0)),
           f("mac", (0, 56, 0), transform="String"), f("start", (0, 152, 0), transform="TimestampMillisString"),
           f("ifin", (0, 10, 0)), f("sport", (0, 7, 0), transform="String"), f("src", (0, 8, 0)), f("dst", (0, 12, 0), transform="String")]
    nf_fields = fields + [f_ for f_ in K.NF_FIELDS if f_[1] not in (11, 1)]
    run(nf_fields, cfg + extras() + sets(1), [(d, V4, 4739), (d, V6, 4740), ([K.nf_packet()], V4, 9995)])


def test_stale_rows_and_emit(dev):
    """Rows of an earlier take are NGZ_E_INVALID; an encode after an emit reads that emit's rows and
    dictionaries, not an earlier flush's."""
    from netgauze_amd import _lib
    from netgauze_amd.output import OutputError
    tpl = [(82, 0xFFFF), (1, 8)]
    d1 = [msg([tset(350, tpl), dset(350, [vl(b"a" * 40) + struct.pack(">Q", 1)])], domain=1)]
    cfg = [f("name", (0, 82, 0)), f("dom", (0, 405, 0)), f("tid", (3746, 3, 0)), f("we", (3746, 2, 0), transform="TimestampMillisString")]
    agg, out, raw1 = run([(0, 82, 0, OK), (0, 1, 0, ADD)], cfg, [(d1, V4, 4739)])
    from netgauze_amd.flow import FlowInfoCodec
    codec, oracle = FlowInfoCodec(), A.FlowAggregatorOracle(agg.fields, 60, 0)
    for t, tid, dom in ((T0, 351, 9), (T0 + 600, 352, 3)):  # the second push closes the first one's window
        dg = [msg([tset(tid, tpl), dset(tid, [vl(b"b" * 50) + struct.pack(">Q", 2)])], t, dom)]
        agg.push(codec.decode_datagrams(dg), 4739, 0, V4)
        A.aggregate_datagrams(agg.fields, dg, collection_ms=0, agg=oracle)
    _hdr, raw2 = agg.emit_raw()
    assert len(raw2) == 1
    with pytest.raises(OutputError) as e:
        out.encode(agg, raw1)
    assert e.value.code == _lib.NGZ_E_INVALID
    with pytest.raises(OutputError):
        out.encode(agg, np.concatenate([raw1, raw2]))  # two takes in one call
    check(out, agg, raw2, [REF.datum(cfg, oracle, g) for g in oracle.emit()])
