"""GPU: float64 fields in the device JSON stages (NGZ_FLOW_JSON_OPT_FLOATS, NGZ_AGG_JSON_OPT_FLOATS) against the
host functions over the same data (DecodedBatch.json, FlowAggregator.flowinfo_json), byte for byte; with the
options off the datagrams stay with the host and the aggregated layout is refused, as before."""
import struct

import pytest

from test_f64_text import edges, patterns
from test_gpu_agg_json import ADD, MN, MX, OK, V4, check as agg_check, dset, msg, tset
from test_gpu_parity import ipfix_msg, ipfix_set, tmpl, vl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE, LINE, HOST = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.output import FlowJson  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def encode(batch, floats):
    """(how, stats, launches) of the batch encoded with the option at `floats`; every LINE against batch.json(d),
    every other line empty, the guard bytes intact."""
    from netgauze_amd import _lib
    from netgauze_amd.output import FlowJson
    fj = FlowJson()
    fj.set_option(_lib.NGZ_FLOW_JSON_OPT_FLOATS, floats)
    st = fj.encode(batch)
    data, offs, how = fj.result(guard=True)
    offs, how = offs.tolist(), how.tolist()
    assert data[offs[-1]:] == b"\xA5" * _lib.NGZ_OUTPUT_GUARD and offs[0] == 0 and st["bytes"] == offs[-1]
    for d, h in enumerate(how):
        assert data[offs[d]:offs[d + 1]] == (batch.json(d).encode() if h == LINE else b""), d
    return how, st, fj.last_launches


def test_flow_json_floats(dev):
    """samplingProbability and absoluteError of the edge list and 2 000 seeded patterns, in sets of 1, 64 and 65
    records, between datagrams of a template without floats and after the template-set datagram."""
    from netgauze_amd.flow import FlowInfoCodec
    vals = edges() + patterns(311, 2000)
    recs = [struct.pack(">IQQ", 0x0A000000 + i, a, b) for i, (a, b) in enumerate(zip(vals[::2], vals[1::2]))]
    plain = ipfix_msg([ipfix_set(300, struct.pack(">IH", 0x0A000001, 80) * 3)])
    dgrams, at = [ipfix_msg([ipfix_set(2, tmpl(300, [(8, 4), (7, 2)]) + tmpl(500, [(8, 4), (311, 8), (320, 8)]))]), plain], 0
    while at < len(recs):
        n = (1, 64, 65)[len(dgrams) % 3]
        dgrams.append(ipfix_msg([ipfix_set(500, b"".join(recs[at:at + n]))]))
        at += n
    dgrams.append(plain)
    n_float = len(dgrams) - 3
    batch = FlowInfoCodec(0).decode_datagrams(dgrams)
    how, st, launches = encode(batch, 1)
    assert how == [HOST] + [LINE] * (n_float + 2) and st["left_float"] == 0 and st["left_template"] == 1
    how0, st0, launches0 = encode(batch, 0)
    assert how0 == [HOST, LINE] + [HOST] * n_float + [LINE] and st0["left_float"] == n_float > 15 and launches == launches0


def test_flow_json_float_in_a_long_record(dev):
    """A float next to a 9 000-byte octetArray of bytes >= 100: the record outgrows a wave's image and goes out
    through the byte writer, between short records of its tile."""
    from netgauze_amd.flow import FlowInfoCodec
    recs = [vl(b"s") + struct.pack(">d", 0.1), vl(b"\xc8" * 9000) + struct.pack(">d", -1.2345678901234567e-300), vl(b"") + struct.pack(">d", 1e23)]
    dgrams = [ipfix_msg([ipfix_set(2, tmpl(510, [(313, 65535), (311, 8)]))]), ipfix_msg([ipfix_set(510, b"".join(recs))])]
    how, st, _ = encode(FlowInfoCodec(0).decode_datagrams(dgrams), 1)
    assert how == [HOST, LINE] and st["bytes"] > 36000


@pytest.mark.parametrize("writer", [0, 1], ids=["accumulating", "bytes"])
def test_agg_json_floats(dev, writer):
    """f64 Add, Min and Max whose groups end at an ordinary sum, inf, NaN (inf + -inf), -0.0 and a 17-digit sum."""
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import AggFlowJson, OutputError
    inf = float("inf")
    groups = [(1.5, 2.25), (1e308, 1e308), (inf, -inf), (-0.0, -0.0), (0.1, 0.2)]
    recs = [struct.pack(">Hddd", 80 + g, x, x * 3, -x) for g, pair in enumerate(groups) for x in pair]
    agg = FlowAggregator([(0, 11, 0, OK), (0, 320, 0, ADD), (0, 321, 0, MN), (0, 336, 0, MX)])
    agg.push(FlowInfoCodec().decode_datagrams([msg([tset(360, [(11, 2), (320, 8), (321, 8), (336, 8)]), dset(360, recs)])]), 4739, 0, V4)
    _hdr, raw = agg.flush_raw()
    assert len(raw) == len(groups)
    out = AggFlowJson()
    out.set_option(_lib.NGZ_AGG_JSON_OPT_WRITER, writer)
    with pytest.raises(OutputError, match="absoluteError") as e:
        out.encode(agg, raw)
    assert e.value.code == _lib.NGZ_OUTPUT_E_UNSUPPORTED
    out.set_option(_lib.NGZ_AGG_JSON_OPT_FLOATS, 1)
    agg_check(out, agg, raw)  # the lines against flowinfo_json, the guard bytes, three launches
    lines = "".join(agg.flowinfo_json(raw))
    assert all(t in lines for t in ('"absoluteError":3.75}', '"absoluteError":null}', '"absoluteError":-0.0}', '"absoluteError":0.30000000000000004}'))
