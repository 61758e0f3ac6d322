"""GPU: the flow output (include/ngz/flow_output.h) against tests/output_ref.py, byte for byte: datums
and offsets of every slot.  One template holds a field of every data type the registry has among the
accepted ones, and one config touches every accepted Identity and String type, the selects and the
defaults; the rows walk the varint width edges, the string lengths and the LDS image's limits."""
import struct

import numpy as np
import pytest

import output_ref
import parity
from netgauze_amd import _lib
from netgauze_amd.flow import FlowInfoCodec
from netgauze_amd.output import FlowOutput

pytestmark = pytest.mark.gpu

# template 700: u8, u16, u32, u64, s32, f64, bool, fixed string, variable string, mac, ipv4, ipv6, fixed
# octets, basicList, u256 (reduced), three MPLS labels, layer2SegmentId, and octetDeltaCount again
T700 = [(5, 1), (7, 2), (10, 4), (1, 8), (434, 4), (320, 8), (276, 1), (82, 16), (83, 0xFFFF), (56, 6), (8, 4), (27, 16),
        (313, 5), (291, 0xFFFF), (515, 20), (316, 3), (71, 3), (72, 3), (351, 8), (1, 5)]
T701 = [(7, 2), (83, 0xFFFF)]
EDGES = [0, 1, 63, 64, 8191, 8192, 2**31 - 1, 2**31, 2**63 - 1, 2**63, 2**64 - 1]
STRLEN = [0, 1, 63, 64, 300]
V6 = [bytes(16), bytes(15) + b"\1", bytes(10) + b"\xff\xff\x0a\0\0\1", bytes.fromhex("20010db8000000000001000000000001"),
      bytes.fromhex("00010000000000020000000000000003"), bytes.fromhex("fe800000000000000000000000000000"),
      bytes.fromhex("0123456789abcdef0123456789abcdef")]

ID = [{"name": "i%d" % ie, "refs": [(0, ie, 0)]} for ie in (5, 7, 10, 1, 434, 320, 276, 82, 83, 56, 8, 27, 313, 291, 515)]
STR = [{"name": "s%d" % ie, "refs": [(0, ie, 0)], "transform": "String"} for ie in (5, 7, 10, 1, 434, 276, 82, 83, 56, 8, 27)]
CONFIG = ID + STR + [
    {"name": "again", "refs": [(0, 1, 1)], "transform": "String"},
    {"name": "co1", "select": "Coalesce", "refs": [(0, 11, 0), (0, 7, 0)]},                     # the first IE absent
    {"name": "co2", "select": "Coalesce", "refs": [(0, 10, 0), (0, 14, 0)], "default": ("U32", 9)},  # only the second absent
    {"name": "comix", "select": "Coalesce", "refs": [(0, 12, 0), (0, 1, 0)], "transform": "String"},
    {"name": "vni", "select": "Layer2SegmentId", "refs": [(0, 351, 0)], "encap": 1},
    {"name": "seg", "select": "Layer2SegmentId", "refs": [(0, 351, 0)], "encap": ("Unassigned", 2), "transform": "String",
     "default": ("String", "none")},
    {"name": "m3", "select": "Multi", "refs": [(0, 72, 0), (0, 316, 0), (0, 71, 0), (0, 79, 0)], "transform": "MplsIndex"},
    {"name": "m1", "select": "Multi", "refs": [(0, 73, 0), (0, 71, 0)], "transform": "MplsIndex"},
    {"name": "m0", "select": "Multi", "refs": [(0, 73, 0), (0, 74, 0)], "transform": "MplsIndex"},
    {"name": "gone", "refs": [(0, 2, 0)]}, {"name": "gone_i", "refs": [(0, 2, 0)], "default": ("I64", -65)},
    {"name": "gone_s", "refs": [(0, 82, 1)], "default": ("String", "n/a")}, {"name": "gone_b", "refs": [(0, 313, 1)], "default": ("Bytes", b"\0\1")},
    {"name": "gone_f", "refs": [(0, 320, 1)], "default": ("F64", -1.5)}, {"name": "gone_t", "refs": [(0, 276, 1)], "default": ("Boolean", True)},
]


def vlen(b):
    return (bytes([len(b)]) if len(b) < 255 else b"\xff" + len(b).to_bytes(3, "big")) + b


def rec700(i, long_string=False):
    e = EDGES[i % len(EDGES)]
    n = 9000 if long_string else STRLEN[i % len(STRLEN)]
    text = bytes(97 + (i + k) % 26 for k in range(n))
    return b"".join([
        bytes([e & 0xFF]), struct.pack(">HIQ", e & 0xFFFF, (e >> (i % 3)) & 0xFFFFFFFF, e), struct.pack(">i", [0, -1, 63, -64, 64, -65, 2**31 - 1, -2**31][i % 8]),
        struct.pack(">d", [0.0, -1.5, 1e300][i % 3]), bytes([i % 2]), (text[:i % 17] + bytes(16))[:16], vlen(text),
        bytes((i * 7 + k) & 0xFF for k in range(6)), struct.pack(">I", [0, 0x0A000001, 0xFFFFFFFF, 0xC0A801FE][i % 4]), V6[i % len(V6)],
        bytes((i + k) & 0xFF for k in range(5)), vlen(bytes(i % 7)), bytes((i + k) & 0xFF for k in range(20)),
        (i * 4099 & 0xFFFFFF).to_bytes(3, "big"), (0xFFFFFF - i).to_bytes(3, "big"), (i % 3).to_bytes(3, "big"),
        struct.pack(">Q", ((1 + i % 3) << 56) | (0xABCDEF012345 >> (i % 5))), ((e >> 3) & 0xFFFFFFFFFF).to_bytes(5, "big")])


def message(sets, seq=0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIII", 10, 16 + len(body), 1_700_000_000, seq, 7) + body


def batch_of(n):
    """n records of template 700 (a 9000-byte string in rows 1 and 65), five of template 701, and for
    n >= 3 a message in the middle that fails after its records were laid out."""
    tmpl = lambda tid, fl: struct.pack(">HH", tid, len(fl)) + b"".join(struct.pack(">HH", ie, ln) for ie, ln in fl)  # noqa: E731
    dgrams = [message([(2, tmpl(700, T700) + tmpl(701, T701))])]
    recs = [rec700(i, i in (1, 65) and n >= 3) for i in range(n)]
    i = 0
    while i < n:
        k = i + 1
        while k < n and k - i < max(1, min(40, n // 3)) and sum(map(len, recs[i:k + 1])) < 60000:
            k += 1
        sets = [(700, b"".join(recs[i:k]))]
        if n >= 3 and i <= n // 2 < k:
            sets.append((999, b"\0" * 4))  # no such template: the whole message is an error
        dgrams.append(message(sets, i))
        if i == 0:
            dgrams.append(message([(701, b"".join(struct.pack(">H", 8190 + j) + vlen(b"x" * (62 + j)) for j in range(5)))]))
        i = k
    return dgrams


def check(out, codec, dgrams, oracle_codec=None):
    batch = codec.decode_datagrams(dgrams)
    oracle, oracle_codec = parity.oracle_datagrams(dgrams, oracle_codec)
    want = output_ref.encode_batch(CONFIG, batch, oracle)
    stats = out.encode(batch)
    assert len(want) == len(batch.slots) == 2
    for s, rows in enumerate(want):
        data, offs = out.slot(s, guard=True)
        ends = np.cumsum([0] + [len(r) for r in rows], dtype=np.uint64)
        assert offs.tolist() == ends.tolist(), "offsets of slot %d" % s
        got = [data[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
        bad = [r for r in range(len(rows)) if got[r] != rows[r]]
        assert not bad, (s, bad[:4], got[bad[0]].hex(), rows[bad[0]].hex())
        assert data[int(offs[-1]):] == b"\xa5" * _lib.NGZ_OUTPUT_GUARD  # nothing written past the end
    failed = sum(1 for rows in want for r in rows if not r)
    assert stats == {"rows": sum(map(len, want)), "rows_failed": failed, "bytes": sum(len(r) for rows in want for r in rows)}
    # the set pass; per slot a size pass and a scan, and a pack pass where it has bytes
    assert out.last_launches == 1 + sum(2 + any(rows) for rows in want)
    return stats, oracle_codec


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1025])
def test_datums_match_the_reference(n):
    stats, _ = check(FlowOutput(CONFIG), FlowInfoCodec(0), batch_of(n))
    assert stats["rows"] == n + 5 and (stats["rows_failed"] > 0) == (n >= 3)


@pytest.mark.parametrize("recompute,image", [(1, 8192), (0, 4096), (1, 4096)])
def test_pack_variants_write_the_same_bytes(recompute, image):
    out = FlowOutput(CONFIG)
    out.set_option(_lib.NGZ_OUTPUT_OPT_RECOMPUTE, recompute)
    out.set_option(_lib.NGZ_OUTPUT_OPT_IMAGE, image)
    check(out, FlowInfoCodec(0), batch_of(257))


def test_a_smaller_batch_on_the_same_object_and_an_empty_one():
    out, codec = FlowOutput(CONFIG), FlowInfoCodec(0)
    _, oc = check(out, codec, batch_of(257))
    check(out, codec, batch_of(3), oc)
    assert out.encode(codec.decode_datagrams([b"\0" * 20])) == {"rows": 0, "rows_failed": 0, "bytes": 0}
    assert out.last_launches == 0 and out.totals()["rows"] == 257 + 5 + 3 + 5
