"""GPU: IPFIX / NetFlow v9 messages written again from the decoded columns (include/ngz/flow_wire.h): the
device stage against ngz_dgram_wire (the specification), and both against bytes no writer of this test
made: the input itself where it is already what the reference's writer emits, the reference's own test
vectors (every parse test there also writes), and plain integer arithmetic."""
import struct

import numpy as np
import pytest

import kat_runner
import kats_packets as K
from test_gpu_parity import ipfix_msg, ipfix_set, nf_msg, tmpl, vl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE, WIRE, HOST, UNWRITABLE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.wire import FlowWire  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def encode(dgrams, how=None, align4=False, codec=None):
    """Decode `dgrams` as one batch and encode it: guard, offsets and stats as specified, `how` as constructed
    (None: WIRE / HOST / NONE by the decode's status and the input's set ids), every WIRE message equal to
    the host function's.  Returns (batch, stage, messages per datagram: the device's, else the host's)."""
    from netgauze_amd import _lib
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.wire import FlowWire
    batch, fw = (codec or FlowInfoCodec(0)).decode_datagrams(dgrams), FlowWire(align4=align4)
    st = fw.encode(batch)
    data, offs, got = fw.result(guard=True)
    offs, got = offs.tolist(), got.tolist()
    assert data[offs[-1]:] == b"\xA5" * _lib.NGZ_OUTPUT_GUARD and offs[0] == 0 and offs == sorted(offs) and st["bytes"] == offs[-1]
    if how is None:
        def has_template(d):
            pos, ids = 16 if d[1] == 10 else 20, []
            while pos + 4 <= len(d):
                ids.append(struct.unpack_from(">H", d, pos)[0])
                pos += max(4, struct.unpack_from(">H", d, pos + 2)[0])
            return any(i < 4 for i in ids)
        how = [NONE if s else HOST if has_template(d) else WIRE for d, s in zip(dgrams, batch.dgram_headers()["status"].tolist())]
    assert got == how
    assert st == dict(wire=how.count(WIRE), bytes=offs[-1], left_template=how.count(HOST), unwritable=how.count(UNWRITABLE), not_ok=how.count(NONE))
    host = [batch.dgram_wire(d, align4) for d in range(len(dgrams))]
    for d, h in enumerate(how):
        assert data[offs[d]:offs[d + 1]] == (host[d] if h == WIRE else b""), d
        assert (host[d] is not None) == (h in (WIRE, HOST)), d
    return batch, fw, host


def canonical(rec, fields):
    """The synthetic records with the high byte of a two-byte tcpControlBits zero: TCPHeaderFlags keeps the low
    byte only (iana/src/tcp.rs:165-168), so the reference's writer, too, gives the field back that way."""
    from netgauze_amd import synth
    for (ie, ln), o in zip(fields, synth.field_offsets(fields)[0]):
        if (ie, ln) == (6, 2):
            rec[:, o] = 0
    return rec


def t20_stream(per_msg):
    from netgauze_amd import synth
    buf, offs, lens = synth.ipfix_data_stream(canonical(synth.t20_records(2 * per_msg + 1), synth.T20), 64, rec_per_msg=per_msg)
    b = bytes(buf.numpy())
    return [synth.template_message()] + [b[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())]


def mixed():
    """Messages of the eight config-3 templates, then one datagram with sets of four of them."""
    from netgauze_amd import synth
    buf, offs, lens, recs = synth.mixed_stream(8 * 70)
    b = bytearray(buf.numpy().tobytes())
    sets = []
    for tid, fields in synth.CFG3_TEMPLATES:
        rl = synth.field_offsets(fields)[1]
        r = canonical(recs[tid].numpy().copy(), fields)
        sets.append(ipfix_set(tid, r[:3].tobytes()))
        for o, n in zip(offs.tolist(), lens.tolist()):
            if struct.unpack_from(">H", b, o + 16)[0] == tid:
                k = (n - 20) // rl
                b[o + 20:o + n] = r[:k].tobytes()  # one message per template at this size
    return [synth.templates_message(synth.CFG3_TEMPLATES)] + [bytes(b[o:o + n]) for o, n in zip(offs.tolist(), lens.tolist())] + \
        [ipfix_msg(sets[:4] + sets[2:3])]


def cfg4():
    """Config 4 (NFv9, and IPFIX with variable-length fields).  Its generator gives every 97th record's first
    variable-length value the three-byte length escape; the writer's prefix for these short values is one
    byte, so the expected message has ff 00 00 ll cut to ll and its two lengths three bytes shorter."""
    from netgauze_amd import synth
    dgrams, lay = synth.cfg4_datagrams(400, layout=True)
    exp, starts, firsts = list(dgrams), np.concatenate([[0], np.cumsum(lay["rec_len"])]), lay["v_first"] + [len(lay["rec_len"])]
    for m, pos in enumerate(lay["v_pos"]):
        recs = [lay["flat"][starts[r]:starts[r + 1]].tobytes() for r in range(firsts[m], firsts[m + 1])]
        body = b"".join(r[:8] + r[11:] if (firsts[m] + i) % 97 == 0 else r for i, r in enumerate(recs))
        exp[pos] = struct.pack(">HH", 10, 20 + len(body)) + dgrams[pos][4:16] + struct.pack(">HH", synth.V900_ID, 4 + len(body)) + body
    return dgrams, exp


@pytest.mark.parametrize("stream", [lambda: t20_stream(1), lambda: t20_stream(63), lambda: t20_stream(64), lambda: t20_stream(65),
                                    lambda: t20_stream(1023), mixed, cfg4], ids=["t20-1", "t20-63", "t20-64", "t20-65", "t20-1023", "mixed", "cfg4"])
def test_identity(dev, stream):
    """Input that is already what the writer emits comes back byte for byte, template messages included."""
    out = stream()
    dgrams, exp = out if isinstance(out, tuple) else (out, out)
    _batch, _fw, host = encode(dgrams)
    assert host == exp


def test_launches_do_not_depend_on_slots(dev):
    from netgauze_amd import synth
    one, eight = t20_stream(65), mixed()
    assert encode(one)[1].last_launches == encode(eight)[1].last_launches
    assert len(synth.CFG3_TEMPLATES) == 8


def test_one_handle_across_batches(dev):
    """One codec and one stage handle over batches of different shape, large, small, large again: after each
    encode the bytes with their guard, the offsets, `how`, the stats and the launches are those of a fresh
    handle on the same batch, whatever the handle's buffers held before."""
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.wire import FlowWire
    codec, fw = FlowInfoCodec(0), FlowWire()
    streams = {65: t20_stream(65), 1: t20_stream(1)}
    for per_msg in (65, 1, 65):
        batch = codec.decode_datagrams(streams[per_msg])
        got, fresh = [], FlowWire()
        for h in (fw, fresh):
            st = h.encode(batch)
            data, offs, how = h.result(guard=True)
            got.append((data, offs.tolist(), how.tolist(), st, h.last_launches))
        assert got[0] == got[1], per_msg
        assert got[0][2] == [HOST] + [WIRE] * (len(streams[per_msg]) - 1) and got[0][3]["bytes"] == got[0][1][-1] > 0
        assert got[0][0][:got[0][1][-1]] == b"".join(streams[per_msg][1:])  # the input is what the writer emits (test_identity)


# Vectors of kats_packets.CASES the reference parses but does not write back, by wire key: what K.CASES itself
# does not mark.  For these the test holds the device to the host function only.
NOT_WRITTEN_BACK = {
    K.B: "serde_benchmark.rs: a benchmark's inputs; no test_write runs over them",  # a key prefix
    K.W + "test_example:good_wire": "ipfix.rs:514: test_write is commented out there (its options template set is padded)",
}


def written_back(key):
    return not any(isinstance(key, str) and key.startswith(k) for k in NOT_WRITTEN_BACK)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_reference_vectors(dev, name):
    """Every vector the reference parses completely it also writes back (test_write* beside each parse in
    wire/tests/*.rs; NOT_WRITTEN_BACK lists the exceptions): the written message is the vector, for NetFlow v9
    under one of the writer's two padding settings (netflow.rs tests write with either).  Item-level vectors
    are wrapped into a message as the parse tests of this suite wrap them."""
    from netgauze_amd.flow import FlowInfoCodec
    for m in K.CASES[name]:
        codec = FlowInfoCodec(0)
        pre, steps = kat_runner.codec_datagrams(m)
        if pre:
            codec.decode_datagrams(pre)
        for (_i, dgram), (kind, key, _exp) in zip(steps, m["steps"]):
            batch = codec.decode_datagrams([dgram])
            if int(batch.dgram_headers()[0]["status"]) != 0:
                continue
            _b, _fw, host = encode([dgram], codec=codec)
            if written_back(key):
                assert dgram in ((host[0], batch.dgram_wire(0, True)) if kind.startswith("nf9") else (host[0],)), (name, key)


def normalising():
    """IPFIX set padding; three-byte length prefixes on short values; a fixed string with bytes after its NUL;
    NTP fractions; reduced-size integers and a two-byte tcpControlBits."""
    fields = [(82, 65535), (83, 8), (154, 8), (156, 8), (1, 3), (6, 2), (313, 65535)]
    rec = lambda i: (b"\xff\0\0\3abc" + b"ab\0cd\0ef" + struct.pack(">IIII", 1_700_000_000, (1, 0x80000000, 0xFFFFFF00)[i], 1_700_000_001 + i,  # noqa: E731
                                                                       (12345, 0xFFFFFFF0, 7)[i]) + bytes([1, 2, i]) + bytes([0xAB, 0x12 + i]) +
                     vl(bytes([i]) * (254 + i)))
    return [ipfix_msg([ipfix_set(2, tmpl(500, fields))]), ipfix_msg([ipfix_set(500, b"".join(rec(i) for i in range(3)) + b"\0\0")])]


def test_normalising_input(dev):
    """Decoding the output again gives the first decode's cells; the written fraction of a micro- / nanosecond
    field is nanos * (2^32 - 1) // 10^9 of the first decode's nanos."""
    dgrams = normalising()
    batch, _fw, host = encode(dgrams, [HOST, WIRE])
    assert len(host[1]) == len(dgrams[1]) - 2 - 3 * 3  # no padding, one-byte prefixes
    assert host[1][20:32] == b"\x03abc" + b"ab\0\0\0\0\0\0" and host[1][48:53] == bytes([1, 2, 0, 0, 0x12])
    again, _fw2, _host2 = encode(host, [HOST, WIRE])
    s0, s1 = batch.slots[0], again.slots[0]
    for f in range(len(s0.fields)):
        a, b = s0.column_bytes(f, rows=3), s1.column_bytes(f, rows=3)
        if f in (2, 3):  # {u32 secs, u32 nanos}
            first = np.frombuffer(bytes(a), dtype="<u4").reshape(3, 2)
            at = 20 + 4 + 8 + 8 * (f - 2)  # the field in the first record: after the headers, "\x03abc" and the string
            assert struct.unpack_from(">II", host[1], at) == (int(first[0, 0]), int(first[0, 1]) * (2 ** 32 - 1) // 10 ** 9)
            assert np.array_equal(np.frombuffer(bytes(b), dtype="<u4").reshape(3, 2)[:, 0], first[:, 0])
        elif f in (0, 6):  # {offset, length}: the lengths
            assert np.array_equal(np.frombuffer(bytes(a), dtype="<u4").reshape(3, 4)[:, 2], np.frombuffer(bytes(b), dtype="<u4").reshape(3, 4)[:, 2])
        elif f == 1:  # a fixed string's cell keeps the raw bytes: the value is what stands before the first NUL
            assert [bytes(r).split(b"\0")[0] for r in a] == [bytes(r).split(b"\0")[0] for r in b] == [b"ab"] * 3
        else:
            assert bytes(a) == bytes(b), f


A = [(8, 4), (7, 2)]
rec_a = lambda i: struct.pack(">IH", 0x0A000000 + i, i)  # noqa: E731
NF_T = struct.pack(">HH", 0, 4 + 4 + 12) + struct.pack(">HH", 260, 3) + struct.pack(">HHHHHH", 8, 4, 7, 2, 6, 1)
NF_BAD = struct.pack(">HH", 0, 4 + 4 + 4) + struct.pack(">HH", 261, 1) + struct.pack(">HH", 95, 65535)  # a literal 65535 bytes
nf_rec = struct.pack(">IHB", 0x0A000001, 80, 0x12)
EDGES = {
    "long-record": ([ipfix_msg([ipfix_set(2, tmpl(420, [(313, 65535), (7, 2)]))]),
                     ipfix_msg([ipfix_set(420, vl(b"s") + b"\0\1" + vl(b"\xc8" * 20000) + b"\0\2" + vl(b"") + b"\0\3"),
                                ipfix_set(420, b"".join(vl(bytes([i]) * 300) + struct.pack(">H", i) for i in range(64)))])], [HOST, WIRE], False),
    "empty": ([ipfix_msg([ipfix_set(2, tmpl(300, A))]), ipfix_msg([]), ipfix_msg([ipfix_set(300, b"")]),
               ipfix_msg([ipfix_set(300, b""), ipfix_set(300, rec_a(1))])], [HOST, WIRE, WIRE, WIRE], False),
    "failed-between": ([ipfix_msg([ipfix_set(2, tmpl(300, A))]), ipfix_msg([ipfix_set(300, rec_a(1) * 65)]), ipfix_msg([ipfix_set(999, b"\0" * 8)]),
                        b"\x00\x0a\x00", ipfix_msg([ipfix_set(300, rec_a(2))])], [HOST, WIRE, NONE, NONE, WIRE], False),
    "refused-template": ([ipfix_msg([ipfix_set(2, tmpl(300, A) + tmpl(310, [(70, 4)]))]),  # an MPLS label of four bytes: stored, refused per record
                          ipfix_msg([ipfix_set(310, b"\0\0\1\1")]), ipfix_msg([ipfix_set(300, rec_a(1))])], [HOST, NONE, WIRE], False),
    "unwritable": ([nf_msg([NF_T, NF_BAD], count=2), nf_msg([struct.pack(">HH", 261, 4)], count=1),
                    nf_msg([struct.pack(">HH", 260, 4 + 7 + 1) + nf_rec + b"\0"], count=1),
                    nf_msg([struct.pack(">HH", 260, 4 + 7 + 1) + nf_rec + b"\0", struct.pack(">HH", 261, 4)], count=2)],
                   [HOST, UNWRITABLE, WIRE, UNWRITABLE], False),
    "nfv9-align": ([nf_msg([NF_T], count=1), nf_msg([struct.pack(">HH", 260, 4 + 7 * 3 + 3) + nf_rec * 3 + b"\0\0\0"], count=3),
                    nf_msg([struct.pack(">HH", 260, 4 + 7 * 4) + nf_rec * 4, struct.pack(">HH", 260, 4 + 7 + 1) + nf_rec + b"\0"], count=5)],
                   [HOST, WIRE, WIRE], True),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_edges(dev, case):
    dgrams, how, align4 = EDGES[case]
    _batch, _fw, host = encode(dgrams, how, align4)
    if case == "nfv9-align":  # length % 4 zero bytes, counted in the set's length (netflow.rs:133-134 as written)
        assert host[1][20:24] == struct.pack(">HH", 260, 25 + 1) and len(host[1]) == 20 + 26
        assert len(host[2]) == 20 + 32 + (11 + 3)
    elif case != "unwritable":  # canonical input
        assert [h for h in host if h is not None] == [d for d, h in zip(dgrams, how) if h != NONE]


def test_after_renormalization(dev):
    """A sampled batch: the counts in the written records are the scaled columns, every other byte the input's."""
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.renormalize import FlowRenormalizer
    from netgauze_amd.wire import FlowWire
    fields = [(8, 4), (1, 8), (2, 4), (34, 4), (7, 2)]  # octets, packets, samplingInterval
    recs = [struct.pack(">IQIIH", 0x0A000000 + i, 1000 + i, 10 + i, 1 + i % 5, i) for i in range(70)]
    dgrams = [ipfix_msg([ipfix_set(2, tmpl(300, fields))]), ipfix_msg([ipfix_set(300, b"".join(recs))])]
    batch = FlowInfoCodec(0).decode_datagrams(dgrams)
    assert FlowRenormalizer(0).apply(batch)["flows_renormalized"] > 0
    octets = np.frombuffer(bytes(batch.slots[0].column_bytes(1, rows=70)), dtype="<u8")
    packets = np.frombuffer(bytes(batch.slots[0].column_bytes(2, rows=70)), dtype="<u8")
    assert int(octets[4]) == 1004 * 5 and int(packets[4]) == 14 * 5
    fw = FlowWire()
    fw.encode(batch)
    data, offs, how = fw.result()
    assert how.tolist() == [HOST, WIRE] and data == batch.dgram_wire(1)
    exp = b"".join(struct.pack(">IQIIH", 0x0A000000 + i, int(octets[i]), int(packets[i]), 1 + i % 5, i) for i in range(70))
    assert data == dgrams[1][:20] + exp
