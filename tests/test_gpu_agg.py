"""GPU parity of the device flow aggregation (include/ngz/flow_aggregate.h) against
oracle/ngz_agg_oracle.py, a restatement of the collector's FlowAggregator /
WindowAggregator (aggregator.rs:68-354, analytics/src/aggregation.rs:124-185),
pinned by the reference's aggregation unit tests (tests/kats_agg.py).

Every comparison is exact: group set, key values, aggregated values (adds wrap at the
IE's Rust width), record counts, export/collection time bounds, sys-up time and the
template / port / observation-domain sets -- for the windows each push closes
(ngz_agg_emit, aggregation.rs:154-160) and for the final flush."""
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_io  # noqa: E402
import kats_agg as K  # noqa: E402
import ngz_agg_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, ADD, MN, MX, OR = K.OP_KEY, K.OP_ADD, K.OP_MIN, K.OP_MAX, K.OP_OR
# ngz_agg_set_option values a test forces on every aggregator it creates (monkeypatch.setitem);
# they choose the reduction path, never the result
AGG_OPTIONS = {}


def new_agg(*args, **kw):
    from netgauze_amd.aggregate import FlowAggregator
    return FlowAggregator(*args, options=dict(AGG_OPTIONS), **kw)


def _opt(name):
    from netgauze_amd import _lib
    return getattr(_lib, name)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.aggregate import FlowAggregator  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def ipfix_msg(sets, export_time, seq=1, domain=7):
    body = b"".join(sets)
    return struct.pack(">HHIII", 10, 16 + len(body), export_time, seq, domain) + body


def tset(tid, fields):
    body = struct.pack(">HH", tid, len(fields)) + b"".join(struct.pack(">HH", i, n) for i, n in fields)
    return struct.pack(">HH", 2, 4 + len(body)) + body


def dset(tid, recs):
    body = b"".join(recs)
    return struct.pack(">HH", tid, 4 + len(body)) + body


def _exact(v):
    # floats by bit pattern (-0 vs +0), every NaN alike (the NaN an x86 and a GPU add produce
    # differ in sign; serde renders every NaN as null)
    if isinstance(v, float):
        return b"NaN" if v != v else struct.pack("<d", v)
    return v


def norm(groups):
    out = {}
    for g in groups:
        k = (g["peer"], g["window_start"], g["flow_type"], tuple(_exact(x) for x in g["key"]))
        assert k not in out, k
        out[k] = (tuple(_exact(v) for v in g["vals"]), g["record_count"], g["min_export"], g["max_export"],
                  g["max_sysup"],
                  g["min_coll"], g["max_coll"], frozenset(g["templates"]), frozenset(g["ports"]),
                  frozenset(g["domains"]))
    return out


def run_device(fields, batches, port=4739, coll=1_700_000_000_000, lateness_s=10, capacity=1 << 16):
    """batches: list of lists of datagrams, decoded in order on one codec (one peer).
    Returns (groups emitted after each push, groups of the final flush, late records)."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    codec = FlowInfoCodec()
    # one peer: 8 peer bits (max_peers 256) keep keys up to 35 bits in the exact packed tag
    agg = new_agg(fields, lateness_s=lateness_s, capacity=capacity, max_peers=256)
    late = 0
    emitted = []
    for b in batches:
        batch = codec.decode_datagrams(b)
        late += agg.push(batch, port, coll)
        emitted.append(agg.emit())
    groups = agg.flush()
    assert agg.n_groups() == 0
    agg.close()
    codec.close()
    return emitted, groups, late


def run_oracle(fields, batches, port=4739, coll=1_700_000_000_000, lateness_s=10):
    import ngz_oracle as O
    codec = O.FlowInfoCodec()
    o = A.FlowAggregatorOracle(fields, 60, lateness_s)
    emitted = []
    for b in batches:
        for d in b:
            try:
                pkt = codec.decode(bytearray(d))
            except O.ParseFail:
                continue
            if pkt is not None:
                o.push_packet(pkt, port, coll)
        emitted.append(o.emit())
    return emitted, o.flush(), o.late


def same_groups(a, b):
    a, b = norm(a), norm(b)
    assert set(a) == set(b), (len(a), len(b), sorted(set(a) ^ set(b))[:5])
    for k in b:
        assert a[k] == b[k], (k, a[k], b[k])


def check(fields, batches, **kw):
    e_dev, g_dev, late_dev = run_device(fields, batches, **kw)
    kw.pop("capacity", None)
    e_ref, g_ref, late_ref = run_oracle(fields, batches, **kw)
    assert late_dev == late_ref
    for a, b in zip(e_dev, e_ref):  # the windows each push closed
        same_groups(a, b)
    same_groups(g_dev, g_ref)
    return [g for e in e_dev for g in e] + g_dev


def test_kat_repeating_ie_fields(dev):
    d = [ipfix_msg([tset(400, K.REPEAT_TEMPLATE), dset(400, [K.REPEAT_RECORD])], K.T_2025_01_01_16, domain=300)]
    (g,) = check(K.REPEAT_FIELDS, [d])
    for k, v in K.REPEAT_EXPECTED.items():
        assert g[k] == v, k


def test_kat_missing_fields(dev):
    d = [ipfix_msg([tset(300, K.MISSING_TEMPLATE), dset(300, [K.MISSING_RECORD])], 1_700_000_000)]
    (g,) = check(K.MISSING_FIELDS, [d])
    for k, v in K.MISSING_EXPECTED.items():
        assert g[k] == v, k


def test_kat_reduce_operations(dev):
    d = [ipfix_msg([tset(256, K.REDUCE_TEMPLATE_1), tset(257, K.REDUCE_TEMPLATE_2),
                    dset(256, [K.REDUCE_WIRE_1]), dset(257, [K.REDUCE_WIRE_2])], 1_700_000_000)]
    (g,) = check(K.REDUCE_FIELDS, [d])
    assert g["vals"] == K.REDUCE_EXPECTED and g["record_count"] == 2


def test_wrapping_add_and_signed_min_max(dev):
    # u8 adds wrap (ipTTL-like unsigned8 IE 192 ipTTL), signed32 IE 434 (mibObjectValueInteger) min/max
    tpl = [(192, 1), (434, 4), (1, 8)]
    recs = [struct.pack(">BiQ", 200, -5, 1), struct.pack(">BiQ", 100, 7, 2), struct.pack(">BiQ", 250, -9, 3)]
    d = [ipfix_msg([tset(500, tpl), dset(500, recs)], 1_700_000_000)]
    fields = [(0, 192, 0, ADD), (0, 434, 0, MN), (0, 434, 0, MX), (0, 1, 0, ADD)]
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    codec = FlowInfoCodec()
    agg = new_agg(fields)
    agg.push(codec.decode_datagrams(d))
    (g,) = agg.flush()
    assert g["vals"] == ((200 + 100 + 250) & 0xFF, -9, 7, 6)
    o = A.aggregate_datagrams(fields, d).flush()
    assert o[0]["vals"] == g["vals"]


def t20_datagrams(n, rec_per_msg, times, seed_first=0):
    from netgauze_amd import synth
    rec = synth.t20_records(n, first=seed_first)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64, rec_per_msg=rec_per_msg)
    b = bytes(buf.numpy())
    out = []
    for i, (o, ln) in enumerate(zip(offs.tolist(), lens.tolist())):
        m = bytearray(b[o:o + ln])
        m[4:8] = struct.pack(">I", times[i % len(times)] + 60 * (i // len(times)))
        out.append(bytes(m))
    return [synth.template_message()] + out


T20_AGG = [(0, 1, 0, ADD), (0, 2, 0, ADD), (0, 6, 0, OR), (0, 22, 0, MN), (0, 21, 0, MX), (0, 16, 0, MX),
           (0, 10, 0, MN)]


@pytest.mark.parametrize("keys", [
    [(0, 4, 0, OK), (0, 61, 0, OK)],                    # 6 groups per window: heavy atomic contention
    [(0, 11, 0, OK)],                                   # destination port: mostly singleton groups
    [(0, 8, 0, OK), (0, 12, 0, OK), (0, 7, 0, OK), (0, 11, 0, OK), (0, 4, 0, OK)],  # 5-tuple
])
def test_t20_groups_windows_lateness(dev, keys):
    """T20 messages whose export times go back and forth: late messages dropped, minute windows."""
    times = [1_700_000_010, 1_700_000_030, 1_700_000_015, 1_700_000_045, 1_700_000_020, 1_700_000_050,
             1_700_000_061, 1_700_000_049]
    d = t20_datagrams(6000, 100, times)
    g = check(keys + T20_AGG, [d[:25], d[25:]])
    assert len(g) > 1


def test_t20_multi_port_collection_times(dev):
    """Two pushes with different peer ports and collection times: port sets and collection bounds."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    keys = [(0, 4, 0, OK)]
    d = t20_datagrams(3000, 300, [1_700_000_000])
    codec = FlowInfoCodec()
    agg = new_agg(keys + T20_AGG)
    agg.push(codec.decode_datagrams(d[:6]), 1000, 5_000)
    agg.push(codec.decode_datagrams(d[6:]), 2000, 9_000)
    o = A.FlowAggregatorOracle(keys + T20_AGG)
    import ngz_oracle as O
    oc = O.FlowInfoCodec()
    for i, x in enumerate(d):
        pkt = oc.decode(bytearray(x))
        if pkt is not None:
            o.push_packet(pkt, 1000 if i < 6 else 2000, 5_000 if i < 6 else 9_000)
    assert norm(agg.emit() + agg.flush()) == norm(o.emit() + o.flush())


def peers_of(name):
    groups = {}
    for src, sp, dst, dp, payload in golden_io.datagrams(name):
        groups.setdefault((src, sp, dst, dp), []).append(payload)
    return groups


GOLDEN_AGG = [(0, 8, 0, OK), (0, 12, 0, OK), (0, 27, 0, OK), (0, 4, 0, OK), (0, 10, 0, OK),
              (0, 1, 0, ADD), (0, 2, 0, ADD), (0, 6, 0, OR), (0, 22, 0, MN), (0, 21, 0, MX), (0, 7, 0, MX),
              (0, 56, 0, OR)]


# a key that packs into the 63-bit tag (exact, no verify pass): protocol + source port
GOLDEN_AGG_PACKED = [(0, 4, 0, OK), (0, 7, 0, OK), (0, 1, 0, ADD), (0, 2, 0, ADD), (0, 6, 0, OR),
                     (0, 22, 0, MN), (0, 21, 0, MX)]


@pytest.mark.parametrize("fields", ["wide", "packed"])
@pytest.mark.parametrize("name", [c[0] for c in golden_io.cases()])
def test_reference_captures(dev, name, fields):
    """Every reference capture, per exporter peer (IPFIX and NetFlow v9, options data,
    several templates and observation domains), in two batches."""
    sel = GOLDEN_AGG if fields == "wide" else GOLDEN_AGG_PACKED
    for key, dgrams in peers_of(name).items():
        h = len(dgrams) // 2
        check(sel, [dgrams[:h], dgrams[h:]], port=key[1], lateness_s=60)


def test_wave_preaggregation_bytes_and_presence(dev):
    """Low-cardinality keys (wave pre-aggregation path) with a byte-wise OR (mac), a
    signed min and fields present in only one of two templates."""
    import random
    rnd = random.Random(7)
    t1 = [(8, 4), (56, 6), (1, 8), (434, 4)]
    t2 = [(8, 4), (2, 8)]
    r1 = [struct.pack(">I6sQi", rnd.choice([1, 2]), bytes(rnd.getrandbits(8) for _ in range(6)),
                      rnd.getrandbits(64), rnd.randint(-2**31, 2**31 - 1)) for _ in range(700)]
    r2 = [struct.pack(">IQ", rnd.choice([1, 2, 3]), rnd.getrandbits(64)) for _ in range(500)]
    d = [ipfix_msg([tset(600, t1), tset(601, t2)], 1_700_000_000)]
    for i in range(0, 700, 100):
        d.append(ipfix_msg([dset(600, r1[i:i + 100]), dset(601, r2[i:i + 100] if i < 500 else [])]
                           if i < 500 else [dset(600, r1[i:i + 100])], 1_700_000_000 + i // 100))
    fields = [(0, 8, 0, OK), (0, 56, 0, OR), (0, 1, 0, ADD), (0, 2, 0, MX), (0, 434, 0, MN)]
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    codec = FlowInfoCodec()
    agg = new_agg(fields)
    agg.push(codec.decode_datagrams(d))
    got = norm(agg.flush())
    ref = norm(A.aggregate_datagrams(fields, d, collection_ms=0).flush())
    assert set(got) == set(ref) and len(got) == 3
    for k in ref:
        assert got[k] == ref[k], (k, got[k], ref[k])


def test_table_full_and_flush_buffer_errors(dev):
    """More groups than the capacity report NGZ_AGG_E_OVERFLOW (no hang) and leave the
    aggregator as it was; a flush buffer that is too small is refused without emptying
    the table."""
    import numpy as np
    from netgauze_amd.aggregate import AggError, FlowAggregator, lib
    from netgauze_amd.flow import FlowInfoCodec
    d = t20_datagrams(5000, 500, [1_700_000_000])
    codec = FlowInfoCodec()
    agg = new_agg([(0, 8, 0, OK), (0, 12, 0, OK)] + T20_AGG, capacity=16)
    with pytest.raises(AggError, match="capacity|table full"):
        agg.push(codec.decode_datagrams(d))
    assert agg.n_groups() == 0 and agg.flush() == []
    agg2 = new_agg([(0, 4, 0, OK)] + T20_AGG)
    agg2.push(codec.decode_datagrams(d[:3]))
    n = agg2.n_groups()
    assert n == 6  # 3 protocols x 2 minute windows (the two data messages are 60 s apart)
    rb = agg2.layout()[0]
    buf = np.zeros(rb * n - 1, dtype=np.uint8)
    assert lib().ngz_agg_flush(agg2._h, buf.ctypes.data, buf.nbytes) == -1  # NGZ_E_INVALID
    assert agg2.n_groups() == n
    assert len(agg2.flush()) == n and agg2.n_groups() == 0


def test_kat_netflowv9_explode(dev):
    (g,) = check(K.NF_FIELDS, [[K.nf_packet()]], port=9995, coll=K.T_2025_01_01_10_MS)
    for k, v in K.NF_EXPECTED.items():
        assert g[k] == v, k


def test_flow_type_separates_groups(dev):
    """The same key exported over NetFlow v9 and IPFIX by one peer makes two groups
    (FlowCacheKey.flow_type; reference test_aggregator_push_netflowv9_and_ipfix_different_flow_types,
    aggregator/tests.rs:1179-1262)."""
    ipfix = ipfix_msg([tset(256, K.NF_TEMPLATE), dset(256, [K.NF_RECORD, K.NF_RECORD])], K.T_2025_01_01_12,
                      domain=100)
    g = check(K.NF_FIELDS, [[K.nf_packet(), ipfix]], port=9995, coll=K.T_2025_01_01_10_MS)
    assert sorted((x["flow_type"], x["record_count"], x["vals"]) for x in g) == [(9, 1, (1000, 10)),
                                                                                 (10, 2, (2000, 20))]


FIVE_TUPLE = [(0, 8, 0, OK), (0, 12, 0, OK), (0, 7, 0, OK), (0, 11, 0, OK), (0, 4, 0, OK)]


def test_hash_collisions_stay_exact(dev, monkeypatch):
    """A 3-bit key hash makes nearly every distinct 5-tuple collide: groups are still exact
    (keys compared, collided records re-probed), where the previous design returned
    NGZ_AGG_E_COLLISION."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_HASH_BITS"), 3)
    d = t20_datagrams(3000, 100, [1_700_000_010, 1_700_000_070])
    g = check(FIVE_TUPLE + T20_AGG, [d[:10], d[10:]])
    assert len(g) > 1000


def test_string_key_declared_at_two_lengths(dev):
    """interfaceName "eth0" in a 16- and a 32-byte fixed string field is one key: the reference
    compares the NUL-truncated Field::String (generator.rs:1654-1669)."""
    t1, t2 = [(82, 16), (1, 8)], [(82, 32), (1, 8)]
    r1 = [b"eth0".ljust(16, b"\0") + struct.pack(">Q", 5)]
    r2 = [b"eth0".ljust(32, b"\0") + struct.pack(">Q", 7), b"eth1".ljust(32, b"\0") + struct.pack(">Q", 1)]
    d = [ipfix_msg([tset(700, t1), tset(701, t2), dset(700, r1), dset(701, r2)], 1_700_000_000)]
    g = check([(0, 82, 0, OK), (0, 1, 0, ADD)], [d])
    assert sorted((x["key"], x["vals"], x["record_count"]) for x in g) == [(("eth0",), (12,), 2), (("eth1",), (1,), 1)]


def test_octet_key_lengths_are_part_of_the_key(dev):
    """An octetArray key is a Box<[u8]>: [1,2,3,4] and [1,2,3,4,0,0] are different keys."""
    t1, t2 = [(95, 4), (1, 8)], [(95, 6), (1, 8)]
    d = [ipfix_msg([tset(710, t1), tset(711, t2), dset(710, [b"\x01\x02\x03\x04" + struct.pack(">Q", 1)]),
                    dset(711, [b"\x01\x02\x03\x04\x00\x00" + struct.pack(">Q", 2)])], 1_700_000_000)]
    g = check([(0, 95, 0, OK), (0, 1, 0, ADD)], [d])
    assert sorted(x["key"] for x in g) == [(b"\x01\x02\x03\x04",), (b"\x01\x02\x03\x04\x00\x00",)]


def test_peer_ports_across_flush_cycles(dev):
    """More than 64 distinct peer ports over the aggregator's life: the set dictionaries start
    over at every flush, so only 64 live ones are a limit (the reference sets are unbounded)."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    d = t20_datagrams(200, 100, [1_700_000_000])  # two data messages, one minute apart
    codec = FlowInfoCodec()
    agg = new_agg([(0, 4, 0, OK), (0, 1, 0, ADD)], lateness_s=60)  # nothing late, no window closes
    for cycle in range(8):
        for i in range(10):
            agg.push(codec.decode_datagrams(d), 10000 + 10 * cycle + i, 0)
        out = agg.flush()
        assert out and all(x["ports"] == {10000 + 10 * cycle + i for i in range(10)} for x in out)


def test_closed_windows_free_dictionary_entries(dev):
    """A long stream whose export time moves on: each push closes the previous windows
    (emitted, aggregation.rs:154-160), their ports / templates / domains no longer count,
    and a stream with 100 distinct ports never overflows a 64-entry dictionary."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    fields = [(0, 4, 0, OK), (0, 1, 0, ADD), (0, 2, 0, MX)]
    codec, oc = FlowInfoCodec(), O.FlowInfoCodec()
    agg = new_agg(fields, lateness_s=10, capacity=64)
    o = A.FlowAggregatorOracle(fields, 60, 10)
    tmpl = t20_datagrams(100, 100, [1_700_000_000])[0]
    oc.decode(bytearray(tmpl))
    codec.decode_datagrams([tmpl])
    for i in range(100):
        d = t20_datagrams(300, 100, [1_700_000_000 + 120 * i], seed_first=1000 * i)[1:]
        agg.push(codec.decode_datagrams(d), 20000 + i, i)
        for x in d:
            o.push_packet(oc.decode(bytearray(x)), 20000 + i, i)
        same_groups(agg.emit(), o.emit())
    same_groups(agg.flush(), o.flush())


def long_key_datagrams(names, export_time, template=False):
    """interfaceName sent variable-length, one record per name (names longer than 32 bytes keep
    their tails in the byte arena)."""
    recs = [_vlen(n.encode()) + struct.pack(">Q", i + 1) for i, n in enumerate(names)]
    return [ipfix_msg(([tset(256, [(82, 0xFFFF), (1, 8)])] if template else []) + [dset(256, recs)], export_time)]


@pytest.mark.parametrize("case", ["general", "long_byte_keys", "lowcard_by_size", "lowcard_forced"])
def test_failed_push_leaves_the_aggregator_unchanged(dev, case, monkeypatch):
    """A push that would exceed the capacity fails without touching the groups, the set
    dictionaries or the event time, and a valid push after it is taken: the flush afterwards
    equals the oracle of the pushes that succeeded.  With a byte key of more than 32 bytes the
    refused push's key tails are given back to the arena (the third push's new tails land where
    they would have without it); with a packed key and NGZ_AGG_OPT_LOWCARD 1 the refusal comes
    out of k_agg_lc_merge."""
    from netgauze_amd.aggregate import AggError
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    if case == "long_byte_keys":
        fields = [(0, 82, 0, OK), (0, 1, 0, ADD)]
        name = "interface-%04d-with-a-name-longer-than-thirty-two-bytes-%s"
        a = long_key_datagrams([name % (j, "a") for j in range(60)], 1_700_000_000, template=True)
        b = long_key_datagrams([name % (j, "b") for j in range(300)], 1_700_000_010)
        # in a's window: eight new keys, eight of a's
        c = long_key_datagrams([name % (j, "c" if j % 2 else "a") for j in range(16)], 1_700_000_020)
        room = 10
    else:
        lowcard = case.startswith("lowcard")
        # lowcard: protocol + direction, a packed key of 6 tuples per window
        fields = ([(0, 4, 0, OK), (0, 61, 0, OK)] if lowcard else [(0, 11, 0, OK)]) + T20_AGG
        if lowcard:
            monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_LOWCARD"), 1 if case == "lowcard_forced" else -1)
        a = t20_datagrams(400, 100, [1_700_000_000])
        # lowcard: six more windows of 6 groups; general: thousands of destination ports
        b = t20_datagrams(600 if lowcard else 4000, 100, [1_700_000_030 + (600 if lowcard else 0)], seed_first=777)[1:]
        c = a[-1:]  # the newest message again: its groups' values move on
        room = 3 if lowcard else 10
    codec, oc = FlowInfoCodec(), O.FlowInfoCodec()
    o = A.aggregate_datagrams(fields, a, peer_port=1, collection_ms=5, codec=oc)
    n_a = len(o.groups) + len(o.closed)
    agg = new_agg(fields, capacity=n_a + room)
    agg.push(codec.decode_datagrams(a), 1, 5)
    if case == "lowcard_forced":
        assert agg.last_path() == "lowcard"
    with pytest.raises(AggError, match="capacity|table full"):
        agg.push(codec.decode_datagrams(b), 2, 9)
    assert agg.n_groups() == n_a
    # the refusal came out of the path meant: the general path names itself before it claims
    assert agg.last_path() == ("none" if case == "lowcard_forced" else "general")
    agg.push(codec.decode_datagrams(c), 1, 7)
    if case == "lowcard_forced":
        assert agg.last_path() == "lowcard"
    A.aggregate_datagrams(fields, c, 1, 7, agg=o, codec=oc)
    assert agg.n_groups() == len(o.groups) + len(o.closed)
    got = agg.emit() + agg.flush()
    same_groups(got, o.emit() + o.flush())
    assert all(g["ports"] == {1} for g in got)
    if case == "long_byte_keys":
        assert sum(len(g["key"][0]) > 32 for g in got) == 60 + 8


def test_peer_limit_refusal_keeps_the_aggregator(dev):
    """A push from a third peer IP with max_peers 2 is refused before anything else is touched:
    the groups stay, the two peers keep their entries and a push from one of them is taken; the
    flush equals the oracle of the pushes that succeeded and names two peers."""
    from netgauze_amd.aggregate import AggError
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    fields = [(0, 4, 0, OK)] + T20_AGG
    d = t20_datagrams(300, 100, [1_700_000_000])
    ips = ["10.0.0.1", "2001:db8::2", "10.0.0.3"]
    agg = new_agg(fields, max_peers=2)
    o = A.FlowAggregatorOracle(fields, 60, 10)
    codecs, ocodecs = [FlowInfoCodec() for _ in ips], [O.FlowInfoCodec() for _ in ips]
    for i in (0, 1):
        agg.push(codecs[i].decode_datagrams(d[:3]), 4739, 5, peer_ip=ips[i])
        A.aggregate_datagrams(fields, d[:3], 4739, 5, peer_ip=ips[i], agg=o, codec=ocodecs[i])
    n = agg.n_groups()
    assert n == len(o.groups) + len(o.closed) and n > 0
    with pytest.raises(AggError, match="max_peers"):
        agg.push(codecs[2].decode_datagrams(d), 4739, 5, peer_ip=ips[2])
    assert agg.n_groups() == n
    agg.push(codecs[0].decode_datagrams(d[3:]), 4739, 6, peer_ip=ips[0])
    A.aggregate_datagrams(fields, d[3:], 4739, 6, peer_ip=ips[0], agg=o, codec=ocodecs[0])
    same_groups(agg.emit() + agg.flush(), o.emit() + o.flush())
    assert len(agg.peers()) == 2


def test_plan_refusal_after_dictionary_insertions(dev):
    """A batch whose template the aggregator cannot take is refused after the push gave its new
    peer port and template id dictionary entries and fixed the first key's width at first sight:
    all of it is taken back.  Decode fixes a column's width by the IE's type, so no IE arrives at
    two widths; the refusal used is "fixed-size key field sent variable-length": template 257
    declares mplsTopLabelStackSection (a [u8; 3] octetArray, which the template parser takes at
    any length) 4 bytes long, so its records fail to decode.  layout() is as before, a further
    push (a third template, a third port) is taken, the flush equals the oracle of the pushes
    that succeeded, and its sets hold neither template 257 nor port 5000."""
    from netgauze_amd.aggregate import AggError
    from netgauze_amd.flow import FlowInfoCodec
    import kat_runner as KR
    import kats_packets as KP
    import ngz_oracle as O
    fields = [(0, 7, 0, OK), (0, 4, 0, OK), (0, 70, 0, OK), (0, 1, 0, ADD)]
    port_s, proto, octets = (KP.S("sourceTransportPort", 2), KP.S("protocolIdentifier", 1),
                             KP.S("octetDeltaCount", 8))
    tpl = lambda tid, *specs: KR.template_datagram(10, tid, (), specs)  # noqa: E731  (observation domain 0)
    data = lambda tid, recs, t: ipfix_msg([dset(tid, recs)], t, domain=0)  # noqa: E731
    p1 = [tpl(256, proto, octets), data(256, [struct.pack(">BQ", 6 + j % 2, j + 1) for j in range(40)], 1_700_000_000)]
    bad = [tpl(257, port_s, proto, KP.S("mplsTopLabelStackSection", 4), octets),
           data(257, [struct.pack(">HB4sQ", 80 + j, 6, b"\0\1\2\3", j + 1) for j in range(40)], 1_700_000_010)]
    p3 = [tpl(258, port_s, proto, octets),
          data(258, [struct.pack(">HBQ", 80 + j % 5, 6 + j % 2, j + 1) for j in range(40)], 1_700_000_020),
          data(256, [struct.pack(">BQ", 17, j + 1) for j in range(10)], 1_700_000_020)]
    codec, oc = FlowInfoCodec(), O.FlowInfoCodec()
    agg = new_agg(fields, max_peers=256)
    agg.push(codec.decode_datagrams(p1), 4739, 5)
    o = A.aggregate_datagrams(fields, p1, 4739, 5, codec=oc)
    layout, n = agg.layout(), agg.n_groups()
    assert layout[2] == [0, 1, 0]  # sourceTransportPort not seen yet
    with pytest.raises(AggError, match="fixed-size key field sent variable-length"):
        agg.push(codec.decode_datagrams(bad), 5000, 6)
    assert agg.layout() == layout and agg.n_groups() == n
    agg.push(codec.decode_datagrams(p3), 4740, 7)
    A.aggregate_datagrams(fields, p3, 4740, 7, agg=o, codec=oc)
    assert agg.layout()[2] == [2, 1, 0]
    got = agg.flush()
    same_groups(got, o.flush())
    templates, ports, _domains = agg.sets()
    assert {t & 0xFFFF for t in templates if t != 0xFFFFFFFF} == {256, 258}
    assert {p for p in ports if p != 0xFFFF} == {4739, 4740}


def test_ordered_reductions(dev):
    """Reductions whose result depends on record order or on a Rust Ord the atomics do not
    have: float64 Add / Min / Max (OrderedFloat: NaN greatest, -0 == +0 with min keeping the
    group's value and max taking the record's), IPv6 Min / Max, and Min / Max over a
    sub-registry enum (protocolIdentifier: Unassigned values after every registered one) and
    TCPHeaderFlags (FIN most significant).  Two pushes: the second folds into the first's values."""
    import random
    rnd = random.Random(11)
    tpl = [(8, 4), (311, 8), (27, 16), (4, 1), (6, 1)]
    specials = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-300, 1.5, -2.25, 3.0e10]

    def rec():
        f = rnd.choice(specials) if rnd.random() < 0.5 else rnd.uniform(-1e6, 1e6)
        return struct.pack(">Id16sBB", rnd.choice([1, 2, 3]), f, bytes(rnd.getrandbits(8) for _ in range(16)),
                           rnd.choice([6, 17, 147, 148, 200, 255]), rnd.getrandbits(8))
    d1 = [ipfix_msg([tset(720, tpl), dset(720, [rec() for _ in range(300)])], 1_700_000_000)]
    d2 = [ipfix_msg([dset(720, [rec() for _ in range(300)])], 1_700_000_001) for _ in range(3)]
    fields = [(0, 8, 0, OK), (0, 311, 0, ADD), (0, 311, 0, MN), (0, 311, 0, MX), (0, 27, 0, MN), (0, 27, 0, MX),
              (0, 4, 0, MN), (0, 4, 0, MX), (0, 6, 0, MN), (0, 6, 0, MX)]
    g = check(fields, [d1, d2])
    assert len(g) == 3


def test_flowinfo_rendering(dev):
    """AggFlowInfo::into_flowinfo_with_extra_fields (aggregator.rs:203-277): key and aggregated
    fields, originalFlowsPresent, min/maxExportSeconds, collectionTimeMilliseconds, then the
    port / domain / template sets (ascending), as the oracle renders the same groups."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    ipfix = ipfix_msg([tset(256, K.NF_TEMPLATE), dset(256, [K.NF_RECORD, K.NF_RECORD])], K.T_2025_01_01_12,
                      domain=100)
    d = [K.nf_packet(), ipfix] + t20_datagrams(500, 100, [1_700_000_000])
    fields = K.NF_FIELDS + [(0, 6, 0, OR), (0, 22, 0, MN)]
    codec = FlowInfoCodec()
    agg = new_agg(fields, lateness_s=10 ** 6 // 1000, window_s=10 ** 6 // 1000)
    agg.push(codec.decode_datagrams(d), 9995, K.T_2025_01_01_10_MS)
    hdr, raw = agg.flush_raw()
    groups = agg.render(hdr, raw)
    lines = agg.flowinfo_json(raw, shard_id=3, seq0=40, export_time_ms=1_760_000_000_123)
    o = A.aggregate_datagrams(fields, d, peer_port=9995, collection_ms=K.T_2025_01_01_10_MS,
                              window_s=1000, lateness_s=1000)
    ref = {k: g for k, g in ((k, g) for g in o.emit() + o.flush() for k in [(g["window_start"], g["flow_type"],
                                                                            tuple(_exact(x) for x in g["key"]))])}
    assert len(lines) == len(groups) == len(ref)
    for i, (g, line) in enumerate(zip(groups, lines)):
        k = (g["window_start"], g["flow_type"], tuple(_exact(x) for x in g["key"]))
        assert line == o.flowinfo_json(ref[k], shard_id=3, seq=40 + i, export_time_ms=1_760_000_000_123), k
    assert any('"NetFlowV9"' in x for x in lines) and any('"IPFIX"' in x for x in lines)


def test_stale_batch_is_refused(dev):
    from netgauze_amd.aggregate import AggError, FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    codec = FlowInfoCodec()
    d = t20_datagrams(200, 100, [1_700_000_000])
    old = codec.decode_datagrams(d)
    codec.decode_datagrams(d[1:])
    agg = new_agg([(0, 4, 0, OK), (0, 1, 0, ADD)])
    with pytest.raises(AggError, match="stale"):
        agg.push(old)


@pytest.mark.parametrize("keys", [
    [(0, 4, 0, OK), (0, 61, 0, OK)],
    [(0, 4, 0, OK), (0, 11, 0, OK)],                    # protocol + destination port (bench key dport)
    [(0, 8, 0, OK), (0, 12, 0, OK), (0, 7, 0, OK), (0, 11, 0, OK), (0, 4, 0, OK)],
])
def test_partitioned_reduction(dev, keys, monkeypatch):
    """The partitioned reduction (slot-range partitions reduced in LDS, rows updated in place),
    forced with NGZ_AGG_OPT_PARTITION 1, on the T20 streams with late messages and closing windows."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_PARTITION"), 1)
    times = [1_700_000_010, 1_700_000_030, 1_700_000_015, 1_700_000_045, 1_700_000_020, 1_700_000_050,
             1_700_000_061, 1_700_000_049]
    d = t20_datagrams(6000, 100, times)
    check(keys + T20_AGG, [d[:25], d[25:]])


@pytest.mark.parametrize("vals", [
    [(0, 1, 0, ADD)],                                                        # 16 + 8 B: 2-piece payloads
    [(0, 1, 0, ADD), (0, 2, 0, ADD), (0, 8, 0, MN), (0, 12, 0, MX), (0, 15, 0, MN),
     (0, 22, 0, MN), (0, 21, 0, MX), (0, 14, 0, OR)],                        # 16 + 52 B: 6-piece payloads
])
def test_partitioned_reduction_payload_sizes(dev, vals, monkeypatch):
    """The partitioned scatter's whole-payload stores at both ends of the payload size: 2 pieces
    (32 payloads per store instruction) and 6 pieces (10 per instruction, four lanes idle), with the
    operands of IPv4 Min / Max at 8 bytes and unsigned ones at their widths; forced partitioned path,
    protocol + destination port key, against the oracle over closing windows."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_PARTITION"), 1)
    times = [1_700_000_010, 1_700_000_030, 1_700_000_061, 1_700_000_049]
    d = t20_datagrams(6000, 100, times)
    check([(0, 4, 0, OK), (0, 11, 0, OK)] + vals, [d[:25], d[25:]])


def test_partitioned_reduction_ports_captures_orders(dev, monkeypatch):
    """Forced partitioned reduction: peer ports and collection times over two pushes, every
    reference capture (wide and packed keys), wrapping adds / signed min-max, and the ordered
    reductions that run after it."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_PARTITION"), 1)
    test_t20_multi_port_collection_times(dev)
    test_wrapping_add_and_signed_min_max(dev)
    test_ordered_reductions(dev)
    for name in [c[0] for c in golden_io.cases()]:
        for fields in ("wide", "packed"):
            test_reference_captures(dev, name, fields)


def test_partitioned_equals_atomic_at_full_size(dev, monkeypatch):
    """Full size: 10^8 T20 records (the bench batch) by protocol + destination port, 393 216
    groups, two pushes (the first creates the groups, the second reduces into them).  The
    partitioned reduction and the LDS / atomic one give byte-identical rows (every reduction
    there is order-free); only the owner word, device bookkeeping whose last writer varies
    from run to run, is left out."""
    import numpy as np
    from netgauze_amd import synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    n = 100_000_000
    codec = FlowInfoCodec(0, rtc_sync=True)
    codec.decode_datagrams([synth.template_message()])
    rec = synth.t20_records(n, device=dev)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64)
    del rec
    m = torch.arange(offs.numel(), device=dev, dtype=torch.int64)
    t = 1_700_000_010 + (m * 60) // offs.numel()  # two minute windows
    for b in range(4):
        buf[offs + 4 + b] = ((t >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    del m, t
    batch = codec.decode_batch(buf, offs, lens)
    assert batch.n_records == n
    fields = [(0, 4, 0, OK), (0, 11, 0, OK)] + T20_AGG
    rows = {}
    for mode in ("0", "1"):
        monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_PARTITION"), int(mode))
        agg = new_agg(fields, capacity=1 << 20, lateness_s=60, max_peers=256)  # packed, as the bench
        for _ in range(2):
            assert agg.push(batch, 4739, 0) == 0
        _, raw = agg.flush_raw()
        agg.close()
        raw = np.array(raw)
        raw[:, 88:92] = 0  # owner word
        rows[mode] = sorted(bytes(r) for r in raw)
    assert len(rows["1"]) > 300_000
    assert rows["0"] == rows["1"]
    codec.close()


def test_owner_path_equals_atomic_5tuple(dev, monkeypatch):
    """10^7 T20 records by the 5-tuple (about one group per record), two pushes: the owner
    path (each group's owner record reduces its row with plain stores, k_agg_apply_own) and
    the per-record atomics (NGZ_AGG_OPT_OWNER 0) give byte-identical rows, owner word aside."""
    import numpy as np
    from netgauze_amd import synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    n = 10_000_000
    codec = FlowInfoCodec(0, rtc_sync=True)
    codec.decode_datagrams([synth.template_message()])
    rec = synth.t20_records(n, device=dev)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64)
    del rec
    m = torch.arange(offs.numel(), device=dev, dtype=torch.int64)
    t = 1_700_000_010 + (m * 60) // offs.numel()  # two minute windows, nothing late
    for b in range(4):
        buf[offs + 4 + b] = ((t >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    del m, t
    batch = codec.decode_batch(buf, offs, lens)
    assert batch.n_records == n
    fields = [(0, 8, 0, OK), (0, 12, 0, OK), (0, 7, 0, OK), (0, 11, 0, OK), (0, 4, 0, OK)] + T20_AGG
    rows = {}
    for mode in ("own", "atomic"):
        if mode == "atomic":
            monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_OWNER"), 0)
        agg = new_agg(fields, capacity=n, lateness_s=60)
        for _ in range(2):
            assert agg.push(batch, 4739, 0) == 0
        _, raw = agg.flush_raw()
        agg.close()
        raw = np.array(raw)
        raw[:, 88:92] = 0  # owner word
        rows[mode] = np.sort(np.ascontiguousarray(raw).view(np.dtype((np.void, raw.shape[1]))).ravel())
    assert len(rows["own"]) > n // 2
    assert np.array_equal(rows["own"], rows["atomic"])
    codec.close()


def run_device_scenario(sc):
    """A kats_agg scenario through the device: one codec per peer address (a peer's
    FlowInfoCodec), one aggregator for the shard."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    agg = new_agg(sc["fields"], window_s=sc["window_s"], lateness_s=sc["lateness_s"], capacity=1024)
    codecs, emits, late = {}, [], 0
    for ip, port, coll, dgrams in sc["pushes"]:
        codec = codecs.setdefault((ip, port), FlowInfoCodec())
        late += agg.push(codec.decode_datagrams(dgrams), port, coll, peer_ip=ip)
        hdr, raw = agg.emit_raw()
        emits.append((agg.render(hdr, raw), raw))
    hdr, raw = agg.flush_raw()
    return agg, emits, (agg.render(hdr, raw), raw), late


def _sorted(groups):
    return sorted(groups, key=lambda g: repr((g["peer"], g["window_start"], g["flow_type"], g["key"])))


@pytest.mark.parametrize("sc", K.SCENARIOS + K.WINDOW_SCENARIOS + K.FIELD_OP_SCENARIOS, ids=lambda s: s["name"])
def test_reference_scenarios(dev, sc):
    """aggregator/tests.rs (:72-1377), the analytics window tests (aggregation.rs:498-788) and the
    Field arithmetic KATs (flow-pkt lib.rs:359-615, two records of one group per KAT plus the
    Inapplicable pair kept apart) as wire-level scenarios on the device: the expected groups of every push's closed windows and of
    the flush, the late records, and each group's FlowInfo text equal to the oracle's."""
    import test_oracle_agg as T
    agg, emits, (flushed, raw), late = run_device_scenario(sc)
    o_agg, o_emits, o_flushed = T.run_oracle_scenario(sc)
    assert late == sc["late"] == o_agg.late
    assert _sorted(flushed) == _sorted(sc["flush"]) == _sorted(o_flushed)
    if sc["emits"] is not None:
        for (got, _raw), exp in zip(emits, sc["emits"]):
            assert _sorted(got) == _sorted(exp)
    # the FlowInfo of every flushed group: the oracle's text, windowStart/windowEnd/exporter IP included
    lines = agg.flowinfo_json(raw, shard_id=2, seq0=7, export_time_ms=1_751_450_400_000)
    for i, (g, line) in enumerate(zip(flushed, lines)):
        assert line == o_agg.flowinfo_json(g, shard_id=2, seq=7 + i, export_time_ms=1_751_450_400_000)


@pytest.mark.parametrize("flow_type", [10, 9])
def test_into_flowinfo_with_extra_fields_kat(dev, flow_type):
    """test_ipfix / test_netflowv9_into_flowinfo_with_extra_fields (tests.rs:339-586) on the device:
    the record's fields sorted (HashSet order is unspecified) equal the test's expected fields plus
    the exporter IP the actor appends (actor.rs:222-225); sequence number 42, shard 5 as the
    observation domain / source id, NetFlow v9 sys-up time 5000."""
    import json
    fields, pushes = K.flowinfo_scenario(flow_type)
    sc = dict(fields=fields, pushes=pushes, window_s=60, lateness_s=10)
    agg, _emits, (flushed, raw), _late = run_device_scenario(sc)
    assert len(flushed) == 1
    (line,) = agg.flowinfo_json(raw, shard_id=5, seq0=42, export_time_ms=K.T_JUL2_10 * 1000)
    body = json.loads(line)["IPFIX" if flow_type == 10 else "NetFlowV9"]
    assert body["sequence_number"] == 42
    assert body["observation_domain_id" if flow_type == 10 else "source_id"] == 5
    if flow_type == 9:
        assert body["sys_up_time"] == 5000
    (st,) = body["sets"]
    (rec,) = st["Data"]["records"]
    assert st["Data"]["id"] == 65535 and rec["scope_fields"] == []
    key = lambda f: json.dumps(f, sort_keys=True)  # noqa: E731
    assert sorted(rec["fields"], key=key) == sorted(K.FLOWINFO_EXPECTED_FIELDS, key=key)


def test_thousand_peers_one_aggregator(dev):
    """One aggregator serves a shard's 1 000 exporter peers (IPv4 and IPv6): groups are keyed by
    peer IP, and each peer's event time closes only its own windows (aggregation.rs:96-172).
    Peers export T20 messages at their own clock offsets; after every round of pushes the
    emitted windows equal the oracle's, and so does the final flush."""
    from netgauze_amd import synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    fields = [(0, 4, 0, OK), (0, 61, 0, OK)] + T20_AGG
    n_peers, rounds, per_msg = 1000, 3, 20
    rec = synth.t20_records(n_peers * rounds * per_msg, first=0)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64, rec_per_msg=per_msg)
    b = bytes(buf.numpy())
    msgs = [bytearray(b[o:o + ln]) for o, ln in zip(offs.tolist(), lens.tolist())]
    peers = ["10.%d.%d.1" % (i // 250, i % 250) if i % 3 else "2001:db8::%x" % (i + 1) for i in range(n_peers)]
    agg = new_agg(fields, capacity=1 << 16, lateness_s=10, max_peers=1024)
    o = A.FlowAggregatorOracle(fields, 60, 10)
    codecs, ocodecs = {}, {}
    tm = synth.template_message()
    emitted = 0
    for r in range(rounds):
        for i, ip in enumerate(peers):
            m = msgs[r * n_peers + i]
            # peer i's clock: offset 7*i s; rounds 50 s apart, so every peer closes windows at its own pace
            m[4:8] = struct.pack(">I", 1_700_000_000 + 7 * i + 50 * r)
            dg = ([tm] if r == 0 else []) + [bytes(m)]
            codec = codecs.setdefault(ip, FlowInfoCodec())
            agg.push(codec.decode_datagrams(dg), 4739 + i % 5, 1_000 * r, peer_ip=ip)
            oc = ocodecs.setdefault(ip, O.FlowInfoCodec())
            A.aggregate_datagrams(fields, dg, 4739 + i % 5, 1_000 * r, peer_ip=ip, agg=o, codec=oc)
        got, ref = agg.emit(), o.emit()
        same_groups(got, ref)
        emitted += len(got)
    assert emitted > 0 and len({g["peer"] for g in ref}) > 1
    same_groups(agg.flush(), o.flush())


# ---- byte values of any length (BVAL): string / octet-array / list keys and values, fixed or
# variable-length on the wire, longer than 32 bytes included (the tail in the byte arena) ----
HUAWEI_BYTES = [(0, 497, 0, OK), (0, 236, 0, OK), (0, 1, 0, ADD), (0, 2, 0, ADD), (0, 210, 0, OR), (0, 210, 1, OR),
                (2011, 704, 0, OR), (2011, 232, 0, OR), (0, 90, 0, OR)]
SRV6_BYTES = [(0, 84, 0, OK), (0, 82, 0, OK), (0, 83, 0, OK), (0, 236, 0, OK), (0, 1, 0, ADD), (0, 90, 0, OR),
              (0, 2, 0, ADD)]


@pytest.mark.parametrize("name,fields", [("106-IPFIXv10-HUAWEI-vrf_name__traffic-00", HUAWEI_BYTES),
                                         ("srv6__srv6", SRV6_BYTES)])
def test_byte_keys_and_values_on_captures(dev, name, fields):
    """the Huawei 106 capture keyed on its variable-length SRv6 segment list
    (srhSegmentIPv6ListSection) and VRF name, with octet-array ORs over paddingOctets (declared
    3 and 1 bytes wide in two templates: the group keeps its first value's length), Huawei
    vendor-unknown fields and the route distinguisher; the srv6 capture keyed on its 90-byte
    samplerName and 64-byte interface name / description (tails beyond 32 bytes in the arena)
    and VRF name.  Per peer, two pushes, equal to the oracle (aggregator.rs:123, 286-354).
    (Those fixed-length strings hold short, NUL-padded text: values beyond 32 bytes are covered
    by test_byte_values_synthetic and test_long_byte_keys_through_table_rebuilds.)"""
    byte_keys = 0
    for key, dgrams in peers_of(name).items():
        h = len(dgrams) // 2
        groups = check(fields, [dgrams[:h], dgrams[h:]], port=key[1], lateness_s=60)
        byte_keys += sum(1 for g in groups for x in g["key"] if isinstance(x, (bytes, str)))
    assert byte_keys > 0


def _vlen(b):
    return (bytes([len(b)]) if len(b) < 255 else b"\xff" + len(b).to_bytes(3, "big")) + b


def byte_value_stream(n_msgs, per_msg, seed=11, t0=1_700_000_000, step=20):
    """Three templates sending the same fields at different wire forms: VRFname (236) fixed 16 /
    fixed 48 / variable-length, forwardingStatus (89) 1 / 4 / 1 bytes, basicList (291) and
    subTemplateList (292) variable-length or fixed, applicationId (95) variable-length / fixed 6."""
    import random
    rnd = random.Random(seed)
    names = [b"red", b"blue", b"", b"a-vrf-name-that-is-longer-than-thirty-two-bytes", b"red\0tail",
             b"x" * 300, "gr\u00fcn".encode()]
    fwd = [0, 3, 64, 66, 68, 69, 100, 128, 143, 150, 192, 195, 200, 255]
    t1 = [(8, 4), (236, 16), (1, 8), (89, 1), (291, 0xFFFF), (95, 0xFFFF)]
    t2 = [(8, 4), (236, 48), (1, 8), (89, 4), (291, 20), (95, 6)]
    t3 = [(8, 4), (236, 0xFFFF), (1, 8), (89, 1), (292, 0xFFFF), (95, 0xFFFF)]
    msgs = [ipfix_msg([tset(600, t1), tset(601, t2), tset(602, t3)], t0)]
    for m in range(n_msgs):
        tid = 600 + m % 3
        recs = []
        for _ in range(per_msg):
            nm = rnd.choice(names)
            blob = bytes(rnd.getrandbits(8) for _ in range(rnd.choice([0, 3, 20, 33, 70])))
            app = bytes(rnd.getrandbits(8) for _ in range(rnd.choice([2, 6, 40])))
            r = struct.pack(">I", rnd.choice([1, 2])) if tid != 601 else struct.pack(">I", rnd.choice([1, 2, 3]))
            if tid == 600:
                r += nm[:16].ljust(16, b"\0") if b"\0" not in nm[:16] else nm[:16].ljust(16, b"\0")
            elif tid == 601:
                r += nm[:48].ljust(48, b"\0")
            else:
                r += _vlen(nm)
            r += struct.pack(">Q", rnd.getrandbits(40))
            f = rnd.choice(fwd)
            r += struct.pack(">I", f) if tid == 601 else bytes([f])
            r += _vlen(blob) if tid != 601 else blob[:20].ljust(20, b"\1")
            r += _vlen(app) if tid != 601 else app[:6].ljust(6, b"\0")
            recs.append(r)
        msgs.append(ipfix_msg([dset(tid, recs)], t0 + step * (m // 3), seq=m + 2))
    return msgs


def test_byte_values_synthetic(dev):
    """String keys that are one key at every wire form (fixed 16, fixed 48 and variable-length:
    the text up to the first NUL of a fixed cell, a variable-length one as sent, so "red\\0tail"
    sent variable-length is its own key), keys of 0 to 300 bytes; Min / Max over basicList and
    subTemplateList (Box<[u8]> order), octet-array OR of 2 to 40 bytes (the group keeps its first
    value's length), forwardingStatus Min / Max in its nested reason-code order -- over pushes whose
    windows close, against the oracle."""
    d = byte_value_stream(30, 40)
    fields = [(0, 236, 0, OK), (0, 8, 0, OK), (0, 1, 0, ADD), (0, 89, 0, MX), (0, 291, 0, MN), (0, 292, 0, MX),
              (0, 95, 0, OR)]
    groups = check(fields, [d[:9], d[9:20], d[20:]], lateness_s=10)
    keys = {g["key"][0] for g in groups}
    assert {"red", "red\0tail", "", "x" * 300} <= keys, sorted(k[:8] for k in keys if k)
    fields2 = [(0, 8, 0, OK), (0, 89, 0, MN), (0, 291, 0, MX), (0, 292, 0, MN), (0, 1, 0, ADD)]
    check(fields2, [d[:15], d[15:]], lateness_s=10)


def test_long_byte_keys_through_table_rebuilds(dev):
    """Keys longer than 32 bytes over 24 pushes whose windows close push by push: the emitted
    groups' tails become garbage and the table rebuild (tombstones) compacts the byte arena;
    every push's emitted windows equal the oracle's, and so does the final flush."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    fields = [(0, 82, 0, OK), (0, 1, 0, ADD)]
    agg = new_agg(fields, capacity=2000, lateness_s=0)
    o = A.FlowAggregatorOracle(fields, 60, 0)
    codec, oc = FlowInfoCodec(), O.FlowInfoCodec()
    tpl = [(82, 0xFFFF), (1, 8)]
    out = 0
    for step in range(24):
        recs = [_vlen(("interface-%06d-of-step-%02d-with-a-long-name" % (j, step)).encode()) +
                struct.pack(">Q", j + 1) for j in range(900)]
        d = [ipfix_msg(([tset(256, tpl)] if step == 0 else []) + [dset(256, recs[i:i + 300])],
                       1_700_000_000 + 60 * step) for i in range(0, 900, 300)]
        agg.push(codec.decode_datagrams(d))
        A.aggregate_datagrams(fields, d, agg=o, codec=oc)
        got = agg.emit()
        same_groups(got, o.emit())
        out += len(got)
    assert out == 23 * 900
    same_groups(agg.flush(), o.flush())


def test_row_bytes_refuses_rows_of_an_earlier_take(dev):
    """ngz_agg_row.take_id: byte values of a row returned by an earlier flush / emit
    are NGZ_E_INVALID, not another row's bytes, and so is its FlowInfo rendering; the last
    call's rows read their own values."""
    import numpy as np
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import AggError
    from netgauze_amd.flow import FlowInfoCodec
    fields = [(0, 82, 0, OK), (0, 1, 0, ADD)]
    agg = new_agg(fields, capacity=2000, lateness_s=0)
    codec = FlowInfoCodec()
    tpl = [(82, 0xFFFF), (1, 8)]
    raws = []
    for step in range(3):
        recs = [_vlen(("a-long-interface-name-%04d-of-step-%02d-padding" % (j, step)).encode()) +
                struct.pack(">Q", j + 1) for j in range(50)]
        d = [ipfix_msg(([tset(256, tpl)] if step == 0 else []) + [dset(256, recs)], 1_700_000_000 + 60 * step)]
        agg.push(codec.decode_datagrams(d))
        hdr, raw = agg.emit_raw() if step else agg.flush_raw()
        raws.append((hdr, raw, step))
    hdr, raw, step = raws[-1]
    assert len(raw) and all(int(h["take_id"]) == 3 for h in hdr)
    assert agg._row_bytes(raw[0], 0, 0).startswith(b"a-long-interface-name-")
    old_hdr, old_raw, _ = raws[0]
    assert len(old_raw) == 50 and all(int(h["take_id"]) == 1 for h in old_hdr)
    for r in old_raw[:5]:
        r = np.ascontiguousarray(r)
        assert _lib.load().ngz_agg_row_bytes(agg._h, r.ctypes.data, 0, 0, None, 0) == -1  # NGZ_E_INVALID
    with pytest.raises(AggError):
        agg.flowinfo_json(old_raw)
    assert len(agg.flowinfo_json(raw)) == len(raw)


def test_wide_byte_key_large_batch(dev):
    """A 200-byte variable-length string key over 10^6 records in one batch, five distinct keys,
    pushed three times: the byte arena is reserved per group and field (table slots x
    byte fields x the longest tail), not per record (10^6 x 168 B), and tail offsets are 8-byte
    units (no 4 GiB wrap).  Groups, counts and sums equal the numpy reference of the same records."""
    import numpy as np
    from netgauze_amd.flow import FlowInfoCodec
    n, per = 1_000_000, 300
    keys = [(b"%d-" % i) + bytes([65 + i]) * 198 for i in range(5)]
    rng = np.random.default_rng(5)
    ki = rng.integers(0, 5, n)
    octets = rng.integers(1, 1 << 40, n, dtype=np.uint64)
    rec = np.zeros((n, 209), np.uint8)
    rec[:, 0] = 200
    rec[:, 1:201] = np.frombuffer(b"".join(keys), np.uint8).reshape(5, 200)[ki]
    rec[:, 201:] = octets.astype(">u8").view(np.uint8).reshape(n, 8)
    tpl = [(82, 0xFFFF), (1, 8)]
    dgrams = [ipfix_msg([tset(256, tpl)], 1_700_000_000)]
    for i in range(0, n, per):
        dgrams.append(ipfix_msg([dset(256, [rec[i:i + per].tobytes()])], 1_700_000_000, seq=2 + i // per))
    codec = FlowInfoCodec(0)
    batch = codec.decode_datagrams(dgrams)
    assert batch.n_records == n
    agg = new_agg([(0, 82, 0, OK), (0, 1, 0, ADD)], capacity=1024, lateness_s=60)
    for _ in range(3):
        assert agg.push(batch) == 0
    got = {g["key"][0]: (g["record_count"], g["vals"][0]) for g in agg.flush()}
    want = {}
    for i, k in enumerate(keys):
        m = ki == i
        want[k.decode()] = (3 * int(m.sum()), int((3 * octets[m].astype(object)).sum()) % (1 << 64))
    assert got == want


def test_tombstones_do_not_fill_the_table(dev):
    """windows emitted push after push leave tombstones; pushes keep succeeding while
    the live groups stay within the capacity (the table is rebuilt before a push when tombstones
    and the push's new groups would crowd it)."""
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    fields = [(0, 8, 0, OK), (0, 12, 0, OK), (0, 1, 0, ADD)]
    agg = new_agg(fields, capacity=2000, lateness_s=0)
    o = A.FlowAggregatorOracle(fields, 60, 0)
    codec, oc = FlowInfoCodec(), O.FlowInfoCodec()
    tpl = [(8, 4), (12, 4), (1, 8)]
    out = 0
    for step in range(24):
        recs = [struct.pack(">IIQ", step * 1000 + j, j, j + 1) for j in range(900)]
        d = [ipfix_msg(([tset(256, tpl)] if step == 0 else []) + [dset(256, recs[i:i + 300])],
                       1_700_000_000 + 60 * step) for i in range(0, 900, 300)]
        agg.push(codec.decode_datagrams(d))
        A.aggregate_datagrams(fields, d, agg=o, codec=oc)
        got = agg.emit()
        same_groups(got, o.emit())
        out += len(got)
    assert out == 23 * 900
    same_groups(agg.flush(), o.flush())


@pytest.mark.parametrize("keys", [
    [(0, 4, 0, OK), (0, 61, 0, OK)],  # protocol + direction: 6 key tuples
    [(0, 4, 0, OK)],                  # protocol: 3
    [(0, 61, 0, OK), (0, 60, 0, OK)],  # direction + ipVersion: 2
])
def test_lowcard_path_equals_oracle(dev, keys, monkeypatch):
    """The low-cardinality path (k_agg_lc_part + k_agg_lc_merge: per-lane LDS accumulators,
    no per-record atomics) on T20 streams whose export times go back and forth (late
    messages dropped, windows closed push by push), equal to the oracle; the path is checked
    to be the one taken."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_LOWCARD"), 1)
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    times = [1_700_000_010, 1_700_000_030, 1_700_000_015, 1_700_000_045, 1_700_000_020, 1_700_000_050,
             1_700_000_061, 1_700_000_049]
    d = t20_datagrams(6000, 100, times)
    fields = keys + T20_AGG
    codec, oc = FlowInfoCodec(), O.FlowInfoCodec()
    agg = new_agg(fields, lateness_s=10)
    o = A.FlowAggregatorOracle(fields, 60, 10)
    late = 0
    for part in (d[:25], d[25:40], d[40:]):
        late += agg.push(codec.decode_datagrams(part), 4739, 1_700_000_000_000)
        assert agg.last_path() == "lowcard"
        A.aggregate_datagrams(fields, part, 4739, 1_700_000_000_000, agg=o, codec=oc)
        same_groups(agg.emit(), o.emit())
    assert late == o.late and late > 0
    same_groups(agg.flush(), o.flush())


@pytest.mark.parametrize("max_peers", [4, 1024, 0])
def test_lowcard_path_many_peers(dev, max_peers, monkeypatch):
    """the low-cardinality path packs the peer entry into the window context
    (k_agg_lc_part) and unpacks it when it writes the group's key (lc_key_write).  Four exporter
    peers (IPv4 and IPv6) at their own clock offsets push T20 messages in turn, each push taking
    the low-cardinality path, with max_peers 4 / 1024 / 65536 (2, 10 and 16 peer bits of the
    packed tag): every push's emitted windows and the final flush equal the oracle's, groups
    land on their own peer and close at that peer's own event time."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_LOWCARD"), 1)
    from netgauze_amd import synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    import ngz_oracle as O
    fields = [(0, 4, 0, OK), (0, 61, 0, OK)] + T20_AGG
    peers = ["10.0.0.1", "2001:db8::7", "192.0.2.200", "10.0.3.9"]
    rounds, msgs_per_push, per_msg = 4, 3, 100
    rec = synth.t20_records(len(peers) * rounds * msgs_per_push * per_msg, first=0)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64, rec_per_msg=per_msg)
    b = bytes(buf.numpy())
    msgs = [bytearray(b[o:o + ln]) for o, ln in zip(offs.tolist(), lens.tolist())]
    agg = new_agg(fields, capacity=1 << 12, lateness_s=10, max_peers=max_peers)
    o = A.FlowAggregatorOracle(fields, 60, 10)
    codecs, ocodecs = {}, {}
    tm = synth.template_message()
    seen_peers = set()
    k = 0
    for r in range(rounds):
        for i, ip in enumerate(peers):
            dg = [tm] if r == 0 else []
            for j in range(msgs_per_push):
                m = msgs[k]
                k += 1
                # peer i's clock: offset 13*i s, rounds 40 s apart, one message 30 s behind (late)
                m[4:8] = struct.pack(">I", 1_700_000_000 + 13 * i + 40 * r - (30 if j == 1 else 0))
                dg.append(bytes(m))
            codec = codecs.setdefault(ip, FlowInfoCodec())
            agg.push(codec.decode_datagrams(dg), 4739 + i, 1_000 * r, peer_ip=ip)
            assert agg.last_path() == "lowcard"
            oc = ocodecs.setdefault(ip, O.FlowInfoCodec())
            A.aggregate_datagrams(fields, dg, 4739 + i, 1_000 * r, peer_ip=ip, agg=o, codec=oc)
            got, ref = agg.emit(), o.emit()
            same_groups(got, ref)
            seen_peers |= {g["peer"] for g in ref}
    assert len(seen_peers) > 1
    fin = o.flush()
    same_groups(agg.flush(), fin)
    assert len({g["peer"] for g in fin}) == len(peers)


def test_lowcard_falls_back_on_many_key_tuples(dev, monkeypatch):
    """A packed key with more than 8 distinct tuples in a push (protocol + source port) makes a
    wave of k_agg_lc_part raise the overflow flag: k_agg_lc_merge does nothing and the push runs
    the general path from scratch (nothing claimed), and every reference capture still equals
    the oracle."""
    monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_LOWCARD"), 1)
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    paths = set()
    for name in [c[0] for c in golden_io.cases()]:
        for key, dgrams in peers_of(name).items():
            codec = FlowInfoCodec()
            agg = new_agg(GOLDEN_AGG_PACKED, lateness_s=60, max_peers=256)  # 8 peer bits: packed tags
            h = len(dgrams) // 2
            emitted = []
            for part in (dgrams[:h], dgrams[h:]):
                agg.push(codec.decode_datagrams(part), key[1], 1_700_000_000_000)
                paths.add(agg.last_path())
                emitted += agg.emit()
            got = emitted + agg.flush()
            o = A.aggregate_datagrams(GOLDEN_AGG_PACKED, dgrams, key[1], 1_700_000_000_000, lateness_s=60)
            same_groups(got, o.emit() + o.flush())
    assert paths - {"none"} == {"lowcard", "general"}, paths


def test_lowcard_equals_general_at_full_size(dev, monkeypatch):
    """Full size: 10^8 T20 records by protocol + flow direction (12 groups over two windows),
    two pushes: the low-cardinality path and the general one give byte-identical rows (owner
    word and push marker aside)."""
    import numpy as np
    from netgauze_amd import synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    n = 100_000_000
    codec = FlowInfoCodec(0, rtc_sync=True)
    codec.decode_datagrams([synth.template_message()])
    rec = synth.t20_records(n, device=dev)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64)
    del rec
    m = torch.arange(offs.numel(), device=dev, dtype=torch.int64)
    t = 1_700_000_010 + (m * 60) // offs.numel()  # two minute windows
    for b in range(4):
        buf[offs + 4 + b] = ((t >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    del m, t
    batch = codec.decode_batch(buf, offs, lens)
    assert batch.n_records == n
    fields = [(0, 4, 0, OK), (0, 61, 0, OK)] + T20_AGG
    rows = {}
    for mode in ("0", "1"):
        monkeypatch.setitem(AGG_OPTIONS, _opt("NGZ_AGG_OPT_LOWCARD"), int(mode))
        agg = new_agg(fields, capacity=1 << 10, lateness_s=60)
        for _ in range(2):
            assert agg.push(batch, 4739, 0) == 0
            assert agg.last_path() == ("lowcard" if mode == "1" else "general")
        _, raw = agg.flush_raw()
        agg.close()
        raw = np.array(raw)
        raw[:, 88:92] = 0  # owner word
        raw[:, 36:40] = 0  # push marker
        rows[mode] = sorted(bytes(r) for r in raw)
    assert len(rows["1"]) == 12
    assert rows["0"] == rows["1"]
    codec.close()
