"""The flow-options input on the device (include/ngz/flow_options.h) against the Python restatement
of the reference (tests/options_ref.py) over the oracle's decode of the same datagrams: the same
operations in the same order with the same value bytes, and the same counters."""
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import enrich_ref as E  # noqa: E402
import ngz_oracle as O  # noqa: E402
import options_ref as OR  # noqa: E402
import parity  # noqa: E402
import renorm_ref as R  # noqa: E402

T0 = 1_700_000_000
PEER = "10.0.0.1"
WEIGHT = 16
V = 0xFFFF


def u(ie, v, w):
    return (0, ie, E.K_UINT, int(v).to_bytes(w, "little"))


def spec(fields):
    return b"".join(struct.pack(">HH", i, n) for i, n in fields)


def tmpl_record(tid, fields):
    return struct.pack(">HH", tid, len(fields)) + spec(fields)


def opt_record(tid, scope, fields):
    """IPFIX options template record (ipfix.rs:276-327)."""
    return struct.pack(">HHH", tid, len(scope) + len(fields), len(scope)) + spec(scope + fields)


def nf_opt_record(tid, scope, fields):
    """NetFlow v9 options template record (netflow.rs:265-310): lengths in bytes."""
    return struct.pack(">HHH", tid, 4 * len(scope), 4 * len(fields)) + spec(scope + fields)


def ipfix_msg(sets, seq=0, domain=1, t=T0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIII", 10, 16 + len(body), t, seq, domain) + body


def nf9_msg(sets, count, seq=0, src=1, t=T0):
    body = b""
    for sid, b in sets:
        b += b"\0" * (-len(b) % 4)
        body += struct.pack(">HH", sid, 4 + len(b)) + b
    return struct.pack(">HHIIII", 9, count, 1000, t, seq, src) + body


def record(fields, values):
    out = b""
    for (_ie, n), v in zip(fields, values):
        if n == V:
            # the reference reads a three-byte length after the 0xFF escape (generator.rs:1775-1793)
            out += (bytes([len(v)]) if len(v) < 255 else b"\xff" + len(v).to_bytes(3, "big")) + v
        elif isinstance(v, bytes):
            out += v
        else:
            out += (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
    return out


S_SEL, F_SEL = [(302, 8)], [(34, 4)]                        # selectorId -> samplingInterval
S_IF, F_IF = [(10, 4), (14, 4)], [(82, V), (83, V)]         # both directions, variable-length names
T_DATA = [(302, 8), (1, 8), (2, 8)]                         # data records: selectorId, no sampling IE


def decode(dgrams):
    from netgauze_amd.flow import FlowInfoCodec
    codec = FlowInfoCodec(0, specialize=False)
    batch = codec.decode_datagrams(dgrams)
    oracle, _ = parity.oracle_datagrams(dgrams)
    parity.check_batch(batch, oracle)
    return codec, batch, oracle


def check(batch, oracle, hv=None, peer=PEER):
    """Harvest and compare with the restatement; returns (harvester, stats, operations)."""
    from netgauze_amd.options import FlowOptionsHarvester
    hv = hv if hv is not None else FlowOptionsHarvester(0, WEIGHT)  # an empty harvester is falsy (len 0)
    ref_stats, ref_ops = OR.harvest_batch(batch, oracle, peer, WEIGHT)
    json_before = batch.json_lines()
    stats = hv.harvest(batch, peer)
    ops = hv.ops()
    assert stats == ref_stats, (stats, ref_stats)
    assert len(ops) == len(ref_ops)
    for i, (a, b) in enumerate(zip(ops, ref_ops)):
        assert a == b, (i, a, b)
    assert batch.json_lines() == json_before  # nothing written into the context's arena
    return hv, stats, ops


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_counts_of_one_sampling_template(n):
    rng = random.Random(n)
    dg = [ipfix_msg([(3, opt_record(400, S_SEL, F_SEL)), (2, tmpl_record(300, T_DATA))])]
    left, sel = n, 0
    while left:  # several sets per message, several messages
        sets = []
        for _ in range(rng.randrange(1, 4)):
            k = min(left, rng.randrange(1, 120))
            if not k:
                break
            sets.append((400, b"".join(record(S_SEL + F_SEL, [sel + i, 10 + (sel + i) % 7]) for i in range(k))))
            sel += k
            left -= k
        dg.append(ipfix_msg(sets, domain=rng.choice([5, 6])))
    dg.append(ipfix_msg([(300, record(T_DATA, [1, 2, 3]) * 5)]))
    _codec, batch, oracle = decode(dg)
    hv, stats, ops = check(batch, oracle)
    assert stats["operations_generated"] == n and stats["received_flows"] == len(dg)
    assert [int.from_bytes(op["scope"][0][3], "little") for op in ops] == list(range(n))
    assert (hv.last_launches == 0) == (n == 0)


def test_three_templates_interleaved_in_stream_order():
    nf_s, nf_f = [(2, 4)], [(82, 8)]
    dg = [ipfix_msg([(3, opt_record(400, S_SEL, F_SEL) + opt_record(401, S_IF, F_IF)), (2, tmpl_record(300, T_DATA))]),
          nf9_msg([(1, nf_opt_record(500, nf_s, nf_f))], 1, src=77)]
    sel = lambda i: record(S_SEL + F_SEL, [i, 100 + i])  # noqa: E731
    itf = lambda i: record(S_IF + F_IF, [i, i, b"eth%d" % i, b"uplink %d" % i])  # noqa: E731
    data = record(T_DATA, [1, 2, 3]) * 3
    dg.append(ipfix_msg([(400, sel(1) + sel(2)), (300, data), (401, itf(1)), (400, sel(3)), (300, data), (401, itf(2) + itf(3))],
                        domain=9))
    dg.append(nf9_msg([(500, record(nf_s + nf_f, [5, b"ge-0/0/5"]) + record(nf_s + nf_f, [6, b"ge-0/0/6"]))], 2, src=77))
    dg.append(ipfix_msg([(401, itf(4)), (400, sel(4))], domain=9))
    _codec, batch, oracle = decode(dg)
    _hv, stats, ops = check(batch, oracle)
    assert stats["operations_generated"] == 4 + 2 * 4 + 2 * 2
    kinds = ["s" if op["fields"][0][1] == 34 else "i" if op["scope"][0][1] == 10 else "e" for op in ops]
    assert kinds == list("ssiesieie" + "ieie" + "ies"), kinds
    assert [op["domain"] for op in ops[9:13]] == [77] * 4


def test_failed_messages_contribute_nothing():
    dg = [ipfix_msg([(3, opt_record(400, S_SEL, F_SEL))]),
          ipfix_msg([(400, record(S_SEL + F_SEL, [1, 10]))]),
          ipfix_msg([(999, b"\0" * 8), (400, record(S_SEL + F_SEL, [2, 20]))]),   # fails before its options set
          ipfix_msg([(400, record(S_SEL + F_SEL, [3, 30])), (999, b"\0" * 8)]),   # fails after its options set
          ipfix_msg([(400, record(S_SEL + F_SEL, [4, 40]))])]
    _codec, batch, oracle = decode(dg)
    assert [k for k, _ in oracle] == ["ok", "ok", "err", "err", "ok"]
    _hv, stats, ops = check(batch, oracle)
    assert stats["received_flows"] == 3 and stats["processed_options_records"] == 2
    assert [int.from_bytes(op["scope"][0][3], "little") for op in ops] == [1, 4]


def test_interface_and_vrf_templates():
    t = {410: ([(10, 4), (14, 4)], [(82, V), (83, V)]),           # both directions
         411: ([(10, 4)], [(82, V)]),                               # ingress only
         412: ([(14, 4)], [(83, 16)]),                              # egress only, a description without a name
         413: ([(10, 4), (141, 4), (144, 4), (14, 4)], [(82, V)]),  # extra scope fields carried into both halves
         414: ([(234, 4), (235, 4)], [(236, V), (90, 8)]),          # VRF, both directions
         415: ([(10, 4), (82, 8)], [(1, 8)]),                       # the name only in the scope: MissingRequiredFields
         416: ([(235, 4)], [(236, V)])}
    dg = [ipfix_msg([(3, b"".join(opt_record(tid, sc, fl) for tid, (sc, fl) in t.items()))])]
    rec = lambda tid, vals: (tid, record(t[tid][0] + t[tid][1], vals))  # noqa: E731
    dg.append(ipfix_msg([rec(410, [7, 7, b"eth7", b"to core"]), rec(410, [7, 8, b"bad", b"ids differ"]),
                         rec(411, [3, b"lo0"]), rec(412, [4, b"desc".ljust(16, b"\0")]),
                         rec(413, [5, 2, 99, 5, b"xe-5"]), rec(413, [5, 2, 99, 6, b"xe-6"]),
                         rec(414, [11, 11, b"red", b"\0\1\0\0\0\2\0\3"]), rec(414, [11, 12, b"blue", b"\0" * 8]),
                         rec(415, [1, b"name".ljust(8, b"\0"), 5]), rec(416, [9, b"green"])], domain=3))
    _codec, batch, oracle = decode(dg)
    _hv, stats, ops = check(batch, oracle)
    assert stats["processed_options_records"] == 10 and stats["normalization_errors"] == 4
    assert stats["operations_generated"] == 2 + 1 + 1 + 2 + 2 + 1
    assert [(op["scope"][0][1], op["fields"][0][:2]) for op in ops[:2]] == [(10, (3746, 8)), (14, (3746, 9))]
    assert [f[:2] for f in ops[4]["scope"]] == [(0, 10), (0, 141)] and [f[:2] for f in ops[5]["scope"]] == [(0, 14), (0, 141)]


@pytest.mark.parametrize("device_input", [False, True])
def test_string_lengths_are_copied_on_the_device(device_input):
    import torch
    from netgauze_amd.flow import FlowInfoCodec
    sc, fl = [(10, 4)], [(82, V), (83, 16)]
    lengths = [0, 1, 15, 16, 17, 254, 255, 300]
    dg = [ipfix_msg([(3, opt_record(400, sc, fl))])]
    recs = [record(sc + fl, [i, bytes(65 + (i + j) % 26 for j in range(n)), b"lo".ljust(16, b"\0")]) for i, n in enumerate(lengths)]
    dg += [ipfix_msg([(400, b"".join(recs[:5]))]), ipfix_msg([(400, b"".join(recs[5:]))])]
    oracle, _ = parity.oracle_datagrams(dg)
    codec = FlowInfoCodec(0, specialize=False)
    if device_input:  # the input exists only in HBM: the bytes can only come from the pack pass
        lens = np.array([len(d) for d in dg], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
        data = torch.from_numpy(np.frombuffer(b"".join(dg) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        batch = codec.decode_batch(data, torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda())
    else:
        batch = codec.decode_datagrams(dg)
    _hv, _stats, ops = check(batch, oracle)
    assert [len(op["fields"][0][3]) for op in ops] == lengths
    assert all(op["fields"][1] == (3746, 10, E.K_STR, b"lo") for op in ops)


def test_netflow_v9_scopes():
    t = {500: ([(1, 4)], [(50, 4)]),         # System + samplerRandomInterval: an empty scope
         501: ([(2, 4)], [(82, 8)]),         # Interface: ingress and egress
         502: ([(3, 2)], [(34, 4)]),         # LineCard
         503: ([(4, 4)], [(34, 4)]),         # Cache
         504: ([(5, 4)], [(34, 4)]),         # Template
         505: ([(9, 4)], [(34, 4)]),         # unknown
         506: ([(1, 4), (2, 4)], [(34, 4)])}  # System dropped, Interface kept: sampling with two scope fields
    dg = [nf9_msg([(1, nf_opt_record(tid, sc, fl))], 1, src=42) for tid, (sc, fl) in t.items()]
    rec = lambda tid, vals: (tid, record(t[tid][0] + t[tid][1], vals))  # noqa: E731
    dg.append(nf9_msg([rec(500, [1, 1000]), rec(501, [8, b"ge-0/0/8"]), rec(502, [2, 64]), rec(503, [1, 5]), rec(504, [1, 5]),
                       rec(505, [1, 5]), rec(506, [1, 9, 128])], 7, src=42))
    _codec, batch, oracle = decode(dg)
    _hv, stats, ops = check(batch, oracle)
    assert stats["netflow_v9_conversion_errors"] == 3 and stats["operations_generated"] == 1 + 2 + 1 + 1
    assert ops[0]["scope"] == [] and ops[0]["domain"] == 42 and ops[0]["fields"] == [u(50, 1000, 4)]
    assert [f[:2] for f in ops[4]["scope"]] == [(0, 10), (0, 14)]


def test_refused_operations_are_counted_and_leave_the_cache():
    from netgauze_amd.enrich import FlowEnricher
    t = {420: ([(236, 8)], [(34, 4)]),                                      # a string-valued scope
         421: ([(302, 8), (10, 4), (14, 4), (141, 4), (143, 4)], [(34, 4)]),  # five scope fields
         422: ([(302, 8)], [(34, 4)])}
    dg = [ipfix_msg([(3, b"".join(opt_record(tid, sc, fl) for tid, (sc, fl) in t.items()))])]
    rec = lambda tid, vals: (tid, record(t[tid][0] + t[tid][1], vals))  # noqa: E731
    dg.append(ipfix_msg([rec(420, [b"red".ljust(8, b"\0"), 10]), rec(421, [1, 2, 3, 4, 5, 10])]))
    dg.append(ipfix_msg([rec(422, [7, 1000])]))
    _codec, batch, oracle = decode(dg)
    hv, stats, ops = check(batch, oracle)
    assert stats["operations_generated"] == 3
    en = FlowEnricher(0, "t")
    gen = en.generation
    assert hv.feed(en) == 1 and hv.totals()["ops_refused"] == 2
    assert en.generation == gen + 1
    assert [g[:2] + (g[4],) for g in en.lookup(PEER, 1, [u(302, 7, 8)])] == [(0, 34, (1000).to_bytes(4, "little"))]


def test_a_batch_without_options_launches_nothing():
    dg = [ipfix_msg([(2, tmpl_record(300, T_DATA))]), ipfix_msg([(300, record(T_DATA, [1, 2, 3]) * 40)]),
          ipfix_msg([(999, b"\0" * 8)])]
    _codec, batch, oracle = decode(dg)
    hv, stats, ops = check(batch, oracle)
    assert hv.last_launches == 0 and ops == [] and stats["received_flows"] == 2


def test_operations_are_kept_per_harvester_and_a_stale_batch_is_refused():
    from netgauze_amd.options import FlowOptionsHarvester, OptionsError
    tm = ipfix_msg([(3, opt_record(400, S_SEL, F_SEL))])
    ca, ba, oa = decode([tm, ipfix_msg([(400, record(S_SEL + F_SEL, [1, 10]))])])
    cb, bb, ob = decode([tm, ipfix_msg([(400, record(S_SEL + F_SEL, [2, 20]) + record(S_SEL + F_SEL, [3, 30]))])])
    ha, _, ops_a = check(ba, oa)
    hb = FlowOptionsHarvester(0, WEIGHT)
    check(bb, ob, hb)
    assert ha.ops() == ops_a and len(hb) == 2  # another context's harvest on a second harvester leaves them
    ca.decode_datagrams([ipfix_msg([(400, record(S_SEL + F_SEL, [4, 40]))])])
    with pytest.raises(OptionsError):
        ha.harvest(ba, PEER)
    assert ha.totals()["operations_generated"] == 1 and hb.totals()["operations_generated"] == 2


def test_end_to_end_options_feed_enrichment_and_renormalization():
    from netgauze_amd.enrich import FlowEnricher
    from netgauze_amd.options import FlowOptionsHarvester
    from netgauze_amd.renormalize import FlowRenormalizer
    nf_data = [(48, 4), (1, 4), (2, 4)]  # flowSamplerId is no scope of any record below: NFv9 rows stay unscaled by it
    first = [ipfix_msg([(3, opt_record(400, S_SEL, F_SEL)), (2, tmpl_record(300, T_DATA))], domain=5),
             nf9_msg([(1, nf_opt_record(500, [(1, 4)], [(50, 4)])), (0, tmpl_record(310, nf_data))], 2, src=6),
             ipfix_msg([(400, record(S_SEL + F_SEL, [7, 1000]))], domain=5),
             nf9_msg([(500, record([(1, 4), (50, 4)], [1, 64]))], 1, src=6)]
    codec, batch, oracle = decode(first)
    hv, en = FlowOptionsHarvester(0, WEIGHT), FlowEnricher(0, "e2e")
    _hv, stats, ops = check(batch, oracle, hv)
    assert stats["operations_generated"] == 2
    assert hv.feed(en) == 2
    cache = E.Cache()
    for op in OR.harvest_batch(batch, oracle, PEER, WEIGHT)[1]:
        cache.apply(op)

    second = [ipfix_msg([(300, b"".join(record(T_DATA, [7 + (i % 2), 1000 + i, 10 + i]) for i in range(70)))], seq=1, domain=5),
              nf9_msg([(310, b"".join(record(nf_data, [1, 500 + i, 5 + i]) for i in range(9)))], 9, seq=1, src=6)]
    batch2 = codec.decode_datagrams(second)
    oracle_codec = parity.oracle_datagrams(first)[1]
    oracle2, _ = parity.oracle_datagrams(second, oracle_codec)
    eref, erows = E.enrich_batch(cache, PEER, batch2, oracle2)
    assert en.apply(batch2, PEER) == eref and eref["records_matched"] == 35 + 9
    # renorm_ref over enrich_ref: the oracle's records with the resolved sampling fields appended
    by_dg, own = {}, []
    for gs in batch2.sets():
        by_dg.setdefault(int(gs["dgram"]), []).append(gs)
    for d, (kind, pkt) in enumerate(oracle2):
        data_sets = [x for x in pkt.sets if x[0] == "Data"]
        for (_, _sid, recs), gs in zip(data_sets, by_dg.get(d, [])):
            for r, (_scope, fields) in enumerate(recs):
                own.append((fields, len(fields)))
                for g in erows[int(gs["slot"])][int(gs["rec0"]) + r] or []:
                    if g[0] == 0 and g[1] in R.PARAM_IES and g[1] != 311:
                        fields.append(O.Field(O.REGISTRY.lookup(0, g[1]), int.from_bytes(g[4], "little")))
    xref, flags = R.renormalize_batch(oracle2)
    for fields, n in own:
        del fields[n:]
    rn = FlowRenormalizer(0)
    assert rn.apply_enriched(batch2, en) == xref and xref["flows_renormalized"] >= 35
    parity.check_batch(batch2, oracle2)  # octet and packet counts, cell by cell: selectorId 8 stays unscaled
    sl = batch2.slots[[s.template_id for s in batch2.slots].index(300)]
    octets = np.frombuffer(sl.column_bytes(1).tobytes(), dtype="<u8")[:70]
    assert octets.tolist() == [(1000 + i) * (1000 if i % 2 == 0 else 1) for i in range(70)]
    got = [(d, j) for d, st, j, _c in en.json_lines(batch2, rn) if st == 0]
    assert got == E.batch_json(batch2, oracle2, erows, "e2e", flags)
