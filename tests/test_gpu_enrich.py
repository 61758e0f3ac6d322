"""Flow enrichment on the device (include/ngz/flow_enrich.h) against the Python restatement of the
reference (tests/enrich_ref.py) over the oracle's decode of the same datagrams: every added cell,
every presence mask and the four counters, with the context's own columns and JSON untouched."""
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import enrich_ref as E  # noqa: E402
import ngz_oracle as O  # noqa: E402
import parity  # noqa: E402
import renorm_ref as R  # noqa: E402
from netgauze_amd.enrich import EnrichError  # noqa: E402

T0 = 1_700_000_000
PEER = "10.0.0.1"
ROW_COUNTS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025]
V6 = bytes.fromhex("20010db8000000000000000000000005")


def u(ie, v, w):
    return (0, ie, E.K_UINT, int(v).to_bytes(w, "little"))


def s(ie, text):
    return (0, ie, E.K_STR, text)


def tmpl_record(tid, fields):
    return struct.pack(">HH", tid, len(fields)) + b"".join(struct.pack(">HH", i, n) for i, n in fields)


def ipfix_msg(sets, seq=0, domain=1, t=T0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIII", 10, 16 + len(body), t, seq, domain) + body


def nf9_msg(sets, count, seq=0, src=1, t=T0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIIII", 9, count, 1000, t, seq, src) + body


def record(fields, values):
    out = b""
    for (_ie, n), v in zip(fields, values):
        if n == 0xFFFF:
            out += (bytes([len(v)]) if len(v) < 255 else b"\xff" + len(v).to_bytes(2, "big")) + v
        elif isinstance(v, bytes):
            out += v
        else:
            out += (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
    return out


# templates: (id, fields)
T_IF = [(8, 4), (10, 4), (14, 4), (1, 8), (2, 8)]          # ingress / egress, no sampling IE
T_SEL = [(302, 4), (1, 8), (2, 8), (34, 4)]                # selectorId on 4 wire bytes, its own samplingInterval
T_TWO = [(10, 4), (10, 4), (1, 8)]                         # two ingressInterface
T_NONE = [(4, 1), (1, 8), (2, 8)]                          # no scope IE at all
T_VLEN = [(82, 0xFFFF), (10, 4), (1, 8)]                   # the scope field after a variable-length field
T_V6 = [(27, 16), (1, 8)]
NF_IF = [(10, 4), (1, 4)]                                  # NetFlow v9: domain = source_id
TEMPLATES = [(300, T_IF), (301, T_SEL), (302, T_TWO), (303, T_NONE), (304, T_VLEN), (305, T_V6)]
OPT_ID = 400                                               # options template: scope meteringProcessId, samplingInterval


def fill_cache(en, ref, ip=PEER):
    ops = [
        ("upsert", 0, 64, [], [u(34, 100, 4), u(35, 1, 1)]),                       # unconditional global scope
        ("upsert", 1000, 64, [], [s(84, b"dom")]),
        ("upsert", 0, 16, [u(302, 1, 8)], [s(84, b"gsel")]),                        # 16 / 64 / 64 on samplerName
        ("upsert", 1000, 64, [u(302, 1, 8)], [s(84, b"sel1"), u(138, 7, 8)]),
        ("upsert", 2000, 16, [], [u(34, 50, 4)]),                                  # loses to the global 64
        ("upsert", 1000, 64, [u(10, 2, 4), u(14, 3, 4)], [u(34, 200, 4)]),         # ties with the global: later wins
        ("upsert", 0, 64, [u(10, 1, 4), u(10, 2, 4)], [u(138, 77, 8)]),            # a scope on index 1
        ("upsert", 0, 64, [(0, 27, E.K_BYTES, V6)], [s(82, b"v6"), (0, 56, E.K_BYTES, b"\1\2\3\4\5\6")]),
        ("upsert", 2000, 200, [u(10, 3, 4)], [s(82, b"")]),                        # strings of 0, 5 and 300 bytes
        ("upsert", 0, 64, [u(10, 5, 4)], [s(82, b"eth05")]),
        ("upsert", 0, 64, [u(10, 4, 4)], [s(82, b"x" * 300)]),
    ]
    ops += [("upsert", 0, 64, [u(10, v, 4)], [s(82, b"if%d" % v)]) for v in (0, 1, 2, 6, 7)]
    for kind, dom, w, scope, fields in ops:
        en.upsert(ip, dom, w, scope, fields)
        ref.apply({"op": kind, "ip": ip, "domain": dom, "weight": w, "scope": scope, "fields": fields})


def build_datagrams(rng):
    opt = struct.pack(">HHH", OPT_ID, 2, 1) + struct.pack(">HH", 143, 4) + struct.pack(">HH", 34, 4)
    dg = [ipfix_msg([(2, b"".join(tmpl_record(t, f) for t, f in TEMPLATES)), (3, opt)]),
          nf9_msg([(0, tmpl_record(310, NF_IF))], 1, src=2000)]
    doms = [1000, 2000, 3000, 0]

    def some(fields, n):
        return [record(fields, [rng.randrange(0, 8) if ie in (10, 14, 302) else rng.randrange(1, 1 << 20) for ie, _ in fields])
                for _ in range(n)]

    seq = 0
    for tid, fields in TEMPLATES[:4]:
        for i in range(6):
            dg.append(ipfix_msg([(tid, b"".join(some(fields, 1 + rng.randrange(40))))], seq=seq, domain=doms[i % 4]))
            seq += 1
    # one message in the middle that fails: a good set, then a set of an unknown template
    dg.append(ipfix_msg([(300, b"".join(some(T_IF, 9))), (999, b"\0" * 8)], seq=seq, domain=1000))
    for i in range(4):
        recs = [record(T_VLEN, [b"n" * rng.randrange(0, 30), rng.randrange(0, 8), 5]) for _ in range(1 + rng.randrange(20))]
        dg.append(ipfix_msg([(304, b"".join(recs))], seq=seq, domain=doms[i % 4]))
        recs = [record(T_V6, [V6 if rng.random() < 0.5 else bytes(16), 5]) for _ in range(1 + rng.randrange(20))]
        dg.append(ipfix_msg([(305, b"".join(recs))], seq=seq, domain=doms[i % 4]))
        dg.append(ipfix_msg([(OPT_ID, struct.pack(">II", 7, 10) * 3)], seq=seq, domain=doms[i % 4]))  # dropped records
        recs = some(NF_IF, 1 + rng.randrange(20))
        dg.append(nf9_msg([(310, b"".join(recs))], len(recs), seq=seq, src=doms[i % 4]))
    return dg


def boundary_datagrams(rng):
    """One template per row count of ROW_COUNTS, records packed as sets of 1 to 300."""
    tmpls = [(500 + i, T_IF) for i in range(len(ROW_COUNTS))]
    dg = [ipfix_msg([(2, b"".join(tmpl_record(t, f) for t, f in tmpls))])]
    for (tid, _), n in zip(tmpls, ROW_COUNTS):
        left = n
        while left:
            k = min(left, rng.randrange(1, 301))
            recs = [record(T_IF, [9, rng.randrange(0, 8), rng.randrange(0, 5), 100, 1]) for _ in range(k)]
            dg.append(ipfix_msg([(tid, b"".join(recs))], domain=rng.choice([1000, 2000, 3000])))
            left -= k
    return dg


def snapshot(batch):
    return [{f: sl.column_bytes(f, rows=sl.capacity).copy() for f in range(len(sl.fields))} if sl.n_records else {}
            for sl in batch.slots]


def check(en, ref, batch, oracle, peer=PEER, trace=None):
    """Apply and compare every slot with the restatement; returns the batch's counters."""
    before, json_before = snapshot(batch), batch.json_lines()
    ref_stats, ref_rows = E.enrich_batch(ref, peer, batch, oracle, trace)
    stats = en.apply(batch, peer)
    assert stats == ref_stats, (stats, ref_stats)
    arena = en.value_arena()
    for si, sl in enumerate(batch.slots):
        cols = en.columns(si)
        refs = [(c["pen"], c["ie_id"], c["index"]) for c in cols]
        assert refs == sorted(refs) and len(set(refs)) == len(refs) <= 32, refs
        mask = en.mask(si).cpu().numpy().view(np.uint32)
        data = [c["data"].cpu().numpy() for c in cols]
        assert len(mask) == sl.n_records
        for r in range(sl.n_records):
            want = {(g[0], g[1], g[2]): g for g in (ref_rows[si][r] or [])}
            assert set(want) <= set(refs), (si, r, want, refs)
            exp_mask = 0
            for c, ref_c in enumerate(refs):
                cell = bytes(data[c][r])
                if ref_c not in want:
                    assert cell == bytes(len(cell)), (si, r, c, cell)
                    continue
                exp_mask |= 1 << c
                _pen, _ie, _idx, kind, value, _w = want[ref_c]
                if cols[c]["kind"] == E.K_VLEN:
                    off, ln, zero = struct.unpack("<QII", cell)
                    assert zero == 0 and arena[off:off + ln] == value and ln == len(value), (si, r, c, cell, value)
                    assert cols[c]["is_string"] == (kind == E.K_STR)
                else:
                    assert cols[c]["kind"] == kind and cell == value, (si, r, c, cell, value)
            assert int(mask[r]) == exp_mask, (si, r, int(mask[r]), exp_mask)
    # the typed per-row view on every row of the small slots: canonical order, the writer id last
    for si, sl in enumerate(batch.slots):
        if sl.n_records > 70:
            continue
        for r in range(sl.n_records):
            if ref_rows[si][r] is None:  # scope fields, or a message that did not decode
                with pytest.raises(EnrichError):
                    en.row_fields(si, r)
                continue
            exp = [(g[0], g[1], g[4], g[3] == E.K_STR) for g in ref_rows[si][r]]
            exp.append((3746, 7, en.writer_id.encode(), True))
            got = en.row_fields(si, r)
            assert [(g[0], g[1], g[3], g[4]) for g in got] == exp, (si, r, got, exp)
    after = snapshot(batch)
    for b, a in zip(before, after):  # nothing written into the context's arena
        assert b.keys() == a.keys() and all(np.array_equal(b[k], a[k]) for k in b)
    assert batch.json_lines() == json_before
    return stats


def decode(dgrams):
    from netgauze_amd.flow import FlowInfoCodec
    codec = FlowInfoCodec(0, specialize=False)
    batch = codec.decode_datagrams(dgrams)
    oracle, _ = parity.oracle_datagrams(dgrams)
    parity.check_batch(batch, oracle)
    return codec, batch, oracle


def test_templates_messages_and_cache_shapes():
    from netgauze_amd.enrich import FlowEnricher
    dgrams = build_datagrams(random.Random(11))
    codec, batch, oracle = decode(dgrams)
    assert sum(1 for k, _ in oracle if k == "err") == 1
    en, ref = FlowEnricher(0, "writer-1"), E.Cache()
    fill_cache(en, ref)
    trace = {}
    E.enrich_batch(ref, PEER, batch, oracle, trace)  # on the CPU, before use: the fixture reaches the cases
    assert trace.get("max_scopes", 0) >= 2 and trace.get("ties", 0) >= 1, trace
    stats = check(en, ref, batch, oracle)
    assert stats["records_dropped"] == 12 and stats["records_matched"] > 0
    assert en.totals() == stats
    # a cache change between applies: re-applying the same batch gives the new result
    en.delete(PEER, 0, 64, [], [(0, 34)])
    ref.apply({"op": "delete", "ip": PEER, "domain": 0, "weight": 64, "scope": [], "ies": [(0, 34)]})
    stats2 = check(en, ref, batch, oracle)
    assert stats2["fields_added"] < stats["fields_added"]
    # another peer's IP matches nothing
    none = check(en, ref, batch, oracle, peer="10.0.0.2")
    assert none["records_matched"] == 0 and none["fields_added"] == 0
    assert none["records_processed"] == stats["records_processed"]
    assert en.last_ms >= 0
    del codec


def test_row_boundaries():
    from netgauze_amd.enrich import FlowEnricher
    codec, batch, oracle = decode(boundary_datagrams(random.Random(5)))
    assert sorted(sl.n_records for sl in batch.slots) == ROW_COUNTS
    en, ref = FlowEnricher(0, "w"), E.Cache()
    fill_cache(en, ref)
    stats = check(en, ref, batch, oracle)
    assert stats["records_processed"] == sum(ROW_COUNTS) == stats["records_matched"]
    del codec


@pytest.mark.parametrize("bits", [0, 13])
def test_five_thousand_interface_scopes(bits):
    from netgauze_amd.enrich import FlowEnricher
    rng = random.Random(7)
    tmpl = ipfix_msg([(2, tmpl_record(300, T_IF))])
    recs = [record(T_IF, [9, rng.randrange(0, 6000), 1, 100, 1]) for _ in range(700)]
    dgrams = [tmpl] + [ipfix_msg([(300, b"".join(recs[i:i + 70]))], domain=1000) for i in range(0, 700, 70)]
    codec, batch, oracle = decode(dgrams)
    en, ref = FlowEnricher(0, "w"), E.Cache()
    if bits:
        en.set_table_bits(bits)  # 5 000 entries in 8 192 slots: long probe chains
    for v in range(5000):
        fields = [s(82, b"if%d" % v)]
        en.upsert(PEER, 0 if v % 2 else 1000, 64, [u(10, v, 4)], fields)
        ref.apply({"op": "upsert", "ip": PEER, "domain": 0 if v % 2 else 1000, "weight": 64, "scope": [u(10, v, 4)],
                   "fields": fields})
    stats = check(en, ref, batch, oracle)
    assert 0 < stats["records_matched"] < 700
    del codec


def test_limits_and_preconditions():
    from netgauze_amd import _lib
    from netgauze_amd.enrich import EnrichError, FlowEnricher
    codec, batch, oracle = decode([ipfix_msg([(2, tmpl_record(300, T_IF))]),
                                   ipfix_msg([(300, record(T_IF, [9, 1, 2, 100, 1]))], domain=5)])
    en = FlowEnricher(0, "w")
    for i in range(33):  # 33 distinct added FieldRefs for one slot
        en.upsert(PEER, 0, 1, [], [u(34, i, 4)] * (i + 1))
    with pytest.raises(EnrichError) as ei:
        en.apply(batch, PEER)
    assert ei.value.code == _lib.NGZ_E_LIMIT
    en2 = FlowEnricher(0, "w")
    shapes = [[], [u(8, 9, 4)], [u(10, 1, 4)], [u(14, 2, 4)], [u(1, 100, 8)], [u(2, 1, 8)], [u(8, 9, 4), u(10, 1, 4)],
              [u(10, 1, 4), u(14, 2, 4)], [u(14, 2, 4), u(10, 1, 4)]]
    for sc in shapes[:8]:
        en2.upsert(PEER, 0, 1, sc, [u(34, 1, 4)])
    assert en2.apply(batch, PEER)["fields_added"] == 1
    en2.upsert(PEER, 0, 1, shapes[8], [u(34, 1, 4)])  # a ninth shape the template can satisfy
    with pytest.raises(EnrichError) as ei:
        en2.apply(batch, PEER)
    assert ei.value.code == _lib.NGZ_E_LIMIT
    en3 = FlowEnricher(0, "w")
    for d in range(1, 255):
        en3.upsert(PEER, d, 1, [], [u(34, 1, 4)])
    with pytest.raises(EnrichError) as ei:
        en3.apply(batch, PEER)
    assert ei.value.code == _lib.NGZ_E_LIMIT
    del codec, oracle


def test_results_are_kept_per_context_and_refused_after_the_next_decode():
    from netgauze_amd.enrich import FlowEnricher
    tmpl = ipfix_msg([(2, tmpl_record(300, T_IF))])
    a = [tmpl, ipfix_msg([(300, b"".join(record(T_IF, [9, v % 8, 1, 100, 1]) for v in range(37)))], domain=1000)]
    b = [tmpl, ipfix_msg([(300, b"".join(record(T_IF, [9, 5, 1, 100, 1]) for v in range(900)))], domain=2000)]
    codec_a, batch_a, oracle_a = decode(a)
    codec_b, batch_b, oracle_b = decode(b)
    en, ref = FlowEnricher(0, "w"), E.Cache()
    fill_cache(en, ref)
    en.apply(batch_a, PEER)
    mask_a = en.mask(0, batch_a).cpu().tolist()
    cells_a = [c["data"].cpu().numpy().copy() for c in en.columns(0, batch_a)]
    check(en, ref, batch_b, oracle_b)  # a larger batch on another context
    assert en.mask(0, batch_a).cpu().tolist() == mask_a  # A's results stand
    assert all(np.array_equal(x, c["data"].cpu().numpy()) for x, c in zip(cells_a, en.columns(0, batch_a)))
    assert len(en.row_fields(0, 0, batch_a)) >= 2
    ctx_a = batch_a._codec._ctx
    codec_a.decode_datagrams(a)  # the context's next decode: its results are refused from here on
    from netgauze_amd import _lib
    n, m = _lib.ctypes.c_uint32(), _lib.ctypes.c_void_p()
    lib = _lib.load()
    assert lib.ngz_enrich_slot_columns(en._h, ctx_a, 0, None, 0, _lib.ctypes.byref(m), _lib.ctypes.byref(n)) == _lib.NGZ_E_INVALID
    assert lib.ngz_enrich_row_fields(en._h, ctx_a, 0, 0, None, 0) == _lib.NGZ_E_INVALID
    assert en.mask(0, batch_b).shape[0] == 900
    del codec_b, oracle_a


T_PLAIN = [(10, 4), (1, 8), (2, 8)]            # no sampling IE of its own
T_OWN = [(10, 4), (1, 8), (2, 8), (34, 4)]     # its own samplingInterval


def enriched_oracle(ref, batch, oracle, peer=PEER):
    """The restatement's enriched records: the resolved sampling fields appended to each record's
    fields (what renormalize() reads of them); returns how many fields each record had."""
    _stats, rows = E.enrich_batch(ref, peer, batch, oracle)
    hdr_sets = {}
    for gs in batch.sets():
        hdr_sets.setdefault(int(gs["dgram"]), []).append(gs)
    own = []
    for d, (kind, pkt) in enumerate(oracle):
        if kind != "ok":
            continue
        data_sets = [x for x in pkt.sets if x[0] == "Data"]
        for (_, _sid, recs), gs in zip(data_sets, hdr_sets.get(d, [])):
            for r, (scope, fields) in enumerate(recs):
                own.append((fields, len(fields)))
                for g in rows[int(gs["slot"])][int(gs["rec0"]) + r] or []:
                    if g[0] == 0 and g[1] in R.PARAM_IES and g[1] != 311:
                        fields.append(O.Field(O.REGISTRY.lookup(0, g[1]), int.from_bytes(g[4], "little")))
    return own


def test_apply_enriched_scales_by_the_enrichment_sampling_parameters():
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.enrich import FlowEnricher
    from netgauze_amd.renormalize import FlowRenormalizer, RenormError
    rng = random.Random(3)
    plain = [record(T_PLAIN, [rng.randrange(1, 4), rng.randrange(1, 1 << 30), rng.randrange(1, 1000)]) for _ in range(130)]
    own = [record(T_OWN, [rng.randrange(1, 4), rng.randrange(1, 1 << 30), rng.randrange(1, 1000), 10]) for _ in range(67)]
    dgrams = [ipfix_msg([(2, tmpl_record(600, T_PLAIN) + tmpl_record(601, T_OWN))]),
              ipfix_msg([(600, b"".join(plain[:64]))], domain=1000), ipfix_msg([(601, b"".join(own[:30]))], domain=1000),
              ipfix_msg([(600, b"".join(plain[64:70])), (999, b"\0" * 8)], domain=1000),  # fails: its rows stay
              ipfix_msg([(600, b"".join(plain[70:]))], domain=2000), ipfix_msg([(601, b"".join(own[30:]))], domain=2000)]
    codec, batch, oracle = decode(dgrams)
    en, ref = FlowEnricher(0, "w"), E.Cache()
    for dom, w, scope, fields in [(0, 64, [u(10, 1, 4)], [u(34, 100, 4)]),            # 100 beats the record's own 10
                                  (2000, 64, [u(10, 2, 4)], [u(34, 7, 4), s(82, b"two")]),
                                  (0, 64, [], [s(84, b"any")])]:                      # ingress 3: no sampling match
        en.upsert(PEER, dom, w, scope, fields)
        ref.apply({"op": "upsert", "ip": PEER, "domain": dom, "weight": w, "scope": scope, "fields": fields})
    rn = FlowRenormalizer(0)
    with pytest.raises(RenormError):
        rn.apply_enriched(batch, en)  # the enricher has not applied this batch
    check(en, ref, batch, oracle)
    lens = enriched_oracle(ref, batch, oracle)
    ref_stats, ref_flags = R.renormalize_batch(oracle)
    for fields, n in lens:
        del fields[n:]
    # the cases are in the batch: a plain record now scaled, own 10 losing to 100, an unmatched row keeping its own
    assert ref_stats["flows_renormalized"] > 67 and ref_stats["flows_processed"] == 191
    stats = rn.apply_enriched(batch, en)
    assert stats == ref_stats, (stats, ref_stats)
    parity.check_batch(batch, oracle)  # every cell: scaled counts, and the failed message's rows untouched
    sets, hdr = batch.sets(), batch.dgram_headers()
    per_dg = {}
    for i in range(len(sets)):
        d, slot, rec0, n = (int(sets[i][k]) for k in ("dgram", "slot", "rec0", "n"))
        k = per_dg.get(d, 0)
        per_dg[d] = k + 1
        flags = rn.flags(slot).cpu().numpy()
        for r in range(n):
            exp = 1 if int(hdr[d]["status"]) == 0 and ref_flags[d].get((k, r)) else 0
            assert int(flags[rec0 + r]) == exp, (d, r)
    with pytest.raises(RenormError):
        rn.apply_enriched(batch, en)  # the same batch twice
    # the JSON with both appended fields: the writer id, then isRenormalized on the flagged records
    _st, rows = E.enrich_batch(ref, PEER, batch, oracle)
    exp = E.batch_json(batch, oracle, rows, en.writer_id, ref_flags)
    got = [(d, text) for d, status, text, _c in en.json_lines(batch, rn) if status == 0]
    assert got == exp
    assert sum(text.count('"isRenormalized":true') for _d, text in got) == ref_stats["flows_renormalized"]
    # the aggregation sums the scaled counts
    want = {}
    for kind, pkt in oracle:
        if kind != "ok":
            continue
        for _sid, (_scope, fields) in pkt.data_records():
            key = fields[0].value
            o, p, c = want.get(key, (0, 0, 0))
            want[key] = (o + fields[1].value, p + fields[2].value, c + 1)
    agg = FlowAggregator([(0, 10, 0, 0), (0, 1, 0, 1), (0, 2, 0, 1)])
    agg.push(batch, 4739, 0)
    got = sorted((int(g["vals"][0]), int(g["vals"][1]), g["record_count"]) for g in agg.flush())
    assert got == sorted(want.values()), (got, want)
    del codec


def test_enriched_json_and_the_plan_of_every_template():
    from netgauze_amd.enrich import FlowEnricher
    dgrams = build_datagrams(random.Random(21))
    codec, batch, oracle = decode(dgrams)
    en, ref = FlowEnricher(0, "writer-json"), E.Cache()
    for dom, w, scope, fields in [(0, 64, [], [u(34, 100, 4)]), (1000, 64, [], [s(84, b"dom")]),
                                  (0, 64, [u(10, 4, 4)], [s(82, b'q"\\' + b"x" * 300)]), (0, 64, [u(10, 3, 4)], [s(82, b"")]),
                                  (1000, 64, [u(302, 1, 8)], [u(138, 7, 8), s(84, b"sel1")]),
                                  (0, 64, [u(10, 1, 4), u(10, 2, 4)], [u(138, 77, 8)]),
                                  (0, 64, [(0, 27, E.K_BYTES, V6)], [s(82, b"v6")])]:
        en.upsert(PEER, dom, w, scope, fields)
        ref.apply({"op": "upsert", "ip": PEER, "domain": dom, "weight": w, "scope": scope, "fields": fields})
    plain = batch.json_lines()
    _st, rows = E.enrich_batch(ref, PEER, batch, oracle)
    check(en, ref, batch, oracle)
    lines = en.json_lines(batch)
    exp = E.batch_json(batch, oracle, rows, en.writer_id)
    assert [(d, text) for d, status, text, _c in lines if status == 0] == exp
    # error datagrams as ngz_batch_json renders them; template and options-template sets are gone
    assert [x for x in lines if x[1] != 0] == [x for x in plain if x[1] != 0] and len(lines) == len(plain)
    assert not any('"Template"' in text or '"OptionsTemplate"' in text for _d, st, text, _c in lines if st == 0)
    assert all(text.count('"dataCollectionManifestName":"writer-json"') == sum(
        len([r for r in recs if not len(r[0])]) for k, _sid, recs in oracle[d][1].sets if k == "Data")
        for d, st, text, _c in lines if st == 0)
    # the no-device plan names the columns the apply produced, for every template of the batch
    wire = {300: T_IF, 301: T_SEL, 302: T_TWO, 303: T_NONE, 304: T_VLEN, 305: T_V6, 310: NF_IF}
    for si, sl in enumerate(batch.slots):
        if sl.template_id == OPT_ID:
            continue
        plan = en.template_plan(PEER, tmpl_record(sl.template_id, wire[sl.template_id]), sl.proto)
        assert [c[:3] for c in plan["columns"]] == [(c["pen"], c["ie_id"], c["index"]) for c in en.columns(si)], si
        assert [(c[3], c[4]) for c in plan["columns"]] == [(c["kind"], c["width"]) for c in en.columns(si)], si
    en.forget(batch)
    with pytest.raises(EnrichError):
        en.columns(0, batch)
    del codec
