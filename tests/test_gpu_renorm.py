"""Flow renormalization on the device (include/ngz/flow_renormalize.h) against the Python
restatement of the reference (tests/renorm_ref.py) applied to the oracle's decode of the same
datagrams: every column cell, the per-row flag, the five counters and the renormalized JSON."""
import json
import math
import os
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ngz_oracle as O  # noqa: E402
import parity  # noqa: E402
import renorm_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "renorm_kats.json")) as f:
    KATS = json.load(f)
NAME = KATS["ie_ids"]
T0 = 1_700_000_000
# full wire lengths of the IEs the renormalization reads, and the shortest the decoder takes
FULL = {1: 8, 2: 8, 85: 8, 86: 8, 34: 4, 35: 1, 49: 1, 50: 4, 304: 2, 305: 4, 306: 4, 309: 4, 310: 4, 311: 8}
MINLEN = {1: 1, 2: 1, 85: 1, 86: 1, 34: 1, 35: 1, 49: 1, 50: 1, 304: 1, 305: 1, 306: 1, 309: 1, 310: 1, 311: 8}
FILLERS = [(8, 4), (7, 2), (4, 1), (12, 4), (11, 2)]  # addresses, ports, protocol
VLEN_IE = 82  # interfaceName (string)


# ----------------------------------------------------------------------------
# small message builders (netgauze_amd/synth.py style)
# ----------------------------------------------------------------------------
def tmpl_record(tid, fields):
    return struct.pack(">HH", tid, len(fields)) + b"".join(struct.pack(">HH", i, n) for i, n in fields)


def ipfix_msg(sets, seq=0, domain=1, t=T0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIII", 10, 16 + len(body), t, seq, domain) + body


def nf9_msg(sets, count, seq=0, src=1, t=T0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIIII", 9, count, 1000, t, seq, src) + body


def record(fields, values):
    """Wire bytes of one record: values[i] is an int (big endian, reduced to the field's length) or
    bytes for a variable-length field."""
    out = b""
    for (_ie, n), v in zip(fields, values):
        if n == 0xFFFF:
            out += (bytes([len(v)]) if len(v) < 255 else b"\xff" + len(v).to_bytes(3, "big")) + v
        else:
            out += (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
    return out


def messages(proto, tid, fields, recs, per_set, sets_per_msg=1, seq0=0):
    """Data messages of one template: per_set records per set."""
    msgs, sets = [], []
    for i in range(0, len(recs), per_set):
        sets.append((tid, b"".join(recs[i:i + per_set]), len(recs[i:i + per_set])))
    for i in range(0, len(sets), sets_per_msg):
        grp = sets[i:i + sets_per_msg]
        if proto == 10:
            msgs.append(ipfix_msg([(s, b) for s, b, _ in grp], seq=seq0 + i, t=T0 + i))
        else:
            msgs.append(nf9_msg([(s, b) for s, b, _ in grp], sum(n for _, _, n in grp), seq=seq0 + i, t=T0 + i))
    return msgs


def template_msg(proto, templates):
    body = b"".join(tmpl_record(tid, f) for tid, f in templates)
    return ipfix_msg([(2, body)]) if proto == 10 else nf9_msg([(0, body)], len(templates))


# ----------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------
def snapshot(batch):
    return [{f: s.column_bytes(f, rows=s.capacity).copy() for f in range(len(s.fields))} if s.n_records else {}
            for s in batch.slots]


def run(dgrams, specialize=False, renorm=None, check_json=True):
    """Decode, apply, and compare everything with the restatement.  Returns a dict of the pieces."""
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.renormalize import FlowRenormalizer
    codec = FlowInfoCodec(0, specialize=specialize)
    batch = codec.decode_datagrams(dgrams)
    oracle, _ = parity.oracle_datagrams(dgrams)
    parity.check_batch(batch, oracle)  # the decode itself agrees before anything is scaled
    before = snapshot(batch)
    ref_stats, ref_flags = R.renormalize_batch(oracle)
    rn = renorm or FlowRenormalizer(0)
    stats = rn.apply(batch)
    assert stats == ref_stats, (stats, ref_stats)
    parity.check_batch(batch, oracle)  # every cell of every OK message, scaled counts included
    after = snapshot(batch)
    # flags, and rows the apply must not touch
    hdr, sets = batch.dgram_headers(), batch.sets()
    exp_flags = [np.zeros(s.n_records, dtype=np.uint8) for s in batch.slots]
    dead = [np.zeros(s.capacity, dtype=bool) for s in batch.slots]
    for s, sl in enumerate(batch.slots):
        dead[s][sl.n_records:] = True
    per_dg = {}
    for i in range(len(sets)):
        d, slot, rec0, n = (int(sets[i][k]) for k in ("dgram", "slot", "rec0", "n"))
        k = per_dg.get(d, 0)
        per_dg[d] = k + 1
        if int(hdr[d]["status"]) != 0:
            dead[slot][rec0:rec0 + n] = True
            continue
        for r in range(n):
            if ref_flags[d].get((k, r)):
                exp_flags[slot][rec0 + r] = 1
    for s, sl in enumerate(batch.slots):
        if not sl.n_records:
            continue
        got = rn.flags(s).cpu().numpy()
        assert got.shape == (sl.n_records,) and np.array_equal(got, exp_flags[s]), (s, got[:16], exp_flags[s][:16])
        scoped = any(fi.is_scope for fi in sl.fields)
        for f in range(len(sl.fields)):
            rows = slice(None) if scoped else dead[s]
            assert np.array_equal(before[s][f][rows], after[s][f][rows]), ("untouched rows changed", s, f)
    lines = None
    if check_json:
        lines = rn.json_lines(batch)
        exp = []
        for d, (kind, val) in enumerate(oracle):
            if kind == "ok":
                exp.append((d, 0, R.packet_json(val, ref_flags[d])))
            elif kind == "err":
                exp.append((d, 2, O.dumps(val)))
        assert [(d, st, t) for d, st, t, _ in lines] == exp
    return dict(codec=codec, batch=batch, oracle=oracle, stats=stats, renorm=rn, before=before, after=after,
                flags=ref_flags, lines=lines, hdr=hdr)


# ----------------------------------------------------------------------------
# reference KATs and edges: one template and one record per case, IPFIX and NetFlow v9
# ----------------------------------------------------------------------------
def kat_value(ie, v):
    if ie == 311:
        return int(v["f64_bits"], 16) if isinstance(v, dict) else R.f64_bits(v)
    return v


@pytest.mark.parametrize("proto", [10, 9])
def test_reference_kats_and_edges(proto):
    cases = KATS["kats"] + KATS["edges"] + [
        dict(name=p["name"], input=p["sets"][-1]["records"][0]["fields"], expected=p["expected_sets"][-1]["records"][0]["fields"])
        for p in KATS["packets"] if p["sets"]]
    templates, data = [], []
    for i, c in enumerate(cases):
        fields = [(NAME[n], FULL[NAME[n]]) for n, _ in c["input"]]
        templates.append((300 + i, fields))
        rec = record(fields, [kat_value(NAME[n], v) for n, v in c["input"]])
        data += messages(proto, 300 + i, fields, [rec], 1, seq0=i)
    res = run([template_msg(proto, templates)] + data)
    assert res["stats"]["flows_processed"] == len(cases)
    # the fixture's expected fields, record by record (the oracle objects now hold the scaled values)
    for i, c in enumerate(cases):
        pkt = res["oracle"][1 + i][1]
        _scope, fields = pkt.sets[0][2][0]
        got = [[f.ie.name, f.value] for f in fields]
        exp = [[n, ("f64", kat_value(311, v)) if NAME.get(n) == 311 else v] for n, v in c["expected"] if n != "isRenormalized"]
        assert got == exp, c["name"]
        assert bool(res["flags"][1 + i].get((0, 0))) == (c["expected"][-1][0] == "isRenormalized"), c["name"]
    # the empty-flow packet case: a message without sets renders with "sets":[]
    res2 = run([ipfix_msg([], seq=1, domain=100)] if proto == 10 else [nf9_msg([], 0, seq=1)])
    assert '"sets":[]' in res2["lines"][0][2]


# ----------------------------------------------------------------------------
# row-count boundaries
# ----------------------------------------------------------------------------
BOUNDARY = [(1, 8), (2, 8), (85, 8), (86, 8), (34, 4), (35, 1)]


@pytest.mark.parametrize("proto", [10, 9])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_count_boundaries(rows, proto):
    rng = random.Random(rows * 16 + proto)
    recs = [record(BOUNDARY, [rng.getrandbits(40), rng.getrandbits(20), rng.getrandbits(63), r, rng.choice([0, 1, 3, 1000]),
                              rng.choice([1, 1, 2, 3])]) for r in range(rows)]
    # sets of 7 records, three sets per message: rec0 of most sets is not a multiple of 4
    res = run([template_msg(proto, [(256, BOUNDARY)])] + messages(proto, 256, BOUNDARY, recs, 7, 3))
    assert res["stats"]["flows_processed"] == rows
    assert res["batch"].slots[0].capacity >= rows


# ----------------------------------------------------------------------------
# differential fuzz
# ----------------------------------------------------------------------------
U32_EDGES = [0, 1, 2, 3, 10, 255, 256, 65535, (1 << 31), (1 << 32) - 1]
P_EDGES = [0, 1, 1 << 63, 0x7ff8000000000000, 0x7ff0000000000000, R.f64_bits(1.0), R.f64_bits(math.nextafter(1.0, 2.0)),
           R.f64_bits(0.1), R.f64_bits(0.5), R.f64_bits(-0.5), R.f64_bits(1e-300), R.f64_bits(1.0 / 3.0)]
C_EDGES = [0, 1, 100, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, 1 << 62, 1 << 63, (1 << 64) - 1]


def fuzz_template(rng, tid):
    ies = [ie for ie in R.PARAM_IES if rng.random() < 0.4] + [ie for ie in R.COUNT_IES if rng.random() < 0.6]
    ies += [rng.choice(ies)] if ies and rng.random() < 0.4 else []
    ies += [rng.choice(R.PARAM_IES)] if rng.random() < 0.3 else []
    rng.shuffle(ies)
    fields = []
    for ie in ies:
        if rng.random() < 0.5:
            fields.append(rng.choice(FILLERS))
        fields.append((ie, rng.randint(MINLEN[ie], FULL[ie]) if rng.random() < 0.5 else FULL[ie]))
    if not fields:
        fields = [rng.choice(FILLERS)]
    vlen = rng.random() < 0.25
    if vlen:
        first_count = next((i for i, (ie, _) in enumerate(fields) if ie in R.COUNT_IES), len(fields))
        fields.insert(rng.randint(0, first_count), (VLEN_IE, 0xFFFF))
    return tid, fields


def fuzz_value(rng, ie):
    if ie == VLEN_IE:
        return bytes(rng.choice(b"abcdefgh/0123") for _ in range(rng.randint(0, 12)))
    if ie == 311:
        return rng.choice(P_EDGES) if rng.random() < 0.6 else R.f64_bits(rng.random())
    if ie in (35, 49):
        return rng.choice([0, 1, 2, 3, 99])
    if ie == 304:
        return rng.choice([0, 1, 2, 3, 4, 5, 300])
    if ie in R.COUNT_IES:
        return rng.choice(C_EDGES) if rng.random() < 0.5 else rng.getrandbits(rng.choice([8, 32, 53, 64]))
    if ie in R.PARAM_IES:
        return rng.choice(U32_EDGES) if rng.random() < 0.6 else rng.getrandbits(32)
    return rng.getrandbits(32)


def fuzz_datagrams(first, count):
    out_t, out_d = [], []
    for t in range(first, first + count):
        rng = random.Random(0x52454E00 + t)
        tid, fields = fuzz_template(rng, 1000 + t)
        out_t.append((tid, fields))
        recs = [record(fields, [fuzz_value(rng, ie) for ie, _ in fields]) for _ in range(300)]
        out_d += messages(10, tid, fields, recs, 37, 2, seq0=t * 1000)
    return [template_msg(10, out_t)] + out_d


def test_fuzz_generic_kernels():
    """64 seeded templates x 300 records, decoded by the generic kernel (NGZ_OPT_SPECIALIZE 0)."""
    res = run(fuzz_datagrams(0, 64), specialize=False)
    assert res["stats"]["flows_processed"] == 64 * 300
    assert res["stats"]["flows_renormalized"] > 0 and res["stats"]["ie_missing_or_invalid"] > 0


@pytest.mark.parametrize("part", range(4))
def test_fuzz_specialised_kernels(part):
    """The same 64 templates decoded by their own kernels (NGZ_OPT_SPECIALIZE 1), 16 per case."""
    res = run(fuzz_datagrams(16 * part, 16), specialize=True)
    assert res["stats"]["flows_processed"] == 16 * 300


# ----------------------------------------------------------------------------
# failed messages, options data, templates without sampling IEs
# ----------------------------------------------------------------------------
VT = [(VLEN_IE, 0xFFFF), (1, 8), (2, 8), (34, 4)]


def vt_rec(i):
    return record(VT, [b"if%d" % i, 1000 + i, 10 + i, 4])


def test_failed_message_rows_are_left_alone():
    ok = [ipfix_msg([(500, b"".join(vt_rec(10 * m + i) for i in range(5)))], seq=m) for m in range(3)]
    # the last record's string runs past the set: UnexpectedEof, the message fails as a whole
    bad = ipfix_msg([(500, b"".join(vt_rec(90 + i) for i in range(4)) + bytes([200]) + b"c" * 30)], seq=9)
    res = run([template_msg(10, [(500, VT)])] + ok[:2] + [bad] + ok[2:])
    assert int(res["hdr"][3]["status"]) == 2
    assert res["stats"] == dict(flows_processed=15, flows_renormalized=15, ie_missing_or_invalid=0,
                                sampling_algorithm_inferred=15, records_dropped=0)


def test_failed_message_with_a_decoded_set():
    """A message whose first data set decodes and whose second names no template: its rows exist and stay."""
    rec = [record(BOUNDARY, [100 + i, 10, 5, 6, 3, 1]) for i in range(6)]
    ok = messages(10, 256, BOUNDARY, rec, 6)
    bad = ipfix_msg([(256, b"".join(rec)), (999, b"\0" * 8)], seq=5)
    res = run([template_msg(10, [(256, BOUNDARY)])] + ok + [bad] + ok)
    assert int(res["hdr"][2]["status"]) == 2 and res["stats"]["flows_processed"] == 12


def test_options_records_are_dropped():
    opt_fields = [(149, 4), (34, 4), (1, 8)]  # scope observationDomainId, then samplingInterval, octetDeltaCount
    opt_t = struct.pack(">HHH", 700, 3, 1) + b"".join(struct.pack(">HH", i, n) for i, n in opt_fields)
    norm = [(1, 8), (34, 4)]
    t = ipfix_msg([(2, tmpl_record(701, norm)), (3, opt_t)])
    opt_recs = b"".join(record(opt_fields, [7, 10, 100 + i]) for i in range(5))
    norm_recs = b"".join(record(norm, [200 + i, 3]) for i in range(4))
    res = run([t, ipfix_msg([(700, opt_recs), (701, norm_recs)], seq=1), ipfix_msg([(700, opt_recs)], seq=2)])
    assert res["stats"] == dict(flows_processed=4, flows_renormalized=4, ie_missing_or_invalid=0,
                                sampling_algorithm_inferred=4, records_dropped=10)
    texts = [t for _, _, t, _ in res["lines"]]
    assert "Template" not in texts[0] and texts[0].endswith('"sets":[]}}')
    assert '{"Data":{"id":700,"records":[]}}' in texts[1] and texts[1].count("isRenormalized") == 4
    assert '"samplingInterval":10' not in "".join(texts)


def test_template_without_sampling_ies_launches_nothing():
    from netgauze_amd import synth
    rec = synth.t20_records(3000)
    buf, offs, lens = synth.ipfix_data_stream(rec, 64)
    b = bytes(buf.numpy())
    dgrams = [synth.template_message()] + [b[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())]
    res = run(dgrams, check_json=False)
    assert res["renorm"].last_ms == 0.0
    assert res["stats"] == dict(flows_processed=3000, flows_renormalized=0, ie_missing_or_invalid=0,
                                sampling_algorithm_inferred=0, records_dropped=0)
    for s in range(len(res["before"])):
        for f in res["before"][s]:
            assert np.array_equal(res["before"][s][f], res["after"][s][f])


# ----------------------------------------------------------------------------
# guards and views
# ----------------------------------------------------------------------------
def test_guards_and_view_invalidation():
    from netgauze_amd import _lib
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.renormalize import FlowRenormalizer, RenormError
    fields = [(1, 8), (2, 8), (34, 4), (35, 1)]
    recs = [record(fields, [1000 + i, 10 + i, 8, 1]) for i in range(20)]
    dgrams = [template_msg(10, [(256, fields)])] + messages(10, 256, fields, recs, 20)
    codec = FlowInfoCodec(0, specialize=False)
    rn = FlowRenormalizer(0)
    batch = codec.decode_datagrams(dgrams)
    assert '"octetDeltaCount":1000}' in batch.json(1)  # loads the context's host view
    assert batch.record_fields(1, 0, 0)[0][7] == (1000).to_bytes(8, "little")
    st = rn.apply(batch)
    assert st["flows_renormalized"] == 20
    assert '"octetDeltaCount":8000}' in batch.json(1) and "isRenormalized" not in batch.json(1)
    assert batch.record_fields(1, 0, 0)[0][7] == (8000).to_bytes(8, "little")
    assert '"octetDeltaCount":8000}' in batch.json_lines()[1][2]
    cols = snapshot(batch)
    with pytest.raises(RenormError) as e:
        rn.apply(batch)
    assert e.value.code == _lib.NGZ_E_INVALID
    again = snapshot(batch)
    assert all(np.array_equal(cols[0][f], again[0][f]) for f in cols[0])
    assert rn.totals() == st
    # a new decode on the context is a new batch
    batch2 = codec.decode_datagrams(dgrams[1:])
    assert rn.apply(batch2)["flows_renormalized"] == 20
    assert rn.totals(reset=True)["flows_renormalized"] == 40 and rn.totals()["flows_processed"] == 0
    # a submitted decode that is not collected yet refuses the apply
    import torch
    from netgauze_amd import synth
    data, offs, lens = (x.cuda() for x in synth.host_batch(dgrams[1:]))
    codec.decode_batch_submit(data, offs, lens)
    out = _lib.BatchOut()
    rc = _lib.load().ngz_renorm_apply(rn._h, codec._ctx, batch2.out, None, None)
    batch3 = codec.decode_batch_wait()
    assert rc == _lib.NGZ_E_INVALID
    assert rn.apply(batch3)["flows_renormalized"] == 20
    torch.cuda.synchronize()
    del out


# ----------------------------------------------------------------------------
# into the aggregation
# ----------------------------------------------------------------------------
def test_aggregation_sums_renormalized_counts():
    import ngz_agg_oracle
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.renormalize import FlowRenormalizer
    fields = [(7, 2), (1, 8), (2, 8), (34, 4), (35, 1)]
    rng = random.Random(7)
    recs = [record(fields, [rng.choice([80, 443, 53]), rng.getrandbits(30), rng.getrandbits(16), rng.choice([1, 10, 1000]), 1])
            for _ in range(500)]
    dgrams = [template_msg(10, [(256, fields)])] + messages(10, 256, fields, recs, 50)
    agg_fields = [(0, 7, 0, 0), (0, 1, 0, 1), (0, 2, 0, 1)]  # key sourceTransportPort, Add octets and packets

    def groups(renormalize):
        codec = FlowInfoCodec(0, specialize=False)
        batch = codec.decode_datagrams(dgrams)
        if renormalize:
            FlowRenormalizer(0).apply(batch)
        agg = FlowAggregator(agg_fields)
        agg.push(batch, 4739, 0)
        return sorted((g["window_start"], g["key"], g["vals"], g["record_count"]) for g in agg.flush())

    # the oracle aggregation fed the records the restatement renormalized
    class RenormCodec(O.FlowInfoCodec):
        def decode(self, buf):
            pkt = super().decode(buf)
            if pkt is not None:
                R.renormalize_packet(pkt, R.new_stats())
            return pkt

    ref = sorted((g["window_start"], g["key"], g["vals"], g["record_count"])
                 for g in ngz_agg_oracle.aggregate_datagrams(agg_fields, dgrams, codec=RenormCodec()).flush())
    got = groups(True)
    assert got == ref
    assert groups(False) != ref  # without the apply the sums are the sampled ones
