"""GPU parity of ngz_agg_push_enriched (include/ngz/flow_aggregate.h) against the composition
tests/agg_enrich_ref.py (enrichment restatement -> aggregation oracle).  Every comparison is exact:
the windows each push closes and the final flush -- keys, presence, values, counts, the three sets,
the time bounds -- the late counts, and the flowinfo_json text.  All quantities are integers or bytes.

A row that has the second of two added fields of one IE without the first cannot come out of the
enrichment cache: no sequence of operations leaves that state (tests/agg_enrich_cases.py).  The four
presence combinations in one quad therefore run on the device through ngz_agg_resolve_rows, the
resolve kernel over a mask given on the host (test_resolve_pass_over_every_presence_combination);
the whole push runs the three the cache can produce, and the composition and the plan entry are pinned
for the fourth on the CPU (tests/test_agg_enrich_ref.py, tests/test_agg_enrich_plan.py)."""
import os
import struct
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_enrich_ref as AE  # noqa: E402
import enrich_ref as E  # noqa: E402
import ngz_agg_oracle as A  # noqa: E402
from agg_enrich_ref import s, u  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

IP = "192.0.2.1"
KEY, ADD, MN, MX, OR = 0, 1, 2, 3, 4
IN, EG, OCT, VRF, NAME, SI, SRI, SSZ, MAC, OCTS = 10, 14, 1, 234, 82, 34, 50, 309, 80, 313
T3 = [(IN, 4), (EG, 4), (OCT, 8)]
LONG = "uplink-to-the-core-router-port-channel-0017"  # 43 bytes: its tail lives in the byte arena
# ingress 1 and 2 are enriched, anything else is not
OPS = [([u(IN, 1)], [u(VRF, 7), s(NAME, LONG), u(SI, 100), u(SRI, 5), u(SSZ, 9)]),
       ([u(IN, 2)], [u(VRF, 8), s(NAME, "ge-0/0/1"), u(SI, 10), u(SRI, 3), u(SSZ, 20)])]
MAIN = [(0, VRF, 0, KEY), (0, NAME, 0, KEY), (3746, 7, 0, KEY), (0, OCT, 0, ADD), (0, SI, 0, ADD), (0, SRI, 0, MN),
        (0, SSZ, 0, MX)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd.aggregate import FlowAggregator  # noqa: F401  (loads libngz.so, fails loudly)
    return torch.device("cuda:0")


def _sorted(groups):
    return sorted(groups, key=AE.group_tuple)


def quad_rows(n):
    """n records of T3 whose ingress splits every quad: rows = 1, 2 (mod 4) are enriched."""
    return [AE.record(T3, ({1: 1, 2: 2}.get(i % 4, 9), i % 3, 1 + i)) for i in range(n)]


def data_msgs(proto, tid, recs, per=256, t=AE.T0, **kw):
    return [AE.data_msg(proto, tid, recs[i:i + per], t=t, seq=1 + i, **kw) for i in range(0, len(recs), per)]


class Pipe:
    """One peer's codec, enricher and aggregator beside the composition's."""

    def __init__(self, fields, ops=OPS, options=None, capacity=1 << 12, renorm=False):
        from netgauze_amd.aggregate import FlowAggregator
        from netgauze_amd.enrich import FlowEnricher
        from netgauze_amd.flow import FlowInfoCodec
        self.fields, self.renorm = fields, renorm
        self.codec = FlowInfoCodec(0, specialize=False)
        self.en, self.cache = FlowEnricher(0, "w"), E.Cache()
        for scope, added in ops:
            AE.upsert(self.cache, IP, scope, added, enricher=self.en)
        self.agg = FlowAggregator(fields, options=options or {}, capacity=capacity)
        self.ref, self.ref_codec = None, None

    def decode(self, dgrams):
        batch = self.codec.decode_datagrams(dgrams)
        self.en.apply(batch, IP)
        if self.renorm:
            from netgauze_amd.renormalize import FlowRenormalizer
            FlowRenormalizer(0).apply_enriched(batch, self.en)
        return batch

    def push(self, dgrams, coll=5):
        late0 = self.ref.late if self.ref else 0
        late = self.agg.push_enriched(self.decode(dgrams), self.en, 4739, coll, IP)
        self.ref, self.ref_codec = AE.aggregate(self.fields, dgrams, self.cache, IP, "w", agg=self.ref, codec=self.ref_codec,
                                                renormalize=self.renorm, collection_ms=coll)
        assert late == self.ref.late - late0
        assert _sorted(self.agg.emit()) == _sorted(self.ref.emit())

    def finish(self):
        hdr, raw = self.agg.flush_raw()
        got, want = self.agg.render(hdr, raw), self.ref.flush()
        assert _sorted(got) == _sorted(want)
        by = {AE.group_tuple(g): g for g in want}
        lines = self.agg.flowinfo_json(raw, shard_id=2, seq0=7, export_time_ms=1_751_450_400_000)
        for i, (g, line) in enumerate(zip(got, lines)):
            assert line == A.FlowAggregatorOracle(self.fields).flowinfo_json(by[AE.group_tuple(g)], shard_id=2, seq=7 + i,
                                                                             export_time_ms=1_751_450_400_000)
        return got


@pytest.mark.parametrize("proto", [10, 9])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025])
def test_row_counts_in_one_slot(dev, n, proto):
    """Keys on an added u32, an added string longer than 32 bytes and the writer id; Add, Min and Max on
    added integers; the rows without the fields form the None group."""
    p = Pipe(MAIN)
    p.push([AE.template_msg(proto, [(300, T3)])] + data_msgs(proto, 300, quad_rows(n)))
    got = p.finish()
    assert p.agg.last_path() in ("general", "none")
    keys = {g["key"] for g in got}
    assert keys == ({(None, None, "w"), (7, LONG, "w"), (8, "ge-0/0/1", "w")} if n >= 3 else {(None, None, "w")})
    assert sum(g["record_count"] for g in got) == n


def test_byte_values_from_added_columns(dev):
    """A byte-wise OR of a fixed added column (macAddress) and an octetArray OR whose values come from
    the enricher's value arena."""
    ops = [([u(IN, 1)], [(0, MAC, E.K_BYTES, bytes([1, 0, 0, 0, 0, 0x10])), (0, OCTS, E.K_BYTES, bytes(range(40)))]),
           ([u(IN, 2)], [(0, MAC, E.K_BYTES, bytes([2, 0, 0, 0, 0, 0x01])), (0, OCTS, E.K_BYTES, bytes([0xF0] * 20))])]
    p = Pipe([(0, EG, 0, KEY), (0, MAC, 0, OR), (0, OCTS, 0, OR), (0, OCT, 0, ADD)], ops)
    p.push([AE.template_msg(10, [(300, T3)])] + data_msgs(10, 300, quad_rows(65)))
    got = p.finish()
    assert any(g["vals"][0] == bytes([3, 0, 0, 0, 0, 0x11]) for g in got)


def test_own_plus_added_and_two_candidates_in_one_quad(dev):
    """Indices 0 and 1 of an IE the template owns once; and two added fields of one IE: none, the first
    alone and both present within one quad."""
    tpl = [(IN, 4), (VRF, 4), (OCT, 8)]
    ops = [([u(IN, 1)], [u(VRF, 70), s(NAME, "first")]), ([u(IN, 2)], [u(VRF, 80), s(NAME, "a"), s(NAME, "b" * 40)])]
    fields = [(0, VRF, 0, KEY), (0, VRF, 1, KEY), (0, NAME, 0, KEY), (0, NAME, 1, KEY), (0, OCT, 0, ADD)]
    for proto in (10, 9):
        p = Pipe(fields, ops)
        recs = [AE.record(tpl, ({1: 1, 2: 2}.get(i % 4, 9), 5, i)) for i in range(67)]
        p.push([AE.template_msg(proto, [(300, tpl)])] + data_msgs(proto, 300, recs))
        assert {g["key"] for g in p.finish()} == {(5, None, None, None), (5, 70, "first", None), (5, 80, "a", "b" * 40)}


@pytest.mark.parametrize("width", [4, 16, 6])
@pytest.mark.parametrize("n", [1, 4, 5, 64, 257])
def test_resolve_pass_over_every_presence_combination(dev, n, width):
    """The resolve kernel alone (ngz_agg_resolve_rows) over masks no cache state produces: two
    candidates of one IE with all four presence combinations in every quad -- none, the first alone,
    the second alone, both -- rotated so each combination meets each quad position, for ordinal 0 and 1;
    and a third, unrelated column whose bit must not count.  Nothing is written past n rows."""
    import numpy as np
    from netgauze_amd.aggregate import resolve_rows
    combos = [0b000, 0b001, 0b100, 0b101, 0b010, 0b111]  # candidates are columns 0 and 2; column 1 is another IE's
    mask = np.array([combos[(i + i // 4) % len(combos)] for i in range(n)], dtype=np.uint32)
    cols = np.zeros((3, n, width), dtype=np.uint8)
    for c in range(3):
        for i in range(n):
            cols[c, i] = [(17 * c + 3 * i + b + 1) & 0xFF for b in range(width)]
    for ordinal in (0, 1, 2):
        present, cells = resolve_rows(mask, cols, width, 0b101, ordinal)
        for i in range(n):
            have = [c for c in (0, 2) if (int(mask[i]) >> c) & 1]
            want = cols[have[ordinal], i] if ordinal < len(have) else np.zeros(width, dtype=np.uint8)
            assert int(present[i]) == int(ordinal < len(have)), (i, ordinal)
            assert bytes(cells[i]) == bytes(want), (i, ordinal)
    assert {0b100} <= {int(m) for m in mask[:4]} or n < 4  # the second alone sits in the first quad


def test_resolve_pass_writer_id_after_the_added_columns(dev):
    """dataCollectionManifestName: the writer id is one more occurrence after the row's present added
    columns of that IE: a variable-length cell {0, length, 1} marking the writer's bytes."""
    import numpy as np
    from netgauze_amd.aggregate import resolve_rows
    n = 67
    mask = np.array([i % 4 for i in range(n)], dtype=np.uint32)  # columns 0 and 1: none, first, second, both
    cols = np.zeros((2, n, 16), dtype=np.uint8)
    for c in range(2):
        for i in range(n):
            cols[c, i] = list(struct.pack("<QII", 100 * c + i, 5 + c, 0))
    for ordinal in (0, 1, 2):
        present, cells = resolve_rows(mask, cols, 16, 0b11, ordinal, writer_after=True, writer_len=9)
        for i in range(n):
            have = [c for c in (0, 1) if (int(mask[i]) >> c) & 1]
            if ordinal < len(have):
                want = bytes(cols[have[ordinal], i])
            elif ordinal == len(have):
                want = struct.pack("<QII", 0, 9, 1)
            else:
                want = bytes(16)
            assert int(present[i]) == int(ordinal <= len(have)) and bytes(cells[i]) == want, (i, ordinal)


def test_two_templates_failed_message_and_dropped_options_records(dev):
    """One template owns the key IE, the other gets it added; a message that does not decode sits
    between good ones; an options template's records are in the batch: dropped, absent from the sets,
    and their export time, far ahead, moves nothing."""
    own = [(IN, 4), (VRF, 4), (OCT, 8)]
    bad = struct.pack(">HHIII", 10, 24, AE.T0, 9, 1) + struct.pack(">HH", 300, 400)
    dgrams = [AE.template_msg(10, [(300, T3), (301, own)]), AE.options_template_msg(400, [(302, 8)], [(SI, 4)]),
              AE.data_msg(10, 300, quad_rows(9), t=AE.T0 + 1, seq=1), bad,
              AE.data_msg(10, 301, [AE.record(own, (1, 7, 1000)), AE.record(own, (9, 8, 2000))], t=AE.T0 + 2, seq=2),
              AE.data_msg(10, 400, [AE.record([(302, 8), (SI, 4)], (7, 1000))] * 3, t=AE.T0 + 100_000, seq=3, domain=2)]
    p = Pipe([(0, VRF, 0, KEY), (0, OCT, 0, ADD)])
    p.push(dgrams)
    p.push([AE.data_msg(10, 300, quad_rows(5), t=AE.T0 + 3, seq=4)])  # not late: the event time did not move
    got = p.finish()
    assert {g["key"] for g in got} == {(None,), (7,), (8,)}
    assert all(t != (10, 400) for g in got for t in g["templates"]) and sum(g["record_count"] for g in got) == 16
    assert all(g["domains"] == {1} for g in got)  # the dropped records' observation domain 2 joined no set
    assert 2 not in p.agg.sets()[2]               # ... nor the dictionary


def test_path_selection_matches_the_plain_push(dev):
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import FlowAggregator
    tpl = [(IN, 4), (4, 1), (OCT, 8)]  # a one-byte key (protocolIdentifier) packs into the group tag
    recs = [AE.record(tpl, ({1: 1, 2: 2}.get(i % 4, 9), 6 + i % 3, 1 + i)) for i in range(300)]
    dgrams = [AE.template_msg(10, [(300, tpl)])] + data_msgs(10, 300, recs)
    fields = [(0, 4, 0, KEY), (0, OCT, 0, ADD)]  # touches no added column; no slot is dropped
    opts = {_lib.NGZ_AGG_OPT_LOWCARD: 1}
    p = Pipe(fields, options=opts)
    p.push(dgrams)
    plain = FlowAggregator(fields, options=opts, capacity=1 << 12)
    plain.push(p.codec.decode_datagrams(dgrams), 4739, 5, IP)
    assert p.agg.last_path() == plain.last_path() == "lowcard"
    assert _sorted(p.finish()) == _sorted(plain.flush())
    q = Pipe([(0, 4, 0, KEY), (0, SI, 0, ADD)], options=opts)  # an added column: the general path
    q.push(dgrams)
    assert q.agg.last_path() == "general"
    q.finish()


@pytest.mark.parametrize("owner", [0, 1])
def test_collided_keys_and_owner_rows(dev, owner):
    """NGZ_AGG_OPT_HASH_BITS=4: distinct added-column keys share tags, so the exact key compare and the
    re-probe run over per-row presence; with and without per-record owner rows."""
    from netgauze_amd import _lib
    ops = [([u(EG, e)], [u(VRF, 1000 + e), s(NAME, "if-%d" % e)]) for e in range(0, 40, 2)]
    recs = [AE.record(T3, (9, i % 40, 1 + i)) for i in range(400)]
    p = Pipe([(0, VRF, 0, KEY), (0, NAME, 0, KEY), (0, OCT, 0, ADD)], ops,
             options={_lib.NGZ_AGG_OPT_HASH_BITS: 4, _lib.NGZ_AGG_OPT_OWNER: owner})
    p.push([AE.template_msg(10, [(300, T3)])] + data_msgs(10, 300, recs))
    assert len(p.finish()) == 21


def test_stale_or_unapplied_enricher_is_refused(dev):
    from netgauze_amd import _lib
    from netgauze_amd.aggregate import AggError
    p = Pipe(MAIN)
    dgrams = [AE.template_msg(10, [(300, T3)])] + data_msgs(10, 300, quad_rows(8))
    batch = p.codec.decode_datagrams(dgrams)
    with pytest.raises(AggError) as e:  # never applied
        p.agg.push_enriched(batch, p.en, 4739, 5, IP)
    assert "(%d)" % _lib.NGZ_E_INVALID in str(e.value)
    p.en.apply(batch, IP)
    batch2 = p.codec.decode_datagrams(dgrams[1:])  # a later decode: the results are stale
    with pytest.raises(AggError) as e:
        p.agg.push_enriched(batch2, p.en, 4739, 5, IP)
    assert "(%d)" % _lib.NGZ_E_INVALID in str(e.value)
    assert p.agg.n_groups() == 0
    p.push(dgrams)
    p.finish()


def test_overflow_leaves_the_aggregator_as_it_was(dev):
    from netgauze_amd.aggregate import AggError
    ops = [([u(EG, e)], [s(NAME, "interface-name-longer-than-32-bytes-%03d" % e)]) for e in range(30)]
    p = Pipe([(0, NAME, 0, KEY), (0, OCT, 0, ADD)], ops, capacity=8)
    tm = AE.template_msg(10, [(300, T3)])
    p.push([tm] + data_msgs(10, 300, [AE.record(T3, (9, i % 5, 1)) for i in range(20)]))
    before = p.agg.n_groups()
    batch = p.decode(data_msgs(10, 300, [AE.record(T3, (9, i % 30, 1)) for i in range(60)], t=AE.T0 + 1))
    with pytest.raises(AggError):
        p.agg.push_enriched(batch, p.en, 4740, 6, IP)
    assert p.agg.n_groups() == before == 5
    p.push(data_msgs(10, 300, [AE.record(T3, (9, i % 5, 2)) for i in range(10)], t=AE.T0 + 2))
    got = p.finish()  # groups, dictionaries (port 4740 absent) and arena as the composition's
    assert len(got) == 5 and all(g["ports"] == {4739} for g in got)


def test_two_contexts_on_one_enricher_and_one_aggregator(dev):
    from netgauze_amd.flow import FlowInfoCodec
    p = Pipe(MAIN)
    other = FlowInfoCodec(0, specialize=False)
    d1 = [AE.template_msg(10, [(300, T3)])] + data_msgs(10, 300, quad_rows(70))
    d2 = [AE.template_msg(9, [(300, T3)])] + data_msgs(9, 300, quad_rows(33), t=AE.T0 + 1)
    b1 = p.codec.decode_datagrams(d1)
    b2 = other.decode_datagrams(d2)
    p.en.apply(b1, IP)
    p.en.apply(b2, IP)  # each context's results are its own
    p.agg.push_enriched(b1, p.en, 4739, 5, IP)
    p.agg.push_enriched(b2, p.en, 4739, 5, IP)
    p.ref, c1 = AE.aggregate(MAIN, d1, p.cache, IP, "w", collection_ms=5)
    p.ref, _ = AE.aggregate(MAIN, d2, p.cache, IP, "w", agg=p.ref, collection_ms=5)
    assert len(p.finish()) == 6


def test_sums_after_apply_enriched_are_the_renormalized_counts(dev):
    p = Pipe([(0, VRF, 0, KEY), (0, OCT, 0, ADD)], [([u(IN, 1)], [u(VRF, 7), u(SI, 100)])], renorm=True)
    p.push([AE.template_msg(10, [(300, T3)])] + data_msgs(10, 300, quad_rows(130)))
    got = {g["key"]: g["vals"][0] for g in p.finish()}
    assert got[(7,)] == 100 * sum(1 + i for i in range(130) if i % 4 == 1)
