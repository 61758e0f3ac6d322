"""Enrichment apply time on one GPU (include/ngz/flow_enrich.h): T20 records with ingressInterface
reduced mod 4096, a cache of 4 096 interface scopes each adding interfaceName and one global scope
adding samplingInterval and samplingAlgorithm; the median of --steps applies (HIP events round the
kernels), then one ngz_renorm_apply_enriched.  Prints one JSON line.

    python tools/bench_enrich.py --records 10000000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--table-bits", type=int, default=0)
    a = ap.parse_args()
    import torch
    from netgauze_amd import _lib, synth
    from netgauze_amd.enrich import FlowEnricher
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.renormalize import FlowRenormalizer

    offs_, rec_len = synth.field_offsets(synth.T20)
    off = dict(zip([ie for ie, _ in synth.T20], offs_))
    rec = synth.t20_records(a.records, device="cuda")
    o = off[10]  # ingressInterface, big endian on the wire: reduce mod 4096
    rec[:, o] = 0
    rec[:, o + 1] = 0
    rec[:, o + 2] &= 0x0F
    buf, offs, lens = synth.ipfix_data_stream(rec, rec_len)
    del rec
    codec = FlowInfoCodec(0, specialize=True)
    codec.decode_datagrams([synth.template_message()])
    en = FlowEnricher(0, "bench")
    if a.table_bits:
        en.set_table_bits(a.table_bits)
    peer = "192.0.2.1"
    u32 = lambda ie, v: (0, ie, _lib.K_UINT, int(v).to_bytes(4, "little"))  # noqa: E731
    en.upsert(peer, 0, 64, [], [u32(34, 100), (0, 35, _lib.K_UINT, b"\x01")])
    for v in range(4096):
        en.upsert(peer, 0, 64, [u32(10, v)], [(0, 82, _lib.K_STR, b"if%d" % v)])
    ms, dec = [], []
    stats = None
    for i in range(a.warmup + a.steps):
        batch = codec.decode_batch(buf, offs, lens)
        stats = en.apply(batch, peer)
        if i >= a.warmup:
            ms.append(en.last_ms)
            dec.append(codec.last_timing()[0])
    rn = FlowRenormalizer(0)
    rstats = rn.apply_enriched(batch, en)
    torch.cuda.synchronize()
    # algorithmic bytes per row, by the plan: the 4-byte key column and the row byte read; the added
    # columns (samplingInterval 4, samplingAlgorithm 1, interfaceName descriptor 16) and the mask written
    row_bytes = 4 + 1 + 4 + 1 + 16 + 4
    med, dmed = statistics.median(ms), statistics.median(dec)
    t20_bytes = 2 * rec_len  # wire bytes read + canonical column bytes written, as tools/bench_renorm.py
    print(json.dumps({"records": a.records, "apply_ms": med, "bytes_per_row": row_bytes,
                      "tbps": a.records * row_bytes / med / 1e9, "decode_kernel_ms": dmed,
                      "decode_tbps": a.records * t20_bytes / dmed / 1e9,
                      "ratio_to_decode": (a.records * row_bytes / med) / (a.records * t20_bytes / dmed),
                      "apply_enriched_ms": rn.last_ms, "stats": stats, "renorm_stats": rstats}))


if __name__ == "__main__":
    main()
