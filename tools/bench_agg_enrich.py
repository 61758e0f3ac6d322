"""Aggregation over enriched records on one GPU (ngz_agg_push_enriched, include/ngz/flow_aggregate.h):
T20 records with ingressInterface reduced mod --scopes, a cache of that many interface scopes each
adding an ingressVRFID (u32) and an interfaceName; per step decode, enrich, then
  - push_enriched keyed on the ADDED u32, Add octetDeltaCount / packetDeltaCount: the push's device
    time and, of it, the resolve kernel's (HIP events, ngz_agg_last_timing / _last_resolve_timing);
  - in the same process a plain push keyed on the scope field itself (ingressInterface): the same
    group count, no added column.
Each aggregator is flushed after every push, so every push meets an empty table.  Prints one JSON
line; --write also rewrites its part of profiles/agg_enrich/summary.txt (the parent-against-tree
section there is kept).

    python tools/bench_agg_enrich.py --records 10000000 --steps 10 --warmup 2 --write
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
    ap.add_argument("--scopes", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--write", action="store_true", help="rewrite profiles/agg_enrich/summary.txt")
    a = ap.parse_args()
    import torch
    from netgauze_amd import _lib, buildinfo, synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.enrich import FlowEnricher
    from netgauze_amd.flow import FlowInfoCodec

    offs_, rec_len = synth.field_offsets(synth.T20)
    off = dict(zip([ie for ie, _ in synth.T20], offs_))
    rec = synth.t20_records(a.records, device="cuda")
    o = off[10]  # ingressInterface, big endian on the wire: reduce mod --scopes
    v = (rec[:, o + 2].to(torch.int32) * 256 + rec[:, o + 3].to(torch.int32)) % a.scopes
    rec[:, o] = 0
    rec[:, o + 1] = 0
    rec[:, o + 2] = (v >> 8).to(torch.uint8)
    rec[:, o + 3] = (v & 0xFF).to(torch.uint8)
    buf, offs, lens = synth.ipfix_data_stream(rec, rec_len)
    del rec, v
    codec = FlowInfoCodec(0, specialize=True)
    codec.decode_datagrams([synth.template_message()])
    en = FlowEnricher(0, "bench")
    peer = "192.0.2.1"
    u32 = lambda ie, x: (0, ie, _lib.K_UINT, int(x).to_bytes(4, "little"))  # noqa: E731
    for x in range(a.scopes):
        en.upsert(peer, 0, 64, [u32(10, x)], [u32(234, 100000 + x), (0, 82, _lib.K_STR, b"if%d" % x)])
    values = [(0, 1, 0, _lib.NGZ_AGG_ADD), (0, 2, 0, _lib.NGZ_AGG_ADD)]
    enriched = FlowAggregator([(0, 234, 0, _lib.NGZ_AGG_KEY)] + values)
    plain = FlowAggregator([(0, 10, 0, _lib.NGZ_AGG_KEY)] + values)
    e_ms, r_ms, p_ms, apply_ms = [], [], [], []
    groups = [0, 0]
    paths = ["", ""]
    for i in range(a.warmup + a.steps):
        batch = codec.decode_batch(buf, offs, lens)
        en.apply(batch, peer)
        enriched.push_enriched(batch, en, 4739, 0, peer)
        t_e, t_r, paths[0] = enriched.push_ms(), enriched.resolve_ms(), enriched.last_path()
        groups[0] = len(enriched.flush_raw()[0])
        plain.push(batch, 4739, 0, peer)
        t_p, paths[1] = plain.push_ms(), plain.last_path()
        groups[1] = len(plain.flush_raw()[0])
        if i >= a.warmup:
            e_ms.append(t_e)
            r_ms.append(t_r)
            p_ms.append(t_p)
            apply_ms.append(en.last_ms)
    torch.cuda.synchronize()
    med = statistics.median
    out = {"records": a.records, "scopes": a.scopes, "steps": a.steps, "push_enriched_ms": med(e_ms),
           "push_enriched_min_max_ms": [min(e_ms), max(e_ms)], "resolve_ms": med(r_ms), "plain_push_ms": med(p_ms),
           "plain_push_min_max_ms": [min(p_ms), max(p_ms)], "enrich_apply_ms": med(apply_ms),
           "groups": {"enriched": groups[0], "plain": groups[1]}, "paths": {"enriched": paths[0], "plain": paths[1]},
           "records_per_s_enriched": a.records / med(e_ms) * 1e3, "agg_source_hash": buildinfo.agg_source_hash()}
    print(json.dumps(out))
    if a.write:
        path = os.path.join(ROOT, "profiles", "agg_enrich", "summary.txt")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        # the parent-against-tree section of the file, taken by hand with bench.py --agg, is kept
        kept, mark = "", "bench.py --agg, parent against this tree"
        if os.path.exists(path):
            text = open(path).read()
            kept = text[text.index(mark):] if mark in text else ""
        with open(path, "w") as f:
            f.write("Aggregation over enriched records (ngz_agg_push_enriched): tools/bench_agg_enrich.py\n\n")
            f.write("%d T20 records, %d scopes each adding a u32 and a name string; medians of %d steps, device ms\n"
                    % (a.records, a.scopes, a.steps))
            f.write("  push_enriched keyed on the added u32   %.3f ms (min %.3f, max %.3f), path %s, %d groups\n"
                    % (out["push_enriched_ms"], min(e_ms), max(e_ms), paths[0], groups[0]))
            f.write("    of which the resolve kernel          %.3f ms\n" % out["resolve_ms"])
            f.write("  plain push keyed on the scope field    %.3f ms (min %.3f, max %.3f), path %s, %d groups\n"
                    % (out["plain_push_ms"], min(p_ms), max(p_ms), paths[1], groups[1]))
            f.write("  enrichment apply                       %.3f ms\n" % out["enrich_apply_ms"])
            f.write("aggregation sources %s\n\n" % out["agg_source_hash"])
            f.write(kept)


if __name__ == "__main__":
    main()
