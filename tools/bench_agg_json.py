#!/usr/bin/env python3
"""JSON lines of aggregated groups (flow_agg_json.h ngz_agg_json_encode) on one device.

Workload: tools/bench_agg_output.py's: --records T20 records decoded once, pushed into an aggregator keyed
on protocolIdentifier and destinationTransportPort over two minute windows (393 216 groups at 10^7
records) and flushed; the rows are then rendered --warmup + --steps times under each pack writer
(NGZ_AGG_JSON_OPT_WRITER 0 accumulating, 1 bytes).  Every field of a group's record is rendered, the
sub-registry key included.  Upload, size pass (with its scan) and pack pass are timed by the HIP events
round them; the whole synchronous encode call, the host's plan, row checks and staging copy included, by
the wall clock.  Beside them, from the same run: ngz_agg_output's pack rate over the same rows
(tools/bench_agg_output.py's config) and the host time of ngz_agg_flowinfo_json over the same rows through
the same binding, whose lines the device's are compared with.  Prints one JSON line; --out appends a
summary line.

    python tools/bench_agg_json.py --records 10000000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEAD = dict(shard_id=1, seq0=0, export_time_ms=1_760_000_000_123)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps below 5 gives no median worth recording")
    import torch
    import bench_agg_output
    from netgauze_amd import _lib, synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import AggFlowJson, AggFlowOutput
    assert torch.cuda.is_available(), "bench_agg_json needs a HIP device"
    n = args.records
    _offs, rec_len = synth.field_offsets(synth.T20)
    rec = synth.t20_records(n, device="cuda")
    buf, moffs, mlens = synth.ipfix_data_stream(rec, rec_len)
    del rec
    # export times restamped so that the batch spans two minute windows, as bench.py's aggregation leg does
    m = torch.arange(moffs.numel(), device=buf.device, dtype=torch.int64)
    t = 1_700_000_010 + (m * 60) // moffs.numel()
    for b in range(4):
        buf[moffs + 4 + b] = ((t >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    codec = FlowInfoCodec(0, specialize=True)
    codec.decode_datagrams([synth.template_message()])
    batch = codec.decode_batch(buf, moffs, mlens)
    agg = FlowAggregator([(0, 4, 0, 0), (0, 11, 0, 0), (0, 1, 0, 1), (0, 2, 0, 1)], capacity=1 << 20, lateness_s=60)
    agg.push(batch, 4739, 1_700_000_000_000)
    _hdr, raw = agg.flush_raw()
    out, runs, texts = AggFlowJson(), {0: ([], []), 1: ([], [])}, {}
    for step in range(args.warmup + args.steps):  # the two writers alternate, so that drift meets both alike
        for writer in (1, 0):
            out.set_option(_lib.NGZ_AGG_JSON_OPT_WRITER, writer)
            t0 = time.perf_counter()
            stats = out.encode(agg, raw, **HEAD)  # synchronous: the host's plan, row checks and staging copy, then the device
            if step >= args.warmup:
                runs[writer][1].append((time.perf_counter() - t0) * 1e3)
                runs[writer][0].append(out.last_ms())
            if step == 0:
                texts[writer] = out.result()[0]
    data = texts[0]
    assert data == texts[1]  # the option changes how the pass runs, never what it writes
    avro, avro_pack = AggFlowOutput(bench_agg_output.CONFIG), []
    for step in range(args.warmup + args.steps):
        avro_stats = avro.encode(agg, raw)
        if step >= args.warmup:
            avro_pack.append(avro.last_ms()[2])
    t0 = time.perf_counter()
    lines = agg.flowinfo_json(raw, **HEAD)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert stats["rows"] == len(raw) == len(lines) and "".join(lines).encode() == data
    med = statistics.median
    (ms, wall), (ms_b, _wall_b) = runs[0], runs[1]
    up, size, pack = (med(x) for x in zip(*ms))
    pack_b, ap_ms = med([x[2] for x in ms_b]), med(avro_pack)
    res = {"records": n, "groups": len(raw), "row_bytes": int(raw.shape[1]), "steps": args.steps,
           "upload_ms": round(up, 4), "size_ms": round(size, 4), "size_ms_min": round(min(x[1] for x in ms), 4),
           "size_ms_max": round(max(x[1] for x in ms), 4), "pack_ms": round(pack, 4), "pack_ms_min": round(min(x[2] for x in ms), 4),
           "pack_ms_max": round(max(x[2] for x in ms), 4), "encode_call_wall_ms": round(med(wall), 3), "output_bytes": stats["bytes"],
           "bytes_per_group": round(stats["bytes"] / max(len(raw), 1), 2), "pack_bytes_per_ms": round(stats["bytes"] / pack),
           "byte_writer_pack_ms": round(pack_b, 4), "byte_writer_pack_ms_min": round(min(x[2] for x in ms_b), 4),
           "byte_writer_pack_ms_max": round(max(x[2] for x in ms_b), 4), "launches": out.last_launches,
           "avro_pack_ms": round(ap_ms, 4), "avro_pack_bytes_per_ms": round(avro_stats["bytes"] / ap_ms),
           "flowinfo_json_host_ms": round(host_ms, 1)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write(time.strftime("%Y-%m-%d ") + " ".join("%s=%s" % kv for kv in res.items()) + "\n")


if __name__ == "__main__":
    main()
