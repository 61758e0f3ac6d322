#!/usr/bin/env python3
"""Avro datums of aggregated groups (flow_agg_output.h ngz_agg_output_encode) on one device.

Workload: --records T20 records decoded once, pushed into an aggregator keyed on protocolIdentifier and
destinationTransportPort over two minute windows (393 216 groups at 10^7 records) and flushed; the rows are then encoded --warmup +
--steps times through a config of the keys, the sums and the fields only a group's record has.  Upload,
size pass (with its scan) and pack pass are timed by the HIP events round them; the whole synchronous encode call,
the host's row checks and staging copy included, by the wall clock.  Beside them, from the same
run: the column encoder's pack rate over the decoded batch (tools/bench_output.py's config) and the host
time of ngz_agg_flowinfo_json over the same rows.  Prints one JSON line; --out appends a summary line.

    python tools/bench_agg_output.py --records 10000000 --steps 20 --warmup 3
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

TS = "TimestampMillisString"
# protocolIdentifier has a sub-registry: no accepted transform reads it, so the config leaves that key out
CONFIG = [{"name": "collected", "refs": [(0, 258, 0)], "transform": TS}, {"name": "port_dst", "refs": [(0, 11, 0)]},
          {"name": "bytes", "refs": [(0, 1, 0)]}, {"name": "packets", "refs": [(0, 2, 0)]},
          {"name": "flows", "refs": [(0, 375, 0)]}, {"name": "window_start", "refs": [(3746, 1, 0)], "transform": TS},
          {"name": "window_end", "refs": [(3746, 2, 0)], "transform": TS},
          {"name": "exporter", "refs": [(0, 403, 0), (0, 404, 0)], "select": "Coalesce", "transform": "String"},
          {"name": "exporter_port", "refs": [(3746, 4, 0)]}, {"name": "template", "refs": [(3746, 3, 0)], "default": ("U16", 0)}]


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
    import bench_output
    from netgauze_amd import synth
    from netgauze_amd.aggregate import FlowAggregator
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import AggFlowOutput, FlowOutput
    assert torch.cuda.is_available(), "bench_agg_output needs a HIP device"
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
    # the column encoder over the same batch, for scale
    col, col_pack = FlowOutput(bench_output.CONFIG), []
    for step in range(args.warmup + args.steps):
        col_stats = col.encode(batch)
        if step >= args.warmup:
            col_pack.append(col.last_ms[1])
    agg = FlowAggregator([(0, 4, 0, 0), (0, 11, 0, 0), (0, 1, 0, 1), (0, 2, 0, 1)], capacity=1 << 20, lateness_s=60)
    agg.push(batch, 4739, 1_700_000_000_000)
    _hdr, raw = agg.flush_raw()
    out = AggFlowOutput(CONFIG)
    ms, wall = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        stats = out.encode(agg, raw)  # synchronous: the host's plan, row checks and staging copy, then the device
        if step >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(out.last_ms())
    t0 = time.perf_counter()
    lines = agg.flowinfo_json(raw)
    json_ms = (time.perf_counter() - t0) * 1e3
    assert stats["rows"] == len(raw) == len(lines)
    up, size, pack = (statistics.median(x) for x in zip(*ms))
    cp, call = statistics.median(col_pack), statistics.median(wall)
    res = {"records": n, "groups": len(raw), "row_bytes": int(raw.shape[1]), "steps": args.steps, "fields": len(CONFIG),
           "upload_ms": round(up, 4), "size_ms": round(size, 4), "pack_ms": round(pack, 4), "encode_call_wall_ms": round(call, 3),
           "pack_ms_min": round(min(m[2] for m in ms), 4), "pack_ms_max": round(max(m[2] for m in ms), 4),
           "output_bytes": stats["bytes"], "pack_bytes_per_ms": round(stats["bytes"] / pack), "launches": out.last_launches,
           "column_pack_ms": round(cp, 4), "column_pack_bytes_per_ms": round(col_stats["bytes"] / cp),
           "flowinfo_json_host_ms": round(json_ms, 1)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("%s records=%d groups=%d row_bytes=%d fields=%d encode_call_wall_ms=%.3f of which device: upload_ms=%.4f size_ms=%.4f pack_ms=%.4f (min %.4f max %.4f, median of %d) "
                    "output_bytes=%d bytes_per_group=%.2f pack_bytes/ms=%d column_pack_bytes/ms=%d flowinfo_json_host_ms=%.1f\n"
                    % (time.strftime("%Y-%m-%d"), n, len(raw), raw.shape[1], len(CONFIG), call, up, size, pack, res["pack_ms_min"],
                       res["pack_ms_max"], len(ms), stats["bytes"], stats["bytes"] / max(len(raw), 1), res["pack_bytes_per_ms"],
                       res["column_pack_bytes_per_ms"], json_ms))


if __name__ == "__main__":
    main()
