#!/usr/bin/env python3
"""Flow output (flow_output.h ngz_output_encode) on one device, beside the decode kernel of the same run.

Workload: --records T20 records in one batch through a ten-field config: six Identity integers, three
IPv4 addresses as strings and one absent IE with a default.  Each encode follows a fresh decode (an
encode is once per batch); the size passes (with their scans) and the pack passes are timed by the HIP
events round their kernels, for the default pack pass and its variants (NGZ_OUTPUT_OPT_RECOMPUTE,
NGZ_OUTPUT_OPT_IMAGE) in turn.  Prints one JSON line; --out appends a summary line per variant.

    python tools/bench_output.py --records 10000000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG = [{"name": "ip_src", "refs": [(0, 8, 0)]}, {"name": "ip_dst", "refs": [(0, 12, 0)], "transform": "String"},
          {"name": "ip_nexthop", "refs": [(0, 15, 0)]}, {"name": "iface_in", "refs": [(0, 10, 0)]},
          {"name": "iface_out", "refs": [(0, 14, 0)]}, {"name": "packets", "refs": [(0, 2, 0)]},
          {"name": "bytes", "refs": [(0, 1, 0)]}, {"name": "port_src", "refs": [(0, 7, 0)]},
          {"name": "port_dst", "refs": [(0, 11, 0)]}, {"name": "vrf_in", "refs": [(0, 234, 0)], "default": ("U32", 0)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from netgauze_amd import synth
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import FlowOutput
    assert torch.cuda.is_available(), "bench_output needs a HIP device"
    n = args.records
    _offs, rec_len = synth.field_offsets(synth.T20)
    rec = synth.t20_records(n, device="cuda")
    buf, moffs, mlens = synth.ipfix_data_stream(rec, rec_len)
    del rec
    codec = FlowInfoCodec(0, specialize=True)
    codec.decode_datagrams([synth.template_message()])
    from netgauze_amd import _lib
    if args.steps < 5:
        ap.error("--steps below 5 gives no median worth recording")
    out = FlowOutput(CONFIG)
    res = {"records": n, "steps": args.steps, "fields": len(CONFIG), "variants": {}}
    lines = []
    # the default first, then the pack pass's other variants: the same bytes, timed the same way
    for name, recompute, image in (("offsets_8k", 0, 8192), ("recompute_8k", 1, 8192), ("offsets_4k", 0, 4096), ("recompute_4k", 1, 4096)):
        out.set_option(_lib.NGZ_OUTPUT_OPT_RECOMPUTE, recompute)
        out.set_option(_lib.NGZ_OUTPUT_OPT_IMAGE, image)
        size_ms, pack_ms, decode_ms = [], [], []
        stats = None
        for step in range(args.warmup + args.steps):
            batch = codec.decode_batch(buf, moffs, mlens)
            stats = out.encode(batch)
            if step >= args.warmup:
                s, p = out.last_ms
                size_ms.append(s)
                pack_ms.append(p)
                decode_ms.append(codec.last_timing()[0])
        assert stats["rows"] == n and stats["rows_failed"] == 0, stats
        s, p, d = statistics.median(size_ms), statistics.median(pack_ms), statistics.median(decode_ms)
        res["variants"][name] = {"size_ms": round(s, 4), "pack_ms": round(p, 4), "pack_ms_min": round(min(pack_ms), 4),
                                 "pack_ms_max": round(max(pack_ms), 4), "output_bytes": stats["bytes"],
                                 "output_gb_s": round(stats["bytes"] / ((s + p) * 1e-3) / 1e9, 2), "decode_ms": round(d, 4),
                                 "encode_over_decode_time": round((s + p) / d, 3) if d else None, "launches": out.last_launches}
        lines.append("%s records=%d fields=%d pack=%s size_ms=%.4f pack_ms=%.4f (min %.4f max %.4f, median of %d) output_bytes=%d "
                     "bytes_per_row=%.2f output_GB/s=%.2f decode_kernel_ms=%.4f encode/decode_time=%.3f\n"
                     % (time.strftime("%Y-%m-%d"), n, len(CONFIG), name, s, p, min(pack_ms), max(pack_ms), len(pack_ms), stats["bytes"],
                        stats["bytes"] / n, res["variants"][name]["output_gb_s"], d, (s + p) / d if d else 0))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
