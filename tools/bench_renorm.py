#!/usr/bin/env python3
"""Renormalization apply (flow_renormalize.h ngz_renorm_apply) on one device, beside the decode
kernel of the same run.

Workload: a 64-byte, 20-field IPFIX template (T20 with samplingInterval and samplingAlgorithm in
place of two fields of the same lengths) carrying octetDeltaCount, packetDeltaCount,
samplingInterval, samplingAlgorithm; --records rows in one batch.  Each apply follows a fresh
decode (an apply is once per batch); only the apply is timed, by the HIP events round its kernels.
Prints one JSON line; --out appends a summary line to a text file.

    python tools/bench_renorm.py --records 100000000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TID = 256
# row bytes the apply moves: samplingInterval (4) + samplingAlgorithm (1) read, two 8-byte counts
# read and written, one flag byte written
PARAM_BYTES, COUNT_BYTES, FLAG_BYTES = 5, 2 * 8 * 2, 1


def template():
    from netgauze_amd import synth
    swap = {15: (34, 4), 60: (35, 1)}
    return [swap.get(ie, (ie, n)) for ie, n in synth.T20]


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
    from netgauze_amd.renormalize import FlowRenormalizer
    assert torch.cuda.is_available(), "bench_renorm needs a HIP device"
    fields = template()
    offs, rec_len = synth.field_offsets(fields)
    o = dict(zip([f for f, _ in fields], offs))
    n = args.records
    rec = synth.t20_records(n, device="cuda")
    rec[:, o[35]] = 1 + (rec[:, o[35] - 1] & 1)       # samplingAlgorithm 1 | 2
    rec[:, o[34]:o[34] + 2] = 0                       # samplingInterval < 65536
    rec[:, o[1]:o[1] + 3] = 0                         # counts below 2^40: the products stay in range
    rec[:, o[2]:o[2] + 3] = 0
    buf, moffs, mlens = synth.ipfix_data_stream(rec, rec_len, tid=TID)
    del rec
    codec = FlowInfoCodec(0, specialize=True)
    codec.decode_datagrams([synth.template_message(TID, fields)])
    rn = FlowRenormalizer(0)
    apply_ms, decode_ms = [], []
    stats = None
    for step in range(args.warmup + max(args.steps, 20)):
        batch = codec.decode_batch(buf, moffs, mlens)
        stats = rn.apply(batch)
        if step >= args.warmup:
            apply_ms.append(rn.last_ms)
            decode_ms.append(codec.last_timing()[0])
    assert stats["flows_processed"] == n and stats["flows_renormalized"] == n, stats
    a, d = statistics.median(apply_ms), statistics.median(decode_ms)
    apply_bytes = n * (PARAM_BYTES + COUNT_BYTES + FLAG_BYTES)
    decode_bytes = n * 2 * rec_len  # wire bytes read + canonical column bytes written
    res = {"records": n, "steps": len(apply_ms), "apply_ms": round(a, 4), "apply_ms_min": round(min(apply_ms), 4),
           "apply_ms_max": round(max(apply_ms), 4), "apply_bytes": apply_bytes,
           "apply_tb_s": round(apply_bytes / (a * 1e-3) / 1e12, 3), "decode_ms": round(d, 4),
           "decode_bytes": decode_bytes, "decode_tb_s": round(decode_bytes / (d * 1e-3) / 1e12, 3),
           "bytes_per_row": {"params_read": PARAM_BYTES, "counts_read_written": COUNT_BYTES, "flags_written": FLAG_BYTES}}
    res["apply_over_decode_rate"] = round(res["apply_tb_s"] / res["decode_tb_s"], 3) if res["decode_tb_s"] else None
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("%s records=%d apply_ms=%.4f (min %.4f max %.4f, median of %d) apply_bytes=%d apply_TB/s=%.3f "
                    "decode_kernel_ms=%.4f decode_TB/s=%.3f ratio=%.3f\n"
                    % (time.strftime("%Y-%m-%d"), n, a, min(apply_ms), max(apply_ms), len(apply_ms), apply_bytes,
                       res["apply_tb_s"], d, res["decode_tb_s"], res["apply_over_decode_rate"] or 0))


if __name__ == "__main__":
    main()
