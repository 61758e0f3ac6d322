#!/usr/bin/env python3
"""JSON lines of decoded messages (flow_json.h ngz_flow_json_encode) on one device.

Workload: --records T20 records in IPFIX messages of 1023-record sets, decoded once; the batch is then
rendered --warmup + --steps times.  Every field of every record is rendered.  The size pass (set pass, tile
table, counting renderers), the offsets (the two sums and the scan) and the glue and pack passes are timed by
the HIP events round them; the whole synchronous encode call, the host's plan and upload included, by the
wall clock.  Beside them, from the same process: the host time of ngz_batch_json over a batch of the same
shape (--host-records caps it: the host renders some microseconds per record), whose lines the device's are
compared with; `host_over_device` scales it to --records by its per-record time.  The pack rate of
ngz_agg_json_encode to set beside this one comes from tools/bench_agg_json.py, run next to it.  Prints one
JSON line; --out appends a summary line.

--floats: the same batch with T20's packetDeltaCount (IE 2, 8 bytes) replaced by samplingProbability (IE 311,
float64) in template 257: seeded finite bit patterns of either sign with the exponent field anywhere below
1024, so nearly every value prints 16 or 17 digits and an exponent, the longest texts there are.  The stage runs
with NGZ_FLOW_JSON_OPT_FLOATS 1; ngz_batch_json over the same batch is what those datagrams cost without it.

    python tools/bench_flow_json.py --records 1000000 --steps 20 --warmup 3
    python tools/bench_flow_json.py --records 1000000 --steps 20 --warmup 3 --floats
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def decode(codec, synth, n, floats=False):
    offs, rec_len = synth.field_offsets(synth.T20)
    rec = synth.t20_records(n, device="cuda")
    if floats:  # the top exponent bit cleared: every pattern is finite
        rec[:, offs[[f for f, _ in synth.T20].index(2)]] &= 0xBF
    buf, moffs, mlens = synth.ipfix_data_stream(rec, rec_len, tid=synth.T20_ID + int(floats))
    return codec.decode_batch(buf, moffs, mlens), (buf, moffs, mlens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--host-records", type=int, default=1_000_000, help="records of the batch ngz_batch_json renders")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--floats", action="store_true", help="T20 with samplingProbability in place of packetDeltaCount, the option on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps below 5 gives no median worth recording")
    import torch
    from netgauze_amd import synth
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import FlowJson
    assert torch.cuda.is_available(), "bench_flow_json needs a HIP device"
    codec = FlowInfoCodec(0, specialize=True)
    fj, res = FlowJson(), {"records": args.records, "steps": args.steps}
    if args.floats:
        from netgauze_amd import _lib
        codec.decode_datagrams([synth.template_message(synth.T20_ID + 1, [(311, 8) if f == 2 else (f, ln) for f, ln in synth.T20])])
        fj.set_option(_lib.NGZ_FLOW_JSON_OPT_FLOATS, 1)
        res["variant"] = "samplingProbability"
    else:
        codec.decode_datagrams([synth.template_message()])
    n_host = min(args.records, args.host_records)
    batch, keep = decode(codec, synth, n_host, args.floats)  # the host function's batch, checked line for line
    stats = fj.encode(batch)
    data, offs, how = fj.result()
    t0 = time.perf_counter()
    host = batch.json_lines()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert all(h == FlowJson.LINE for h in how.tolist()) and stats["lines"] == len(host) == batch.n_dgrams
    assert "".join(js for _d, _st, js, _c in host).encode() == data
    res.update(host_records=n_host, batch_json_host_ms=round(host_ms, 1), batch_json_host_us_per_record=round(host_ms * 1e3 / n_host, 3))
    if n_host != args.records:
        del batch, keep, host, data
        batch, keep = decode(codec, synth, args.records, args.floats)
    ms, wall = [], []
    for step in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        stats = fj.encode(batch)  # synchronous: the host's plan and upload, then the device
        if step >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(fj.last_ms())
    med = statistics.median
    size, offsets, pack = (med(x) for x in zip(*ms))
    res.update(dgrams=batch.n_dgrams, sets=batch.n_sets, size_ms=round(size, 4), size_ms_min=round(min(x[0] for x in ms), 4),
               size_ms_max=round(max(x[0] for x in ms), 4), offsets_ms=round(offsets, 4), pack_ms=round(pack, 4),
               pack_ms_min=round(min(x[2] for x in ms), 4), pack_ms_max=round(max(x[2] for x in ms), 4),
               encode_call_wall_ms=round(med(wall), 3), output_bytes=stats["bytes"], bytes_per_record=round(stats["bytes"] / args.records, 2),
               pack_bytes_per_ms=round(stats["bytes"] / pack), launches=fj.last_launches,
               host_over_device=round(host_ms / n_host * args.records / med(wall), 1))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write(time.strftime("%Y-%m-%d ") + " ".join("%s=%s" % kv for kv in res.items()) + "\n")


if __name__ == "__main__":
    main()
