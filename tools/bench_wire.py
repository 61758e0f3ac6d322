#!/usr/bin/env python3
"""IPFIX messages written again from the decoded columns (flow_wire.h ngz_wire_encode) on one device.

Workload: --records T20 records in IPFIX messages of 1023-record sets.  Each step decodes the batch and
encodes it, so the decode kernel's time (ngz_last_timing) and the encode's passes (HIP events: size,
offsets, glue, pack) come from the same process and the same batch; the whole synchronous encode call, the
host's plan and upload included, by the wall clock.  Beside them the pack pass of ngz_flow_json_encode over
the same batch.  The pack pass is set against the bytes it moves: 63 B of columns read and 64 B written per
T20 record.  Checked once before timing: every message equals its input with the high byte of
tcpControlBits zero (what the reference's writer gives).  Prints one JSON line; --out appends a summary line.

    python tools/bench_wire.py --records 1000000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps below 5 gives no median worth recording")
    import torch
    from netgauze_amd import synth
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.output import FlowJson
    from netgauze_amd.wire import FlowWire
    assert torch.cuda.is_available(), "bench_wire needs a HIP device"
    codec = FlowInfoCodec(0, specialize=True)
    codec.decode_datagrams([synth.template_message()])
    offs, rec_len = synth.field_offsets(synth.T20)
    rec = synth.t20_records(args.records, device="cuda")
    rec[:, offs[[f for f, _ in synth.T20].index(6)]] = 0  # tcpControlBits keeps its low byte
    buf, moffs, mlens = synth.ipfix_data_stream(rec, rec_len)
    fw, fj, res = FlowWire(), FlowJson(), {"records": args.records, "steps": args.steps}
    batch = codec.decode_batch(buf, moffs, mlens)
    stats = fw.encode(batch)
    ptr, _o, _h, n, nb = fw.result_pointers()
    assert stats["wire"] == n == batch.n_dgrams and nb == buf.numel() - 16
    got = torch.empty(nb, dtype=torch.uint8, device="cuda")
    from netgauze_amd import _lib
    assert _lib.hip().hipMemcpy(got.data_ptr(), ptr, nb, 3) == 0  # device to device
    assert torch.equal(got, buf[:nb]), "the messages are not their input"
    ms, wall, dec, jpack = [], [], [], []
    for step in range(args.warmup + args.steps):
        batch = codec.decode_batch(buf, moffs, mlens)
        t0 = time.perf_counter()
        stats = fw.encode(batch)  # synchronous: the host's plan and upload, then the device
        w = (time.perf_counter() - t0) * 1e3
        fj.encode(batch)
        if step >= args.warmup:
            wall.append(w)
            ms.append(fw.last_ms())
            dec.append(codec.last_timing()[0])
            jpack.append(fj.last_ms()[2])
    med = statistics.median
    size, offsets, glue, pack = (med(x) for x in zip(*ms))
    moved = args.records * (63 + 64)
    res.update(dgrams=batch.n_dgrams, sets=batch.n_sets, size_ms=round(size, 4), offsets_ms=round(offsets, 4), glue_ms=round(glue, 4),
               pack_ms=round(pack, 4), pack_ms_min=round(min(x[3] for x in ms), 4), pack_ms_max=round(max(x[3] for x in ms), 4),
               encode_call_wall_ms=round(med(wall), 3), output_bytes=stats["bytes"], pack_moved_bytes=moved,
               pack_gb_per_s=round(moved / pack / 1e6, 1), decode_kernel_ms=round(med(dec), 4), pack_over_decode=round(pack / med(dec), 2),
               flow_json_pack_ms=round(med(jpack), 4), launches=fw.last_launches)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write(time.strftime("%Y-%m-%d ") + " ".join("%s=%s" % kv for kv in res.items()) + "\n")


if __name__ == "__main__":
    main()
