"""Flow-options harvest time on one GPU (include/ngz/flow_options.h): --records T20 data records plus
--options options rows, half of a sampling template (selectorId -> samplingInterval) and half of an
interface template with variable-length interfaceName / interfaceDescription, in one batch.  The
median of --steps harvests, each after a fresh decode (wall clock round the call, and the HIP events
round its kernels), and beside it what a host would pay without this stage: ngz_columns_to_host of
the same batch into pinned memory.  Prints one JSON line.

    python tools/bench_options.py --records 10000000 --options 100000 --steps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_SEL, F_SEL = [(302, 8)], [(34, 4)]
S_IF, F_IF = [(10, 4), (14, 4)], [(82, 0xFFFF), (83, 0xFFFF)]


def spec(fields):
    return b"".join(struct.pack(">HH", i, n) for i, n in fields)


def msg(sets, seq=0):
    body = b"".join(struct.pack(">HH", sid, 4 + len(b)) + b for sid, b in sets)
    return struct.pack(">HHIII", 10, 16 + len(body), 1_700_000_000, seq, 1) + body


def options_messages(n):
    """n options rows as messages of one set of at most ~1400 bytes."""
    rows = []
    for i in range(n // 2):
        rows.append((400, struct.pack(">QI", i, 1000 + i % 7)))
        name, desc = b"xe-%d/0/%d" % (i % 8, i % 48), b"uplink to core %d" % (i % 1000)
        rows.append((401, struct.pack(">II", i, i) + bytes([len(name)]) + name + bytes([len(desc)]) + desc))
    out, cur = [], {400: b"", 401: b""}
    for tid, r in rows:
        if len(cur[tid]) + len(r) > 1400:
            out.append(msg([(tid, cur[tid])], len(out)))
            cur[tid] = b""
        cur[tid] += r
    out += [msg([(tid, b)], len(out)) for tid, b in cur.items() if b]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--options", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from netgauze_amd import _lib, synth
    from netgauze_amd.flow import FlowInfoCodec
    from netgauze_amd.options import FlowOptionsHarvester

    _offs, rec_len = synth.field_offsets(synth.T20)
    rec = synth.t20_records(a.records, device="cuda")
    buf, offs, lens = synth.ipfix_data_stream(rec, rec_len)
    del rec
    om = options_messages(a.options)
    ob = np.frombuffer(b"".join(om) + b"\0" * 16, dtype=np.uint8).copy()
    ol = np.array([len(m) for m in om], dtype=np.int64)
    n_data = int(lens.to(torch.int64).sum().item())
    oo = n_data + np.concatenate([[0], np.cumsum(ol[:-1])])
    buf = torch.cat([buf[:n_data], torch.from_numpy(ob).cuda()])
    offs = torch.cat([offs, torch.from_numpy(oo).to(offs.dtype).cuda()])
    lens = torch.cat([lens, torch.from_numpy(ol).to(lens.dtype).cuda()])
    codec = FlowInfoCodec(0, specialize=True)
    opt = struct.pack(">HHH", 400, 2, 1) + spec(S_SEL + F_SEL) + struct.pack(">HHH", 401, 4, 2) + spec(S_IF + F_IF)
    codec.decode_datagrams([synth.template_message(), msg([(3, opt)])])
    hv = FlowOptionsHarvester(0, 16)
    wall, dev, dec = [], [], []
    stats = None
    for i in range(a.warmup + a.steps):
        batch = codec.decode_batch(buf, offs, lens)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = hv.harvest(batch, "192.0.2.1")
        t1 = time.perf_counter()
        if i >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(hv.last_ms)
            dec.append(codec.last_timing()[1])
    # the yardstick: every column of the same batch to pinned host memory
    total = sum(((sl.block_bytes() + 255) & ~255) for sl in batch.slots if sl.n_records) + 4096
    host = torch.empty(total, dtype=torch.uint8).pin_memory()
    d2h = []
    for i in range(3 + 5):
        t0 = time.perf_counter()
        n = codec.columns_to_host(host.data_ptr(), total)
        t1 = time.perf_counter()
        if i >= 3:
            d2h.append((t1 - t0) * 1e3)
    print(json.dumps({"records": a.records, "options_rows": a.options, "harvest_wall_ms": statistics.median(wall),
                      "harvest_kernels_ms": statistics.median(dev), "launches": hv.last_launches,
                      "decode_pipeline_ms": statistics.median(dec), "columns_to_host_ms": statistics.median(d2h),
                      "columns_bytes": int(n), "operations": len(hv), "stats": stats, "abi": _lib.NGZ_OPTIONS_ABI_VERSION}))


if __name__ == "__main__":
    main()
