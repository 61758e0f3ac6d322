"""bench.py --dump-outputs: the row sample is fixed by its seed and stays inside the slot (CPU), and
the files hold the decoded batch's own column bytes, headers and sets at the rows they name (GPU)."""
import os

import numpy as np
import pytest

import bench


@pytest.mark.parametrize("n,rows", [(0, 100), (1, 100), (100, 100), (257, 256), (1000, 512), (10**8, 130_000)])
def test_sample_rows(n, rows):
    blocks = bench.sample_rows(n, rows, np.random.default_rng(bench.DUMP_SEED))
    assert blocks == bench.sample_rows(n, rows, np.random.default_rng(bench.DUMP_SEED))
    ids = np.concatenate([np.arange(r0, r0 + k) for r0, k in blocks] or [np.zeros(0, dtype=np.int64)])
    assert len(ids) <= max(rows, 2 * bench.DUMP_BLOCK)
    assert np.all(np.diff(ids) > 0)  # sorted, no row twice
    if n:
        assert ids[0] == 0 and ids[-1] == n - 1
    if n <= rows:
        assert len(ids) == n


@pytest.mark.gpu
def test_dump_holds_the_batch(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from netgauze_amd import synth
    from netgauze_amd.flow import FlowInfoCodec
    n = 3000
    buf, offs, lens = synth.ipfix_data_stream(synth.t20_records(n), 64)
    b = bytes(buf.numpy())
    dgrams = [synth.template_message()] + [b[o:o + k] for o, k in zip(offs.tolist(), lens.tolist())]
    codec = FlowInfoCodec(0, rtc_sync=True)
    batch = codec.decode_datagrams(dgrams)
    assert batch.n_records == n
    monkeypatch.setattr(bench, "DUMP_COLUMN_VALUES", 63 * 1024)  # 1024 of the 3000 rows: four blocks
    monkeypatch.setattr(bench, "DUMP_TABLE_ROWS", 2)             # fewer than the batch's datagrams
    for d in ("a", "b"):
        bench.dump_outputs(batch, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    files = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert np.array_equal(files[f[:-4]], np.load(tmp_path / "b" / f)), f
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    (slot,) = [s for s in batch.slots if s.n_records]
    assert files["slot_records"].tolist() == [[s.template_id, s.proto, s.n_records] for s in batch.slots]
    stem = "slot%02d_p%d_t%d" % (slot.index, slot.proto, slot.template_id)
    rows = files[stem + "_rows"].astype(np.int64)
    assert bench.DUMP_BLOCK < len(rows) <= 1024 and rows[0] == 0 and rows[-1] == n - 1
    for j, f in enumerate(slot.fields):
        got = files["%s_f%03d_ie%d_%d" % (stem, j, f.pen, f.ie_id)]
        assert got.dtype == np.float32 and np.array_equal(got, slot.column_bytes(j)[rows])
    assert len(files) == 2 + len(slot.fields) + 4
    hdr = batch.dgram_headers().view(np.uint8).reshape(-1, 32)
    assert np.array_equal(files["dgram_headers"], hdr[files["dgram_headers_rows"].astype(np.int64)])
    sets = batch.sets().view(np.uint8).reshape(-1, 16)
    assert np.array_equal(files["sets"], sets[files["sets_rows"].astype(np.int64)])
    codec.close()
