"""Host-side mirror of the collector's flow output, over the C ABI in include/ngz/flow_output.h
(libngz.so).

`FlowOutput(fields)` stands for one validated FlowOutputConfig (crates/collector/src/flow/config.rs:56-216);
`encode(batch)` turns every record of the codec's latest DecodedBatch into its Avro datum on the device;
`slot(s)` copies one slot's datums to the host; `schema` is get_avro_schema's text; `template_plan` is
the part of the selects a template alone decides, without a device.

`AggFlowOutput(fields)` is the same config over aggregated groups (include/ngz/flow_agg_output.h): what
the reference's Avro publisher sends.  `encode(aggregator, raw)` takes the rows `FlowAggregator.flush_raw()`
/ `emit_raw()` just returned; TimestampMillisString is accepted there on the dateTime IEs.

`AggFlowJson()` is the JSON publisher over the same rows (include/ngz/flow_agg_json.h): `encode(aggregator,
raw, shard_id, seq0, export_time_ms)` renders on the device the lines `FlowAggregator.flowinfo_json` gives.

`FlowJson()` is the JSON publisher over the decoded messages themselves (include/ngz/flow_json.h):
`encode(batch)` renders on the device the line `DecodedBatch.json(d)` gives for every datagram it does not
leave to the host (`how`); `lines(batch)` fills those in.

A field is a dict: {"name", "select": "Single" | "Coalesce" | "Multi" | "Layer2SegmentId", "refs":
[(pen, ie_id, index)], "transform": "Identity" | "String" | "MplsIndex" | ..., "default": None |
(RawValue kind, value) such as ("U32", 7) or ("String", "n/a"), "encap": the Layer2SegmentId's
encapsulation type (1 VxLAN, 2 NVGRE, ("Unassigned", n))}.
"""
import ctypes
import struct
import sys

import numpy as np

from . import _lib

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _lib.load()
    return _LIB


class OutputError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def _c_fields(fields):
    """The ngz_output_field array of a config, and the objects it points into."""
    arr = (_lib.OutputField * max(len(fields), 1))()
    keep = []
    for c, f in zip(arr, fields):
        c.name = f["name"].encode()
        c.select = _lib.OUTPUT_SELECTS[f.get("select", "Single")]
        c.transform = _lib.OUTPUT_TRANSFORMS[f.get("transform", "Identity")]
        refs = (_lib.EnrichRef * max(len(f["refs"]), 1))(*[_lib.EnrichRef(*r) for r in f["refs"]])
        keep.append(refs)
        c.n_refs, c.refs = len(f["refs"]), refs
        encap = f.get("encap", 0)
        if isinstance(encap, tuple):
            c.encap_type, c.encap_unassigned = encap[1], 1
        else:
            c.encap_type = encap
        if f.get("default") is not None:
            kind, v = f["default"]
            c.default_kind = _lib.OUTPUT_DEFAULTS[kind]
            if kind in ("Bytes", "String"):
                b = v.encode() if isinstance(v, str) else bytes(v)
                c.default_bytes, c.default_len = b, len(b)
            elif kind == "F32":
                c.default_scalar = struct.unpack("<I", struct.pack("<f", v))[0]
            elif kind == "F64":
                c.default_scalar = struct.unpack("<Q", struct.pack("<d", v))[0]
            elif not isinstance(v, (list, dict)):
                c.default_scalar = int(v) % (1 << 64)
    return arr, keep


class FlowOutput:
    def __init__(self, fields, device=0):
        arr, keep = _c_fields(fields)
        h, err = ctypes.c_void_p(), ctypes.create_string_buffer(512)
        rc = lib().ngz_output_create(device, arr, len(fields), ctypes.byref(h), err, len(err))
        del keep
        if rc != 0:
            raise OutputError(err.value.decode() or "ngz_output_create failed (%d)" % rc, rc)
        self._h = h
        self.device = device
        self.n_fields = len(fields)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_output_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if sys.is_finalizing():  # the HIP runtime may be torn down already: leave it to the process exit
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise OutputError("%s (%d)" % (lib().ngz_output_last_error(self._h).decode(), rc), rc)
        return rc

    def set_option(self, opt, value):
        """ngz_output_set_option: NGZ_OUTPUT_OPT_RECOMPUTE 0 | 1, NGZ_OUTPUT_OPT_IMAGE 8192 | 4096 (how the
        pack pass runs, never what it writes)."""
        self._check(lib().ngz_output_set_option(self._h, opt, value))

    @property
    def schema(self):
        n = int(lib().ngz_output_schema(self._h, None, 0))
        buf = ctypes.create_string_buffer(n + 1)
        lib().ngz_output_schema(self._h, buf, n + 1)
        return buf.value.decode()

    def template_plan(self, tmpl_bytes, proto=10, options=False):
        """ngz_output_template_plan (no device) of one (options) template record: per field {"type",
        "nullable", "src": [template field index of each present ref, select order]}."""
        plan = _lib.OutputPlan()
        buf = (ctypes.c_uint8 * max(len(tmpl_bytes), 1)).from_buffer_copy(bytes(tmpl_bytes) or b"\0")
        rc = lib().ngz_output_template_plan(self._h, buf, len(tmpl_bytes), proto | (_lib.NGZ_OUTPUT_OPTIONS if options else 0),
                                            ctypes.byref(plan))
        if rc != 0:
            raise OutputError("ngz_output_template_plan failed (%d)" % rc, rc)
        return [{"type": _lib.OUTPUT_TYPES[p.avro_type], "nullable": bool(p.nullable), "src": [p.src[i] for i in range(p.n_present)]}
                for p in plan.f[:plan.n_fields]]

    def encode(self, batch, stream=None):
        """Encode the codec's latest DecodedBatch; this batch's counters.  The batch's input must still
        be valid: variable-length values are read from it."""
        if batch.generation != batch._codec.generation:
            raise OutputError("stale DecodedBatch: its codec has decoded another batch since", _lib.NGZ_E_INVALID)
        st = _lib.OutputStats()
        self._check(lib().ngz_output_encode(self._h, batch._codec._ctx, ctypes.byref(batch.out), ctypes.byref(st),
                                            ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def slot_pointers(self, s):
        """(device pointer of the datums, device pointer of the u64 offsets, rows, bytes) of slot s."""
        b, o, n, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().ngz_output_slot(self._h, s, ctypes.byref(b), ctypes.byref(o), ctypes.byref(n), ctypes.byref(nb)))
        return b.value, o.value, int(n.value), int(nb.value)

    def slot(self, s, guard=False):
        """Slot s on the host: (datums as bytes, offsets as a uint64 array of rows + 1); with `guard`
        the guard bytes the stage keeps after the datums follow them."""
        _b, _o, n, nb = self.slot_pointers(s)
        data = np.empty(nb + (_lib.NGZ_OUTPUT_GUARD if guard else 0), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        self._check(lib().ngz_output_to_host(self._h, s, data.ctypes.data, data.size, offs.ctypes.data, offs.size))
        return data.tobytes(), offs

    def totals(self, reset=False):
        st = _lib.OutputStats()
        self._check(lib().ngz_output_totals(self._h, ctypes.byref(st), 1 if reset else 0))
        return st.as_dict()

    @property
    def last_launches(self):
        return int(lib().ngz_output_last_launches(self._h))

    @property
    def last_ms(self):
        """(size passes with their scans, pack passes) of the last encode, device milliseconds."""
        a, b = ctypes.c_float(), ctypes.c_float()
        lib().ngz_output_last_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value


class AggFlowOutput:
    """One validated FlowOutputConfig over the groups of a FlowAggregator (ngz_agg_output)."""

    def __init__(self, fields, device=0):
        arr, keep = _c_fields(fields)
        h, err = ctypes.c_void_p(), ctypes.create_string_buffer(512)
        rc = lib().ngz_agg_output_create(device, arr, len(fields), ctypes.byref(h), err, len(err))
        del keep
        if rc != 0:
            raise OutputError(err.value.decode() or "ngz_agg_output_create failed (%d)" % rc, rc)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_agg_output_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if sys.is_finalizing():  # the HIP runtime may be torn down already: leave it to the process exit
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise OutputError("%s (%d)" % (lib().ngz_agg_output_last_error(self._h).decode(), rc), rc)
        return rc

    def schema(self):
        n = int(lib().ngz_agg_output_schema(self._h, None, 0))
        buf = ctypes.create_string_buffer(n + 1)
        lib().ngz_agg_output_schema(self._h, buf, n + 1)
        return buf.value.decode()

    def encode(self, aggregator, raw, stream=None):
        """Encode the rows `raw` ([n, row_bytes] uint8) that the aggregator's LAST flush_raw / emit_raw
        returned; this encode's counters."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        st = _lib.AggOutputStats()
        self._check(lib().ngz_agg_output_encode(self._h, aggregator._h, raw.ctypes.data if len(raw) else None, len(raw),
                                                ctypes.byref(st), ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def result_pointers(self):
        """(device pointer of the datums, device pointer of the u64 offsets, rows, bytes) of the last encode."""
        b, o, n, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().ngz_agg_output_result(self._h, ctypes.byref(b), ctypes.byref(o), ctypes.byref(n), ctypes.byref(nb)))
        return b.value, o.value, int(n.value), int(nb.value)

    def result(self, guard=False):
        """The last encode on the host: (datums as bytes, offsets as a uint64 array of rows + 1); with
        `guard` the guard bytes the stage keeps after the datums follow them."""
        _b, _o, n, nb = self.result_pointers()
        data = np.empty(nb + (_lib.NGZ_OUTPUT_GUARD if guard else 0), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        self._check(lib().ngz_agg_output_to_host(self._h, data.ctypes.data, data.size, offs.ctypes.data, offs.size))
        return data.tobytes(), offs

    def last_ms(self):
        """(upload, size pass with its scan, pack pass) of the last encode, device milliseconds."""
        t = [ctypes.c_float() for _ in range(3)]
        lib().ngz_agg_output_last_timing(self._h, *[ctypes.byref(x) for x in t])
        return tuple(x.value for x in t)

    @property
    def last_launches(self):
        return int(lib().ngz_agg_output_last_launches(self._h))


class AggFlowJson:
    """The serde JSON lines of the groups of a FlowAggregator, rendered on the device (ngz_agg_json)."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        rc = lib().ngz_agg_json_create(device, ctypes.byref(h))
        if rc != 0:
            raise OutputError("ngz_agg_json_create failed (%d)" % rc, rc)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_agg_json_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if sys.is_finalizing():  # the HIP runtime may be torn down already: leave it to the process exit
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise OutputError("%s (%d)" % (lib().ngz_agg_json_last_error(self._h).decode(), rc), rc)
        return rc

    def set_option(self, opt, value):
        """ngz_agg_json_set_option: NGZ_AGG_JSON_OPT_WRITER 0 accumulating | 1 byte writer (how the pack pass
        runs, never what it writes); NGZ_AGG_JSON_OPT_FLOATS 0 a float key or aggregated field is refused
        (NGZ_OUTPUT_E_UNSUPPORTED) | 1 a float64 one is rendered on the device (what an encode accepts;
        float32 stays refused)."""
        self._check(lib().ngz_agg_json_set_option(self._h, opt, value))

    def encode(self, aggregator, raw, shard_id=0, seq0=0, export_time_ms=0, stream=None):
        """Render the rows `raw` ([n, row_bytes] uint8) that the aggregator's LAST flush_raw / emit_raw
        returned, with the packet header of FlowAggregator.flowinfo_json; this encode's counters."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        st = _lib.AggOutputStats()
        self._check(lib().ngz_agg_json_encode(self._h, aggregator._h, raw.ctypes.data if len(raw) else None, len(raw), shard_id, seq0,
                                              export_time_ms, ctypes.byref(st), ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def result_pointers(self):
        """(device pointer of the lines, device pointer of the u64 offsets, rows, bytes) of the last encode."""
        b, o, n, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().ngz_agg_json_result(self._h, ctypes.byref(b), ctypes.byref(o), ctypes.byref(n), ctypes.byref(nb)))
        return b.value, o.value, int(n.value), int(nb.value)

    def result(self, guard=False):
        """The last encode on the host: (lines back to back as bytes, offsets as a uint64 array of rows + 1);
        with `guard` the guard bytes the stage keeps after the lines follow them."""
        _b, _o, n, nb = self.result_pointers()
        data = np.empty(nb + (_lib.NGZ_OUTPUT_GUARD if guard else 0), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        self._check(lib().ngz_agg_json_to_host(self._h, data.ctypes.data, data.size, offs.ctypes.data, offs.size))
        return data.tobytes(), offs

    def last_ms(self):
        """(upload, size pass with its scan, pack pass) of the last encode, device milliseconds."""
        t = [ctypes.c_float() for _ in range(3)]
        lib().ngz_agg_json_last_timing(self._h, *[ctypes.byref(x) for x in t])
        return tuple(x.value for x in t)

    @property
    def last_launches(self):
        return int(lib().ngz_agg_json_last_launches(self._h))


class FlowJson:
    """The serde JSON lines of the decoded messages of a batch, rendered on the device (ngz_flow_json): for
    every datagram whose `how` is LINE, what `DecodedBatch.json(d)` returns."""

    NONE, LINE, HOST = _lib.NGZ_FLOW_JSON_NONE, _lib.NGZ_FLOW_JSON_LINE, _lib.NGZ_FLOW_JSON_HOST

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        rc = lib().ngz_flow_json_create(device, ctypes.byref(h))
        if rc != 0:
            raise OutputError("ngz_flow_json_create failed (%d)" % rc, rc)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_flow_json_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if sys.is_finalizing():  # the HIP runtime may be torn down already: leave it to the process exit
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise OutputError("%s (%d)" % (lib().ngz_flow_json_last_error(self._h).decode(), rc), rc)
        return rc

    def set_option(self, opt, value):
        """ngz_flow_json_set_option: NGZ_FLOW_JSON_OPT_FLOATS 0 (default) the datagrams of a template with a
        float64 field are left to the host (HOST, `left_float`) | 1 they are rendered on the device."""
        self._check(lib().ngz_flow_json_set_option(self._h, opt, value))

    @staticmethod
    def f64_text(bits):
        """serde_json's text of the float64 with bit pattern `bits` (ngz_flow_json_f64_text: the device's
        routine compiled for the host; no HIP call)."""
        buf = ctypes.create_string_buffer(32)
        n = lib().ngz_flow_json_f64_text(bits, buf, 32)
        if n < 0:
            raise OutputError("ngz_flow_json_f64_text failed (%d)" % n, n)
        return buf.raw[:n].decode()

    def encode(self, batch, stream=None):
        """Render the codec's latest DecodedBatch; this encode's counters.  The batch's input must still be
        valid: variable-length values are read from it."""
        if batch.generation != batch._codec.generation:
            raise OutputError("stale DecodedBatch: its codec has decoded another batch since", _lib.NGZ_E_INVALID)
        st = _lib.FlowJsonStats()
        self._check(lib().ngz_flow_json_encode(self._h, batch._codec._ctx, ctypes.byref(batch.out), ctypes.byref(st),
                                               ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def result_pointers(self):
        """(device pointers of the lines, of the u64 offsets and of `how`, datagrams, bytes) of the last encode."""
        b, o, w, n, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().ngz_flow_json_result(self._h, ctypes.byref(b), ctypes.byref(o), ctypes.byref(w), ctypes.byref(n), ctypes.byref(nb)))
        return b.value, o.value, w.value, int(n.value), int(nb.value)

    def result(self, guard=False):
        """The last encode on the host: (lines back to back as bytes, offsets as a uint64 array of datagrams + 1,
        `how` as a uint8 array); with `guard` the guard bytes the stage keeps after the lines follow them."""
        _b, _o, _w, n, nb = self.result_pointers()
        data = np.empty(nb + (_lib.NGZ_OUTPUT_GUARD if guard else 0), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        how = np.zeros(n, dtype=np.uint8)
        self._check(lib().ngz_flow_json_to_host(self._h, data.ctypes.data, data.size, offs.ctypes.data, offs.size, how.ctypes.data, how.size))
        return data.tobytes(), offs, how

    def lines(self, batch):
        """Encode `batch` and return [(datagram, text)] of its OK datagrams: the device's lines, and
        `batch.json(d)` for the datagrams it leaves to the host."""
        self.encode(batch)
        data, offs, how = self.result()
        offs = offs.tolist()
        return [(d, data[offs[d]:offs[d + 1]].decode("utf-8") if h == self.LINE else batch.json(d))
                for d, h in enumerate(how.tolist()) if h != self.NONE]

    def last_ms(self):
        """(size pass, offsets, glue and pack passes) of the last encode, device milliseconds."""
        t = [ctypes.c_float() for _ in range(3)]
        lib().ngz_flow_json_last_timing(self._h, *[ctypes.byref(x) for x in t])
        return tuple(x.value for x in t)

    last_timing = last_ms

    @property
    def last_launches(self):
        return int(lib().ngz_flow_json_last_launches(self._h))
