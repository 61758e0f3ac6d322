"""Host-side mirror of the collector's flow enrichment, over the C ABI in
include/ngz/flow_enrich.h (libngz.so).

`FlowEnricher(device, writer_id)` stands for one EnrichmentActor shard
(crates/collector/src/flow/enrichment/actor.rs) with its EnrichmentCache (enrichment/cache.rs).
`upsert` / `delete` / `delete_all` are the cache operations and `lookup` is
get_enrichment_fields for one record; none of them touches the device.  `apply(batch, peer)`
resolves every record of the codec's latest DecodedBatch on the device: the fields the reference
appends land in added columns (`columns(slot)`) with one presence mask per row (`mask(slot)`).

A field is a tuple (pen, ie_id, kind, value bytes) with the value in the canonical column
encoding (kind is a _lib.K_* constant, K_STR for a string).
"""
import ctypes
import sys

from . import _lib

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _lib.load()
    return _LIB


class EnrichError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def _field_array(fields, keep):
    """ngz_enrich_field[] of [(pen, ie_id, kind, bytes)]; the value buffers go into `keep`."""
    arr = (_lib.EnrichField * max(len(fields), 1))()
    for i, (pen, ie, kind, value) in enumerate(fields):
        value = bytes(value)
        buf = ctypes.create_string_buffer(value, max(len(value), 1))
        keep.append(buf)
        arr[i].pen, arr[i].ie_id, arr[i].kind, arr[i].len = pen, ie, kind, len(value)
        arr[i].value = ctypes.cast(buf, ctypes.c_void_p)
    return arr


class FlowEnricher:
    def __init__(self, device=0, writer_id="netgauze_amd"):
        h = ctypes.c_void_p()
        rc = lib().ngz_enrich_create(device, writer_id.encode("utf-8"), ctypes.byref(h))
        if rc != 0:
            raise EnrichError("ngz_enrich_create(%d) failed (%d)" % (device, rc), rc)
        self._h = h
        self.device = device
        self.writer_id = writer_id

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_enrich_destroy(self._h)
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
            raise EnrichError("%s (%d)" % (lib().ngz_enrich_last_error(self._h).decode(), rc), rc)
        return rc

    # --- cache ---------------------------------------------------------------------------------
    def _op(self, kind, ip, domain, weight, scope, fields=(), ies=()):
        keep = []
        op = _lib.EnrichOperation()
        op.kind, op.weight, op.peer, op.obs_domain_id = kind, weight, _lib.EnrichPeer.of(ip), domain
        sc, fl = _field_array(list(scope), keep), _field_array(list(fields), keep)
        ia = (_lib.EnrichIe * max(len(ies), 1))()
        for i, (pen, ie) in enumerate(ies):
            ia[i].pen, ia[i].ie_id = pen, ie
        op.n_scope, op.n_fields, op.n_ies = len(scope), len(fields), len(ies)
        op.scope, op.fields, op.ies = sc, fl, ia
        self._check(lib().ngz_enrich_op(self._h, ctypes.byref(op)))

    def upsert(self, ip, domain, weight, scope, fields):
        self._op(_lib.NGZ_ENRICH_UPSERT, ip, domain, weight, scope, fields=fields)

    def delete(self, ip, domain, weight, scope, ies):
        self._op(_lib.NGZ_ENRICH_DELETE, ip, domain, weight, scope, ies=ies)

    def delete_all(self, ip, domain, weight, scope):
        self._op(_lib.NGZ_ENRICH_DELETE_ALL, ip, domain, weight, scope)

    @property
    def peer_count(self):
        return int(lib().ngz_enrich_peer_count(self._h))

    @property
    def generation(self):
        return int(lib().ngz_enrich_generation(self._h))

    def set_table_bits(self, bits):
        """NGZ_ENRICH_OPT_TABLE_BITS: force the device lookup tables to 2**bits slots (0: sized by entries)."""
        self._check(lib().ngz_enrich_set_option(self._h, _lib.NGZ_ENRICH_OPT_TABLE_BITS, bits))

    def lookup(self, ip, domain, record):
        """get_enrichment_fields for one record ([(pen, ie_id, kind, bytes)], its non-scope fields):
        [(pen, ie_id, index, kind, bytes, weight)] in ascending (pen, ie_id, index)."""
        keep = []
        rec = _field_array(list(record), keep)
        peer = _lib.EnrichPeer.of(ip)
        cap = 64
        while True:
            out = (_lib.EnrichResolved * cap)()
            n = self._check(lib().ngz_enrich_lookup(self._h, ctypes.byref(peer), domain, rec, len(record), out, cap))
            if n <= cap:
                break
            cap = n
        return [(o.pen, o.ie_id, o.index, o.kind, ctypes.string_at(o.value, o.len) if o.len else b"", o.weight)
                for o in out[:n]]

    # --- device --------------------------------------------------------------------------------
    @staticmethod
    def _fresh(batch):
        if batch.generation != batch._codec.generation:
            raise EnrichError("stale DecodedBatch: its codec has decoded another batch since", _lib.NGZ_E_INVALID)

    def apply(self, batch, peer, stream=None):
        """Enrich the codec's latest DecodedBatch for the exporter `peer` (an IP address string);
        the four counters of this batch."""
        self._fresh(batch)
        self._batch = batch
        st = _lib.EnrichStats()
        p = _lib.EnrichPeer.of(peer)
        self._check(lib().ngz_enrich_apply(self._h, batch._codec._ctx, ctypes.byref(batch.out), ctypes.byref(p),
                                           ctypes.byref(st), ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def totals(self, reset=False):
        st = _lib.EnrichStats()
        self._check(lib().ngz_enrich_totals(self._h, ctypes.byref(st), 1 if reset else 0))
        return st.as_dict()

    def _ctx(self, batch):
        batch = batch if batch is not None else getattr(self, "_batch", None)
        if batch is None:
            raise EnrichError("no batch applied yet", _lib.NGZ_E_INVALID)
        return batch._codec._ctx

    def _slot(self, slot, batch=None):
        ctx = self._ctx(batch)
        n, mask = ctypes.c_uint32(), ctypes.c_void_p()
        nc = self._check(lib().ngz_enrich_slot_columns(self._h, ctx, slot, None, 0, ctypes.byref(mask), ctypes.byref(n)))
        cols = (_lib.EnrichColumn * max(nc, 1))()
        self._check(lib().ngz_enrich_slot_columns(self._h, ctx, slot, cols, nc, None, None))
        return list(cols[:nc]), mask.value, n.value

    def _device_copy(self, ptr, nbytes):
        import torch
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda:%d" % self.device)
        if nbytes:
            torch.cuda.synchronize(self.device)
            rc = _lib.hip().hipMemcpy(t.data_ptr(), ptr, nbytes, 3)  # hipMemcpyDeviceToDevice
            if rc != 0:
                raise EnrichError("hipMemcpy D2D failed: %d" % rc, _lib.NGZ_E_DEVICE)
        return t

    def columns(self, slot, batch=None):
        """The added columns of a slot of `batch` (default: the batch last applied), while it is its codec's latest: [{"pen", "ie_id", "index", "kind",
        "is_string", "width", "data"}], data a torch.uint8 device tensor [n_records, width] (a copy)."""
        cols, _mask, n = self._slot(slot, batch)
        return [{"pen": c.pen, "ie_id": c.ie_id, "index": c.index, "kind": c.kind, "is_string": bool(c.is_string),
                 "width": c.width, "data": self._device_copy(c.data, n * c.width).view(n, c.width)} for c in cols]

    def mask(self, slot, batch=None):
        """One presence word per row of a slot: bit c = added column c is present.  A torch.int32
        device tensor (a copy; the bits of the uint32_t)."""
        import torch
        _cols, mask, n = self._slot(slot, batch)
        return self._device_copy(mask, 4 * n).view(torch.int32)

    def row_fields(self, slot, row, batch=None):
        """The fields appended to one record (ngz_enrich_row_fields), the writer id last:
        [(pen, ie_id, kind, value bytes, is_string)]; kind K_VLEN for a variable-length value."""
        ctx = self._ctx(batch)
        n = self._check(lib().ngz_enrich_row_fields(self._h, ctx, slot, row, None, 0))
        out = (_lib.FieldValue * max(n, 1))()
        self._check(lib().ngz_enrich_row_fields(self._h, ctx, slot, row, out, n))
        return [(o.pen, o.ie_id, o.kind, ctypes.string_at(o.value, o.len) if o.len else b"",
                 bool(o.flags & _lib.FV_STRING)) for o in out[:n]]

    def json_lines(self, batch, renormalizer=None, host_bytes=None):
        """[(dgram, status, json, consumed)] of the enriched FlowInfos (ngz_enrich_batch_json); with a
        FlowRenormalizer that applied this batch, isRenormalized follows the writer id."""
        import numpy as np
        self._fresh(batch)
        out = []

        def cb(_user, d, status, text, n, consumed):
            out.append((int(d), int(status), ctypes.string_at(text, n).decode("utf-8"), int(consumed)))
            return 0

        fn = _lib.JSON_LINE_FN(cb)
        if host_bytes is None and isinstance(batch._source, np.ndarray):
            host_bytes = batch._source
        ptr = host_bytes.ctypes.data if host_bytes is not None else None
        self._check(lib().ngz_enrich_batch_json(self._h, renormalizer._h if renormalizer is not None else None,
                                                batch._codec._ctx, ptr, fn, None))
        return out

    def template_plan(self, peer, tmpl_bytes, proto=10, options=False):
        """ngz_enrich_template_plan (no device): {"dropped", "launches", "shapes": [[(pen, ie_id, index)]],
        "columns": [(pen, ie_id, index, kind, width)]} of one (options) template record for `peer`."""
        plan = _lib.EnrichPlan()
        p = _lib.EnrichPeer.of(peer)
        buf = (ctypes.c_uint8 * max(len(tmpl_bytes), 1)).from_buffer_copy(bytes(tmpl_bytes) or b"\0")
        self._check(lib().ngz_enrich_template_plan(self._h, ctypes.byref(p), buf, len(tmpl_bytes),
                                                   proto | (_lib.NGZ_ENRICH_OPTIONS if options else 0), ctypes.byref(plan)))
        ref = lambda r: (r.pen, r.ie_id, r.index)  # noqa: E731
        return {"dropped": bool(plan.dropped), "launches": int(plan.launches),
                "shapes": [[ref(plan.shape[s][f]) for f in range(plan.shape_len[s])] for s in range(plan.n_shapes)],
                "columns": [ref(plan.column[c]) + (plan.column_kind[c], plan.column_width[c])
                            for c in range(plan.n_columns)]}

    def forget(self, batch):
        """Drop what the enricher keeps for the batch's codec (before the codec is closed)."""
        self._check(lib().ngz_enrich_forget(self._h, batch._codec._ctx))

    def value_arena(self):
        """The bytes variable-length added columns point into (the host copy)."""
        host, size = ctypes.c_void_p(), ctypes.c_uint64()
        self._check(lib().ngz_enrich_value_arena(self._h, None, ctypes.byref(host), ctypes.byref(size)))
        return ctypes.string_at(host.value, size.value) if size.value else b""

    @property
    def last_ms(self):
        t = ctypes.c_float()
        lib().ngz_enrich_last_timing(self._h, ctypes.byref(t))
        return t.value
