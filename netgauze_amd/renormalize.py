"""Host-side mirror of the collector's flow renormalization, over the C ABI in
include/ngz/flow_renormalize.h (libngz.so; the counts are scaled in place in HBM).

`FlowRenormalizer(device)` stands for one RenormalizationActor shard
(crates/collector/src/flow/renormalization/actor.rs) and serves every codec on its device.
`apply(batch)` is renormalize() (renormalization/logic.rs:381-524) over every FlowInfo of
the codec's latest DecodedBatch: octet / packet counts multiplied by the sampling factor of
each record, in the batch's columns, so FlowAggregator.push on the same batch sums
renormalized counts.  It returns the batch's RenormalizationStats as a dict.
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


class RenormError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def template_plan(tmpl_bytes, proto=10, options=False):
    """ngz_renorm_template_plan (no device): the plan of one (options) template record as a dict:
    param_field {IE: field index}, count_field [field index], dropped, launches."""
    plan = _lib.RenormPlan()
    buf = (ctypes.c_uint8 * max(len(tmpl_bytes), 1)).from_buffer_copy(bytes(tmpl_bytes) or b"\0")
    rc = lib().ngz_renorm_template_plan(buf, len(tmpl_bytes), proto | (_lib.NGZ_RENORM_OPTIONS if options else 0),
                                        ctypes.byref(plan))
    if rc != 0:
        raise RenormError("ngz_renorm_template_plan failed (%d)" % rc, rc)
    ies = (34, 35, 49, 50, 304, 305, 306, 309, 310, 311)
    return {"param_field": {ie: int(f) for ie, f in zip(ies, plan.param_field) if f >= 0},
            "count_field": [int(plan.count_field[i]) for i in range(plan.n_counts)],
            "dropped": bool(plan.dropped), "launches": int(plan.launches)}


class FlowRenormalizer:
    def __init__(self, device=0):
        h = ctypes.c_void_p()
        rc = lib().ngz_renorm_create(device, ctypes.byref(h))
        if rc != 0:
            raise RenormError("ngz_renorm_create(%d) failed (%d)" % (device, rc), rc)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_renorm_destroy(self._h)
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
            raise RenormError("%s (%d)" % (lib().ngz_renorm_last_error(self._h).decode(), rc), rc)
        return rc

    @staticmethod
    def _fresh(batch):
        if batch.generation != batch._codec.generation:
            raise RenormError("stale DecodedBatch: its codec has decoded another batch since", _lib.NGZ_E_INVALID)

    def apply(self, batch, stream=None):
        """Renormalize the codec's latest DecodedBatch in place; the five counters of this batch."""
        self._fresh(batch)
        st = _lib.RenormStats()
        self._check(lib().ngz_renorm_apply(self._h, batch._codec._ctx, ctypes.byref(batch.out), ctypes.byref(st),
                                           ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def apply_enriched(self, batch, enricher, stream=None):
        """apply() over enriched records: the sampling IEs `enricher` (a FlowEnricher that applied this
        batch last) resolved override the record's own (ngz_renorm_apply_enriched)."""
        self._fresh(batch)
        st = _lib.RenormStats()
        self._check(lib().ngz_renorm_apply_enriched(self._h, enricher._h, batch._codec._ctx, ctypes.byref(batch.out),
                                                    ctypes.byref(st), ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def totals(self, reset=False):
        st = _lib.RenormStats()
        self._check(lib().ngz_renorm_totals(self._h, ctypes.byref(st), 1 if reset else 0))
        return st.as_dict()

    def flags(self, slot):
        """Per row of a slot of the batch last applied: bit 0 = isRenormalized(true) was appended.
        A torch.uint8 device tensor (a copy)."""
        import torch
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        self._check(lib().ngz_renorm_flags(self._h, slot, ctypes.byref(p), ctypes.byref(n)))
        t = torch.empty(n.value, dtype=torch.uint8, device="cuda:%d" % self.device)
        if n.value:
            torch.cuda.synchronize(self.device)
            rc = _lib.hip().hipMemcpy(t.data_ptr(), p, n.value, 3)  # hipMemcpyDeviceToDevice
            if rc != 0:
                raise RenormError("hipMemcpy D2D failed: %d" % rc, _lib.NGZ_E_DEVICE)
        return t

    def json_lines(self, batch, host_bytes=None):
        """[(dgram, status, json, consumed)] of the renormalized FlowInfos (ngz_renorm_batch_json)."""
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
        self._check(lib().ngz_renorm_batch_json(self._h, batch._codec._ctx, ptr, fn, None))
        return out

    @property
    def last_ms(self):
        t = ctypes.c_float()
        lib().ngz_renorm_last_timing(self._h, ctypes.byref(t))
        return t.value

    template_plan = staticmethod(template_plan)
