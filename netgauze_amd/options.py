"""Host-side mirror of the collector's flow-options input, over the C ABI in
include/ngz/flow_options.h (libngz.so).

`FlowOptionsHarvester(device, weight)` stands for one FlowOptionsActor with its
FlowEnrichmentOptionsHandler (crates/collector/src/inputs/flow_options/actor.rs, handlers.rs).
`harvest(batch, peer)` turns the options data records of the codec's latest DecodedBatch into
upserts on the device; `ops()` returns them in stream order, `feed(enricher)` hands them to a
FlowEnricher's cache.  `template_plan` is the per-template part of normalize.rs, without a device.

A field is a tuple (pen, ie_id, kind, value bytes) as in netgauze_amd.enrich.
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


class OptionsError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def template_plan(tmpl_bytes, proto=10, options=True):
    """ngz_options_template_plan (no device) of one (options) template record: {"class", "outcome",
    "id_equal", "ops": [{"scope": [(pen, ie_id, index)], "fields": [...], "scope_src": [template field
    index], "fields_src": [...]}]}."""
    plan = _lib.OptionsPlan()
    buf = (ctypes.c_uint8 * max(len(tmpl_bytes), 1)).from_buffer_copy(bytes(tmpl_bytes) or b"\0")
    rc = lib().ngz_options_template_plan(buf, len(tmpl_bytes), proto | (_lib.NGZ_OPTIONS_OPTIONS if options else 0),
                                         ctypes.byref(plan))
    if rc != 0:
        raise OptionsError("ngz_options_template_plan failed (%d)" % rc, rc)
    ref = lambda r: (r.pen, r.ie_id, r.index)  # noqa: E731
    ops = [{"scope": [ref(plan.scope[o][i]) for i in range(plan.n_scope[o])],
            "fields": [ref(plan.fields[o][i]) for i in range(plan.n_fields[o])],
            "scope_src": [plan.scope_src[o][i] for i in range(plan.n_scope[o])],
            "fields_src": [plan.fields_src[o][i] for i in range(plan.n_fields[o])]} for o in range(plan.n_ops)]
    return {"class": _lib.OPTIONS_CLASSES[plan.klass], "outcome": _lib.OPTIONS_OUTCOMES[plan.outcome],
            "id_equal": bool(plan.id_equal), "ops": ops}


class FlowOptionsHarvester:
    def __init__(self, device=0, weight=16):
        h = ctypes.c_void_p()
        rc = lib().ngz_options_create(device, weight, ctypes.byref(h))
        if rc != 0:
            raise OptionsError("ngz_options_create(%d) failed (%d)" % (device, rc), rc)
        self._h = h
        self.device = device
        self.weight = weight

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_options_destroy(self._h)
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
            raise OptionsError("%s (%d)" % (lib().ngz_options_last_error(self._h).decode(), rc), rc)
        return rc

    template_plan = staticmethod(template_plan)

    def harvest(self, batch, peer, stream=None):
        """Harvest the codec's latest DecodedBatch for the exporter `peer` (an IP address string);
        the counters of this batch."""
        if batch.generation != batch._codec.generation:
            raise OptionsError("stale DecodedBatch: its codec has decoded another batch since", _lib.NGZ_E_INVALID)
        st = _lib.OptionsStats()
        p = _lib.EnrichPeer.of(peer)
        self._peer = peer
        self._check(lib().ngz_options_harvest(self._h, batch._codec._ctx, ctypes.byref(batch.out), ctypes.byref(p),
                                              ctypes.byref(st), ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def __len__(self):
        return int(lib().ngz_options_op_count(self._h))

    def ops(self):
        """The harvested operations in order, as the dicts tests/enrich_ref.py's Cache.apply takes:
        {"op": "upsert", "ip", "domain", "weight", "scope": [field], "fields": [field]}."""
        def fields(arr, n):
            return [(arr[i].pen, arr[i].ie_id, arr[i].kind, ctypes.string_at(arr[i].value, arr[i].len) if arr[i].len else b"")
                    for i in range(n)]

        out = []
        op = _lib.EnrichOperation()
        for i in range(len(self)):
            self._check(lib().ngz_options_op(self._h, i, ctypes.byref(op)))
            out.append({"op": "upsert", "ip": self._peer, "domain": int(op.obs_domain_id), "weight": int(op.weight),
                        "scope": fields(op.scope, op.n_scope), "fields": fields(op.fields, op.n_fields)})
        return out

    def feed(self, enricher):
        """ngz_options_feed: every operation into the FlowEnricher's cache, in order; the number it took
        (refused ones count in totals()["ops_refused"])."""
        n = ctypes.c_uint64()
        self._check(lib().ngz_options_feed(self._h, enricher._h, ctypes.byref(n)))
        return int(n.value)

    def totals(self, reset=False):
        st = _lib.OptionsStats()
        self._check(lib().ngz_options_totals(self._h, ctypes.byref(st), 1 if reset else 0))
        return st.as_dict()

    @property
    def last_launches(self):
        return int(lib().ngz_options_last_launches(self._h))

    @property
    def last_ms(self):
        t = ctypes.c_float()
        lib().ngz_options_last_timing(self._h, ctypes.byref(t))
        return t.value
