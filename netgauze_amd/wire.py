"""The Encoder half of the codec: IPFIX / NetFlow v9 messages written again from the decoded columns on
the device (include/ngz/flow_wire.h).

`FlowWire()` is the stage: `encode(batch)` writes the message of every datagram of the codec's latest
DecodedBatch whose `how` is WIRE; `result()` brings messages, offsets and `how` to the host;
`messages(batch)` adds `batch.dgram_wire(d)` (ngz_dgram_wire, the specification) for the datagrams the
device leaves to the host.  The columns are read as they are: after a renormalization the messages carry
the scaled counts."""
import ctypes
import sys

import numpy as np

from netgauze_amd import _lib
from netgauze_amd._lib import load as lib
from netgauze_amd.output import OutputError


class FlowWire:
    NONE, WIRE, HOST, UNWRITABLE = _lib.NGZ_WIRE_NONE, _lib.NGZ_WIRE_WIRE, _lib.NGZ_WIRE_HOST, _lib.NGZ_WIRE_UNWRITABLE

    def __init__(self, device=0, align4=False):
        h = ctypes.c_void_p()
        rc = lib().ngz_wire_create(device, ctypes.byref(h))
        if rc != 0:
            raise OutputError("ngz_wire_create failed (%d)" % rc, rc)
        self._h = h
        self.device = device
        self.align4 = bool(align4)
        if align4:
            self.set_option(_lib.NGZ_WIRE_OPT_ALIGN4, 1)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ngz_wire_destroy(self._h)
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
            raise OutputError("%s (%d)" % (lib().ngz_wire_last_error(self._h).decode(), rc), rc)
        return rc

    def set_option(self, option, value):
        self._check(lib().ngz_wire_set_option(self._h, option, value))
        if option == _lib.NGZ_WIRE_OPT_ALIGN4:
            self.align4 = bool(value)

    def encode(self, batch, stream=None):
        """Write the messages of the codec's latest DecodedBatch; this encode's counters.  The batch's
        input must still be valid: variable-length values are read from it."""
        if batch.generation != batch._codec.generation:
            raise OutputError("stale DecodedBatch: its codec has decoded another batch since", _lib.NGZ_E_INVALID)
        st = _lib.WireStats()
        self._check(lib().ngz_wire_encode(self._h, batch._codec._ctx, ctypes.byref(batch.out), ctypes.byref(st),
                                          ctypes.c_void_p(stream) if stream else None))
        return st.as_dict()

    def result_pointers(self):
        """(device pointers of the messages, of the u64 offsets and of `how`, datagrams, bytes) of the last encode."""
        b, o, w, n, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().ngz_wire_result(self._h, ctypes.byref(b), ctypes.byref(o), ctypes.byref(w), ctypes.byref(n), ctypes.byref(nb)))
        return b.value, o.value, w.value, int(n.value), int(nb.value)

    def result(self, guard=False):
        """The last encode on the host: (messages back to back as bytes, offsets as a uint64 array of
        datagrams + 1, `how` as a uint8 array); with `guard` the guard bytes after the messages follow them."""
        _b, _o, _w, n, nb = self.result_pointers()
        data = np.empty(nb + (_lib.NGZ_OUTPUT_GUARD if guard else 0), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        how = np.zeros(n, dtype=np.uint8)
        self._check(lib().ngz_wire_to_host(self._h, data.ctypes.data, data.size, offs.ctypes.data, offs.size, how.ctypes.data, how.size))
        return data.tobytes(), offs, how

    def messages(self, batch):
        """Encode `batch` and return [(datagram, message)] of its OK datagrams: the device's bytes, and
        `batch.dgram_wire(d)` for the ones it leaves to the host (None for an unwritable one)."""
        self.encode(batch)
        data, offs, how = self.result()
        offs = offs.tolist()
        return [(d, data[offs[d]:offs[d + 1]] if h == self.WIRE else batch.dgram_wire(d, self.align4))
                for d, h in enumerate(how.tolist()) if h != self.NONE]

    def last_ms(self):
        """(size pass, offsets, glue passes, pack passes) of the last encode, device milliseconds."""
        t = [ctypes.c_float() for _ in range(4)]
        lib().ngz_wire_last_timing(self._h, *[ctypes.byref(x) for x in t])
        return tuple(x.value for x in t)

    @property
    def last_launches(self):
        return int(lib().ngz_wire_last_launches(self._h))
