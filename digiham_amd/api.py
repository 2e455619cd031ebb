"""Python front-end over the C ABI (include/digiham_amd.h).

Device memory and streams come from PyTorch-ROCm (plumbing only): inputs are
``torch`` CUDA tensors, an engine enqueues its HIP kernels on the stream that was
torch's current stream WHEN THE ENGINE WAS CREATED (inputs produced on another stream
must be ordered against it by the caller), outputs are fetched into numpy arrays on request.  All compute happens
in ``libdigiham_amd.so``; nothing here computes or falls back.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import DhError

EVENT_DTYPE = np.dtype([("sym_index", "<u4"), ("type", "u1"), ("a", "u1"), ("b", "u1"), ("len", "u1"),
                        ("payload", "u1", (24,))])

_CODES = {"hamming_7_4": np.uint8, "hamming_13_9": np.uint16, "hamming_15_11": np.uint16,
          "hamming_16_11": np.uint16, "quadratic_residue": np.uint16, "golay_20_8": np.uint32, "golay_24_12": np.uint32, "bch_31_21": np.uint32}


class TorchCudaMemory:
    """Device arrays as torch CUDA tensors."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("digiham_amd needs an MI355X (gfx950) visible to PyTorch-ROCm; there is no CPU path")
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.index = device

    _NP2T = {"uint8": "uint8", "int16": "int16", "uint16": "int16", "uint32": "int32", "int32": "int32",
             "float32": "float32", "uint64": "int64", "int64": "int64"}

    def from_numpy(self, a):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.view(getattr(np, self._NP2T[a.dtype.name])) if a.dtype.name in ("uint16", "uint32", "uint64") else a)
        return t.to(self.device)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=getattr(self.torch, self._NP2T[np.dtype(dtype).name]), device=self.device)

    def to_numpy(self, t, dtype=None):
        a = t.detach().cpu().numpy()
        return a.view(dtype) if dtype is not None else a

    def ptr(self, t):
        return C.c_void_p(t.data_ptr())

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def is_device_array(self, x):
        return self.torch.is_tensor(x) and x.is_cuda


def dmr_split_slots(frame_bytes):
    """The frames of a DMR engine with dmr_both_slots=True -- 28-byte records, 27 payload bytes and the slot -- as (slot0, slot1):
    two uint8 arrays of 27-byte payloads, each in the order of its bursts.  ValueError on a length that is no multiple of 28 or
    on a tag above 1."""
    a = np.ascontiguousarray(frame_bytes, np.uint8).ravel()
    rec = _capi.DMR_SLOT_RECORD_BYTES
    if a.size % rec:
        raise ValueError("dmr_split_slots: %d bytes are no whole number of %d-byte records" % (a.size, rec))
    a = a.reshape(-1, rec)
    tag = a[:, rec - 1]
    if (tag > 1).any():
        raise ValueError("dmr_split_slots: a record tagged %d" % int(tag[tag > 1][0]))
    return a[tag == 0, :rec - 1].ravel().copy(), a[tag == 1, :rec - 1].ravel().copy()


def parse_lc(payload):
    """Fields of a 9-byte DMR link control word (DH_EV_DMR_LC payload): what Digiham::Dmr::Lc's getters return
    (src/dmr_decoder/lc.cpp:26-43)."""
    d = bytes(bytearray(payload[:9]))
    return {"opcode": d[0] & 0x3F, "feature_set_id": d[1], "target": d[3] << 16 | d[4] << 8 | d[5],
            "source": d[6] << 16 | d[7] << 8 | d[8], "data": d[2:9]}


_CALL_SYNC = {"dmr": (None, "data", "voice", "unknown"), "nxdn": (None, "voice")}
_CALL_TYPE = {"dmr": (None, "group", "direct"), "nxdn": (None, "conference", "individual")}
_YSF_MODE = (None, "V1", "FR data", "DN", "VW")


def _ysf_string(raw):
    """ten raw bytes cut at the first blank or newline (treatYsfString, ysf_phase.cpp:351-361); nothing left: None"""
    raw = bytes(raw)
    for c in (b"\n", b" "):
        at = raw.find(c)
        if at >= 0:
            raw = raw[:at]
    return raw.decode("latin-1") if raw.strip(b"\0") else None


def parse_call(proto, event):
    """The call record an EV_CALL event carries (DH_FLAG_CALL_DIGEST; include/digiham_amd.h, "Call digest"), as a dict.
    "dmr": {"changed": (slot, ...) from the event's `a`, "slots": [per slot {"sync", "type", "source", "target"}]};
    "nxdn": {"changed": (0,), "sync", "type", "source", "destination"}; "ysf": {"changed": (0,), "mode", "target", "source"},
    the strings cut at the first blank or newline as treatYsfString does.  A field of zeros reads as None, and so does a DMR
    slot whose record is all zeros."""
    if int(event["type"]) != _capi.EV_CALL or int(event["len"]) != _capi.CALL_RECORD_BYTES[proto]:
        raise ValueError("parse_call: not a %s EV_CALL event: type %d, len %d" % (proto, int(event["type"]), int(event["len"])))
    d = bytes(bytearray(event["payload"]))
    changed = tuple(i for i in range(2) if int(event["a"]) >> i & 1)
    num = lambda b: int.from_bytes(b, "big") or None
    name = lambda table, i: table[i] if i < len(table) else "unknown"
    if proto == "dmr":
        return {"changed": changed, "slots": [{"sync": name(_CALL_SYNC["dmr"], d[8 * s]), "type": name(_CALL_TYPE["dmr"], d[8 * s + 1]),
                                               "source": num(d[8 * s + 2:8 * s + 5]), "target": num(d[8 * s + 5:8 * s + 8])}
                                              if any(d[8 * s:8 * s + 8]) else None for s in range(2)]}
    if proto == "nxdn":
        return {"changed": changed, "sync": name(_CALL_SYNC["nxdn"], d[0]), "type": name(_CALL_TYPE["nxdn"], d[1]),
                "source": num(d[2:4]), "destination": num(d[4:6])}
    return {"changed": changed, "mode": name(_YSF_MODE, d[0]), "target": _ysf_string(d[1:11]), "source": _ysf_string(d[11:21])}


def _check(rc, what, lib):
    if rc != 0:
        raise DhError(rc, what, lib.dh_last_error().decode(errors="replace"))


def _host(a):
    """The pointer the library reads or fills a host (numpy) array through, for the duration of one call."""
    return a.ctypes.data_as(C.c_void_p)


def _float_rows(mem, x, B, what):
    """(array, row stride) of float32 [B][n] rows the library can read where they are: a device array whose rows are
    contiguous -- a column slice of a wider array included, rows need no alignment -- or a copy of anything else."""
    torch = getattr(mem, "torch", None)
    if torch is not None and torch.is_tensor(x) and x.is_cuda:
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != B or (x.shape[1] > 1 and x.stride(1) != 1):
            raise ValueError("%s: need a float32 [%d][n] device array with contiguous rows, got %s %s strides %s"
                             % (what, B, x.dtype, tuple(x.shape), tuple(x.stride())))
        if x.device.index != mem.index:
            raise ValueError("%s: the array lives on cuda:%s, the handle on cuda:%s" % (what, x.device.index, mem.index))
        return x, (x.stride(0) if B > 1 else x.shape[1])
    in_place = torch is None and isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 2 and x.shape[0] == B and \
        (x.shape[1] <= 1 or x.strides[1] == 4) and (B == 1 or (x.strides[0] > 0 and x.strides[0] % 4 == 0))
    if not in_place:
        x = mem.from_numpy(np.ascontiguousarray(x, np.float32).reshape(B, -1))
    if callable(getattr(x, "stride", None)):
        return x, (x.stride(0) if B > 1 else x.shape[1])
    return x, (x.strides[0] // 4 if B > 1 else x.shape[1])


def _vector(mem, a, dtype, n, what):
    """The [n] vector of a call (counts, flags, mask, tag, from): None, a device array as it is, or an upload of anything
    else as `dtype`.  ValueError unless it has n entries (n None: any number) of dtype's size -- an int64 device array may
    hold uint64 bits."""
    if a is None:
        return None
    if not mem.is_device_array(a):
        a = mem.from_numpy(np.ascontiguousarray(a, dtype))
    size = np.dtype(dtype).itemsize
    if (n is not None and tuple(a.shape) != (n,)) or (a.element_size() if callable(getattr(a, "element_size", None)) else a.itemsize) != size:
        raise ValueError("%s needs %s %d-bit entries" % (what, "its" if n is None else n, 8 * size))
    return a


def _ptr(mem, a):
    return None if a is None else mem.ptr(a)


class Context:
    """A loaded library + a device-memory provider."""

    def __init__(self, lib=None, mem=None, device=0):
        self.lib = lib if lib is not None else _capi.load()
        self.mem = mem if mem is not None else TorchCudaMemory(device)

    def _call(self, name, *args):
        _check(getattr(self.lib, name)(*args), name, self.lib)

    # ------------------------------------------------------------------ batch FEC
    def block_decode(self, code, words):
        """words: numpy array -> (corrected words, ok flags) as numpy."""
        dt = _CODES[code]
        w = self.mem.from_numpy(np.ascontiguousarray(words, dt).ravel())
        ok = self.mem.zeros((w.shape[0],), np.uint8)
        self._call("dh_" + code, self.mem.ptr(w), self.mem.ptr(ok), w.shape[0], self.mem.stream())
        return self.mem.to_numpy(w, dt), self.mem.to_numpy(ok)

    def bptc_196_96(self, payloads):
        p = self.mem.from_numpy(np.ascontiguousarray(payloads, np.uint8).reshape(-1, 25))
        n = p.shape[0]
        out = self.mem.zeros((n, 12), np.uint8)
        ok = self.mem.zeros((n,), np.uint8)
        self._call("dh_bptc_196_96", self.mem.ptr(p), self.mem.ptr(out), self.mem.ptr(ok), n, self.mem.stream())
        return self.mem.to_numpy(out), self.mem.to_numpy(ok)

    def trellis(self, packed, n_dibits):
        p = np.ascontiguousarray(packed, np.uint8)
        n, stride = p.shape
        ob = (n_dibits + 7) // 8
        d = self.mem.from_numpy(p)
        out = self.mem.zeros((n, ob), np.uint8)
        metric = self.mem.zeros((n,), np.uint8)
        self._call("dh_trellis", self.mem.ptr(d), stride, n_dibits, self.mem.ptr(out), ob, self.mem.ptr(metric), n, self.mem.stream())
        return self.mem.to_numpy(out), self.mem.to_numpy(metric)

    def crc16(self, data, count):
        a = np.ascontiguousarray(data, np.uint8)
        n, stride = a.shape
        d = self.mem.from_numpy(a)
        out = self.mem.zeros((n,), np.uint16)
        self._call("dh_crc16", self.mem.ptr(d), stride, count, self.mem.ptr(out), n, self.mem.stream())
        return self.mem.to_numpy(out, np.uint16)

    def whitening(self, data, n_bits):
        a = np.ascontiguousarray(data, np.uint8)
        n, stride = a.shape
        d = self.mem.from_numpy(a)
        out = self.mem.zeros((n, stride), np.uint8)
        self._call("dh_whitening", self.mem.ptr(d), self.mem.ptr(out), stride, n_bits, n, self.mem.stream())
        return self.mem.to_numpy(out)

    def debug_div_gain(self, x, narrow=False):
        d = self.mem.from_numpy(np.ascontiguousarray(x, np.float32).ravel())
        out = self.mem.zeros((d.shape[0],), np.float32)
        self._call("dh_debug_div_gain", self.mem.ptr(d), self.mem.ptr(out), d.shape[0], int(narrow), self.mem.stream())
        return self.mem.to_numpy(out)

    def frontend(self, x, mode, dcblock=True, state=None):
        """The receiver front-end (dh_frontend_s16): x int16 [B][n] audio (mode "audio") or [B][2 n] interleaved I / Q ("iq").
        Returns (float32 device array [B][n] for Engine.push, state) -- pass the state back in to continue the streams."""
        a = x if self.mem.is_device_array(x) else self.mem.from_numpy(np.ascontiguousarray(x, np.int16))
        B, w = a.shape
        n = w if mode == "audio" else w // 2
        out = self.mem.zeros((B, n), np.float32)
        if state is None:
            state = self.mem.zeros((B, 4), np.float32)
        self._call("dh_frontend_s16", self.mem.ptr(a), w, self.mem.ptr(out), n, self.mem.ptr(state), B, n,
                                        1 if mode == "audio" else 2, int(bool(dcblock)), self.mem.stream())
        return out, state

    def debug_div_const(self, x, divisor):
        """x (numpy float32, or a device array) / float(divisor) as the slicer kernels compute it; returns what it was given."""
        dev = self.mem.is_device_array(x)
        d = x if dev else self.mem.from_numpy(np.ascontiguousarray(x, np.float32).ravel())
        out = self.mem.zeros((d.shape[0],), np.float32)
        self._call("dh_debug_div_const", self.mem.ptr(d), self.mem.ptr(out), d.shape[0], int(divisor), self.mem.stream())
        return out if dev else self.mem.to_numpy(out)

    def debug_mfma_f16(self, a, b, c):
        """d[t] = c[t] + a[t] @ b[t] on the matrix cores: a [T][16][32], b [T][32][16] as float16 (or uint16 bit patterns), c [T][16][16] float32."""
        a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
        a = a.view(np.uint16) if a.dtype == np.float16 else a.astype(np.uint16)
        b = b.view(np.uint16) if b.dtype == np.float16 else b.astype(np.uint16)
        T = a.shape[0]
        da, db = self.mem.from_numpy(a.reshape(T, 512)), self.mem.from_numpy(b.reshape(T, 512))
        dc = self.mem.from_numpy(np.ascontiguousarray(c, np.float32).reshape(T, 256))
        out = self.mem.zeros((T, 256), np.float32)
        self._call("dh_debug_mfma_f16", self.mem.ptr(da), self.mem.ptr(db), self.mem.ptr(dc), self.mem.ptr(out), T, self.mem.stream())
        return self.mem.to_numpy(out).reshape(T, 16, 16)

    def debug_f16_split(self, x, scale=1.0):
        """(h1, h2) as float16 arrays: the two halves the error-bounded FIR makes of x * scale."""
        d = self.mem.from_numpy(np.ascontiguousarray(x, np.float32).ravel())
        n = d.shape[0]
        h1, h2 = self.mem.zeros((n,), np.uint16), self.mem.zeros((n,), np.uint16)
        self._call("dh_debug_f16_split", self.mem.ptr(d), self.mem.ptr(h1), self.mem.ptr(h2), n, float(scale), self.mem.stream())
        return self.mem.to_numpy(h1).view(np.float16), self.mem.to_numpy(h2).view(np.float16)

    def seam_probe_words(self, op):
        """(input words, output words) per case of a seam-probe op (dh_debug_seam_probe_words)."""
        a, b = C.c_size_t(), C.c_size_t()
        self._call("dh_debug_seam_probe_words", int(op), C.byref(a), C.byref(b))
        return a.value, b.value

    def debug_seam_probe(self, op, words):
        """One primitive of the kernels' device / CPU layer run alone (dh_debug_seam_probe): words uint32 [cases][in_words(op)],
        one wavefront per case; returns uint32 [cases][out_words(op)].  Words the probe does not write come back as 0xA5A5A5A5."""
        nin, nout = self.seam_probe_words(op)
        w = np.ascontiguousarray(words, np.uint32)
        if w.ndim != 2 or w.shape[1] != nin:
            raise ValueError("Context.debug_seam_probe: op %d takes [cases][%d] words, got %s" % (op, nin, w.shape))
        d = self.mem.from_numpy(w)
        out = self.mem.from_numpy(np.full((w.shape[0], nout), 0xA5A5A5A5, np.uint32))
        self._call("dh_debug_seam_probe", int(op), self.mem.ptr(d), self.mem.ptr(out), w.shape[0], self.mem.stream())
        return self.mem.to_numpy(out, np.uint32).reshape(w.shape[0], nout)

    def dvfilter(self, x, state=None):
        """x: int16 [B][n] numpy; returns (y, state) with state a device array [B][22] to carry on."""
        a = np.ascontiguousarray(x, np.int16)
        if a.ndim == 1:
            a = a[None, :]
        B, n = a.shape
        d = self.mem.from_numpy(a)
        out = self.mem.zeros((B, n), np.int16)
        if state is None:
            state = self.mem.zeros((B, 22), np.float32)
        self._call("dh_dvfilter_s16", self.mem.ptr(d), self.mem.ptr(out), self.mem.ptr(state), B, n, n, self.mem.stream())
        return self.mem.to_numpy(out), state


class _Handle:
    """What the classes below share.  One that owns a library handle names its kind (`_kind` = "dh_x": dh_x_create and
    dh_x_destroy), opens it from its config struct with _open() and talks to it through _call(), which passes `_h`
    first; close() destroys an owned handle once and a call on a closed one is the library's DH_EINVAL.  One that is made
    of other handles (Scanner, Monitor) takes its context from _resolve(), closes its parts in close() and asks _live()
    before it works.  A half-built object -- the constructor raised -- closes like any other."""
    _kind, _h, _owned, _closed = None, None, True, False

    def _resolve(self, ctx, device):
        self.ctx = ctx if ctx is not None else Context(device=device)
        return self.ctx.mem

    def _open(self, ctx, device, cfg_type, **fields):
        """dh_x_create from cfg_type(struct_size, device, stream: the context's; the rest, or other values of these: fields)."""
        mem = self._resolve(ctx, device)
        cfg = cfg_type(**dict(dict(struct_size=C.sizeof(cfg_type), device=getattr(mem, "index", 0), stream=mem.stream()), **fields))
        h = C.c_void_p()
        self.ctx._call(self._kind + "_create", C.byref(cfg), C.byref(h))
        self._h = h

    def _call(self, name, *args):
        self.ctx._call(name, self._h, *args)

    def _live(self, what):
        if self._closed:
            raise DhError(_capi.DH_EINVAL, what, "closed")

    def close(self):
        if self._h and self._owned:
            getattr(self.ctx.lib, self._kind + "_destroy")(self._h)
        self._h, self._closed = None, True

    def __del__(self):
        self.close()


class Engine(_Handle):
    """B independent `rrc_filter | gfsk_demodulator | dmr_decoder` pipes with state resident in HBM."""
    _kind = "dh_engine"

    def __init__(self, n_channels, max_samples, rrc="wide", demod="gfsk", sps=10, proto="dmr", fast_fir=False,
                 keep_filtered=False, invert=False, events=True, slot_filter=3, ctx=None, device=0, ordered_timing=False, split_stages=False,
                 taps=None, gain=None, exact_symbols=False, exact_fir=False, overlap_pushes=False, one_launch=False, dmr_both_slots=False,
                 call_digest=False):
        """rrc = "custom" takes the caller's coefficient table: `taps` (nZeros + 1 floats, any shape) and `gain`, as
        Digiham::RrcFilter::RrcFilter(nZeros, gain, coeffs[]) does (include/rrc_filter.hpp:12).
        dmr_both_slots (proto "dmr" only): the voice of both timeslots leaves as 28-byte slot-tagged records
        (DH_FLAG_DMR_BOTH_SLOTS; dmr_split_slots takes them apart).
        call_digest (proto "dmr", "ysf" or "nxdn", with events, without overlap_pushes; anything else is the library's DH_EINVAL,
        raised as a DhError that is a ValueError too): every push ends with the k_call_digest launch, and events() are the
        digested rows -- an EV_CALL where the channel's call record changed (parse_call), the pass-through events, nothing else
        (DH_FLAG_CALL_DIGEST; include/digiham_amd.h, "Call digest")."""
        flags = (_capi.FLAG_FAST_FIR if fast_fir else 0) | (_capi.FLAG_KEEP_FILTERED if keep_filtered else 0) | \
                (_capi.FLAG_FSK_INVERT if invert else 0) | (0 if events else _capi.FLAG_NO_EVENTS) | \
                (_capi.FLAG_ORDERED_TIMING if ordered_timing else 0) | (_capi.FLAG_SPLIT_STAGES if split_stages else 0) | \
                (_capi.FLAG_EXACT_SYMBOLS if exact_symbols else 0) | (_capi.FLAG_EXACT_FIR if exact_fir else 0) | \
                (_capi.FLAG_OVERLAP_PUSHES if overlap_pushes else 0) | (_capi.FLAG_ONE_LAUNCH if one_launch else 0) | \
                (_capi.FLAG_DMR_BOTH_SLOTS if dmr_both_slots else 0) | (_capi.FLAG_CALL_DIGEST if call_digest else 0)
        custom = dict(struct_size=_capi.EngineConfig.rrc_taps.offset)     # the layout before the custom-filter fields: every library version takes it
        if rrc == "custom":
            t = np.ascontiguousarray(taps, np.float32).ravel()                # copied by dh_engine_create
            custom = dict(rrc_taps=t.ctypes.data_as(C.POINTER(C.c_float)), rrc_nzeros=len(t) - 1, rrc_gain=float(gain))
        try:
            self._open(ctx, device, _capi.EngineConfig, n_channels=n_channels, max_samples=max_samples, rrc=_capi.RRC[rrc],
                       demod=_capi.DEMOD[demod], sps=sps, proto=_capi.PROTO[proto], flags=flags, slot_filter=slot_filter, **custom)
        except DhError as e:
            if call_digest and e.code == _capi.DH_EINVAL:
                raise _capi.DhInvalid(e.code, "Engine(call_digest=True, proto=%r, events=%r, overlap_pushes=%r)" % (proto, events, overlap_pushes)) from None
            raise
        self.B, self.max_samples = n_channels, max_samples
        self.has_demod, self.has_proto = _capi.DEMOD[demod] != 0, _capi.PROTO[proto] != 0
        self.keep_filtered = (keep_filtered or rrc == "custom") and _capi.RRC[rrc] != 0
        self._keep = None
        # DH_FLAG_OVERLAP_PUSHES: the kernels of a push run on the engine's own streams, which torch's caching allocator knows
        # nothing about -- EVERY pushed buffer has to stay alive (and untouched) until the streams are joined again
        # (sync, reset or any read), not just the latest one
        self._overlap = bool(overlap_pushes)
        self._inflight = []

    @classmethod
    def _borrowed(cls, ctx, handle, n_channels, max_samples):
        """A view of an engine another handle owns (DeviceMonitor's): every call of Engine, and close() leaves it alive."""
        self = cls.__new__(cls)
        self.ctx, self._h, self._owned = ctx, C.c_void_p(handle), False
        self.B, self.max_samples = n_channels, max_samples
        self.has_demod, self.has_proto, self.keep_filtered = True, True, False
        self._keep, self._overlap, self._inflight = None, False, []
        return self

    def reset(self):
        self._call("dh_engine_reset")
        if self._inflight:
            self.sync()                          # the reset joined the streams; inputs are released once it has run

    def reset_channel(self, ch):
        self._call("dh_engine_reset_channel", ch)

    def reset_channels(self, flags):
        """reset_channel for every channel with flags[b] != 0 ([B] uint8, numpy or a device array), in one launch."""
        mem = self.ctx.mem
        f = _vector(mem, flags, np.uint8, self.B, "Engine.reset_channels: flags")
        self._keep_flags = f        # the launch is asynchronous: keep the flags alive
        self._call("dh_engine_reset_channels", mem.ptr(f))

    def set_slot_filter(self, f):
        self._call("dh_engine_set_slot_filter", f)

    def set_slot_filter_channel(self, ch, f):
        self._call("dh_engine_set_slot_filter_channel", ch, f)

    def push(self, x, n=None, counts=None):
        """x: device array float32 [B][stride] (torch CUDA tensor); processes the first n samples of every row -- or, with
        `counts` ([B] uint32), the first counts[b] <= n samples of row b (dh_engine_push_ragged)."""
        mem = self.ctx.mem
        x, stride = _float_rows(mem, x, self.B, "Engine.push")
        n = x.shape[1] if n is None else n
        self._keep = x          # the launch is asynchronous: keep the input alive
        if self._overlap:
            self._inflight.append(x)
        if counts is not None:  # ragged push: channel b brings counts[b] <= n samples
            c = _vector(mem, counts, np.uint32, self.B, "Engine.push: counts")
            self._keep = (x, c)
            if self._overlap:
                self._inflight.append(c)
            self._call("dh_engine_push_ragged", mem.ptr(x), stride, mem.ptr(c), n)
            return
        self._call("dh_engine_push", mem.ptr(x), stride, n)

    def push_host(self, x):
        a = np.ascontiguousarray(x, np.float32).reshape(self.B, -1)
        self._call("dh_engine_push_host", _host(a), a.shape[1], a.shape[1])

    def push_symbols(self, syms, counts):
        mem = self.ctx.mem
        s = syms if mem.is_device_array(syms) else mem.from_numpy(np.ascontiguousarray(syms, np.uint8).reshape(self.B, -1))
        c = _vector(mem, counts, np.uint32, self.B, "Engine.push_symbols: counts")
        self._keep = (s, c)
        self._call("dh_engine_push_symbols", mem.ptr(s), s.shape[1], mem.ptr(c))

    def timing_enable(self, max_pushes):
        self._call("dh_engine_timing_enable", max_pushes)
        self._timing_cap = max_pushes

    def timing_read(self):
        """(rrc_ms, slicer_ms, decoder_ms) arrays, one entry per push since the last read (HIP events)."""
        cap = getattr(self, "_timing_cap", 0)
        a, b, c = (np.zeros(max(cap, 1), np.float32) for _ in range(3))
        n = C.c_uint32(cap)
        self._call("dh_engine_timing_read", _host(a), _host(b),
                                                  _host(c), C.byref(n))
        return a[:n.value], b[:n.value], c[:n.value]

    def timing_read_split(self):
        """(first_ms, first_channels) per push since the last timing_read: duration and channel count of the first of the
        two launches of a push of a large engine with overlap_pushes (zeros otherwise).  Call before timing_read()."""
        cap = getattr(self, "_timing_cap", 0)
        a, c = np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.uint32)
        n = C.c_uint32(cap)
        self._call("dh_engine_timing_read_split", _host(a), _host(c), C.byref(n))
        return a[:n.value], c[:n.value]

    def timing_stats(self):
        """(blocks, ordered) per channel: 100-symbol timing blocks evaluated, and those decided by the in-order chain."""
        blocks, ordered = np.zeros(self.B, np.uint32), np.zeros(self.B, np.uint32)
        self._call("dh_engine_timing_stats", _host(blocks), _host(ordered))
        return blocks, ordered

    def dmr_pass_b_stats(self):
        """(lanes, scalar) per channel: chunks of the DMR decoder whose slot / superframe bookkeeping (pass B) ran one burst per
        lane, and chunks that took the burst-serial pass (irregular traffic, the chunk behind a sync search, or
        DH_DMR_SCALAR_PASS_B=1 when the engine was created), since the channel's last reset."""
        return self.debug_header(100 + 30), self.debug_header(100 + 31)

    def debug_header(self, word):
        out = np.zeros(self.B, np.uint32)
        self._call("dh_engine_debug_header", word, _host(out))
        return out

    def sync(self):
        try:
            self._call("dh_engine_sync")
        finally:
            del self._inflight[:-1]              # everything queued has run (the latest stays in _keep as before)

    _ROWS = {"symbols": np.dtype(np.uint8), "frames": np.dtype(np.uint8), "events": EVENT_DTYPE, "filtered": np.dtype(np.float32)}

    def _view(self, what):
        """(device pointer, row stride in elements, device pointer of the counts -- null for "filtered") of one output."""
        p, stride, cnt = C.c_void_p(), C.c_size_t(), C.c_void_p()
        self._call("dh_engine_" + what, C.byref(p), C.byref(stride), *([] if what == "filtered" else [C.byref(cnt)]))
        return p, stride.value, cnt

    def _read_counts(self, cnt):
        counts = np.empty(self.B, np.uint32)
        self.ctx._call("dh_copy_to_host", _host(counts), cnt, counts.nbytes)
        return counts

    def _fetch(self, what):
        p, stride, cnt = self._view(what)
        self.sync()
        rows = np.empty((self.B, stride), self._ROWS[what])
        self.ctx._call("dh_copy_to_host", _host(rows), p, rows.nbytes)
        return rows, (self._read_counts(cnt) if cnt else None)

    def symbols(self):
        """(dibits [B][stride] uint8, counts [B]) of the last push."""
        return self._fetch("symbols")

    def frames(self):
        return self._fetch("frames")

    def events(self):
        return self._fetch("events")

    def filtered(self):
        return self._fetch("filtered")[0]

    def read_rows(self, what, channels):
        """The current push's rows of the given channels only: what = "symbols" | "frames" | "events" -> (rows [len(channels)][stride],
        counts [len(channels)]); "filtered" -> (rows, None).  For looking at a few channels of a large engine (bench.py checks the
        engine it has just timed) without copying every row to the host."""
        p, stride, cnt = self._view(what)
        self.sync()
        channels = [int(c) for c in channels]
        rows = np.empty((len(channels), stride), self._ROWS[what])
        row_bytes = stride * rows.itemsize
        for j, b in enumerate(channels):
            if not 0 <= b < self.B:
                raise ValueError("Engine.read_rows: channel %d of %d" % (b, self.B))
            self.ctx._call("dh_copy_to_host", _host(rows[j]), C.c_void_p(p.value + b * row_bytes), row_bytes)
        return rows, (self._read_counts(cnt)[channels] if cnt else None)

    def device_views(self):
        """Raw device pointers of the output buffers (for zero-copy consumers)."""
        out = {}
        for name in ("symbols", "frames", "events"):
            try:
                p, stride, cnt = self._view(name)
                out[name] = (p.value, stride, cnt.value)
            except DhError:             # the engine has no such output
                pass
        return out


SCAN_STAT_DTYPE = np.dtype(_capi.SCAN_STAT_DTYPE)
SCAN_PATTERNS = _capi.SCAN_PATTERNS
# the four demodulator front ends the five protocols are received through (Engine arguments)
SCAN_FRONTS = {"wide10": dict(rrc="wide", demod="gfsk", sps=10, invert=False),        # DMR, YSF
               "narrow20": dict(rrc="narrow", demod="gfsk", sps=20, invert=False),    # NXDN48
               "fsk10": dict(rrc="none", demod="fsk", sps=10, invert=False),          # D-Star
               "fsk40i": dict(rrc="none", demod="fsk", sps=40, invert=True)}          # POCSAG 1200
# the front end each pattern is read from, and the families classify() chooses between, in its order of preference
SCAN_SOURCE = ("wide10",) * 5 + ("narrow20", "fsk10", "fsk10", "fsk40i")
SCAN_FAMILIES = (("dmr", (0, 1, 2, 3)), ("ysf", (4,)), ("nxdn", (5,)), ("dstar", (6, 7)), ("pocsag", (8,)))
# the front end a protocol's decoder sits behind: the one its sync patterns are read from
PROTO_FRONT = {"dmr": "wide10", "ysf": "wide10", "nxdn": "narrow20", "dstar": "fsk10", "pocsag": "fsk40i"}


class Scanner(_Handle):
    """Which protocol does each channel carry?  One protocol-scan engine (proto="scan", include/digiham_amd.h "Protocol
    scan") per front end in `fronts`, all fed the same rows: what Channelizer.push returns, with its squelch-gated
    `counts`, or any float32 [B][n] device array Engine.push takes.  Every engine counts, per channel, the hits of all nine
    sync patterns and how many of them came one frame period behind an earlier hit of the same family.

    stats() is a [B][9] array of SCAN_STAT_DTYPE (hits, periodic, last_sym, best_dist), each pattern read from the front
    end that can receive it (SCAN_SOURCE); classify() names the family with the most periodic hits.

    Why a single hit is not enough: a test passes on random symbols with probability sum_k C(n, k) / 2^n over the
    distances k it accepts.  For NXDN (10 dibits = 20 bits, <= 2 errors) that is 211 / 2^20, about once in 5 000 positions
    or once every two seconds of noise at 2 400 symbols per second; for DMR (48 bits, <= 3) it is about once in 10^10.
    Two hits exactly one frame apart are what a transmission produces and noise does not: with a hit every 5 000
    positions, a given period is met by chance once in 5 000 hits.  Requiring the period is what makes NXDN usable."""

    def __init__(self, n_channels, max_samples, fronts=("wide10", "narrow20", "fsk10", "fsk40i"), ctx=None, device=0):
        self._resolve(ctx, device)
        self.B, self.max_samples = n_channels, max_samples
        self.fronts = tuple(fronts)
        self.engines = {}
        for f in self.fronts:
            self.engines[f] = Engine(n_channels, max_samples, proto="scan", ctx=self.ctx, **SCAN_FRONTS[f])

    def close(self):
        for e in getattr(self, "engines", {}).values():
            e.close()
        self.engines = {}
        super().close()

    def reset(self):
        self._live("Scanner.reset")
        for e in self.engines.values():
            e.reset()

    def reset_channel(self, ch):
        self._live("Scanner.reset_channel")
        for e in self.engines.values():
            e.reset_channel(ch)

    def push(self, x, n=None, counts=None):
        """The same rows into every front end (Engine.push: float32 [B][stride], the first n samples, or counts[b] <= n)."""
        self._live("Scanner.push")
        x, _ = _float_rows(self.ctx.mem, x, self.B, "Scanner.push")
        counts = _vector(self.ctx.mem, counts, np.uint32, self.B, "Scanner.push: counts")
        for e in self.engines.values():
            e.push(x, n=n, counts=counts)

    def front_stats(self, front):
        """[B][9] SCAN_STAT_DTYPE of one front end, all nine patterns (a channel that has not been pushed since its
        reset: no hits, best_dist 255)."""
        rows, counts = self.engines[front].frames()
        out = np.zeros((self.B, len(SCAN_PATTERNS)), SCAN_STAT_DTYPE)
        out["best_dist"] = 255
        have = counts >= out.itemsize * len(SCAN_PATTERNS)
        got = np.ascontiguousarray(rows[:, :out.itemsize * len(SCAN_PATTERNS)]).view(SCAN_STAT_DTYPE)
        out[have] = got[have]
        return out

    def stats(self):
        out = np.zeros((self.B, len(SCAN_PATTERNS)), SCAN_STAT_DTYPE)
        out["best_dist"] = 255
        for f in self.fronts:
            ids = [i for i, src in enumerate(SCAN_SOURCE) if src == f]
            if ids:
                out[:, ids] = self.front_stats(f)[:, ids]
        return out

    def hits(self, channel):
        """The DH_EV_SCAN_HIT events of the last push of one channel (EVENT_DTYPE: sym_index, a = pattern, b = distance),
        each pattern from its own front end, ordered by position, then pattern.  A position counts the symbols of the
        pattern's front end since create or reset."""
        parts = []
        for f in self.fronts:
            ids = [i for i, src in enumerate(SCAN_SOURCE) if src == f]
            rows, counts = self.engines[f].read_rows("events", [channel])
            ev = rows[0, :counts[0]]
            parts.append(ev[np.isin(ev["a"], ids)])
        ev = np.concatenate(parts) if parts else np.zeros(0, EVENT_DTYPE)
        return ev[np.lexsort((ev["a"], ev["sym_index"]))]

    def classify(self, confirm=2):
        """Per channel None or "dmr" / "ysf" / "nxdn" / "dstar" / "pocsag": the family whose patterns have the most periodic
        hits, at least `confirm` of them; the first in that order where two are level."""
        periodic = self.stats()["periodic"].astype(np.int64)
        sums = np.stack([periodic[:, list(ids)].sum(axis=1) for _, ids in SCAN_FAMILIES], axis=1)
        best = sums.argmax(axis=1)                       # (the first of equal sums)
        return [SCAN_FAMILIES[k][0] if sums[b, k] >= confirm else None for b, k in enumerate(best)]


PREROLL_NONE = _capi.PREROLL_NONE


class Preroll(_Handle):
    """Every channel's last `depth` samples in a ring on the device (dh_preroll; include/digiham_amd.h "Pre-roll"), and
    for every channel the stream index at which its current run of open pushes began.

    append(rows, n, counts) takes what Channelizer.push returns and cz.counts; gather(from_, skip, max_n) hands back,
    per channel, the samples from max(from_[b], oldest) + skip on as (rows, counts, start): rows and counts are device
    arrays, exactly what Engine.push(rows, n=max_n, counts=counts) takes.  The counts array is the handle's own and is
    rewritten by the next gather.  The ring takes n_channels x depth x 4 bytes."""
    _kind = "dh_preroll"

    def __init__(self, n_channels, depth, ctx=None, device=0):
        self.B, self.depth = int(n_channels), int(depth)
        self._open(ctx, device, _capi.PrerollConfig, n_channels=self.B, depth=self.depth)
        self._counts = self.ctx.mem.zeros((self.B,), np.uint32)
        self._keep = None

    def reset(self):
        self._call("dh_preroll_reset")

    def append(self, rows, n=None, counts=None):
        """rows: float32 [B][stride]; the first n samples of every row (default: all).  counts: [B] uint32, non-zero = the
        channel's gate was open in this push; None = every channel is open."""
        mem = self.ctx.mem
        x, stride = _float_rows(mem, rows, self.B, "Preroll.append")
        n = x.shape[1] if n is None else int(n)
        c = _vector(mem, counts, np.uint32, self.B, "Preroll.append: counts")
        self._keep = (x, c)         # the launch is asynchronous: keep the inputs alive
        self._call("dh_preroll_append", mem.ptr(x), stride, n, _ptr(mem, c))

    @property
    def total(self):
        t = C.c_uint64(0)
        self._call("dh_preroll_total", C.byref(t))
        return t.value

    def open_at(self):
        """[B] uint64: PREROLL_NONE for a channel whose gate was closed in the last push.  Synchronises."""
        out = np.empty(self.B, np.uint64)
        self._call("dh_preroll_open_at", _host(out))
        return out

    def gather(self, from_, skip, max_n, out=None):
        """from_: [B] stream indices, PREROLL_NONE for channels that are not wanted.  Returns (rows [B][>= max_n] device
        float32 -- `out` if given --, counts [B] device uint32, start [B] numpy uint64)."""
        mem = self.ctx.mem
        f = np.ascontiguousarray(from_, np.uint64)
        if f.shape != (self.B,):
            raise ValueError("Preroll.gather: from_ needs %d entries" % self.B)
        max_n = int(max_n)
        if out is None:
            out = mem.zeros((self.B, max(max_n, 1)), np.float32)
        rows, stride = _float_rows(mem, out, self.B, "Preroll.gather")
        if rows is not out:
            raise ValueError("Preroll.gather: out must be a float32 [%d][n] device array with contiguous rows" % self.B)
        start = np.empty(self.B, np.uint64)
        self._call("dh_preroll_gather", _host(f), int(skip), max_n, mem.ptr(rows), stride,
                                              mem.ptr(self._counts), _host(start))
        return rows, self._counts, start

    def gather_device(self, from_dev, skip, max_n, out=None):
        """gather with `from_dev` ([B] uint64, or int64 holding the same bits) on the device already: no upload, no start.
        Returns (rows, counts)."""
        mem = self.ctx.mem
        f = _vector(mem, from_dev, np.uint64, self.B, "Preroll.gather_device: from_dev")
        max_n = int(max_n)
        if out is None:
            out = mem.zeros((self.B, max(max_n, 1)), np.float32)
        rows, stride = _float_rows(mem, out, self.B, "Preroll.gather_device")
        if rows is not out:
            raise ValueError("Preroll.gather_device: out must be a float32 [%d][n] device array with contiguous rows" % self.B)
        self._keep = (f, rows)
        self._call("dh_preroll_gather_device", mem.ptr(f), int(skip), max_n, mem.ptr(rows), stride, mem.ptr(self._counts))
        return rows, self._counts


def _row_blocks(eng, name, channels, first_sample, blocks):
    """The monitors' blocks of one engine push, read from the engine's rows: one per channel of `channels` (first_sample
    [len(channels)]) that has frames or events."""
    if 16 * len(channels) >= eng.B:                      # many rows: two whole arrays cost less than a copy per row (~17 us each on an MI355X)
        (frames, fc), (events, ec) = eng.frames(), eng.events()
        frames, fc, events, ec = frames[channels], fc[channels], events[channels], ec[channels]
    else:
        frames, fc = eng.read_rows("frames", channels)
        events, ec = eng.read_rows("events", channels)
    for j, b in enumerate(channels):
        if fc[j] or ec[j]:
            blocks.append({"channel": int(b), "proto": name, "first_sample": int(first_sample[j]),
                           "frames": frames[j, :fc[j]].copy(), "events": events[j, :ec[j]].copy()})


def _packed_blocks(entries, events, frames, user_key, tag_key, names=None):
    """One dict per entry of a pack that was read: "channel", the entry's user word under user_key (names: the name of its
    low byte instead), its tag under tag_key, and its "frames" and "events"."""
    return [{"channel": b, user_key: user if names is None else names[user & 255], tag_key: tag,
             "frames": frames[16 * off:16 * off + fc], "events": events[ei:ei + ec]} for b, user, tag, fc, ec, off, ei in entries.tolist()]


def _by_position(blocks):
    blocks.sort(key=lambda blk: (blk["channel"], blk["first_sample"]))
    return blocks


# naming on close (Monitor, DeviceMonitor: on_close="default"): per family (hits, dist) -- the hits a closing channel
# needs and the largest best distance accepted; hits = 0: the family is never named on close
CLOSE_DEFAULT = {"dmr": (1, 1), "ysf": (1, 1), "nxdn": (0, 0), "dstar": (2, 1), "pocsag": (1, 1)}


def _close_rule(on_close):
    """on_close as (close_hits[5], close_dist[5]) in the order of SCAN_FAMILIES; None: all zeros, the mode is off"""
    rule = {} if on_close is None else CLOSE_DEFAULT if isinstance(on_close, str) and on_close == "default" else on_close
    if not isinstance(rule, dict) or set(rule) - {name for name, _ in SCAN_FAMILIES}:
        raise ValueError("on_close: None, \"default\" or {family: (hits, dist)} over %s" % ", ".join(name for name, _ in SCAN_FAMILIES))
    pairs = [tuple(int(v) for v in rule.get(name, (0, 0))) for name, _ in SCAN_FAMILIES]
    if any(len(p) != 2 or not 0 <= p[0] <= 0xFFFFFFFF or not 0 <= p[1] <= 0xFFFFFFFF for p in pairs):
        raise ValueError("on_close: (hits, dist) are two unsigned 32-bit numbers per family")
    return [p[0] for p in pairs], [p[1] for p in pairs]


class Monitor(_Handle):
    """A band monitor over the rows of a channelizer: one Scanner names the protocol an open channel carries, one Preroll
    keeps every channel's recent past, and one Engine per protocol in `protos` (behind the front end of PROTO_FRONT)
    decodes a named channel FROM WHERE ITS SQUELCH OPENED -- `lead` samples earlier, as far as the ring reaches -- not from
    where the scanner made up its mind.  The monitor does not own the channelizer:

        blocks = mon.push(*cz.push(iq), counts=cz.counts)

    is the whole receiver.  `counts` is read as a flag per channel (non-zero: open, and the channel brings all n samples);
    None means every channel is open.  One round:

      1. n == 0 returns [].
      2. The ring appends the rows; a channel is closed in this round when its open_at is PREROLL_NONE.
      3. An unassigned channel that closed in this round has its scanner state reset -- with `on_close`, after its
         evidence was judged once more (below); an assigned channel closed for `release` rounds in a row becomes
         unassigned.
      4. The scanner sees the open, unassigned channels only; names = classify(confirm).
      5. An open, unassigned channel with a name is assigned: start = max(open_at - lead, total - depth, 0), the channel
         is reset in its engine and in the scanner, and the ring is replayed from start into the engine in chunks of
         max_samples.  The ring already holds this round's samples, so the channel gets no live push in this round.
      6. Every engine gets one ragged push of the rows for the channels assigned before this round and open now.
      7. The outputs come back as blocks ordered by channel, then by stream position: dicts with `channel`, `proto`,
         `first_sample` (stream index of the block's first input sample), `frames` (uint8) and `events` (EVENT_DTYPE).
         A push that produced neither frames nor events for a channel makes no block.  (Read with Engine.read_rows;
         from a sixteenth of the channels on, with frames() / events() whole.)

    `assigned[b]` is None or the protocol's name, `start[b]` the stream index where the decoder's input began.

    dmr_both_slots=True: the DMR engine is created with it, and the `frames` of a "dmr" block are 28-byte slot-tagged
    records (dmr_split_slots) -- both calls of a two-slot channel instead of the one that holds the decoder's output.

    call_digest=True: the DMR, YSF and NXDN engines are created with it; the `events` of their blocks are the digested rows
    (Engine; parse_call reads an EV_CALL).

    on_close=None | "default" (CLOSE_DEFAULT) | {family: (hits, dist)}: naming on close.  In the round in which an
    unassigned channel closes, before its scanner state is reset, H = the sum of `hits` and D = the smallest `best_dist`
    over each family's patterns are read from scanner.stats().  A family with hits != 0, H >= hits and D <= dist is
    eligible; the eligible family with the largest H wins, the first in the order of SCAN_FAMILIES where two are level.
    If its protocol is in `protos` the channel is assigned as in step 5, with open_at that of its last open round; the
    replay runs to the end of this round, whose samples flush the decoder's look-ahead.  Otherwise it stays unassigned
    (the next-best family is not considered).  A channel named on close is closed: it gets no live push, is released by
    the ordinary rule after `release` closed rounds, and continues live in the same engine if its gate opens before.

    Without on_close, a transmission that ends before the scanner has confirmed it is never decoded -- a single POCSAG
    batch, a D-Star transmission shorter than three sync periods.  With it, what is lost is a transmission whose
    evidence stays below its family's thresholds; under CLOSE_DEFAULT, NXDN is never named on close."""

    def __init__(self, n_channels, max_samples, depth=96000, lead=480, confirm=2, release=4,
                 protos=("dmr", "ysf", "nxdn", "dstar", "pocsag"), ctx=None, device=0, dmr_both_slots=False, on_close=None,
                 call_digest=False):
        self._resolve(ctx, device)
        self.B, self.max_samples, self.depth = int(n_channels), int(max_samples), int(depth)
        self.lead, self.confirm, self.release = int(lead), int(confirm), int(release)
        self.close_hits, self.close_dist = _close_rule(on_close)
        self.protos = tuple(protos)
        self.engines = {}
        self.scanner = Scanner(self.B, self.max_samples, fronts=tuple(dict.fromkeys(PROTO_FRONT[p] for p in self.protos)), ctx=self.ctx)
        self.pre = Preroll(self.B, self.depth, ctx=self.ctx)
        self.stage = self.ctx.mem.zeros((self.B, self.max_samples), np.float32)
        for p in self.protos:
            self.engines[p] = Engine(self.B, self.max_samples, proto=p, ctx=self.ctx, dmr_both_slots=bool(dmr_both_slots) and p == "dmr",
                                     call_digest=bool(call_digest) and p in _capi.CALL_RECORD_BYTES, **SCAN_FRONTS[PROTO_FRONT[p]])
        self._clear()

    def _clear(self):
        self.assigned = [None] * self.B
        self.start = [None] * self.B
        self.closed_run = np.zeros(self.B, np.int64)
        self.opened = np.full(self.B, PREROLL_NONE, np.uint64)

    def _name_on_close(self, st):
        """the family a closing channel with the statistics st [9] is named as, or None"""
        best, most = None, 0
        for k, (name, ids) in enumerate(SCAN_FAMILIES):
            H, D = int(st["hits"][list(ids)].astype(np.int64).sum()), int(st["best_dist"][list(ids)].min())
            if self.close_hits[k] != 0 and H >= self.close_hits[k] and D <= self.close_dist[k] and (best is None or H > most):
                best, most = name, H
        return best

    def close(self):
        for e in getattr(self, "engines", {}).values():
            e.close()
        self.engines = {}
        for h in ("scanner", "pre"):
            if getattr(self, h, None) is not None:
                getattr(self, h).close()
                setattr(self, h, None)
        super().close()

    def reset(self):
        self._live("Monitor.reset")
        self.scanner.reset()
        self.pre.reset()
        for e in self.engines.values():
            e.reset()
        self._clear()

    def push(self, rows, n=None, counts=None):
        self._live("Monitor.push")
        mem = self.ctx.mem
        x, _ = _float_rows(mem, rows, self.B, "Monitor.push")
        n = x.shape[1] if n is None else int(n)
        if n == 0:
            return []
        if n > self.max_samples:
            raise DhError(_capi.DH_EINVAL, "Monitor.push", "n = %d > max_samples = %d" % (n, self.max_samples))
        counts = _vector(mem, counts, np.uint32, self.B, "Monitor.push: counts")
        self.pre.append(x, n, counts)
        open_at, total = self.pre.open_at(), self.pre.total
        is_open = open_at != np.uint64(PREROLL_NONE)
        self.closed_run = np.where(is_open, 0, self.closed_run + 1)
        self.opened[is_open] = open_at[is_open]
        closing = []
        for b in np.flatnonzero(~is_open):
            if self.assigned[b] is None:
                if self.closed_run[b] == 1:
                    closing.append(int(b))
            elif self.closed_run[b] >= self.release:
                self.assigned[b], self.start[b] = None, None
        before = list(self.assigned)
        new, since = {}, {}
        if closing and any(self.close_hits):             # naming on close: the evidence, before the reset forgets it
            stats = self.scanner.stats()
            for b in closing:
                name = self._name_on_close(stats[b])
                if name in self.engines:
                    new.setdefault(name, []).append(b)
                    since[b] = int(self.opened[b])
        for b in closing:
            self.scanner.reset_channel(b)
        scan = np.array([n if is_open[b] and before[b] is None else 0 for b in range(self.B)], np.uint32)
        if scan.any():                                   # (a push of all-zero counts would change nothing)
            self.scanner.push(x, n=n, counts=scan)
            names = self.scanner.classify(self.confirm)
            for b in np.flatnonzero(scan):
                if names[b] in self.engines:
                    new.setdefault(names[b], []).append(int(b))
                    since[int(b)] = int(open_at[b])
        blocks = []
        for name, chans in new.items():
            eng = self.engines[name]
            from_ = np.full(self.B, PREROLL_NONE, np.uint64)
            for b in chans:
                self.start[b] = max(since[b] - self.lead, total - self.depth, 0)
                self.assigned[b] = name
                eng.reset_channel(b)
                self.scanner.reset_channel(b)
                from_[b] = self.start[b]
            first = np.array([self.start[b] for b in chans], np.int64)
            for skip in range(0, total - int(first.min()), self.max_samples):
                stage, cnt, _ = self.pre.gather(from_, skip, self.max_samples, out=self.stage)
                eng.push(stage, n=self.max_samples, counts=cnt)
                _row_blocks(eng, name, chans, first + skip, blocks)
        for name, eng in self.engines.items():
            chans = [b for b in range(self.B) if before[b] == name and is_open[b]]
            if chans:
                live = np.zeros(self.B, np.uint32)
                live[chans] = n
                eng.push(x, n=n, counts=live)
                _row_blocks(eng, name, chans, np.full(len(chans), total - n, np.int64), blocks)
        return _by_position(blocks)


PROTO_NAMES = {_capi.PROTO[name]: name for name in ("dmr", "ysf", "nxdn", "pocsag", "dstar")}

OUTPACK_ENTRY_DTYPE = np.dtype(_capi.OUTPACK_ENTRY_DTYPE)


class OutPack(_Handle):
    """What the pushes of a round produced, compacted on the device (dh_outpack; include/digiham_amd.h "Packed read-out").

    append(engine, ...) is asynchronous on the engine's stream and may follow any number of pushes of any engines that
    share the pack's stream; read() synchronises once and copies what was kept: (header, entries, events, frames) with
    header a dict of the dh_outpack_header fields, entries an OUTPACK_ENTRY_DTYPE array, events an EVENT_DTYPE array and
    frames uint8.  Entry i owns frames[16 * frame_offset16:][:n_frame_bytes] and events[event_index:][:n_events].  A pack
    that had to drop something says so in header["dropped"] (and `rc` is DH_ECAPACITY); what was kept is delivered."""
    _kind = "dh_outpack"

    def __init__(self, max_entries, max_events, max_frame_bytes, ctx=None, device=0):
        self.max_entries, self.max_events, self.max_frame_bytes = int(max_entries), int(max_events), int(max_frame_bytes)
        self._open(ctx, device, _capi.OutpackConfig, max_entries=self.max_entries, max_events=self.max_events,
                   max_frame_bytes=self.max_frame_bytes)
        # dh_outpack_read takes arrays of the create capacities; only what a read fills is ever touched
        self._entries = np.empty(self.max_entries, OUTPACK_ENTRY_DTYPE)
        self._events = np.empty(self.max_events, EVENT_DTYPE)
        self._frames = np.empty(self.max_frame_bytes, np.uint8)
        self._keep, self.rc = [], 0

    def clear(self):
        self._call("dh_outpack_clear")

    def append(self, engine, mask=None, tag=None, tag_add=0, user=0):
        """mask: [B] uint32 (non-zero: the channel takes part) or None; tag: [B] uint64 or None; numpy or device arrays."""
        mem = self.ctx.mem
        B = getattr(engine, "B", None)          # (None: a bare dh_engine handle, whose channel count only the caller knows)
        m, t = _vector(mem, mask, np.uint32, B, "OutPack.append: mask"), _vector(mem, tag, np.uint64, B, "OutPack.append: tag")
        self._keep.append((m, t))       # the launches are asynchronous: keep the arrays alive until the next read
        self._call("dh_outpack_append", getattr(engine, "_h", engine), _ptr(mem, m), _ptr(mem, t), int(tag_add) & 0xFFFFFFFFFFFFFFFF, int(user))

    def read(self):
        lib, hdr = self.ctx.lib, _capi.OutpackHeader()
        self.rc = lib.dh_outpack_read(self._h, C.byref(hdr), _host(self._entries), _host(self._events), _host(self._frames))
        self._keep = []
        if self.rc != _capi.DH_ECAPACITY:
            _check(self.rc, "dh_outpack_read", lib)
        header = {k: int(getattr(hdr, k)) for k in ("n_entries", "n_events", "frame_bytes", "dropped", "appends")}
        return (header, self._entries[:hdr.n_entries].copy(), self._events[:hdr.n_events].copy(), self._frames[:hdr.frame_bytes].copy())

    def blocks(self):
        """read(), as a list of {"channel", "user", "tag", "frames", "events"} in the pack's order."""
        return _packed_blocks(*self.read()[1:], "user", "tag")


class DeviceMonitor(_Handle):
    """Monitor behind the C ABI (dh_monitor; include/digiham_amd.h "Band monitor"): the same constructor arguments, the same
    rounds, the same blocks from push() -- but the scan engines, the ring, the protocol engines and the staging array
    belong to one library handle, and the per-round bookkeeping runs in kernels: the host reads one fixed-size summary per
    step instead of every channel's open_at, resets channels with one masked launch per engine, and uploads nothing per
    channel.  Blocks are built in the handle's sink, after every engine push, from one download of that push's counts and
    starts and the engine's frames() / events() (read_rows for fewer than a sixteenth of the channels), as Monitor does.

    `assigned` and `start` are read from the device when asked for (once per round at most); `engines` and
    `scanner.engines` are views of the handle's engines and die with it.

    dmr_both_slots=True: as for Monitor (dh_monitor_config.dmr_both_slots); "dmr" blocks carry 28-byte slot-tagged records.

    on_close: as for Monitor (dh_monitor_config.close_hits, close_dist; step C of a round, one more kernel).

    packed=True: the monitor owns an OutPack sized so that a round can never drop, and push() is clear,
    dh_monitor_push_packed, one read: no sink, no read-back per engine push, copies sized by what was decoded."""
    _kind = "dh_monitor"

    def __init__(self, n_channels, max_samples, depth=96000, lead=480, confirm=2, release=4,
                 protos=("dmr", "ysf", "nxdn", "dstar", "pocsag"), ctx=None, device=0, packed=False, dmr_both_slots=False, on_close=None):
        self.B, self.max_samples, self.depth = int(n_channels), int(max_samples), int(depth)
        self.lead, self.confirm, self.release = int(lead), int(confirm), int(release)
        self.protos = tuple(protos)
        self.close_hits, self.close_dist = _close_rule(on_close)
        bits = 0
        for p in self.protos:
            bits |= 1 << _capi.PROTO[p]
        self._open(ctx, device, _capi.MonitorConfig, n_channels=self.B, max_samples=self.max_samples, depth=self.depth, lead=self.lead,
                   confirm=self.confirm, release=self.release, protos=bits, dmr_both_slots=int(bool(dmr_both_slots)),
                   close_hits=(C.c_uint32 * 5)(*self.close_hits), close_dist=(C.c_uint32 * 5)(*self.close_dist))
        lib, h = self.ctx.lib, self._h
        self.engines = {p: Engine._borrowed(self.ctx, lib.dh_monitor_engine(h, _capi.PROTO[p]), self.B, self.max_samples) for p in self.protos}
        self.scanner = Scanner.__new__(Scanner)
        self.scanner.ctx, self.scanner.B, self.scanner.max_samples = self.ctx, self.B, self.max_samples
        self.scanner.engines = {}
        for i, f in enumerate(_capi.MONITOR_FRONTS):
            e = lib.dh_monitor_scan_engine(h, i)
            if e:
                self.scanner.engines[f] = Engine._borrowed(self.ctx, e, self.B, self.max_samples)
        self.scanner.fronts = tuple(self.scanner.engines)
        self.scanner_engines = self.scanner.engines
        self._sink = _capi.MONITOR_SINK(self._on_push)
        self._blocks, self._error, self._state, self._keep = None, None, None, None
        self.pack = None
        if packed:
            # per protocol: the engine's row capacities x B x the chunks of the longest replay (a channel is replayed or
            # live in a round, never both)
            chunks = max(1, -(-self.depth // self.max_samples))
            n_ev = n_fb = 0
            for e in self.engines.values():
                n_fb += e._view("frames")[1] * self.B * chunks
                n_ev += e._view("events")[1] * self.B * chunks
            self.pack = OutPack(min(len(self.engines) * self.B * chunks, 0xFFFFFFFF), min(n_ev, 0xFFFFFFFF), min(n_fb, (1 << 36) - 16), ctx=self.ctx)

    def close(self):
        if getattr(self, "pack", None) is not None:
            self.pack.close()
            self.pack = None
        if self._h:
            for e in list(self.engines.values()) + list(self.scanner.engines.values()):
                e.close()
            self.engines, self.scanner.engines = {}, {}
        super().close()

    def reset(self):
        self._call("dh_monitor_reset")
        self._state = None

    @property
    def total(self):
        t = C.c_uint64(0)
        self._call("dh_monitor_total", C.byref(t))
        return t.value

    def _read_state(self):
        if self._state is None:
            a, s = np.empty(self.B, np.uint8), np.empty(self.B, np.uint64)
            self._call("dh_monitor_state", _host(a), _host(s))
            self._state = ([PROTO_NAMES.get(int(v)) for v in a], [None if int(v) == PREROLL_NONE else int(v) for v in s])
        return self._state

    @property
    def assigned(self):
        return self._read_state()[0]

    @property
    def start(self):
        return self._read_state()[1]

    def _on_push(self, user, info):
        try:
            i = info.contents
            name = PROTO_NAMES[i.proto]
            eng = self.engines[name]
            eng.sync()
            channels = np.flatnonzero(eng._read_counts(C.c_void_p(i.d_counts)))
            if i.replay:
                start = np.empty(self.B, np.uint64)
                self.ctx._call("dh_copy_to_host", _host(start), C.c_void_p(i.d_start), start.nbytes)
                first = start[channels].astype(np.int64) + int(i.skip)
            else:
                first = np.full(len(channels), int(i.live_first), np.int64)
            _row_blocks(eng, name, channels, first, self._blocks)
        except BaseException as e:          # (an exception cannot cross the C frames: push() raises it)
            if self._error is None:
                self._error = e

    def push(self, rows, n=None, counts=None):
        mem = self.ctx.mem
        x, stride = _float_rows(mem, rows, self.B, "DeviceMonitor.push")
        n = x.shape[1] if n is None else int(n)
        if n == 0:
            return []
        if n > self.max_samples:
            raise DhError(_capi.DH_EINVAL, "DeviceMonitor.push", "n = %d > max_samples = %d" % (n, self.max_samples))
        counts = _vector(mem, counts, np.uint32, self.B, "DeviceMonitor.push: counts")
        self._keep = (x, counts)
        if self.pack is not None:
            self._state = None
            self.pack.clear()
            self._call("dh_monitor_push_packed", mem.ptr(x), stride, n, _ptr(mem, counts), self.pack._h)
            header, entries, events, frames = self.pack.read()
            if header["dropped"]:
                raise DhError(_capi.DH_ECAPACITY, "DeviceMonitor.push", "the pack dropped %d blocks" % header["dropped"])
            return _by_position(_packed_blocks(entries, events, frames, "proto", "first_sample", PROTO_NAMES))
        self._blocks, self._error, self._state = [], None, None
        rc = self.ctx.lib.dh_monitor_push(self._h, mem.ptr(x), stride, n, _ptr(mem, counts), self._sink, None)
        blocks, self._blocks = self._blocks, None
        if self._error is not None:
            raise self._error
        _check(rc, "dh_monitor_push", self.ctx.lib)
        return _by_position(blocks)


def channel_taps(input_rate, decimation, passband_hz, stopband_hz, atten_db=60.0, interpolation=1):
    """Real low-pass prototype for Channelizer: a Kaiser-windowed sinc with its cut-off halfway between the pass- and
    stopband edges, the length and beta of Kaiser's estimates for `atten_db` of stopband attenuation, unity gain at DC.
    (`decimation` is not part of the design; it is checked against the stopband: the output rate must hold it.)
    With interpolation = L > 1 the design is at the virtual rate L * input_rate and the sum is L: each of the L phases
    h[r::L] that Channelizer applies to the input has a DC gain of 1 to within the stopband level, so 0 dB stays a
    full-scale tone."""
    L = int(interpolation)
    out_rate = input_rate * L / decimation
    if L < 1:
        raise ValueError("channel_taps: interpolation < 1")
    if not 0 < passband_hz < stopband_hz:
        raise ValueError("channel_taps: need 0 < passband < stopband")
    if stopband_hz > out_rate:
        raise ValueError("channel_taps: the stopband edge %.0f Hz aliases at the output rate %.0f Hz" % (stopband_hz, out_rate))
    input_rate = input_rate * L
    a = float(atten_db)
    dw = 2.0 * np.pi * (stopband_hz - passband_hz) / input_rate
    n = int(np.ceil((a - 7.95) / (2.285 * dw))) + 1
    beta = 0.1102 * (a - 8.7) if a > 50 else (0.5842 * (a - 21) ** 0.4 + 0.07886 * (a - 21) if a >= 21 else 0.0)
    fc = 0.5 * (passband_hz + stopband_hz) / input_rate
    t = np.arange(n) - (n - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * np.kaiser(n, beta)
    return (h * (L / h.sum())).astype(np.float32)


def nco_increment(offset_hz, input_rate):
    """uint32 NCO increment of a channel at `offset_hz` from the centre: offset / rate * 2^32 (two's complement below 0)."""
    return int(round(float(offset_hz) / float(input_rate) * 2.0 ** 32)) & 0xFFFFFFFF


CZ_MAX_INTERPOLATION, CZ_MAX_DECIMATION = 64, 1024
CZ_MAX_RASTER = 16384


def resample_ratio(input_rate, output_rate=48000.0):
    """(L, M), the reduced ratio output_rate / input_rate = L / M: Channelizer's interpolation and decimation for a capture
    rate that is no multiple of the output rate (2.048 MS/s -> 48 kS/s: (3, 128)).  ValueError outside L <= 64, M <= 1024,
    L <= M."""
    from fractions import Fraction
    f = Fraction(output_rate).limit_denominator(10 ** 6) / Fraction(input_rate).limit_denominator(10 ** 6)
    L, M = f.numerator, f.denominator
    if not (1 <= L <= CZ_MAX_INTERPOLATION and L <= M <= CZ_MAX_DECIMATION):
        raise ValueError("resample_ratio: %g -> %g Hz is %d / %d, outside interpolation <= %d, decimation <= %d, ratio <= 1"
                         % (input_rate, output_rate, L, M, CZ_MAX_INTERPOLATION, CZ_MAX_DECIMATION))
    return L, M


def raster_steps(input_rate, raster_hz):
    """K = input_rate / raster_hz of a uniform raster: an integer within 1e-9 relative, in 2 .. 16384, else ValueError."""
    k = float(input_rate) / float(raster_hz)
    K = int(round(k))
    if K < 1 or abs(k - K) > 1e-9 * K:
        raise ValueError("raster: input_rate / raster_hz = %.12g is no integer" % k)
    if not 2 <= K <= CZ_MAX_RASTER:
        raise ValueError("raster: input_rate / raster_hz = %d steps, outside 2 .. %d" % (K, CZ_MAX_RASTER))
    return K


def raster_bins(freqs_hz, input_rate, raster_hz):
    """int32 bins of channels on a uniform raster: freqs_hz[b] = bins[b] * raster_hz, each within 1e-9 relative (of the
    raster step for bin 0), else ValueError naming the channel.  What Channelizer(raster_hz=...) passes as `bins`."""
    raster_steps(input_rate, raster_hz)
    bins = np.zeros(len(freqs_hz), np.int32)
    for b, f in enumerate(freqs_hz):
        q = float(f) / float(raster_hz)
        n = int(round(q))
        if abs(q - n) > 1e-9 * max(abs(n), 1) or abs(n) >= 1 << 31:
            raise ValueError("raster: channel %d at %.12g Hz is no multiple of the %.12g Hz raster" % (b, float(f), float(raster_hz)))
        bins[b] = n
    return bins


def frequency_error_hz(ferr, gate, output_rate):
    """Per channel, how far off its channel the carrier sits, in Hz: the median of ferr * output_rate / 2 over the columns
    whose gate byte is 1, NaN where there is none.  ferr, gate: host arrays [B][n] (Channelizer.ferr_blocks() and
    power_blocks() of one or more pushes, copied to the host).  The value to subtract is what Channelizer.retune takes:
    retune(ch, channel frequency + error)."""
    f = np.asarray(ferr, np.float64) * (float(output_rate) / 2.0)
    g = np.asarray(gate) == 1
    if f.ndim != 2 or f.shape != g.shape:
        raise ValueError("frequency_error_hz: ferr %s and gate %s must be [B][n] both" % (f.shape, g.shape))
    return np.array([np.median(row[m]) if m.any() else np.nan for row, m in zip(f, g)], np.float64)


class Channelizer(_Handle):
    """One wideband complex stream -> one row per channel at input_rate * interpolation / decimation (dh_channelizer; the
    arithmetic is specified in digiham_amd/csrc/channelizer_core.hpp).  interpolation is 1 unless the capture rate is no
    multiple of the output rate; resample_ratio gives the pair, and `taps` is then channel_taps(..., interpolation=L).
    input "cs16" (int16 I / Q pairs) or "cf32" (float32 pairs, or
    complex64); output "fm" (discriminator audio for Engine.push, optionally DC-blocked) or "iq" (complex rows).
    push(x) returns (rows, n_out): rows is the channelizer's own device array [B][max_input * L // D + 1] (x 2 for "iq"),
    valid in [:, :n_out] until the next push.
    raster_hz: every channel sits on a multiple of raster_hz and input_rate / raster_hz is an integer K (12.5 kHz steps of a
    2.4 MS/s capture: K = 192).  All channels then share one polyphase fold of `taps` and differ in a K-point DFT -- the
    same bank for about n_taps / K times less matrix work; needs interpolation = 1.  Without it (the general case) each
    channel may sit anywhere.
    enable_power(...) adds per-channel block power and a squelch gate: after every push `counts` (device uint32 [B]) is what
    Engine.push(rows, n=n_out, counts=cz.counts) takes, and power_blocks() the blocks that push completed; with ferr=True
    also ferr_blocks(), how far off its channel each carrier sits (frequency_error_hz)."""
    _kind = "dh_channelizer"

    def __init__(self, input_rate, decimation, freqs_hz, taps, input="cs16", output="fm", dcblock=True, max_input=1 << 20,
                 ctx=None, device=0, interpolation=1, raster_hz=None):
        self.rate, self.D, self.B = float(input_rate), int(decimation), len(freqs_hz)
        self.L = max(int(interpolation), 1)
        self.input, self.output = input, output
        self.raster_hz = None if raster_hz is None else float(raster_hz)
        t = np.ascontiguousarray(taps, np.float32).ravel()
        if raster_hz is None:
            inc = np.array([nco_increment(f, input_rate) for f in freqs_hz], np.uint32)
            where = dict(increments=inc.ctypes.data_as(C.POINTER(C.c_uint32)))
        else:                         # increments stays NULL: the library does not read it on a raster
            bins = raster_bins(freqs_hz, input_rate, raster_hz)
            where = dict(raster=raster_steps(input_rate, raster_hz), bins=bins.ctypes.data_as(C.POINTER(C.c_int32)))
        self._open(ctx, device, _capi.ChannelizerConfig, n_channels=self.B, decimation=self.D, taps=t.ctypes.data_as(C.POINTER(C.c_float)),
                   n_taps=len(t), input_format=_capi.CZ_INPUT[input],
                   output_mode=_capi.CZ_OUTPUT[output], dcblock=int(bool(dcblock) and output == "fm"), max_input=int(max_input),
                   interpolation=int(interpolation), **where)
        mem = self.ctx.mem
        self.max_input = int(max_input)
        self.out_stride = self.max_input * self.L // self.D + 1
        self.rows = mem.zeros((self.B, self.out_stride) if output == "fm" else (self.B, self.out_stride, 2), np.float32)
        self._keep = None
        self.block, self.power, self.gate, self.counts, self.ferr = 0, None, None, None, None

    @staticmethod
    def _level(db):
        return 0.0 if db is None else float(10.0 ** (float(db) / 10.0))

    def enable_power(self, block=480, open_db=None, close_db=None, hang_blocks=0, ferr=False):
        """Block power over `block` outputs and the squelch gate (before the first push, or right after reset()).  Levels in dB
        relative to |z|^2 = 1 -- a full-scale CS16 tone through unity-gain taps is 0 dB; None: level 0.0 (with both None
        every channel passes: power only).  ferr: also the frequency-error blocks (ferr_blocks(), frequency_error_hz)."""
        mem, block = self.ctx.mem, int(block)
        if block < 1:
            raise DhError(_capi.DH_EINVAL, "dh_channelizer_power_enable", "block < 1")
        stride = self.out_stride // block + 1
        power, gate = mem.zeros((self.B, stride), np.float32), mem.zeros((self.B, stride), np.uint8)
        counts = mem.zeros((self.B,), np.uint32)
        fe = mem.zeros((self.B, stride), np.float32) if ferr else None
        cfg = _capi.ChannelizerPowerConfig(C.sizeof(_capi.ChannelizerPowerConfig), block, self._level(open_db), self._level(close_db),
                                           int(hang_blocks), mem.ptr(power), mem.ptr(gate), mem.ptr(counts), stride,
                                           mem.ptr(fe) if ferr else None)
        self._call("dh_channelizer_power_enable", C.byref(cfg))
        self.block, self.power, self.gate, self.counts, self.ferr = block, power, gate, counts, fe

    def set_squelch(self, open_db, close_db, hang_blocks):
        self._call("dh_channelizer_set_squelch", self._level(open_db), self._level(close_db), int(hang_blocks))

    def power_blocks(self):
        """(power[:, :n], gate[:, :n], first_block) of the last push, device arrays: column i is block first_block + i."""
        first, n = C.c_uint64(0), C.c_size_t(0)
        self._call("dh_channelizer_power_last", C.byref(first), C.byref(n))
        return self.power[:, :n.value], self.gate[:, :n.value], first.value

    def ferr_blocks(self):
        """(ferr[:, :n], first_block) of the last push, a device array: column i is block first_block + i, in units of half
        the output rate (frequency_error_hz).  Needs enable_power(ferr=True)."""
        first, n = C.c_uint64(0), C.c_size_t(0)
        self._call("dh_channelizer_power_last", C.byref(first), C.byref(n))
        if self.ferr is None:
            raise DhError(_capi.DH_EINVAL, "Channelizer.ferr_blocks", "enable_power(ferr=True) first")
        return self.ferr[:, :n.value], first.value

    def reset(self):
        self._call("dh_channelizer_reset")

    def retune(self, ch, hz):
        if self.raster_hz is not None:
            try:
                v = int(raster_bins([hz], self.rate, self.raster_hz)[0]) & 0xFFFFFFFF
            except ValueError:
                raise ValueError("raster: channel %d at %.12g Hz is no multiple of the %.12g Hz raster" % (ch, float(hz), self.raster_hz)) from None
        else:
            v = nco_increment(hz, self.rate)
        self._call("dh_channelizer_retune", int(ch), v)

    def push(self, x):
        """x: numpy (host) or a device array: int16 [n][2] / [2 n] for "cs16", float32 [n][2] / [2 n] or complex64 [n] for
        "cf32".  Returns (rows, n_out)."""
        mem = self.ctx.mem
        if isinstance(x, np.ndarray):
            a = np.ascontiguousarray(x.view(np.float32) if x.dtype == np.complex64 else x, np.int16 if self.input == "cs16" else np.float32)
            n = a.size // 2
            dev = mem.is_device_array(a) and not hasattr(mem, "torch")
        else:
            want = mem.torch.int16 if self.input == "cs16" else mem.torch.float32
            if x.dtype != want or not x.is_contiguous():
                raise ValueError("Channelizer.push: need a contiguous %s device array, got %s" % (want, x.dtype))
            a, n, dev = x, x.numel() // 2, True
        cnt = C.c_size_t(0)
        self._keep = a              # asynchronous: the input stays alive until the next push
        self._call("dh_channelizer_push" if dev else "dh_channelizer_push_host", mem.ptr(a) if dev else _host(a), n, mem.ptr(self.rows),
                   self.out_stride, C.byref(cnt))
        return self.rows, cnt.value

    def phasor(self, phi):
        """P(phi) of the specification for uint32 phase words (host arithmetic) -> complex128 array."""
        p = np.ascontiguousarray(phi, np.uint32).ravel()
        out = np.zeros((p.size, 2), np.float32)
        self.ctx._call("dh_channelizer_phasor", _host(p), _host(out), p.size)
        return out[:, 0].astype(np.float64) + 1j * out[:, 1].astype(np.float64)
