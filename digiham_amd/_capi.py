"""ctypes declarations for include/digiham_amd.h and the loader of the gfx950 library.

The product library is ``digiham_amd/libdigiham_amd.so`` (built in-tree by
``__graft_entry__.build()``).  There is no CPU implementation behind this
module: if the library is missing, or no MI355X is visible, loading raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdigiham_amd.so")

DH_OK, DH_EINVAL, DH_ENOMEM, DH_EDEVICE, DH_ENODEV, DH_ECAPACITY = 0, -1, -2, -3, -4, -5
RRC = {"none": 0, None: 0, "wide": 1, "narrow": 2, "custom": 3}
DEMOD = {"none": 0, None: 0, "fsk": 2, "fsk2": 2, "gfsk": 4, "gfsk4": 4}
PROTO = {"none": 0, None: 0, "dmr": 1, "ysf": 2, "nxdn": 3, "pocsag": 4, "dstar": 5, "scan": 6}
FLAG_FAST_FIR, FLAG_KEEP_FILTERED, FLAG_FSK_INVERT, FLAG_NO_EVENTS, FLAG_ORDERED_TIMING, FLAG_SPLIT_STAGES = 1, 2, 4, 8, 16, 32
FLAG_EXACT_SYMBOLS, FLAG_EXACT_FIR, FLAG_OVERLAP_PUSHES, FLAG_ONE_LAUNCH = 64, 128, 256, 512
FLAG_DMR_BOTH_SLOTS = 0x400
FLAG_CALL_DIGEST = 0x800                   # DH_FLAG_CALL_DIGEST: the event rows leave as call records ("Call digest", include/digiham_amd.h)
EV_CALL = 96                               # DH_EV_CALL
CALL_RECORD_BYTES = {"dmr": 16, "nxdn": 8, "ysf": 21}
DMR_SLOT_RECORD_BYTES = 28                 # DH_DMR_SLOT_RECORD_BYTES: 27 payload bytes and the slot


class EngineConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32),
                ("max_samples", C.c_uint32), ("rrc", C.c_int32), ("demod", C.c_int32), ("sps", C.c_uint32),
                ("proto", C.c_int32), ("flags", C.c_uint32), ("slot_filter", C.c_uint32), ("stream", C.c_void_p),
                ("rrc_taps", C.POINTER(C.c_float)), ("rrc_nzeros", C.c_uint32), ("rrc_gain", C.c_double)]


class ChannelizerConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("decimation", C.c_uint32),
                ("taps", C.POINTER(C.c_float)), ("n_taps", C.c_uint32), ("increments", C.POINTER(C.c_uint32)),
                ("input_format", C.c_int32), ("output_mode", C.c_int32), ("dcblock", C.c_int32), ("max_input", C.c_uint32),
                ("stream", C.c_void_p), ("interpolation", C.c_uint32), ("raster", C.c_uint32), ("bins", C.POINTER(C.c_int32))]


class ChannelizerPowerConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("block", C.c_uint32), ("open_level", C.c_float), ("close_level", C.c_float),
                ("hang_blocks", C.c_uint32), ("d_power", C.c_void_p), ("d_gate", C.c_void_p), ("d_counts", C.c_void_p),
                ("stride", C.c_size_t), ("d_ferr", C.c_void_p)]


CHANNELIZER_POWER_CONFIG_V1_SIZE = ChannelizerPowerConfig.d_ferr.offset      # DH_CHANNELIZER_POWER_CONFIG_V1_SIZE


class PrerollConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("depth", C.c_uint32),
                ("stream", C.c_void_p)]


class MonitorConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_channels", C.c_uint32), ("max_samples", C.c_uint32),
                ("depth", C.c_uint32), ("lead", C.c_uint32), ("confirm", C.c_uint32), ("release", C.c_uint32),
                ("protos", C.c_uint32), ("stream", C.c_void_p), ("dmr_both_slots", C.c_uint32), ("reserved", C.c_uint32),
                ("close_hits", C.c_uint32 * 5), ("close_dist", C.c_uint32 * 5)]


MONITOR_CONFIG_V1_SIZE = MonitorConfig.dmr_both_slots.offset       # DH_MONITOR_CONFIG_V1_SIZE
MONITOR_CONFIG_V2_SIZE = MonitorConfig.close_hits.offset           # DH_MONITOR_CONFIG_V2_SIZE


class MonitorPushInfo(C.Structure):
    _fields_ = [("proto", C.c_int32), ("replay", C.c_int32), ("engine", C.c_void_p), ("d_counts", C.c_void_p),
                ("d_start", C.c_void_p), ("skip", C.c_uint64), ("live_first", C.c_uint64)]


class OutpackConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("max_entries", C.c_uint32), ("max_events", C.c_uint32),
                ("max_frame_bytes", C.c_uint64), ("stream", C.c_void_p)]


class OutpackHeader(C.Structure):
    _fields_ = [("n_entries", C.c_uint32), ("n_events", C.c_uint32), ("frame_bytes", C.c_uint64), ("dropped", C.c_uint32),
                ("appends", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# dh_outpack_entry
OUTPACK_ENTRY_DTYPE = [("channel", "<u4"), ("user", "<u4"), ("tag", "<u8"), ("n_frame_bytes", "<u4"), ("n_events", "<u4"),
                       ("frame_offset16", "<u4"), ("event_index", "<u4")]

MONITOR_SINK = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(MonitorPushInfo))       # dh_monitor_sink
MONITOR_FRONTS = ("wide10", "narrow20", "fsk10", "fsk40i")                    # dh_monitor_scan_engine's index

PREROLL_NONE = 0xFFFFFFFFFFFFFFFF          # DH_PREROLL_NONE

# protocol scan (DH_PROTO_SCAN): the patterns in the order of DH_SCAN_*, dh_scan_stat, DH_EV_SCAN_HIT
SCAN_PATTERNS = ("dmr_bs_data", "dmr_bs_voice", "dmr_ms_data", "dmr_ms_voice", "ysf", "nxdn", "dstar_header", "dstar_voice", "pocsag")
SCAN_STAT_DTYPE = [("hits", "<u4"), ("periodic", "<u4"), ("last_sym", "<u4"), ("best_dist", "u1"), ("pad", "u1", (3,))]
EV_SCAN_HIT = 80


class _ChannelizerConfigV2(C.Structure):    # dh_channelizer_config when it ended with interpolation
    _fields_ = ChannelizerConfig._fields_[:-2]


# what a caller built against that header passes as struct_size: its tail padding (where raster now sits) included
CHANNELIZER_CONFIG_V2_SIZE = C.sizeof(_ChannelizerConfigV2)

CZ_INPUT = {"cs16": 1, "cf32": 2}
CZ_OUTPUT = {"iq": 1, "fm": 2}


class DhError(RuntimeError):
    def __init__(self, code, what, detail=""):
        names = {-1: "DH_EINVAL", -2: "DH_ENOMEM", -3: "DH_EDEVICE", -4: "DH_ENODEV", -5: "DH_ECAPACITY"}
        super().__init__("%s failed: %s %s" % (what, names.get(code, code), detail))
        self.code = code


class DhInvalid(DhError, ValueError):
    """a DH_EINVAL that names the Python arguments that caused it"""


def _signatures():
    """name -> (restype, argtypes) of every symbol of include/digiham_amd.h: the one list declare() and EXPORTED_SYMBOLS read."""
    vp, sz, u32, u64, P = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.POINTER
    def i(*args):
        return C.c_int, list(args)
    block, view = i(vp, vp, sz, vp), i(vp, P(vp), P(sz), P(vp))
    return {
        "dh_version": (C.c_char_p, []), "dh_last_error": (C.c_char_p, []), "dh_device_count": i(),
        "dh_device_alloc": i(C.c_int, sz, P(vp)), "dh_device_free": i(vp),
        "dh_copy_to_host": i(vp, vp, sz), "dh_copy_to_device": i(vp, vp, sz),
        "dh_hamming_7_4": block, "dh_hamming_13_9": block, "dh_hamming_15_11": block, "dh_hamming_16_11": block,
        "dh_quadratic_residue": block, "dh_golay_20_8": block, "dh_golay_24_12": block, "dh_bch_31_21": block,
        "dh_bptc_196_96": i(vp, vp, vp, sz, vp),
        "dh_trellis": i(vp, sz, C.c_int, vp, sz, vp, sz, vp),
        "dh_crc16": i(vp, sz, C.c_int, vp, sz, vp),
        "dh_whitening": i(vp, vp, sz, C.c_int, sz, vp),
        "dh_dvfilter_s16": i(vp, vp, vp, sz, sz, sz, vp),
        "dh_frontend_s16": i(vp, sz, vp, sz, vp, sz, sz, C.c_int, C.c_int, vp),
        "dh_debug_div_gain": i(vp, vp, sz, C.c_int, vp),
        "dh_debug_div_const": i(vp, vp, sz, C.c_uint, vp),
        "dh_debug_mfma_f16": i(vp, vp, vp, vp, sz, vp),
        "dh_debug_f16_split": i(vp, vp, vp, sz, C.c_float, vp),
        "dh_debug_copy": i(vp, vp, sz, vp),
        "dh_debug_seam_probe": i(C.c_int, vp, vp, sz, vp), "dh_debug_seam_probe_words": i(C.c_int, P(sz), P(sz)),
        "dh_engine_create": i(P(EngineConfig), P(vp)), "dh_engine_destroy": (None, [vp]),
        "dh_engine_reset": i(vp), "dh_engine_set_slot_filter": i(vp, u32),
        "dh_engine_reset_channel": i(vp, u32), "dh_engine_reset_channels": i(vp, vp), "dh_engine_set_slot_filter_channel": i(vp, u32, u32),
        "dh_engine_push": i(vp, vp, sz, sz), "dh_engine_push_host": i(vp, vp, sz, sz),
        "dh_engine_push_ragged": i(vp, vp, sz, vp, sz), "dh_engine_push_host_ragged": i(vp, vp, sz, vp, sz),
        "dh_engine_push_symbols": i(vp, vp, sz, vp),
        "dh_engine_filtered": i(vp, P(vp), P(sz)), "dh_engine_symbols": view, "dh_engine_frames": view, "dh_engine_events": view,
        "dh_engine_read_symbols": i(vp, u32, vp, P(sz)), "dh_engine_read_frames": i(vp, u32, vp, P(sz)),
        "dh_engine_read_events": i(vp, u32, vp, P(sz)), "dh_engine_read_filtered": i(vp, u32, vp, P(sz)),
        "dh_engine_sync": i(vp),
        "dh_engine_timing_enable": i(vp, u32),
        "dh_engine_timing_read": i(vp, vp, vp, vp, P(u32)),
        "dh_engine_timing_read_split": i(vp, vp, vp, P(u32)),
        "dh_engine_timing_stats": i(vp, vp, vp),
        "dh_engine_debug_header": i(vp, u32, vp),
        "dh_channelizer_create": i(P(ChannelizerConfig), P(vp)), "dh_channelizer_destroy": (None, [vp]),
        "dh_channelizer_reset": i(vp), "dh_channelizer_retune": i(vp, u32, u32),
        "dh_channelizer_push": i(vp, vp, sz, vp, sz, P(sz)), "dh_channelizer_push_host": i(vp, vp, sz, vp, sz, P(sz)),
        "dh_channelizer_phasor": i(vp, vp, sz),
        "dh_channelizer_power_enable": i(vp, P(ChannelizerPowerConfig)),
        "dh_channelizer_set_squelch": i(vp, C.c_float, C.c_float, u32),
        "dh_channelizer_power_last": i(vp, P(u64), P(sz)),
        "dh_preroll_create": i(P(PrerollConfig), P(vp)), "dh_preroll_destroy": (None, [vp]),
        "dh_preroll_reset": i(vp), "dh_preroll_append": i(vp, vp, sz, sz, vp),
        "dh_preroll_total": i(vp, P(u64)), "dh_preroll_open_at": i(vp, vp),
        "dh_preroll_gather": i(vp, vp, u64, sz, vp, sz, vp, vp),
        "dh_preroll_gather_device": i(vp, vp, u64, sz, vp, sz, vp),
        "dh_monitor_create": i(P(MonitorConfig), P(vp)), "dh_monitor_destroy": (None, [vp]), "dh_monitor_reset": i(vp),
        "dh_monitor_push": i(vp, vp, sz, sz, vp, MONITOR_SINK, vp), "dh_monitor_push_packed": i(vp, vp, sz, sz, vp, vp),
        "dh_monitor_state": i(vp, vp, vp), "dh_monitor_total": i(vp, P(u64)),
        "dh_monitor_engine": (vp, [vp, C.c_int]), "dh_monitor_scan_engine": (vp, [vp, C.c_int]),
        "dh_outpack_create": i(P(OutpackConfig), P(vp)), "dh_outpack_destroy": (None, [vp]), "dh_outpack_clear": i(vp),
        "dh_outpack_append": i(vp, vp, vp, vp, u64, u32),
        "dh_outpack_read": i(vp, P(OutpackHeader), vp, vp, vp),
        "dh_outpack_device": i(vp, P(vp), P(vp), P(vp), P(vp)),
    }


# the ops of dh_debug_seam_probe, in the order of enum dh_probe_op (include/digiham_amd.h)
PROBE_OPS = {name: i for i, name in enumerate(
    """VMIN VMAX MIN3_ABS MAX3_ABS MAX_ABS_GROUPS5 MUL_UNIFORM SQRT_UPPER DIV_CONST2 F2_MAC F2_MAC_FAST F2_MAC_PAIR_LO F2_MAC_PAIR_HI
    F2_MAC_PAIR_FAST_LO F2_MAC_PAIR_FAST_HI F2_FMA F2_SCALE F16_SPLIT4_PLAIN WAVE_MAX WAVE_MAX_NAN WAVE_MIN ROW0_MIN ROW_SUM5_PAIR
    AGC_SCAN AGC_SCAN_PAIRS LDS_RUN20 LDS_RUN40 LDS_RUN20_WITH_PAIR LDS_PAIRS3_NOW LDS_READS LDS_STORE4_AT LDS_STORE4_AT_PLAIN
    LDS_STORE_ROW10_0 LDS_STORE_ROW10_1000 LDS_STORE_ROW10_2000 LDS_STORE_ROW10_3000 LDS_STORE_PAIR LDS_STORE_ROWS10_PAIR
    LV_READ LV_DOWN LS_WRITE_READ LS_GATHER LANES_BELOW STATE BITS""".split())}

SIGNATURES = _signatures()
EXPORTED_SYMBOLS = list(SIGNATURES)


def declare(L, lenient=False):
    """Attach argtypes / restypes for every symbol of include/digiham_amd.h."""
    for name, (restype, argtypes) in SIGNATURES.items():
        if lenient and not hasattr(L, name):        # A/B build variants of older sources (tools/) may lack new entry points
            continue
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    return L


_LIB = None


def load(path=None):
    """Load the gfx950 library.  Raises if it has not been built -- there is no fallback."""
    global _LIB
    if path is None and _LIB is not None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError("digiham_amd: %s is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback." % p)
    # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be the HIP runtime of the process, so it has to
    # be loaded before this library's NEEDED entry is resolved (two HIP runtimes in one process cannot see
    # each other's devices, streams or allocations).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = declare(C.CDLL(p), lenient=path is not None)
    if path is None:
        _LIB = L
    return L
