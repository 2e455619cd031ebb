"""The binding's handle plumbing (digiham_amd/api.py: _Handle, _float_rows, _vector; _capi.SIGNATURES): every class that owns
a library handle, or is made of such classes, opens, closes twice, refuses work once closed and survives a constructor
that the library turned down; the argument conversions hand the library what they were given wherever it can read that in
place.  The smallest shapes: 2 channels, 256 samples, a ring of 512, a 16-tap channelizer at decimation 4."""
import numpy as np
import pytest

import hostemu
from digiham_amd import _capi, api
from digiham_amd._capi import DhError

TAPS = np.hanning(18)[1:-1].astype(np.float32)

# name -> (constructor arguments, arguments the library rejects, a method that needs the object open)
KINDS = {
    "Engine": (lambda ctx: api.Engine(2, 256, ctx=ctx), lambda ctx: api.Engine(2, 256, sps=2, ctx=ctx), "reset"),
    "Scanner": (lambda ctx: api.Scanner(2, 256, ctx=ctx), lambda ctx: api.Scanner(0, 256, ctx=ctx), "reset"),
    "Preroll": (lambda ctx: api.Preroll(2, 512, ctx=ctx), lambda ctx: api.Preroll(2, 0, ctx=ctx), "reset"),
    "OutPack": (lambda ctx: api.OutPack(4, 8, 64, ctx=ctx), lambda ctx: api.OutPack(0, 8, 64, ctx=ctx), "clear"),
    "Channelizer": (lambda ctx: api.Channelizer(192000.0, 4, [0.0, 12500.0], TAPS, max_input=256, ctx=ctx),
                    lambda ctx: api.Channelizer(192000.0, 0, [0.0, 12500.0], TAPS, max_input=256, ctx=ctx), "reset"),
    "Monitor": (lambda ctx: api.Monitor(2, 256, depth=512, ctx=ctx), lambda ctx: api.Monitor(2, 256, depth=0, ctx=ctx), "reset"),
    "DeviceMonitor": (lambda ctx: api.DeviceMonitor(2, 256, depth=512, ctx=ctx), lambda ctx: api.DeviceMonitor(2, 256, depth=0, ctx=ctx), "reset"),
    "DeviceMonitor(packed)": (lambda ctx: api.DeviceMonitor(2, 256, depth=512, ctx=ctx, packed=True),
                              lambda ctx: api.DeviceMonitor(2, 256, depth=0, ctx=ctx, packed=True), "reset"),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_open_close_twice_and_closed_means_error(ctx, kind):
    make, _, method = KINDS[kind]
    obj = make(ctx)
    getattr(obj, method)()                      # open: the method works
    obj.close()
    assert obj._h is None
    obj.close()
    assert obj._h is None
    with pytest.raises(DhError):
        getattr(obj, method)()
    obj.__del__()                               # what the collector will do


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rejected_constructor_leaves_an_object_that_dies_quietly(ctx, kind, monkeypatch):
    _, make_bad, _ = KINDS[kind]
    born = []
    cls = getattr(api, kind.split("(")[0])
    real_init = cls.__init__
    monkeypatch.setattr(cls, "__init__", lambda self, *a, **kw: (born.append(self), real_init(self, *a, **kw))[1])
    with pytest.raises(DhError) as err:
        make_bad(ctx)
    assert err.value.code == _capi.DH_EINVAL
    assert len(born) == 1 and born[0]._h is None
    born[0].__del__()                           # must not raise
    born[0].close()


def test_device_monitor_owns_its_engines(ctx):
    mon = api.DeviceMonitor(2, 256, depth=512, ctx=ctx)
    assert set(mon.engines) == {"dmr", "ysf", "nxdn", "dstar", "pocsag"} and mon.scanner_engines is mon.scanner.engines
    borrowed = mon.engines["dmr"]
    borrowed.close()                            # a view: the monitor's engine lives on
    assert borrowed._h is None
    rows = ctx.mem.from_numpy(np.zeros((2, 256), np.float32))
    assert mon.push(rows) == [] and mon.total == 256
    mon.close()
    assert mon.engines == {} and mon.scanner.engines == {}
    with pytest.raises(DhError):
        mon.push(rows)


def test_float_rows_hands_over_what_the_library_can_read_in_place():
    mem = hostemu.NumpyMemory()
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    wide = np.arange(30, dtype=np.float32).reshape(3, 10)
    col, one = wide[:, 2:7], wide[:1, 2:7]
    for x, B, stride in ((a, 3, 4), (col, 3, 10), (one, 1, 5), (a[1:2], 1, 4), (np.zeros(6, np.float32)[None, :], 1, 6)):
        got, s = api._float_rows(mem, x, B, "test")
        assert got is x and s == stride
    for x in (a.astype(np.float64), a.tolist(), a.astype(np.int16), wide[:, ::2], a.ravel()):
        got, s = api._float_rows(mem, x, 3, "test")
        want = np.asarray(x, np.float32).reshape(3, -1)
        assert got is not x and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and s == want.shape[1] and (got == want).all()
        assert not np.shares_memory(got, np.asarray(x))


def test_vector_checks_length_and_element_size():
    mem = hostemu.NumpyMemory()
    assert api._vector(mem, None, np.uint32, 4, "test") is None
    for a, dtype in ((np.arange(4, dtype=np.uint32), np.uint32), (np.arange(4, dtype=np.int32), np.uint32),
                     (np.arange(4, dtype=np.int64), np.uint64), (np.ones(4, np.uint8), np.uint8), (np.ones(4, bool), np.uint8)):
        assert api._vector(mem, a, dtype, 4, "test") is a
    for a in ([1, 0, 3, 2], (1, 0, 3, 2)):
        got = api._vector(mem, a, np.uint32, 4, "test")
        assert got is not a and got.dtype == np.uint32 and list(got) == [1, 0, 3, 2]
    strided = np.arange(8, dtype=np.uint32)[::2]            # not contiguous: no device array, copied
    got = api._vector(mem, strided, np.uint32, 4, "test")
    assert got is not strided and got.flags["C_CONTIGUOUS"] and list(got) == [0, 2, 4, 6]
    for a, dtype, n in ((np.zeros(5, np.uint32), np.uint32, 4), (np.zeros(3, np.uint32), np.uint32, 4), ([1, 2, 3], np.uint32, 4),
                        (np.zeros((4, 1), np.uint32), np.uint32, 4), (np.zeros(4, np.uint8), np.uint32, 4),
                        (np.zeros(4, np.int64), np.uint32, 4), (np.zeros(4, np.uint32), np.uint64, 4), (np.zeros(4, np.uint32), np.uint8, 4)):
        with pytest.raises(ValueError, match="test"):
            api._vector(mem, a, dtype, n, "test")


def test_rejections_name_the_class(emu_ctx):
    eng = api.Engine(2, 256, ctx=emu_ctx)
    pre = api.Preroll(2, 512, ctx=emu_ctx)
    with pytest.raises(ValueError, match="Engine.reset_channels"):
        eng.reset_channels(np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match="Engine.push"):
        eng.push(np.zeros((2, 16), np.float32), counts=np.zeros(3, np.uint32))
    with pytest.raises(ValueError, match="Preroll.gather_device"):
        pre.gather_device(np.zeros(3, np.uint64), 0, 4)
    with pytest.raises(ValueError, match="Preroll.append"):
        pre.append(np.zeros((2, 16), np.float32), counts=np.zeros(2, np.uint8))
    eng.close()
    pre.close()


SYMBOLS = [
    "dh_bch_31_21", "dh_bptc_196_96", "dh_channelizer_create", "dh_channelizer_destroy", "dh_channelizer_phasor",
    "dh_channelizer_power_enable", "dh_channelizer_power_last", "dh_channelizer_push", "dh_channelizer_push_host",
    "dh_channelizer_reset", "dh_channelizer_retune", "dh_channelizer_set_squelch", "dh_copy_to_device", "dh_copy_to_host", "dh_crc16",
    "dh_debug_copy", "dh_debug_div_const", "dh_debug_div_gain", "dh_debug_f16_split", "dh_debug_mfma_f16", "dh_debug_seam_probe",
    "dh_debug_seam_probe_words", "dh_device_alloc",
    "dh_device_count", "dh_device_free", "dh_dvfilter_s16", "dh_engine_create", "dh_engine_debug_header", "dh_engine_destroy",
    "dh_engine_events", "dh_engine_filtered", "dh_engine_frames", "dh_engine_push", "dh_engine_push_host", "dh_engine_push_host_ragged",
    "dh_engine_push_ragged", "dh_engine_push_symbols", "dh_engine_read_events", "dh_engine_read_filtered", "dh_engine_read_frames",
    "dh_engine_read_symbols", "dh_engine_reset", "dh_engine_reset_channel", "dh_engine_reset_channels", "dh_engine_set_slot_filter",
    "dh_engine_set_slot_filter_channel", "dh_engine_symbols", "dh_engine_sync", "dh_engine_timing_enable", "dh_engine_timing_read",
    "dh_engine_timing_read_split", "dh_engine_timing_stats", "dh_frontend_s16", "dh_golay_20_8", "dh_golay_24_12", "dh_hamming_13_9",
    "dh_hamming_15_11", "dh_hamming_16_11", "dh_hamming_7_4", "dh_last_error", "dh_monitor_create", "dh_monitor_destroy",
    "dh_monitor_engine", "dh_monitor_push", "dh_monitor_push_packed", "dh_monitor_reset", "dh_monitor_scan_engine", "dh_monitor_state",
    "dh_monitor_total", "dh_outpack_append", "dh_outpack_clear", "dh_outpack_create", "dh_outpack_destroy", "dh_outpack_device",
    "dh_outpack_read", "dh_preroll_append", "dh_preroll_create", "dh_preroll_destroy", "dh_preroll_gather", "dh_preroll_gather_device",
    "dh_preroll_open_at", "dh_preroll_reset", "dh_preroll_total", "dh_quadratic_residue", "dh_trellis", "dh_version", "dh_whitening"]


def test_exported_symbols_are_the_same_list():
    assert sorted(_capi.EXPORTED_SYMBOLS) == SYMBOLS and len(set(_capi.EXPORTED_SYMBOLS)) == len(SYMBOLS)
    assert list(_capi.SIGNATURES) == _capi.EXPORTED_SYMBOLS
