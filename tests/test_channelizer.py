"""dh_channelizer: one wideband I / Q stream -> B channel rows at rate / D (digiham_amd/csrc/channelizer_core.hpp).

Both tiers (the `ctx` fixture: CPU emulation of the kernel bodies, and the gfx950 library on -m gpu):
  * byte-for-byte equality with tests/cz_restate.c, a scalar restatement of the written specification;
  * streaming: ragged pushes, retune, reset;
  * physics in float64: passband gain and phase, stopband attenuation, FM of a tone, the phasor table;
  * end to end: a CS16 composite of DMR / YSF transmitters -> channelizer (FM + DC) -> engines, equal to the oracle on the
    channelizer's own rows, with the generated source / target in the LC events;
  * argument validation.
"""
import ctypes as C

import numpy as np
import pytest

from cz_harness import cfg, create, end_to_end, end_to_end_fixture, fixed, incs_for, make_input, restate, run_lib, taps_for      # noqa: F401  (fixture)
from digiham_amd import api
from digiham_amd._capi import DhError


# (format, output, dcblock, D, T, B)
EXACT_CASES = [("cs16", "iq", False, 1, 13, 3), ("cf32", "fm", False, 7, 37, 17), ("cs16", "fm", True, 16, 70, 20),
               ("cf32", "iq", False, 50, 101, 9), ("cs16", "fm", True, 50, 130, 70)]


@pytest.mark.parametrize("fmt,output,dc,D,T,B", EXACT_CASES)
def test_bit_exact_against_restatement(ctx, restate, fmt, output, dc, D, T, B):
    x = make_input(fmt, 1500 + 3 * D, D + T)
    h = taps_for(T)
    incs = incs_for(B, B)
    got = run_lib(ctx, fixed(D), x, fmt, h, incs, output, dc)
    ref = restate.run(fixed(D), x, fmt == "cf32", h, incs, output == "fm", dc)
    assert got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()


def test_subnormal_operands_bit_exact(ctx, restate):
    """Tiny CF32 input and taps: products, sums and rotations land in the subnormal range; they are kept (IEEE) on both
    sides, and device, emulation and restatement agree byte for byte."""
    x = make_input("cf32", 600, 5, scale=1e-36)
    x[::7] = 0.0
    h = taps_for(21, 1e-3, seed=3)
    incs = incs_for(12, 4)
    for output, dc in (("iq", False), ("fm", True)):
        got = run_lib(ctx, fixed(7), x, "cf32", h, incs, output, dc)
        ref = restate.run(fixed(7), x, True, h, incs, output == "fm", dc)
        if output == "iq":
            assert (np.abs(ref[ref != 0]) < 1.1754944e-38).any(), "the case must reach subnormal outputs"
        assert got.tobytes() == ref.tobytes()


def test_streaming_pushes_retune_reset(ctx, restate):
    D, T, B = 7, 45, 19
    bank = fixed(D)
    x = make_input("cs16", 4000, 9)
    h = taps_for(T, seed=1)
    incs = incs_for(B, 2)
    whole = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True)
    pushes = [0, 1, D - 1, D, 7 * D + 3, 0, 2500, 5]
    pushes.append(4000 - sum(pushes))
    ragged = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True, pushes=pushes)
    assert ragged.tobytes() == whole.tobytes()
    # a retune mid-stream (channels 3 and 11 at push 6), then one more at push 8
    ret = {6: {3: 0x12345678, 11: 0}, 8: {3: 0xFEDCBA98}}
    got = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True, pushes=pushes, retunes=ret)
    ref = restate.run(bank, x, False, h, incs, True, True, pushes=pushes, retunes=ret)
    assert got.tobytes() == ref.tobytes()
    # reset: a fresh stream
    cz = api.Channelizer(1.0, D, [0.0] * B, h, input="cs16", output="fm", max_input=4000, ctx=ctx)
    for ch, u in enumerate(incs):
        assert ctx.lib.dh_channelizer_retune(cz._h, ch, u) == 0
    first = run_lib(ctx, bank, x[:3000], "cs16", h, incs, "fm", True, pushes=[1000, 2000], cz=cz)
    cz.reset()
    again = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True, pushes=[4000], cz=cz)
    cz.close()
    assert again.tobytes() == whole.tobytes()
    assert first.tobytes() == whole[:, :first.shape[1]].tobytes()


def test_phasor_table(ctx):
    cz = api.Channelizer(1.0, 1, [0.0], [1.0], output="iq", max_input=16, ctx=ctx)
    rng = np.random.default_rng(0)
    phi = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
                          np.array([0, 1, 127, 128, 255, 256, 0x7FFFFF80, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], np.uint32)])
    p = cz.phasor(phi)
    cz.close()
    err = np.abs(p - np.exp(2j * np.pi * phi.astype(np.float64) / 2.0 ** 32))
    assert err.max() <= 1e-6


def test_ddc_physics(ctx):
    rate, D = 768000.0, 16
    h = api.channel_taps(rate, D, 6500.0, 12000.0, 60.0)
    T = len(h)
    Tp = 16 * ((T + 15) // 16)
    freqs = [0.0, 100000.0, -237500.0, 312500.0]
    incs = [api.nco_increment(f, rate) for f in freqs]
    n = 8000
    nn = np.arange(n, dtype=np.float64)
    A = 0.5
    H = lambda d: np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * d / rate * np.arange(T)))
    sum_h = float(np.abs(h.astype(np.float64)).sum())
    for b, u in enumerate(incs):
        fb = u / 2.0 ** 32 * rate
        for delta, stop in ((1234.5, False), (-4000.0, False), (15000.0, True), (-40000.0, True)):
            xs = A * np.exp(2j * np.pi * ((u / 2.0 ** 32) + delta / rate) * nn)
            x = np.stack([xs.real, xs.imag], 1).astype(np.float32)
            z = run_lib(ctx, fixed(D), x, "cf32", h, [u], "iq", False, rate=rate)[0]
            z = z[:, 0].astype(np.float64) + 1j * z[:, 1]
            j = np.arange(len(z))
            nj = j * D + D - 1
            ok = nj >= Tp
            if not stop:
                want = H(delta) * A * np.exp(2j * np.pi * delta * nj / rate)
                err = np.abs(z - want)[ok].max()
                assert err <= 1e-5 * sum_h * A, (fb, delta, err)
            else:
                fgrid = np.linspace(12000.0, rate / 2, 4000) * np.sign(delta)
                hmax = max(abs(H(f)) for f in fgrid)
                assert hmax <= 10 ** (-60 / 20) * 1.2
                assert np.abs(z[ok]).max() <= abs(H(delta)) * A + 1e-5 * sum_h * A
                assert np.abs(z[ok]).max() <= 1.2e-3 * A
    # FM of a pure tone: 2 delta / rate_out; with the DC blocker it decays
    delta = 2100.0
    xs = A * np.exp(2j * np.pi * ((incs[1] / 2.0 ** 32) + delta / rate) * nn)
    x = np.stack([xs.real, xs.imag], 1).astype(np.float32)
    fm = run_lib(ctx, fixed(D), x, "cf32", h, [incs[1]], "fm", False, rate=rate)[0].astype(np.float64)
    steady = fm[Tp // D + 2:]
    assert np.abs(steady - 2 * delta / (rate / D)).max() <= 1e-6
    dc = run_lib(ctx, fixed(D), x, "cf32", h, [incs[1]], "fm", True, rate=rate)[0].astype(np.float64)
    assert abs(dc[-1]) < 0.15 * np.abs(dc[Tp // D + 2:Tp // D + 20]).max()        # 0.995^(n_out - 30) ~ 0.1


def test_validation(ctx):
    lib = ctx.lib
    h = np.ones(8, np.float32)
    bad = [dict(decimation=0), dict(decimation=1025), dict(n_taps=0), dict(n_taps=16385), dict(n_channels=0), dict(n_channels=65537),
           dict(input_format=3), dict(output_mode=0), dict(max_input=0), dict(struct_size=8),
           dict(taps=C.POINTER(C.c_float)()), dict(increments=C.POINTER(C.c_uint32)()), dict(output_mode=1, dcblock=1)]
    for kw in bad:
        assert create(ctx, cfg(ctx, **kw)) == -1, kw
    assert create(ctx, cfg(ctx, n_taps=2, taps=np.array([1.0, np.nan], np.float32))) == -1
    assert lib.dh_channelizer_create(None, C.byref(C.c_void_p())) == -1
    cz = api.Channelizer(1.0, 4, [0.0] * 4, h, max_input=1000, ctx=ctx)
    x = np.zeros((100, 2), np.int16)
    n_out = C.c_size_t(0)
    xp = ctx.mem.from_numpy(x)
    assert lib.dh_channelizer_push(cz._h, ctx.mem.ptr(xp), 100, ctx.mem.ptr(cz.rows), 24, C.byref(n_out)) == -1      # 25 outputs
    assert lib.dh_channelizer_push(cz._h, ctx.mem.ptr(xp), 1001, ctx.mem.ptr(cz.rows), 300, C.byref(n_out)) == -1    # > max_input
    assert lib.dh_channelizer_push(cz._h, None, 100, ctx.mem.ptr(cz.rows), 300, C.byref(n_out)) == -1
    assert lib.dh_channelizer_push(cz._h, ctx.mem.ptr(xp), 100, None, 300, C.byref(n_out)) == -1
    assert lib.dh_channelizer_push(cz._h, ctx.mem.ptr(xp), 100, ctx.mem.ptr(cz.rows), 300, None) == -1
    assert lib.dh_channelizer_push(None, ctx.mem.ptr(xp), 100, ctx.mem.ptr(cz.rows), 300, C.byref(n_out)) == -1
    assert lib.dh_channelizer_retune(cz._h, 4, 0) == -1 and lib.dh_channelizer_retune(None, 0, 0) == -1
    assert lib.dh_channelizer_reset(None) == -1
    assert lib.dh_channelizer_phasor(None, None, 3) == -1
    assert lib.dh_channelizer_push(cz._h, ctx.mem.ptr(xp), 3, None, 0, C.byref(n_out)) == 0 and n_out.value == 0   # no output
    assert lib.dh_channelizer_push(cz._h, None, 0, None, 0, C.byref(n_out)) == 0 and n_out.value == 0
    cz.close()
    with pytest.raises(DhError):
        api.Channelizer(1.0, 2000, [0.0], h, ctx=ctx)


def test_end_to_end_small(emu_ctx, oracle):
    """The harness's scene, its noise of seed 7 from the generator of the device that sums the carriers -> channelizer
    (FM + DC) -> DMR / YSF engines == oracle.chain on the channelizer's rows."""
    end_to_end(emu_ctx, oracle, fixed(16), end_to_end_fixture(1, 16, 8, 1.5, "cpu", seed=7))


@pytest.mark.gpu
def test_end_to_end_wideband_gpu(gpu_ctx, oracle):
    end_to_end(gpu_ctx, oracle, fixed(50), end_to_end_fixture(1, 50, 32, 4.0, "cuda", seed=7))
