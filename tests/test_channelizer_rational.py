"""dh_channelizer at rational rates: rows at input_rate * L / M (digiham_amd/csrc/channelizer_core.hpp, "Rational rates").

Both tiers through the `ctx` fixture unless a test says otherwise:
  * byte-for-byte equality with tests/cz_rational_restate.c, the literal zero-stuffed restatement of the written text;
  * L = 1 (and 0) is the integer channelizer: the bytes of tests/cz_restate.c;
  * streaming: ragged pushes, retunes, reset; subnormal operands;
  * physics in float64: every phase's gain and phase in the passband, the stopband, FM of a tone;
  * block power, gate and counts against tests/cz_power_restate.c on the rational restatement's z rows;
  * argument validation and api.resample_ratio;
  * end to end: a composite at a rate that is no multiple of 48 kS/s -> channelizer (FM + DC) -> engines == the oracle.
"""
import ctypes as C
from math import gcd

import numpy as np
import pytest

from cz_harness import (cfg, create, end_to_end, end_to_end_fixture, fixed, incs_for, make_cz, make_input, out_pushes, rational,
                        restate, run_lib, taps_for)      # noqa: F401  (fixture)
from digiham_amd import _capi, api
from digiham_amd._capi import DhError


# ---------------------------------------------------------------------------------------------------------------- 1. bit-exact
# (format, output, dcblock, L, M, T, B): 2/3 -- more than 128 rows per phase; 5/6 -- B across the 64-channel tile, a ratio
# near 1; 24/125 -- few rows per phase, many phases, unequal tap counts; 7/9 with T = 5 -- all-zero phases
EXACT_CASES = [("cs16", "iq", False, 2, 3, 13, 3), ("cf32", "fm", False, 3, 8, 50, 17), ("cs16", "fm", True, 3, 128, 401, 20),
               ("cf32", "iq", False, 24, 125, 700, 9), ("cs16", "fm", True, 5, 6, 130, 70), ("cf32", "iq", False, 7, 9, 5, 4)]


@pytest.mark.parametrize("fmt,output,dc,L,M,T,B", EXACT_CASES)
def test_bit_exact_against_restatement(ctx, restate, fmt, output, dc, L, M, T, B):
    assert gcd(L, M) == 1
    n = 1500 + 3 * M
    x = make_input(fmt, n, M + T)
    h = taps_for(T)
    incs = incs_for(B, B)
    got = run_lib(ctx, rational(L, M), x, fmt, h, incs, output, dc)
    ref = restate.run(rational(L, M), x, fmt == "cf32", h, incs, output == "fm", dc)
    assert got.shape[1] == L * n // M
    assert got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------------------------------- 2. L = 1
@pytest.mark.parametrize("interp", [1, 0])
def test_interpolation_one_is_the_integer_channelizer(ctx, restate, interp):
    fmt, output, dc, D, T, B = "cs16", "fm", True, 16, 70, 20           # an exact case of test_channelizer.py
    x = make_input(fmt, 1500 + 3 * D, D + T)
    h = taps_for(T)
    incs = incs_for(B, B)
    got = run_lib(ctx, rational(interp, D), x, fmt, h, incs, output, dc)
    ref = restate.run(fixed(D), x, False, h, incs, True, dc)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


# --------------------------------------------------------------------------------------------------------------- 3. streaming
def test_streaming_pushes_retune_reset(ctx, restate):
    L, M, T, B = 3, 8, 45, 19
    bank = rational(L, M)
    x = make_input("cs16", 4000, 9)
    h = taps_for(T, seed=1)
    incs = incs_for(B, 2)
    whole = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True)
    pushes = [0, 1, 2, 3, 7, 8 * 7 + 3, 0, 2500, 5]
    pushes.append(4000 - sum(pushes))
    ragged = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True, pushes=pushes)
    assert ragged.tobytes() == whole.tobytes()
    assert whole.tobytes() == restate.run(bank, x, False, h, incs, True, True).tobytes()
    ret = {6: {3: 0x12345678, 11: 0}, 8: {3: 0xFEDCBA98}}
    got = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True, pushes=pushes, retunes=ret)
    ref = restate.run(bank, x, False, h, incs, True, True, pushes=pushes, retunes=ret)
    assert got.tobytes() == ref.tobytes() and got.tobytes() != whole.tobytes()
    cz = make_cz(ctx, bank, "cs16", h, incs, "fm", True, 4000)
    first = run_lib(ctx, bank, x[:3000], "cs16", h, incs, "fm", True, pushes=[1000, 2000], cz=cz)
    cz.reset()
    again = run_lib(ctx, bank, x, "cs16", h, incs, "fm", True, pushes=[4000], cz=cz)
    cz.close()
    assert again.tobytes() == whole.tobytes()
    assert first.tobytes() == whole[:, :first.shape[1]].tobytes()


# -------------------------------------------------------------------------------------------------------------- 4. subnormals
def test_subnormal_operands_bit_exact(ctx, restate):
    """The subnormal case of test_channelizer.py at L / M = 3 / 7."""
    x = make_input("cf32", 600, 5, scale=1e-36)
    x[::7] = 0.0
    h = taps_for(21, 1e-3, seed=3)
    incs = incs_for(12, 4)
    for output, dc in (("iq", False), ("fm", True)):
        got = run_lib(ctx, rational(3, 7), x, "cf32", h, incs, output, dc)
        ref = restate.run(rational(3, 7), x, True, h, incs, output == "fm", dc)
        if output == "iq":
            assert (np.abs(ref[ref != 0]) < 1.1754944e-38).any(), "the case must reach subnormal outputs"
        assert got.tobytes() == ref.tobytes()


# ----------------------------------------------------------------------------------------------------------------- 5. physics
def test_rational_ddc_physics(ctx):
    """L / M = 3 / 50 at 800 kS/s.  Output j of phase p = j mod L is the input through h_p[k] = h[r_p + k L], so a tone at
    delta from the channel centre gives z[j] = A H_p(delta) e^(2 pi i delta n_j / rate), H_p(delta) = sum_k h_p[k] e^(-2 pi i
    delta k / rate).  Bounds: 1e-5 sum|h_p| A in the passband (the bound of test_ddc_physics); in the stopband the prototype's
    own |H|: by the polyphase identity H_p(delta) = (1 / L) sum_m H(delta + m rate) e^(...), H the prototype's response at the
    virtual rate, so |H_p| <= (1 / L) sum_m |H(delta + m rate)|.  FM: n_j advances unevenly (16, 17, 17 samples), and the
    phases' fractional delays r_p / L make up for it: with Hv_p = H_p e^(-2 pi i delta r_p / (L rate)), H_p referred to the
    virtual index v_j = L n_j + r_p, z[j] = A Hv_p e^(2 pi i delta v_j / (L rate)) and v_j advances by M: the discriminator
    gives 2 delta M / (L rate) = 2 delta / 48000 plus arg(Hv_p / Hv_p') / pi, and two numbers within eps |mean| of their mean
    differ in angle by at most 2 asin(eps) = 2 eps (1 + O(eps^2)); eps ~ 1e-3, the cubic term ~ 1e-10."""
    rate, L, M = 800000.0, 3, 50
    h = api.channel_taps(rate, M, 6500.0, 12000.0, 60.0, interpolation=L)
    h64 = h.astype(np.float64)
    T = len(h)
    Tp = 16 * ((-(-T // L) + 15) // 16)
    rp = [(p * M + M - 1) % L for p in range(L)]
    hp = [h64[r::L] for r in rp]
    stop = 10 ** (-60 / 20) * 1.2
    for p in range(L):
        assert abs(hp[p].sum() - 1.0) <= stop, (p, hp[p].sum())
    Hp = lambda p, d: np.sum(hp[p] * np.exp(-2j * np.pi * d / rate * np.arange(len(hp[p]))))
    Hv = lambda f: np.sum(h64 * np.exp(-2j * np.pi * f / (L * rate) * np.arange(T)))
    freqs = [0.0, 100000.0, -237500.0, 312500.0]
    incs = [api.nco_increment(f, rate) for f in freqs]
    n = 8000
    nn = np.arange(n, dtype=np.float64)
    A = 0.5
    j = np.arange(L * n // M)
    nj = (j * M + M - 1) // L
    ph = j % L
    ok = nj >= Tp
    fgrid = np.linspace(12000.0, L * rate / 2, 4000)
    assert max(abs(Hv(f)) for f in fgrid) / L <= stop
    for b, u in enumerate(incs):
        for delta, stopband in ((1234.5, False), (-4000.0, False), (15000.0, True), (-40000.0, True)):
            xs = A * np.exp(2j * np.pi * ((u / 2.0 ** 32) + delta / rate) * nn)
            x = np.stack([xs.real, xs.imag], 1).astype(np.float32)
            z = run_lib(ctx, rational(L, M), x, "cf32", h, [u], "iq", False, rate=rate)[0]
            z = z[:, 0].astype(np.float64) + 1j * z[:, 1]
            assert len(z) == len(j)
            for p in range(L):
                sel = ok & (ph == p)
                bound = 1e-5 * np.abs(hp[p]).sum() * A
                if not stopband:
                    want = Hp(p, delta) * A * np.exp(2j * np.pi * delta * nj / rate)
                    err = np.abs(z - want)[sel].max()
                    assert err <= bound, (freqs[b], delta, p, err)
                else:
                    proto = sum(abs(Hv(delta + m * rate)) for m in range(L)) / L
                    assert np.abs(z[sel]).max() <= proto * A + bound, (freqs[b], delta, p)
                    assert np.abs(z[sel]).max() <= 1.2e-3 * A
    delta = 2100.0
    hv = np.array([Hp(p, delta) * np.exp(-2j * np.pi * delta * rp[p] / (L * rate)) for p in range(L)])
    tol = (2 / np.pi) * np.abs(hv - hv.mean()).max() / abs(hv.mean()) + 1e-6
    print("FM tolerance %.3g" % tol)
    xs = A * np.exp(2j * np.pi * ((incs[1] / 2.0 ** 32) + delta / rate) * nn)
    x = np.stack([xs.real, xs.imag], 1).astype(np.float32)
    fm = run_lib(ctx, rational(L, M), x, "cf32", h, [incs[1]], "fm", False, rate=rate)[0].astype(np.float64)
    first = int(np.argmax(ok)) + 2
    dev = np.abs(fm[first:] - 2 * delta / 48000.0).max()
    print("FM deviation %.3g" % dev)
    assert dev <= tol


# ---------------------------------------------------------------------------------------------------------- 6. power and counts
def test_power_gate_counts(ctx, restate):
    L, M, block, B = 3, 8, 16, 5
    bank = rational(L, M)
    n = 4000
    incs = [0x60000000] + incs_for(B - 1, 6)
    rng = np.random.default_rng(8)
    t = np.arange(n)
    tone = 0.5 * np.exp(2j * np.pi * (incs[0] / 2.0 ** 32) * t) * ((t >= 1000) & (t < 2600))       # keyed
    xs = tone + 0.003 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.round(np.stack([xs.real, xs.imag], 1) * 32767).astype(np.int16)
    h = (np.hanning(98)[1:-1] * 3 / np.hanning(98).sum()).astype(np.float32)                        # every phase sums to ~1
    pushes = [300, 0, 5, 1200, 37, 900, 800, 2]
    pushes.append(n - sum(pushes))
    op = out_pushes(pushes, M, L)
    levels = (np.float32(0.05), np.float32(0.02), 1)
    z = restate.run(bank, x, False, h, incs, False, False)
    pw_ref, gate_ref, counts_ref = restate.power(z, block, *levels, op)
    assert gate_ref[0].any() and not gate_ref[0].all() and not gate_ref[1:].any(), "the fixture must key channel 0 only"
    for output, dc in (("iq", False), ("fm", True)):
        got = run_lib(ctx, bank, x, "cs16", h, incs, output, dc, pushes=pushes, power=(block, levels), keep_rows=False)
        assert got["power"].shape == pw_ref.shape and got["power"].tobytes() == pw_ref.tobytes(), output
        assert got["gate"].tobytes() == gate_ref.tobytes(), output
        assert got["counts"].tobytes() == counts_ref.tobytes(), output
        for s in range(len(pushes)):
            assert set(got["counts"][s].tolist()) <= {0, op[s]}
    # the stride of the enable: (max_input L / M + 1) / block + 1
    cz = make_cz(ctx, bank, "cs16", h, incs, "iq", False, 4000)
    mem = ctx.mem
    need = (4000 * L // M + 1) // block + 1
    assert need > (4000 // M + 1) // block + 1
    power, gate, counts = mem.zeros((B, need), np.float32), mem.zeros((B, need), np.uint8), mem.zeros((B,), np.uint32)
    for stride, rc in ((need - 1, _capi.DH_EINVAL), (need, 0)):
        pcfg = _capi.ChannelizerPowerConfig(C.sizeof(_capi.ChannelizerPowerConfig), block, 0.0, 0.0, 0, mem.ptr(power), mem.ptr(gate),
                                           mem.ptr(counts), stride)
        assert ctx.lib.dh_channelizer_power_enable(cz._h, C.byref(pcfg)) == rc, stride
    cz.close()


# -------------------------------------------------------------------------------------------------------------- 7. validation
def test_validation(ctx):
    rcreate = lambda L, M, T, **kw: create(ctx, cfg(ctx, interpolation=L, decimation=M, n_taps=T, taps=np.ones(T, np.float32), **kw))
    assert rcreate(65, 128, 8) == _capi.DH_EINVAL
    assert rcreate(5, 3, 8) == _capi.DH_EINVAL                          # L > M
    assert rcreate(4, 6, 8) == _capi.DH_EINVAL                          # gcd 2
    assert rcreate(3, 8, 16384 * 3 + 1) == _capi.DH_EINVAL
    assert rcreate(3, 8, 16384 * 3) == 0
    assert rcreate(64, 1023, 8) == 0
    old = _capi.ChannelizerConfig.interpolation.offset                 # a caller built before the field existed
    assert rcreate(65, 128, 8, struct_size=old) == 0
    assert rcreate(1, 8, 16385) == _capi.DH_EINVAL
    with pytest.raises(DhError):
        api.Channelizer(1.0, 8, [0.0], np.ones(8, np.float32), ctx=ctx, interpolation=6)
    assert api.resample_ratio(2.048e6) == (3, 128)
    assert api.resample_ratio(2.4e6) == (1, 50)
    assert api.resample_ratio(250e3) == (24, 125)
    with pytest.raises(ValueError):
        api.resample_ratio(20e6)                                       # 3 / 1250
    with pytest.raises(ValueError):
        api.channel_taps(800000.0, 50, 6500.0, 50000.0, 60.0, interpolation=3)      # the stopband edge is beyond 48 kS/s
    assert abs(float(api.channel_taps(800000.0, 50, 6500.0, 12000.0, 60.0, interpolation=3).sum()) - 3.0) < 1e-4


# -------------------------------------------------------------------------------------------------------------- 8. end to end
def test_end_to_end_small(emu_ctx, oracle):
    """The scene of test_channelizer.py at the capture rate 48 kS/s * M / L."""
    end_to_end(emu_ctx, oracle, rational(3, 50), end_to_end_fixture(3, 50, 8, 1.5, "cpu", seed=7))


@pytest.mark.gpu
def test_end_to_end_wideband_gpu(gpu_ctx, oracle):
    """2.048 MS/s, 32 rows, 4 s, composite built on the device, noise seed 8.  The fixture has to be one that a float64
    model of the channelizer decodes on every row; tools/channelizer_model.py --seed 8 is that check (not yet run on the
    device: the library passes this test with seed 8, the model's own run is outstanding).  With the device's noise of seed 7 the model itself, like
    the library, decodes a sixth LC with wrong ids in row 10 (-16.5 dB): a false decode that 2 LSB of noise tip either way
    (the CPU generator's noise of seed 7 gives five, all right), not a property of the channelizer."""
    end_to_end(gpu_ctx, oracle, rational(3, 128), end_to_end_fixture(3, 128, 32, 4.0, "cuda", seed=8))
