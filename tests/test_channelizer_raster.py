"""dh_channelizer on a uniform raster: one polyphase fold + a K-point DFT on the GEMM tile (channelizer_core.hpp, "Uniform
raster").

Both tiers through the `ctx` fixture (the CPU emulation of the kernel bodies, and the gfx950 library on -m gpu):
  * byte-for-byte equality with tests/cz_raster_restate.c, a literal triple loop written from the specification's text;
  * streaming: ragged pushes, retune, reset, block power / gate / counts against tests/cz_power_restate.c;
  * the mathematics in float64 and the existing fixed-offset bank, within a derived bound;
  * argument validation, the older struct size;
  * end to end: a CS16 composite -> Channelizer(raster_hz=...) FM + DC -> DMR / YSF engines, equal to the oracle.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cz_harness import (HERE, bins_for, cfg, create, end_to_end, end_to_end_fixture, host, make_cz, make_input, out_pushes, raster,
                        restate, run_lib, taps_for)      # noqa: F401  (fixture)
from digiham_amd import _capi, api


# (format, output, dcblock, K, D, T, B)
EXACT_CASES = [("cs16", "iq", False, 2, 1, 1, 2),           # smallest everything
               ("cf32", "fm", False, 24, 7, 101, 17),       # K' > K, T no multiple of K, D coprime to K
               ("cs16", "fm", True, 16, 50, 130, 70),       # D > K, two column tiles
               ("cf32", "iq", False, 40, 16, 37, 9),        # T < K: P = 1
               ("cs16", "iq", False, 64, 16, 500, 64),
               # the fold kernel's other paths: K' > 256 (two r blocks per tile) with the taps staged in two chunks of p, and
               # D > 392, where the input span of a tile's sixteen instants no longer fits LDS
               ("cf32", "fm", True, 272, 300, 2400, 5),
               ("cs16", "iq", False, 24, 400, 101, 6)]


@pytest.mark.parametrize("fmt,output,dc,K,D,T,B", EXACT_CASES)
def test_bit_exact_against_restatement(ctx, restate, fmt, output, dc, K, D, T, B):
    x = make_input(fmt, 310 * D + 3, K + D + T)             # >= 300 outputs: two full 128-row tiles and a partial one
    h = taps_for(T)
    bins = bins_for(B, K, B)
    got = run_lib(ctx, raster(K, D), x, fmt, h, bins, output, dc)
    ref = restate.run(raster(K, D), x, fmt == "cf32", h, bins, output == "fm", dc)
    assert got.shape == ref.shape and got.shape[1] >= 300
    assert got.tobytes() == ref.tobytes()


def test_subnormal_operands_bit_exact(ctx, restate):
    """Tiny CF32 input and taps: fold sums, DFT sums and rotations land in the subnormal range and are kept (IEEE)."""
    K, D, T, B = 24, 7, 50, 12
    x = make_input("cf32", 310 * D, 5, scale=1e-36)
    x[::7] = 0.0
    h = taps_for(T, 1e-3)
    bins = bins_for(B, K, 4)
    for output, dc in (("iq", False), ("fm", True)):
        got = run_lib(ctx, raster(K, D), x, "cf32", h, bins, output, dc)
        ref = restate.run(raster(K, D), x, True, h, bins, output == "fm", dc)
        if output == "iq":
            assert (np.abs(ref[ref != 0]) < 1.1754944e-38).any(), "the case must reach subnormal outputs"
        assert got.tobytes() == ref.tobytes()


@pytest.fixture(scope="module")
def slab_rows(tmp_path_factory):
    """K -> (DH_CZ_FOLD_SLAB_BYTES, dh_cz_fold_slab_rows(K')) as the implementation's header has them: tests/host_cpp/
    raster_slab_rows.cpp, compiled over channelizer_core.hpp, prints the two."""
    exe = str(tmp_path_factory.mktemp("czslab") / "raster_slab_rows")
    subprocess.run(["g++", "-std=c++17", "-O0", "-Wno-unknown-pragmas", "-Wno-unused-function",
                    os.path.join(HERE, "host_cpp", "raster_slab_rows.cpp"), "-o", exe], check=True)
    return lambda K: tuple(int(v) for v in subprocess.run([exe, str(K)], check=True, stdout=subprocess.PIPE).stdout.split())


def test_push_longer_than_a_fold_slab(ctx, restate, slab_rows):
    """D = 1, K = 16: a fold slab holds dh_cz_fold_slab_rows(16) output instants -- the number comes from the implementation's
    header, so the push grows with the constant -- and the push some 8 000 more: two slabs, the second one starting inside
    the push, with its own row offset in the rotation and in the output rows."""
    K, D, T, B = 16, 1, 40, 2
    slab_bytes, rows = slab_rows(K)
    assert slab_bytes <= 32 << 20 and rows % 128 == 0 and 128 <= rows <= slab_bytes // (8 * 16)     # the issue's limits on a slab
    n = rows + 7877
    x = make_input("cs16", n, 11)
    h = taps_for(T)
    bins = [5, -3]
    got = run_lib(ctx, raster(K, D), x, "cs16", h, bins, "iq", False)
    ref = restate.run(raster(K, D), x, False, h, bins, False, False)
    assert got.shape == ref.shape == (B, n, 2)
    assert got.tobytes() == ref.tobytes()


def test_streaming_pushes_retune_reset_power(ctx, restate):
    K, D, T, B, n = 24, 7, 101, 17, 4000
    bank = raster(K, D)
    x = make_input("cf32", n, 9, scale=0.3)
    h = taps_for(T)
    bins = bins_for(B, K, 2)
    whole = run_lib(ctx, bank, x, "cf32", h, bins, "fm", True)
    pushes = [0, 1, D - 1, D, 7 * D + 3, 0, 2500, 5]
    pushes.append(n - sum(pushes))
    ragged = run_lib(ctx, bank, x, "cf32", h, bins, "fm", True, pushes=pushes)
    assert ragged.tobytes() == whole.tobytes()
    assert whole.tobytes() == restate.run(bank, x, True, h, bins, True, True).tobytes()
    # a retune of two channels mid-stream (push 6), then one more at push 8
    ret = {6: {3: 5, 11: -7}, 8: {3: K // 2 + 3 * K}}
    got = run_lib(ctx, bank, x, "cf32", h, bins, "fm", True, pushes=pushes, retunes=ret)
    ref = restate.run(bank, x, True, h, bins, True, True, pushes=pushes, retunes=ret)
    assert got.tobytes() == ref.tobytes() and got.tobytes() != whole.tobytes()
    # reset: a fresh stream
    cz = make_cz(ctx, bank, "cf32", h, bins, "fm", True, n)
    first = run_lib(ctx, bank, x[:3000], "cf32", h, bins, "fm", True, pushes=[1000, 2000], cz=cz)
    cz.reset()
    again = run_lib(ctx, bank, x, "cf32", h, bins, "fm", True, pushes=[n], cz=cz)
    cz.close()
    assert again.tobytes() == whole.tobytes()
    assert first.tobytes() == whole[:, :first.shape[1]].tobytes()
    # block power, gate and counts of the ragged stream == cz_power_restate.c fed with the restatement's z rows
    L, levels = 7, (0.06, 0.04, 1)
    _, z = restate.run(bank, x, True, h, bins, True, True, want_z=True)
    pw_ref, gate_ref, counts_ref = restate.power(z, L, *levels, out_pushes(pushes, D))
    assert 0 < gate_ref.mean() < 1 and (counts_ref == 0).any() and (counts_ref != 0).any(), "the levels must toggle the gates"
    got = run_lib(ctx, bank, x, "cf32", h, bins, "fm", True, pushes=pushes, power=(L, levels), keep_rows=False)
    assert got["power"].tobytes() == pw_ref.tobytes()
    assert got["gate"].tobytes() == gate_ref.tobytes()
    assert got["counts"].tobytes() == counts_ref.tobytes()


# ---- against the mathematics and against the existing bank -------------------------------------------------------------
def model_rows(x, h, K, D, bins):
    """float64: y_c[j] = e^{-2 pi i c n_j / K} sum_{r<K} e^{+2 pi i c r / K} sum_p h[r + p K] x[n_j - r - p K], x[n < 0] = 0."""
    xs = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    P = -(-len(h) // K)
    hp = np.zeros(P * K)
    hp[:len(h)] = h
    n_out = len(xs) // D
    nj = np.arange(n_out) * D + D - 1
    pad = np.concatenate([np.zeros(P * K, complex), xs])
    r = np.arange(K)
    v = np.zeros((n_out, K), complex)
    for p in range(P):
        v += hp[r + p * K][None, :] * pad[P * K + nj[:, None] - r[None, :] - p * K]
    c = np.mod(np.array(bins), K)
    return (np.exp(-2j * np.pi * np.outer(c, nj % K) / K) * (np.exp(2j * np.pi * np.outer(c, r) / K) @ v.T))


def test_against_float64_and_fixed_offset_bank(ctx):
    """K = 64, D = 16 at 768 kS/s on a 12 kHz raster; the increments c 2^26 of the fixed-offset bank are exact, so both modes
    compute the same quantity.

    The bound, derived (not measured).  Each component of y is a sum of products h[k] x[.] g with |g| <= 1 over all
    k = r + p K, so its magnitude sum is at most S = sum|h| max|x| (|x| the modulus of a complex sample; a component of
    x g is at most |x|).  A term passes through the fold chain (P fused steps), the DFT chain (two fused steps per r:
    2 K' in all) and the rotation (a product and a sum per component; with the roundings of the four table products of a
    phasor and of the conversion to the result, 8 more), so by Higham's bound for recursive summation the rounding error
    of a component is at most gamma_(2 K' + P + 8) S ~ (2 K' + P + 8) 2^-24 S.  The two phasors that multiply a term
    (G and the rotation) are each within the tested 1e-6 of the exact exponentials: 2e-6 S.  Two components: sqrt(2).
      E_r = ((2 K' + P + 8) 2^-24 + 2e-6) sqrt(2) sum|h| max|x|
    and for the fixed-offset bank, whose single chain has 2 T' steps, E_d is the same with 2 T' in place of 2 K' + P."""
    rate, D, K = 768000.0, 16, 64
    h = api.channel_taps(rate, D, 5500.0, 8000.0, 60.0)
    T = len(h)
    Tp, Kp, P = 16 * ((T + 15) // 16), 16 * ((K + 15) // 16), -(-T // K)
    bins = [0, 8, -19, 26]
    freqs = [c * rate / K for c in bins]
    assert all(api.nco_increment(f, rate) == (c << 26) & 0xFFFFFFFF for f, c in zip(freqs, bins))
    n, A = 8000, 0.5
    nn = np.arange(n, dtype=np.float64)
    sum_h = float(np.abs(h.astype(np.float64)).sum())
    H = lambda d: np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * d / rate * np.arange(T)))
    inputs = []
    for b, f in enumerate(freqs):
        for delta, stop in ((1234.5, False), (-4000.0, False), (15000.0, True), (-40000.0, True)):
            xs = A * np.exp(2j * np.pi * (f + delta) / rate * nn)
            inputs.append((np.stack([xs.real, xs.imag], 1).astype(np.float32), b, delta, stop))
    inputs.append((make_input("cf32", n, 3, scale=0.3), None, None, False))
    ras = api.Channelizer(rate, D, freqs, h, input="cf32", output="iq", max_input=n, ctx=ctx, raster_hz=rate / K)
    fix = api.Channelizer(rate, D, freqs, h, input="cf32", output="iq", max_input=n, ctx=ctx)
    cplx = lambda rows, k: host(ctx, rows)[:, :k, 0].astype(np.float64) + 1j * host(ctx, rows)[:, :k, 1]
    for x, b, delta, stop in inputs:
        xmax = float(np.abs(x[:, 0].astype(np.float64) + 1j * x[:, 1]).max())
        E_r = ((2 * Kp + P + 8) * 2.0 ** -24 + 2e-6) * np.sqrt(2.0) * sum_h * xmax
        E_d = ((2 * Tp + 8) * 2.0 ** -24 + 2e-6) * np.sqrt(2.0) * sum_h * xmax
        ras.reset(); fix.reset()
        zr = cplx(*ras.push(x))
        zf = cplx(*fix.push(x))
        want = model_rows(x, h, K, D, bins)
        err_m, err_f = np.abs(zr - want).max(), np.abs(zr - zf).max()
        print("bin %s delta %s: |raster - float64| %.3g (E_r %.3g), |raster - fixed| %.3g (E_r + E_d %.3g)"
              % (b, delta, err_m, E_r, err_f, E_r + E_d))
        assert err_m <= E_r, (b, delta, err_m, E_r)
        assert err_f <= E_r + E_d, (b, delta, err_f, E_r + E_d)
        if b is None:
            continue
        nj = np.arange(zr.shape[1]) * D + D - 1
        ok = nj >= P * K
        if not stop:                  # the float64 model is the tone through H, as test_ddc_physics has it
            tone = H(delta) * A * np.exp(2j * np.pi * delta * nj / rate)
            assert np.abs(zr[b] - tone)[ok].max() <= E_r + 2.0 ** -24 * np.sqrt(2.0) * sum_h * A      # (+ the input's own rounding)
        else:
            assert np.abs(zr[b][ok]).max() <= abs(H(delta)) * A + E_r
            assert np.abs(zr[b][ok]).max() <= 1.2e-3 * A
    ras.close(); fix.close()
    # FM of an offset tone: 2 delta / rate_out in the steady state
    delta = 2100.0
    xs = A * np.exp(2j * np.pi * (freqs[1] + delta) / rate * nn)
    x = np.stack([xs.real, xs.imag], 1).astype(np.float32)
    cz = api.Channelizer(rate, D, freqs[1:2], h, input="cf32", output="fm", dcblock=False, max_input=n, ctx=ctx, raster_hz=rate / K)
    rows, k = cz.push(x)
    fm = host(ctx, rows)[0, :k].astype(np.float64)
    cz.close()
    assert np.abs(fm[P * K // D + 2:] - 2 * delta / (rate / D)).max() <= 1e-6


# ---- validation -------------------------------------------------------------------------------------------------------
def test_validation(ctx):
    lib = ctx.lib
    h = np.ones(8, np.float32)
    bins = np.array([0, 1, -1, 5], np.int32)
    big = np.ones(64 * 2 + 1, np.float32)
    rcfg = lambda **kw: cfg(ctx, **dict(dict(interpolation=1, raster=8, bins=bins), **kw))
    rcreate = lambda **kw: create(ctx, rcfg(**kw))
    assert rcreate() == 0
    bad = [dict(raster=1), dict(raster=16385), dict(bins=C.POINTER(C.c_int32)()), dict(interpolation=3),
           dict(raster=2, n_taps=129, taps=big)]                                          # T > 64 K
    for kw in bad:
        assert rcreate(**kw) == -1, kw
    assert rcreate(raster=2, n_taps=128, taps=big) == 0
    assert rcreate(increments=C.POINTER(C.c_uint32)()) == 0                               # ignored on a raster
    assert rcreate(raster=0, increments=C.POINTER(C.c_uint32)()) == -1                   # ... and only there
    # the older struct ended with interpolation, and its size -- what its callers pass -- covers the tail padding behind it,
    # where raster sits now (72 bytes, raster at 68, with 8-byte pointers).  Such a caller never wrote those bytes: 0xA5 in
    # them, and behind them, is not read.  The same goes for every size below the whole struct: raster is read only together
    # with bins.
    v2, full = _capi.CHANNELIZER_CONFIG_V2_SIZE, C.sizeof(_capi.ChannelizerConfig)
    r_off, b_off = _capi.ChannelizerConfig.raster.offset, _capi.ChannelizerConfig.bins.offset
    assert r_off < v2 < full, "the older size must cover raster for this case to mean anything"
    x = make_input("cs16", 400, 1)
    xp = ctx.mem.from_numpy(x)
    cz = api.Channelizer(1.0, 4, [0.0] * 4, h, max_input=1000, ctx=ctx)                   # the fixed-offset bank it must be
    r2, k = cz.push(x)
    want = host(ctx, r2)[:, :k].tobytes()
    cz.close()
    for size in sorted({v2, r_off, b_off, full - 1}):
        old = rcfg(struct_size=size)
        C.memset(C.byref(old, r_off), 0xA5, full - r_off)
        hh = C.c_void_p()
        assert lib.dh_channelizer_create(C.byref(old), C.byref(hh)) == 0, size
        rows = ctx.mem.zeros((4, 101), np.float32)
        n_out = C.c_size_t(0)
        assert lib.dh_channelizer_push(hh, ctx.mem.ptr(xp), 400, ctx.mem.ptr(rows), 101, C.byref(n_out)) == 0 and n_out.value == 100
        got = host(ctx, rows)[:, :100].copy()
        lib.dh_channelizer_destroy(hh)
        assert got.tobytes() == want, size
    # retune, and the Python side's raster rules
    cz = api.Channelizer(96000.0, 4, [0.0, 12000.0, -24000.0], h, max_input=100, ctx=ctx, raster_hz=12000.0)
    assert lib.dh_channelizer_retune(cz._h, 3, 0) == -1 and lib.dh_channelizer_retune(cz._h, 2, 0xFFFFFFFF) == 0
    cz.retune(0, -36000.0)
    with pytest.raises(ValueError, match="channel 1"):
        cz.retune(1, 12500.0)
    cz.close()
    with pytest.raises(ValueError, match="channel 2"):
        api.Channelizer(96000.0, 4, [0.0, 12000.0, 12001.0], h, ctx=ctx, raster_hz=12000.0)
    with pytest.raises(ValueError, match="no integer"):
        api.Channelizer(96000.0, 4, [0.0], h, ctx=ctx, raster_hz=12500.0)
    for k_bad in (1, 16385):
        with pytest.raises(ValueError, match="outside 2 .. 16384"):
            api.Channelizer(float(k_bad), 4, [0.0], h, ctx=ctx, raster_hz=1.0)
    assert list(api.raster_bins([0.0, -25000.0, 1.2e6], 2.4e6, 12500.0)) == [0, -2, 96]


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_end_to_end_small(emu_ctx, oracle):
    """768 kS/s, 12 kHz raster (K = 64), 8 rows, 1.5 s."""
    end_to_end(emu_ctx, oracle, raster(64, 16), end_to_end_fixture(1, 16, 8, 1.5, "cpu", seed=7, raster_hz=12000.0, noise_device="cpu"))


@pytest.mark.gpu
def test_end_to_end_raster_gpu(gpu_ctx, oracle):
    """2.4 MS/s, 12.5 kHz raster (K = 192), 32 rows, 4 s; the carriers are summed on the device, the noise is the CPU
    generator's of seed 7.  The fixture is one that a float64 model of fold + DFT decodes on every row.  Run on the device,
    where the tool builds this very composite (carriers summed there, CPU noise),
    `tools/channelizer_model.py --raster 12500 --decimation 50 --rows 32 --seconds 4 --seed 7 --device cuda` ends with
    "raster 12500 Hz, D 50, 32 rows, 4 s: seed 7, cpu noise: the model decodes every row; the library does too; counts agree".
    The seed was picked where there is no device, with `--device cpu` (carriers summed on the CPU as well), which ends with
    "raster 12500 Hz, D 50, 32 rows, 4 s: seed 7, cpu noise: the model decodes every row" (seed 8 does too).  (The device
    generator's noise of seed 7 is the one DESIGN.md section 4.6 found a false LC decode in; it is not used here.)"""
    end_to_end(gpu_ctx, oracle, raster(192, 50), end_to_end_fixture(1, 50, 32, 4.0, "cuda", seed=7, raster_hz=12500.0, noise_device="cpu"))
