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

from digiham_amd import _capi, api, wideband

HERE = os.path.dirname(os.path.abspath(__file__))


class Restate:
    def __init__(self, d):
        libs = []
        for name in ("cz_raster_restate", "cz_power_restate"):
            so = str(d / ("lib%s.so" % name))
            subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(HERE, name + ".c"),
                            "-o", so, "-lm"], check=True)
            libs.append(C.CDLL(so))
        self.cz, self.pw = libs
        self.cz.cz_raster_restate.restype = None
        self.cz.cz_raster_restate.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self.pw.cz_power_restate.restype = None
        self.pw.cz_power_restate.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(self, x, cf32, D, h, K, bins, fm, dcblock, pushes=None, retunes=None, want_z=False):
        """bins: [B] at the start; pushes: the push lengths (for retunes); retunes: {push index: {ch: bin}}."""
        x = np.ascontiguousarray(x)
        n = x.size // 2
        B = len(bins)
        pushes = pushes or [n]
        starts = np.cumsum([0] + list(pushes[:-1])).astype(np.uint64)
        nseg = len(pushes)
        bn = np.zeros((nseg, B), np.int32)
        reset = np.zeros((nseg, B), np.uint8)
        cur = np.array(bins, np.int32)
        for s in range(nseg):
            for ch, c in (retunes or {}).get(s, {}).items():
                cur[ch] = c
                reset[s, ch] = 1
            bn[s] = cur
        h = np.ascontiguousarray(h, np.float32)
        n_out = n // D
        out = np.zeros((B, n_out) if fm else (B, n_out, 2), np.float32)
        z = np.zeros((B, n_out, 2), np.float32) if want_z else None
        self.cz.cz_raster_restate(x.ctypes.data, int(cf32), n, D, h.ctypes.data, len(h), K, B, starts.ctypes.data, bn.ctypes.data,
                                  reset.ctypes.data, nseg, int(fm), int(dcblock), out.ctypes.data, z.ctypes.data if want_z else None)
        return (out, z) if want_z else out

    def power(self, z, L, open_level, close_level, hang, out_pushes):
        """-> power [B][n // L] float32, gate [B][n // L] uint8, counts [npush][B] uint32."""
        z = np.ascontiguousarray(z, np.float32)
        B, n = z.shape[0], z.shape[1]
        npush = len(out_pushes)
        per = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (npush,)))
        ol, cl, hg = per(open_level, np.float32), per(close_level, np.float32), per(hang, np.uint32)
        pl = np.array(out_pushes, np.uint64)
        rt = np.zeros((npush, B), np.uint8)
        power, gate = np.zeros((B, n // L), np.float32), np.zeros((B, n // L), np.uint8)
        counts = np.zeros((npush, B), np.uint32)
        self.pw.cz_power_restate(z.ctypes.data, B, n, L, ol.ctypes.data, cl.ctypes.data, hg.ctypes.data, pl.ctypes.data, npush,
                                 rt.ctypes.data, power.ctypes.data, gate.ctypes.data, counts.ctypes.data)
        return power, gate, counts


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return Restate(tmp_path_factory.mktemp("czr"))


def host(ctx, a):
    return np.asarray(ctx.mem.to_numpy(a))


def make_cz(ctx, fmt, D, h, K, bins, output, dc, max_input):
    """input_rate = K and raster_hz = 1: a channel's frequency is its bin, exactly."""
    return api.Channelizer(float(K), D, [float(c) for c in bins], h, input=fmt, output=output, dcblock=dc, max_input=max_input,
                           ctx=ctx, raster_hz=1.0)


def run_lib(ctx, x, fmt, D, h, K, bins, output, dc, pushes=None, retunes=None, cz=None):
    """Push x in the given lengths; returns the concatenated rows."""
    flat = np.ascontiguousarray(x).reshape(-1, 2)
    pushes = pushes or [len(flat)]
    own = cz is None
    if own:
        cz = make_cz(ctx, fmt, D, h, K, bins, output, dc, max(max(pushes), 1))
    parts, pos = [], 0
    for s, c in enumerate(pushes):
        for ch, b in (retunes or {}).get(s, {}).items():
            cz.retune(ch, float(b))
        rows, k = cz.push(np.ascontiguousarray(flat[pos:pos + c]))
        parts.append(host(ctx, rows)[:, :k].copy())
        pos += c
    if own:
        cz.close()
    return np.concatenate(parts, axis=1)


def make_input(fmt, n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    if fmt == "cs16":
        return rng.integers(-30000, 30000, (n, 2)).astype(np.int16)
    return (rng.standard_normal((n, 2)) * scale).astype(np.float32)


def bins_for(B, K, seed):
    """0, K/2, -1, K-1, -K/2 and a duplicate first, then bins from four turns of the raster."""
    edge = [0, K // 2, -1, K - 1, -(K // 2), K // 2]
    extra = [int(v) for v in np.random.default_rng(seed).integers(-2 * K, 2 * K, max(B - len(edge), 0))]
    return (edge + extra)[:B]


def taps_for(T, scale=0.05):
    return np.random.default_rng(T).standard_normal(T).astype(np.float32) * scale


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
    got = run_lib(ctx, x, fmt, D, h, K, bins, output, dc)
    ref = restate.run(x, fmt == "cf32", D, h, K, bins, output == "fm", dc)
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
        got = run_lib(ctx, x, "cf32", D, h, K, bins, output, dc)
        ref = restate.run(x, True, D, h, K, bins, output == "fm", dc)
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
    got = run_lib(ctx, x, "cs16", D, h, K, bins, "iq", False)
    ref = restate.run(x, False, D, h, K, bins, False, False)
    assert got.shape == ref.shape == (B, n, 2)
    assert got.tobytes() == ref.tobytes()


def out_pushes(pushes, D):
    pos, res = 0, []
    for c in pushes:
        res.append((pos + c) // D - pos // D)
        pos += c
    return res


def test_streaming_pushes_retune_reset_power(ctx, restate):
    K, D, T, B, n = 24, 7, 101, 17, 4000
    x = make_input("cf32", n, 9, scale=0.3)
    h = taps_for(T)
    bins = bins_for(B, K, 2)
    whole = run_lib(ctx, x, "cf32", D, h, K, bins, "fm", True)
    pushes = [0, 1, D - 1, D, 7 * D + 3, 0, 2500, 5]
    pushes.append(n - sum(pushes))
    ragged = run_lib(ctx, x, "cf32", D, h, K, bins, "fm", True, pushes=pushes)
    assert ragged.tobytes() == whole.tobytes()
    assert whole.tobytes() == restate.run(x, True, D, h, K, bins, True, True).tobytes()
    # a retune of two channels mid-stream (push 6), then one more at push 8
    ret = {6: {3: 5, 11: -7}, 8: {3: K // 2 + 3 * K}}
    got = run_lib(ctx, x, "cf32", D, h, K, bins, "fm", True, pushes=pushes, retunes=ret)
    ref = restate.run(x, True, D, h, K, bins, True, True, pushes=pushes, retunes=ret)
    assert got.tobytes() == ref.tobytes() and got.tobytes() != whole.tobytes()
    # reset: a fresh stream
    cz = make_cz(ctx, "cf32", D, h, K, bins, "fm", True, n)
    first = run_lib(ctx, x[:3000], "cf32", D, h, K, bins, "fm", True, pushes=[1000, 2000], cz=cz)
    cz.reset()
    again = run_lib(ctx, x, "cf32", D, h, K, bins, "fm", True, pushes=[n], cz=cz)
    cz.close()
    assert again.tobytes() == whole.tobytes()
    assert first.tobytes() == whole[:, :first.shape[1]].tobytes()
    # block power, gate and counts of the ragged stream == cz_power_restate.c fed with the restatement's z rows
    L, levels = 7, (0.06, 0.04, 1)
    _, z = restate.run(x, True, D, h, K, bins, True, True, want_z=True)
    pw_ref, gate_ref, counts_ref = restate.power(z, L, *levels, out_pushes(pushes, D))
    assert 0 < gate_ref.mean() < 1 and (counts_ref == 0).any() and (counts_ref != 0).any(), "the levels must toggle the gates"
    cz = make_cz(ctx, "cf32", D, h, K, bins, "fm", True, max(pushes))
    cz.enable_power(block=L)
    assert ctx.lib.dh_channelizer_set_squelch(cz._h, *[float(np.float32(v)) for v in levels[:2]], levels[2]) == 0
    flat, pos, pw, gate, counts = x.reshape(-1, 2), 0, [], [], []
    for c in pushes:
        cz.push(np.ascontiguousarray(flat[pos:pos + c]))
        p, g, _ = cz.power_blocks()
        pw.append(host(ctx, p).copy()); gate.append(host(ctx, g).copy()); counts.append(host(ctx, cz.counts).view(np.uint32).copy())
        pos += c
    cz.close()
    assert np.concatenate(pw, axis=1).tobytes() == pw_ref.tobytes()
    assert np.concatenate(gate, axis=1).tobytes() == gate_ref.tobytes()
    assert np.stack(counts).tobytes() == counts_ref.tobytes()


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
    inc = np.zeros(4, np.uint32)
    bins = np.array([0, 1, -1, 5], np.int32)
    big = np.ones(64 * 2 + 1, np.float32)

    def cfg(**kw):
        c = _capi.ChannelizerConfig(C.sizeof(_capi.ChannelizerConfig), 0, 4, 4, h.ctypes.data_as(C.POINTER(C.c_float)), 8,
                                    inc.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 2, 1, 1000, ctx.mem.stream(), 1, 8,
                                    bins.ctypes.data_as(C.POINTER(C.c_int32)))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def create(c):
        hh = C.c_void_p()
        rc = lib.dh_channelizer_create(C.byref(c), C.byref(hh))
        if rc == 0:
            lib.dh_channelizer_destroy(hh)
        else:
            assert not hh.value
        return rc

    assert create(cfg()) == 0
    bad = [dict(raster=1), dict(raster=16385), dict(bins=C.POINTER(C.c_int32)()), dict(interpolation=3),
           dict(raster=2, n_taps=129, taps=big.ctypes.data_as(C.POINTER(C.c_float)))]      # T > 64 K
    for kw in bad:
        assert create(cfg(**kw)) == -1, kw
    assert create(cfg(raster=2, n_taps=128, taps=big.ctypes.data_as(C.POINTER(C.c_float)))) == 0
    assert create(cfg(increments=C.POINTER(C.c_uint32)())) == 0                           # ignored on a raster
    assert create(cfg(raster=0, increments=C.POINTER(C.c_uint32)())) == -1               # ... and only there
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
        old = cfg(struct_size=size)
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
def end_to_end_fixture(D, raster_hz, n_rows, seconds, device, seed):
    """The composite of test_channelizer.py's _end_to_end on a raster of raster_hz (tools/channelizer_model.py --raster runs its
    float64 model on the same).  With a device, the carriers are summed there and the noise still comes from the CPU
    generator, so a seed names the same noise on both tiers."""
    rate = 48000.0 * D
    n = int(seconds * rate)
    half = n_rows // 2
    raster = [(r - half) * raster_hz for r in range(n_rows)]
    rng = np.random.default_rng(n_rows)
    ysf_row, empty = 1, {2, n_rows - 2}
    strong, weak = 4, 5
    carriers, meta = [], {}
    for r in range(n_rows):
        if r in empty:
            continue
        off = raster[r] + float(rng.uniform(-150, 150))
        level = {strong: 0.0, weak: -20.0, 0: -30.0, ysf_row: -20.0}.get(r, float(rng.uniform(-20, -5)))
        if r == ysf_row:
            audio = wideband.ysf_audio(100 + r, 30)
        else:
            audio, meta[r] = wideband.dmr_audio(100 + r, n_calls=1 if seconds < 2.5 else 2)
            meta[r]["level_db"] = level
        carriers.append((off, level, audio))
    x = wideband.composite(D, carriers, n, seed=seed, device=device, noise_device="cpu")
    h = api.channel_taps(rate, D, 5500.0, 8000.0, 70.0)        # a neighbour 30 dB stronger must stay out of the passband
    return dict(rate=rate, n=n, raster=raster, raster_hz=raster_hz, x=x, h=h, meta=meta, ysf_row=ysf_row, empty=empty)


def _end_to_end(ctx, oracle, D, raster_hz, n_rows, seconds, device, seed):
    f = end_to_end_fixture(D, raster_hz, n_rows, seconds, device, seed)
    rate, n, raster, x, h, meta, ysf_row, empty = (f[k] for k in ("rate", "n", "raster", "x", "h", "meta", "ysf_row", "empty"))
    cz = api.Channelizer(rate, D, raster, h, input="cs16", output="fm", dcblock=True, max_input=n, ctx=ctx, raster_hz=raster_hz)
    rows, k = cz.push(x)
    assert k == n // D
    audio = np.ascontiguousarray(host(ctx, rows)[:, :k])
    cz.close()
    dmr_rows = [r for r in range(n_rows) if r != ysf_row]
    eng = api.Engine(len(dmr_rows), k, proto="dmr", ctx=ctx)
    eng.push(ctx.mem.from_numpy(audio[dmr_rows]))
    ev, ec = eng.events()
    ref = oracle.chain(audio[dmr_rows], proto=1)
    for i, r in enumerate(dmr_rows):
        e = ev[i, :ec[i]]
        assert ec[i] == ref["event_count"][i] and e.tobytes() == ref["events"][i, :ec[i]].tobytes(), "row %d differs from the oracle" % r
        if r in empty:
            assert not (e["type"] == 1).any(), "empty row %d: sync events" % r
            continue
        lcs = [api.parse_lc(p) for p in e[e["type"] == 4]["payload"]]
        assert lcs, "row %d: no LC" % r
        assert all(l["source"] == meta[r]["src"] and l["target"] == meta[r]["dst"] for l in lcs), "row %d: wrong ids" % r
        assert (e["type"] == 1).sum() >= meta[r]["superframes"], "row %d: fewer syncs than generated voice superframes" % r
    eng.close()
    yeng = api.Engine(1, k, proto="ysf", ctx=ctx)
    yeng.push(ctx.mem.from_numpy(audio[ysf_row:ysf_row + 1]))
    yev, yec = yeng.events()
    yref = oracle.chain(audio[ysf_row:ysf_row + 1], proto=2)
    assert yec[0] == yref["event_count"][0] and yev[0, :yec[0]].tobytes() == yref["events"][0, :yec[0]].tobytes()
    assert (yev[0, :yec[0]]["type"] == 16).sum() > 10, "YSF row: FICH events missing"
    yeng.close()


def test_end_to_end_small(emu_ctx, oracle):
    """768 kS/s, 12 kHz raster (K = 64), 8 rows, 1.5 s."""
    _end_to_end(emu_ctx, oracle, 16, 12000.0, 8, 1.5, "cpu", 7)


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
    _end_to_end(gpu_ctx, oracle, 50, 12500.0, 32, 4.0, "cuda", 7)
