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
import os
import subprocess

import numpy as np
import pytest

from digiham_amd import api, wideband
from digiham_amd._capi import DhError

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cz") / "libcz_restate.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(HERE, "cz_restate.c"),
                    "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    L.cz_restate.restype = None
    L.cz_restate.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    return L


def run_restate(L, x, cf32, D, h, B, incs, fm, dcblock, pushes=None, retunes=None):
    """incs: [B] increments at the start; pushes: the push lengths (for retunes); retunes: {push index: {ch: inc}}."""
    x = np.ascontiguousarray(x)
    n = x.size // 2
    pushes = pushes or [n]
    starts = np.cumsum([0] + list(pushes[:-1])).astype(np.uint64)
    nseg = len(pushes)
    inc = np.zeros((nseg, B), np.uint32)
    reset = np.zeros((nseg, B), np.uint8)
    cur = np.array(incs, np.uint32)
    for s in range(nseg):
        for ch, u in (retunes or {}).get(s, {}).items():
            cur[ch] = u
            reset[s, ch] = 1
        inc[s] = cur
    h = np.ascontiguousarray(h, np.float32)
    n_out = n // D
    out = np.zeros((B, n_out) if fm else (B, n_out, 2), np.float32)
    L.cz_restate(x.ctypes.data, int(cf32), n, D, h.ctypes.data, len(h), B, starts.ctypes.data, inc.ctypes.data, reset.ctypes.data,
                 nseg, int(fm), int(dcblock), out.ctypes.data)
    return out


def host(ctx, a):
    return np.asarray(ctx.mem.to_numpy(a))


def run_lib(ctx, x, fmt, D, h, incs, output, dcblock, pushes=None, retunes=None, rate=1.0, cz=None):
    """Push x in the given lengths; returns the concatenated rows."""
    n = x.size // 2
    pushes = pushes or [n]
    freqs = [u * rate / 2.0 ** 32 for u in incs]
    own = cz is None
    if own:
        cz = api.Channelizer(rate, D, freqs, h, input=fmt, output=output, dcblock=dcblock, max_input=max(max(pushes), 1), ctx=ctx)
        for ch, u in enumerate(incs):            # exact increments (the frequency round trip above may not be)
            ctx.lib.dh_channelizer_retune(cz._h, ch, int(u))
    parts, pos = [], 0
    flat = np.ascontiguousarray(x).reshape(-1, 2)
    for s, c in enumerate(pushes):
        for ch, u in (retunes or {}).get(s, {}).items():
            assert ctx.lib.dh_channelizer_retune(cz._h, ch, int(u)) == 0
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


EDGE_INCS = [0, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, (-123456789) & 0xFFFFFFFF, 0x40000000, 0xC0000000, 1]


def incs_for(B, seed):
    rng = np.random.default_rng(seed)
    extra = [int(v) for v in rng.integers(0, 1 << 32, max(B - len(EDGE_INCS), 0), dtype=np.uint64)]
    return (EDGE_INCS + extra)[:B]


# (format, output, dcblock, D, T, B)
EXACT_CASES = [("cs16", "iq", False, 1, 13, 3), ("cf32", "fm", False, 7, 37, 17), ("cs16", "fm", True, 16, 70, 20),
               ("cf32", "iq", False, 50, 101, 9), ("cs16", "fm", True, 50, 130, 70)]


@pytest.mark.parametrize("fmt,output,dc,D,T,B", EXACT_CASES)
def test_bit_exact_against_restatement(ctx, restate, fmt, output, dc, D, T, B):
    x = make_input(fmt, 1500 + 3 * D, D + T)
    h = np.random.default_rng(T).standard_normal(T).astype(np.float32) * 0.05
    incs = incs_for(B, B)
    got = run_lib(ctx, x, fmt, D, h, incs, output, dc)
    ref = run_restate(restate, x, fmt == "cf32", D, h, B, incs, output == "fm", dc)
    assert got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()


def test_subnormal_operands_bit_exact(ctx, restate):
    """Tiny CF32 input and taps: products, sums and rotations land in the subnormal range; they are kept (IEEE) on both
    sides, and device, emulation and restatement agree byte for byte."""
    x = make_input("cf32", 600, 5, scale=1e-36)
    x[::7] = 0.0
    h = np.random.default_rng(3).standard_normal(21).astype(np.float32) * 1e-3
    incs = incs_for(12, 4)
    for output, dc in (("iq", False), ("fm", True)):
        got = run_lib(ctx, x, "cf32", 7, h, incs, output, dc)
        ref = run_restate(restate, x, True, 7, h, 12, incs, output == "fm", dc)
        if output == "iq":
            assert (np.abs(ref[ref != 0]) < 1.1754944e-38).any(), "the case must reach subnormal outputs"
        assert got.tobytes() == ref.tobytes()


def test_streaming_pushes_retune_reset(ctx, restate):
    D, T, B = 7, 45, 19
    x = make_input("cs16", 4000, 9)
    h = np.random.default_rng(1).standard_normal(T).astype(np.float32) * 0.05
    incs = incs_for(B, 2)
    whole = run_lib(ctx, x, "cs16", D, h, incs, "fm", True)
    pushes = [0, 1, D - 1, D, 7 * D + 3, 0, 2500, 5]
    pushes.append(4000 - sum(pushes))
    ragged = run_lib(ctx, x, "cs16", D, h, incs, "fm", True, pushes=pushes)
    assert ragged.tobytes() == whole.tobytes()
    # a retune mid-stream (channels 3 and 11 at push 6), then one more at push 8
    ret = {6: {3: 0x12345678, 11: 0}, 8: {3: 0xFEDCBA98}}
    got = run_lib(ctx, x, "cs16", D, h, incs, "fm", True, pushes=pushes, retunes=ret)
    ref = run_restate(restate, x, False, D, h, B, incs, True, True, pushes=pushes, retunes=ret)
    assert got.tobytes() == ref.tobytes()
    # reset: a fresh stream
    cz = api.Channelizer(1.0, D, [0.0] * B, h, input="cs16", output="fm", max_input=4000, ctx=ctx)
    for ch, u in enumerate(incs):
        ctx.lib.dh_channelizer_retune(cz._h, ch, u)
    first = run_lib(ctx, x[:3000], "cs16", D, h, incs, "fm", True, pushes=[1000, 2000], cz=cz)
    cz.reset()
    again = run_lib(ctx, x, "cs16", D, h, incs, "fm", True, pushes=[4000], cz=cz)
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
            z = run_lib(ctx, x, "cf32", D, h, [u], "iq", False, rate=rate)[0]
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
    fm = run_lib(ctx, x, "cf32", D, h, [incs[1]], "fm", False, rate=rate)[0].astype(np.float64)
    steady = fm[Tp // D + 2:]
    assert np.abs(steady - 2 * delta / (rate / D)).max() <= 1e-6
    dc = run_lib(ctx, x, "cf32", D, h, [incs[1]], "fm", True, rate=rate)[0].astype(np.float64)
    assert abs(dc[-1]) < 0.15 * np.abs(dc[Tp // D + 2:Tp // D + 20]).max()        # 0.995^(n_out - 30) ~ 0.1


def test_validation(ctx):
    lib = ctx.lib
    h = np.ones(8, np.float32)
    inc = np.zeros(4, np.uint32)

    def cfg(**kw):
        from digiham_amd import _capi
        c = _capi.ChannelizerConfig(C.sizeof(_capi.ChannelizerConfig), 0, 4, 4, h.ctypes.data_as(C.POINTER(C.c_float)), 8,
                                    inc.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 2, 1, 1000, ctx.mem.stream())
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    bad = [dict(decimation=0), dict(decimation=1025), dict(n_taps=0), dict(n_taps=16385), dict(n_channels=0), dict(n_channels=65537),
           dict(input_format=3), dict(output_mode=0), dict(max_input=0), dict(struct_size=8),
           dict(taps=C.POINTER(C.c_float)()), dict(increments=C.POINTER(C.c_uint32)()), dict(output_mode=1, dcblock=1)]
    for kw in bad:
        hh = C.c_void_p()
        assert lib.dh_channelizer_create(C.byref(cfg(**kw)), C.byref(hh)) == -1, kw
    hnan = np.array([1.0, np.nan], np.float32)
    c = cfg(n_taps=2)
    c.taps = hnan.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.dh_channelizer_create(C.byref(c), C.byref(C.c_void_p())) == -1
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


def _end_to_end(ctx, oracle, D, n_rows, seconds, device):
    """Composite on a 12.5 kHz raster: DMR carriers at 0 .. -30 dB with small offsets, one YSF row, empty rows, a strong
    carrier next to one 20 dB weaker (FM capture sets that limit: a neighbour's spectral skirt inside the passband takes
    the discriminator over at about -30 dB).  Channelizer (FM + DC) -> DMR / YSF engines == oracle.chain on the channelizer's rows."""
    rate = 48000.0 * D
    n = int(seconds * rate)
    half = n_rows // 2
    raster = [(r - half) * 12500.0 for r in range(n_rows)]
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
        carriers.append((off, level, audio))
    x = wideband.composite(D, carriers, n, seed=7, device=device)
    h = api.channel_taps(rate, D, 5500.0, 8000.0, 70.0)        # a neighbour 30 dB stronger must stay out of the passband
    cz = api.Channelizer(rate, D, raster, h, input="cs16", output="fm", dcblock=True, max_input=n, ctx=ctx)
    rows, k = cz.push(x)
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
    _end_to_end(emu_ctx, oracle, 16, 8, 1.5, "cpu")


@pytest.mark.gpu
def test_end_to_end_wideband_gpu(gpu_ctx, oracle):
    _end_to_end(gpu_ctx, oracle, 50, 32, 4.0, "cuda")
