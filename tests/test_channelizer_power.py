"""dh_channelizer's block power, squelch gate and push counts (digiham_amd/csrc/channelizer_core.hpp).

Both tiers through the `ctx` fixture unless a test says otherwise:
  * byte-for-byte equality of power rows, gate rows and per-push counts with tests/cz_power_restate.c, a scalar restatement
    of the written specification fed with the z rows of tests/cz_restate.c (IQ mode);
  * streaming: ragged pushes, retunes, reset, and the host arithmetic of dh_channelizer_power_last;
  * the gate machine in isolation, against the restatement and against a second reading of the text in Python;
  * physics: the block power of a passband tone, a full-scale CS16 tone at 0 dB;
  * argument validation;
  * end to end: a keyed CS16 composite -> channelizer (FM + DC) with power -> a DMR engine fed with the counts.
"""
import ctypes as C

import numpy as np
import pytest

from cz_harness import (STRONG, WEAK, check_dmr_row, end_to_end_fixture, fixed, host, incs_for, make_cz, make_input, out_pushes,
                        restate, run_lib, same, segment_table, taps_for)      # noqa: F401  (fixture)
from digiham_amd import _capi, api, wideband
from digiham_amd._capi import DhError


# ---------------------------------------------------------------------------------------------------------------- 1. bit-exact
# (format, D, T, B, dc); every case runs IQ and FM (+ DC blocker when dc) output
EXACT_CASES = [("cs16", 1, 13, 3, False), ("cf32", 7, 37, 17, False), ("cf32", 16, 70, 20, True), ("cs16", 50, 130, 70, True)]
N_OUT = 2500


@pytest.mark.parametrize("L", [1, 7, 480, 1400])                 # 1400: longer than any single push below
@pytest.mark.parametrize("fmt,D,T,B,dc", EXACT_CASES)
def test_bit_exact_against_restatement(ctx, restate, fmt, D, T, B, dc, L):
    pushes = [400 * D + 1, 300 * D + 5, 450 * D - 3, 1350 * D - 3]
    n = sum(pushes)
    assert n // D == N_OUT and max(out_pushes(pushes, D)) < 1400
    x = make_input(fmt, n, D + T)
    h = taps_for(T)
    incs = incs_for(B, B)
    z = restate.run(fixed(D), x, fmt == "cf32", h, incs, False, False)
    op = out_pushes(pushes, D)
    p0, _, _ = restate.power(z, L, 0.0, 0.0, 0, op)
    # levels inside the spread of the restated powers, so that gates open and close; (L = 1400 completes one block: it opens)
    lv = (np.float32(np.quantile(p0, 0.7)), np.float32(np.quantile(p0, 0.4)), 1)
    rp, rg, rc = restate.power(z, L, lv[0], lv[1], lv[2], op)
    assert rg.any() and (L == 1400 or not rg.all())
    iq = run_lib(ctx, fixed(D), x, fmt, h, incs, "iq", False, pushes=pushes, power=(L, lv))
    fm = run_lib(ctx, fixed(D), x, fmt, h, incs, "fm", dc, pushes=pushes, power=(L, lv))
    assert same(iq["rows"], z)                                  # (what test_channelizer.py proves; the premise of this test)
    for got, what in ((iq, "iq"), (fm, "fm")):
        assert same(got["power"], rp), what
        assert same(got["gate"], rg), what
        assert same(got["counts"], rc), what
    assert same(fm["power"], iq["power"])


@pytest.mark.parametrize("offset_floats", [0, 1, 2, 3])
def test_iq_rows_at_any_alignment(ctx, restate, offset_floats):
    """IQ mode reads the caller's rows: 16-byte loads where a segment allows them, whatever the rows' own alignment (float32
    rows are only promised to be 4-byte aligned)."""
    D, T, B, L = 3, 20, 5, 37
    x = make_input("cf32", 1200, 4)
    h = taps_for(T, seed=8)
    incs = incs_for(B, 6)
    z = restate.run(fixed(D), x, True, h, incs, False, False)
    rp, rg, rc = restate.power(z, L, 0.0, 0.0, 0, [400])
    cz = make_cz(ctx, fixed(D), "cf32", h, incs, "iq", False, 1200)
    cz.enable_power(block=L)
    stride = 401
    buf = ctx.mem.zeros((2 * B * stride + 4,), np.float32)
    xd = ctx.mem.from_numpy(x)
    k = C.c_size_t(0)
    rows = C.c_void_p(ctx.mem.ptr(buf).value + 4 * offset_floats)
    assert ctx.lib.dh_channelizer_push(cz._h, ctx.mem.ptr(xd), 1200, rows, stride, C.byref(k)) == 0 and k.value == 400
    pw, g, first = cz.power_blocks()
    got = host(ctx, buf)[offset_floats:offset_floats + 2 * B * stride].reshape(B, stride, 2)[:, :400]
    assert same(np.ascontiguousarray(got), z)
    assert same(host(ctx, pw).copy(), rp) and same(host(ctx, g).copy(), rg) and first == 0
    cz.close()


# ---------------------------------------------------------------------------------------------------------------- 2. streaming
def test_streaming_pushes_retune_reset(ctx, restate):
    D, T, B, L = 7, 45, 19, 13
    x = make_input("cs16", 4000, 9)
    h = taps_for(T, seed=1)
    incs = incs_for(B, 2)
    z = restate.run(fixed(D), x, False, h, incs, False, False)
    p0, _, _ = restate.power(z, L, 0.0, 0.0, 0, [4000 // D])
    lv = (np.float32(np.quantile(p0, 0.75)), np.float32(np.quantile(p0, 0.35)), 2)
    whole = run_lib(ctx, fixed(D), x, "cs16", h, incs, "fm", True, power=(L, lv))
    pushes = [0, 1, D - 1, D, 7 * D + 3, 0, 2500, 5]
    pushes.append(4000 - sum(pushes))
    op = out_pushes(pushes, D)
    ragged = run_lib(ctx, fixed(D), x, "cs16", h, incs, "fm", True, pushes=pushes, power=(L, lv))          # (first / n_blocks checked per push)
    assert same(ragged["power"], whole["power"]) and same(ragged["gate"], whole["gate"]) and same(ragged["rows"], whole["rows"])
    rp, rg, rc = restate.power(z, L, lv[0], lv[1], lv[2], op)
    assert same(ragged["power"], rp) and same(ragged["gate"], rg) and same(ragged["counts"], rc)
    assert (ragged["counts"][[0, 1, 2, 5]] == 0).all()         # pushes without an output
    # two retunes mid-stream (channels 3 and 11 at push 6, channel 3 again at push 8)
    ret = {6: {3: 0x12345678, 11: 0}, 8: {3: 0xFEDCBA98}}
    zr = restate.run(fixed(D), x, False, h, incs, False, False, pushes=pushes, retunes=ret)
    mask = segment_table(len(x), incs, np.uint32, pushes, ret)[2]
    rp, rg, rc = restate.power(zr, L, lv[0], lv[1], lv[2], op, retune=mask)
    for output, dc in (("fm", True), ("iq", False)):
        got = run_lib(ctx, fixed(D), x, "cs16", h, incs, output, dc, pushes=pushes, retunes=ret, power=(L, lv))
        assert same(got["power"], rp) and same(got["gate"], rg) and same(got["counts"], rc), output
    # levels and hang change between pushes; the state is kept
    lvs = [(lv[0], lv[1], 2)] * 6 + [(lv[1], np.float32(0.0), 0), (lv[0], lv[0], 65535), (np.float32(0.0), np.float32(0.0), 0)]
    got = run_lib(ctx, fixed(D), x, "cs16", h, incs, "iq", False, pushes=pushes, power=(L, lvs))
    rp, rg, rc = restate.power(z, L, [t[0] for t in lvs], [t[1] for t in lvs], [t[2] for t in lvs], op)
    assert same(got["power"], rp) and same(got["gate"], rg) and same(got["counts"], rc)
    # reset: a fresh stream, the configuration stays
    cz = make_cz(ctx, fixed(D), "cs16", h, incs, "fm", True, 4000)
    cz.enable_power(block=L)
    first = run_lib(ctx, fixed(D), x[:3000], "cs16", h, incs, "fm", True, pushes=[1000, 2000], cz=cz, power=(L, lv))
    cz.reset()
    again = run_lib(ctx, fixed(D), x, "cs16", h, incs, "fm", True, pushes=[4000], cz=cz, power=(L, lv))
    cz.close()
    assert same(again["power"], whole["power"]) and same(again["gate"], whole["gate"]) and same(again["counts"], whole["counts"])
    nb = first["power"].shape[1]
    assert same(first["power"], whole["power"][:, :nb]) and same(first["gate"], whole["gate"][:, :nb])


# ---------------------------------------------------------------------------------------------------- 3. the gate in isolation
def python_gate(power, open_level, close_level, hang):
    """The gate of the specification, read a second time: closed -> open at p >= open_level; open: p >= close_level clears the
    quiet counter, anything else (NaN included) counts, and more than `hang` in a row close."""
    out = np.zeros(power.shape, np.uint8)
    for b, row in enumerate(power):
        is_open, quiet = False, 0
        for m, p in enumerate(row):
            if not is_open:
                if p >= open_level:
                    is_open, quiet = True, 0
            elif p >= close_level:
                quiet = 0
            else:
                quiet += 1
                if quiet > hang:
                    is_open, quiet = False, 0
            out[b, m] = is_open
    return out


@pytest.mark.parametrize("hang", [0, 1, 3])
def test_gate_machine_in_isolation(ctx, restate, hang):
    """CF32, D = 1, taps [1.0], increment 0: z = x bit for bit, and amplitudes that are powers of two make every block power exact."""
    L = 64
    q, m, l = 2.0 ** -7, 2.0 ** -4, 2.0 ** -2                    # powers 2^-14 (quiet), 2^-8 (between the levels), 2^-4 (loud)
    open_level, close_level = np.float32(2.0 ** -6), np.float32(2.0 ** -10)
    NAN = -1.0                                                   # a loud block with one NaN sample in its middle
    script = [q, q, m, l, m, q, m, q, q, m, q, q, q, q, q, m, l, q, l, NAN, l, q, q, NAN, q, q, q, q, l, NAN, NAN, NAN, NAN, NAN, l, l, q]
    rng = np.random.default_rng(hang)
    scripts = [script] + [list(rng.choice([q, m, l, NAN], len(script), p=[0.45, 0.25, 0.2, 0.1])) for _ in range(4)]
    nb = len(script)
    ref_rows = []
    for sc in scripts:                                           # one single-channel channelizer per script: the input is the channel
        x = np.zeros((nb * L, 2), np.float32)
        want = np.zeros(nb, np.float32)
        for i, a in enumerate(sc):
            x[i * L:(i + 1) * L, 0] = l if a == NAN else a
            want[i] = np.float32(l * l) if a == NAN else np.float32(a * a)
            if a == NAN:
                x[i * L + 20, 1] = np.nan                        # outputs 20 .. 35 of the block: 16 and more from both of its ends
                want[i] = np.nan
        z = restate.run(fixed(1), x, True, [1.0], [0], False, False)
        clean = np.repeat(np.array([a != NAN for a in sc]), L)
        assert same(z[0][clean], x[clean])
        pushes = [3 * L + 5, L - 5, 7, 10 * L, 1, nb * L - (14 * L + 8)]
        op = out_pushes(pushes, 1)
        rp, rg, rc = restate.power(z, L, open_level, close_level, hang, op)
        assert np.array_equal(rp[0], want, equal_nan=True)       # exact powers, NaN where scripted
        pg = python_gate(rp, open_level, close_level, hang)
        assert same(pg, rg), "the two readings of the specification differ"
        got = run_lib(ctx, fixed(1), x, "cf32", [1.0], [0], "iq", False, pushes=pushes, power=(L, (open_level, close_level, hang)))
        assert same(got["power"], rp) and same(got["gate"], rg) and same(got["counts"], rc)
        assert same(got["gate"], pg)
        ref_rows.append(rg[0])
    g = ref_rows[0]                                              # the scripted row crosses both levels in both directions
    assert g[2] == 0 and g[3] == 1 and g[4] == 1 and g[16] == 1 and g.min() == 0
    assert g[5] == (1 if hang >= 1 else 0) and g[14] == 0 and g[15] == 0
    assert g[19] == (1 if hang >= 1 else 0)                      # a NaN block counts as quiet ...
    assert g[29:34].max() == (1 if hang >= 1 else 0) and g[33] == 0            # ... and never opens or holds a gate


# ---------------------------------------------------------------------------------------------------------------- 4. physics
def test_block_power_of_a_tone(ctx):
    """Passband tone of amplitude A at offset delta, blocks after the filter has filled: power / (A^2 |H(delta)|^2) - 1 within
    2 * 1e-5 * sum|h| / |H(delta)| (twice the amplitude bound test_ddc_physics asserts) + (L + 4) * 2^-24 (the roundings of
    q, of an in-order float sum of L non-negative terms, of inv and its multiply).  Full scale of CS16 is 32767 * 2^-15."""
    rate, D, L = 768000.0, 16, 100
    h = api.channel_taps(rate, D, 6500.0, 12000.0, 60.0)
    T = len(h)
    Tp = 16 * ((T + 15) // 16)
    n = 8000
    nn = np.arange(n, dtype=np.float64)
    H = lambda d: np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * d / rate * np.arange(T)))
    sum_h = float(np.abs(h.astype(np.float64)).sum())
    first_full = -(-Tp // (D * L))                                # first block whose outputs all have n_j >= T'
    for fmt, A in (("cf32", 0.5), ("cs16", 32767.0 / 32768.0)):
        for u in (0, api.nco_increment(100000.0, rate), api.nco_increment(-237500.0, rate)):
            for delta in ((1234.5, -4000.0) if fmt == "cf32" else (0.0, 2100.0)):
                xs = A * np.exp(2j * np.pi * ((u / 2.0 ** 32) + delta / rate) * nn)
                x = np.stack([xs.real, xs.imag], 1)
                x = x.astype(np.float32) if fmt == "cf32" else np.round(x * 32768.0).astype(np.int16)
                got = run_lib(ctx, fixed(D), x, fmt, h, [u], "iq", False, rate=rate, power=(L, (0.0, 0.0, 0)))
                p = got["power"][0].astype(np.float64)
                assert len(p) == n // D // L and len(p) > first_full + 2
                gain = abs(H(delta))
                bound = 2.0 * 1e-5 * sum_h / gain + (L + 4) * 2.0 ** -24
                err = np.abs(p[first_full:] / (A * A * gain * gain) - 1.0).max()
                print("tone %s u=%08x delta=%.1f: |power / (A^2 |H|^2) - 1| = %.3g, bound %.3g, %.4f dB"
                      % (fmt, u, delta, err, bound, 10 * np.log10(p[first_full:].mean() / gain ** 2)))
                assert err <= bound, (fmt, u, delta, err, bound)
                assert got["gate"][0, first_full:].all() and got["counts"][0, 0] == n // D          # power only: open


# ---------------------------------------------------------------------------------------------------------------- 5. validation
def test_validation(ctx):
    lib, mem = ctx.lib, ctx.mem
    h = np.ones(8, np.float32)
    cz = api.Channelizer(1.0, 4, [0.0] * 4, h, max_input=1000, ctx=ctx)           # out_stride 251
    power, gate, counts = mem.zeros((4, 64), np.float32), mem.zeros((4, 64), np.uint8), mem.zeros((4,), np.uint32)

    def cfg(**kw):
        c = _capi.ChannelizerPowerConfig(C.sizeof(_capi.ChannelizerPowerConfig), 10, 0.5, 0.25, 3, mem.ptr(power), mem.ptr(gate),
                                         mem.ptr(counts), 64)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    first, nb = C.c_uint64(), C.c_size_t()
    # before the enable
    assert lib.dh_channelizer_power_last(cz._h, C.byref(first), C.byref(nb)) == -1
    assert lib.dh_channelizer_set_squelch(cz._h, 0.5, 0.25, 0) == -1
    inf, nan = float("inf"), float("nan")
    bad = [dict(block=0), dict(block=65537), dict(stride=25), dict(d_power=None), dict(d_gate=None), dict(d_counts=None),
           dict(open_level=inf), dict(open_level=nan), dict(close_level=nan), dict(close_level=-0.5), dict(open_level=-1.0, close_level=-2.0),
           dict(close_level=0.75), dict(hang_blocks=65536), dict(struct_size=8)]
    for kw in bad:
        assert lib.dh_channelizer_power_enable(cz._h, C.byref(cfg(**kw))) == -1, kw
    assert lib.dh_channelizer_power_enable(cz._h, None) == -1 and lib.dh_channelizer_power_enable(None, C.byref(cfg())) == -1
    assert lib.dh_channelizer_power_last(cz._h, C.byref(first), C.byref(nb)) == -1          # still off
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(cfg(stride=26))) == 0             # (1000 / 4 + 1) / 10 + 1
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(cfg(block=65536, hang_blocks=65535, open_level=0.0, close_level=0.0))) == 0
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(cfg())) == 0                      # (again, before any sample: fine)
    assert lib.dh_channelizer_power_last(cz._h, C.byref(first), C.byref(nb)) == 0 and (first.value, nb.value) == (0, 0)
    assert lib.dh_channelizer_power_last(cz._h, None, C.byref(nb)) == -1 and lib.dh_channelizer_power_last(cz._h, C.byref(first), None) == -1
    assert lib.dh_channelizer_power_last(None, C.byref(first), C.byref(nb)) == -1
    for args in ((inf, 0.25, 0), (nan, 0.25, 0), (0.5, nan, 0), (0.5, -0.25, 0), (0.25, 0.5, 0), (0.5, 0.25, 65536)):
        assert lib.dh_channelizer_set_squelch(cz._h, *args) == -1, args
    assert lib.dh_channelizer_set_squelch(None, 0.5, 0.25, 0) == -1
    assert lib.dh_channelizer_set_squelch(cz._h, 0.5, 0.5, 65535) == 0 and lib.dh_channelizer_set_squelch(cz._h, 0.0, 0.0, 0) == 0
    # after samples: enabling again is refused until a reset
    x = np.full((103, 2), 16384, np.int16)
    n_out = C.c_size_t(0)
    assert lib.dh_channelizer_push_host(cz._h, x.ctypes.data_as(C.c_void_p), 103, mem.ptr(cz.rows), cz.out_stride, C.byref(n_out)) == 0
    assert n_out.value == 25
    assert lib.dh_channelizer_power_last(cz._h, C.byref(first), C.byref(nb)) == 0 and (first.value, nb.value) == (0, 2)
    assert (host(ctx, counts).view(np.uint32) == 25).all() and host(ctx, gate)[:, :2].all()
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(cfg())) == -1
    assert lib.dh_channelizer_reset(cz._h) == 0
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(cfg())) == 0
    cz.close()
    # the Python front-end
    cz = api.Channelizer(1.0, 4, [0.0] * 4, h, max_input=1000, ctx=ctx)
    with pytest.raises(DhError):
        cz.power_blocks()
    with pytest.raises(DhError):
        cz.set_squelch(-10.0, -20.0, 0)
    for kw in (dict(block=0), dict(block=65537), dict(open_db=-20.0, close_db=-10.0), dict(hang_blocks=65536)):
        with pytest.raises(DhError):
            cz.enable_power(**kw)
    assert cz.counts is None
    cz.enable_power(block=10, open_db=-6.0, close_db=-9.0, hang_blocks=1)
    assert cz.power.shape == (4, 26) and cz.gate.shape == (4, 26) and cz.counts.shape == (4,)
    cz.set_squelch(-3.0, -3.0, 0)
    with pytest.raises(DhError):
        cz.set_squelch(-3.0, -2.0, 0)
    cz.close()


def test_composite_without_keying_is_unchanged():
    audio, _ = wideband.dmr_audio(3, n_calls=1)
    carriers = [(1000.0, 0.0, audio), (-26000.0, -12.0, audio[::-1].copy())]
    a = wideband.composite(4, carriers, 40000, seed=3)
    b = wideband.composite(4, carriers, 40000, seed=3, keying=None)
    c = wideband.composite(4, carriers, 40000, seed=3, keying=[None, None])
    assert a.dtype == np.int16 and a.tobytes() == b.tobytes() == c.tobytes()
    k = wideband.composite(4, carriers, 40000, seed=3, keying=[(0.05, 0.15), None])
    only = wideband.composite(4, carriers[1:], 40000, seed=3, peak=0.9 * 10 ** (-12 / 20.0) / (1 + 10 ** (-12 / 20.0)))
    t = np.arange(40000) / (4 * 48000.0)
    off = (t < 0.05) | (t >= 0.15)
    assert np.abs(k[off].astype(np.int32) - only[off]).max() <= 1          # keyed off: the other carrier (and the noise) alone
    assert np.abs(k[~off].astype(np.int32) - only[~off]).max() > 1000


# ------------------------------------------------------------------------------------------------------- 6. end to end, gated
GATED_L, GATED_HANG, GATED_PUSH = 480, 2, 4807                    # pushes of 0.1 s + 7 outputs: they end inside blocks


def _gated_scene(restate, D, n_rows, seconds, device, weakest_db, threads):
    """A keyed composite on a 12.5 kHz raster (all carriers key on at 0.2 s and off 0.3 s before the end, their audio starting
    at key-on; two rows are never keyed), the restatement's powers, and the precondition on the scene asserted from them."""
    L, hang, P = GATED_L, GATED_HANG, GATED_PUSH
    assert seconds < 2.5                                          # one call per carrier
    key = (0.2, seconds - 0.3)
    f = end_to_end_fixture(1, D, n_rows, seconds, device, seed=7, key=key, levels={STRONG: 0.0, WEAK: -20.0, 0: weakest_db}, ysf_row=None)
    x, h, raster, rate, n, empty, meta, keyed = f["x"], f["h"], f["raster"], f["rate"], f["n"], f["empty"], f["meta"], sorted(f["meta"])
    for _, _, audio in f["carriers"]:
        assert len(audio) / 48000.0 <= key[1] - key[0], "the keyed interval must hold the whole generated audio"
    xh = x if isinstance(x, np.ndarray) else x.cpu().numpy()
    Tp = 16 * ((len(h) + 15) // 16)
    incs = [api.nco_increment(f, rate) for f in raster]
    n_out = n // D
    pushes = [P * D] * (n_out // P) + ([n - (n_out // P) * P * D] if n - (n_out // P) * P * D else [])
    op = out_pushes(pushes, D)
    edges = np.cumsum([0] + op)
    # ---- the restatement, and the precondition on the scene (from the restatement's powers only)
    z = restate.run(fixed(D), xh, False, h, incs, False, False, threads=threads)
    pw, _, _ = restate.power(z, L, 0.0, 0.0, 0, op)
    nb = pw.shape[1]
    F = -(-Tp // D)                                               # the filter's length in outputs
    on_j, off_j = int(round(key[0] * 48000)), int(round(key[1] * 48000))
    blk = np.arange(nb)
    inside = (blk * L >= on_j + F) & ((blk + 1) * L <= off_j)
    outside = ((blk + 1) * L <= on_j) | (blk * L >= off_j + F)
    assert inside.sum() > 100 and outside.sum() > 40
    min_keyed = float(pw[keyed][:, inside].min())
    max_empty = float(pw[sorted(empty)].max())
    db = lambda v: 10.0 * np.log10(v)
    print("gated scene: weakest keyed block %.1f dBFS, strongest block of an empty row %.1f dBFS" % (db(min_keyed), db(max_empty)))
    assert db(min_keyed) - db(max_empty) >= 8.0, "the scene does not meet the test's precondition"
    open_db = db(min_keyed) - 3.0
    close_db = open_db - 3.0
    open_level, close_level = np.float32(10.0 ** (open_db / 10.0)), np.float32(10.0 ** (close_db / 10.0))
    assert pw[keyed][:, outside].max() < close_level, "a keyed row is above close_db outside its keyed interval"
    rp, rg, rc = restate.power(z, L, open_level, close_level, hang, op)
    return dict(x=x, h=h, raster=raster, rate=rate, pushes=pushes, op=op, edges=edges, blk=blk, inside=inside, on_j=on_j, off_j=off_j, F=F,
                open_db=open_db, close_db=close_db, rp=rp, rg=rg, rc=rc, empty=empty, keyed=keyed, meta=meta)


def _end_to_end_gated(ctx, oracle, restate, D, n_rows, seconds, device, weakest_db, threads):
    """The scene above -> channelizer (FM + DC, power with L = 480) -> DMR engines fed with the counts."""
    L, hang, P = GATED_L, GATED_HANG, GATED_PUSH
    sc = _gated_scene(restate, D, n_rows, seconds, device, weakest_db, threads)
    x, h, raster, rate, pushes, op, edges, blk, inside = (sc[k] for k in ("x", "h", "raster", "rate", "pushes", "op", "edges", "blk", "inside"))
    on_j, off_j, F, open_db, close_db, rp, rg, rc = (sc[k] for k in ("on_j", "off_j", "F", "open_db", "close_db", "rp", "rg", "rc"))
    empty, keyed, meta = sc["empty"], sc["keyed"], sc["meta"]
    # ---- the library
    cz = api.Channelizer(rate, D, raster, h, input="cs16", output="fm", dcblock=True, max_input=P * D, ctx=ctx)
    cz.enable_power(block=L, open_db=open_db, close_db=close_db, hang_blocks=hang)
    lo = 3                                                        # two engines on slices of the rows and of the counts
    engs = [(api.Engine(lo, cz.out_stride, proto="dmr", ctx=ctx), 0, lo), (api.Engine(n_rows - lo, cz.out_stride, proto="dmr", ctx=ctx), lo, n_rows)]
    counts, power, gate = [], [], []
    passed_rows, evs, nsym = [[] for _ in range(n_rows)], [[] for _ in range(n_rows)], np.zeros(n_rows, np.int64)
    pos = 0
    for s, c in enumerate(pushes):
        rows, k = cz.push(x[pos:pos + c])
        pos += c
        assert k == op[s]
        cnt = host(ctx, cz.counts).view(np.uint32).copy()
        counts.append(cnt)
        p_, g_, first = cz.power_blocks()
        assert first == edges[s] // L
        power.append(host(ctx, p_).copy()); gate.append(host(ctx, g_).copy())
        hr = host(ctx, rows)
        for r in range(n_rows):
            if cnt[r]:
                passed_rows[r].append(hr[r, :k].copy())
        for eng, a, b in engs:
            eng.push(rows[a:b], n=k, counts=cz.counts[a:b])
            _, sym_n = eng.symbols()
            e, ec = eng.events()
            for r in range(a, b):
                evs[r].append(e[r - a, :ec[r - a]].copy())
                nsym[r] += sym_n[r - a]
    for eng, _, _ in engs:
        eng.close()
    cz.close()
    counts = np.stack(counts)
    assert same(np.concatenate(power, axis=1), rp) and same(np.concatenate(gate, axis=1), rg)
    assert same(counts, rc), "counts differ from the restatement"
    # ---- what the gate did (bounds that hold whatever the restatement says)
    for r in sorted(empty):
        assert (counts[:, r] == 0).all(), "empty row %d passed a push" % r
        assert nsym[r] == 0 and sum(len(e) for e in evs[r]) == 0, "empty row %d: the engine saw input" % r
    m_off = (off_j + F) // L
    for r in keyed:
        passed = np.nonzero(counts[:, r])[0]
        assert len(passed) and (np.diff(passed) == 1).all(), "row %d: the passed pushes are not one run: %s" % (r, passed)
        for s in range(len(pushes)):
            a, b = edges[s], edges[s + 1]
            done = blk[((blk + 1) * L > a) & ((blk + 1) * L <= b)]           # blocks this push completes
            if inside[done].any():
                assert counts[s, r] == op[s], "row %d: push %d completes a keyed block and did not pass" % (r, s)
            if b <= on_j:
                assert counts[s, r] == 0, "row %d: push %d ends before key-on and passed" % (r, s)
            if a >= (m_off + hang + 2 + 1) * L:
                assert counts[s, r] == 0, "row %d: push %d begins after the hang time and passed" % (r, s)
            assert counts[s, r] in (0, op[s])
        audio = np.concatenate(passed_rows[r])
        ref = oracle.chain(audio[None, :], proto=1)
        check_dmr_row(r, np.concatenate(evs[r]), ref, 0, meta[r])


def test_end_to_end_gated_small(emu_ctx, oracle, restate):
    _end_to_end_gated(emu_ctx, oracle, restate, 16, 8, 2.0, "cpu", -26.0, 4)


@pytest.mark.gpu
def test_end_to_end_gated_wideband_gpu(gpu_ctx, oracle, restate):
    """The large scene holds no carrier below -20 dB.  An empty row sees the skirts of its neighbours only some 30 dB below
    those neighbours, so with a -30 dB carrier the weakest keyed block would lie about 2 dB above the strongest block of an
    empty row; at -20 dB the restatement gives 16 dB.  The asserted precondition guards it."""
    _end_to_end_gated(gpu_ctx, oracle, restate, 50, 32, 2.0, "cuda", -20.0, 16)


# -------------------------------------------------------------------------------------------------------------- 7. GPU tier only
@pytest.mark.gpu
def test_thousand_channels_gpu(gpu_ctx, restate):
    """A size a user would run: 1 000 channels (not a multiple of 64) of a 2.4 MS/s CS16 stream, D = 50, L = 480, 1 s in three pushes."""
    ctx = gpu_ctx
    rate, D, B, L = 2.4e6, 50, 1000, 480
    n = 2400000
    h = api.channel_taps(rate, D, 5000.0, 20000.0, 40.0)
    rng = np.random.default_rng(77)
    incs = [int(v) for v in rng.integers(0, 1 << 32, B, dtype=np.uint64)]
    x = rng.integers(-3000, 3000, (n, 2)).astype(np.int16)
    nn = np.arange(n, dtype=np.float64)
    for b, (a0, t0, t1) in {5: (9000.0, 0.1, 0.6), 500: (4000.0, 0.3, 0.35), 999: (12000.0, 0.0, 1.0)}.items():      # keyed tones
        tone = a0 * np.exp(2j * np.pi * (incs[b] / 2.0 ** 32) * nn) * ((nn >= t0 * rate) & (nn < t1 * rate))
        x += np.stack([tone.real, tone.imag], 1).round().astype(np.int16)
    pushes = [1000003, 399997, 1000000]
    op = out_pushes(pushes, D)
    z = restate.run(fixed(D), x, False, h, incs, False, False, threads=16)
    p0, _, _ = restate.power(z, L, 0.0, 0.0, 0, op)
    lv = (np.float32(np.quantile(p0, 0.9)), np.float32(np.quantile(p0, 0.5)), 3)
    rp, rg, rc = restate.power(z, L, lv[0], lv[1], lv[2], op)
    assert rg.any() and not rg.all() and rc.any() and not rc.all()
    for output, dc in (("fm", True), ("iq", False)):
        got = run_lib(ctx, fixed(D), x, "cs16", h, incs, output, dc, pushes=pushes, rate=rate, keep_rows=False, power=(L, lv))
        assert same(got["power"], rp) and same(got["gate"], rg) and same(got["counts"], rc), output


@pytest.mark.gpu
@pytest.mark.parametrize("output,dc", [("iq", False), ("fm", True)])
def test_more_segments_than_one_grid_pass_gpu(gpu_ctx, restate, output, dc):
    """Short blocks, long pushes: 192 channels x 14 287 segments per push is more lanes than one pass of k_cz_power's grid
    (8 192 workgroups of 256), and the second and third push begin inside a block.  The lane that continues the carried block
    and the lane that leaves the next carry are then far apart in the launch; the carried S must not pass between them."""
    ctx = gpu_ctx
    D, T, B, L = 2, 16, 192, 7
    pushes = [200006, 200001, 40003]
    op = out_pushes(pushes, D)
    assert B * (op[0] // L) > 8192 * 256 and op[0] % L and (op[0] + op[1]) % L
    x = make_input("cs16", sum(pushes), 21)
    h = taps_for(T, seed=5)
    incs = incs_for(B, 12)
    z = restate.run(fixed(D), x, False, h, incs, False, False, threads=16)
    p0, _, _ = restate.power(z, L, 0.0, 0.0, 0, op)
    lv = (np.float32(np.quantile(p0, 0.8)), np.float32(np.quantile(p0, 0.3)), 1)
    rp, rg, rc = restate.power(z, L, lv[0], lv[1], lv[2], op)
    got = run_lib(ctx, fixed(D), x, "cs16", h, incs, output, dc, pushes=pushes, keep_rows=False, power=(L, lv))
    assert same(got["power"], rp) and same(got["gate"], rg) and same(got["counts"], rc)
