"""dh_channelizer's frequency-error blocks (digiham_amd/csrc/channelizer_core.hpp).

Both tiers through the `ctx` fixture unless a test says otherwise:
  * bit patterns of the ferr rows against tests/cz_ferr_restate.c, a scalar restatement of the written specification fed with
    the z rows of the bank's own restatement (a NaN may be any NaN): three kinds of bank, both output modes, ragged pushes,
    rows that are only 4-byte aligned, more items than one pass of the launch's grid;
  * the discriminator cross-check, retune in mid-block, reset, special operands;
  * off means off: the same stream with and without d_ferr, and the struct_size rule;
  * physics: an unmodulated carrier against a bound derived here, a DMR carrier against a tolerance measured with the
    restatement;
  * the Python surface.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cz_harness import (KINDS, bins_for, fixed, host, incs_for, make_cz, make_input, out_pushes, raster, rational, restate, same,
                        segment_table, taps_for)      # noqa: F401  (fixture)
from digiham_amd import _capi, api, wideband
from digiham_amd._capi import DhError

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the restatement, and the library driven push by push ----------------------------------------------------------------
class FerrRestate:
    def __init__(self, d):
        so = str(d / "libcz_ferr_restate.so")
        subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(HERE, "cz_ferr_restate.c"),
                        "-o", so, "-lm"], check=True)
        self.fn = C.CDLL(so).cz_ferr_restate
        self.fn.restype = None
        self.fn.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]

    def __call__(self, z, block, op, retune=None):
        """z [B][n][2], the outputs of every push, the reset table of the run that made z -> ferr [B][n // block] float32."""
        z = np.ascontiguousarray(z, np.float32)
        B, n = z.shape[0], z.shape[1]
        assert sum(op) <= n
        pl = np.array(op, np.uint64)
        rt = np.zeros((len(op), B), np.uint8) if retune is None else np.ascontiguousarray(retune, np.uint8)
        ferr = np.zeros((B, n // block), np.float32)
        self.fn(z.ctypes.data, B, n, block, pl.ctypes.data, len(op), rt.ctypes.data, ferr.ctypes.data)
        return ferr


_ferr_restate = []


@pytest.fixture(scope="session")
def ferr_restate(tmp_path_factory):
    if not _ferr_restate:
        _ferr_restate.append(FerrRestate(tmp_path_factory.mktemp("czferr")))
    return _ferr_restate[0]


def same_bits(a, b):
    """Equal shapes, NaN in the same places (any NaN), every other value bit for bit."""
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()


def z_rows(restate, bank, x, fmt, h, words, pushes=None, retunes=None, threads=1):
    """The rotated outputs [B][n_out][2] of the bank's restatement."""
    return restate.run(bank, x, fmt == "cf32", h, words, False, False, pushes, retunes, want_z=True, threads=threads)[1]


def run_ferr(ctx, bank, x, fmt, h, words, output, dc, pushes, block, ferr=True, retunes=None, levels=(0.0, 0.0, 0), rate=None, cz=None,
             row_offset=0, keep_rows=True):
    """Push x in the given lengths through a channelizer with power (and ferr) enabled.  row_offset: the rows go to a buffer
    of the test's, that many floats behind an aligned address.  -> dict(rows, power, gate, ferr: concatenated over the
    pushes; counts [npush][B]; first, nblk per push)."""
    flat = np.ascontiguousarray(x).reshape(-1, 2)
    op = out_pushes(pushes, bank.M, max(bank.L, 1))
    own = cz is None
    if own:
        cz = make_cz(ctx, bank, fmt, h, words, output, dc, max(max(pushes), 1), rate)
        cz.enable_power(block=block, ferr=ferr)
    assert ctx.lib.dh_channelizer_set_squelch(cz._h, float(levels[0]), float(levels[1]), int(levels[2])) == 0
    B, per = len(words), 1 if output == "fm" else 2
    buf = ctx.mem.zeros((B * cz.out_stride * per + 4,), np.float32) if row_offset else None
    res = dict(rows=[], power=[], gate=[], ferr=[], counts=[], first=[], nblk=[])
    pos = 0
    for s, c in enumerate(pushes):
        for ch, w in (retunes or {}).get(s, {}).items():
            KINDS[bank.kind].retune(ctx, cz, ch, w)
        part = np.ascontiguousarray(flat[pos:pos + c])
        if row_offset:
            k = C.c_size_t(0)
            rows = C.c_void_p(ctx.mem.ptr(buf).value + 4 * row_offset)
            assert ctx.lib.dh_channelizer_push_host(cz._h, part.ctypes.data_as(C.c_void_p), c, rows, cz.out_stride, C.byref(k)) == 0
            k = k.value
            got = host(ctx, buf)[row_offset:row_offset + B * cz.out_stride * per].reshape((B, cz.out_stride) + ((2,) if per == 2 else ()))
        else:
            rows, k = cz.push(part)
            got = host(ctx, rows)
        assert k == op[s], (s, k)
        if keep_rows:
            res["rows"].append(got[:, :k].copy())
        pw, g, first = cz.power_blocks()
        res["power"].append(host(ctx, pw).copy())
        res["gate"].append(host(ctx, g).copy())
        res["counts"].append(host(ctx, cz.counts).view(np.uint32).copy())
        res["first"].append(first)
        res["nblk"].append(pw.shape[1])
        if ferr:
            fe, ffirst = cz.ferr_blocks()
            assert ffirst == first and fe.shape == pw.shape
            res["ferr"].append(host(ctx, fe).copy())
        pos += c
    if own:
        cz.close()
    for key in ("rows", "power", "gate", "ferr"):
        res[key] = np.concatenate(res[key], axis=1) if res[key] else None
    res["counts"] = np.stack(res["counts"])
    return res


def words_for(bank, B, seed):
    return bins_for(B, bank.K, seed) if bank.K else incs_for(B, seed)


# ---------------------------------------------------------------------------------------------------------------- 1. bit-exact
BANKS = {"fixed": (fixed(4), 37), "rational": (rational(3, 7), 50), "raster": (raster(16, 5), 40)}     # bank, taps
PUSHES = [1, 2, 3, 5, 0, 1500, 7, 9, 11, 900, 1, 1561]          # 4 000 input samples
N_IN, B_EXACT = 4000, 70                                         # 70 channels: more than a wavefront and a 64-channel column tile


def push_properties(op, L):
    """What the cut of the stream exercises for block length L: (a push ends inside a block, a push yields no output, a push
    completes several blocks, one block takes outputs from three pushes)."""
    edges = np.cumsum([0] + list(op))
    inside = any(e % L for e in edges[1:])
    several = any(edges[s + 1] // L - edges[s] // L >= 2 for s in range(len(op)))
    spans = False
    for m in range(edges[-1] // L + 1):
        spans |= sum(1 for s in range(len(op)) if op[s] and edges[s] < (m + 1) * L and edges[s + 1] > m * L) >= 3
    return inside, 0 in op, several, spans


@pytest.mark.parametrize("L", [1, 7, 480])
@pytest.mark.parametrize("fmt,output,dc", [("cs16", "fm", True), ("cf32", "iq", False)])
@pytest.mark.parametrize("kind", sorted(BANKS))
def test_bit_exact_against_restatement(ctx, restate, ferr_restate, kind, fmt, output, dc, L):
    bank, T = BANKS[kind]
    assert sum(PUSHES) == N_IN and 1 in PUSHES
    op = out_pushes(PUSHES, bank.M, max(bank.L, 1))
    inside, empty, several, spans = push_properties(op, L)
    # all four with blocks of 7; a block of one output has no inside, and 4 000 samples hold too few blocks of 480
    assert empty and (several or L == 480) and (L == 1 or (inside and spans)), (op, L)
    x = make_input(fmt, N_IN, T + L)
    h = taps_for(T)
    words = words_for(bank, B_EXACT, 3)
    z = z_rows(restate, bank, x, fmt, h, words)
    want = ferr_restate(z, L, op)
    assert want.shape[1] == sum(op) // L and np.abs(want).max() > 0.01
    got = run_ferr(ctx, bank, x, fmt, h, words, output, dc, PUSHES, L)
    if output == "iq":
        assert same(got["rows"], z)                             # (what the banks' own tests prove; the premise of this one)
    assert same_bits(got["ferr"], want)
    j0 = np.cumsum([0] + op)
    assert got["first"] == [int(j) // L for j in j0[:-1]]
    assert got["nblk"] == [int(j0[s + 1]) // L - int(j0[s]) // L for s in range(len(op))]


@pytest.mark.parametrize("row_offset", [1, 3])
def test_iq_rows_only_4_byte_aligned(ctx, restate, ferr_restate, row_offset):
    """IQ mode reads the caller's rows; at an odd float offset they go word by word."""
    bank, T = BANKS["fixed"]
    L = 37
    op = out_pushes(PUSHES, bank.M)
    x = make_input("cf32", N_IN, 5)
    h = taps_for(T)
    words = words_for(bank, 9, 4)
    z = z_rows(restate, bank, x, "cf32", h, words)
    got = run_ferr(ctx, bank, x, "cf32", h, words, "iq", False, PUSHES, L, row_offset=row_offset)
    assert same(got["rows"], z)
    assert same_bits(got["ferr"], ferr_restate(z, L, op))


# -------------------------------------------------------------------------------------------------------------- 2. grid stride
@pytest.mark.gpu
@pytest.mark.parametrize("output,dc", [("iq", False), ("fm", True)])
def test_more_segments_than_one_grid_pass_gpu(gpu_ctx, restate, ferr_restate, output, dc):
    """Short blocks, long pushes: 192 channels x 11 668 segments per push is more lanes than one pass of k_cz_ferr's grid
    (grid_for clamps it to 8 192 workgroups of 256), and the second and third push begin inside a block: the lane that
    continues the carried block and the lane that leaves the next carry are far apart in the launch."""
    D, T, B, L = 2, 16, 192, 3
    pushes = [70006, 70003, 10001]
    op = out_pushes(pushes, D)
    assert B * (op[0] // L) > 8192 * 256 and B * (op[1] // L) > 8192 * 256 and op[0] % L and (op[0] + op[1]) % L
    x = make_input("cs16", sum(pushes), 21)
    h = taps_for(T, seed=5)
    incs = incs_for(B, 12)
    z = z_rows(restate, fixed(D), x, "cs16", h, incs, threads=16)
    got = run_ferr(gpu_ctx, fixed(D), x, "cs16", h, incs, output, dc, pushes, L, keep_rows=False)
    assert same_bits(got["ferr"], ferr_restate(z, L, op))


# ------------------------------------------------------------------------------------------------------ 3. the discriminator
def test_block_of_one_is_the_discriminator(ctx):
    """block = 1, FM without the DC blocker: the same product and the same polynomial, with one addition to +0 in between (it
    turns a -0 into +0, which the polynomial's result can show as the sign of a zero: equal as floats)."""
    bank, T = BANKS["fixed"]
    x = make_input("cf32", 1203, 11)
    x[700, 0] = np.nan
    h = taps_for(T)
    words = words_for(bank, 70, 9)
    got = run_ferr(ctx, bank, x, "cf32", h, words, "fm", False, [403, 1, 799], 1)
    fm, fe = got["rows"], got["ferr"]
    assert fm.shape == fe.shape == (70, 300)
    nan = np.isnan(fm)
    assert nan.any() and not nan.all() and (nan == np.isnan(fe)).all()
    assert np.array_equal(fm[~nan], fe[~nan])


# --------------------------------------------------------------------------------------------------- 4. retune and reset
def test_retune_in_mid_block_and_reset(ctx, restate, ferr_restate):
    bank, T = BANKS["fixed"]
    B, L = 19, 13
    n = 3000
    pushes = [4 * 20 + 1, 4 * 30, 4 * 100 + 2, 1000]
    pushes.append(n - sum(pushes))
    op = out_pushes(pushes, bank.M)
    edges = np.cumsum([0] + op)
    assert edges[2] % L and edges[4] % L                         # the retunes below fall inside blocks
    x = make_input("cs16", n, 9)
    h = taps_for(T, seed=1)
    incs = incs_for(B, 2)
    ret = {2: {3: 0x12345678, 11: 0}, 4: {3: 0xFEDCBA98}}
    z0 = z_rows(restate, bank, x, "cs16", h, incs)
    zr = z_rows(restate, bank, x, "cs16", h, incs, pushes=pushes, retunes=ret)
    mask = segment_table(n, incs, np.uint32, pushes, ret)[2]
    plain, want = ferr_restate(z0, L, op), ferr_restate(zr, L, op, retune=mask)
    others = [b for b in range(B) if b not in (3, 11)]
    assert same_bits(want[others], plain[others]) and not same_bits(want[[3, 11]], plain[[3, 11]])
    for output, dc in (("fm", True), ("iq", False)):
        got = run_ferr(ctx, bank, x, "cs16", h, incs, output, dc, pushes, L, retunes=ret)
        assert same_bits(got["ferr"], want), output
        assert same_bits(got["ferr"][others], plain[others]), output          # every other channel is untouched
    # the retuned channel's block is the chain over the outputs after the retune: the restatement of the outputs from the
    # retune on alone (z[-1] = 0, sums from +0), cut at the block's end
    m, j = int(edges[2]) // L, int(edges[2])
    tail = ferr_restate(np.ascontiguousarray(zr[[3, 11], j:(m + 1) * L]), (m + 1) * L - j, [(m + 1) * L - j])
    assert same_bits(want[[3, 11], m:m + 1], tail)
    # reset: block 0 again, z[-1] = 0, the configuration kept
    cz = make_cz(ctx, bank, "cs16", h, incs, "fm", True, n)
    cz.enable_power(block=L, ferr=True)
    first = run_ferr(ctx, bank, x[:1000], "cs16", h, incs, "fm", True, [333, 667], L, cz=cz)
    cz.reset()
    again = run_ferr(ctx, bank, x, "cs16", h, incs, "fm", True, [n], L, cz=cz)
    cz.close()
    assert again["first"] == [0] and same_bits(again["ferr"], plain)
    assert same_bits(first["ferr"], plain[:, :first["ferr"].shape[1]])


# ------------------------------------------------------------------------------------------------------------ 5. off means off
def test_off_means_off(ctx):
    bank, T = BANKS["fixed"]
    B, L = 7, 5
    pushes = [401, 0, 3, 796]
    x = make_input("cs16", sum(pushes), 13)
    h = taps_for(T)
    incs = incs_for(B, 5)
    lv = (np.float32(0.06), np.float32(0.03), 0)                 # inside the spread of the block powers: gates open and close
    for output, dc in (("fm", True), ("iq", False)):
        on = run_ferr(ctx, bank, x, "cs16", h, incs, output, dc, pushes, L, ferr=True, levels=lv)
        off = run_ferr(ctx, bank, x, "cs16", h, incs, output, dc, pushes, L, ferr=False, levels=lv)
        assert off["ferr"] is None and on["gate"].any() and not on["gate"].all()
        for key in ("rows", "power", "gate", "counts"):
            assert same(on[key], off[key]), (output, key)
        assert on["first"] == off["first"] and on["nblk"] == off["nblk"]


class _OlderCaller(C.Structure):
    """A power configuration followed by memory that belongs to the caller."""
    _fields_ = [("cfg", _capi.ChannelizerPowerConfig), ("behind", C.c_uint8 * 24)]


def test_struct_size_rule(ctx):
    lib, mem = ctx.lib, ctx.mem
    v1, full = _capi.CHANNELIZER_POWER_CONFIG_V1_SIZE, C.sizeof(_capi.ChannelizerPowerConfig)
    assert v1 == _capi.ChannelizerPowerConfig.stride.offset + C.sizeof(C.c_size_t) and full == v1 + C.sizeof(C.c_void_p)
    h = np.ones(8, np.float32)
    cz = api.Channelizer(1.0, 4, [0.0] * 4, h, max_input=1000, ctx=ctx)
    power, gate, counts = mem.zeros((4, 64), np.float32), mem.zeros((4, 64), np.uint8), mem.zeros((4,), np.uint32)
    canary = mem.from_numpy(np.full((4, 64), 0xA5A5A5A5, np.uint32).view(np.float32))

    def caller(size, d_ferr):
        o = _OlderCaller()
        C.memset(C.byref(o), 0xA5, C.sizeof(o))
        o.cfg.struct_size, o.cfg.block, o.cfg.open_level, o.cfg.close_level, o.cfg.hang_blocks = size, 10, 0.0, 0.0, 0
        o.cfg.d_power, o.cfg.d_gate, o.cfg.d_counts, o.cfg.stride = mem.ptr(power), mem.ptr(gate), mem.ptr(counts), 64
        if d_ferr is not None:
            o.cfg.d_ferr = d_ferr
        return o

    def push():
        x = np.full((103, 2), 16384, np.int16)
        n_out = C.c_size_t(0)
        assert lib.dh_channelizer_push_host(cz._h, x.ctypes.data_as(C.c_void_p), 103, mem.ptr(cz.rows), cz.out_stride, C.byref(n_out)) == 0
        assert n_out.value == 25 and host(ctx, gate)[:, :2].all()

    first, nb = C.c_uint64(), C.c_size_t()
    for size in list(range(v1 + 1, full)) + [8, v1 - 1, full + 1, full + 8]:
        assert lib.dh_channelizer_power_enable(cz._h, C.byref(caller(size, None).cfg)) == -1, size
    assert lib.dh_channelizer_power_last(cz._h, C.byref(first), C.byref(nb)) == -1              # still off
    # the older size with 0xA5 in and behind the new field: accepted, the field neither read nor anything written
    o = caller(v1, None)
    before = bytes(o)
    assert bytes(o)[v1:] == b"\xa5" * (C.sizeof(o) - v1)
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(o.cfg)) == 0
    if not hasattr(mem, "torch"):         # on the host tier a library that read the field would now write through 0xA5A5...
        push()
        assert lib.dh_channelizer_reset(cz._h) == 0
    assert bytes(o) == before
    # d_ferr set, with the older size: ignored
    o = caller(v1, mem.ptr(canary).value)
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(o.cfg)) == 0
    push()
    assert (host(ctx, canary).view(np.uint32) == 0xA5A5A5A5).all()
    # ... and with the whole struct: written
    assert lib.dh_channelizer_reset(cz._h) == 0
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(caller(full, mem.ptr(canary).value).cfg)) == 0
    push()
    got = host(ctx, canary).view(np.uint32)
    assert (got[:, :2] == 0).all() and (got[:, 2:] == 0xA5A5A5A5).all()        # a constant input: w real and positive, ferr = +0
    # NULL with the whole struct: off
    assert lib.dh_channelizer_reset(cz._h) == 0
    canary2 = host(ctx, canary).copy()
    assert lib.dh_channelizer_power_enable(cz._h, C.byref(caller(full, 0).cfg)) == 0
    push()
    assert same(host(ctx, canary), canary2)
    cz.close()


# ------------------------------------------------------------------------------------------------------- 6. special operands
@pytest.mark.parametrize("what", ["inf_nan", "zeros", "tiny", "tiny_w"])
def test_special_operands(ctx, restate, ferr_restate, what):
    bank, T = BANKS["fixed"]
    B, L = 9, 7
    pushes = [403, 1, 796]
    op = out_pushes(pushes, bank.M)
    x = make_input("cf32", sum(pushes), 17)
    if what == "inf_nan":
        x[300, 0], x[800, 1], x[810, 0] = np.inf, np.nan, -np.inf
    elif what == "zeros":
        x[:] = 0.0
    elif what == "tiny":
        x *= np.float32(1e-36)                                   # tap products are subnormal, products of two outputs zero
    else:
        x *= np.float32(3e-20)                                   # products of two outputs are subnormal
    h = taps_for(T)
    incs = incs_for(B, 8)
    z = z_rows(restate, bank, x, "cf32", h, incs)
    for block in (L, 1):
        want = ferr_restate(z, block, op)
        if what == "inf_nan":
            assert np.isnan(want).any() and not np.isnan(want).all()
        elif what == "zeros":
            assert want.tobytes() == bytes(want.nbytes)          # ferr = +0 throughout
        else:
            w = np.abs(z[:, 1:, 0].astype(np.float64) * z[:, :-1, 0])
            assert np.abs(z).max() > 0 and (w.max() < 2.0 ** -149 if what == "tiny" else 2.0 ** -149 < np.median(w) < 2.0 ** -126)
            assert (want == 0).all() if what == "tiny" else (want != 0).any()
        for output in ("iq", "fm"):
            got = run_ferr(ctx, bank, x, "cf32", h, incs, output, False, pushes, block)
            assert same_bits(got["ferr"], want), (block, output)
            if block == 1:
                assert (got["ferr"][:, 0] == 0).all()            # z[-1] = 0 at j = 0: w = 0


# --------------------------------------------------------------------------------------------------------------------- 7. a tone
def tone_bound(sum_h, gain, chain, L):
    """Bound on |ferr - 2 delta / rate_out| for an unmodulated carrier A e^(i ...) in float32 input, blocks after the filter
    has filled.  eps_z, the relative error of an output: every term of the chains carries the phasor's tested 1e-6 (1e-9 more
    for a raster's phase word), one rounding of the rotated tap and the rounding of the input sample (sqrt 2 * 2^-24), the
    chain of `chain` fused steps at most chain * 2^-24 of sum|h| A, all relative to |z| = gain A; the final rotation 1e-6 and
    three roundings.  w = z conj(p): 2 eps_z + eps_z^2 and four roundings.  The in-order sums over the block: the terms are
    all W (1 + error), so |sum - L W| <= L |W| (eps_w + sqrt 2 (L - 1) 2^-24).  An error of eps relative in a complex number
    turns its angle by at most asin(eps) <= 1.01 eps (eps < 0.1); divided by pi.  The polynomial: 2e-8 rad, and eleven float
    operations on values below 1.6 (|ferr| <= 1): 16 * 2^-24."""
    u = 2.0 ** -24
    eps_z = sum_h / gain * (1e-6 + 1e-9 + (1.0 + 2.0 ** 0.5 + chain) * u) + 1e-6 + 3 * u
    eps_w = 2 * eps_z + eps_z ** 2 + 4 * u
    eps_s = eps_w + 2.0 ** 0.5 * (L - 1) * u
    assert eps_s < 0.1
    return 1.01 * eps_s / np.pi + 2e-8 / np.pi + 16 * u


TONE_RATE, TONE_D, TONE_L = 768000.0, 16, 100
TONE_BANKS = [("fixed", None, 100000.0), ("fixed", None, -237500.0), ("raster", 64, 96000.0), ("raster", 64, -240000.0)]


@pytest.mark.parametrize("kind,K,centre", TONE_BANKS)
def test_frequency_error_of_a_tone(ctx, restate, ferr_restate, kind, K, centre):
    rate, D, L = TONE_RATE, TONE_D, TONE_L
    rate_out = rate / D
    h = api.channel_taps(rate, D, 6500.0, 12000.0, 60.0)
    T, A, n = len(h), 0.5, 8000
    if kind == "fixed":
        bank, word = fixed(D), api.nco_increment(centre, rate)
        f_ch, chain, fill = word / 2.0 ** 32 * rate, 16 * ((T + 15) // 16), 16 * ((T + 15) // 16)
    else:
        bank, word = raster(K, D), int(round(centre / (rate / K)))
        P = -(-T // K)
        f_ch, chain, fill = word * rate / K, P + 16 * ((K + 15) // 16), P * K
    nn = np.arange(n, dtype=np.float64)
    H = lambda d: np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * d / rate * np.arange(T)))
    sum_h = float(np.abs(h.astype(np.float64)).sum())
    first_full = -(-(-(-fill // D) + 1) // L)                     # first block whose outputs j and j - 1 all have n_j >= the filter's fill
    for delta in (150.0, -150.0, 1234.5, -1234.5, 4000.0, -4000.0):
        xs = A * np.exp(2j * np.pi * (f_ch + delta) / rate * nn)
        x = np.stack([xs.real, xs.imag], 1).astype(np.float32)
        bound = tone_bound(sum_h, abs(H(delta)), chain, L)
        want = 2.0 * delta / rate_out
        z = z_rows(restate, bank, x, "cf32", h, [word])
        ref = ferr_restate(z, L, [n // D])[0].astype(np.float64)
        assert len(ref) == n // D // L and len(ref) > first_full + 2
        err_ref = np.abs(ref[first_full:] - want).max()
        assert err_ref <= bound, ("the restatement", kind, delta, err_ref, bound)      # the bound holds for the text itself
        got = run_ferr(ctx, bank, x, "cf32", h, [word], "fm" if kind == "fixed" else "iq", kind == "fixed", [3000, 5000], L,
                       rate=rate if kind == "fixed" else None)
        fe = got["ferr"][0].astype(np.float64)
        err = np.abs(fe[first_full:] - want).max()
        print("tone %s centre %.0f delta %.1f: |ferr rate / 2 - delta| = %.3g Hz (restatement %.3g Hz), bound %.3g Hz"
              % (kind, centre, delta, err * rate_out / 2, err_ref * rate_out / 2, bound * rate_out / 2))
        assert err <= bound, (kind, delta, err, bound)
        hz = api.frequency_error_hz(got["ferr"][:, first_full:], got["gate"][:, first_full:], rate_out)
        assert abs(hz[0] - delta) <= bound * rate_out / 2


# ------------------------------------------------------------------------------------------------------- 8. a modulated carrier
DMR_D, DMR_SECONDS, DMR_OFFSET_HZ, DMR_L = 8, 0.5, 137.0, 480
DMR_CHANNELS = [25000.0, -50000.0]                               # the carrier's channel, and an empty one
DMR_TOLERANCE_HZ = 2.0 * 115.9


def dmr_scene(seed):
    rate = 48000.0 * DMR_D
    n = int(DMR_SECONDS * rate)
    audio, _ = wideband.dmr_audio(seed, n_calls=1)
    x = wideband.composite(DMR_D, [(DMR_CHANNELS[0] + DMR_OFFSET_HZ, 0.0, audio)], n, seed=seed)
    h = api.channel_taps(rate, DMR_D, 5500.0, 8000.0, 70.0)
    return rate, n, x, h, [api.nco_increment(f, rate) for f in DMR_CHANNELS]


def dmr_restated_error_hz(restate, ferr_restate, seed):
    """|median over the open blocks - the generated offset| of the restatements alone (what DMR_TOLERANCE_HZ was measured with)."""
    rate, n, x, h, incs = dmr_scene(seed)
    z = z_rows(restate, fixed(DMR_D), x, "cs16", h, incs)
    op = [n // DMR_D]
    fe = ferr_restate(z, DMR_L, op)
    _, gate, _ = restate.power(z, DMR_L, np.float32(10.0 ** -2.0), np.float32(10.0 ** -2.3), 2, op)      # -20 / -23 dB
    hz = api.frequency_error_hz(fe, gate, 48000.0)
    return hz, gate


def test_frequency_error_of_a_dmr_carrier(ctx, restate, ferr_restate):
    """One DMR carrier (wideband.dmr_audio, seed 3) 137 Hz off its channel, and an empty channel; gate at -20 / -23 dB, blocks
    of 10 ms; api.frequency_error_hz over the open blocks of 0.5 s.  The block mean of 4FSK data wobbles with the symbols, so
    the tolerance is measured, with the restatements alone (dmr_restated_error_hz, seeds 1 .. 5): the errors were 86.8, 75.0,
    44.0, 27.4 and 115.9 Hz (all upwards: the idle and sync bursts that open the stream do not average to zero), the worst
    115.9 Hz; the tolerance is twice that, 231.8 Hz.  The empty channel gives NaN."""
    seed = 3
    rate, n, x, h, incs = dmr_scene(seed)
    ref, gate = dmr_restated_error_hz(restate, ferr_restate, seed)
    assert gate[0, 1:].all() and not gate[1].any()
    assert abs(ref[0] - DMR_OFFSET_HZ) <= DMR_TOLERANCE_HZ and np.isnan(ref[1])
    cz = api.Channelizer(rate, DMR_D, DMR_CHANNELS, h, input="cs16", output="fm", dcblock=True, max_input=50000, ctx=ctx)
    cz.enable_power(block=DMR_L, open_db=-20.0, close_db=-23.0, hang_blocks=2, ferr=True)
    fe, g = [], []
    for pos in range(0, n, 50000):
        cz.push(x[pos:pos + 50000])
        f_, _ = cz.ferr_blocks()
        _, g_, _ = cz.power_blocks()
        fe.append(host(ctx, f_).copy()); g.append(host(ctx, g_).copy())
    cz.close()
    fe, g = np.concatenate(fe, axis=1), np.concatenate(g, axis=1)
    assert same(g, gate)
    hz = api.frequency_error_hz(fe, g, 48000.0)
    print("DMR carrier: %.1f Hz for %.1f Hz generated (restatement %.1f Hz)" % (hz[0], DMR_OFFSET_HZ, ref[0]))
    assert abs(hz[0] - DMR_OFFSET_HZ) <= DMR_TOLERANCE_HZ
    assert np.isnan(hz[1])


# ----------------------------------------------------------------------------------------------------------- 9. Python surface
def test_python_surface(ctx):
    h = np.ones(8, np.float32)
    cz = api.Channelizer(1.0, 4, [0.0] * 4, h, max_input=1000, ctx=ctx)
    with pytest.raises(DhError):
        cz.ferr_blocks()                                         # before the enable
    assert cz.ferr is None
    cz.enable_power(block=10)
    assert cz.ferr is None and len(cz.power_blocks()) == 3
    with pytest.raises(DhError):
        cz.ferr_blocks()                                         # enabled without ferr
    cz.enable_power(block=10, ferr=True)
    assert cz.ferr.shape == cz.power.shape == (4, 26)
    fe, first = cz.ferr_blocks()
    assert fe.shape == (4, 0) and first == 0
    cz.push(np.full((103, 2), 16384, np.int16))
    fe, first = cz.ferr_blocks()
    pw, g, pfirst = cz.power_blocks()
    assert fe.shape == pw.shape == (4, 2) and first == pfirst == 0
    assert (host(ctx, fe) == 0).all()                            # a constant input sits on its channel
    cz.close()
    with pytest.raises(DhError):
        cz.ferr_blocks()                                         # a closed handle
    with pytest.raises(DhError):
        cz.enable_power(block=10, ferr=True)
    # frequency_error_hz: the median over the open columns, NaN without one
    fe = np.array([[0.5, 0.01, 0.02, 0.03], [0.1, 0.2, 0.3, 0.4], [0.0, -0.5, 0.25, 0.0]], np.float32)
    g = np.array([[0, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0]], np.uint8)
    hz = api.frequency_error_hz(fe, g, 48000.0)
    assert hz.shape == (3,) and hz[0] == np.float64(np.float32(0.02)) * 24000.0 and np.isnan(hz[1]) and hz[2] == -6000.0
    with pytest.raises(ValueError):
        api.frequency_error_hz(fe, g[:, :3], 48000.0)
