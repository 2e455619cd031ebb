"""What the channelizer tests share (test_channelizer.py, _rational.py, _raster.py, _power.py; tools/channelizer_model.py):
the C restatements, the three kinds of bank as data, make_cz / run_lib on top of them, the inputs, the end-to-end scene with
its verdict, and the raw config builder of the validation tests."""
import ctypes as C
import os
import subprocess
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from digiham_amd import _capi, api, wideband

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the three kinds of bank ---------------------------------------------------------------------------------------------
# A bank: rows at input rate * max(L, 1) / M; K bins on a uniform raster (0: none).  A channel's tuning word is its NCO
# increment (uint32), on a raster its bin (int32).
Bank = namedtuple("Bank", "kind L M K")

# What differs between the kinds, as plain functions of the bank; KINDS below names them per kind.
def _increment_hz(bank, rate, u):
    """The frequency that names increment u at creation (the round trip may not be exact: make_cz retunes exactly)."""
    return u * rate / 2.0 ** 32


def _bin_hz(bank, rate, c):
    """Bin c of the raster; with raster_hz = 1 at input_rate = K the frequency is the bin, exactly."""
    return float(c) * (rate / bank.K)


def _retune_increment(ctx, cz, ch, u):
    assert ctx.lib.dh_channelizer_retune(cz._h, ch, int(u)) == 0


def _retune_bin(ctx, cz, ch, c):
    cz.retune(ch, float(c) * cz.raster_hz)            # (raises unless the library returns 0)


def _restated_rational(bank):
    """L = 0 is L = 1 to the library, and the integer channelizer to the restatements."""
    return ("cz_rational_restate", (bank.L, bank.M), ()) if bank.L else ("cz_restate", (bank.M,), ())


Kind = namedtuple("Kind", "cz_args hz exact retune word restatement")
KINDS = {
    "fixed": Kind(
        cz_args=lambda bank, rate: {},                                    # api.Channelizer's arguments beyond decimation = M
        hz=_increment_hz,                                                 # the frequency given for a tuning word at creation
        exact=True,                                                       # ... and the word then written through retune
        retune=_retune_increment,                                         # how a channel is tuned mid-stream
        word=np.uint32,                                                   # the tuning table's type
        restatement=lambda bank: ("cz_restate", (bank.M,), ())),          # C entry point, its arguments before and after (h, T)
    "rational": Kind(
        cz_args=lambda bank, rate: dict(interpolation=bank.L),
        hz=_increment_hz,
        exact=True,
        retune=_retune_increment,
        word=np.uint32,
        restatement=_restated_rational),
    "raster": Kind(
        cz_args=lambda bank, rate: dict(raster_hz=rate / bank.K),
        hz=_bin_hz,
        exact=False,
        retune=_retune_bin,
        word=np.int32,
        restatement=lambda bank: ("cz_raster_restate", (bank.M,), (bank.K,))),
}


def fixed(D):
    return Bank("fixed", 1, D, 0)


def rational(L, M):
    return Bank("rational", L, M, 0)


def raster(K, D):
    return Bank("raster", 1, D, K)


def out_pushes(pushes, M, L=1):
    """Outputs completed by each push of the given input lengths: floor(L (pos + c) / M) - floor(L pos / M)."""
    pos, res = 0, []
    for c in pushes:
        res.append(L * (pos + c) // M - L * pos // M)
        pos += c
    return res


# ---- the restatements ----------------------------------------------------------------------------------------------------
P, U32, I32, SZ = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SEGMENTS = [P, P, P, U32, I32, I32, P]              # seg_start, tuning words, reset, nseg, fm, dcblock, out
ENTRIES = {"cz_restate": [P, I32, SZ, U32, P, U32, U32] + SEGMENTS,
           "cz_rational_restate": [P, I32, SZ, U32, U32, P, U32, U32] + SEGMENTS,
           "cz_raster_restate": [P, I32, SZ, U32, P, U32, U32, U32] + SEGMENTS + [P],
           "cz_power_restate": [P, U32, SZ, U32, P, P, P, P, U32, P, P, P, P]}


def segment_table(n, words, dtype, pushes=None, retunes=None):
    """The stream of n inputs cut into pushes; retunes: {push index: {ch: word}}.  -> starts [nseg] uint64, the words in
    force per push [nseg][B], reset [nseg][B] uint8 (1 where a retune restarts the channel's FM / DC state)."""
    pushes = pushes or [n]
    starts = np.cumsum([0] + list(pushes[:-1])).astype(np.uint64)
    table, reset = np.zeros((len(pushes), len(words)), dtype), np.zeros((len(pushes), len(words)), np.uint8)
    cur = np.array(words, dtype)
    for s in range(len(pushes)):
        for ch, w in (retunes or {}).get(s, {}).items():
            cur[ch] = w
            reset[s, ch] = 1
        table[s] = cur
    return starts, table, reset


class Restate:
    """tests/cz_*.c, each compiled once (the `restate` fixture keeps one instance per process)."""

    def __init__(self, d):
        self.fn = {}
        for name, argtypes in ENTRIES.items():
            so = str(d / ("lib%s.so" % name))
            subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(HERE, name + ".c"),
                            "-o", so, "-lm"], check=True)
            lib = C.CDLL(so)
            self.fn[name] = getattr(lib, name)
            self.fn[name].restype, self.fn[name].argtypes = None, argtypes
            if name == "cz_restate":
                lib.cz_phasor.argtypes = [U32, P, P]
                a, b = C.c_float(), C.c_float()
                lib.cz_phasor(0, C.byref(a), C.byref(b))  # fills the restatement's tables once, before any thread uses them

    def run(self, bank, x, cf32, h, words, fm, dcblock, pushes=None, retunes=None, want_z=False, threads=1):
        """The whole stream through the bank's restatement -> rows [B][n_out] (FM) or [B][n_out][2] (IQ); with want_z
        (rows, z), z the rows before the discriminator.  words: [B] increments or bins at the start; pushes: the push lengths
        (for retunes); retunes: {push index: {ch: word}}; threads: the channels are split over that many calls."""
        name, before, after = KINDS[bank.kind].restatement(bank)
        assert threads <= 1 or name == "cz_restate", "only cz_restate.c's tables are filled before the threads start"
        x = np.ascontiguousarray(x)
        n, B = x.size // 2, len(words)
        starts, table, reset = segment_table(n, words, KINDS[bank.kind].word, pushes, retunes)
        h = np.ascontiguousarray(h, np.float32)
        n_out = max(bank.L, 1) * n // bank.M
        out = np.zeros((B, n_out) if fm else (B, n_out, 2), np.float32)
        z = np.zeros((B, n_out, 2), np.float32) if want_z and bank.K else None

        def one(lo, hi):
            t, r = np.ascontiguousarray(table[:, lo:hi]), np.ascontiguousarray(reset[:, lo:hi])
            tail = (starts.ctypes.data, t.ctypes.data, r.ctypes.data, len(starts), int(fm), int(dcblock), out[lo:hi].ctypes.data)
            if bank.K:
                tail += (z[lo:hi].ctypes.data if want_z else None,)
            self.fn[name](x.ctypes.data, int(cf32), n, *before, h.ctypes.data, len(h), *after, hi - lo, *tail)

        if threads <= 1:
            one(0, B)
        else:
            cuts = np.linspace(0, B, min(threads, B) + 1).astype(int)
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(lambda k: one(int(cuts[k]), int(cuts[k + 1])), range(len(cuts) - 1)))
        if want_z and not bank.K:                     # these restatements' z rows are their IQ rows
            z = self.run(bank, x, cf32, h, words, False, False, pushes, retunes, threads=threads) if fm else out
        return (out, z) if want_z else out

    def power(self, z, block, open_level, close_level, hang, out_pushes, retune=None):
        """-> power [B][n // block] float32, gate [B][n // block] uint8, counts [npush][B] uint32.  Levels and hang: a scalar,
        or one value per push; retune: the reset table of the run that made z."""
        z = np.ascontiguousarray(z, np.float32)
        B, n, npush = z.shape[0], z.shape[1], len(out_pushes)
        assert sum(out_pushes) <= n
        per = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (npush,)))
        ol, cl, hg = per(open_level, np.float32), per(close_level, np.float32), per(hang, np.uint32)
        pl = np.array(out_pushes, np.uint64)
        rt = np.zeros((npush, B), np.uint8) if retune is None else np.ascontiguousarray(retune, np.uint8)
        power, gate = np.zeros((B, n // block), np.float32), np.zeros((B, n // block), np.uint8)
        counts = np.zeros((npush, B), np.uint32)
        self.fn["cz_power_restate"](z.ctypes.data, B, n, block, ol.ctypes.data, cl.ctypes.data, hg.ctypes.data, pl.ctypes.data, npush,
                                    rt.ctypes.data, power.ctypes.data, gate.ctypes.data, counts.ctypes.data)
        return power, gate, counts


_restate = []


@pytest.fixture(scope="session")
def restate(tmp_path_factory):
    if not _restate:                                  # (a fixture imported into four modules is instantiated in each)
        _restate.append(Restate(tmp_path_factory.mktemp("cz")))
    return _restate[0]


# ---- the library -----------------------------------------------------------------------------------------------------------
def host(ctx, a):
    return np.asarray(ctx.mem.to_numpy(a))


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def make_cz(ctx, bank, fmt, h, words, output, dc, max_input, rate=None):
    """rate: 1.0, on a raster K (with raster_hz = 1: a channel's frequency is its bin, exactly)."""
    kind = KINDS[bank.kind]
    rate = rate or float(bank.K or 1)
    cz = api.Channelizer(rate, bank.M, [kind.hz(bank, rate, w) for w in words], h, input=fmt, output=output, dcblock=dc,
                         max_input=max_input, ctx=ctx, **kind.cz_args(bank, rate))
    if kind.exact:
        for ch, w in enumerate(words):
            kind.retune(ctx, cz, ch, w)
    return cz


def run_lib(ctx, bank, x, fmt, h, words, output, dc, pushes=None, retunes=None, rate=None, cz=None, power=None, check_last=True,
            keep_rows=True):
    """Push x in the given lengths; every push must complete out_pushes' count and every retune succeed.  Returns the
    concatenated rows.
    power = (block, levels), levels (open, close, hang) as float32 levels (not dB), or one such triple per push (a cz of the
    caller's has its power enabled already): returns dict(rows, power, gate: concatenated over the pushes; counts [npush][B];
    first, nblk per push), and with check_last asserts the host arithmetic of dh_channelizer_power_last."""
    flat = np.ascontiguousarray(x).reshape(-1, 2)
    pushes = pushes or [len(flat)]
    op = out_pushes(pushes, bank.M, max(bank.L, 1))
    own = cz is None
    if own:
        cz = make_cz(ctx, bank, fmt, h, words, output, dc, max(max(pushes), 1), rate)
        if power:
            cz.enable_power(block=power[0])
    per_push = power and isinstance(power[1][0], (tuple, list))
    res = dict(rows=[], power=[], gate=[], counts=[], first=[], nblk=[])
    pos = 0
    for s, c in enumerate(pushes):
        for ch, w in (retunes or {}).get(s, {}).items():
            KINDS[bank.kind].retune(ctx, cz, ch, w)
        if power:
            open_level, close_level, hang = power[1][s] if per_push else power[1]
            assert ctx.lib.dh_channelizer_set_squelch(cz._h, float(open_level), float(close_level), int(hang)) == 0
        rows, k = cz.push(np.ascontiguousarray(flat[pos:pos + c]))
        assert k == op[s], (s, k)
        res["rows"].append(host(ctx, rows)[:, :k].copy() if keep_rows else np.zeros((len(words), 0), np.float32))
        if power:
            pw, g, first = cz.power_blocks()
            res["power"].append(host(ctx, pw).copy())
            res["gate"].append(host(ctx, g).copy())
            res["counts"].append(host(ctx, cz.counts).view(np.uint32).copy())
            res["first"].append(first)
            res["nblk"].append(pw.shape[1])
            if check_last:
                j0, L = max(bank.L, 1) * pos // bank.M, power[0]
                assert first == j0 // L and pw.shape[1] == (j0 + k) // L - j0 // L and g.shape[1] == pw.shape[1], (s, first, pw.shape)
        pos += c
    if own:
        cz.close()
    if not power:
        return np.concatenate(res["rows"], axis=1)
    for key in ("rows", "power", "gate"):
        res[key] = np.concatenate(res[key], axis=1)
    res["counts"] = np.stack(res["counts"])
    return res


# ---- inputs ----------------------------------------------------------------------------------------------------------------
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


def bins_for(B, K, seed):
    """0, K/2, -1, K-1, -K/2 and a duplicate first, then bins from four turns of the raster."""
    edge = [0, K // 2, -1, K - 1, -(K // 2), K // 2]
    extra = [int(v) for v in np.random.default_rng(seed).integers(-2 * K, 2 * K, max(B - len(edge), 0))]
    return (edge + extra)[:B]


def taps_for(T, scale=0.05, seed=None):
    return np.random.default_rng(T if seed is None else seed).standard_normal(T).astype(np.float32) * scale


# ---- the end-to-end scene and its verdict ------------------------------------------------------------------------------
STRONG, WEAK, YSF_ROW = 4, 5, 1
LEVELS_DB = {STRONG: 0.0, WEAK: -20.0, 0: -30.0, YSF_ROW: -20.0}


def end_to_end_fixture(L, M, n_rows, seconds, device, seed=7, raster_hz=12500.0, noise_device=None, key=None,
                        levels=LEVELS_DB, ysf_row=YSF_ROW):
    """Composite at the capture rate 48 kS/s * M / L on a raster of raster_hz: DMR carriers at 0 .. -30 dB with small offsets,
    one YSF row, two empty rows, a strong carrier next to one 20 dB weaker (FM capture sets that limit: a neighbour's
    spectral skirt inside the passband takes the discriminator over at about -30 dB).  tools/channelizer_model.py runs its
    float64 models on the same.  noise_device "cpu": with a device, the carriers are summed there and the noise still comes
    from the CPU generator, so a seed names the same noise on both tiers.  key = (on, off) in seconds keys every carrier, its
    audio starting at key-on.  levels: row -> dB for the rows that are not drawn.
    -> dict(rate, n, raster, raster_hz, x, h, meta, ysf_row, empty, carriers)."""
    rate = 48000.0 * M / L
    n = int(seconds * rate)
    half = n_rows // 2
    raster = [(r - half) * raster_hz for r in range(n_rows)]
    rng = np.random.default_rng(n_rows)
    empty = {2, n_rows - 2}
    carriers, meta = [], {}
    for r in range(n_rows):
        if r in empty:
            continue
        off = raster[r] + float(rng.uniform(-150, 150))
        level = levels.get(r, float(rng.uniform(-20, -5)))               # (drawn for every row, used or not)
        if r == ysf_row:
            audio = wideband.ysf_audio(100 + r, 30)
        else:
            audio, meta[r] = wideband.dmr_audio(100 + r, n_calls=1 if seconds < 2.5 else 2)
            meta[r]["level_db"] = level
        carriers.append((off, level, audio))
    more = dict(noise_device=noise_device) if noise_device else {}
    if key:
        more["keying"] = [key] * len(carriers)
    x = wideband.composite(M / L, carriers, n, seed=seed, device=device, **more)
    h = api.channel_taps(rate, M, 5500.0, 8000.0, 70.0, interpolation=L)      # a neighbour 30 dB stronger must stay out of the passband
    return dict(rate=rate, n=n, raster=raster, raster_hz=raster_hz, x=x, h=h, meta=meta, ysf_row=ysf_row, empty=empty, carriers=carriers)


def check_dmr_row(r, e, ref, i, meta):
    """Row r's events e == row i of oracle.chain's; meta None: an empty row, no sync; else every LC has the generated ids,
    and there are at least as many syncs as generated voice superframes."""
    assert len(e) == ref["event_count"][i] and e.tobytes() == ref["events"][i, :len(e)].tobytes(), "row %d differs from the oracle" % r
    if meta is None:
        assert not (e["type"] == 1).any(), "empty row %d: sync events" % r
        return
    lcs = [api.parse_lc(p) for p in e[e["type"] == 4]["payload"]]
    assert lcs, "row %d: no LC" % r
    assert all(l["source"] == meta["src"] and l["target"] == meta["dst"] for l in lcs), "row %d: wrong ids" % r
    assert (e["type"] == 1).sum() >= meta["superframes"], "row %d: fewer syncs than generated voice superframes" % r


def check_rows(ctx, oracle, audio, f):
    """The channelizer's rows of the scene f through DMR / YSF engines == oracle.chain on the same rows, ids and sync counts."""
    k, ysf_row = audio.shape[1], f["ysf_row"]
    dmr_rows = [r for r in range(len(audio)) if r != ysf_row]
    eng = api.Engine(len(dmr_rows), k, proto="dmr", ctx=ctx)
    eng.push(ctx.mem.from_numpy(audio[dmr_rows]))
    ev, ec = eng.events()
    ref = oracle.chain(audio[dmr_rows], proto=1)
    for i, r in enumerate(dmr_rows):
        assert (r in f["empty"]) != (r in f["meta"])
        check_dmr_row(r, ev[i, :ec[i]], ref, i, f["meta"].get(r))
    eng.close()
    yeng = api.Engine(1, k, proto="ysf", ctx=ctx)
    yeng.push(ctx.mem.from_numpy(audio[ysf_row:ysf_row + 1]))
    yev, yec = yeng.events()
    yref = oracle.chain(audio[ysf_row:ysf_row + 1], proto=2)
    assert yec[0] == yref["event_count"][0] and yev[0, :yec[0]].tobytes() == yref["events"][0, :yec[0]].tobytes()
    assert (yev[0, :yec[0]]["type"] == 16).sum() > 10, "YSF row: FICH events missing"
    yeng.close()


def end_to_end(ctx, oracle, bank, f):
    """The scene f in one push through the bank (FM + DC) -> check_rows."""
    assert not bank.K or f["rate"] / bank.K == f["raster_hz"], "the bank's raster is not the scene's"
    cz = api.Channelizer(f["rate"], bank.M, f["raster"], f["h"], input="cs16", output="fm", dcblock=True, max_input=f["n"], ctx=ctx,
                         **KINDS[bank.kind].cz_args(bank, f["rate"]))
    rows, k = cz.push(f["x"])
    assert k == max(bank.L, 1) * f["n"] // bank.M
    audio = np.ascontiguousarray(host(ctx, rows)[:, :k])
    cz.close()
    check_rows(ctx, oracle, audio, f)


# ---- the raw configuration of the validation tests -----------------------------------------------------------------------
POINTERS = {"taps": C.c_float, "increments": C.c_uint32, "bins": C.c_int32}
CFG_TAPS, CFG_INCREMENTS = np.ones(8, np.float32), np.zeros(4, np.uint32)


def cfg(ctx, **fields):
    """A dh_channelizer_config of four channels at increment 0, D = 4, eight taps of 1.0, CS16 -> FM + DC, max_input 1000,
    no interpolation, no raster; fields replace its members.  An array given for a pointer member is held by the returned
    struct (`_arrays`): a ctypes pointer field does not keep numpy's array alive.  struct_size: a caller built against an
    older, shorter struct."""
    c = _capi.ChannelizerConfig(C.sizeof(_capi.ChannelizerConfig), 0, 4, 4, None, 8, None, 1, 2, 1, 1000, ctx.mem.stream())
    c._arrays = []
    for k, v in dict(dict(taps=CFG_TAPS, increments=CFG_INCREMENTS), **fields).items():
        if isinstance(v, np.ndarray):
            c._arrays.append(v)
            v = v.ctypes.data_as(C.POINTER(POINTERS[k]))
        setattr(c, k, v)
    return c


def create(ctx, c):
    """dh_channelizer_create's return code; the handle is destroyed, or was never written."""
    hh = C.c_void_p()
    rc = ctx.lib.dh_channelizer_create(C.byref(c), C.byref(hh))
    if rc == 0:
        ctx.lib.dh_channelizer_destroy(hh)
    else:
        assert not hh.value
    return rc
