"""Protocol scan (proto="scan", include/digiham_amd.h "Protocol scan"): the nine sync patterns of the five protocols,
tested at every symbol position and counted.

The checker `model` below is a plain numpy restatement of the specification -- distances, the position that is examined
when symbol p + 31 has arrived, events, statistics, families, periods, the two-entry history -- and never calls the
engine.  Every test holds the engine (CPU wave emulation, and the MI355X library under -m gpu) to it byte for byte:
hand-planted edges on symbols, invariance under how the stream is cut, reset of one channel, the four demodulator front
ends on synthetic transmissions of all five protocols, and 512 channels at once on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

from digiham_amd import _capi, _taps, api, synth

EV_SCAN_HIT = 80
STAT = np.dtype([("hits", "<u4"), ("periodic", "<u4"), ("last_sym", "<u4"), ("best_dist", "u1"), ("pad", "u1", (3,))])
SPAN = 32                                     # position p is examined once symbol p + 31 is there

# the patterns as symbols (dibits, or bits for D-Star and POCSAG), their distance limits, families and periods
PATTERNS = [np.array(synth.DMR_SYNC[k], np.uint8) for k in ("bs_data", "bs_voice", "ms_data", "ms_voice")] + [
    np.array(synth.YSF_SYNC, np.uint8), np.array(synth.NXDN_SYNC, np.uint8),
    np.array([int(c) for c in "010101010" + "111011001010000"], np.uint8),          # the end of the bit sync + the frame sync
    np.array(synth.DSTAR_VOICE_SYNC, np.uint8),
    np.array(synth._bits_of(synth.POCSAG_SYNC, 32), np.uint8)]
LIMIT = [3, 3, 3, 3, 3, 2, 2, 1, 3]
FAMILY = [0, 0, 0, 0, 1, 2, 3, 3, 4]
PERIODS = [(144, 288), (480,), (192,), (2016,), (544,)]
NAMES = ["dmr", "ysf", "nxdn", "dstar", "pocsag"]
assert [len(p) for p in PATTERNS] == [24, 24, 24, 24, 20, 10, 24, 24, 32]
_POPC2 = np.array([0, 1, 1, 2], np.int32)


def distances(syms, pid):
    """distance of pattern pid at every examined position of the stream: differing bits, both bits of a symbol counted"""
    syms = np.asarray(syms, np.uint8)
    n = len(syms) - SPAN + 1
    if n <= 0:
        return np.zeros(0, np.int32)
    pat = PATTERNS[pid]
    w = np.lib.stride_tricks.sliding_window_view(syms, len(pat))[:n]
    return _POPC2[w ^ pat].sum(axis=1)


def model(syms, base=0):
    """(events, statistics[9]) of a stream of symbols that starts at position `base`, pushed whole"""
    hits = []
    for pid in range(9):
        d = distances(syms, pid)
        for p in np.nonzero(d <= LIMIT[pid])[0]:
            hits.append((int(p), pid, int(d[p])))
    hits.sort()
    st = np.zeros(9, STAT)
    st["best_dist"] = 255
    ev = np.zeros(len(hits), api.EVENT_DTYPE)
    hist = [[] for _ in PERIODS]                         # most recent first, two entries
    i = 0
    while i < len(hits):
        j = i
        while j < len(hits) and hits[j][0] == hits[i][0]:
            j += 1
        p = (hits[i][0] + base) & 0xFFFFFFFF
        for k in range(i, j):                            # all patterns at p against the history before p
            _, pid, d = hits[k]
            f = FAMILY[pid]
            st[pid]["hits"] += 1
            st[pid]["periodic"] += any(((p - q) & 0xFFFFFFFF) in PERIODS[f] for q in hist[f])
            st[pid]["last_sym"] = p
            st[pid]["best_dist"] = min(int(st[pid]["best_dist"]), d)
            ev[k]["sym_index"], ev[k]["type"], ev[k]["a"], ev[k]["b"] = p, EV_SCAN_HIT, pid, d
        for f in sorted({FAMILY[hits[k][1]] for k in range(i, j)}):
            hist[f] = [p] + hist[f][:1]
        i = j
    return ev, st


def family_periodic(st):
    return [int(sum(st[pid]["periodic"] for pid in range(9) if FAMILY[pid] == f)) for f in range(len(PERIODS))]


def read_stats(eng):
    rows, counts = eng.frames()
    assert (counts == 9 * STAT.itemsize).all()
    return np.ascontiguousarray(rows[:, :9 * STAT.itemsize]).view(STAT)


def push_symbol_rows(eng, rows, cuts, starved=None, reset_at=None):
    """rows[B][n] through push_symbols in pushes of cuts[k % len(cuts)] symbols; channel `starved` brings nothing on every
    other push.  reset_at = (channel, push index): reset_channel before that push.  Returns (events per channel and push,
    final statistics, the cut positions of every channel)."""
    B, n = rows.shape
    cur = np.zeros(B, np.int64)
    evs = [[] for _ in range(B)]
    bounds = [[] for _ in range(B)]
    k = 0
    while (cur < n).any() or k == 0:
        c = cuts[k % len(cuts)]
        cnt = np.minimum(c, n - cur)
        if starved is not None and k % 2 == 1:
            cnt[starved] = 0
        if reset_at is not None and reset_at[1] == k:
            eng.reset_channel(reset_at[0])
        buf = np.zeros((B, max(c, 4)), np.uint8)
        for b in range(B):
            buf[b, :cnt[b]] = rows[b, cur[b]:cur[b] + cnt[b]]
        eng.push_symbols(buf, cnt.astype(np.uint32))
        e, ec = eng.events()
        for b in range(B):
            evs[b].append(e[b, :ec[b]].copy())
            bounds[b].append(int(cur[b] + cnt[b]))
        cur += cnt
        k += 1
    return evs, read_stats(eng), bounds


def cat(parts):
    return np.concatenate(parts) if parts else np.zeros(0, api.EVENT_DTYPE)


# ----------------------------------------------------------------------------- planted rows
T = 704                                       # symbols per planted row


def filler(rng, n):
    """symbols no pattern is made of: bit 0 clear -- at least 8 bits away from every pattern wherever they stand alone"""
    return rng.choice(np.array([0, 2], np.uint8), n)


def with_errors(pid, nerr, rng, high=False):
    """pattern pid with nerr wrong bits, each in another symbol; high: one of them is bit 1 of a symbol (a symbol 2 or 3
    where the pattern is made of bits)"""
    s = PATTERNS[pid].copy()
    at = rng.choice(len(s), nerr, replace=False)
    for i, a in enumerate(at):
        s[a] ^= 2 if (high and i == 0) else 1
    return s


def plant(row, p, s):
    row[p:p + len(s)] = s


def _edge_rows():
    """(rows, expectations): expectations are (row, position, pattern, distance or None for "no hit") the MODEL has to
    agree with before the engine is asked anything"""
    rng = np.random.default_rng(2024)
    rows, expect = [], []
    for pid in range(9):
        two_level = pid >= 6
        for positions in ((0, 32, 64, T - 32), (1, 63), (31,)):
            r = filler(rng, T)
            for p in positions:
                plant(r, p, PATTERNS[pid]); expect.append((len(rows), p, pid, 0))
            rows.append(r)
        r = filler(rng, T + 1)                                    # T - 31: examined only when symbol T arrives
        plant(r, T - 31, PATTERNS[pid])
        expect.append((len(rows), T - 31, pid, "late"))
        # exactly the limit of wrong bits: a hit of that distance; one more: none
        plant(r, 40, with_errors(pid, LIMIT[pid], rng, high=two_level)); expect.append((len(rows), 40, pid, LIMIT[pid]))
        plant(r, 120, with_errors(pid, LIMIT[pid] + 1, rng, high=two_level)); expect.append((len(rows), 120, pid, None))
        rows.append(r)
    # DMR: 144 and 288 behind a hit are periodic, 145 is not
    r = filler(rng, T)
    for p, pid in ((20, 0), (164, 1), (452, 2), (597, 3)):
        plant(r, p, PATTERNS[pid])
    rows.append(r); periodic = {len(rows) - 1: {0: 0, 1: 1, 2: 1, 3: 0}}
    # NXDN: the partner is the OLDER of the two remembered positions
    r = filler(rng, T)
    for p in (50, 150, 242):
        plant(r, p, PATTERNS[5])
    rows.append(r); periodic[len(rows) - 1] = {5: 1}
    # ... and here it has left the history: two hits in between
    r = filler(rng, T)
    for p in (50, 100, 150, 242):
        plant(r, p, PATTERNS[5])
    rows.append(r); periodic[len(rows) - 1] = {5: 0}
    rows = [np.concatenate([r, filler(rng, T + 1 - len(r))]) for r in rows]       # (the extra symbol of the late rows: pushed last)
    return np.stack(rows), expect, periodic


@pytest.fixture(scope="module")
def edges():
    rows, expect, periodic = _edge_rows()
    want = [model(r[:T]) for r in rows]
    late = [model(r) for r in rows]
    # the model itself says what the rows were built to show
    for row, p, pid, d in expect:
        found = {(int(e["sym_index"]), int(e["a"])): int(e["b"]) for e in want[row][0]}
        if d == "late":
            assert (p, pid) not in found and (p, pid) in {(int(e["sym_index"]), int(e["a"])) for e in late[row][0]}
        elif d is None:
            assert (p, pid) not in found
        else:
            assert found.get((p, pid)) == d, (row, p, pid, d)
    for row, per in periodic.items():
        for pid, k in per.items():
            assert want[row][1][pid]["periodic"] == k and want[row][1][pid]["hits"] >= 1, (row, pid)
    return rows, want, late


def _groups(n, B=4):
    return [list(range(i, min(i + B, n))) for i in range(0, n, B)]


def test_symbol_level_edges(ctx, edges):
    rows, want, late = edges
    eng = api.Engine(4, 64, rrc="none", demod="none", proto="scan", ctx=ctx)
    for g in _groups(len(rows)):
        idx = g + [g[-1]] * (4 - len(g))
        eng.reset()
        evs, st, _ = push_symbol_rows(eng, rows[idx][:, :T], [T])
        for b, r in enumerate(idx):
            assert cat(evs[b]).tobytes() == want[r][0].tobytes(), r
            assert st[b].tobytes() == want[r][1].tobytes(), r
        # one more symbol: position T - 31 is examined now, and only it
        eng.push_symbols(np.ascontiguousarray(np.repeat(rows[idx][:, T:T + 1], 4, axis=1)), np.ones(4, np.uint32))
        e, ec = eng.events()
        st = read_stats(eng)
        for b, r in enumerate(idx):
            assert e[b, :ec[b]].tobytes() == late[r][0][len(want[r][0]):].tobytes(), r
            assert st[b].tobytes() == late[r][1].tobytes(), r
    eng.close()


# ----------------------------------------------------------------------------- cuts
CUTS = [1, 7, 31, 32, 33, 64, 0, 65]


def _cut_rows():
    """four rows with a pattern every 41 symbols, all nine in turn"""
    rng = np.random.default_rng(7)
    rows, plants = [], []
    for r in range(4):
        row = filler(rng, T)
        for k in range((T - 40) // 41):
            pid = (k + 2 * r) % 9
            plant(row, 5 + 41 * k + r, PATTERNS[pid]); plants.append((r, 5 + 41 * k + r, pid))
        rows.append(row)
    return np.stack(rows), plants


def test_cut_invariance(ctx):
    rows, plants = _cut_rows()
    want = [model(r) for r in rows]
    assert all(w[1]["hits"].sum() >= 14 for w in want)
    eng = api.Engine(4, 80, rrc="none", demod="none", proto="scan", ctx=ctx)
    evs, st, bounds = push_symbol_rows(eng, rows, CUTS, starved=3)
    for pid in range(9):                                  # every pattern starts in one push and ends in a later one
        assert any(p < c < p + len(PATTERNS[pid]) for r, p, q in plants if q == pid for c in bounds[r]), pid
    assert any(len(e) == 0 for e in evs[0]) and len(evs[0]) > 20
    eng.close()
    eng = api.Engine(4, T, rrc="none", demod="none", proto="scan", ctx=ctx)
    evs1, st1, _ = push_symbol_rows(eng, rows, [T])
    eng.close()
    for b in range(4):
        assert cat(evs[b]).tobytes() == cat(evs1[b]).tobytes() == want[b][0].tobytes(), b
        assert st[b].tobytes() == st1[b].tobytes() == want[b][1].tobytes(), b


def test_carry_seam_at_every_carry_length(ctx):
    """The scan keeps the symbols whose position could not be examined yet in the channel's carry row (dh_channel_carry_out /
    dh_channel_open): fewer than SPAN of them.  SPAN + 1 channels carry the same row, which opens with a sync word; channel b's first
    push ends b symbols into it, its second push brings the rest.  Between them the channels leave every carry length the scan can
    leave, 0 .. SPAN - 1, and every channel's events and statistics are the model's for the whole row."""
    rows, _ = _cut_rows()
    row = rows[0].copy()
    plant(row, 0, PATTERNS[8])
    want_ev, want_st = model(row)
    B = SPAN + 1
    cuts = np.arange(B)
    eng = api.Engine(B, T, rrc="none", demod="none", proto="scan", ctx=ctx)
    rest = np.zeros((B, T), np.uint8)
    for b in range(B):
        rest[b, :T - b] = row[b:]
    evs = [[] for _ in range(B)]
    eng.push_symbols(np.ascontiguousarray(np.broadcast_to(row[:SPAN], (B, SPAN))), cuts.astype(np.uint32))
    e, ec = eng.events()
    carried = eng.debug_header(100 + 23)                  # DS_CARRY (decoder_core.hpp)
    for b in range(B):
        evs[b].append(e[b, :ec[b]].copy())
    eng.push_symbols(rest, (T - cuts).astype(np.uint32))
    e, ec = eng.events()
    st = read_stats(eng)
    eng.close()
    assert carried.tolist() == [min(b, SPAN - 1) for b in range(B)]
    for b in range(B):
        evs[b].append(e[b, :ec[b]].copy())
        assert cat(evs[b]).tobytes() == want_ev.tobytes(), b
        assert st[b].tobytes() == want_st.tobytes(), b


def test_empty_push_and_no_events(ctx):
    rows, _ = _cut_rows()
    want = [model(r) for r in rows]
    eng = api.Engine(4, T, rrc="none", demod="none", proto="scan", events=False, ctx=ctx)
    eng.push_symbols(rows, np.full(4, T, np.uint32))
    eng.push_symbols(rows, np.zeros(4, np.uint32))        # nothing new: the statistics are rewritten as they were
    st = read_stats(eng)
    for b in range(4):
        assert st[b].tobytes() == want[b][1].tobytes()
    eng.close()


def test_event_overflow_keeps_counting(ctx):
    """more hits than the event row holds: DH_ECAPACITY's flag, truncated events, complete statistics"""
    n = 64 * 44
    row = np.concatenate([np.tile(PATTERNS[5], n // 10), np.zeros(n % 10, np.uint8)])[None, :]   # NXDN sync words back to back
    ev, st = model(row[0])
    eng = api.Engine(1, n, rrc="none", demod="none", proto="scan", ctx=ctx)
    cap = eng.events()[0].shape[1]
    assert cap == (512 + n) // 16 + 16 and len(ev) > cap
    eng.push_symbols(row, np.full(1, n, np.uint32))
    with pytest.raises(api.DhError) as err:               # reported by the synchronisation behind the push, as for every protocol
        eng.sync()
    assert err.value.code == _capi.DH_ECAPACITY
    lib, views = ctx.lib, eng.device_views()
    e, ec, fr = np.zeros(cap, api.EVENT_DTYPE), np.zeros(1, np.uint32), np.zeros(9, STAT)
    for dst, src in ((e, views["events"][0]), (ec, views["events"][2]), (fr, views["frames"][0])):
        assert lib.dh_copy_to_host(dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), dst.nbytes) == 0
    assert ec[0] == cap and e.tobytes() == ev[:cap].tobytes()
    assert fr.tobytes() == st.tobytes()
    eng.close()


def test_reset_channel(ctx):
    rows, _ = _cut_rows()
    eng = api.Engine(4, 80, rrc="none", demod="none", proto="scan", ctx=ctx)
    K = 9                                                 # reset before push 9: channel 1 has had 1 + 7 + 31 + 32 + 33 + 64 + 0 + 65 + 1 symbols
    at = sum(CUTS) + CUTS[0]
    evs, st, bounds = push_symbol_rows(eng, rows, CUTS, reset_at=(1, K))
    eng.close()
    assert bounds[1][K - 1] == at
    for b in (0, 2, 3):                                   # the neighbours never noticed
        ev, s = model(rows[b])
        assert cat(evs[b]).tobytes() == ev.tobytes() and st[b].tobytes() == s.tobytes()
    before, _ = model(rows[1][:at])
    after, s = model(rows[1][at:])                        # a new stream: positions, history and statistics from zero
    assert len(before) and len(after)
    assert cat(evs[1][:K]).tobytes() == before.tobytes()
    assert cat(evs[1][K:]).tobytes() == after.tobytes() and st[1].tobytes() == s.tobytes()


# ----------------------------------------------------------------------------- through the slicers
FRONTS = {"wide10": dict(rrc="wide", demod="gfsk", sps=10, invert=False),
          "narrow20": dict(rrc="narrow", demod="gfsk", sps=20, invert=False),
          "fsk10": dict(rrc="none", demod="fsk", sps=10, invert=False),
          "fsk40i": dict(rrc="none", demod="fsk", sps=40, invert=True)}
SOURCE = ["wide10"] * 5 + ["narrow20", "fsk10", "fsk10", "fsk40i"]
N_SAMPLES = 90000                   # D-Star: header + 3 x 2016 bits at 10 samples; POCSAG: 576 + 3 x 544 bits at 40 samples


def protocol_rows():
    """[7][N_SAMPLES]: DMR, YSF, NXDN48, D-Star, POCSAG as their own front ends receive them, noise, silence"""
    rng = np.random.default_rng(99)
    dmr = synth.impair(synth.shape(synth.dmr_stream(31, 64)), 1, snr_db=24, dc=0.05, delay=3)
    ysf = synth.impair(synth.shape(synth.ysf_stream(32, 20)), 2, snr_db=22, dc=-0.05, delay=5, gain=0.8)
    nxdn = synth.impair(synth.shape(synth.nxdn_stream(33, 25), sps=20, taps=_taps.narrow()), 3, snr_db=24, delay=7)
    bits, _, _ = synth.dstar_transmission(np.random.default_rng(34), n_superframes=4)
    dstar = synth.impair(synth.fsk_shape(np.concatenate([rng.integers(0, 2, 41).astype(np.uint8), bits]), sps=10), 4, snr_db=22, dc=0.03)
    text = lambda n: "".join(chr(int(c)) for c in rng.integers(32, 127, n))
    words = synth.pocsag_batches([(int(rng.integers(8, 1 << 21)), 3, text(39)) for _ in range(5)])
    assert len(words) >= 4 * 16
    pbits = [1, 0] * 288
    for i in range(0, len(words), 16):
        for w in [synth.POCSAG_SYNC] + words[i:i + 16]:
            pbits += synth._bits_of(w, 32)
    pocsag = synth.impair(synth.fsk_shape(np.array(pbits, np.uint8), sps=40, invert=True), 5, snr_db=22, dc=0.02, delay=11)
    noise = rng.normal(0, 0.3, N_SAMPLES).astype(np.float32)
    rows = []
    for x in (dmr, ysf, nxdn, dstar, pocsag, noise, np.zeros(N_SAMPLES, np.float32)):
        assert len(x) >= N_SAMPLES - 4000, len(x)
        rows.append(np.concatenate([x[:N_SAMPLES], np.zeros(max(0, N_SAMPLES - len(x)), np.float32)]))
    return np.stack(rows)


def run_front(ctx, x, front, proto, chunks, counts_of=None):
    """x through Engine(proto) behind one front end, in ragged chunks (row b brings counts_of(push, b, c) <= c samples of
    each chunk; default: all).  Returns symbols, events per channel and the final statistics row."""
    B, n = x.shape
    eng = api.Engine(B, max(chunks), proto=proto, ctx=ctx, **FRONTS[front])
    syms, evs = [[] for _ in range(B)], [[] for _ in range(B)]
    cur = np.zeros(B, np.int64)
    k = 0
    while (cur < n).any():
        c = chunks[k % len(chunks)]
        cnt = np.minimum(c, n - cur)
        if counts_of is not None:
            cnt = np.minimum(cnt, [counts_of(k, b, c) for b in range(B)])
        buf = np.zeros((B, c), np.float32)
        for b in range(B):
            buf[b, :cnt[b]] = x[b, cur[b]:cur[b] + cnt[b]]
        eng.push(buf, n=c, counts=cnt.astype(np.uint32))
        cur += cnt
        k += 1
        s, sc = eng.symbols()
        for b in range(B):
            syms[b].append(s[b, :sc[b]].copy())
        if proto == "scan":
            e, ec = eng.events()
            for b in range(B):
                evs[b].append(e[b, :ec[b]].copy())
    st = read_stats(eng) if proto == "scan" else None
    eng.close()
    return [np.concatenate(s) for s in syms], [cat(e) for e in evs], st


_SHARED = {}                                  # computed once per session, for tests/test_scanner_api.py too; never modified


@pytest.fixture(scope="module")
def rows7():
    if "x" not in _SHARED:
        _SHARED["x"] = protocol_rows()
        _SHARED["x"].setflags(write=False)
    return _SHARED["x"]


@pytest.fixture(scope="module")
def protocols(emu_ctx, rows7):
    """the seven rows, their symbols behind each front end (slicer of an Engine(proto="none") on the CPU emulation, whole
    pushes) and the model on those symbols"""
    if "want" not in _SHARED:
        syms, want = {}, {}
        for f in FRONTS:
            syms[f], _, _ = run_front(emu_ctx, rows7, f, "none", [N_SAMPLES])
            want[f] = [model(s) for s in syms[f]]
        _SHARED["syms"], _SHARED["want"] = syms, want
    return rows7, _SHARED["syms"], _SHARED["want"]


def test_model_confirms_each_protocol_and_nothing_else(protocols):
    """before any engine is asked: each row reaches periodic >= 2 for its own family at its own front end, the noise and
    the silent row for none at any"""
    _, _, want = protocols
    merged = [np.zeros(9, STAT) for _ in range(7)]
    for b in range(7):
        for pid in range(9):
            merged[b][pid] = want[SOURCE[pid]][b][1][pid]
    for b in range(5):
        per = family_periodic(merged[b])
        assert per[b] >= 2 and per[b] == max(per) and per.index(max(per)) == b, (NAMES[b], per)
    for b in (5, 6):
        for f in FRONTS:
            assert max(family_periodic(want[f][b][1])) < 2, (b, f)


@pytest.mark.parametrize("front", list(FRONTS))
def test_through_the_slicers(ctx, protocols, front):
    x, syms, want = protocols
    ragged = lambda k, b, c: c - (17 * b + 5 * k) % 64 if (k + b) % 5 else 0
    got, evs, st = run_front(ctx, x, front, "scan", [30000, 12345, 24000], counts_of=ragged)
    none, _, _ = run_front(ctx, x, front, "none", [30000, 12345, 24000], counts_of=ragged)
    for b in range(7):
        assert len(got[b]) == len(none[b]) and (got[b] == none[b]).all(), b          # the slicer is untouched
        ev, s = model(got[b])
        assert evs[b].tobytes() == ev.tobytes() and st[b].tobytes() == s.tobytes(), b


# ----------------------------------------------------------------------------- many workgroups
@pytest.mark.gpu
def test_many_channels(gpu_ctx, rows7):
    x = rows7
    B, n = 512, 20000
    rng = np.random.default_rng(5)
    rows = np.stack([np.roll(x[b % 7], -int(rng.integers(0, N_SAMPLES)))[:n] for b in range(B)])
    syms, evs, st = run_front(gpu_ctx, rows, "wide10", "scan", [n])
    assert sum(len(e) for e in evs) > B
    for b in range(B):
        ev, s = model(syms[b])
        assert evs[b].tobytes() == ev.tobytes() and st[b].tobytes() == s.tobytes(), b
