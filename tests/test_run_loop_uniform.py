"""The slicer's run loop takes its wave-uniform decisions once (dsp_core.hpp: dh_rrc_demod_channel, dh_slice_symbols,
dh_timing_decision): the slicing phase stores every valid dibit under one predicate and lets the exact evaluation overwrite
the doubtful ones, the fetch-ahead test is one 32-bit compare against a bound taken once per push, and the timing verdict
is scalar logic on three ballots.  None of that may show: dibits, frames, events and the timing-block counters are the
oracle's, bit for bit, on both tiers -- for every store form (runs of 1, 2, 99 and 100 symbols, starting at an even and at an
odd row position), with every symbol in doubt, through the generic forms (two levels, invert, sps 20) and for the timing
verdict's cases (both steps, silence, a large DC, the smallest variance above the reference's limit)."""
import numpy as np
import pytest

from common import assert_matches_oracle
from digiham_amd import _taps, api, synth


class _Runner:
    """An engine fed push by push, all channels the same count (an int) or each its own (an array, ragged push); keeps the
    per-channel outputs and the symbols each push produced"""

    def __init__(self, ctx, x, cap, **kw):
        self.x, (self.B, self.n) = x, x.shape
        self.cap = cap
        self.eng = api.Engine(self.B, cap, ctx=ctx, **kw)
        self.pos = np.zeros(self.B, np.int64)
        self.syms, self.frames, self.evs = ([[] for _ in range(self.B)] for _ in range(3))
        self.per_push, self.pushes = [], []

    def push(self, cnt):
        cnt = np.minimum(np.broadcast_to(np.asarray(cnt, np.int64), (self.B,)), self.n - self.pos)
        buf = np.full((self.B, self.cap), np.nan, np.float32)          # behind a channel's count: not its business
        for b in range(self.B):
            buf[b, :cnt[b]] = self.x[b, self.pos[b]:self.pos[b] + cnt[b]]
        self.eng.push(buf, n=int(cnt.max()), counts=cnt.astype(np.uint32))
        self.pos += cnt
        self.pushes.append(cnt.copy())
        s, sc = self.eng.symbols()
        self.per_push.append(np.array(sc, np.int64))
        for b in range(self.B):
            self.syms[b].append(s[b, :sc[b]].copy())
        if self.eng.has_proto:
            f, fc = self.eng.frames(); e, ec = self.eng.events()
            for b in range(self.B):
                self.frames[b].append(f[b, :fc[b]].copy()); self.evs[b].append(e[b, :ec[b]].copy())
        return self.per_push[-1]

    def finish(self):
        while (self.pos < self.n).any():
            self.push(self.cap)
        eng = self.eng
        unc, ex = eng.debug_header(16), eng.debug_header(17)
        blocks, ordered = eng.timing_stats()
        has_proto = eng.has_proto
        eng.close()
        cat = lambda parts, dt: [np.concatenate(p) if p else np.zeros(0, dt) for p in parts]
        res = {"syms": cat(self.syms, np.uint8), "frames": cat(self.frames, np.uint8) if has_proto else [None] * self.B,
               "events": cat(self.evs, api.EVENT_DTYPE), "filtered": None}
        return res, np.stack(self.per_push), dict(unc=unc, ex=ex, blocks=blocks, ordered=ordered)


def _run_cuts(ctx, x, cuts, **kw):
    """x[B][n] in pushes of cuts[0], cuts[1], ... samples (an int: every channel; an array: each channel its own), the rest in
    pushes of 3 000 -> per-channel concatenated outputs, the symbols each push produced [push][B], and the counters (uncertain
    symbols, exact runs, timing blocks, blocks through the in-order chain)"""
    r = _Runner(ctx, x, 3000, **kw)
    for c in cuts:
        r.push(c)
    return r.finish()


# what a push has to yield, from which position of the variance block, for every store form to occur: (block position, symbols).
# From position 99 the first run is one symbol and the next one starts at an odd row position.
_GOALS = [(0, 100), (0, 99), (50, 1), (50, 2), (99, 2), (99, 3), (99, 100), (99, 101)]


def _steer(ctx, x, **kw):
    """Feeds every channel towards _GOALS, one after the other: 10 samples per symbol wanted, first to reach the block position,
    then the push itself; a push that came out a symbol off (the timing stepped) is tried again; the rest of the streams follows.
    -> the pushes made (per-channel counts), and what _run_cuts returns for them"""
    r = _Runner(ctx, x, 3000, **kw)
    k, goal = np.zeros(r.B, np.int64), np.zeros(r.B, np.int64)
    for _ in range(120):
        if (goal >= len(_GOALS)).all():
            break
        cnt, want = np.zeros(r.B, np.int64), np.full(r.B, -1, np.int64)
        for b in range(r.B):
            if goal[b] < len(_GOALS):
                at, c = _GOALS[goal[b]]
                if k[b] == at:
                    cnt[b], want[b] = 10 * c, c
                else:
                    cnt[b] = 10 * ((at - k[b]) % 100)
        sc = r.push(cnt)
        goal += (want >= 0) & (sc == want)
        k = (k + sc) % 100
    assert (goal >= len(_GOALS)).all(), (goal, r.pos)
    out = r.finish()
    return r.pushes, out


def _run_shapes(per_push, sps=10):
    """What the run loop made of the pushes: a push that yields c symbols from block position k is cut into runs at the ends
    of the 100-symbol variance blocks and at the (1024 - 2) / sps symbols whose windows fit one FIR pass (102 at sps 10: only
    the blocks cut; 51 at sps 20) -> the set of (symbols in the run, parity of the push's symbol count at the run's start)
    over all channels"""
    shapes = set()
    for b in range(per_push.shape[1]):
        k = 0
        for c in per_push[:, b]:
            done = 0
            while done < c:
                m = int(min(c - done, 100 - k, 1022 // sps))
                shapes.add((m, done % 2))
                done += m; k = (k + m) % 100
    return shapes


def _dmr(seeds, units, snr):
    chans = [synth.impair(synth.shape(synth.dmr_stream(s, units, two_slots=s % 2 == 1)), s, snr_db=snr[i % len(snr)],
                          dc=[0.0, 0.1, -0.2][i % 3], delay=(7 * s) % 19, gain=[1.0, 0.4, 1.8][i % 3]) for i, s in enumerate(seeds)]
    n = min(len(c) for c in chans)
    return np.stack([c[:n] for c in chans])


@pytest.fixture(scope="module")
def dmr_case(oracle):
    x = _dmr([61, 62, 63, 64], 14, [None, 24, 9, 6])
    return x, oracle.chain(x, proto=1)


def test_every_store_form_of_the_slicing_phase(ctx, dmr_case):
    """Runs of 1, 2, 99 and 100 symbols at both row parities (the 16-bit pair store, the byte stores, an odd last symbol stored
    as a byte), a noisy default engine beside one with every symbol in doubt: the provisional dibits of the doubtful symbols
    are all overwritten by the exact evaluation's."""
    x, ref = dmr_case
    B = x.shape[0]
    total = int(ref["sym_count"].sum())
    cuts, (res, per_push, st) = _steer(ctx, x, proto="dmr")
    shapes = _run_shapes(per_push)
    print("run shapes (symbols, parity at start):", sorted(shapes), "doubtful symbols", st["unc"], "of", ref["sym_count"])
    for m in (1, 2, 99, 100):
        assert (m, 0) in shapes and (m, 1) in shapes, (m, sorted(shapes))
    assert_matches_oracle(res, ref, B, "default engine")
    assert 0 < int(st["unc"].sum()) < total                 # the noisy channels leave symbols in doubt, the clean one decides by itself
    res, per_push2, st = _run_cuts(ctx, x, cuts, proto="dmr", exact_symbols=True)
    assert (per_push2 == per_push).all()
    assert_matches_oracle(res, ref, B, "every symbol in doubt")
    assert int(st["unc"].sum()) == total                    # every stored dibit is the exact evaluation's


def test_exact_fir_and_default_agree(ctx, dmr_case):
    """exact_mode is read once per push: the engine that sends every run through the reference-order FIR (exact_mode 2) and the
    default one give the same dibits, frames and events -- also with pushes down to one sample short of a symbol and blocks
    that straddle pushes (runs that start inside a block)."""
    x, ref = dmr_case
    B, n = x.shape
    cuts = [9, 1, 333, 9, 1500, 9, 9, 9, 777, 2, 2999]
    a, pa, sa = _run_cuts(ctx, x, cuts, proto="dmr")
    b, pb, sb = _run_cuts(ctx, x, cuts, proto="dmr", exact_fir=True)
    assert any(k != 0 for k in np.cumsum(pa[:-1, 0]) % 100)    # runs that start inside a block
    assert (pa == pb).all() and int(sb["ex"].min()) > 0 and int(sa["ex"].sum()) == 0
    assert_matches_oracle(a, ref, B, "default, ragged")
    assert_matches_oracle(b, ref, B, "exact fir, ragged")
    for ch in range(B):
        assert (a["syms"][ch] == b["syms"][ch]).all() and (a["frames"][ch] == b["frames"][ch]).all()
        assert a["events"][ch].tobytes() == b["events"][ch].tobytes()
    assert (sa["blocks"] == sb["blocks"]).all() and (sa["blocks"] == ref["timing_blocks"]).all()


@pytest.mark.parametrize("route", ["dstar", "dstar_invert", "nxdn48"])
def test_generic_forms_behind_the_constants(ctx, oracle, route):
    """Two levels (D-Star), two levels inverted, and the narrow filter at sps 20 (NXDN): the forms of the slicing phase and the
    run planning that the sps-10, four-level constants fold away still run, on noisy streams in ragged pushes."""
    if route == "nxdn48":
        chans = [synth.impair(synth.shape(synth.nxdn_stream(s, 4), sps=20, taps=_taps.narrow()), s, snr_db=snr, dc=0.05, gain=g)
                 for s, snr, g in ((71, None, 1.0), (72, 12, 0.5), (73, 8, 1.6), (74, 20, 1.0))]
        kw, okw, cuts = dict(proto="nxdn", rrc="narrow", sps=20), dict(proto=3, rrc=2, sps=20), [2187, 20, 40, 1980, 19, 2000]
    else:
        inv = route == "dstar_invert"
        chans = [synth.impair(synth.fsk_shape(synth.dstar_stream(s, 1)[0], sps=10), s, snr_db=snr, dc=0.02, gain=g)
                 for s, snr, g in ((81, None, 1.0), (82, 10, 0.7), (83, 6, 1.3), (84, 15, 1.0))]
        kw = dict(proto="none" if inv else "dstar", rrc="none", demod="fsk", sps=10, invert=inv)
        okw = dict(proto=0 if inv else 5, rrc=0, levels=2, sps=10, invert=inv)
        cuts = [1013, 10, 20, 970, 9, 1000, 990, 2000]
    n = min(min(len(c) for c in chans), 9000)
    x = np.stack([c[:n] for c in chans])
    assert sum(cuts) < n
    ref = oracle.chain(x, **okw)
    res, per_push, st = _run_cuts(ctx, x, cuts, **kw)
    assert_matches_oracle(res, ref, x.shape[0], route)
    assert (st["blocks"] == ref["timing_blocks"]).all() and int(ref["timing_blocks"].min()) >= 2
    shapes = _run_shapes(per_push, kw["sps"])
    assert {p for _, p in shapes} == {0, 1}, sorted(shapes)   # runs at both row parities


def _drift(x, r):
    """x resampled at 1 + r times its rate: the symbol instants walk by r samples per sample"""
    t = np.arange(int(len(x) / (1.0 + r)) - 2) * (1.0 + r)
    return np.interp(t, np.arange(len(x)), x).astype(np.float32)


def test_timing_verdict_cases(ctx, oracle):
    """The timing decision's verdict on streams whose symbol clock drifts by a sample per block either way (both steps), on
    silence (every variance 0), under a DC 300 times the signal (the estimate cannot decide: the in-order chain does) and on a
    channel scaled until its smallest phase variance is above the reference's 5e6 (no step): the timing-block counters are the
    oracle's, and so are the dibits, frames and events (with their positions)."""
    n = 6 * 1000 + 400
    base = [synth.shape(synth.dmr_stream(s, 8)) for s in (91, 92, 93)]
    up = _drift(base[0][:n + 200], +1.0 / 1000.0)[:n]
    down = _drift(base[1][:n + 200], -1.0 / 1000.0)[:n]
    plain = base[2][:n]
    rms = float(np.sqrt(np.mean(plain.astype(np.float64) ** 2)))
    x = np.stack([synth.impair(up, 1, snr_db=30), synth.impair(down, 2, snr_db=30), np.zeros(n, np.float32),
                  (up + np.float32(300.0 * rms)).astype(np.float32), (np.float32(40000.0) * (down - down.mean())).astype(np.float32), plain])
    ref = oracle.chain(x, proto=1)
    cuts = [2217, 1983, n - 4200]
    res, _, st = _run_cuts(ctx, x, cuts, proto="dmr")
    print("oracle blocks", ref["timing_blocks"], "up", ref["steps_up"], "down", ref["steps_down"], "over 5e6", ref["blocks_over"],
          "engine blocks", st["blocks"], "in-order", st["ordered"])
    assert_matches_oracle(res, ref, x.shape[0], "timing verdict")
    assert (st["blocks"] == ref["timing_blocks"]).all() and int(ref["timing_blocks"].min()) >= 5
    assert ref["steps_up"][0] > 0 and ref["steps_down"][1] > 0                      # both steps are taken
    assert ref["steps_up"][2] + ref["steps_down"][2] == 0                           # silence: variance 0, no step
    assert ref["blocks_over"][4] == ref["timing_blocks"][4] and ref["steps_up"][4] + ref["steps_down"][4] == 0
    est = st["blocks"] - st["ordered"]
    assert est[0] > 0 and est[1] > 0 and est[5] > 0                                  # the estimate's verdict decided these
    assert st["ordered"][3] > 0                                                      # the DC channel went to the in-order chain
