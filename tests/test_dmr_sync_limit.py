"""The sync limit of the DMR decoder: a 48-bit sync word with 3 wrong bits is a sync, with 4 it is none (dmr_phase.cpp:18-33).

The decoder compares the sync slot of a burst with four patterns twice over -- dh_dmr_sync_type on the symbol planes during the search
(dmr_phase.cpp:35-47) and dh_dmr_sync_type_bits per lane in pass A once locked (:102) -- as popc(h ^ P) + popc(l ^ 0xFFFFFF) <= 3 over
the two bit planes of the 24 dibits.  Words with 0..5 wrong bits of each of the four patterns are placed where each comparison decides:

* the search: behind a noise lead the first burst carries 4 wrong bits, the second 3 -- the decoder locks at the second;
* locked, data bursts: a damaged word in every third burst of either slot of an idle-burst stream (the decoder stays locked);
* locked, voice: burst A of the superframes of both slots carries a damaged voice sync word.

At the limit the wrong bits are {i, i + 16, i + 32} (one plane) and the same plus i + 7 (the other plane), i = 0..47 mod 48: every bit
of both planes is wrong in some word that must pass and in some word that must fail.  Expectation by construction: a SYNC event (b = 1
data, 2 voice) at a burst exactly when its word has at most 3 wrong bits; everything else -- a data burst whose sync failed still has its
slot type parsed, dmr_phase.cpp:235 -- is compared with the oracle's events and frame bytes, in one push, in pushes of 1 000 and of 97
symbols, and with the burst-serial pass B.
"""
import numpy as np
import pytest

from dec_harness import expected, run_dmr_pass_b
from digiham_amd import synth

EV_SYNC, EV_META_RESET, EV_SLOTTYPE, EV_EMB = 1, 3, 7, 8
NAMES = ("bs_data", "bs_voice", "ms_data", "ms_voice")
WORD = {k: np.array(synth.DMR_SYNC[k], np.uint8) for k in NAMES}
CACH = [np.array(synth.dmr_cach(s), np.uint8) for s in (0, 1)]
LEAD0 = 29
CC = 5


def _damage(word, bits):
    """sync bit j of 48: bit 1 (j even) or bit 0 (j odd) of dibit j / 2"""
    w = word.copy()
    for j in bits:
        w[j // 2] ^= 1 if j % 2 else 2
    return w


def _bit_sets():
    """wrong-bit sets, ascending weight: [(weight, bits)] -- the limit sets for every i, a dozen each of the weights around them"""
    rng = np.random.default_rng(48)
    sets = [()]
    for w in (1, 2):
        sets += [tuple(int(x) for x in rng.choice(48, w, replace=False)) for _ in range(12)]
    sets += [(i, (i + 16) % 48, (i + 32) % 48) for i in range(48)]
    sets += [(i, (i + 7) % 48, (i + 23) % 48) for i in range(48)]                     # three wrong bits over both planes
    sets += [(i, (i + 16) % 48, (i + 32) % 48, (i + 7) % 48) for i in range(48)]
    sets += [tuple(int(x) for x in rng.choice(48, 5, replace=False)) for _ in range(12)]
    assert all(len(set(s)) == len(s) for s in sets)
    return [(len(s), s) for s in sets]


SETS = _bit_sets()
LIMIT3 = [s for w, s in SETS if w == 3][:48]
LIMIT4 = [s for w, s in SETS if w == 4]


def _distance(a, b):
    return int(sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b)))


def test_the_damaged_words_decide_what_they_are_meant_to():
    """The four clean patterns lie more than 6 bits apart (more than 8 in fact), so a word within 5 bits of one is further than 3 from
    every other: which of the four comparisons comes first cannot matter, and `wrong bits <= 3` is the whole expectation.  The limit
    sets touch every bit of both planes on either side of the limit."""
    for a in NAMES:
        for b in NAMES:
            if a != b:
                assert _distance(WORD[a], WORD[b]) > 8, (a, b)
    for name in NAMES:
        assert set(WORD[name].tolist()) <= {1, 3}                                     # the bit-0 plane of every pattern is all ones
        for w, s in SETS:
            d = _damage(WORD[name], s)
            assert _distance(d, WORD[name]) == w
            assert all(_distance(d, WORD[o]) > 3 for o in NAMES if o != name)
    for sets in (LIMIT3, LIMIT4):
        assert {j for s in sets for j in s} == set(range(48))
    assert all(len({j % 2 for j in s}) == 1 for s in LIMIT3) and all(len({j % 2 for j in s}) == 2 for s in LIMIT4)
    assert sorted({w for w, _ in SETS}) == [0, 1, 2, 3, 4, 5]


# ------------------------------------------------------------------ bursts
_ST9 = np.array(synth.bits_to_dibits(synth._bits_of(synth.block_encode("golay_20_8", (CC << 4) | 9), 20)), np.uint8)


def _idle_bursts(n, rng):
    """[n][144] data bursts of type 9 (idle) around clean BPTC blocks of random content; CACH and sync slot left to the caller"""
    b = np.zeros((n, 144), np.uint8)
    for i in range(n):
        tx = np.array(synth.bits_to_dibits(synth.bptc_196_96_encode_bits(list(rng.integers(0, 2, 96)))), np.uint8)
        b[i, 12:61], b[i, 95:144] = tx[:49], tx[49:]
    b[:, 61:66], b[:, 90:95] = _ST9[:5], _ST9[5:]
    return b


_EMB_MID = np.array(synth.dmr_emb_mid(CC, 0, [0] * 16), np.uint8)


def _voice_bursts(n, rng):
    """[n][144] voice bursts of random payload with a clean EMB (single fragment, LCSS 0) in the middle"""
    b = rng.integers(0, 4, (n, 144)).astype(np.uint8)
    b[:, 66:90] = _EMB_MID
    return b


def _streams(per_channel, leads):
    """bursts [K][144] per channel (slots alternate from 0) behind noise leads -> [B][n]"""
    rng = np.random.default_rng(49)
    n = max(l + 144 * len(b) for l, b in zip(leads, per_channel)) + 8         # fewer than 144 dibits behind the last burst
    out = np.zeros((len(leads), n), np.uint8)
    for c, (l, b) in enumerate(zip(leads, per_channel)):
        b = b.copy()
        b[0::2, :12], b[1::2, :12] = CACH[0], CACH[1]
        out[c, :l] = rng.integers(0, 4, l)
        out[c, l:l + 144 * len(b)] = b.ravel()
        out[c, l + 144 * len(b):] = rng.integers(0, 4, n - l - 144 * len(b))
    return out


def _check(ctx, oracle, streams, leads, expect, sync_b, chunks, lanes_in):
    """expect[c]: {burst: wrong bits of its sync word} for the bursts that carry a full sync word.  Runs the streams in one push and in
    the given pushes, lane-parallel and burst-serial, and holds every run to the oracle and the SYNC events to the construction."""
    want = expected(oracle, "dmr", streams)
    for chunk in (None,) + tuple(chunks):
        for scalar in (False, True):
            run, counts = run_dmr_pass_b(ctx, streams, chunk, scalar)
            lanes, serial = counts.sum(axis=0)
            what = "pushes of %s, %s pass B" % (chunk, "burst-serial" if scalar else "lane-parallel")
            assert (lanes == 0).all() if scalar else (chunk not in lanes_in or (lanes > 0).all()), (what, lanes, serial)
            for c, (frames, ev) in enumerate(run.results):
                sync = {int(e["sym_index"]): int(e["b"]) for e in ev[ev["type"] == EV_SYNC]}
                exp = {leads[c] + 144 * k: sync_b[c] for k, w in expect[c].items() if w <= 3}
                assert sync == exp, "%s, channel %d: SYNC events at other bursts than those with at most 3 wrong bits: %s" % (
                    what, c, sorted(set(sync.items()) ^ set(exp.items()))[:6])
                assert not (ev["type"] == EV_META_RESET).any(), (what, c, "the decoder lost its lock")
                assert int(ev["sym_index"][0]) == min(exp), (what, c, "first event not at the first burst with a sync")
                assert ev.tobytes() == want[c][1].tobytes(), "%s, channel %d: events differ from the oracle's" % (what, c)
                assert frames.tobytes() == want[c][0].tobytes(), "%s, channel %d: frame bytes differ from the oracle's" % (what, c)
    return want


def test_search_locks_at_three_wrong_bits_not_at_four(ctx, oracle):
    """Noise lead, a burst whose sync word has 4 wrong bits, one with 3, three clean ones -- for each of the four patterns and i = 0..47.
    The search (dh_dmr_sync_type on the planes) walks over the first burst: the first event of the channel is at the second."""
    rng = np.random.default_rng(50)
    per_channel, leads, expect, sync_b = [], [], [], []
    for name in NAMES:
        for i in range(48):
            b = _idle_bursts(5, rng) if name.endswith("data") else _voice_bursts(5, rng)
            b[:, 66:90] = WORD[name]
            b[0, 66:90], b[1, 66:90] = _damage(WORD[name], LIMIT4[i]), _damage(WORD[name], LIMIT3[i])
            per_channel.append(b); leads.append(LEAD0 + len(leads) % 32)
            expect.append({0: 4, 1: 3, 2: 0, 3: 0, 4: 0}); sync_b.append(1 if name.endswith("data") else 2)
    streams = _streams(per_channel, leads)
    _check(ctx, oracle, streams, leads, expect, sync_b, (97,), lanes_in=(97,))


def _word_plan(n_slots_of_words):
    """SETS dealt out in ascending weight: words that pass first, so that whole chunks of the stream stay regular for pass B"""
    return [SETS[j::n_slots_of_words] for j in range(n_slots_of_words)]


@pytest.mark.parametrize("family", ["bs", "ms"])
def test_locked_data_bursts_at_the_limit(ctx, oracle, family):
    """Idle bursts on both slots; every third burst of a slot (bursts 4, 5 of every six) carries a damaged data sync word, weights
    ascending.  The decoder stays locked throughout, and every burst -- sync or not -- has its slot type parsed."""
    name = family + "_data"
    rng = np.random.default_rng(51)
    K = 6 * ((len(SETS) + 1) // 2) + 4
    per_channel, leads, expect = [], [], []
    for c in range(4):
        b = _idle_bursts(K, rng)
        b[:, 66:90] = WORD[name]
        exp = {k: 0 for k in range(K)}
        spots = [k for k in range(K - 4) if (k // 2) % 3 == 2]
        assert len(spots) >= len(SETS)
        for k, (w, s) in zip(spots, SETS):
            b[k, 66:90] = _damage(WORD[name], tuple((j + 2 * c) % 48 for j in s))      # (the same bit plane, two dibits further per channel)
            exp[k] = w
        assert sorted(set(exp.values())) == [0, 1, 2, 3, 4, 5]
        per_channel.append(b); leads.append(LEAD0 + 9 * c); expect.append(exp)
    streams = _streams(per_channel, leads)
    want = _check(ctx, oracle, streams, leads, expect, [1] * 4, (1000, 97), lanes_in=(None, 1000, 97))
    for c in range(4):
        st = want[c][1][want[c][1]["type"] == EV_SLOTTYPE]
        assert (st["sym_index"] == leads[c] + 144 * np.arange(K)).all() and (st["b"] == 9).all() and (st["payload"][:, 0] == CC).all()


@pytest.mark.parametrize("family", ["bs", "ms"])
def test_locked_voice_superframes_at_the_limit(ctx, oracle, family):
    """Voice superframes on both slots; burst A of each carries a damaged voice sync word (weights ascending, dealt out over the two
    slots), bursts B..F a clean EMB.  A burst A without sync costs a count and no more: the superframe goes on, voice bytes come out."""
    name = family + "_voice"
    rng = np.random.default_rng(52)
    deal = _word_plan(2)
    S = len(deal[0]) + 1                                           # superframes per slot, the first one clean
    K = 12 * S
    per_channel, leads, expect = [], [], []
    for c in range(2):
        b = _voice_bursts(K, rng)
        exp = {}
        for slot in (0, 1):
            words = [(0, ())] + deal[slot ^ c]
            words += [(0, ())] * (S - len(words))
            for i, (w, s) in enumerate(words):
                k = 12 * i + slot                                  # burst A of superframe i on this slot
                b[k, 66:90] = _damage(WORD[name], s)
                exp[k] = w
        assert sorted(set(exp.values())) == [0, 1, 2, 3, 4, 5]
        per_channel.append(b); leads.append(LEAD0 + 1 + 14 * c); expect.append(exp)
    streams = _streams(per_channel, leads)
    want = _check(ctx, oracle, streams, leads, expect, [2] * 2, (1000, 97), lanes_in=(None, 1000, 97))
    for c in range(2):
        assert len(want[c][0]) == 27 * (K // 2)                    # slot 0 speaks from its first burst to its last
        emb = want[c][1][want[c][1]["type"] == EV_EMB]
        assert len(emb) == 10 * S and (emb["payload"][:, 0] == CC).all()
