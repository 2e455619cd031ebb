"""BPTC(196,96) of the DMR decoder on designed error patterns, against the REFERENCE's own bptc_196_96.c.

dh_dmr_bptc_lane (decoder_core.hpp) is a rewrite of bptc_196_96.c: the 13 x 15 matrix gathered straight from the received bits, the
fifteen Hamming(13,9) column decodes bit-sliced over row words, the error row found by pattern match.  Random noise practically never
reaches the cases such a decoder gets wrong, so tests/common.py: bptc_patterns builds them -- every single bit, every pair (two errors in
a column are rejected or miscorrected into a third cell), every triple inside a column and inside a row, every 2 x 2 rectangle (accepted
with WRONG data, which the product must reproduce), patterns inside the four parity rows that are dropped after the column pass, the R(3)
bit outside the matrix, random weights 3..12 -- and tests/golden/bptc_patterns_ref.npz holds what the reference's decoder, compiled where
it lies, makes of each (tests/golden/make_golden_bptc_patterns.py).

* the fixture on its own: the classes hold what they were designed to hold (accepted, rejected, accepted-but-wrong);
* the oracle's restatement, and oracle/_ref where it is built, reproduce it;
* the batch entry (dh_bptc_196_96) reproduces it: all N blocks in one call, and batches of 1, 63, 64, 65 blocks (one block per lane);
* the same vectors as DATA BURSTS through decoder-only engines: received bit r is bit 1 - r % 2 of info dibit r / 2, info dibit d sits at
  burst position 12 + d (d < 49) or 46 + d, under every data type 0..15 and behind leads of 29 + c dibits, so that the funnel shift of
  pass A (bursts lie 144 = 4 * 32 + 16 bits apart) meets every word alignment.  The SLOTTYPE / BPTC / LC / SOFT_RESET events of every
  burst follow from the fixture and the rule of dmr_phase.cpp:247-288 alone -- rate 3/4 data (8) is not decoded, a voice LC header (1)
  gives an LC, terminator (2) and idle (9) a soft reset -- and the whole event stream equals the oracle's, in one push, in pushes of 997
  symbols, and with the burst-serial pass B.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from common import BPTC_CLASSES, BPTC_PATTERN_SEED, bptc_pattern_fixture, bptc_patterns, npz_digest
from dec_harness import expected, is_emu, run_dmr_pass_b
from digiham_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bptc_patterns_ref.npz")
EV_SYNC, EV_META_RESET, EV_LC, EV_SOFT_RESET, EV_BPTC, EV_SLOTTYPE = 1, 3, 4, 5, 6, 7
REJECTED, RIGHT, WRONG = 0, 1, 2


@pytest.fixture(scope="module")
def pat(oracle):
    """the generated vectors with the reference's verdicts; fails loudly when the generator no longer produces the fixture's list"""
    payload, sent, cls = bptc_patterns(oracle)
    ok, out, z = bptc_pattern_fixture(FIXTURE)
    assert int(z["seed"]) == BPTC_PATTERN_SEED and int(z["n"]) == len(payload) == len(ok)
    assert hashlib.sha256(payload.tobytes()).digest() == z["payload_sha256"].tobytes(), "the generator drifted away from the fixture"
    assert (np.bincount(cls, minlength=len(BPTC_CLASSES)) == z["class_counts"]).all()
    outcome = np.where(ok == 0, REJECTED, np.where((out == sent).all(axis=1), RIGHT, WRONG)).astype(np.uint8)
    for a in (payload, sent, cls, ok, out, outcome):
        a.setflags(write=False)
    return {"payload": payload, "sent": sent, "cls": cls, "ok": ok, "out": out, "outcome": outcome}


def _of(pat, *names):
    return np.isin(pat["cls"], [BPTC_CLASSES.index(n) for n in names])


def test_fixture_holds_what_the_classes_were_designed_for(pat):
    """On the reference's results alone, before any product runs.  The counts are the reference's (they equal what the oracle's
    restatement gives): of the 19 110 pairs the 180 that the column code cannot resolve are rejected, every rectangle that is accepted is
    accepted with wrong data."""
    cls, outcome = pat["cls"], pat["outcome"]
    assert (outcome[_of(pat, "a_clean", "b_single")] == RIGHT).all()
    count = lambda name, what: int((outcome[_of(pat, name)] == what).sum())
    assert (_of(pat, "a_clean").sum(), _of(pat, "b_single").sum()) == (10, 4 * 196)
    assert (count("c_pair", RIGHT), count("c_pair", REJECTED), count("c_pair", WRONG)) == (18930, 180, 0)
    assert (count("d_column_triple", RIGHT), count("d_column_triple", REJECTED), count("d_column_triple", WRONG)) == (3630, 660, 0)
    assert count("d_row_triple", RIGHT) == 5915 == _of(pat, "d_row_triple").sum()
    assert (count("e_rectangle", WRONG), count("e_rectangle", REJECTED), count("e_rectangle", RIGHT)) == (6930, 1260, 0)
    assert _of(pat, "f_parity_pair").sum() == 1770 and _of(pat, "f_parity_triple").sum() == 1000
    assert count("f_parity_pair", REJECTED) > 0 and count("f_parity_pair", WRONG) == 0 == count("f_parity_triple", WRONG)
    assert (outcome[_of(pat, "g_r3_alone", "g_r3_single", "g_r3_two_columns")] == RIGHT).all() and _of(pat, "g_r3_single").sum() == 195
    h = outcome[_of(pat, "h_random")]
    assert len(h) == 3000 and 0.10 < (h == REJECTED).mean() < 0.30 and 0.08 < (h == WRONG).mean() < 0.25
    assert set(cls.tolist()) == set(range(len(BPTC_CLASSES)))


@pytest.mark.parametrize("which", ["oracle", "ref"])
def test_oracle_and_reference_reproduce_the_fixture(oracle, pat, which):
    if which == "ref":
        want = json.load(open(os.path.join(HERE, "golden", "ref_compare_hashes.json")))["bptc_patterns_ref_npz"]
        assert npz_digest(FIXTURE) == want                 # the committed file is the one the reference produced
        if oracle.ref() is None:
            return
    out, ok = oracle.bptc_196_96(pat["payload"], which)
    assert (ok == pat["ok"]).all()
    assert (out[ok == 1] == pat["out"][ok == 1]).all()


def test_batch_entry_reproduces_the_fixture(ctx, pat):
    """dh_bptc_196_96 runs dh_dmr_bptc_lane, one block per lane: all N blocks at once, then 1, 63, 64 and 65 blocks cut from the pairs
    where accepted and rejected words lie side by side."""
    out, ok = ctx.bptc_196_96(pat["payload"].copy())                  # (the fixture's arrays are read-only)
    bad = np.nonzero(ok != pat["ok"])[0]
    assert len(bad) == 0, "verdict differs at %s (classes %s)" % (bad[:8], [BPTC_CLASSES[c] for c in pat["cls"][bad[:8]]])
    bad = np.nonzero((out != pat["out"]).any(axis=1))[0]
    assert len(bad) == 0, "output differs at %s (classes %s)" % (bad[:8], [BPTC_CLASSES[c] for c in pat["cls"][bad[:8]]])
    c = np.nonzero(_of(pat, "c_pair"))[0]
    rej = c[pat["ok"][c] == 0]
    for n in (1, 63, 64, 65):
        for first in (int(rej[0]), int(rej[len(rej) // 2]) - n // 2, int(rej[-1]) - n + 1, int(c[0])):
            sl = slice(first, first + n)
            assert c[0] <= first and first + n - 1 <= c[-1]
            out, ok = ctx.bptc_196_96(pat["payload"][sl].copy())
            assert (ok == pat["ok"][sl]).all() and (out == pat["out"][sl]).all(), (n, first)
        assert (pat["ok"][int(rej[0]):int(rej[0]) + n] == 0).any() and (n == 1 or (pat["ok"][int(rej[0]):int(rej[0]) + n] == 1).any())


# ------------------------------------------------------------------ the same vectors as data bursts
CACH = [np.array(synth.dmr_cach(s), np.uint8) for s in (0, 1)]
SYNCS = [np.array(synth.DMR_SYNC[k], np.uint8) for k in ("bs_data", "ms_data")]
LEAD0 = 29


def _slot_type_dibits():
    """[256][10]: Golay(20,8) of cc << 4 | dt as ten dibits, first on top (dmr_phase.cpp:236-245)"""
    w = np.array([synth.block_encode("golay_20_8", v) for v in range(256)], np.uint32)
    return np.stack([(w >> (18 - 2 * k)) & 3 for k in range(10)], axis=1).astype(np.uint8)


def _pick(pat, per_group):
    """indices into the vectors: all of them, or `per_group` of every (class, outcome) that exists, spread over the group"""
    if per_group is None:
        return np.arange(len(pat["ok"]))
    idx = []
    for c in range(len(BPTC_CLASSES)):
        for o in (REJECTED, RIGHT, WRONG):
            g = np.nonzero((pat["cls"] == c) & (pat["outcome"] == o))[0]
            if len(g):
                idx.append(g[np.unique(np.linspace(0, len(g) - 1, min(per_group, len(g))).astype(int))])
    return np.concatenate(idx)


def _plan(pat, idx, B):
    """Lay the vectors idx out over B channels: -> streams [B][n], and per channel its lead and the (vector, dt, cc) of its K bursts.
    The data type runs 0..15 inside every outcome, so each type meets accepted, rejected and accepted-but-wrong blocks."""
    K = -(-len(idx) // B)
    idx = np.resize(idx, B * K)                                   # the last channel is filled up from the front
    dt, cc = np.zeros(B * K, np.uint8), np.zeros(B * K, np.uint8)
    for o in (REJECTED, RIGHT, WRONG):
        m = np.nonzero(pat["outcome"][idx] == o)[0]
        dt[m] = np.arange(len(m)) % 16
        cc[m] = (np.arange(len(m)) // 16 + o) % 16
    assert {(int(d), int(o)) for d, o in zip(dt, pat["outcome"][idx])} == {(d, o) for d in range(16) for o in (REJECTED, RIGHT, WRONG)}
    bits = np.unpackbits(pat["payload"][idx], axis=1)[:, :196]
    info = (bits[:, 0::2] << 1 | bits[:, 1::2]).astype(np.uint8)  # received bit r: bit 1 - r % 2 of dibit r / 2
    st = _slot_type_dibits()[cc.astype(int) << 4 | dt]
    bursts = np.zeros((B, K, 144), np.uint8)
    flat = bursts.reshape(B * K, 144)
    flat[:, 12:61], flat[:, 95:144] = info[:, :49], info[:, 49:]
    flat[:, 61:66], flat[:, 90:95] = st[:, :5], st[:, 5:]
    bursts[:, 0::2, :12], bursts[:, 1::2, :12] = CACH[0], CACH[1]
    bursts[0::2, :, 66:90], bursts[1::2, :, 66:90] = SYNCS[0], SYNCS[1]
    leads = LEAD0 + np.arange(B) % 32
    n = int(leads.max()) + 144 * K + 8                            # fewer than 144 dibits behind the last burst: nothing is decoded there
    rng = np.random.default_rng(21)
    streams = np.zeros((B, n), np.uint8)
    for b in range(B):
        streams[b, :leads[b]] = rng.integers(0, 4, leads[b])
        streams[b, leads[b]:leads[b] + 144 * K] = bursts[b].ravel()
    rows = lambda a: a.reshape(B, K)
    return streams, leads, rows(idx), rows(dt), rows(cc)


def _check_events_by_rule(pat, ev, lead, idx, dt, cc, what):
    """one channel's events against dmr_phase.cpp:247-288 applied to the reference's BPTC verdicts"""
    K = len(idx)
    at = lead + 144 * np.arange(K)
    ok, out = pat["ok"][idx] == 1, pat["out"][idx]
    slot = (np.arange(K) & 1).astype(np.uint8)
    sync = ev[ev["type"] == EV_SYNC]
    assert int(sync["sym_index"][0]) == lead == int(ev["sym_index"][0]), (what, "the first burst was not found at the lead")
    assert (sync["sym_index"] == at).all() and (sync["b"] == 1).all() and (sync["a"] == slot).all(), what
    assert not (ev["type"] == EV_META_RESET).any(), what

    def events(typ, where):
        e = ev[ev["type"] == typ]
        assert len(e) == where.sum() and (e["sym_index"] == at[where]).all(), (what, "events of type %d at other bursts than the rule gives" % typ)
        assert (e["a"] == slot[where]).all(), (what, typ)
        return e
    e = events(EV_SLOTTYPE, np.ones(K, bool))
    assert (e["b"] == dt).all() and (e["len"] == 1).all() and (e["payload"][:, 0] == cc).all() and not e["payload"][:, 1:].any(), what
    m = ok & (dt != 8)
    e = events(EV_BPTC, m)
    assert (e["b"] == dt[m]).all() and (e["len"] == 12).all() and (e["payload"][:, :12] == out[m]).all() and not e["payload"][:, 12:].any(), what
    m = ok & (dt == 1)
    e = events(EV_LC, m)
    assert (e["b"] == 0).all() and (e["len"] == 9).all() and (e["payload"][:, :9] == out[m][:, :9]).all() and not e["payload"][:, 9:].any(), what
    m = ok & ((dt == 2) | (dt == 9))
    e = events(EV_SOFT_RESET, m)
    assert (e["b"] == dt[m]).all() and (e["len"] == 0).all(), what


def test_vectors_as_data_bursts(ctx, oracle, pat):
    emu = is_emu(ctx)
    B = 8 if emu else 64
    idx = _pick(pat, 40 if emu else None)
    assert set(pat["cls"][idx].tolist()) == set(range(len(BPTC_CLASSES))) and (emu or len(idx) == len(pat["ok"]))
    streams, leads, vidx, dt, cc = _plan(pat, idx, B)
    K = vidx.shape[1]
    assert K > 64                                                 # more than the chunk behind the sync search: pass B goes lane-parallel
    assert len({int(l) % 2 for l in leads}) == 2 and len(set(leads.tolist())) == min(B, 32)
    want = expected(oracle, "dmr", streams)

    run, counts = run_dmr_pass_b(ctx, streams, None, False)
    got, (lanes, serial) = run.results, counts.sum(axis=0)
    assert (lanes > 0).all() and (serial == 1).all(), (lanes, serial)   # only the chunk behind the search is taken burst after burst
    for b in range(B):
        _check_events_by_rule(pat, got[b][1], int(leads[b]), vidx[b], dt[b], cc[b], "channel %d" % b)
        _check_events_by_rule(pat, want[b][1], int(leads[b]), vidx[b], dt[b], cc[b], "oracle, channel %d" % b)
        assert got[b][1].tobytes() == want[b][1].tobytes(), "channel %d: events differ from the oracle's" % b
        assert len(got[b][0]) == 0 == len(want[b][0]), "channel %d: frame bytes from data bursts" % b

    run, counts = run_dmr_pass_b(ctx, streams, None, True)
    forced, (lanes, serial) = run.results, counts.sum(axis=0)
    assert (lanes == 0).all() and (serial > 1).all()
    for b in range(B):
        assert forced[b][1].tobytes() == got[b][1].tobytes() and len(forced[b][0]) == 0, "channel %d: the burst-serial pass B differs" % b

    sub = slice(0, B if emu else 8)                               # bursts straddle the pushes
    run, counts = run_dmr_pass_b(ctx, streams[sub], 997, False)
    pushed, (lanes, serial) = run.results, counts.sum(axis=0)
    assert (lanes > 0).all()
    for b in range(sub.stop):
        assert pushed[b][1].tobytes() == got[b][1].tobytes() and len(pushed[b][0]) == 0, "channel %d: pushes of 997 symbols differ" % b
