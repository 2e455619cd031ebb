"""NXDN48: narrow RRC -> gfsk_demodulator -s 20 -> nxdn_decoder (examples/nxdn48-decoder.sh:19-21).

* the oracle's frame elements (scrambler, LICH, SACCH, FACCH1, trellis) against tests/golden/nxdn_ref.npz, whose
  expected values come from the reference's own classes compiled in place (PINNED), incl. the four SACCH
  patterns of the NXDN "Common Air Interface Test" document quoted at nxdn_phase.cpp:73-98;
* the engine (CPU wave emulation / MI355X) against the oracle: decoder on dibits, and the whole chain on audio -- on the
  calls of synth.nxdn_stream and on synth.nxdn_mixed_stream, whose frames walk the whole frame machine (every LICH class,
  releases in either block, damaged sync words and LICHs, sync loss at every frame index); what those streams reach is
  asserted on the oracle's events.  The frame elements through the product against the reference's vectors:
  tests/test_nxdn_elements.py.
"""
import json
import os

import numpy as np
import pytest

from digiham_amd import synth, _taps
from common import assert_matches_oracle, nxdn_digests, run_engine
from dec_harness import assert_rows, expected, run_symbols, stack_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nx():
    return np.load(os.path.join(ROOT, "tests", "golden", "nxdn_ref.npz"))


def test_oracle_frame_elements_match_the_reference_vectors(oracle, nx):
    for i in range(len(nx["scr_in"])):
        assert (oracle.nxdn_scramble(nx["scr_in"][i]) == nx["scr_out"][i]).all()
    assert [oracle.nxdn_lich(r) for r in nx["lich_in"]] == list(nx["lich_out"])
    for nb in (72, 192):
        for p, o, m in zip(nx["trellis%d_in" % nb], nx["trellis%d_out" % nb], nx["trellis%d_metric" % nb]):
            got, metric = oracle.nxdn_trellis(p, nb)
            assert metric == m and (got == o).all()
    for name, fn in (("sacch", oracle.nxdn_sacch), ("facch1", oracle.nxdn_facch1)):
        n_ok = 0
        for d, ok, o in zip(nx[name + "_in"], nx[name + "_ok"], nx[name + "_out"]):
            got_ok, got = fn(d)
            assert got_ok == bool(ok) and (not got_ok or (got == o).all())
            n_ok += got_ok
        assert n_ok > 20


def test_oracle_vs_compiled_reference_when_present(oracle):
    """Scrambler, LICH, SACCH and FACCH1 of the oracle against the reference's classes on 300 random blocks: against the
    reference's outputs stored as digests (tests/golden/ref_compare_hashes.json), and against oracle/_ref live where it is built."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_compare_hashes.json")))["nxdn"]
    assert nxdn_digests(oracle, "oracle") == want
    if oracle.ref_nxdn() is not None:
        assert nxdn_digests(oracle, "ref") == want


def test_cai_test_patterns_form_a_vcall_superframe(oracle, nx):
    """The four transmitted SACCH patterns of the CAI test document, put into frames, give one VCALL superframe."""
    rng = np.random.default_rng(1)
    frames = []
    for row in nx["cai_sacch_tx"]:
        body = synth.nxdn_scramble(synth.nxdn_lich_dibits(0x56) + [0] * 30 + list(rng.integers(0, 4, 144)))
        body[8:38] = list(row)                       # the patterns are given as transmitted (already scrambled)
        frames += synth.NXDN_SYNC + body
    s = np.array(list(rng.integers(0, 4, 17)) + frames + [0] * 200, np.uint8)
    out, ev = oracle.Decoder("nxdn").process(s)
    sf = ev[ev["type"] == 34]
    assert len(sf) == 1 and sf[0]["payload"][0] & 0x3F == 0x01          # NXDN_MESSAGE_TYPE_VCALL
    assert [int(e["a"]) for e in ev[ev["type"] == 33]] == [0, 1, 2, 3]


@pytest.mark.parametrize("seed", [3, 4])
def test_decoder_on_dibits_matches_oracle(ctx, oracle, seed):
    s = synth.nxdn_stream(seed, 40)
    rng = np.random.default_rng(seed)
    noisy = s.copy()
    hit = rng.random(len(s)) < 0.01                  # dibit errors: FEC, CRC failures, lost sync words
    noisy[hit] ^= rng.integers(1, 4, int(hit.sum())).astype(np.uint8)
    for stream in (s, noisy):
        want = expected(oracle, "nxdn", stream[None])
        out, ev = want[0]
        assert len(out) > 0 and (ev["type"] == 34).sum() > 0
        for chunk in (len(stream), 1000, 193):
            assert_rows(run_symbols(ctx, "nxdn", stream[None], chunk, capacity=max(chunk, 16)), want, "pushes of %d" % chunk)


@pytest.fixture(scope="module")
def mixed(oracle):
    """36 channels of synth.nxdn_mixed_stream with what oracle.Decoder("nxdn") makes of them.  Channels 0..23: frames of
    every RF type / functional channel / option, FACCH1 payloads the decoder accepts, releases in either block, damaged
    sync words, broken LICH parity; channel c loses its signal from frame c on for 1 + c % 9 frames; the odd channels
    have 0.5 % wrong dibits.  Channels 24..35: a voice call (SACCHs decoded four frames ahead) that loses its signal from
    frame 6 + k on (k = 0..11: every residue of the ahead group) for 1 + 2 k % 9 frames."""
    accept = lambda d: oracle.nxdn_facch1(d)[0]
    rows, starts, loss, inside = [], [], [], []
    for c in range(24):
        loss.append((c, 1 + c % 9))
        s, st, ins = synth.nxdn_mixed_stream(500 + c, 44, accept, lead_in=20 + c, loss=loss[-1], err=0.005 * (c & 1))
        rows.append(s); starts.append(st); inside.append(ins)
    for k in range(12):
        loss.append((6 + k, 1 + 2 * k % 9))
        s, st, _ = synth.nxdn_mixed_stream(600 + k, 30, accept, lead_in=20 + k, loss=loss[-1], voice_only=True)
        rows.append(s); starts.append(st)
    rows = stack_rows(rows)
    want = expected(oracle, "nxdn", rows)
    return rows, starts, loss, inside, want


def test_mixed_streams_walk_the_whole_frame_machine(mixed):
    """What the comparison below rests on, read off the ORACLE's output alone: both FACCH1 positions, releases in either
    block, sync losses (the drop right after the count reached 0, and the seven-frame run-down from 6), SACCH superframes,
    every option, and both kinds of LICH whose frame body is skipped."""
    rows, starts, loss, inside, want = mixed
    ev = np.concatenate([e for _, e in want[:24]])
    fa = ev[ev["type"] == 36]
    rel = fa[(fa["payload"][:, 0] & 0x3F) == 0x08]
    for blk in (0, 1):
        assert (fa["a"] == blk).sum() >= 20 and (rel["a"] == blk).sum() >= 10
    assert ((ev["type"] == 37) & (ev["b"] == 0)).sum() >= 10 and ((ev["type"] == 37) & (ev["b"] == 1)).sum() == len(rel)
    assert (ev["type"] == 34).sum() >= 5
    # frame starts INSIDE a released block (it is not consumed: the search resumes at its first dibit) that the decoder took
    taken = sum(int(((e["type"] == 32) & (e["sym_index"] == p)).any()) for ins, (_, e) in zip(inside, want) for p in ins)
    assert taken >= 4, taken
    lich = ev[ev["type"] == 32]["payload"][:, 0]
    assert set((lich >> 1) & 3) == {0, 1, 2, 3} and set((lich >> 5) & 3) == {0, 1, 2, 3} and set((lich >> 3) & 3) == {0, 1, 2, 3}
    # frames the decoder still took on the old grid after the signal went, before it gave up: 0 .. 6
    ridden = set()
    for (first, count), st, (_, e) in zip(loss, starts, want):
        lo, hi = int(st[first]), int(st[first]) + 192 * count
        r = e[(e["type"] == 37) & (e["b"] == 0) & (e["sym_index"] >= lo) & (e["sym_index"] <= hi)]
        if len(r) and (int(r[0]["sym_index"]) - lo) % 192 == 0:
            ridden.add((int(r[0]["sym_index"]) - lo) // 192)
    assert {1, 6} <= ridden, ridden            # count 1 -> one frame at count 0, then the drop; count 6 -> six frames, dropped at the seventh
    voice = np.concatenate([e for _, e in want[24:]])
    assert ((voice["type"] == 37) & (voice["b"] == 0)).sum() >= 6 and (voice["type"] == 34).sum() >= 12


@pytest.mark.parametrize("chunk", [None, 1000, 193, 200, 385, 577, 769])
def test_mixed_streams_match_oracle(ctx, mixed, chunk):
    """Decoder bytes, events and counts of the 36 mixed channels equal the oracle decoder's, in one push and in pushes that
    leave every number of whole frames (and, with 200, every offset) in hand."""
    rows, _, _, _, want = mixed
    n = rows.shape[1]
    assert_rows(run_symbols(ctx, "nxdn", rows, chunk, capacity=max(min(chunk or n, n), 16)), want, "pushes of %s" % chunk)


def test_full_chain_narrow_rrc_sps20_mixed_frames(ctx, oracle):
    """The chain of test_full_chain_narrow_rrc_sps20 on mixed frames (synth.nxdn_mixed_stream): every kind of Viterbi pass
    behind the slicer, in one kernel and as two launches."""
    accept = lambda d: oracle.nxdn_facch1(d)[0]
    chans = []
    for i, seed in enumerate((21, 22, 23)):
        s, _, _ = synth.nxdn_mixed_stream(seed, 14, accept)
        x = synth.shape(s, sps=20, taps=_taps.narrow())
        chans.append(synth.impair(x, seed, snr_db=[None, 22, 16][i], dc=[0, 0.1, -0.2][i], delay=7 * i, gain=[1, 0.5, 1.7][i]))
    n = min(len(c) for c in chans)
    x = np.stack([c[:n] for c in chans])
    ref = oracle.chain(x, rrc=2, sps=20, proto=3)
    assert ref["out_count"].sum() > 0 and ref["event_count"].min() > 10      # (every channel locked and decoded frames)
    for chunks in ([n], [4800, 12345]):
        for split in (False, True):
            res = run_engine(ctx, x, "nxdn", chunks, rrc="narrow", sps=20, split_stages=split)
            assert_matches_oracle(res, ref, len(x), "nxdn mixed %s %s" % (chunks[:1], "split" if split else "chain"))


def test_full_chain_narrow_rrc_sps20(ctx, oracle):
    chans = []
    for i, seed in enumerate((11, 12, 13)):
        s = synth.nxdn_stream(seed, 14)
        x = synth.shape(s, sps=20, taps=_taps.narrow())
        chans.append(synth.impair(x, seed, snr_db=[None, 22, 16][i], dc=[0, 0.1, -0.2][i], delay=7 * i, gain=[1, 0.5, 1.7][i]))
    n = min(len(c) for c in chans)
    x = np.stack([c[:n] for c in chans])
    ref = oracle.chain(x, rrc=2, sps=20, proto=3)
    assert ref["out_count"].sum() > 0
    for chunks in ([n], [4800, 12345]):
        for split in (False, True):                    # one-wavefront chain kernel / slicer and decoder as two launches
            res = run_engine(ctx, x, "nxdn", chunks, rrc="narrow", sps=20, split_stages=split)
            assert_matches_oracle(res, ref, len(x), "nxdn %s %s" % (chunks[:1], "split" if split else "chain"))
