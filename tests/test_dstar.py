"""D-Star (examples/dstar-decoder.sh: fsk_demodulator -s 10 | dstar_decoder).

* scrambler and CRC: the oracle against tests/golden/dstar_ref.npz, whose expected values come from the reference's own
  src/dstar_decoder/{scrambler,crc}.cpp compiled in place (PINNED);
* the radio header (de-interleave + K=3 Viterbi + CRC): PINNED since header.cpp was compiled in place against ICU
  (tests/test_elements.py, tests/golden/elements_ref.npz); here known-answer round trips through an independent encoder,
  error tolerance as header.cpp:37 states it (path metric <= 10);
* the decoder on bits and the whole chain on 2-level FSK audio, engine (CPU wave emulation / MI355X) against the oracle.
"""
import os

import numpy as np
import pytest

from digiham_amd import synth
from common import assert_matches_oracle, run_engine
from dec_harness import assert_rows, expected, run_symbols, stack_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV_HEADER, EV_VOICE_START, EV_SYNC_VOICE, EV_MESSAGE, EV_SIMPLE, EV_FRAME_SYNC, EV_META_RESET = range(64, 71)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dstar_ref.npz"))


def test_oracle_scrambler_and_crc_match_the_reference_vectors(oracle, gold):
    for i, o in zip(gold["scr_in"], gold["scr_out"]):
        assert (oracle.dstar_scramble(i) == o).all()
    assert (synth.dstar_pn(660) == gold["scr_out"][0]).all()           # the generator's own sequence, and the product's below
    for d, n, c, v in zip(gold["crc_data"], gold["crc_len"], gold["crc_cand"], gold["crc_valid"]):
        assert oracle.dstar_crc_valid(d[:n], int(c)) == bool(v)
        assert (synth.dstar_crc(d[:n]) == int(c)) == bool(v)
    assert 0 < gold["crc_valid"].sum() < len(gold["crc_valid"])


def test_oracle_header_known_answers(oracle):
    rng = np.random.default_rng(5)
    for t in range(40):
        call = "".join(chr(int(c)) for c in rng.integers(48, 91, 8))
        h = synth.dstar_header_bytes("DB0ABC G", "DB0ABC B", "CQCQCQ", call, "X%d" % t, flags=(int(rng.integers(0, 128)), 0, 0))
        bits = synth.dstar_header_bits(h)
        ok, out = oracle.dstar_header_parse(bits)
        assert ok and bytes(out) == h
        few = bits.copy(); few[rng.choice(660, 4, replace=False)] ^= 1  # isolated errors are corrected
        ok, out = oracle.dstar_header_parse(few)
        assert ok and bytes(out) == h
        many = bits.copy(); many[rng.choice(660, 60, replace=False)] ^= 1
        assert not oracle.dstar_header_parse(many)[0]                   # metric > 10 or CRC failure
        bad = bytearray(h); bad[int(rng.integers(0, 39))] ^= 0x10       # a consistent code word with a wrong FCS
        assert not oracle.dstar_header_parse(synth.dstar_header_bits(bytes(bad)))[0]


def _headers(ev):
    h = ev[ev["type"] == EV_HEADER]
    return [(int(a["b"]), bytes(a["payload"][:24]) + bytes(b["payload"][:17])) for a, b in zip(h[0::2], h[1::2])]


@pytest.mark.parametrize("seed", [3, 4])
def test_decoder_on_bits_matches_oracle(ctx, oracle, seed):
    clean, infos = synth.dstar_stream(seed, 8)
    noisy, _ = synth.dstar_stream(seed, 8, ber=0.004)                  # corrected headers, missed syncs, broken slow data
    for stream in (clean, noisy):
        want = expected(oracle, "dstar", stream[None])
        out, ev = want[0]
        if stream is clean:                                            # the stream says what it should: headers, messages, voice
            heads = _headers(ev)
            for i in infos:
                if i["kind"] not in (3, 6, 7):
                    assert (0, i["header"]) in heads
                if i["kind"] != 4 and i["frames"] > 44:
                    assert (1, i["header"]) in heads
                assert i["kind"] == 6 or any(bytes(m["payload"][:20]).decode("latin1").rstrip() == i["message"].rstrip()
                                             for m in ev[ev["type"] == EV_MESSAGE])
            simple = b"".join(bytes(e["payload"][:e["len"]]) for e in ev[ev["type"] == EV_SIMPLE])
            assert all(i["simple"] in simple for i in infos if i["kind"] != 6)
            # the voice bytes are the AMBE bits sent: all of them behind a radio header; behind a voice sync (no header, kind 3;
            # a data or a broken header, kinds 6 and 7, where the search meets the first sync frame) the 20 frames up to the next
            # sync frame and that frame itself are heard but not written (dstar_phase.cpp:59, :76, :101-113)
            sent = [i["voice"][{3: 21, 6: 22, 7: 22}.get(i["kind"], 0):] for i in infos]
            assert bytes(out) == b"".join(bytes(v) for t in sent for v in t)
            assert (ev["type"] == EV_META_RESET).sum() >= sum(i["kind"] != 6 for i in infos)
        for chunk in (len(stream), 1000, 97):
            assert_rows(run_symbols(ctx, "dstar", stream[None], chunk), want, "pushes of %d" % chunk)


def test_decoder_on_noise_and_sync_storms(ctx, oracle):
    """Random bits (false syncs, false header starts), runs of sync words, and a header cut by the end of the input."""
    rng = np.random.default_rng(11)
    h = synth.dstar_header_bits(synth.dstar_header_bytes("A", "B", "C", "D"))
    parts = [rng.integers(0, 2, 30000).astype(np.uint8)]
    for _ in range(40):
        parts += [np.array([1, 0] * 16 + synth.DSTAR_FRAME_SYNC, np.uint8), rng.integers(0, 2, int(rng.integers(0, 700))).astype(np.uint8),
                  np.array(synth.DSTAR_VOICE_SYNC, np.uint8), rng.integers(0, 2, int(rng.integers(0, 300))).astype(np.uint8),
                  np.array(synth.DSTAR_TERMINATOR, np.uint8)]
    parts += [np.array([1, 0] * 16 + synth.DSTAR_FRAME_SYNC, np.uint8), h[:500]]
    stream = np.concatenate(parts)
    want = expected(oracle, "dstar", stream[None])
    ev = want[0][1]
    assert (ev["type"] == EV_VOICE_START).sum() >= 5 and (ev["type"] == EV_META_RESET).sum() >= 5
    for chunk in (len(stream), 4096, 661):
        assert_rows(run_symbols(ctx, "dstar", stream[None], chunk), want, "pushes of %d" % chunk)


def test_full_chain_fsk_sps10(ctx, oracle):
    chans = []
    for i, seed in enumerate((21, 22, 23)):
        bits, _ = synth.dstar_stream(seed, 3)
        x = synth.fsk_shape(bits, sps=10)
        chans.append(synth.impair(x, seed, snr_db=[None, 20, 14][i], dc=[0.0, 0.1, -0.05][i], delay=3 * i, gain=[1, 0.6, 1.5][i]))
    n = min(len(c) for c in chans)
    x = np.stack([c[:n] for c in chans])
    ref = oracle.chain(x, rrc=0, levels=2, sps=10, proto=5)
    assert ref["out_count"].min() > 0
    for chunks in ([n], [48000, 12345]):
        for split in (False, True):                    # one-wavefront chain kernel / slicer and decoder as two launches
            res = run_engine(ctx, x, "dstar", chunks, rrc="none", demod="fsk", sps=10, split_stages=split)
            assert_matches_oracle(res, ref, len(x), "dstar %s %s" % (chunks[:1], "split" if split else "chain"))


def test_tiny_empty_and_ragged_pushes(ctx, oracle):
    """Pushes of 0..13 samples, one just under / over a bit, and a header that arrives split over many pushes."""
    bits, _ = synth.dstar_stream(31, 2)
    x = synth.impair(synth.fsk_shape(bits, sps=10), 3, snr_db=25, dc=0.02)[None, :]
    ref = oracle.chain(x, rrc=0, levels=2, sps=10, proto=5)
    assert ref["out_count"][0] > 0
    res = run_engine(ctx, x, "dstar", [1, 0, 2, 3, 9, 10, 11, 13, 0, 659, 661, 6600, 37, 5000], rrc="none", demod="fsk", sps=10)
    assert_matches_oracle(res, ref, 1)
    # decoder-only engine fed 1 .. 7 bits at a time through a header and the first superframe
    rng = np.random.default_rng(8)
    stream = np.concatenate([rng.integers(0, 2, 50).astype(np.uint8), synth.dstar_transmission(rng, n_superframes=1)[0]])
    want = expected(oracle, "dstar", [stream])
    assert_rows(run_symbols(ctx, "dstar", [stream], [1, 7, 0, 3, 5, 2], cycle=True, pitch=64), want)
    assert (want[0][1]["type"] == EV_HEADER).sum() >= 2


def test_decoder_only_rows_at_odd_addresses(ctx, oracle):
    """Three channels in a symbol buffer with an odd row pitch: the packed fast path funnel-shifts unaligned rows."""
    streams = [synth.dstar_stream(s, 4)[0] for s in (41, 42, 43)]
    n = min(len(s) for s in streams)
    rows = [s[:n] for s in streams]
    want = expected(oracle, "dstar", rows)
    assert all(len(out) > 0 for out, _ in want)
    assert_rows(run_symbols(ctx, "dstar", rows, 1501, pitch=1503), want)


# ------------------------------------------------------------------ the five-frame fast path of the voice phase, by construction
VOICE_AT = 64 + 15 + 660                       # dstar_transmission: bit sync, frame sync, header; then 96-bit frames


def _assert_rows_match(ctx, oracle, rows, pushes, pitch=None):
    """rows [B][n] in pushes of each of the given lists of sizes (cycled); pitch = row pitch of the pushed buffer"""
    want = expected(oracle, "dstar", rows)
    for sizes in pushes:
        run = run_symbols(ctx, "dstar", rows, sizes, cycle=True, pitch=max(max(sizes), 64) if pitch is None else pitch)
        assert_rows(run, want, "pushes of %s" % sizes[:2])
    return want


def test_end_pattern_at_every_frame_of_the_fast_path(ctx, oracle):
    """The end pattern, and its second half alone (dstar_phase.cpp:92-96), in the data frame of frame 1..20 of a superframe:
    each of the five positions of a fast-path batch, in each of the four batches.  The batch has to stop in front of that
    frame.  Four channels of ten transmissions; after each end the search has to find the next header."""
    rng = np.random.default_rng(60)
    term = np.array(synth.DSTAR_TERMINATOR, np.uint8)
    rows = [[rng.integers(0, 2, 30 + c).astype(np.uint8)] for c in range(4)]
    for k, (idx, half) in enumerate((i, h) for h in (False, True) for i in range(1, 21)):
        b, _, _ = synth.dstar_transmission(rng, my="T%02d" % idx, message="end in frame %d" % idx, n_superframes=2)
        at = VOICE_AT + 96 * (21 + idx) + 72
        tail = term[24:] if half else term
        rows[k % 4] += [b[:at], tail, rng.integers(0, 2, int(rng.integers(150, 400))).astype(np.uint8)]
    rows = stack_rows([np.concatenate(r) for r in rows])
    want = _assert_rows_match(ctx, oracle, rows, ([rows.shape[1]], [4096], [997]))
    ev = np.concatenate([e for _, e in want])
    assert ((ev["type"] == EV_META_RESET) & (ev["b"] == 0)).sum() >= 40 and (ev["type"] == EV_MESSAGE).sum() >= 40


def test_symbols_with_bit_1_set_in_every_byte_lane_of_a_batch(ctx, oracle):
    """A symbol 2 or 3 in each of the 60 eight-symbol lanes of a batch (frames 1..5 of a superframe, and one more in frames
    11..15): the batch must go frame by frame, where the reference compares whole symbols (a difference in a sync or end
    pattern) and packs bit 0."""
    rng = np.random.default_rng(61)
    rows = []
    for c in range(4):
        b, _, _ = synth.dstar_transmission(rng, my="ODD%d" % c, n_superframes=16, simple=synth.dstar_dprs_sentence("X>APDPRS:!4916.45N/01131.00E>"))
        b = b.copy()
        for k in range(1, 16):
            lane = 15 * c + k - 1
            b[VOICE_AT + 96 * (21 * k + 1) + 8 * lane + lane % 8] |= 2
            b[VOICE_AT + 96 * (21 * k + 11) + 8 * (lane * 7 % 60) + 7 - lane % 8] |= 2
        rows.append(np.concatenate([rng.integers(0, 2, 40 + c).astype(np.uint8), b, rng.integers(0, 2, 300).astype(np.uint8)]))
    rows = stack_rows(rows)
    assert (rows > 1).sum() == 4 * 30
    want = _assert_rows_match(ctx, oracle, rows, ([rows.shape[1]], [5000]))
    assert all(len(o) // 9 >= 16 * 21 - 2 for o, _ in want)                 # the calls went through to their ends


def test_fast_path_at_the_end_of_a_push_at_every_row_misalignment(ctx, oracle):
    """A batch needs 516 symbols of the push from its (aligned) first word: pushes of 515..518 + 96 k symbols put the last
    batch of a push on both sides of that limit, and four rows at a pitch of 4 m + 3 bytes give every misalignment."""
    rng = np.random.default_rng(62)
    rows = []
    for c in range(4):
        b, _, _ = synth.dstar_transmission(rng, my="MIS%d" % c, n_superframes=9, message="misaligned row %d" % c)
        rows.append(np.concatenate([rng.integers(0, 2, 33 + 5 * c).astype(np.uint8), b, rng.integers(0, 2, 200).astype(np.uint8)]))
    sizes = [515 + d + 96 * k for k in range(3) for d in range(4)]
    want = _assert_rows_match(ctx, oracle, stack_rows(rows), (sizes, sizes[::-1], [s + 96 for s in sizes[5:] + sizes[:5]]), pitch=811)
    assert all(len(o) // 9 >= 9 * 21 - 2 and (e["type"] == EV_MESSAGE).sum() >= 4 for o, e in want)


def test_superframe_that_begins_without_sync_collects_slow_data_only(ctx, oracle):
    """Late entry: the voice phase starts at a data-frame sync with a sync count of 0.  Until the next sync frame no voice
    bytes are written, but the slow data of that superframe is collected and its message comes out at that sync frame
    (dstar_phase.cpp:60-70, :81-86, :122-129)."""
    rng = np.random.default_rng(63)
    rows = []
    sent = []
    for c in range(2):
        b, _, voice = synth.dstar_transmission(rng, my="LATE%d" % c, message="late entry %d" % c, n_superframes=3, with_header=False, inline_header=False)
        sent.append(np.concatenate(voice[21:]))                            # 20 data frames and the first due sync frame are heard, not written
        rows.append(np.concatenate([np.zeros(50 + 3 * c, np.uint8), b, rng.integers(0, 2, 300).astype(np.uint8)]))
    rows = stack_rows(rows)
    want = _assert_rows_match(ctx, oracle, rows, ([rows.shape[1]], [1000], [97]))
    for (o, e), v in zip(want, sent):
        start = e[e["type"] == EV_VOICE_START]
        assert len(start) >= 1 and start[0]["b"] == 0                      # entered at a voice sync, not behind a header
        assert (e["type"] == EV_MESSAGE).sum() == 3 and len(o) == 9 * 43 and (o == v).all()      # three superframes' messages; the voice sent, from the second superframe's frame 1 on
