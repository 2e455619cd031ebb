"""POCSAG (examples/pocsag-decoder.sh: fsk_demodulator -i -s 40 | pocsag_decoder).

* BCH(31,21): oracle and product against tests/golden/pocsag_ref.npz, whose expected values come from the reference's
  own bch_31_21.c compiled in place (PINNED);
* the decoder on bits and the whole chain on 2-level FSK audio, engine (CPU wave emulation / MI355X) against the oracle;
  the decoded pages are the module's output bytes (`address:<n>;message:<text>` lines).
"""
import os

import numpy as np
import pytest

from digiham_amd import synth
from common import assert_matches_oracle, run_engine
from dec_harness import assert_rows, expected, run_symbols, stack_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "pocsag_ref.npz"))


def test_oracle_bch_matches_the_reference_vectors(oracle, gold):
    out, ok = oracle.block_decode("bch_31_21", gold["bch_in"])
    assert (ok == gold["bch_ok"]).all() and (np.where(ok == 1, out, 0) == gold["bch_out"]).all()
    assert 5000 < int(ok.sum()) < len(ok)


def test_product_bch_matches_the_reference_vectors(ctx, gold):
    out, ok = ctx.block_decode("bch_31_21", gold["bch_in"])
    assert (ok == gold["bch_ok"]).all() and (np.where(ok == 1, out, 0) == gold["bch_out"]).all()


@pytest.mark.parametrize("seed", [3, 4])
def test_decoder_on_bits_matches_oracle(ctx, oracle, seed):
    bits, sent = synth.pocsag_stream(seed, 8)
    rng = np.random.default_rng(seed)
    noisy = bits.copy()
    hit = rng.random(len(bits)) < 0.004                # bit errors: BCH corrections, dropped messages, lost sync words
    noisy[hit] ^= 1
    for stream in (bits, noisy):
        want = expected(oracle, "pocsag", stream[None])
        lines = bytes(want[0][0]).decode("latin1").split("\n")
        if stream is bits:                             # most pages come out verbatim (a transmission right behind another is missed)
            assert sum(("address:%d;message:%s" % (a, t)) in lines for a, f, t in sent) >= len(sent) // 2
        for chunk in (len(stream), 1000, 97):
            assert_rows(run_symbols(ctx, "pocsag", stream[None], chunk), want, "pushes of %d" % chunk)


def test_full_chain_fsk_inverted_sps40(ctx, oracle):
    chans = []
    for i, seed in enumerate((21, 22)):
        bits, _ = synth.pocsag_stream(seed, 3)
        x = synth.fsk_shape(bits, sps=40, invert=True)
        chans.append(synth.impair(x, seed, snr_db=[None, 20][i], dc=[0.0, 0.1][i], delay=11 * i, gain=[1, 0.6][i]))
    n = min(len(c) for c in chans)
    x = np.stack([c[:n] for c in chans])
    ref = oracle.chain(x, rrc=0, levels=2, invert=True, sps=40, proto=4)
    assert ref["out_count"].sum() > 0
    for chunks in ([n], [48000, 12345]):
        res = run_engine(ctx, x, "pocsag", chunks, rrc="none", demod="fsk", sps=40, invert=True)
        assert_matches_oracle(res, ref, len(x), "pocsag %s" % chunks[:1])


def _transmission(words, missed_sync=(), odd=()):
    """preamble + batches of 16 codewords; the sync words of the batches in `missed_sync` are replaced by an idle codeword
    (the grid has to survive on its hysteresis); the bits at the offsets in `odd` arrive as symbols 2 / 3 (bit 1 set)"""
    words = list(words) + [synth.POCSAG_IDLE] * (-len(words) % 16)
    bits = [1, 0] * 288
    for j in range(len(words) // 16):
        for w in [synth.POCSAG_IDLE if j in missed_sync else synth.POCSAG_SYNC] + words[16 * j:16 * j + 16]:
            bits += synth._bits_of(w, 32)
    bits = np.array(bits, np.uint8)
    for k in odd:
        bits[576 + k] |= 2
    return bits


def _edge_streams():
    """Eight channels of what synth.pocsag_stream never sends (its pages: function 3, 3..39 characters, an idle codeword
    behind every page, clean sync words): all four functions, empty pages, texts around the 80-character limit of
    message.cpp:29-38 (77..81 and 120 characters) and a NUL inside a text (the string ends there), an address codeword
    directly behind another page, one / two / three missed sync words in a row (ridden out, pocsag_phase.cpp:40-52) and
    four (grid dropped), symbols with bit 1 set inside sync words, address and message codewords."""
    rng = np.random.default_rng(77)
    text = lambda n: "".join(chr(int(c)) for c in rng.integers(32, 127, n))
    addr = lambda a, f: synth.pocsag_codeword(((a >> 3) & 0x3FFFF) << 2 | (f & 3))
    page = lambda a, f, t: [addr(a, f)] + [synth.pocsag_codeword(1 << 20 | pl) for pl in synth.pocsag_alpha_payloads(t)]
    gap = lambda: list(rng.integers(0, 2, int(rng.integers(3300, 3400))))      # (longer than the grid outlives a transmission)
    rows = []
    # functions 0..3, empty and short pages, every page in the frame its address selects
    rows.append(np.concatenate([np.concatenate([_transmission(synth.pocsag_batches([(int(rng.integers(8, 1 << 21)), f, t)])), gap()])
                                for f in range(4) for t in ("", text(9))]))
    # lengths around the cut of the 560-bit buffer; a NUL in the middle of a text
    rows.append(np.concatenate([np.concatenate([_transmission(synth.pocsag_batches([(int(rng.integers(8, 1 << 21)), 3, t)])), gap()])
                                for t in [text(n) for n in (77, 78, 79, 80, 81, 120)] + [text(12) + "\0" + text(12)]]))
    # address codewords back to back: an empty page, a page, a page, idle -- twice, once starting at an odd codeword
    for lead in (0, 3):
        a = [int(x) for x in rng.integers(8, 1 << 21, 4)]
        words = [synth.POCSAG_IDLE] * lead + [addr(a[0], 3)] + page(a[1], 3, text(14)) + page(a[2], 1, text(30)) + [addr(a[3], 3), synth.POCSAG_IDLE]
        rows.append(np.concatenate([_transmission(words), gap()]))
    # missed sync words at batch boundaries: pages in every batch, sync word of batches 2 / 2-3 / 2-4 / 2-5 replaced
    for missed in ((2,), (2, 3), (2, 3, 4), (2, 3, 4, 5)):
        words = []
        for j in range(8):
            words += ([synth.POCSAG_IDLE] * 2 + page(8 * int(rng.integers(1, 1 << 17)) + 1, 3, text(25)) + [synth.POCSAG_IDLE] * 16)[:16]
        rows.append(np.concatenate([_transmission(words, missed_sync=missed), gap()]))
    # symbols 2 / 3 in the first batch's sync word, an address codeword and a message codeword, on the page of row 2
    words = [synth.POCSAG_IDLE] * 2 + page(8 * 4711 + 1, 3, text(40))
    for odd in ((3,), (3, 17, 30), (32 * 3 + 5,), (32 * 4 + 9, 32 * 5 + 1), (1, 32 * 3 + 31, 32 * 6)):
        rows.append(np.concatenate([_transmission(words, odd=odd), gap()]))
    return stack_rows(rows)


def test_decoder_edges_match_oracle(ctx, oracle):
    rows = _edge_streams()
    want = expected(oracle, "pocsag", rows)
    lines = [bytes(o).decode("latin1").split("\n") for o, _ in want]
    assert len(lines[0]) - 1 >= 1 and len(lines[1]) - 1 >= 6               # pages came out (only function 3 yields text, message.cpp:27-72)
    assert max(len(l) for l in lines[1]) >= 77 + len("address:8;message:")
    for missed in range(4):                                                  # 1..3 missed sync words: the later pages still arrive; 4: fewer
        assert len(lines[4 + missed]) - 1 >= 5 if missed < 3 else len(lines[4 + missed]) < len(lines[4])
    for chunk in (rows.shape[1], 1000, 97, 33):
        assert_rows(run_symbols(ctx, "pocsag", rows, chunk), want, "pushes of %d" % chunk)
