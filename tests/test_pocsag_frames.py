"""POCSAG pages through the product, held to what the test sent.

Decoder-only engines (the CPU wave emulation and, with -m gpu, libdigiham_amd.so) are fed transmissions built from
synth.pocsag_codeword / pocsag_alpha_payloads / pocsag_batches and test_pocsag._transmission.  Every output byte and every
event is held to `_Pager` below: the codeword machine of pocsag_phase.cpp:18-92 and message.cpp:17-36 restated in a few
lines and fed with what the TEST put on the air -- the codewords it encoded, the sync words it damaged.  What a damaged
codeword decodes to is taken from the reference's own Codeword::parse compiled in place (tests/golden/frames_ref.npz,
make_golden_frames.py).  The oracle is no comparand here: once the engine has been held to the expectation, the CPU leg
holds oracle/decoders.c to the same expectation.

sym_index (include/digiham_amd.h: "absolute symbol index of the frame start"): a CODEWORD event carries the stream
position of its codeword's first symbol.

Between transmissions the rows are silent (zeros) for as long as the decoder keeps its batch grid: the all-zero word is a
valid codeword (the code is linear; synth.pocsag_codeword(0) == 0), so what the decoder makes of the silence is known from
the sender's side -- an address codeword of function 0 in every slot.  Random bits follow only once the grid is lost.
"""
import json
import os
from collections import Counter

import numpy as np
import pytest

from common import npz_digest
from dec_harness import assert_rows, event_record, expected, frames_fixture, is_emu, run_symbols, stack_rows
from digiham_amd import api, synth
from test_pocsag import _transmission

HERE = os.path.dirname(os.path.abspath(__file__))
EV_CODEWORD = 48
SYNC_BITS = np.array(synth._bits_of(synth.POCSAG_SYNC, 32), np.uint8)
IDLE = synth.POCSAG_IDLE
PUSHES = (None, 500, 33)                      # one push, pushes of a few hundred symbols, a prime below one codeword + 1


@pytest.fixture(scope="module")
def fx():
    return frames_fixture()


def _word_of(bits32):
    return int((np.asarray(bits32, np.uint64) << np.arange(31, -1, -1, dtype=np.uint64)).sum())


def _sync_distance(window):
    """hamming_distance() of 32 symbols against the sync word (pocsag_phase.cpp:11): a symbol differs or it does not"""
    return int((np.asarray(window) != SYNC_BITS).sum())


# ------------------------------------------------------------------ the fixture itself
def test_fixture_conditions_and_reference(oracle, fx):
    """The committed codewords are the ones the reference judged (digest taken at generation; oracle/_ref, where it is built,
    reproduces every column), each class is populated -- repaired, rejected by the BCH decoder, rejected on parity alone
    (codeword.cpp:21-28) --, and the oracle's restatement agrees with all of them."""
    path = os.path.join(HERE, "golden", "frames_ref.npz")
    assert npz_digest(path) == json.load(open(os.path.join(HERE, "golden", "ref_compare_hashes.json")))["frames_ref_npz"]
    assert os.path.getsize(path) < 300 * 1024
    ok, bch, flips = fx["cw_ok"] == 1, fx["cw_bch_ok"] == 1, fx["cw_flips"]
    same = fx["cw_word"] == fx["cw_sent"]
    assert fx["cw_in"].shape[1] == 32 and set(np.unique(fx["cw_in"])) == {0, 1}
    assert (ok & same).sum() >= 50 and (ok & ~same).sum() >= 5           # repaired; repaired into ANOTHER codeword than sent
    assert (~ok & ~bch).sum() >= 20 and (~ok & bch).sum() >= 20          # beyond the BCH decoder; BCH content, parity odd
    assert not (ok & ~bch).any() and (fx["cw_word"][~ok] == 0).all()
    single = flips == 1
    wrong = (fx["cw_in"] != np.array([synth._bits_of(int(w), 32) for w in fx["cw_sent"]], np.uint8))
    assert (wrong.sum(axis=1) == flips).all()
    assert (ok & same)[single & ~wrong[:, 31]].all() and (~ok & bch)[single & wrong[:, 31]].all()     # one wrong bit: repaired, unless it is the parity bit
    assert (ok & same)[(flips == 2) & ~wrong[:, 31]].all()               # two wrong bits inside the BCH word: repaired (bch_31_21.c)
    for which in ("oracle", "ref"):
        if which == "ref" and (oracle.ref() is None or oracle.ref_lib("pocsag") is None):
            continue
        out, words = oracle.Elements(which).pocsag_codeword(fx["cw_in"])
        assert (out[:, 0] == fx["cw_ok"]).all() and (np.where(out[:, 0] == 1, words[:, 0], 0) == fx["cw_word"]).all(), which
        received = np.array([_word_of(b) for b in fx["cw_in"]], np.uint32)
        assert (oracle.block_decode("bch_31_21", received >> 1, which)[1] == fx["cw_bch_ok"]).all(), which


# ------------------------------------------------------------------ what the reference's codeword machine makes of what was sent
def _address(a, f):
    return synth.pocsag_codeword(((a >> 3) & 0x3FFFF) << 2 | (f & 3))


def _page(a, f, text):
    return [_address(a, f)] + [synth.pocsag_codeword(1 << 20 | pl) for pl in synth.pocsag_alpha_payloads(text)]


def _cut(text):
    """The text a function 3 page of `text` prints, from the sender's side (message.cpp:29-35, :20): 20-bit payloads are
    taken while pos + 20 < 560, i.e. 27 of them = 540 bits = 77 characters and bit 0 of the 78th; the string ends at the
    first zero byte."""
    chars = [ord(c) for c in text[:77]]
    if len(text) >= 78 and ord(text[77]) & 1:
        chars.append(1)
    return bytes(chars).split(b"\0")[0]


class _Pager:
    """One channel: the bits on the air and the lines / events SyncPhase and CodewordPhase give for them.

    `verdict` maps a received 32-bit word the test damaged to what the REFERENCE's Codeword::parse made of it; every other
    word on the air is a codeword the test encoded itself, which parse returns unchanged."""

    def __init__(self, rng, verdict, lead=41):
        self.rng, self.verdict = rng, verdict
        self.bits = [rng.integers(0, 2, lead).astype(np.uint8)]
        self.pos = lead
        self.locked, self.count, self.counter, self.msg = False, 0, 0, None
        self.search_from, self.walks = 0, []                        # (first position searched, position of the sync word found)
        self.lines, self.ev, self.seen = [], [], Counter()

    # ---- message.cpp
    def _print(self, why):
        m = self.msg
        if m is None:
            return
        if len(m["bits"]) == 0:                                      # message.cpp:18 -- function 1 pages never get here with text
            self.seen["empty page not printed (function %d)" % m["type"]] += 1
            return
        b = m["bits"] + [0] * (-len(m["bits"]) % 7)
        chars = bytes(sum(b[7 * i + k] << k for k in range(7)) for i in range(len(b) // 7))
        self.lines.append(b"address:%d;message:%s\n" % (m["address"], chars.split(b"\0")[0]))        # :19-21, std::string(content)
        self.seen["printed at " + why] += 1

    def _append(self, payload):
        m = self.msg
        if m["type"] == 3:                                           # :28-36
            if len(m["bits"]) + 20 < 80 * 7:
                m["bits"] += [(payload >> (19 - i)) & 1 for i in range(20)]
            else:
                self.seen["payload beyond the text limit"] += 1

    # ---- pocsag_phase.cpp
    def _codeword(self, received, at):
        if received in self.verdict:
            ok, word = self.verdict[received]
            self.seen["damaged codeword " + ("repaired" if ok else "rejected")] += 1
        else:
            assert synth.pocsag_codeword(received >> 11) == received, hex(received)       # a codeword of the encoder's
            ok, word = True, received
        if ok:                                                       # :55
            self.ev.append(event_record(at, EV_CODEWORD, self.counter, 0, int(word).to_bytes(4, "big")))
            if word == IDLE:                                         # :56-61
                self._print("idle")
                self.msg = None
            elif word >> 31 == 0:                                    # :62-75
                self._print("address")
                self.msg = None
                f = (word >> 11) & 3
                self.seen["address function %d" % f] += 1
                if f in (1, 3):
                    self.msg = {"address": ((word >> 13) & 0x3FFFF) << 3 | self.counter // 2, "type": f, "bits": []}
            elif self.msg is not None:                               # :76-79
                self._append((word >> 11) & 0xFFFFF)
                self.seen["payload appended" + (" (repaired)" if received in self.verdict else "")] += 1
            else:
                self.seen["message codeword without a page"] += 1
        else:                                                        # :82-85
            self.seen["page dropped" if self.msg is not None else "rejected without a page"] += 1
            self.msg = None
        self.counter += 1                                            # :88

    def transmit(self, words, sync=None, preamble=True):
        """preamble (unless the transmission goes on) + batches of sync word + 16 received words.  sync: batch -> "idle"
        (an idle codeword in the sync slot), "zero", a tuple of bit positions of the sync word that are inverted, or
        ("slip", bits): these bits come in front of the intact sync word, and the batch grid is that much later from there on"""
        sync = sync or {}
        words = list(words) + [IDLE] * (-len(words) % 16)
        bits = _transmission(words, missed_sync=[j for j, s in sync.items() if s == "idle"])
        slips = {j: s[1] for j, s in sync.items() if s[0] == "slip"}
        for j, s in sync.items():
            at = 576 + 544 * j
            if s == "zero":
                bits[at:at + 32] = 0
            elif s != "idle" and j not in slips:
                bits[at + np.array(s, int)] ^= 1
        for j in sorted(slips, reverse=True):
            bits = np.insert(bits, 576 + 544 * j, slips[j])
        if not preamble:
            bits = bits[576:]
        else:
            assert not self.locked
        self.bits.append(bits)
        p = self.pos + (576 if preamble else 0)
        self.pos += len(bits)
        for j in range(len(words) // 16):
            d = _sync_distance(bits[p - (self.pos - len(bits)):][:32])
            if j in sync and sync[j] not in ("idle", "zero") and j not in slips:
                assert d == len(sync[j])
            if self.locked:                                          # :39-52
                assert self.counter == 16
                if d <= 3:
                    self.seen["sync word hit at count %d, distance %d" % (self.count, d)] += 1
                    old = self.count; self.count += 1                # `if (syncCount++ > 2) syncCount = 2;`
                    if old > 2:
                        self.count = 2
                else:
                    old = self.count; self.count -= 1                # `if (syncCount-- < 0)`
                    if old < 0:
                        self._print("sync loss")
                        self.seen["sync lost"] += 1
                        self.locked, self.msg, self.search_from = False, None, p      # the search resumes HERE: no advance (:47)
                    else:
                        self.seen["sync word missed at count %d%s" % (old, ", distance 4" if isinstance(sync.get(j), tuple) else "")] += 1
            assert j not in slips or not self.locked, "a grid that slips has to be lost at that sync word"
            if not self.locked:                                      # :18-28
                if j in slips:                                       # the search goes bit by bit and meets the sync word where it is
                    p += len(slips[j])
                    d = _sync_distance(bits[p - (self.pos - len(bits)):][:32])
                    self.seen["sync word found %d bits behind the position of the loss" % (p - self.search_from)] += 1
                if d > 3:
                    p += 544
                    continue
                self.walks.append((self.search_from, p))
                self.locked, self.count, self.counter, self.msg = True, 1, 0, None   # pocsag_phase.hpp:33-35
            p += 32
            self.counter = 0
            for w in words[16 * j:16 * j + 16]:
                self._codeword(int(w), p)
                p += 32
        return self

    def silence(self):
        """zeros, in whole batches, until the decoder has given up its grid; then random bits (searched, so free of sync words)"""
        n = 0
        while self.locked:
            self.transmit([0] * 16, sync={0: "zero"}, preamble=False)
            n += 1
        self.seen["missed sync words ridden out before a loss: %d" % (n - 1)] += 1
        noise = self.rng.integers(0, 2, int(self.rng.integers(40, 90))).astype(np.uint8)
        self.bits.append(noise); self.pos += len(noise)
        return self

    def row(self):
        assert not self.locked
        return np.concatenate(self.bits)

    def check_search(self, row):
        """the sync search finds the sync words the test sent and nothing else (pocsag_phase.cpp:11, :19)"""
        d = (np.lib.stride_tricks.sliding_window_view(row, 32) != SYNC_BITS).sum(axis=1)
        for a, hit in self.walks + [(self.search_from, None)]:
            stop = len(d) if hit is None else hit
            assert (d[a:stop] > 3).all(), (a, hit, np.flatnonzero(d[a:stop] <= 3)[:3] + a)
            assert hit is None or d[hit] <= 3

    def events(self):
        return np.concatenate(self.ev) if self.ev else np.zeros(0, api.EVENT_DTYPE)

    def output(self):
        return np.frombuffer(b"".join(self.lines), np.uint8)


def _hold(ctx, oracle, pagers, pushes=PUSHES):
    """the engine, pushed three ways, gives exactly what the pagers expect; then oracle/decoders.c does"""
    rows = stack_rows([p.row() for p in pagers])
    assert rows.shape[0] <= 8 and rows.shape[1] <= 25000 and rows.max() <= 1
    for p, r in zip(pagers, rows):
        p.check_search(r)                                            # before any decoder runs
    want = [(p.output(), p.events()) for p in pagers]
    for size in pushes:
        assert_rows(run_symbols(ctx, "pocsag", rows, size, pitch=max(size or rows.shape[1], 64)), want, "pushes of %s" % size)
    if is_emu(ctx):
        assert_rows(expected(oracle, "pocsag", rows), want, "the oracle")
    seen = Counter()
    for p in pagers:
        seen.update(p.seen)
    return seen


def _verdicts(fx):
    return {_word_of(b): (bool(ok), int(w)) for b, ok, w in zip(fx["cw_in"], fx["cw_ok"], fx["cw_word"])}


def _text(rng, n):
    return "".join(chr(int(c)) for c in rng.integers(32, 127, n))


# ------------------------------------------------------------------ pages
def test_pages_by_function_and_position(ctx, oracle, fx):
    """address:<n>;message:<text> with n = (18 address bits << 3) | (codeword index // 2) (pocsag_phase.cpp:73) for pages
    that begin at every codeword index; functions 0 and 2 open nothing (:70), function 1 opens a page that never prints
    (message.cpp:27-36 appends nothing, :18), an empty function 3 page prints nothing (:18); an address codeword prints the
    page before it (:63-65); a message codeword with no page open is ignored (:77)."""
    rng = np.random.default_rng(501)
    pagers = []
    p, sent = _Pager(rng, _verdicts(fx)), []                         # every function, with text and empty, in the frame the address selects
    for k, (f, t) in enumerate((f, t) for f in range(4) for t in ("", _text(rng, 9))):
        a = int(rng.integers(8, 1 << 21))
        p.transmit(synth.pocsag_batches([(a, f, t)]), preamble=k == 0)
        if f == 3 and t:
            sent.append(b"address:%d;message:%s\n" % (a, t.encode("latin1")))
    p.silence()
    assert b"".join(p.lines) == b"".join(sent) and len(sent) == 1    # the sender's view of the whole row
    pagers.append(p)
    p, sent, words = _Pager(rng, _verdicts(fx), lead=70), [], []     # a page at every codeword index: the low address bits come from the position
    for k in range(16):                                              # three codewords each: they begin at 0, 3, 6, .. mod 16, every index once
        hi, t = int(rng.integers(1, 1 << 18)), _text(rng, 2)
        sent.append(b"address:%d;message:%s\n" % (hi << 3 | (3 * k % 16) // 2, t.encode("latin1")))
        words += _page(hi << 3, 3, t) + [IDLE]
    assert len(words) == 48 and sorted(3 * k % 16 for k in range(16)) == list(range(16))
    p.transmit(words).silence()
    assert b"".join(p.lines) == b"".join(sent)
    pagers.append(p)
    p = _Pager(rng, _verdicts(fx), lead=33)                          # address codewords back to back, over a batch boundary too
    a = [int(x) for x in rng.integers(8, 1 << 21, 6)]
    t = [_text(rng, n) for n in (14, 30, 7, 22)]
    words = [IDLE] * 3 + [_address(a[0], 3)] + _page(a[1], 3, t[0]) + _page(a[2], 1, t[1]) + [_address(a[3], 2)] + \
        [synth.pocsag_codeword(1 << 20 | 0x54321)] + _page(a[4], 3, t[2]) + _page(a[5], 3, t[3]) + [_address(a[0], 0)] + \
        [synth.pocsag_codeword(1 << 20 | 0x12345), IDLE]
    p.transmit(words).silence()
    assert [l.split(b":")[-1] for l in p.lines] == [x.encode("latin1") + b"\n" for x in (t[0], t[2], t[3])] and len(words) > 16
    pagers.append(p)
    seen = _hold(ctx, oracle, pagers)
    for f in range(4):
        assert seen["address function %d" % f] >= 2, seen
    for k in ("printed at idle", "printed at address", "empty page not printed (function 3)", "empty page not printed (function 1)",
              "message codeword without a page"):
        assert seen[k] >= 1, (k, seen)


def test_text_is_cut_at_540_bits(ctx, oracle, fx):
    """message.cpp:29: payloads are appended while pos + 20 < 560 -- 27 payloads, 77 characters and bit 0 of the 78th (which
    prints as a character of value 1 when set) -- and the printed string ends at the first zero byte (:20)."""
    rng = np.random.default_rng(502)
    texts = []
    for n in (76, 77, 78, 79, 80, 81, 82, 120):
        for bit in (0, 1):
            t = list(_text(rng, n))
            if n >= 78:
                t[77] = chr(int(rng.integers(16, 63)) << 1 | bit)
            texts.append("".join(t))
    assert {ord(t[77]) & 1 for t in texts if len(t) >= 78} == {0, 1}
    texts += [_text(rng, 12) + "\0" + _text(rng, 12), _text(rng, 77) + "\0" + _text(rng, 5)]
    assert {len(_cut(t)) for t in texts} == {12, 76, 77, 78}
    pagers = [_Pager(rng, _verdicts(fx), lead=37 + 5 * k) for k in range(3)]
    for k, p in enumerate(pagers):
        pages = [(int(rng.integers(8, 1 << 21)), 3, t) for t in texts[k::3]]
        p.transmit(synth.pocsag_batches(pages)).silence()
        assert b"".join(p.lines) == b"".join(b"address:%d;message:%s\n" % (a, _cut(t)) for a, _, t in pages)    # machine and sender-side rule agree
    seen = _hold(ctx, oracle, pagers)
    assert seen["payload beyond the text limit"] >= 10 and seen["printed at idle"] == len(texts), seen


def test_what_ends_or_drops_a_page(ctx, oracle, fx):
    """pocsag_phase.cpp:54-85 with damaged codewords from the fixture: one the reference cannot repair (beyond the BCH
    decoder, or BCH content with odd parity) drops the open page unprinted (:82-85); one it repairs -- into the codeword
    sent or into another -- continues the page with the repaired payload (:78); a repaired address codeword opens its page
    with the repaired address."""
    rng = np.random.default_rng(503)
    ok, bch = fx["cw_ok"] == 1, fx["cw_bch_ok"] == 1
    received = [_word_of(b) for b in fx["cw_in"]]
    rows_of = lambda cond: [r for r, c in zip(received, cond) if c]
    word, sent = fx["cw_word"].astype(np.int64), fx["cw_sent"].astype(np.int64)
    is_msg, damaged = (word >> 31) == 1, np.array(received, np.int64) != word
    classes = {"bch": rows_of(~ok & ~bch), "parity": rows_of(~ok & bch), "repaired": rows_of(ok & (word == sent) & is_msg & damaged),
               "other": rows_of(ok & (word != sent) & is_msg), "address": rows_of(ok & ~is_msg & ((word >> 11) & 3 == 3) & damaged)}
    assert all(len(v) >= 6 for v in classes.values()), {k: len(v) for k, v in classes.items()}
    pagers = []
    for row in range(3):
        p = _Pager(rng, _verdicts(fx), lead=35 + 9 * row)
        first = True
        for cls in ("bch", "parity", "repaired", "other", "address"):
            for k, w in enumerate(classes[cls][row::3][:2]):
                a = int(rng.integers(8, 1 << 21))
                body = _page(a, 3, _text(rng, 11))                   # address + 4 payloads
                if cls == "address":
                    words = [IDLE] * (k + 1) + [w] + body[1:] + [IDLE]
                else:
                    words = [IDLE] * (2 * k) + body[:2 + k] + [w] + body[2 + k:] + [IDLE] + _page(a ^ 8, 3, _text(rng, 4)) + [IDLE]
                n_before = len(p.lines)
                p.transmit(words, preamble=first)
                first = False
                assert len(p.lines) - n_before == {"bch": 1, "parity": 1, "repaired": 2, "other": 2, "address": 1}[cls], cls
        p.transmit([IDLE, classes["bch"][row], synth.pocsag_codeword(1 << 20 | 7), IDLE], preamble=False).silence()      # nothing open: nothing dropped
        pagers.append(p)
    seen = _hold(ctx, oracle, pagers)
    for k in ("page dropped", "rejected without a page", "damaged codeword repaired", "damaged codeword rejected", "payload appended (repaired)",
              "message codeword without a page", "printed at idle"):
        assert seen[k] >= 3, (k, seen)
    assert seen["page dropped"] == 12 and seen["payload appended (repaired)"] >= 12


def test_sync_word_hysteresis(ctx, oracle, fx):
    """pocsag_phase.cpp:39-52.  `if (syncCount++ > 2) syncCount = 2;` takes the count 1 -> 2 -> 3 -> 2 -> 3 ...;
    `if (syncCount-- < 0)` gives up at the miss that FINDS the count below zero: from a count of c, c + 1 missed sync words in
    a row are ridden out and the next one ends the grid.  From each reachable count (1 after the first sync word, 2 and 3
    after one and two more) one to five sync words in a row are replaced -- by an idle codeword, by zeros, by the sync word
    with four wrong bits; a sync word with three wrong bits counts as found (:11).  A page is open over every batch boundary:
    it goes on behind a missed sync word that is ridden out, and is printed at the loss (:44-46), where the search resumes at
    the missed sync word's own position (:47 returns without advancing): a sync word that comes 1, 5 or 31 bits late at that
    moment is found."""
    rng = np.random.default_rng(504)
    ridden = {}                                                      # count c -> misses ridden out, by running the test of :43 itself
    for c in (-1, 0, 1, 2, 3):
        n, count = 0, c
        while True:
            old = count; count -= 1
            if old < 0:
                break
            n += 1
        ridden[c] = n
    assert ridden == {-1: 0, 0: 1, 1: 2, 2: 3, 3: 4}
    pagers, lost_in_runs = [], 0
    for start, runs in ((1, (1, 2, 3)), (1, (4, 5)), (2, (1, 2, 3)), (2, (4, 5)), (3, (1, 2, 3)), (3, (4, 5))):
        p = _Pager(rng, _verdicts(fx), lead=30 + 7 * len(pagers))
        for run in runs:
            words = []
            for j in range(start + run + 1):                         # every batch: the rest of the last page, idle, ..., a page that stays open
                tail = _page(8 * int(rng.integers(1, 1 << 17)) + 6, 3, _text(rng, 8))          # address + 3 payloads: codewords 12..15
                head = [synth.pocsag_codeword(1 << 20 | pl) for pl in synth.pocsag_alpha_payloads(_text(rng, 5))]     # 2 more payloads
                words += head + [IDLE] * (12 - len(head)) + tail
            kind = ("idle", "zero", tuple(int(x) for x in rng.choice(32, 4, replace=False)))
            sync = {start + i: kind[(run + i) % 3] for i in range(run)}          # batch 0 locks, batches 1 .. start - 1 count up
            if start > 1:
                sync[1] = tuple(int(x) for x in rng.choice(32, 3, replace=False))          # three wrong bits: still a sync word
            n_lost = p.seen["sync lost"]
            p.transmit(words, sync=sync)
            assert (p.seen["sync lost"] > n_lost) == (run > ridden[start]), (start, run)
            lost_in_runs += run > ridden[start]
            p.silence()
        pagers.append(p)
    p = _Pager(rng, _verdicts(fx), lead=44)                          # the count past 3: 1 2 3 2 3 2 over six clean sync words, 1 2 3 2 3 over five
    for n, left in ((6, 2), (5, 3)):
        before = Counter(p.seen)
        words = _page(int(rng.integers(8, 1 << 21)), 3, _text(rng, 20)) + [IDLE]
        p.transmit(words + [IDLE] * (16 * n - len(words))).silence()
        assert (p.seen - before)["missed sync words ridden out before a loss: %d" % ridden[left]] == 1
    pagers.append(p)
    p = _Pager(rng, _verdicts(fx), lead=51)                          # the grid slips by 1, 5 and 31 bits at the sync word that ends it: found from there
    for n in (1, 5, 31):
        words = []
        for j in range(5):
            words += [IDLE] * 11 + _page(8 * int(rng.integers(1, 1 << 17)) + 5, 3, _text(rng, 11)) + [IDLE] * (j == 4)
        before = len(p.lines)
        p.transmit(words[:16 * 5], sync={1: "idle", 2: "zero", 3: ("slip", rng.integers(0, 2, n).astype(np.uint8))}).silence()
        assert len(p.lines) - before == 5 and p.seen["sync word found %d bits behind the position of the loss" % n] == 1
    pagers.append(p)
    seen = _hold(ctx, oracle, pagers)
    for c in (0, 1, 2, 3):
        assert seen["sync word missed at count %d" % c] + seen["sync word missed at count %d, distance 4" % c] >= 5, (c, seen)
    assert lost_in_runs == 6 and seen["sync lost"] == 6 + 15 + 2 + 6 and seen["printed at sync loss"] == 6 + 3, seen
    assert sum(v for k, v in seen.items() if k.endswith("distance 4")) >= 6 and sum(v for k, v in seen.items() if k.endswith("distance 3")) == 10
    assert seen["sync word hit at count 3, distance 0"] >= 3, seen
