"""D-Star frames through the product, held to what the test sent.

Decoder-only engines (the CPU wave emulation and, with -m gpu, libdigiham_amd.so) are fed transmissions built from
synth.dstar_transmission / dstar_slow_blocks / dstar_header_bits and the frame builder below (`_Radio`, laid out as
synth.dstar_voice_frames lays its frames out, frame by frame so that single frames can be damaged).  Every output byte
and every event is held to `_Radio.expect`: SyncPhase, HeaderPhase and VoicePhase of dstar_phase.cpp:17-194 restated in a
few lines and fed with what the TEST put on the air -- the AMBE bits it drew, the slow-data bytes it sent, the sync
frames it damaged and by how many bits, the end pattern it sent and how.  What a damaged radio header decodes to is taken
from the reference's own Header::parseFromHeader compiled in place (tests/golden/frames_ref.npz, make_golden_frames.py);
the slow-data header copy needs the CRC rule of header.cpp:48-54 alone (synth.dstar_crc, held to the reference's
Crc::isCrcValid by test_dstar.py through dstar_ref.npz).  The oracle is no comparand here: once the engine has been held
to the expectation, the CPU leg holds oracle/decoders.c to the same expectation.

sym_index (include/digiham_amd.h): an event raised while a voice frame is processed carries the stream position of that
frame's first symbol; HEADER (radio header) and VOICE_START are raised between frames and carry the position of the
first symbol not yet consumed -- the first symbol of the first voice frame of the new voice phase.

Every case is laid out twice: in a plain row, where a single push takes it through the five-frame fast path of
dh_dstar_channel wherever that path applies, and in an `odd` row with the same content whose every voice frame has one
symbol with bit 1 set (the reference packs bit 0, dstar_phase.cpp:82), which sends every frame down the one-frame path.
Pushes of 97 symbols take the one-frame path throughout, pushes of 700 at an odd row pitch change paths at every push.
"""
import json
import os
from collections import Counter
from itertools import permutations

import numpy as np
import pytest

from common import npz_digest
from dec_harness import assert_rows, event_record, expected, frames_fixture, is_emu, run_symbols, stack_rows
from digiham_amd import api, synth

HERE = os.path.dirname(os.path.abspath(__file__))
EV_HEADER, EV_VOICE_START, EV_SYNC_VOICE, EV_MESSAGE, EV_SIMPLE, EV_FRAME_SYNC, EV_META_RESET = range(64, 71)
PN24 = synth.dstar_pn(24)
HEADER_SYNC = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0] + synth.DSTAR_FRAME_SYNC, np.uint8)        # dstar_phase.hpp:19-26: 9 bits of the bit sync + frame sync
VOICE_SYNC = np.array(synth.DSTAR_VOICE_SYNC, np.uint8)
TERM = np.array(synth.DSTAR_TERMINATOR, np.uint8)
FILL = b"\x66" * 6
PUSHES = ((None, None), (700, 703), (97, None))          # (symbols per push, row pitch): one push; a few hundred, odd pitch; a prime below one frame


@pytest.fixture(scope="module")
def fx():
    return frames_fixture()


def _dist(a, b):
    """hamming_distance(): symbols that differ"""
    return int((np.asarray(a) != np.asarray(b)).sum())


def _flipped(pattern, flips):
    b = np.array(pattern, np.uint8)
    b[list(flips)] ^= 1
    return b


def _bits_of_bytes(data):
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little")


# ------------------------------------------------------------------ the fixture itself
def test_fixture_conditions_and_reference(oracle, fx):
    """The committed radio headers are the ones the reference judged (digest taken at generation; oracle/_ref, where it is
    built, reproduces every column), accepted and rejected ones are both there, an accepted header is the header sent, and
    the oracle's restatement agrees with all of them."""
    path = os.path.join(HERE, "golden", "frames_ref.npz")
    assert npz_digest(path) == json.load(open(os.path.join(HERE, "golden", "ref_compare_hashes.json")))["frames_ref_npz"]
    assert os.path.getsize(path) < 300 * 1024
    ok, flips = fx["hdr_ok"] == 1, fx["hdr_flips"]
    assert fx["hdr_in"].shape[1] == 660 and set(np.unique(fx["hdr_in"])) == {0, 1}
    assert ok.sum() >= 8 and (~ok).sum() >= 8 and (ok & (flips >= 4)).sum() >= 8
    assert (fx["hdr_out"][ok] == fx["hdr_sent"][ok]).all() and (fx["hdr_out"][~ok] == 0).all()
    for raw, sent, n in zip(fx["hdr_in"], fx["hdr_sent"], flips):
        assert _dist(raw, synth.dstar_header_bits(bytes(sent))) == n and synth.dstar_crc(bytes(sent[:39])) == int(sent[39]) | int(sent[40]) << 8
    for which in ("oracle", "ref"):
        if which == "ref" and oracle.ref_lib("dstar") is None:
            continue
        o, data, _ = oracle.Elements(which).dstar_header(fx["hdr_in"])
        assert (o == fx["hdr_ok"]).all() and (data[ok] == fx["hdr_out"][ok]).all(), which


# ------------------------------------------------------------------ what the reference's phases make of what was sent
class _Radio:
    """One channel: the symbols on the air, item by item, and what the reference's three phases give for them."""

    def __init__(self, rng, lead=50, odd=False):
        self.rng, self.odd, self.items, self.n = rng, odd, [], 0
        self.prefix = None
        self.noise(lead)

    def _add(self, kind, bits, **kw):
        bits = np.asarray(bits, np.uint8)
        self.items.append(dict(kind=kind, at=self.n, bits=bits, **kw))
        self.n += len(bits)
        return self

    # ---- the sender
    def noise(self, n):
        return self._add("noise", self.rng.integers(0, 2, n).astype(np.uint8))

    def header(self, bits660, ok, data41, sync_at=None):
        """bit sync, frame sync and the 660 header bits as received; ok / data41: what Header::parseFromHeader makes of them.
        sync_at: the header is one the reference rejects and its bits sync_at .. sync_at + 23 hold the voice sync pattern; what
        is left of it behind that pattern is a whole number of frames to the voice phase that begins there"""
        bits = np.concatenate([np.array([1, 0] * 32 + synth.DSTAR_FRAME_SYNC, np.uint8), bits660])
        if sync_at is None:
            return self._add("header", bits, ok=bool(ok), data=bytes(data41), sync_at=None)
        cut = 79 + sync_at + 24
        assert not ok and (739 - cut) % 96 == 0 and _dist(bits[cut - 24:cut], VOICE_SYNC) == 0
        self._add("header", bits[:cut], ok=False, data=bytes(data41), sync_at=sync_at)
        for lo in range(cut, 739, 96):
            self.frame(bits[lo + 72:lo + 96], voice=bits[lo:lo + 72], plain=True)
        return self

    def clean_header(self, my="DL1ABC", data_flag=False):
        h = synth.dstar_header_bytes("DB0XYZ G", "DB0XYZ B", "CQCQCQ", my, "TEST", flags=(0x80 if data_flag else 0, 0, 0))
        return self.header(synth.dstar_header_bits(h), True, h)      # (what the encoder made, the decoder reads back: test_dstar.py)

    def frame(self, data24, voice=None, extra=None, end=None, note=None, plain=False):
        """72 AMBE bits + 24 data bits (+ `extra` bits that an end pattern takes with it); end: None, "full" or "half" -- the
        condition of dstar_phase.cpp:92 / :94 this frame is built to meet"""
        v = self.rng.integers(0, 2, 72).astype(np.uint8) if voice is None else np.asarray(voice, np.uint8)
        if self.prefix is not None:
            v[:24], self.prefix = self.prefix, None
        at = 24 + int(self.rng.integers(0, 48))                      # (drawn in plain rows too: both rows carry the same bits)
        sym = v.copy()
        if self.odd and not plain:
            sym[at] |= 2
        data24 = np.asarray(data24, np.uint8)
        bits = np.concatenate([sym, data24] + ([np.asarray(extra, np.uint8)] if extra is not None else []))
        half = bytes(np.packbits(data24 ^ PN24, bitorder="little"))                           # :117-125, from the sender's side
        return self._add("frame", bits, voice=np.packbits(v, bitorder="little"), sync_dist=_dist(data24, VOICE_SYNC), half=half, end=end, note=note)

    def sync_frame(self, flips=(), voice=None):
        return self.frame(_flipped(VOICE_SYNC, flips), voice=voice)

    def slow_frames(self, blocks, frames=20):
        """`frames` data frames carrying the 6-byte blocks, two frames to a block, filler blocks (0x66 ..) after them"""
        blocks = list(blocks) + [FILL] * (10 - len(blocks))
        assert len(blocks) == 10 and all(len(b) == 6 for b in blocks)
        for f in range(frames):
            half = blocks[f // 2][3 * (f % 2):3 * (f % 2) + 3]
            self.frame(_bits_of_bytes(half) ^ PN24)
            assert self.items[-1]["half"] == half
        return self

    def superframe(self, blocks=(), sync_flips=(), frames=20, sync_voice=None):
        return self.sync_frame(sync_flips, sync_voice).slow_frames(blocks, frames)

    def end(self, variant, extra=None):
        """the end pattern in the next data frame: "full1" all 48 bits with one wrong, "full2" with two wrong (no end: the
        transmission goes on, the second half being the first AMBE bits of the next frame), "half0" / "half1" its second half
        alone in the data frame with none / one wrong.  An end takes 24 more bits with it (:97)."""
        n = int(variant[-1])
        if variant.startswith("full"):
            t = _flipped(TERM, self.rng.choice(48, n, replace=False))
            if n == 2:
                self.frame(t[:24], note="all 48 bits with two wrong: no end")
                self.prefix = t[24:].copy()
                return self
            return self.frame(t[:24], extra=t[24:], end="full")
        t = _flipped(TERM[24:], self.rng.choice(24, n, replace=False))
        noise = self.rng.integers(0, 2, 24).astype(np.uint8)
        return self.frame(t, extra=noise if extra is None else extra, end="half")

    def adopt(self, bits, with_header, h41=None):
        """a transmission of synth.dstar_transmission, cut into its items by its layout"""
        lo = 0
        if with_header:
            self._add("header", bits[:739], ok=True, data=bytes(h41))
            lo = 739
        else:
            self._add("noise", bits[:24])                            # late entry: the stream begins with the data part of a sync frame
            self.items[-1]["kind"] = "frame_tail"
            lo = 24
        while len(bits) - lo > 120:
            self.frame(bits[lo + 72:lo + 96], voice=bits[lo:lo + 72])
            lo += 96
        assert len(bits) - lo == 120
        return self.frame(bits[lo + 72:lo + 96], voice=bits[lo:lo + 72], extra=bits[lo + 96:], end="full")

    def row(self):
        assert self.prefix is None
        return np.concatenate([it["bits"] for it in self.items])

    # ---- the receiver (dstar_phase.cpp)
    def expect(self):
        """-> output bytes, events; fills self.walks (the stretches SyncPhase searches and what it finds at their ends),
        self.voiced (the frames VoicePhase processes, with the end condition each was built to meet) and self.seen"""
        out, ev, seen = [], [], Counter()
        emit = lambda at, typ, a=0, b=0, payload=b"": ev.append(event_record(at, typ, a, b, payload))
        self.walks, self.voiced = [], []
        state, search_from, at = "search", 0, 0
        fc = sc = 0
        slow = None

        def enter(where, after_header):                              # the two constructors, :59-68, dstar_phase.hpp:70-75
            nonlocal state, at, fc, sc, slow
            state, at = "voice", where
            fc, sc = (21, 1) if after_header else (0, 0)
            slow = {"even": b"", "message": bytearray(20), "blocks": 0, "header": bytearray(41), "count": 0}
            emit(where, EV_VOICE_START, 0, int(after_header))

        for it in self.items:
            p, kind = it["at"], it["kind"]
            if state == "search":
                if kind == "header":                                 # :20-23, then HeaderPhase :36-57
                    self.walks.append((search_from, p + 55, "header"))
                    if not it["ok"]:
                        seen["radio header rejected"] += 1
                        search_from = p + 79 + 1                     # :41
                        if it["sync_at"] is not None:                # ... and the search walks into the header it has just rejected
                            self.walks.append((search_from, p + 79 + it["sync_at"], "voice"))
                            seen["late entry inside a rejected header"] += 1
                            enter(p + 79 + it["sync_at"] + 24, False)
                        continue
                    if it["data"][0] & 0x80:                         # isVoice (header.hpp:16, header.cpp:150)
                        seen["radio header with the data flag"] += 1
                        search_from = p + 79 + 660
                        continue
                    seen["radio header accepted"] += 1
                    emit(p + 739, EV_HEADER, 0, 0, it["data"][:24])
                    emit(p + 739, EV_HEADER, 1, 0, it["data"][24:])
                    enter(p + 739, True)
                elif kind == "frame_tail" or (kind == "frame" and it["sync_dist"] <= 1):          # :25-28
                    hit = p if kind == "frame_tail" else p + 72
                    self.walks.append((search_from, hit, "voice"))
                    seen["late entry"] += 1
                    enter(hit + 24, False)
                continue
            assert kind == "frame" and p == at, (kind, p, at)
            self.voiced.append((p, it["end"]))
            if it["note"]:
                seen[it["note"]] += 1
            if sc >= 1:                                              # :76-85
                out.append(it["voice"])
                seen["voice frame written"] += 1
            else:
                seen["voice frame muted"] += 1
            if it["end"] is not None:                                # :91-100
                seen["end pattern (%s) at frame count %d" % (it["end"], fc)] += 1
                emit(p, EV_META_RESET, 0, 0)
                state, search_from = "search", p + 120
                continue
            if fc >= 20:                                             # :101-115
                muted = sc < 1
                if it["sync_dist"] > 1:
                    seen["sync frame missed at count %d" % sc] += 1
                    sc -= 1
                    if sc < 0:
                        emit(p, EV_META_RESET, 0, 1)
                        state, search_from = "search", p + 96
                        continue
                else:
                    seen["sync frame at distance %d" % it["sync_dist"]] += 1
                    sc = min(sc + 1, 3)
                    if sc > 1:
                        emit(p, EV_SYNC_VOICE)
                if slow["blocks"] == 0x0F:                           # parseFrameData :196-210
                    emit(p, EV_MESSAGE, 0, 0, slow["message"])
                    seen["message" + (" collected while muted" if muted else "")] += 1
                if slow["count"] == 41:
                    h = slow["header"]
                    if synth.dstar_crc(h[:39]) == h[39] | h[40] << 8:                              # header.cpp:48-54
                        emit(p, EV_HEADER, 0, 1, h[:24])
                        emit(p, EV_HEADER, 1, 1, h[24:])
                        seen["slow-data header"] += 1
                    else:
                        seen["slow-data header with a wrong CRC"] += 1
                emit(p, EV_FRAME_SYNC)
                fc = 0                                               # resetFrames :140-146
                slow.update(message=bytearray(20), blocks=0, header=bytearray(41), count=0)
            else:                                                    # collectDataFrame :148-194
                if fc % 2 == 0:
                    slow["even"] = it["half"]
                else:
                    c = slow["even"] + it["half"]
                    kind4, n = c[0] >> 4, c[0] & 0x0F
                    if kind4 == 4:
                        if n <= 3:
                            slow["message"][5 * n:5 * n + 5] = c[1:6]
                            slow["blocks"] |= 1 << n
                        else:
                            seen["message block index above 3"] += 1
                    elif kind4 == 5:
                        if n > 5:
                            seen["header block with a length above 5"] += 1
                        elif slow["count"] + n > 41:
                            seen["header block past 41 bytes"] += 1
                        else:
                            slow["header"][slow["count"]:slow["count"] + n] = c[1:1 + n]
                            slow["count"] += n
                    elif kind4 == 3:
                        if n <= 5:                                   # :173-176: a length of 0 appends an empty string; the event says so
                            emit(p, EV_SIMPLE, 0, 0, c[1:1 + n])
                            seen["simple data of length %d" % n] += 1
                        else:
                            seen["simple data with a length above 5"] += 1
                    else:
                        seen["mini header 0x%Xn ignored" % kind4] += 1
                fc += 1
            at = p + 96
        assert state == "search", "the row has to end after an end pattern or a loss"
        self.walks.append((search_from, None, None))
        self.seen = seen
        return (np.concatenate(out) if out else np.zeros(0, np.uint8)), (np.concatenate(ev) if ev else np.zeros(0, api.EVENT_DTYPE))

    def check(self, row):
        """Nothing on the air looks like a sync or end pattern by accident: the search finds what the test sent and nothing
        before it (distances of dstar_phase.cpp:20, :25), and no frame of a voice phase meets :92 or :94 unless built to."""
        win = np.lib.stride_tricks.sliding_window_view(row, 24)
        dh, dv = (win != HEADER_SYNC).sum(axis=1), (win != VOICE_SYNC).sum(axis=1)
        for a, hit, kind in self.walks:
            stop = len(dh) if hit is None else hit
            bad = np.flatnonzero((dh[a:stop] <= 2) | (dv[a:stop] <= 1))
            assert len(bad) == 0, (a, hit, bad[:3] + a)
            assert hit is None or (dh[hit] <= 2 if kind == "header" else dh[hit] > 2 and dv[hit] <= 1), (hit, kind)
        for p, end in self.voiced:
            full, half = _dist(row[p + 72:p + 120], TERM), _dist(row[p + 72:p + 96], TERM[24:])
            assert (full <= 1, half <= 1) == (end == "full", end == "half"), (p, end, full, half)


def _hold(ctx, oracle, radios, pushes=PUSHES):
    """the engine, pushed three ways, gives exactly what was expected; then oracle/decoders.c does"""
    want = [r.expect() for r in radios]
    rows = stack_rows([np.concatenate([r.row(), np.zeros(130, np.uint8)]) for r in radios])
    assert rows.shape[0] <= 8 and rows.shape[1] <= 25000, rows.shape
    for r, row in zip(radios, rows):
        r.check(row)                                                 # before any decoder runs
    for size, pitch in pushes:
        run = run_symbols(ctx, "dstar", rows, size, pitch=max(size or rows.shape[1], 64) if pitch is None else pitch)
        assert_rows(run, want, "pushes of %s" % size)
    if is_emu(ctx):
        assert_rows(expected(oracle, "dstar", rows), want, "the oracle")
    seen = Counter()
    for r in radios:
        seen.update(r.seen)
    return seen, want


def _both(build, seeds):
    """every case as a plain row and as an `odd` row with the same bits"""
    radios = []
    for seed in seeds:
        for odd in (False, True):
            r = _Radio(np.random.default_rng(seed), lead=40 + seed % 23, odd=odd)
            build(r, seed)
            radios.append(r)
    for plain, odd in zip(radios[0::2], radios[1::2]):
        assert ((plain.row() ^ odd.row()) & 1).sum() == 0 and (odd.row() > 1).sum() > 0 and plain.row().max() == 1
    return radios


def _message_blocks(text):
    return synth.dstar_slow_blocks(text)


# ------------------------------------------------------------------ voice bytes
def test_voice_bytes_from_a_header_on_and_late_entry(ctx, oracle):
    """From a radio header on every frame's nine bytes are the 72 AMBE bits sent, LSB first -- sync frames and the frame
    that carries the end pattern included (dstar_phase.cpp:76-85 writes before :91 tests).  Entered at a voice sync
    (VoicePhase(0), :25-28, :59) nothing is written until the first due sync frame has been counted; that frame itself is not
    written (:76 sees a count of 0), but the superframe's slow data is collected and its message comes out there."""
    radios, sent = [], []
    for seed, with_header in ((701, True), (702, False)):
        for odd in (False, True):
            rng = np.random.default_rng(seed)
            bits, h, voice = synth.dstar_transmission(rng, my="VOICE%d" % (seed % 10), message="voice bytes %d" % seed, n_superframes=3,
                                                      with_header=with_header, inline_header=with_header)
            r = _Radio(np.random.default_rng(seed + 50), lead=45 + seed % 7, odd=odd)
            r.adopt(bits, with_header, h).noise(150)
            radios.append(r)
            sent.append(np.concatenate(voice))
    seen, want = _hold(ctx, oracle, radios)
    for k in (0, 1):                                                 # the sender's view: everything it sent, 3 x 21 + 2 frames
        assert len(sent[k]) == 9 * 65 and (want[k][0] == sent[k]).all()
    for k in (2, 3):                                                 # late entry: 20 frames heard and muted, the sync frame muted, the rest written
        assert len(sent[k]) == 9 * 64 and (want[k][0] == sent[k][9 * 21:]).all()
        ev = want[k][1]
        assert list(ev["type"][:3]) == [EV_VOICE_START, EV_MESSAGE, EV_FRAME_SYNC] and ev["b"][0] == 0
        assert ev["sym_index"][1] == ev["sym_index"][0] + 20 * 96 and bytes(ev["payload"][1][:20]).rstrip() == b"voice bytes 702"
    assert seen["late entry"] == 2 and seen["message collected while muted"] == 2 and seen["voice frame muted"] == 42 and seen["slow-data header"] == 2
    assert seen["end pattern (full) at frame count 0"] == 4


# ------------------------------------------------------------------ sync hysteresis
def _sync_counter(start, hits):
    """the count after each sync frame (True: found), None from the loss on -- dstar_phase.cpp:101-113 on its own"""
    count, trace = start, []
    for hit in hits:
        if count is None:
            trace.append(None)
        elif not hit:
            count -= 1
            count = None if count < 0 else count
            trace.append(count)
        else:
            count = min(count + 1, 3)
            trace.append(count)
    return trace


@pytest.mark.parametrize("start", [1, 2, 3])
def test_sync_frames_missed_in_a_row(ctx, oracle, start):
    """dstar_phase.cpp:101-113: k = 1..4 sync frames in a row replaced by patterns at distance 2 or more, the first of them
    met at a sync count of `start`.  Voice is written while the count is at least 1 (:76) and the slow data is collected
    throughout; SYNC_VOICE comes when a sync frame takes the count above 1 (:110); the miss that takes the count below zero
    resets with b = 1 and the search goes on behind that frame (:103-106), so the next clean sync frame is a late entry.  A
    sync frame with one wrong bit is a hit (:102)."""
    def build(r, seed):
        k = seed % 10
        r.clean_header(my="SYN%d%d" % (start, k))
        n_sf = (start - 1) + k + 3
        for sf in range(n_sf):
            missed = start - 1 <= sf < start - 1 + k
            flips = r.rng.choice(24, int(r.rng.integers(2, 6)), replace=False) if missed else [int(r.rng.integers(0, 24))] if sf == n_sf - 2 else []
            blocks = _message_blocks("sf %d of %d.%d" % (sf, start, k)) + synth.dstar_slow_blocks(None, None, b"simple %02d of %d.%d;" % (sf, start, k))
            planted = None
            if missed and sf - (start - 1) == start:                 # the miss that ends the voice phase: the search resumes BEHIND this frame
                planted = r.rng.integers(0, 2, 72).astype(np.uint8)  # (:86, :89 have advanced), so a sync pattern in its AMBE bits is not seen
                planted[10:34] = VOICE_SYNC
            r.superframe(blocks, sync_flips=flips, frames=20 if sf < n_sf - 1 else 6, sync_voice=planted)
        r.end("full1").noise(140)

    radios = _both(build, [10 * (start + 80) + k for k in (1, 2, 3, 4)])
    seen, want = _hold(ctx, oracle, radios)
    for i, k in enumerate((1, 2, 3, 4)):                             # the counter alone says which frames are heard and which events come
        n_sf = (start - 1) + k + 3
        hits = [not (start - 1 <= sf < start - 1 + k) for sf in range(n_sf)]
        trace = _sync_counter(1, hits)
        lost = None in trace
        assert lost == (k > start) and (start == 1 or trace[start - 2] == start)
        ev = want[2 * i][1]
        assert ((ev["type"] == EV_META_RESET) & (ev["b"] == 1)).sum() == int(lost)
        if not lost:
            frames = 0
            count = 1
            for sf, c in enumerate(trace):                           # frame 0 of superframe sf is written under the count before it, the rest under c
                n = 20 if sf < n_sf - 1 else 6
                frames += (count >= 1) + n * (c >= 1)
                count = c
            frames += count >= 1                                     # the frame with the end pattern
            assert len(want[2 * i][0]) == 9 * frames
            assert (ev["type"] == EV_SYNC_VOICE).sum() == sum(1 for c, hit in zip(trace, hits) if hit and c > 1) and (ev["type"] == EV_MESSAGE).sum() == n_sf - 1
    assert seen["sync frame missed at count %d" % start] == 8 and seen["sync frame at distance 1"] == 8, seen
    assert seen["message collected while muted"] >= 2 and seen["voice frame muted"] >= 40, seen
    assert seen["late entry"] == 2 * (4 - start), seen          # the rows with k > start lose the sync and come back


# ------------------------------------------------------------------ slow data
def test_slow_data_collection(ctx, oracle):
    """collectDataFrame / parseFrameData / resetFrames, dstar_phase.cpp:140-210."""
    orders = list(permutations(range(4)))
    h = synth.dstar_header_bytes("DB0SLO G", "DB0SLO B", "CQCQCQ", "DL9SLOW", "COPY")
    copy = synth.dstar_slow_blocks(None, h)
    assert [b[0] for b in copy] == [0x55] * 8 + [0x51]
    payload = bytes(range(0x41, 0x41 + 23))

    def build(r, seed):
        r.clean_header(my="SLOW%d" % (seed % 10))
        which = seed % 10
        if which < 3:                                                # the four message blocks in every order; beside them blocks that give nothing
            for i, order in enumerate(orders[8 * which:8 * which + 8]):
                m = _message_blocks("order %d%d%d%d of blocks" % order)
                quiet = [bytes([k << 4 | int(r.rng.integers(0, 16))]) + bytes(r.rng.integers(0, 256, 5).astype(np.uint8).tolist())
                         for k in ((0, 1, 2, 6, 7, 8), (9, 10, 11, 12, 13, 14), (15, 0, 6, 10, 13, 2))[i % 3]]
                blocks = [m[j] for j in order] + quiet
                r.superframe([blocks[j] for j in r.rng.permutation(10)] if i % 2 else blocks)
        else:
            m = _message_blocks("split over two frames")
            r.superframe(m[:3])                                      # three blocks here, the fourth in the next superframe: no message (:142-143)
            r.superframe(m[3:])
            r.superframe(m + [bytes([0x44 + i]) + b"WRONG" for i in (0, 1, 7, 11)])               # block indices above 3 are ignored (:158)
            r.superframe(m[:2] + [bytes([0x41]) + b"LATER"] + m[2:])                              # a block sent twice: the later text stays (:159)
            r.superframe(copy)                                       # the header copy, 8 x 5 + 1 bytes (:163-170, :200-206)
            bad = [bytes(b) for b in copy]
            bad[3] = bad[3][:2] + bytes([bad[3][2] ^ 0x20]) + bad[3][3:]
            r.superframe(bad)                                        # one wrong byte: CRC fails, no event
            r.superframe(copy[:8] + [bytes([0x55]) + b"EXTRA"] + copy[8:])                        # a block that would pass 41 bytes is dropped, the last byte still counts (:167)
            r.superframe(copy[:4] + [bytes([0x56]) + b"SIX__"] + copy[4:])                        # a length above 5 is dropped (:166)
            r.superframe(copy[:8])                                   # 40 bytes here, the last in the next superframe: no header (:144-145)
        r.superframe(copy[8:] + synth.dstar_slow_blocks(None, None, payload) + [bytes([0x30]) + b"EMPTY", bytes([0x36]) + b"SIX__", bytes([0x3F]) + b"FIFTN"], frames=20)
        r.superframe([], frames=4)
        r.end("half0").noise(130)

    radios = _both(build, [910, 911, 912, 913])
    seen, want = _hold(ctx, oracle, radios)
    for i in range(3):                                               # every order: the one text, once per superframe
        msgs = want[2 * i][1][want[2 * i][1]["type"] == EV_MESSAGE]
        assert [bytes(m["payload"][:20]) for m in msgs] == [("order %d%d%d%d of blocks" % o).encode().ljust(20) for o in orders[8 * i:8 * i + 8]]
    ev = want[6][1]
    msgs, t = [bytes(m["payload"][:20]) for m in ev[ev["type"] == EV_MESSAGE]], b"split over two frames"[:20]
    assert msgs == [t, t[:5] + b"LATER" + t[10:]], msgs
    heads = ev[(ev["type"] == EV_HEADER) & (ev["b"] == 1)]
    assert len(heads) == 2 * 3 and all(bytes(a["payload"][:24]) + bytes(b["payload"][:17]) == h for a, b in zip(heads[0::2], heads[1::2]))
    for w in want:                                                   # simple data: the bytes sent, in order, with the lengths sent; length 0 is an empty event
        simple = w[1][w[1]["type"] == EV_SIMPLE]
        assert b"".join(bytes(e["payload"][:e["len"]]) for e in simple) == payload and list(simple["len"]) == [5, 5, 5, 5, 3, 0]
    for k in ("message block index above 3", "header block with a length above 5", "header block past 41 bytes", "slow-data header with a wrong CRC",
              "simple data of length 0", "simple data with a length above 5", "slow-data header", "message") + tuple("mini header 0x%Xn ignored" % k for k in (0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)):
        assert seen[k] >= 2, (k, seen)


# ------------------------------------------------------------------ end pattern
def test_end_pattern_variants(ctx, oracle):
    """dstar_phase.cpp:91-100: all 48 bits with one wrong bit, the second half alone in the data frame with none or one wrong
    -- an end: the frame's voice is written first (:76-85), META_RESET b = 0, 120 symbols consumed (:89, :97), and the search
    finds the next transmission's header -- the 24 bits behind the frame are gone even when they are a voice sync pattern.
    All 48 bits with two wrong is no end.  Each in the third and in the last frame of a five-frame batch (frame counts 7 and
    19, the latter the frame before a sync frame) and in a sync frame's place."""
    def build(r, seed):
        for variant in (("full1", "half0"), ("full2", "half1"))[seed % 2]:
            for n_before in (7, 19, 20):
                r.clean_header(my="END%d" % n_before)
                r.sync_frame().slow_frames(_message_blocks("end %s at %d" % (variant, n_before)), frames=n_before)
                r.end(variant, extra=VOICE_SYNC if n_before == 19 else None)       # (a sync pattern in the 24 bits that go with the end is not seen)
                if variant == "full2":                               # no end: the transmission goes on, and is ended for good
                    if n_before == 19:
                        r.sync_frame()
                    r.slow_frames([], frames=3).end("half1")
                r.noise(int(r.rng.integers(60, 200)))

    radios = _both(build, [920, 921])
    seen, want = _hold(ctx, oracle, radios)
    assert sum(v for k, v in seen.items() if k.startswith("end pattern")) == 4 * 6 and seen["radio header accepted"] == 4 * 6
    assert seen["all 48 bits with two wrong: no end"] == 2 * 3
    for k in ("end pattern (full) at frame count 7", "end pattern (half) at frame count 7", "end pattern (full) at frame count 19",
              "end pattern (half) at frame count 19", "end pattern (full) at frame count 20", "end pattern (half) at frame count 20"):
        assert seen[k] >= 2, (k, seen)
    for out, ev in want[0:2]:                                        # the sender's view: header, sync frame, n frames and the frame with the end, all heard
        assert len(out) == 9 * sum(2 * (1 + n + 1) for n in (7, 19, 20))
        resets = ev[ev["type"] == EV_META_RESET]
        assert len(resets) == 6 and (resets["b"] == 0).all()


# ------------------------------------------------------------------ radio headers
def test_radio_headers_with_bit_errors(ctx, oracle, fx):
    """dstar_phase.cpp:36-57 with the fixture's damaged headers: where the reference's parseFromHeader accepts, the two HEADER
    events carry ITS 41 bytes and the voice follows from the first frame; where it rejects, the search goes on one bit
    further (:41) and enters late at the first voice sync -- inside the rejected header's own bits, where they hold one; a
    header with the data flag gives nothing (:47, :55-56)."""
    ok, flips = fx["hdr_ok"] == 1, fx["hdr_flips"]
    accepted = [i for i in np.flatnonzero(ok) if flips[i] >= 3]
    rejected = list(np.flatnonzero(~ok & (fx["hdr_burst"] != 2)))
    planted = list(np.flatnonzero(~ok & (fx["hdr_burst"] == 2)))
    assert len(planted) >= 4

    def build(r, seed):
        k = seed % 10
        for i in accepted[k::4][:3] + rejected[k::4][:2]:
            r.header(fx["hdr_in"][i], fx["hdr_ok"][i], fx["hdr_out"][i])
            r.superframe(_message_blocks("header vector %d" % i))
            r.superframe([], frames=3)
            r.end("full1").noise(int(r.rng.integers(60, 200)))
        i = planted[k]                                               # rejected, with a voice sync pattern in its bits 60..83: entered there
        r.header(fx["hdr_in"][i], fx["hdr_ok"][i], fx["hdr_out"][i], sync_at=60).slow_frames(_message_blocks("behind a planted sync"), frames=14)
        r.superframe([], frames=3).end("half1").noise(int(r.rng.integers(60, 200)))
        r.clean_header(my="DATA%d" % k, data_flag=True).noise(400)   # no voice frames behind it: nothing to enter late at
        r.clean_header(my="LAST%d" % k).superframe([], frames=2).end("half0").noise(130)

    radios = _both(build, [930, 931, 932, 933])
    seen, want = _hold(ctx, oracle, radios)
    assert seen["radio header accepted"] == 8 * 4 and seen["radio header rejected"] == 8 * 3 and seen["late entry inside a rejected header"] == 8 and seen["radio header with the data flag"] == 8
    assert seen["late entry"] == 8 * 2 and seen["message collected while muted"] == 8 * 3
    for k, (out, ev) in enumerate(want[0::2]):
        heads = ev[(ev["type"] == EV_HEADER) & (ev["b"] == 0)]
        got = [bytes(a["payload"][:24]) + bytes(b["payload"][:17]) for a, b in zip(heads[0::2], heads[1::2])]
        assert got[:3] == [bytes(fx["hdr_sent"][i]) for i in accepted[k::4][:3]]
        assert len(out) == 9 * (3 * 26 + 3 * 4 + 4)                 # 21 + 1 + 3 + 1 frames behind an accepted header, 3 + 1 behind a rejected one
