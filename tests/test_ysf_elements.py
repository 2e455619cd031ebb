"""YSF frame elements through the product, against the REFERENCE's own results.

tests/golden/ysf_elements_ref.npz (make_golden_ysf_elements.py) holds V/D2 data-channel (DCH) codewords, header CSD
codewords and FICH codewords -- clean, one wrong dibit at every position, pairs of wrong dibits, k flipped bits, random
dibits -- each with what the reference's decode_trellis / crc16_checksum / decode_whitening (oracle/_ref/
libdigiham_ref_fec.so) and Fich::parse (libdigiham_ref_ysf.so) made of it; elements_ref.npz holds FICHs of every frame
and data type.  Decoder-only engines (the CPU wave emulation and, with -m gpu, libdigiham_amd.so) are fed frames that
carry these vectors, and every event and output byte is held to the frame machine of ysf_phase.cpp:45-172 restated
below (`_Channel`) and fed with the REFERENCE's element results.  The V/D2 voice block has no csdr-free reference
function: its expected bytes come from the encoder side alone (the 49 AMBE bits given to synth.ysf_v2_voice_dibits and
the wrong bits the test injected).  The oracle is the comparand only in the two mixed-stream tests and the full-chain
case at the end.

The tests aim at dh_ysf_decode_ahead (decoder_core.hpp): the chunk's bit planes at every alignment, the 5 x 20
de-interleave, the clean / single-dibit shortcut, the dirty codewords packed four to a Viterbi pass and scattered back to
their frames, chunks of every size, and the state carried over a push boundary.
"""
import json
import os

import numpy as np
import pytest

from common import assert_matches_oracle, npz_digest, run_engine
from dec_harness import assert_rows, first_differing_frame, run_symbols, tier
from digiham_amd import api, synth

HERE = os.path.dirname(os.path.abspath(__file__))
EV_FICH, EV_MODE, EV_DCH, EV_HEADER_DCH, EV_META_RESET = 16, 17, 18, 19, 20
LEAD = 29
SYNC = np.array(synth.YSF_SYNC, np.uint8)
SYNC_BITS = np.unpackbits(SYNC[:, None], axis=1)[:, 6:].reshape(-1)
_I = np.arange(100)
AT_FICH = 20 + (_I % 5) * 20 + _I // 5                          # codeword dibit i of the FICH in the frame (fich.cpp:16-19)
AT_DCH = 120 + (_I % 5) * 72 + _I // 5                          # ... of the V/D2 DCH (ysf_phase.cpp:103-106)
_SP = (np.arange(180) % 9) * 20 + np.arange(180) // 9
AT_CSD = [120 + h * 36 + (_SP // 36) * 72 + _SP % 36 for h in (0, 1)]      # ... of CSD1 / CSD2 of a header (:323-333)
V2_MAP = np.array(synth._V2_MAP)
V2_PN = np.array(synth.pn9_bits(104), np.uint8)
V2_AIR = (np.arange(104) * 4) % 104 + (np.arange(104) * 4) // 104     # where bit k of the whitened block goes on the air


@pytest.fixture(scope="module")
def yse():
    with np.load(os.path.join(HERE, "golden", "ysf_elements_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "elements_ref.npz")) as z:
        return {k: z[k] for k in ("fich_in", "fich_out", "fich_data")}


# ------------------------------------------------------------------ the fixture itself
def _pack_dibits(d):
    d = np.asarray(d, np.uint8)
    return np.packbits(np.stack([d >> 1, d & 1], axis=-1).reshape(len(d), -1), axis=1)


def _hard_single(v, name):
    """the singles the reference's decoder does not repair: both bits of dibit n - 5 wrong (rejected for every codeword),
    both bits of dibit 4 or 5 wrong (rejected for about half of them) -- make_golden_ysf_elements.py, hard_single"""
    n = v[name + "_in"].shape[1]
    return (v[name + "_pat"] == 3) & np.isin(v[name + "_pos"], (4, 5, n - 5))


def test_fixture_conditions_and_reference(oracle, yse):
    """The committed vectors are the ones the reference produced (digest taken at generation; oracle/_ref, where it is
    built, reproduces every expected column), every class the product tests rely on is populated on both sides of the
    CRC, and the oracle's restatement agrees with all of them.

    One condition is stated as the reference behaves, not as first assumed: its decoder does NOT repair every single
    wrong dibit.  With both bits of dibit n - 5 wrong it rejects every codeword tried (40 of 40, both lengths), with both
    bits of dibit 4 or 5 wrong about half (18 and 16 of 40 at 100 dibits) -- trellis.c starts every state at metric 0 and
    takes the best end state.  Every other single is accepted with the payload sent; the fixture keeps all of them, and
    the product has to reject where the reference rejects."""
    path = os.path.join(HERE, "golden", "ysf_elements_ref.npz")
    assert npz_digest(path) == json.load(open(os.path.join(HERE, "golden", "ref_compare_hashes.json")))["ysf_elements_ref_npz"]
    assert os.path.getsize(path) < 300 * 1024
    for name, n, nbytes, n_single in (("dch", 100, 10, 300), ("csd", 180, 20, 3 * 71)):
        ok, src = yse[name + "_ok"] == 1, yse[name + "_src"]
        same = (yse[name + "_out"] == yse[name + "_sent"]).all(axis=1)
        assert yse[name + "_in"].shape[1] == n and yse[name + "_out"].shape[1] == nbytes
        assert (ok & (src >= 2)).sum() >= 100 and (~ok & (src >= 2)).sum() >= 100, name
        assert sorted(set(src)) == [0, 1, 2, 3, 4] and (src == 1).sum() == n_single, name
        assert (ok & same)[(src <= 1) & ~_hard_single(yse, name)].all(), name
        assert not ok[(yse[name + "_pos"] == n - 5) & (yse[name + "_pat"] == 3)].any(), name
        print("%s: accepted with another payload than sent: %d" % (name, (ok & ~same & (src < 4)).sum()))
        assert not ok[src == 4].any()
    assert sorted(set(zip(yse["dch_pos"][yse["dch_src"] == 1].tolist(), yse["dch_pat"][yse["dch_src"] == 1].tolist()))) == \
        [(p, w) for p in range(100) for w in (1, 2, 3)]
    fsrc = yse["fichx_src"]
    assert sorted(set(fsrc)) == [0, 1, 2] and (fsrc == 1).sum() == 300
    assert ((yse["fichx_ok"] == 1) & (yse["fichx_data"] == yse["fichx_sent"]))[fsrc <= 1].all()
    assert len(set(yse["fichx_sent"][fsrc == 0].tolist())) == 48 and len({bytes(r) for r in yse["dch_sent"][yse["dch_src"] == 0]}) == 32
    for which in ("oracle", "ref"):
        if which == "ref" and (oracle.ref() is None or oracle.ref_lib("ysf") is None):
            continue
        for name, n, nbytes in (("dch", 100, 10), ("csd", 180, 20)):
            w, metric = oracle.trellis(_pack_dibits(yse[name + "_in"]), n, which)                      # ysf_phase.cpp:260 / :336
            ok = oracle.crc16(w, nbytes, which) == (w[:, nbytes].astype(np.uint16) << 8 | w[:, nbytes + 1])    # :262-263 / :338-339
            out = oracle.whitening(w, 100 if n == 100 else 160, which)[:, :nbytes]                     # :267 / :346
            assert (ok == (yse[name + "_ok"] == 1)).all() and (metric == yse[name + "_metric"]).all(), (which, name)
            assert (out[ok] == yse[name + "_out"][ok]).all(), (which, name)
        air = np.zeros((len(yse["fichx_in"]), 100), np.uint8)
        air[:, AT_FICH - 20] = yse["fichx_in"]
        o, data = oracle.Elements(which).ysf_fich(air)
        assert (o[:, 0] == yse["fichx_ok"]).all() and (data == yse["fichx_data"]).all(), which


# ------------------------------------------------------------------ frames, and what the reference's frame machine makes of them
def _v2_block(ambe49, wrong=()):
    """52 dibits of a V/D2 voice block that carries `ambe49`, with the bits `wrong` (indices into the 104 bits before
    whitening and interleave: 27 triplets, 22 unprotected bits, one pad bit) inverted on the air; and the 7 bytes
    decodeV2VoicePayload has to give -- from the encoder side: a triplet with one wrong bit still reads as sent, with two or
    three it flips; a wrong unprotected bit flips that bit; the pad bit is not looked at (ysf_phase.cpp:180-256)"""
    voice = np.array(ambe49, np.uint8)[V2_MAP]                     # the order on the air: voice bit i = AMBE bit V2_MAP[i]
    air = np.zeros(104, np.uint8)                                  # synth.ysf_v2_voice_dibits, on arrays (compared with it below)
    air[V2_AIR] = np.concatenate([np.repeat(voice[:27], 3), voice[27:], [0]]) ^ V2_PN
    wrong = list(wrong)
    for k in wrong:
        air[V2_AIR[k]] ^= 1
    for t in range(27):
        if sum(1 for k in wrong if k // 3 == t and k < 81) >= 2:
            voice[t] ^= 1
    for k in wrong:
        if 81 <= k < 103:
            voice[27 + k - 81] ^= 1
    ambe = np.zeros(56, np.uint8)
    ambe[V2_MAP] = voice
    return (air[0::2] << 1 | air[1::2]).astype(np.uint8), np.packbits(ambe)


def _sync(wrong_bits=()):
    b = SYNC_BITS.copy()
    b[list(wrong_bits)] ^= 1
    return (b[0::2] << 1 | b[1::2]).astype(np.uint8)


def _is_sync(d20):
    return int((np.unpackbits(np.asarray(d20, np.uint8)[:, None], axis=1)[:, 6:].reshape(-1) ^ SYNC_BITS).sum()) <= 3


class _Channel:
    """One channel's frames and the events / output bytes FramePhase::process (ysf_phase.cpp:45-172) gives for them when
    Fich::parse, decodeV2DataChannel's CRC and decodeHeaderDataChannel return what the REFERENCE returned for the vectors
    each frame carries.  SyncPhase (:25-34) is restated too: after the sync count falls below zero the search walks on dibit
    by dibit and locks at the next frame whose sync word has at most three wrong bits (`stream` asserts that nothing in
    between looks like one)."""

    def __init__(self, lead=LEAD):
        self.lead, self.rows, self.ev, self.out = lead, [], [], []
        self.locked, self.count, self.fich, self.expect_sub = False, 0, None, False
        self.searched = []                                          # frames the sync search walks through

    def _emit(self, pos, typ, a, b, payload):
        e = np.zeros(1, api.EVENT_DTYPE)
        e["sym_index"], e["type"], e["a"], e["b"], e["len"] = pos, typ, a, b, len(payload)
        e["payload"][0, :len(payload)] = np.frombuffer(bytes(payload), np.uint8)
        self.ev.append(e)

    def frame(self, fich, payload, dch=None, csd=None, v2=None, sync_wrong=()):
        """fich = (100 dibits as on the air, Fich::parse succeeded, its 32-bit word); payload = 360 dibits; dch = (CRC ok, 10
        bytes) of a V/D2 frame; csd = two (CRC ok, 20 bytes) of a header; v2 = the five 7-byte voice blocks of a V/D2 frame
        (from the encoder side); sync_wrong = bits of the sync word that are inverted"""
        pos = self.lead + 480 * len(self.rows)
        sync_ok = len(sync_wrong) <= 3
        self.rows.append(np.concatenate([_sync(sync_wrong), fich[0], payload]).astype(np.uint8))
        assert len(self.rows[-1]) == 480
        if not self.locked:
            if not sync_ok:
                self.searched.append(len(self.rows) - 1)
                return
            self.locked, self.count, self.fich, self.expect_sub = True, 0, None, False      # new FramePhase()
        if sync_ok:
            self.count = min(self.count + 1, 12)
        else:
            self.count -= 1
            if self.count < 0:
                self._emit(pos, EV_META_RESET, 0, 0, [])
                self.locked = False
                self.searched.append(len(self.rows) - 1)
                return
        fresh = bool(fich[1])
        if fresh:
            self.fich = int(fich[2])
            self._emit(pos, EV_FICH, 0, 0, self.fich.to_bytes(4, "big"))
        if self.fich is None:
            return
        ft, dt = (self.fich >> 30) & 3, (self.fich >> 8) & 3
        p = np.asarray(payload, np.uint8)
        if ft == 1:
            self._emit(pos, EV_MODE, 0, dt, [])
            if dt == 0:                                             # V/D1: `=` at ysf_phase.cpp:176 keeps dibit 4 j + 3 of every byte, unshifted
                for i in range(5):
                    self.out.append(np.concatenate([[dt], p[36 + 72 * i + 3:36 + 72 * i + 36:4]]).astype(np.uint8))
            elif dt == 2:
                for i in range(5):
                    self.out.append(np.concatenate([[dt], v2[i]]).astype(np.uint8))
                if fresh and dch[0]:
                    self._emit(pos, EV_DCH, (self.fich >> 19) & 7, 0, np.asarray(dch[1], np.uint8))
            elif dt == 3:
                start = 3 if self.expect_sub else 0
                self.expect_sub = False
                for i in range(start, 5):
                    d = p[72 * i:72 * i + 72].reshape(18, 4)
                    self.out.append(np.concatenate([[dt], d[:, 0] << 6 | d[:, 1] << 4 | d[:, 2] << 2 | d[:, 3]]).astype(np.uint8))
        elif ft == 0:
            self._emit(pos, EV_META_RESET, 0, 1, [])
            for half in (0, 1):
                if csd[half][0]:
                    self._emit(pos, EV_HEADER_DCH, half, 0, np.asarray(csd[half][1], np.uint8))
            self.expect_sub = True
        elif ft == 2:
            self._emit(pos, EV_META_RESET, 0, 2, [])

    def stream(self, lead):
        s = np.concatenate([lead[:self.lead]] + self.rows + [np.zeros(200, np.uint8)])       # (the last frame needs one more dibit in hand)
        walked = list(range(self.lead)) + [self.lead + 480 * k + j for k in self.searched for j in range(1 if k > 0 and k - 1 not in self.searched else 0, 480)]
        for k in walked:                                             # the sync search must lock at the frames, nowhere else
            assert not _is_sync(s[k:k + 20]), k
        return s

    def events(self):
        return np.concatenate(self.ev) if self.ev else np.zeros(0, api.EVENT_DTYPE)

    def bytes(self):
        return np.concatenate(self.out) if self.out else np.zeros(0, np.uint8)


def _run(ctx, streams, chunk=None, pitch=None, aligned=False):
    """streams (one row of dibits per channel) through a decoder-only engine in pushes of `chunk` symbols; pitch = row pitch
    of the pushed buffer; aligned: the buffer's first row starts at a multiple of 16 bytes (host memory only)"""
    if pitch is None:
        pitch = max(chunk or max(len(s) for s in streams), 64)
    return run_symbols(ctx, "ysf", streams, chunk, pitch=pitch, aligned=aligned)


def _check(ctx, chans, chunk, pitch=None, aligned=False):
    """push the channels' streams and hold events and output bytes to the model; returns all expected events"""
    lead = np.random.default_rng(5).integers(0, 4, 64).astype(np.uint8)
    run = _run(ctx, [c.stream(lead) for c in chans], chunk, pitch, aligned)
    what = ["push %s frame %s" % (chunk, first_differing_frame(got, c.events(), c.lead, 480)) for got, c in zip(run.events, chans)]
    assert_rows(run, [(c.bytes(), c.events()) for c in chans], what)
    return np.concatenate([c.events() for c in chans])


def _chunk_sizes(n_stream, lead, push):
    """how many frames each decode-ahead of a channel takes: min((avail - 1) / 480, 16) whenever the frames decoded ahead
    are used up (dh_ysf_channel) -- only used to assert that a push size reaches the chunk size it is there for"""
    sizes, pos, ahead = [], lead, 0
    for lo in range(0, n_stream, push):
        have, ahead = min(lo + push, n_stream), 0
        while have - pos > 480:
            if ahead == 0:
                ahead = min((have - pos - 1) // 480, 16)
                sizes.append(ahead)
            pos += 480; ahead -= 1
    return sizes


class _Parts:
    """frame parts drawn from the fixtures, each with the reference's result"""

    def __init__(self, yse, gold, seed):
        self.v, self.g, self.rng = yse, gold, np.random.default_rng(seed)
        self.clean_fich = np.nonzero(yse["fichx_src"] == 0)[0]
        ok = gold["fich_out"][:, 0] == 1
        self.by_type = {(ft, dt): np.nonzero(ok & (gold["fich_out"][:, 1] == ft) & (gold["fich_out"][:, 2] == dt))[0] for ft in range(4) for dt in range(4)}
        self.broken = np.nonzero(~ok)[0]

    def fichx(self, i):
        """vector i of ysf_elements_ref.npz (codeword order) as on the air"""
        air = np.zeros(100, np.uint8)
        air[AT_FICH - 20] = self.v["fichx_in"][i]
        return air, bool(self.v["fichx_ok"][i]), int(self.v["fichx_data"][i])

    def v2_fich(self, fn, k=0):
        """a clean V/D2 communication FICH with that frame number"""
        c = self.clean_fich[(self.v["fichx_sent"][self.clean_fich] >> 19) & 7 == fn]
        return self.fichx(c[k % len(c)])

    def fich(self, ft, dt, k=0):
        """a FICH of elements_ref.npz that the reference parses as (frame type, data type)"""
        i = self.by_type[(ft, dt)][k % len(self.by_type[(ft, dt)])]
        return self.g["fich_in"][i], True, int(self.g["fich_data"][i])

    def broken_fich(self, k=0):
        i = self.broken[k % len(self.broken)]
        return self.g["fich_in"][i], False, 0

    def random_payload(self):
        return self.rng.integers(0, 4, 360).astype(np.uint8)

    def v2_payload(self, i, blocks=None):
        """a V/D2 payload with DCH vector i and five voice blocks (random AMBE bits, or the given (dibits, bytes))"""
        p = self.random_payload()
        p[AT_DCH - 120] = self.v["dch_in"][i]
        blocks = blocks or [_v2_block(self.rng.integers(0, 2, 49)) for _ in range(5)]
        for b in range(5):
            p[72 * b + 20:72 * b + 72] = blocks[b][0]
        return p, (bool(self.v["dch_ok"][i]), self.v["dch_out"][i]), [blk[1] for blk in blocks]

    def header_payload(self, i, j):
        p = self.random_payload()
        p[AT_CSD[0] - 120], p[AT_CSD[1] - 120] = self.v["csd_in"][i], self.v["csd_in"][j]
        return p, [(bool(self.v["csd_ok"][k]), self.v["csd_out"][k]) for k in (i, j)]

    def v2_frame(self, c, fich, i, blocks=None, sync_wrong=()):
        p, dch, v2 = self.v2_payload(i, blocks)
        c.frame(fich, p, dch=dch, v2=v2, sync_wrong=sync_wrong)


# ------------------------------------------------------------------ DCH
PUSHES = [None, 481, 961, 1441, 2401, 7681, 8161, 37]
WANT_CHUNKS = {481: {1}, 961: {2}, 1441: {3}, 2401: {5}, 7681: {16}, 8161: {16, 1}}


def _dch_channels(yse, gold, idx, B):
    P = _Parts(yse, gold, 31)
    chans = []
    for b, part in enumerate(np.array_split(idx, B)):
        c = _Channel()
        for k, i in enumerate(part):
            P.v2_frame(c, P.v2_fich(k & 7, b + k // 8), i)
        chans.append(c)
    return chans


@pytest.mark.parametrize("chunk", PUSHES)
def test_dch_events_vs_reference(ctx, yse, gold, chunk):
    """Every DCH vector (a fixed third of them on the emulation, every class) in V/D2 frames with a clean FICH, frame number
    cycling 0..7: a DCH event exactly where the reference's CRC passed, with the frame number and the reference's ten
    de-whitened bytes; FICH and MODE events and the 40 voice bytes of every frame.  The push sizes make the decode-ahead take
    1, 2, 3, 5, 16 and 16 + 1 frames; 37 symbols a push leaves every frame to a push of its own with most of it carried."""
    n = len(yse["dch_in"])
    idx = np.arange(n) if tier(ctx, True, False) else np.arange(2, n, 3)
    assert sorted(set(yse["dch_src"][idx])) == [0, 1, 2, 3, 4]
    chans = _dch_channels(yse, gold, idx, tier(ctx, 16, 3))
    if chunk in WANT_CHUNKS:
        sizes = set(_chunk_sizes(len(chans[0].rows) * 480 + LEAD + 200, LEAD, chunk))
        assert WANT_CHUNKS[chunk] <= sizes, sizes
    exp = _check(ctx, chans, chunk)
    n_ok = int(yse["dch_ok"][idx].sum())
    assert (exp["type"] == EV_DCH).sum() == n_ok and 0 < n_ok < len(idx)
    assert (exp["type"] == EV_FICH).sum() == len(idx) == (exp["type"] == EV_MODE).sum()
    assert set(exp["a"][exp["type"] == EV_DCH]) == set(range(8))


# ------------------------------------------------------------------ dirty codewords in every lane pattern
def _masks():
    """bit f: the FICH of frame f of the chunk is dirty (lane f), bit 16 + f: its DCH (lane 16 + f)"""
    rng = np.random.default_rng(32)
    m = {"none": 0, "fichs": 0xFFFF, "dchs": 0xFFFF0000, "lane 0": 1, "lane 31": 1 << 31, "lanes 0 and 31": 1 | 1 << 31,
         "lanes 15 and 16": 3 << 15, "even lanes": 0x55555555, "odd lanes": 0xAAAAAAAA, "all but lane 7": 0xFFFFFFFF ^ 1 << 7, "all": 0xFFFFFFFF}
    for count in (1, 2, 3, 4, 5, 7, 8, 9, 16):
        m["%d dirty" % count] = sum(1 << int(l) for l in rng.choice(32, count, replace=False))
    return m


def test_dirty_codewords_in_every_lane_pattern(ctx, yse, gold):
    """One channel per dirty mask over the 32 codewords of a 16-frame chunk (then five clean frames): a codeword is dirty
    when it carries a pair of wrong dibits (its syndrome is no single's, so it goes to the Viterbi decoder), clean
    otherwise.  0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 31 and 32 dirty codewords fill whole and partial passes of four; every frame
    of the chunk has its own FICH word and DCH payload, so a result scattered to another frame shows.  The last channel's
    DCH is dirty in 20 consecutive frames with intact sync words: no META_RESET, i.e. the sync bit that shares a word with
    the DCH's last byte survives the scatter-back."""
    P = _Parts(yse, gold, 33)
    v = yse

    def vectors(name, sent_col):
        clean = np.nonzero(v[name + "_src"] == 0)[0]
        dirty = {}
        for i in np.nonzero((v[name + "_src"] == 2) & (v[name + "_ok"] == 1))[0]:
            dirty.setdefault(bytes(np.atleast_1d(v[sent_col][i])), []).append(i)
        both = [(c, dirty[bytes(np.atleast_1d(v[sent_col][c]))]) for c in clean if bytes(np.atleast_1d(v[sent_col][c])) in dirty]
        return both
    fv, dv = vectors("fichx", "fichx_sent"), vectors("dch", "dch_sent")
    assert len(fv) >= 16 and len(dv) >= 21
    masks = _masks()
    assert {bin(m).count("1") for m in masks.values()} >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 32}
    chans = []
    for j, (name, m) in enumerate(list(masks.items()) + [("20 dirty DCHs in a row", None)]):
        c = _Channel()
        for f in range(21):
            fd = m is not None and f < 16 and (m >> f) & 1
            dd = f < 20 if m is None else f < 16 and (m >> (16 + f)) & 1
            fc, fdirty = fv[(f + j) % 16 if f < 16 else f % 16]
            dc, ddirty = dv[(f + 3 * j) % 21]
            P.v2_frame(c, P.fichx(fdirty[j % len(fdirty)] if fd else fc), ddirty[j % len(ddirty)] if dd else dc)
        chans.append(c)
    for chunk in (None, 7681):
        exp = _check(ctx, chans, chunk)
        assert not (exp["type"] == EV_META_RESET).any()
        assert (exp["type"] == EV_DCH).sum() == 21 * len(chans) == (exp["type"] == EV_FICH).sum()


# ------------------------------------------------------------------ one wrong dibit, every position, every alignment of the planes
def test_single_dibit_at_every_position_and_alignment(ctx, yse, gold):
    """The 300 singles (every position x wrong bit 1 / bit 0 / both; on the emulation positions 0, 13..18, 86..92, 95 and 99) as
    the FICH and as the DCH of consecutive frames, in channels whose first frame starts 0..15 dibits into the row of a symbol
    buffer with an odd row pitch: the chunk's bit planes start `off0` = 0..15 dibits before the first frame (all 16 on the GPU;
    0, 1, 7 and 15 on the emulation).  Inside positions 16..88 the product repairs the dibit lane-locally, outside it runs
    its Viterbi decoder; either way the events are the reference's -- including the DCH it REJECTS (both bits of dibit 95)."""
    P = _Parts(yse, gold, 34)
    fs, ds = np.nonzero(yse["fichx_src"] == 1)[0], np.nonzero(yse["dch_src"] == 1)[0]
    assert (yse["fichx_pos"][fs] == yse["dch_pos"][ds]).all() and (yse["fichx_pat"][fs] == yse["dch_pat"][ds]).all()
    keep = np.ones(300, bool) if tier(ctx, True, False) else np.isin(yse["dch_pos"][ds], [0, 13, 14, 15, 16, 17, 18, 86, 87, 88, 89, 90, 91, 92, 95, 99])
    pitch = 300 * 480 + 301
    assert pitch % 2 == 1
    wants = tier(ctx, list(range(16)), [0, 1, 7, 15])
    # row b starts b * pitch bytes behind a multiple of 16: a lead-in of (want - b * pitch) & 15 dibits puts the first frame `want`
    # dibits behind one.  (With an odd pitch no 16 rows have both every lead-in and every alignment, so on the GPU 16 more rows
    # take the lead-ins 0..15 in order.)
    leads = [(want - b * pitch) & 15 for b, want in enumerate(wants)] + tier(ctx, list(range(16)), [])
    chans = []
    for lead in leads:
        c = _Channel(lead)
        for f, d in zip(fs[keep], ds[keep]):
            P.v2_frame(c, P.fichx(f), d)
        chans.append(c)
    assert {(lead + b * pitch) & 15 for b, lead in enumerate(leads)} >= set(wants) and set(leads) >= set(tier(ctx, range(16), []))
    exp = _check(ctx, chans, None, pitch=pitch, aligned=tier(ctx, False, True))
    assert (exp["type"] == EV_FICH).sum() == len(chans) * keep.sum()
    assert (exp["type"] == EV_DCH).sum() == len(chans) * yse["dch_ok"][ds[keep]].sum() < len(chans) * keep.sum()


# ------------------------------------------------------------------ header CSD, sub frame flag, outlived FICH
def test_header_csd_vs_reference(ctx, yse, gold):
    """Header frames whose halves carry CSD vectors in all four combinations of accepted and rejected (every vector shown in
    both halves): META_RESET b = 1, then HEADER_DCH for exactly the accepted halves with the reference's 20 bytes.  Around
    them: an FR frame after a header gives blocks 3 and 4 only (38 bytes), also with a V/D2 frame in between (only an FR
    frame clears the flag) and with a push boundary in between (481 symbols a push: every frame in a push of its own); a
    terminator gives META_RESET b = 2; a V/D2 frame with a broken FICH after a good one still gives 40 bytes and a MODE
    event but neither FICH nor DCH; frames before any valid FICH give nothing."""
    P = _Parts(yse, gold, 35)
    v = yse
    acc, rej = np.nonzero(v["csd_ok"] == 1)[0], np.nonzero(v["csd_ok"] == 0)[0]
    step = tier(ctx, 1, 12)
    combos = []
    for k in range(0, max(len(acc), len(rej)), step):
        a, a2, r, r2 = acc[k % len(acc)], acc[(k + 7) % len(acc)], rej[k % len(rej)], rej[(k + 5) % len(rej)]
        combos += [(a, a2), (a, r), (r, a), (r, r2)]
    B = tier(ctx, 8, 2)
    chans, n38 = [], 0
    dch_ok = np.nonzero((v["dch_ok"] == 1) & (v["dch_src"] >= 1))[0]
    for b in range(B):
        c = _Channel()
        for k in range(2):                                           # nothing before the first valid FICH, whatever the frames carry
            P.v2_frame(c, P.broken_fich(2 * b + k), dch_ok[b + k])
        for k, (i, j) in enumerate(combos[b::B]):
            p, csd = P.header_payload(i, j)
            c.frame(P.fich(0, (k + b) & 3, k), p, csd=csd)
            kind = (k + b) % 5
            if kind == 0:                                            # FR right behind the header: 38 bytes, then a full FR frame
                c.frame(P.fich(1, 3, k), P.random_payload()); n38 += 1
                c.frame(P.fich(1, 3, k + 1), P.random_payload())
            elif kind == 1:                                          # a V/D2 frame leaves the flag set
                P.v2_frame(c, P.v2_fich(k & 7, k), dch_ok[(k + b) % len(dch_ok)])
                c.frame(P.fich(1, 3, k), P.random_payload()); n38 += 1
            elif kind == 2:                                          # V/D2, then a V/D2 frame under the outlived FICH, then a terminator
                P.v2_frame(c, P.v2_fich(k & 7, k), dch_ok[(k + b) % len(dch_ok)])
                P.v2_frame(c, P.broken_fich(k), dch_ok[(k + b + 1) % len(dch_ok)])
                c.frame(P.fich(2, k & 3, k), P.random_payload())
            elif kind == 3:                                          # V/D1 and data FR leave the flag too; frame type 3 gives nothing
                c.frame(P.fich(1, 0, k), P.random_payload())
                c.frame(P.fich(1, 1, k), P.random_payload())
                c.frame(P.fich(3, k & 3, k), P.random_payload())
                c.frame(P.fich(1, 3, k), P.random_payload()); n38 += 1
        chans.append(c)
    shown = {(h, int(x[h])) for x in combos for h in (0, 1)}
    assert step > 1 or shown == {(h, i) for h in (0, 1) for i in range(len(v["csd_in"]))}
    assert {int(v["csd_src"][i]) for _, i in shown} == {0, 1, 2, 3, 4}
    for chunk in (None, 481, 1000):
        exp = _check(ctx, chans, chunk)
        hd = exp[exp["type"] == EV_HEADER_DCH]
        assert (hd["a"] == 0).sum() == 2 * len(combos) // 4 == (hd["a"] == 1).sum()
        assert {int(b) for b in exp["b"][exp["type"] == EV_META_RESET]} == {1, 2}
    sizes = [sum(len(o) for o in c.out) for c in chans]
    assert n38 >= tier(ctx, 20, 6) and all(s > 0 for s in sizes)


# ------------------------------------------------------------------ V/D2 voice blocks
def _v2_cases(thin):
    tri = [0, 8, 17, 26] if thin else range(27)                      # (triplets 8 and 17 straddle two rows of the 26 x 4 de-interleave)
    cases = [()]
    cases += [(3 * t + k,) for t in tri for k in range(3)]
    cases += [tuple(3 * t + k for k in range(3) if k != skip) for t in tri for skip in range(3)]
    cases += [(3 * t, 3 * t + 1, 3 * t + 2) for t in ([8] if thin else range(0, 27, 5))]
    cases += [(81 + k,) for k in ([0, 10, 21] if thin else range(22))]
    cases += [(103,), (1, 4), (25, 26, 27, 28)]                       # pad bit; one wrong bit in each of two triplets; two and two
    return cases


def test_v2_voice_majority_vote(ctx, yse, gold):
    """V/D2 voice blocks with no wrong bit, one wrong bit at each place of each of the 27 triplets, two (each pair) and three
    wrong bits in a triplet, each of the 22 unprotected bits wrong, the pad bit wrong -- every case in each of the five
    blocks of a frame and in frames at every position 0..15 of a 16-frame chunk (on the emulation a thinned set of cases that
    keeps the two triplets straddling de-interleave rows).  The expected 7 bytes come from the AMBE bits
    given to the encoder and the wrong bits injected, never from a decoder."""
    P = _Parts(yse, gold, 36)
    cases = _v2_cases(tier(ctx, False, True))
    C = len(cases)
    clean = np.nonzero(yse["dch_src"] == 0)[0]
    chans, seen = [], set()
    for j in range(16):
        c = _Channel()
        for k in range(C + 4 + j):
            blocks = []
            for b in range(5):
                i = k - b - j
                blocks.append(_v2_block(P.rng.integers(0, 2, 49), cases[i] if 0 <= i < C else ()))
                if 0 <= i < C:
                    seen.add((i, b, k % 16))
            P.v2_frame(c, P.v2_fich(k & 7, k), clean[k % len(clean)], blocks)
        chans.append(c)
    assert seen == {(i, b, q) for i in range(C) for b in range(5) for q in range(16)}
    exp = _check(ctx, chans, None)
    assert (exp["type"] == EV_DCH).sum() == sum(len(c.rows) for c in chans)


def test_v2_block_model_is_the_encoders_inverse():
    """the expectation above on its own terms: no wrong bit -> the AMBE bits as given, packed; a flipped triplet flips exactly
    the AMBE bit the encoder took it from"""
    rng = np.random.default_rng(37)
    ambe = rng.integers(0, 2, 49)
    assert _v2_block(ambe)[0].tolist() == synth.ysf_v2_voice_dibits([int(b) for b in ambe])
    assert (_v2_block(ambe)[1] == np.packbits(np.concatenate([ambe, np.zeros(7, int)]).astype(np.uint8))).all()
    for t in range(27):
        a, b = _v2_block(ambe, (3 * t, 3 * t + 2))[1], _v2_block(ambe)[1]
        assert np.nonzero(np.unpackbits(a ^ b))[0].tolist() == [synth._V2_MAP[t]]
        assert (_v2_block(ambe, (3 * t + 1,))[1] == b).all() and (_v2_block(ambe, (3 * t + 1,))[0] != _v2_block(ambe)[0]).any()
    for k in range(22):
        assert np.nonzero(np.unpackbits(_v2_block(ambe, (81 + k,))[1] ^ _v2_block(ambe)[1]))[0].tolist() == [synth._V2_MAP[27 + k]]


# ------------------------------------------------------------------ V/D1, voice FR, data FR
def test_v1_and_full_rate_bytes(ctx, yse, gold):
    """V/D1 (50 bytes a frame: the mode byte and nine bytes that each hold dibit 4 (j - 1) + 3 of the block unshifted), voice FR
    (95 bytes: mode byte and 18 bytes of four dibits, first on top) and data FR (nothing) frames of random payload, in runs
    and mixed; expected bytes straight from the dibits."""
    P = _Parts(yse, gold, 38)
    chans = []
    for b in range(tier(ctx, 8, 2)):
        c = _Channel()
        kinds = [0] * 5 + [3] * 5 + [1] * 3 + list(P.rng.choice([0, 1, 3], tier(ctx, 40, 12)))
        for k, dt in enumerate(kinds):
            c.frame(P.fich(1, int(dt), k + b), P.random_payload())
        chans.append(c)
    for chunk in (None, 481, 37):
        exp = _check(ctx, chans, chunk)
        assert set(exp["type"]) == {EV_FICH, EV_MODE} and set(exp["b"][exp["type"] == EV_MODE]) == {0, 1, 3}
    assert all(len(c.bytes()) >= 5 * 50 + 5 * 95 for c in chans)


# ------------------------------------------------------------------ sync count: META_RESET b = 0 and the search behind it
def test_sync_count_and_relock(ctx, yse, gold):
    """Sync words with 3 wrong bits count for the sync, with 4 against it (ysf_phase.cpp:16-18); the count starts at 0 with
    every lock, so a second bad sync word right behind a lock gives META_RESET b = 0 at that frame and the search walks on to
    the next frame with a good one -- where the frame phase starts anew WITHOUT a FICH (a frame with a broken FICH there
    gives nothing)."""
    P = _Parts(yse, gold, 39)
    rng = np.random.default_rng(40)
    dch_ok = np.nonzero(yse["dch_ok"] == 1)[0]
    chans = []
    for b in range(tier(ctx, 6, 2)):
        c = _Channel()
        plan = [3, 4, 3, 0, 4, 4, 4, 0, 0, 3, 4, 4, 4, 4, 2, 0, 0, 0, 4, 0, 4, 0, 4, 4, 4, 0]
        for k, nwrong in enumerate(plan):
            wrong = tuple(rng.choice(40, nwrong, replace=False))
            fich = P.broken_fich(k + b) if k in (7, 14) else P.v2_fich(k & 7, k + b)
            P.v2_frame(c, fich, dch_ok[(5 * k + b) % len(dch_ok)], sync_wrong=wrong)
        chans.append(c)
    for chunk in (None, 961, 37):
        exp = _check(ctx, chans, chunk)
        assert (exp["type"] == EV_META_RESET).sum() >= 2 * len(chans) and not exp["b"][exp["type"] == EV_META_RESET].any()


# ------------------------------------------------------------------ mixed streams against the oracle
def _mixed(n_channels=36):
    """36 channels of synth.ysf_mixed_stream: six with a loss at a different frame each, some with scattered wrong dibits, two
    whose sync words sit exactly at the limit"""
    out = []
    for s in range(n_channels):
        kw = {}
        if s % 6 == 1:
            kw["loss"] = (3 + 2 * (s // 6), 2 + s // 12)
        if s % 6 == 4:
            kw["err"] = [0.002, 0.01, 0.03][(s // 6) % 3]
        if s == 2:                                                   # 3 wrong bits lock and count; 4 and 4 behind a lock: back to the search
            kw.update(absent=0, force={0: {"sync_errors": 3, "fich": "intact"}, 1: {"sync_errors": 3}, 2: {"sync_errors": 4}, 3: {"sync_errors": 4},
                                       4: {"sync_errors": 4}, 5: {"sync_errors": 0, "fich": "intact"}})
        if s == 3:                                                   # 4 wrong bits do not lock: the first frame is searched through
            kw.update(absent=0, force={0: {"sync_errors": 4, "fich": "intact"}, 1: {"sync_errors": 3, "fich": "intact"}})
        out.append(synth.ysf_mixed_stream(100 + s, 26, lead_in=17 + 3 * s, **kw))
    return out


@pytest.fixture(scope="module")
def mixed(oracle):
    """the streams, their records, and the oracle's bytes and events: whole, and frame by frame"""
    res = []
    for s, rec in _mixed():
        out, ev = oracle.Decoder("ysf").process(s)
        dec, per_frame, lo = oracle.Decoder("ysf"), [], 0
        for k in range(len(rec)):
            hi = rec[k]["start"] + 481
            o, e = dec.process(s[lo:hi]); lo = hi
            per_frame.append((o, e))
        o, e = dec.process(s[lo:])
        per_frame.append((o, e))
        assert (np.concatenate([p[0] for p in per_frame]) == out).all() and np.concatenate([p[1] for p in per_frame]).tobytes() == ev.tobytes()
        res.append((s, rec, out, ev, per_frame))
    return res


def test_mixed_streams_walk_the_whole_frame_machine(mixed):
    """what the mixed streams make the ORACLE do (so what the comparison below covers): every event type, META_RESET for sync
    loss, header and terminator, frames of 50, 40, 95 and 38 output bytes, frames decoded under a FICH that outlived a broken
    one, frames before any FICH, and sync words exactly at the limit on both sides"""
    ev = np.concatenate([m[3] for m in mixed])
    assert set(ev["type"]) == {EV_FICH, EV_MODE, EV_DCH, EV_HEADER_DCH, EV_META_RESET}
    assert set(ev["b"][ev["type"] == EV_META_RESET]) == {0, 1, 2}
    assert set(ev["a"][ev["type"] == EV_HEADER_DCH]) == {0, 1}
    sizes, outlived, before_fich = set(), 0, 0
    for s, rec, out, e, per_frame in mixed:
        for k, r in enumerate(rec):
            o, fe = per_frame[k]
            fe = fe[fe["sym_index"] == r["start"]]
            sizes.add(len(o))
            if r["fich"] == "random" and (fe["type"] == EV_MODE).any() and not (fe["type"] == EV_FICH).any():
                outlived += 1
            if r["fich"] == "absent" and len(fe) == 0 and len(o) == 0:
                before_fich += 1
    assert {50, 40, 95, 38, 0} <= sizes and sizes <= {50, 40, 95, 38, 0, 90, 135, 145, 80, 78, 88, 133, 190, 100}, sizes
    assert outlived >= 10 and before_fich >= 30
    # channel 2: locks at frame 0 with 3 wrong bits (FICH event there), frame 1 counts up with 3, frames 2..3 count down to 0
    # with 4 each, frame 4 falls below: META_RESET b = 0 exactly there
    s, rec, out, e, _ = mixed[2]
    assert [r["sync_errors"] for r in rec[:5]] == [3, 3, 4, 4, 4]
    assert (e[e["sym_index"] == rec[0]["start"]]["type"] == EV_FICH).any()
    first_reset = e[(e["type"] == EV_META_RESET) & (e["b"] == 0)][0]
    assert first_reset["sym_index"] == rec[4]["start"]
    # channel 3: 4 wrong bits do not lock
    s, rec, out, e, _ = mixed[3]
    assert rec[0]["sync_errors"] == 4 and rec[1]["sync_errors"] == 3 and e[0]["sym_index"] == rec[1]["start"] and e[0]["type"] == EV_FICH


@pytest.mark.parametrize("chunk", [None, 1000, 481, 37])
def test_mixed_streams_match_oracle(ctx, mixed, chunk):
    """the 36 mixed streams (a fixed six of them on the emulation: a loss, scattered errors, the two at the sync limit)
    through decoder-only engines, whole and in pushes of 1000, 481 and 37 symbols: bytes and events equal the oracle's"""
    pick = tier(ctx, list(range(36)), [0, 1, 2, 3, 4, 11])
    streams = [mixed[i][0] for i in pick]
    assert_rows(_run(ctx, streams, chunk), [mixed[i][2:4] for i in pick], ["stream %d push %s" % (i, chunk) for i in pick])


def test_mixed_stream_through_the_full_chain(ctx, oracle, mixed):
    """one mixed stream (and one with a loss) shaped to samples and run through a full proto="ysf" engine -- the chain kernel
    decodes from its own symbol view, not from a pushed symbol buffer -- against oracle.chain"""
    x = [synth.shape(mixed[i][0]) for i in (0, 7)]
    n = min(len(a) for a in x)
    x = np.stack([a[:n] for a in x])
    ref = oracle.chain(x, proto=2)
    assert ref["event_count"].min() > 30 and ref["out_count"].min() > 300
    assert_matches_oracle(run_engine(ctx, x, "ysf", [50000, 20011]), ref, len(x), "mixed")
