"""NXDN frame elements through the product, against the REFERENCE's own results.

tests/golden/nxdn_elements_ref.npz (make_golden_nxdn_elements.py) holds SACCH and FACCH1 blocks chosen so that the tie
rules and the start-state rule of the reference's channel decoder decide (single and paired dibit errors, k flipped bits,
random blocks its CRC passes), each with what oracle/_ref/libdigiham_ref_nxdn.so made of it.  Decoder-only engines (the
CPU wave emulation and, with -m gpu, libdigiham_amd.so -- whose Viterbi forward pass is code the emulation never runs)
are fed frames that carry one vector each, under every LICH that changes how the frame is decoded, and every event
they emit is held to the frame machine of nxdn_phase.cpp:43-170 restated below (`_Channel`) and fed with the REFERENCE's
element results: LICH, SACCH, SACCH_SF, SYNC_VOICE and FACCH1 events, position by position, and the voice bytes.
"""
import json
import os

import numpy as np
import pytest

from common import npz_digest
from dec_harness import assert_rows, first_differing_frame, run_symbols, tier
from digiham_amd import api, synth

HERE = os.path.dirname(os.path.abspath(__file__))
EV_LICH, EV_SACCH, EV_SACCH_SF, EV_VOICE, EV_FACCH1, EV_META_RESET = 32, 33, 34, 35, 36, 37
TX_RELEASE = 0x08
LEAD = 29
SYNC = np.array(synth.NXDN_SYNC, np.uint8)
PN = np.array(synth.nxdn_scramble([0] * 182), np.uint8)          # the frame's scrambler sequence as an XOR mask
PUSHES = [None, 193, 385, 577, 769]                              # one push; pushes that leave 1, 2, 3, 4 whole frames in hand


@pytest.fixture(scope="module")
def nxe():
    with np.load(os.path.join(HERE, "golden", "nxdn_elements_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def nx():
    return np.load(os.path.join(HERE, "golden", "nxdn_ref.npz"))


def _miscorrected(v, name):
    return (v[name + "_ok"] == 1) & (v[name + "_has_clean"] == 1) & (v[name + "_out"] != v[name + "_clean"]).any(axis=1)


# ------------------------------------------------------------------ the fixture itself
def test_fixture_conditions_and_reference(oracle, nxe):
    """The committed vectors are the ones the reference produced (digest taken at generation; oracle/_ref, where it is
    built, reproduces every expected column), every class the product tests rely on is populated, and the oracle's
    restatement agrees with all of them."""
    path = os.path.join(HERE, "golden", "nxdn_elements_ref.npz")
    assert npz_digest(path) == json.load(open(os.path.join(HERE, "golden", "ref_compare_hashes.json")))["nxdn_elements_ref_npz"]
    assert os.path.getsize(path) < 300 * 1024
    for name, n_each, n_mis in (("sacch", 500, 100), ("facch1", 300, 30)):
        ok = nxe[name + "_ok"] == 1
        assert ok.sum() >= n_each and (~ok).sum() >= n_each, name
        assert _miscorrected(nxe, name).sum() >= n_mis, name                 # accepted by the CRC with another payload than sent
        assert sorted(set(nxe[name + "_src"])) == [0, 1, 2, 3, 4][:5 if name == "sacch" else 4]
    assert not ((nxe["facch1_ok"] == 1) & ((nxe["facch1_out"][:, 0] & 0x3F) == TX_RELEASE)).any()
    assert len(nxe["filler_facch1_in"]) >= 4 and not nxe["filler_facch1_ok"].any() and not nxe["filler_sacch_ok"].any()
    for which in ("oracle", "ref"):
        if which == "ref" and oracle.ref_nxdn() is None:
            continue
        for name, fn in (("sacch", oracle.nxdn_sacch), ("facch1", oracle.nxdn_facch1)):
            for d, ok, o in zip(nxe[name + "_in"], nxe[name + "_ok"], nxe[name + "_out"]):
                got_ok, got = fn(d, which)
                assert got_ok == bool(ok) and (not got_ok or (got == o).all()), (which, name)
            for d in nxe["filler_" + name + "_in"]:                          # filler blocks: rejected, so they leave no event
                assert not fn(d, which)[0], (which, name)


# ------------------------------------------------------------------ frames, and what the reference's frame machine makes of them
def _lich8(value):
    return np.array(synth.nxdn_lich_dibits(value), np.uint8)


def _pack_voice(d72):
    d = np.asarray(d72, np.uint8).reshape(18, 4)
    return (d[:, 0] << 6 | d[:, 1] << 4 | d[:, 2] << 2 | d[:, 3]).astype(np.uint8)


class _Channel:
    """One channel's frames and the events / voice bytes FramedPhase::process (nxdn_phase.cpp:43-170) gives for them when
    Lich::parse, Sacch::parse and Facch1::parse return what the REFERENCE returned for the vector each frame carries
    (SacchSuperframeCollector: sacch.cpp:90-131).  All frames carry an intact sync word, so the sync count never falls."""

    def __init__(self):
        self.rows, self.ev, self.out = [], [], []
        self.lich, self.have, self.data = -1, 0, [None] * 4

    def _emit(self, pos, typ, a, payload):
        e = np.zeros(1, api.EVENT_DTYPE)
        e["sym_index"], e["type"], e["a"], e["len"] = pos, typ, a, len(payload)
        e["payload"][0, :len(payload)] = np.frombuffer(bytes(payload), np.uint8)
        self.ev.append(e)

    def frame(self, lich8, lich, sacch30, sacch, blocks):
        """lich = Lich::parse's value or -1; sacch = (ok, 5 bytes); blocks = two (72 dibits, (ok, 12 bytes) or None when the
        block is never read as a FACCH1)"""
        pos = LEAD + 192 * len(self.rows)
        self.rows.append(np.concatenate([lich8, sacch30, blocks[0][0], blocks[1][0]]).astype(np.uint8))
        if lich >= 0:
            self.lich = int(lich)
            self._emit(pos, EV_LICH, 0, [self.lich])
        g = self.lich                                                       # a parity failure leaves the previous LICH in charge
        if g < 0 or (g >> 5) & 3 == 0 or (g >> 3) & 3 == 1:                 # RCCH, UDCH: the frame body is skipped
            return
        if (g >> 3) & 3 == 2 and sacch[0]:
            o = np.asarray(sacch[1], np.uint8)
            index = int(o[0] >> 6) ^ 3
            self._emit(pos, EV_SACCH, index, o)
            if not (index > 0 and not (self.have >> (index - 1)) & 1):
                self.have |= 1 << index
                self.data[index] = o[1:5]
            if self.have == 0xF:
                bits = np.concatenate([np.unpackbits(d)[:18] for d in self.data])
                self._emit(pos, EV_SACCH_SF, 0, np.packbits(bits))
                self.have = 0
        for i in (0, 1):
            d72, facch1 = blocks[i]
            if ((g >> 1) & 3) >> (1 - i) & 1:
                self._emit(pos, EV_VOICE, 0, [])
                self.out.append(_pack_voice(d72))
            elif facch1[0]:
                assert facch1[1][0] & 0x3F != TX_RELEASE
                self._emit(pos, EV_FACCH1, i, np.asarray(facch1[1], np.uint8))

    def stream(self, lead):
        body = np.stack(self.rows) ^ PN
        fr = np.concatenate([np.broadcast_to(SYNC, (len(body), 10)), body], axis=1).reshape(-1)
        s = np.concatenate([lead, fr, np.zeros(200, np.uint8)])              # (the last frame needs one more dibit in hand)
        for k in range(LEAD):                                                # the sync search must lock at LEAD, not before
            assert int(np.unpackbits(s[k:k + 10] ^ SYNC).sum()) > 2
        return s


def _check(ctx, chans, chunk):
    """push the channels' streams and hold events and voice bytes to the model; returns all expected events"""
    lead = np.random.default_rng(5).integers(0, 4, LEAD).astype(np.uint8)
    K = len(chans[0].rows)
    assert all(len(c.rows) == K for c in chans)
    streams = np.stack([c.stream(lead) for c in chans])
    run = run_symbols(ctx, "nxdn", streams, chunk, capacity=max(chunk or streams.shape[1], 16))
    end = LEAD + 192 * K
    got, want, what = [], [], []
    for c, out, ev in zip(chans, run.frames, run.events):
        voice = np.concatenate(c.out) if c.out else np.zeros(0, np.uint8)
        assert len(out) - len(voice) <= 36, "push %s: voice bytes" % chunk   # (at most the zero padding's first frame)
        got.append((out[:len(voice)], ev[ev["sym_index"] < end]))
        want.append((voice, np.concatenate(c.ev)))
        what.append("push %s frame %s" % (chunk, first_differing_frame(got[-1][1], want[-1][1], LEAD, 192)))
    assert_rows(got, want, what)
    return np.concatenate([np.concatenate(c.ev) for c in chans])


def _split(idx, B, group):
    """idx dealt to B channels in whole groups; the last group is filled up from the front, so every index is shown"""
    per = -(-len(idx) // (B * group)) * group
    idx = np.resize(idx, B * per)
    return idx.reshape(B, per // group, group)


def _voice(rng):
    return (rng.integers(0, 4, 72).astype(np.uint8), None)


# ------------------------------------------------------------------ SACCH
def _sacch_channels(v, idx, B):
    """every vector in a both-voice frame (LICH 0x56: SACCHs decoded four ahead into S.colword) and in frames with two, the
    first or the second block a FACCH1 (0x50, 0x52, 0x54: the ragged pass), in runs of five frames per kind"""
    fill = [(d, (False, None)) for d in v["filler_facch1_in"]]
    chans, rng = [], np.random.default_rng(21)
    for groups in _split(idx, B, 5):
        c = _Channel()
        for g in groups:
            for lich in (0x56, 0x50, 0x52, 0x54):
                for i in g:
                    opt = (lich >> 1) & 3
                    blocks = [_voice(rng) if (opt >> (1 - k)) & 1 else fill[(i + k) % len(fill)] for k in (0, 1)]
                    c.frame(_lich8(lich), lich, v["sacch_in"][i], (v["sacch_ok"][i], v["sacch_out"][i]), blocks)
        chans.append(c)
    return chans


@pytest.mark.parametrize("chunk", PUSHES)
def test_sacch_events_vs_reference(ctx, nxe, chunk):
    """Every SACCH vector (a fixed quarter of them on the emulation), 4 frame kinds, 16 channels: a SACCH event exactly where
    the reference's CRC passed, with its structure index and five bytes -- 127 of them miscorrections that only the
    reference's tie rules reproduce; SACCH_SF events as SacchSuperframeCollector gives them for those results."""
    n = len(nxe["sacch_in"])
    idx = np.arange(n) if tier(ctx, True, False) else np.arange(3, n, 4)
    exp = _check(ctx, _sacch_channels(nxe, idx, tier(ctx, 16, 2)), chunk)
    assert (exp["type"] == EV_SACCH).sum() >= 4 * nxe["sacch_ok"][idx].sum() > 0
    assert _miscorrected(nxe, "sacch")[idx].sum() >= tier(ctx, 100, 25)
    assert (exp["type"] == EV_SACCH_SF).sum() >= tier(ctx, 5, 1) and not (exp["type"] == EV_FACCH1).any()


def test_no_sacch_event_without_superframe_sacch(ctx, nxe):
    """SACCHs the reference accepts, under LICHs whose functional channel is not the superframe SACCH (0 and 3; voice or
    FACCH1 blocks): the 30 dibits are skipped, no SACCH or SACCH_SF event (nxdn_phase.cpp:104)."""
    acc = np.nonzero(nxe["sacch_ok"])[0][:tier(ctx, 160, 40)]
    fill = [(d, (False, None)) for d in nxe["filler_facch1_in"]]
    chans, rng = [], np.random.default_rng(22)
    for groups in _split(acc, tier(ctx, 4, 2), 5):
        c = _Channel()
        for g in groups:
            for lich in (0x46, 0x5E, 0x40, 0x42, 0x5C):
                for i in g:
                    opt = (lich >> 1) & 3
                    blocks = [_voice(rng) if (opt >> (1 - k)) & 1 else fill[(i + k) % len(fill)] for k in (0, 1)]
                    c.frame(_lich8(lich), lich, nxe["sacch_in"][i], (True, nxe["sacch_out"][i]), blocks)
        chans.append(c)
    for chunk in (None, 577):
        exp = _check(ctx, chans, chunk)
        assert set(exp["type"]) == {EV_LICH, EV_VOICE}


# ------------------------------------------------------------------ FACCH1
def _facch1_channels(v, idx, B):
    """every vector in block 0 and in block 1, under options 0 (with another vector in the other block), 1 and 2 (voice in
    the other block), with the superframe SACCH wanted (0x50 / 0x52 / 0x54) and not (0x40 / 0x42 / 0x44).  A both-voice
    frame in front of each run with SACCH leaves the next frames' SACCHs in S.colword, so the pass sizes are {0,96,96},
    {0,96,0}, {0,0,96} there and {36,96,96}, {36,96,0}, {36,0,96} from the run's fourth frame on."""
    n_s = len(v["sacch_in"])
    sacch = lambda j: (v["sacch_in"][j % n_s], (v["sacch_ok"][j % n_s], v["sacch_out"][j % n_s]))
    fa = lambda i: (v["facch1_in"][i], (v["facch1_ok"][i], v["facch1_out"][i]))
    mirror = dict(zip(idx.tolist(), idx[::-1].tolist()))
    chans, rng = [], np.random.default_rng(23)
    for b, groups in enumerate(_split(idx, B, 5)):
        c = _Channel()
        for g in groups:
            for lich in (0x50, 0x52, 0x54, 0x40, 0x42, 0x44):
                if lich & 0x10:
                    s30, s = sacch(7 * len(c.rows) + b)
                    c.frame(_lich8(0x56), 0x56, s30, s, [_voice(rng), _voice(rng)])
                for i in g:
                    opt = (lich >> 1) & 3
                    blocks = [fa(i), fa(mirror[int(i)])] if opt == 0 else [fa(i), _voice(rng)] if opt == 1 else [_voice(rng), fa(i)]
                    s30, s = sacch(7 * len(c.rows) + b)
                    c.frame(_lich8(lich), lich, s30, s, blocks)
        chans.append(c)
    return chans


@pytest.mark.parametrize("chunk", [None, 1000, 385])
def test_facch1_events_vs_reference(ctx, nxe, chunk):
    """Every FACCH1 vector (a fixed quarter on the emulation) in both block positions under six LICHs: a FACCH1 event exactly
    where the reference's CRC-12 passed, with the block index and its 12 bytes (40 of them miscorrections); the voice
    block of a mixed frame comes out as its 18 descrambled bytes."""
    n = len(nxe["facch1_in"])
    idx = np.arange(n) if tier(ctx, True, False) else np.arange(1, n, 4)
    exp = _check(ctx, _facch1_channels(nxe, idx, tier(ctx, 16, 2)), chunk)
    fa = exp[exp["type"] == EV_FACCH1]
    n_ok = int(nxe["facch1_ok"][idx].sum())
    assert (fa["a"] == 0).sum() >= 4 * n_ok > 0 and (fa["a"] == 1).sum() >= 4 * n_ok
    assert _miscorrected(nxe, "facch1")[idx].sum() >= tier(ctx, 30, 8)


# ------------------------------------------------------------------ LICH
def test_lich_events_and_governing_lich_vs_reference(ctx, oracle, nx, nxe):
    """All 320 LICH vectors of nxdn_ref.npz (random dibits and the 128 values): a LICH event exactly where the reference's
    parity check passes, with its value.  After a parity failure the previous LICH governs, and RCCH / UDCH LICHs skip
    the frame body: both show in which SACCH / FACCH1 / voice events the frame produces.  Every frame carries a SACCH and
    two FACCH1 blocks the reference accepts; each channel sees the vectors in another order."""
    lich_in, lich_out = nx["lich_in"], nx["lich_out"]
    if oracle.ref_nxdn() is not None:
        assert [oracle.nxdn_lich(r, "ref") for r in lich_in] == list(lich_out)
    s_acc, f_acc = np.nonzero(nxe["sacch_ok"])[0], np.nonzero(nxe["facch1_ok"])[0]
    chans, after_failure, rng = [], set(), np.random.default_rng(24)
    for b in range(tier(ctx, 16, 2)):
        order = np.random.default_rng(40 + b).permutation(len(lich_in))
        c = _Channel()
        c.frame(_lich8(0x56), 0x56, nxe["sacch_in"][s_acc[b]], (True, nxe["sacch_out"][s_acc[b]]), [_voice(rng), _voice(rng)])
        for k, i in enumerate(order):
            s, f0, f1 = s_acc[(3 * k + b) % len(s_acc)], f_acc[(5 * k + b) % len(f_acc)], f_acc[(7 * k + 3 * b + 1) % len(f_acc)]
            if lich_out[i] < 0:
                g = c.lich
                after_failure.add("skipped" if (g >> 5) & 3 == 0 or (g >> 3) & 3 == 1 else "sf" if (g >> 3) & 3 == 2 else "no sf")
            c.frame(lich_in[i], int(lich_out[i]), nxe["sacch_in"][s], (True, nxe["sacch_out"][s]),
                    [(nxe["facch1_in"][f], (True, nxe["facch1_out"][f])) for f in (f0, f1)])
        chans.append(c)
    assert (lich_out < 0).sum() >= 50 and after_failure == {"skipped", "sf", "no sf"}
    for chunk in (None, 769):
        exp = _check(ctx, chans, chunk)
        assert (exp["type"] == EV_LICH).sum() == len(chans) * (1 + (lich_out >= 0).sum())
