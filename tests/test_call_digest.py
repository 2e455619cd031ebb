"""DH_FLAG_CALL_DIGEST / Engine(call_digest=True): the event row of a push folded into call records on the device (include/digiham_amd.h,
"Call digest"; digest_core.hpp).

The checker is `digest` below, a plain restatement of that section on bytes.  Raw events come from an engine WITHOUT the flag on the same
symbols, digested events from one with it; both are compared bit for bit, the final records (read from the decoder state) included."""
import functools

import numpy as np
import pytest

from dec_harness import SymbolRun, push_plan
from digiham_amd import _capi, api, synth

EV = api.EVENT_DTYPE
LEN = _capi.CALL_RECORD_BYTES
DS_CALL_RECORD = 56                     # digest_core.hpp: the record's first word in the decoder state


# ------------------------------------------------------------------ the restatement
def digest(proto, record, raw_events):
    """-> (digested events, record after them): the section "Call digest", event by event"""
    rec, out = bytearray(record), []
    assert len(rec) == LEN[proto]
    for ev in raw_events:
        t, a, b, n, p = int(ev["type"]), int(ev["a"]), int(ev["b"]), int(ev["len"]), bytes(bytearray(ev["payload"]))
        before, passes = bytes(rec), False
        if proto == "dmr":
            o = 8 * (a & 1)
            if t == 1:                                                      # SYNC
                rec[o] = b if b in (1, 2) else 3
                if n > 0 and p[0]:
                    rec[o + 1:o + 8] = bytes(7)
            elif t == 2:                                                    # SLOT_RESET
                rec[o:o + 8] = bytes(8)
            elif t == 3:                                                    # META_RESET
                rec[:] = bytes(16)
            elif t == 5:                                                    # SOFT_RESET
                rec[o + 1:o + 8] = bytes(7)
            elif t == 4:                                                    # LC
                op = p[0] & 0x3F
                if n >= 9 and op in (0, 3):
                    rec[o + 1] = 1 if op == 0 else 2
                    rec[o + 2:o + 5] = p[6:9]
                    rec[o + 5:o + 8] = p[3:6]
                else:
                    passes = 4 <= op <= 8                                   # talker alias header .. GPS info
            parts = (before[:8] != bytes(rec[:8])) | (before[8:] != bytes(rec[8:])) << 1
        elif proto == "nxdn":
            if t == 35:                                                     # SYNC_VOICE
                rec[0] = 1
            elif t == 37:                                                   # META_RESET
                rec[:] = bytes(8)
            elif t == 34 and n >= 9 and (p[0] & 0x3F) == 1:                 # SACCH_SF carrying a VCALL
                rec[1] = {1: 1, 4: 2}.get(p[2] >> 5, 0)
                rec[2:4] = p[3:5]
                rec[4:6] = p[5:7]
            parts = 1
        else:
            if t == 17:                                                     # MODE
                rec[0] = 1 + (b & 3)
            elif t == 20:                                                   # META_RESET
                rec[:] = bytes(21)
            elif t == 18:                                                   # DCH
                if n >= 10 and a < 2:
                    rec[1 + 10 * a:11 + 10 * a] = p[:10]
                else:
                    passes = a >= 2
            elif t == 19:                                                   # HEADER_DCH
                if n >= 20 and a == 0:
                    rec[1:21] = p[:20]
                else:
                    passes = a == 1
            parts = 1
        if bytes(rec) != before:
            e = np.zeros((), EV)
            e["sym_index"], e["type"], e["a"], e["b"], e["len"] = ev["sym_index"], _capi.EV_CALL, parts, 0, len(rec)
            e["payload"][:len(rec)] = np.frombuffer(bytes(rec), np.uint8)
            out.append(e)
        elif passes:
            out.append(ev.copy())
    return (np.array(out, EV) if out else np.zeros(0, EV)), bytes(rec)


def records(eng, proto):
    """the call records of an engine's channels, from the decoder state"""
    words = (LEN[proto] + 3) // 4
    w = np.stack([eng.debug_header(100 + DS_CALL_RECORD + i) for i in range(words)], axis=1).astype("<u4")
    return [w[b].tobytes()[:LEN[proto]] for b in range(eng.B)]


def run(ctx, proto, rows, sizes=None, after=None, **kw):
    """-> (events per channel and push, frames per channel, final records).  after(k, eng): called behind push k"""
    with SymbolRun(ctx, proto, rows, sizes, cycle=True, **kw) as r:
        for k in r:
            if after is not None:
                after(k, r.eng)
        rec = records(r.eng, proto)
    return r.events_by_push, r.frames, rec


def same(got, want, what):
    assert len(got) == len(want) and got.tobytes() == want.tobytes(), "%s: %d events, expected %d; first difference at %s" % (
        what, len(got), len(want), next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), None))


# ------------------------------------------------------------------ the streams
def _call(rng, slot, header, embedded, cc=1):
    """a voice call: header LC, one superframe per embedded LC, terminator LC (synth.dmr_call with the LCs chosen)"""
    bursts = [synth.dmr_data_burst(slot, cc, 1, header + bytes(3), "bs_data", rng)]
    for lc in embedded:
        frags = synth.dmr_embedded_lc_fragments(lc)
        for f in range(6):
            mid = synth.DMR_SYNC["bs_voice"] if f == 0 else synth.dmr_emb_mid(cc, [1, 3, 3, 2][f - 1], frags[f - 1]) if f <= 4 else \
                synth.dmr_emb_mid(cc, 0, [0] * 16)
            bursts.append(synth.dmr_voice_burst(slot, list(rng.integers(0, 4, 108)), mid, rng))
    bursts.append(synth.dmr_data_burst(slot, cc, 2, header + bytes(3), "bs_data", rng))
    return bursts


def _tdma(rng, q0, q1, lead_in=37):
    n = 2 * min(len(q0), len(q1))
    out = [int(d) for d in rng.integers(0, 4, lead_in)]
    for i in range(n):
        out += (q0, q1)[i & 1][i >> 1]
    return out


def _noise(rng, n):
    return [int(d) for d in rng.integers(0, 4, n)]


@functools.lru_cache(None)
def dmr_rows():
    """8 channels, about 3 s each: on slot 0 a group call whose superframes carry the group LC, a talker-alias block and a GPS LC, then a
    unit-to-unit call; on slot 1 idle bursts and a group call of its own; a missing burst (the slots swap places: a TACT slot change);
    noise of a few bursts (sync loss); then another call behind noise."""
    rows = []
    for b in range(8):
        rng = np.random.default_rng(4100 + b)
        ids = [int(v) for v in rng.integers(1, 1 << 24, 8)]
        group, alias, gps = synth.dmr_lc(0, 0, 0, ids[0], ids[1]), synth.dmr_lc(4, 0, 0x4A, 0x414243, 0x444546), synth.dmr_lc(8, 0, 0, 0x123456, 0x654321)
        direct, other = synth.dmr_lc(3, 0, 0, ids[2], ids[3]), synth.dmr_lc(0, 0, 0, ids[4], ids[5])
        q0 = [synth.dmr_idle_burst(0, 1, rng) for _ in range(b % 3)] + _call(rng, 0, group, [group, group, alias, group, gps, group]) + \
            [synth.dmr_idle_burst(0, 1, rng) for _ in range(2)] + _call(rng, 0, direct, [direct] * 4)
        q1 = [synth.dmr_idle_burst(1, 1, rng) for _ in range(3 + b % 2)] + _call(rng, 1, other, [other] * 5)
        q1 += [synth.dmr_idle_burst(1, 1, rng) for _ in range(len(q0) - len(q1))]
        first = _tdma(rng, q0, q1[:len(q0)])
        cut = 37 + 144 * (20 + b)                                          # one burst missing: the slots change places
        first = first[:cut] + first[cut + 144:]
        again = synth.dmr_lc(0, 0, 0, ids[6], ids[7])
        q0 = _call(rng, 0, again, [again] * 3)
        q1 = [synth.dmr_idle_burst(1, 1, rng) for _ in range(len(q0))]
        rows.append(np.array(first + _noise(rng, 144 * 3 + 11 * b) + _tdma(rng, q0, q1, lead_in=0) + _noise(rng, 300), np.uint8))
    return tuple(rows)


@functools.lru_cache(None)
def ysf_rows():
    """8 channels: header, V/D2 cycle, terminator, repeated (synth.ysf_stream), 30 frames = 3 s"""
    return tuple(synth.ysf_stream(4200 + b, 30, mode="vd2", lead_in=53 + 7 * b) for b in range(8))


@functools.lru_cache(None)
def nxdn_rows():
    """8 channels of 75 frames (3 s): the frame machine's walk with VCALL superframes and TX releases (synth.nxdn_mixed_stream), and on the
    odd channels whole calls -- FACCH1 VCALL, voice frames, TX_RELEASE -- with noise between them (synth.nxdn_stream)"""
    return tuple(synth.nxdn_stream(4300 + b, 75) if b & 1 else synth.nxdn_mixed_stream(4300 + b, 75)[0] for b in range(8))


ROWS = {"dmr": dmr_rows, "ysf": ysf_rows, "nxdn": nxdn_rows}
_RAW = {}


def raw_run(ctx, proto):
    """the unflagged engine's events and frames on ROWS[proto], one push: computed once per tier, never modified"""
    key = (id(ctx), proto)
    if key not in _RAW:
        ev, frames, rec = run(ctx, proto, ROWS[proto]())
        assert all(r == bytes(LEN[proto]) for r in rec)                    # without the flag nobody writes the record
        _RAW[key] = ([np.concatenate(e) for e in ev], frames)
    return _RAW[key]


# ------------------------------------------------------------------ 1. the contract, three protocols, three cuttings
@pytest.mark.parametrize("proto", ["dmr", "ysf", "nxdn"])
def test_contract(ctx, proto):
    rows = ROWS[proto]()
    raw, raw_frames = raw_run(ctx, proto)
    want = [digest(proto, bytes(LEN[proto]), r) for r in raw]
    assert sum(len(w[0]) for w in want) > 8 and any((w[0]["type"] != _capi.EV_CALL).any() for w in want) == (proto != "nxdn")
    whole = None
    for sizes in (None, 1440, [1441, 333, 2879, 1, 977, 4001]):
        ev, frames, rec = run(ctx, proto, rows, sizes, call_digest=True)
        for b in range(len(rows)):
            got = np.concatenate(ev[b])
            same(got, want[b][0], "%s cut %s channel %d" % (proto, sizes, b))
            assert rec[b] == want[b][1], (proto, sizes, b)
            assert frames[b].tobytes() == raw_frames[b].tobytes()
        # ... and push by push: the record carries over
        plan = push_plan([len(r) for r in rows], sizes, cycle=isinstance(sizes, list))
        assert all(len(e) == len(plan) for e in ev)
        cat = b"".join(np.concatenate(e).tobytes() for e in ev)
        assert whole is None or cat == whole
        whole = cat


# ------------------------------------------------------------------ 2. chunk seams
def _seam_row(lead, second):
    rng = np.random.default_rng(77)
    a, b, c = synth.dmr_lc(0, 0, 0, 1001, 2002), synth.dmr_lc(3, 0, 0, 3003, 4004), synth.dmr_lc(0, 0, 0, 5005, 6006)
    q0 = [synth.dmr_idle_burst(0, 1, rng) for _ in range(lead)] + _call(rng, 0, a, [a]) + _call(rng, 0, c, [c, a])
    q1 = [synth.dmr_idle_burst(1, 1, rng) for _ in range(second)] + _call(rng, 1, b, [b, c])
    q0 += [synth.dmr_idle_burst(0, 1, rng) for _ in range(20)]
    q1 += [synth.dmr_idle_burst(1, 1, rng) for _ in range(20)]
    return np.array(_tdma(rng, q0[:20], q1[:20]) + _noise(rng, 60), np.uint8)


def test_chunk_seam(ctx):
    """one channel, 40 bursts, one push: more than 64 raw events, with identity changes on both sides of raw index 63 | 64"""
    found = None
    for lead in range(0, 8):
        for second in range(0, 8):
            row = _seam_row(lead, second)
            ev, _, _ = run(ctx, "dmr", [row])
            raw = np.concatenate(ev[0])
            changes, r = [], bytes(16)
            for i in range(len(raw)):
                before, (_, r) = r, digest("dmr", r, raw[i:i + 1])
                if r != before:
                    changes.append(i)
            if {62, 63} & set(changes) and {64, 65, 66} & set(changes):
                found = (row, raw, changes)
                break
        if found:
            break
    assert found, "no stream of the family puts identity changes at raw indices 62 .. 66"
    row, raw, changes = found
    want, rec = digest("dmr", bytes(16), raw)
    ev, _, got_rec = run(ctx, "dmr", [row], call_digest=True)
    same(np.concatenate(ev[0]), want, "seam (changes at %s)" % [c for c in changes if 60 <= c <= 68])
    assert got_rec[0] == rec


# ------------------------------------------------------------------ 3. both slots at once
def test_meta_reset_clears_both_slots_in_one_event(ctx):
    rng = np.random.default_rng(5)
    a, b = synth.dmr_lc(0, 0, 0, 91, 92), synth.dmr_lc(3, 0, 0, 93, 94)
    calls = _tdma(rng, _call(rng, 0, a, [a] * 3)[:16], _call(rng, 1, b, [b] * 3)[:16])
    # noise passes for an EMB now and then and keeps a slot alive: take the first noise behind which the raw row has a META_RESET that
    # finds both slots with a call (by the restatement)
    for seed in range(40):
        row = np.array(calls + _noise(np.random.default_rng(seed), 144 * 14), np.uint8)
        ev, _, _ = run(ctx, "dmr", [row])
        want, rec = digest("dmr", bytes(16), np.concatenate(ev[0]))
        if any(e["type"] == _capi.EV_CALL and e["a"] == 3 for e in want):
            break
    ev, _, got_rec = run(ctx, "dmr", [row], call_digest=True, dmr_both_slots=True)
    got = np.concatenate(ev[0])
    same(got, want, "two calls, then noise")
    calls = [api.parse_call("dmr", e) for e in got if e["type"] == _capi.EV_CALL]
    full = [c for c in calls if c["slots"][0] and c["slots"][1] and c["slots"][0]["source"] == 92 and c["slots"][1]["source"] == 94]
    assert full and full[-1]["slots"][0]["type"] == "group" and full[-1]["slots"][1]["type"] == "direct" and full[-1]["slots"][1]["target"] == 93
    both = [e for e in got if e["type"] == _capi.EV_CALL and e["a"] == 3]
    assert len(both) == 1 and api.parse_call("dmr", both[0]) == {"changed": (0, 1), "slots": [None, None]}
    assert got_rec[0] == rec == bytes(16)


# ------------------------------------------------------------------ 4. the reduction is real
def test_reduction(ctx):
    raw, _ = raw_run(ctx, "dmr")
    n_raw = sum(len(r) for r in raw)
    n_restated = sum(len(digest("dmr", bytes(16), r)[0]) for r in raw)
    ev, _, _ = run(ctx, "dmr", dmr_rows(), call_digest=True)
    n_got = sum(len(np.concatenate(e)) for e in ev)
    print("DMR contract stream: %d raw events, %d digested (restatement %d): 1 / %.1f" % (n_raw, n_got, n_restated, n_raw / max(n_got, 1)))
    assert 4 * n_restated <= n_raw and 4 * n_got <= n_raw


# ------------------------------------------------------------------ 5. resets
@pytest.mark.parametrize("how", ["reset_channel", "reset_channels"])
def test_resets_clear_the_record_and_raise_nothing(ctx, how):
    rows = dmr_rows()[:3]
    hit, at = 1, 3                                                         # channel 1, behind the fourth push of 1440 symbols: in mid-call
    seen = {}

    def reset(k, eng):
        if k != at:
            return
        seen["before"] = records(eng, "dmr")
        if how == "reset_channel":
            eng.reset_channel(hit)
        else:
            eng.reset_channels(np.array([b == hit for b in range(len(rows))], np.uint8))
        eng.sync()
        seen["after"] = records(eng, "dmr")
        seen["count"] = eng.events()[1].copy()

    raw, _, _ = run(ctx, "dmr", rows, 1440, after=reset)
    got, _, rec = run(ctx, "dmr", rows, 1440, after=reset, call_digest=True)
    assert seen["before"][hit] != bytes(16) and seen["after"][hit] == bytes(16)          # in mid-call; zero afterwards
    assert [seen["after"][b] for b in (0, 2)] == [seen["before"][b] for b in (0, 2)]     # the others keep theirs
    assert seen["count"][hit] == 0                                                       # no event is raised
    for b in range(len(rows)):
        r, want = bytes(16), []
        for k, e in enumerate(raw[b]):
            w, r = digest("dmr", r, e)
            want.append(w)
            if k == at and b == hit:
                r = bytes(16)
            same(got[b][k], w, "%s channel %d push %d" % (how, b, k))
        assert rec[b] == r
    later = np.concatenate(got[hit][at + 1:])
    calls = [api.parse_call("dmr", e) for e in later if e["type"] == _capi.EV_CALL]
    assert any(s and s["source"] for c in calls for s in c["slots"]), "the next LC raises a CALL event again"


# ------------------------------------------------------------------ 6. validation
def test_validation(ctx):
    assert _capi.FLAG_CALL_DIGEST == 0x800 and _capi.EV_CALL == 96
    bad = [dict(proto="dstar", rrc="none", demod="fsk"), dict(proto="pocsag", rrc="none", demod="fsk", sps=40), dict(proto="scan"),
           dict(proto="none"), dict(proto="dmr", events=False), dict(proto="ysf", overlap_pushes=True), dict(proto="nxdn", events=False),
           dict(proto="dmr", rrc="none", demod="none", overlap_pushes=True)]
    for kw in bad:
        api.Engine(2, 4800, ctx=ctx, **kw).close()                         # legal without the flag
        with pytest.raises(ValueError) as e:
            api.Engine(2, 4800, ctx=ctx, call_digest=True, **kw)
        assert isinstance(e.value, _capi.DhError) and e.value.code == _capi.DH_EINVAL, kw
        import ctypes as C
        cfg = _capi.EngineConfig(struct_size=_capi.EngineConfig.rrc_taps.offset, device=0, n_channels=2, max_samples=4800,
                                 rrc=_capi.RRC[kw.get("rrc", "wide")], demod=_capi.DEMOD[kw.get("demod", "gfsk")], sps=kw.get("sps", 10),
                                 proto=_capi.PROTO[kw["proto"]], slot_filter=3, stream=ctx.mem.stream(),
                                 flags=_capi.FLAG_CALL_DIGEST | (0 if kw.get("events", True) else _capi.FLAG_NO_EVENTS) |
                                 (_capi.FLAG_OVERLAP_PUSHES if kw.get("overlap_pushes") else 0))
        h = C.c_void_p(0x1234)
        assert ctx.lib.dh_engine_create(C.byref(cfg), C.byref(h)) == _capi.DH_EINVAL and not h.value, kw      # no handle
    for proto, kw in (("dmr", {}), ("ysf", {}), ("nxdn", dict(rrc="narrow", sps=20))):
        api.Engine(2, 4800, ctx=ctx, proto=proto, call_digest=True, **kw).close()


# ------------------------------------------------------------------ 7. frames and symbols are untouched
@pytest.mark.parametrize("kw", [dict(), dict(dmr_both_slots=True), dict(split_stages=True)], ids=["plain", "both_slots", "split_stages"])
def test_frames_and_symbols_are_untouched(ctx, kw):
    from common import run_engine
    x = np.stack([synth.shape(r[:4800]) for r in dmr_rows()[:2]]).astype(np.float32)
    res = [run_engine(ctx, x, "dmr", [16000, 9000, 23000], call_digest=flag, **kw) for flag in (False, True)]
    for b in range(len(x)):
        assert res[0]["syms"][b].tobytes() == res[1]["syms"][b].tobytes() and len(res[0]["syms"][b]) > 4700
        assert res[0]["frames"][b].tobytes() == res[1]["frames"][b].tobytes() and len(res[0]["frames"][b]) > 0
        same(res[1]["events"][b], digest("dmr", bytes(16), res[0]["events"][b])[0], "chain %s channel %d" % (kw, b))


# ------------------------------------------------------------------ 8. the full chain at width (GPU tier)
@pytest.mark.gpu
def test_chain_70_channels(gpu_ctx):
    from common import run_engine
    base = np.stack([synth.shape(r[:4800]) for r in dmr_rows()]).astype(np.float32)          # 1 s each
    x = np.stack([np.roll(base[b % 8], 480 * (b // 8)) for b in range(70)])
    res = [run_engine(gpu_ctx, x, "dmr", [30000, 18000], call_digest=flag) for flag in (False, True)]
    assert sum(len(e) for e in res[0]["events"]) > 70 * 40
    for b in range(70):
        same(res[1]["events"][b], digest("dmr", bytes(16), res[0]["events"][b])[0], "channel %d" % b)
        assert res[0]["frames"][b].tobytes() == res[1]["frames"][b].tobytes()


@pytest.mark.gpu
def test_chain_8227_channels_behind_the_fixup_launch(gpu_ctx, monkeypatch):
    """The tail split takes pushes of at least 65 536 samples (1.4 s), so that is what the rows bring.  Every third channel's later part
    gives up (DH_TAIL_SPLIT_FORCE_FAIL): the fix-up launch finishes those rows, and the digest has to come behind it."""
    import hashlib
    import torch
    from digiham_amd import synth_torch
    U, B = 16, 8192 + 35
    base, info = synth_torch.make_batch(torch, gpu_ctx.mem.device, "dmr", U, 50, U=U, seed=778)
    T = info["samples_per_channel"]
    assert T >= 65536
    x = base.repeat((B + U - 1) // U, 1)[:B].contiguous()
    monkeypatch.setenv("DH_TAIL_SPLIT", "80")
    monkeypatch.setenv("DH_TAIL_SPLIT_FORCE_FAIL", "3")
    out = []
    for flag in (False, True):
        eng = api.Engine(B, T, proto="dmr", ctx=gpu_ctx, call_digest=flag)
        eng.push(x)
        (e, ec), (f, fc) = eng.events(), eng.frames()
        assert int(eng.debug_header(202)[0]) > 0                           # hand-overs that did not come: the fix-up launch had rows to finish
        out.append(([e[b, :ec[b]].copy() for b in range(B)], [hashlib.sha256(f[b, :fc[b]].tobytes()).digest() for b in range(B)]))
        eng.close()
    assert out[0][1] == out[1][1]
    want = [digest("dmr", bytes(16), out[0][0][u])[0] for u in range(U)]
    assert sum(len(w) for w in want) > U
    for b in range(B):
        assert out[0][0][b].tobytes() == out[0][0][b % U].tobytes()
        assert out[1][0][b].tobytes() == want[b % U].tobytes(), b


# ------------------------------------------------------------------ 9. the monitor, and the packed read-out of a flagged engine
# (dh_monitor_config keeps its size -- tests/test_monitor_close.py pins it --, so the C monitor and DeviceMonitor have no field for the
# flag: the monitor that takes it is api.Monitor, and the pack is held to a flagged engine through dh_outpack_append.)
from test_scan import rows7      # noqa: F401,E402  (fixture)


def test_monitor(ctx, rows7):
    from test_monitor import PUSH, WANT, chunks, drive, outputs, yardstick
    mon = api.Monitor(7, PUSH, ctx=ctx, depth=96000, call_digest=True)
    segs, _ = drive(mon, [(c, None) for c in chunks(rows7)])
    assert mon.assigned == WANT
    for b, proto in enumerate(WANT[:5]):
        assert len(segs[b]) == 1
        f, e = outputs(segs[b][0])
        wf, we = yardstick(ctx, proto, np.concatenate(segs[b][0]["fed"]))
        assert f.tobytes() == wf.tobytes()
        if proto not in LEN:                                               # D-Star, POCSAG: raw
            assert e.tobytes() == we.tobytes()
            continue
        want, rec = digest(proto, bytes(LEN[proto]), we)
        same(e, want, "monitor channel %d (%s)" % (b, proto))
        # every event of a block is a CALL or a pass-through event; the last CALL names the ids that were sent
        assert all(t == _capi.EV_CALL or (proto, t) in (("dmr", 4), ("ysf", 18), ("ysf", 19)) for t in e["type"])
        last = api.parse_call(proto, e[e["type"] == _capi.EV_CALL][-1])
        named = [api.parse_call(proto, c) for c in e[e["type"] == _capi.EV_CALL]]
        if proto == "dmr":
            sent = [api.parse_lc(r["payload"]) for r in we if r["type"] == 4 and r["len"] >= 9 and (r["payload"][0] & 0x3F) in (0, 3)]
            assert sent and {(lc["source"], lc["target"]) for lc in sent} == {(s["source"], s["target"]) for c in named for s in c["slots"] if s and s["source"]}
            assert last["slots"] == api.parse_call("dmr", dict(type=_capi.EV_CALL, len=16, a=0, payload=np.frombuffer(rec + bytes(8), np.uint8)))["slots"]
        elif proto == "nxdn":
            sent = [(int(r["payload"][3]) << 8 | int(r["payload"][4]), int(r["payload"][5]) << 8 | int(r["payload"][6])) for r in we if r["type"] == 34 and (r["payload"][0] & 0x3F) == 1]
            assert sent and set(map(tuple, sent)) == {(c["source"], c["destination"]) for c in named if c["source"]}
        else:
            assert any(c["mode"] == "DN" and c["source"] and c["target"] for c in named)
    mon.close()


def test_outpack_sees_the_digested_rows(ctx):
    rows = dmr_rows()[:4]
    raw, _ = raw_run(ctx, "dmr")
    pack = api.OutPack(16, 4096, 1 << 16, ctx=ctx)
    with SymbolRun(ctx, "dmr", rows, None, call_digest=True) as r:
        for _ in r:
            pack.append(r.eng)
        blocks = pack.blocks()
    pack.close()
    assert [blk["channel"] for blk in blocks] == list(range(len(rows)))
    for b, blk in enumerate(blocks):
        same(blk["events"], digest("dmr", bytes(16), raw[b])[0], "pack entry %d" % b)
        assert blk["frames"].tobytes() == r.frames[b].tobytes()


# ------------------------------------------------------------------ 10. the existing checker
@pytest.mark.parametrize("proto", ["dmr", "nxdn"])
def test_final_record_against_the_meta_lines(ctx, proto):
    """the numeric fields of the last line oracle/meta.py prints per channel (and slot) equal the final record"""
    from oracle import meta
    raw, _ = raw_run(ctx, proto)
    _, _, rec = run(ctx, proto, ROWS[proto](), call_digest=True)
    checked = 0
    for b, events in enumerate(raw):
        lines = meta.DmrLines() if proto == "dmr" else meta.NxdnLines()
        for e in events:
            lines.consume(e)
        fields = [dict(kv.split(b":", 1) for kv in line.split(b";")) for line in lines.lines]
        for s in range(2 if proto == "dmr" else 1):
            mine = [f for f in fields if proto != "dmr" or f[b"slot"] == b"%d" % s]
            if not mine:
                continue
            r = rec[b][8 * s:8 * s + 8]
            first, second = ("source", "target") if proto == "dmr" else ("source", "destination")
            got = {first: int.from_bytes(r[2:5] if proto == "dmr" else r[2:4], "big"), second: int.from_bytes(r[5:8] if proto == "dmr" else r[4:6], "big")}
            assert got == {k: int(mine[-1].get(k.encode(), b"0")) for k in got}, (proto, b, s, mine[-1])
            checked += 1
    assert checked >= 8
