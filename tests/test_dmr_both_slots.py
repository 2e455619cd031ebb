"""DH_FLAG_DMR_BOTH_SLOTS / Engine(dmr_both_slots=True): both timeslots of a DMR channel leave the decoder as 28-byte slot-tagged
records (include/digiham_amd.h, "DMR: both timeslots").

The yardstick is the reference-shaped oracle decoder through its slot filter: the payloads tagged s, in order, are the oracle's
output on the same input at slot filter f & (s + 1); the events are the oracle's at any filter; the symbols are untouched.  Every engine
case runs on the CPU wave emulation and on the device.  Oracle outputs are computed once per input and shared."""
import ctypes as C

import numpy as np
import pytest

from common import assert_matches_oracle, make_channels, run_engine
from dec_harness import SymbolRun
from digiham_amd import _capi, api, synth
from test_monitor import PUSH, WANT, check, chunks, drive
from test_monitor_device import same_blocks
from test_scan import N_SAMPLES, rows7      # noqa: F401  (fixture)

SEEDS = (41, 43, 45, 47, 49, 53)        # 45: idle bursts on slot 1, the others calls on both slots
TWO = [s != 45 for s in SEEDS]
NB = 150
REC = 28
_SHARED = {}


def shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def streams():
    def make():
        rows = [synth.dmr_stream(seed, NB, two_slots=two) for seed, two in zip(SEEDS, TWO)]
        n = min(len(r) for r in rows)
        a = np.stack([r[:n] for r in rows])
        a.setflags(write=False)
        return a
    return shared("streams", make)


def oracle_run(oracle, row, f):
    d = oracle.Decoder("dmr")
    d.set_slot_filter(f)
    o, ev = d.process(row)
    return o.tobytes(), ev.tobytes()


def wanted(oracle, key, syms):
    """per channel {filter: (frame bytes, event bytes)} for filters 0..3, once per input"""
    return shared(("want", key), lambda: [{f: oracle_run(oracle, row, f) for f in range(4)} for row in syms])


def cuts_of(n, step):
    step = n if step is None else step
    return [step] * -(-n // step)


class Run:
    """a decoder-only DMR engine fed syms[B][n] in pushes of cuts[0], cuts[1], ... symbols: per channel the frames of every push, the
    events, and the pass B counters at the end.  scalar: pass B burst after burst (True) or lane-parallel where a chunk allows it
    (False); None leaves DH_DMR_SCALAR_PASS_B as the process has it.  before_push(eng, k, lo) runs in front of push k."""

    def __init__(self, ctx, syms, cuts, both=True, scalar=None, before_push=None, max_syms=None, **kw):
        env = None if scalar is None else {"DH_DMR_SCALAR_PASS_B": "1" if scalar else None}
        with SymbolRun(ctx, "dmr", syms, cuts, capacity=max_syms or max(cuts), env=env, dmr_both_slots=both, **kw) as run:
            self.stride = run.eng._view("frames")[1]
            if before_push is not None:
                before_push(run.eng, 0, 0)
            for k in run:
                if before_push is not None and k + 1 < len(run.plan):
                    before_push(run.eng, k + 1, run.plan[k + 1][0])
            self.lanes, self.scalar = (a.astype(np.int64) for a in run.eng.dmr_pass_b_stats())
            self.active = run.eng.debug_header(100 + 8).astype(np.int32)       # DS_ACTIVE_SLOT
            self.phase = run.eng.debug_header(100 + 0)
        self.pushes, self.events = run.frames_by_push, run.events_by_push
        self.frames = [f.tobytes() for f in run.frames]
        self.ev = [e.tobytes() for e in run.events]


def split(frame_bytes):
    s0, s1 = api.dmr_split_slots(np.frombuffer(frame_bytes, np.uint8))
    assert s0.dtype == np.uint8 and s1.dtype == np.uint8
    return s0.tobytes(), s1.tobytes()


def assert_both(run, want, f=3, what=""):
    for b, w in enumerate(want):
        s0, s1 = split(run.frames[b])
        assert s0 == w[f & 1][0], (what, b, "slot 0 payloads differ from the oracle's at filter %d" % (f & 1))
        assert s1 == w[f & 2][0], (what, b, "slot 1 payloads differ from the oracle's at filter %d" % (f & 2))
        assert run.ev[b] == w[3][1], (what, b, "events differ from the oracle's")


# ------------------------------------------------------------------ 1. decoder-only engines
def test_inputs_overlap(oracle):
    """the streams hold what the mode is for: voice on both slots at the same time.  n(filter 1) + n(filter 2) - n(filter 3) payloads
    are the ones the one-pipe decoder drops; events never depend on the filter."""
    want = wanted(oracle, "streams", streams())
    dropped = []
    for b, w in enumerate(want):
        n = {f: len(w[f][0]) // 27 for f in range(4)}
        assert all(len(w[f][0]) % 27 == 0 for f in range(4)) and n[0] == 0
        assert len({w[f][1] for f in range(4)}) == 1
        dropped.append(n[1] + n[2] - n[3])
        if TWO[b]:
            assert dropped[-1] >= 30, (SEEDS[b], n)
        else:
            assert n[2] == 0 and dropped[-1] == 0
    print("payloads the one-pipe decoder drops:", dict(zip(SEEDS, dropped)))
    assert dropped[0] == 47 and dropped[1] == 53 and dropped[3] == 49


@pytest.mark.parametrize("step", [None, 1000, 150, 9300])
def test_decoder_only(ctx, oracle, step):
    syms = streams()
    want = wanted(oracle, "streams", syms)
    run = Run(ctx, syms, cuts_of(syms.shape[1], step))
    assert_both(run, want, 3, step)
    for b in range(len(SEEDS)):
        assert all(len(p) % REC == 0 for p in run.pushes[b])
        tags = np.frombuffer(run.frames[b], np.uint8)[REC - 1::REC]
        assert set(tags.tolist()) == ({0, 1} if TWO[b] else {0})
    assert (run.phase == 1).all() and (run.active == -1).all()          # DS_ACTIVE_SLOT is never claimed
    one = shared(("one push", id(ctx)), lambda: Run(ctx, syms, [syms.shape[1]]).frames)
    assert run.frames == one                                              # the bytes do not depend on the cuts


# ------------------------------------------------------------------ 2. order
def test_order(ctx, oracle):
    syms = streams()
    B, n = syms.shape
    run = Run(ctx, syms, cuts_of(n, 144))
    pair = [[oracle.Decoder("dmr"), oracle.Decoder("dmr")] for _ in range(B)]
    for b in range(B):
        pair[b][0].set_slot_filter(1); pair[b][1].set_slot_filter(2)
    seen = 0
    for k, lo in enumerate(range(0, n, 144)):
        for b in range(B):
            o = [d.process(syms[b, lo:lo + 144])[0].tobytes() for d in pair[b]]
            got = run.pushes[b][k].tobytes()
            assert len(got) in (0, REC), (b, k)                           # one burst per push at the most
            assert not (o[0] and o[1])
            want = o[0] + b"\x00" if o[0] else o[1] + b"\x01" if o[1] else b""
            assert got == want, (b, k)
            seen += len(got) // REC
    assert seen > 300
    one = shared(("one push", id(ctx)), lambda: Run(ctx, syms, [n]).frames)
    assert run.frames == one


# ------------------------------------------------------------------ 3. the slot filter in the mode
@pytest.mark.parametrize("f", [0, 1, 2, 3])
def test_filter_at_create(ctx, oracle, f):
    syms = streams()
    want = wanted(oracle, "streams", syms)
    run = Run(ctx, syms, [syms.shape[1]], slot_filter=f)
    assert_both(run, want, f, f)
    for b in range(len(SEEDS)):
        tags = set(np.frombuffer(run.frames[b], np.uint8)[REC - 1::REC].tolist())
        assert tags <= set(([], [0], [1], [0, 1])[f])
        if f == 0:
            assert run.frames[b] == b""
        if f == 1:
            assert run.frames[b] and split(run.frames[b])[0] == want[b][1][0]
    assert (run.active == -1).all()


def test_filter_calls_and_reset(ctx, oracle):
    """set_slot_filter and set_slot_filter_channel between pushes of 1 000 symbols, and a masked reset of one channel, against an
    oracle pair per channel driven the same way: decoder s of the pair gets f & (s + 1).  The reset channel starts again from a
    fresh pair at the engine's filter, and goes on emitting both slots: the mode is still on."""
    syms = streams()
    B, n = syms.shape
    step, RESET_AT, CH = 1000, 9, 1
    plan = {2: ("all", 1), 4: ("one", 3, 2), 5: ("one", 0, 0), 7: ("all", 2), 8: ("one", 1, 3), 12: ("all", 3), 15: ("one", 5, 1), 17: ("one", 5, 3)}
    engine_filter = [3]

    def set_pair(pair, b, f):
        for s in range(2):
            pair[b][s].set_slot_filter(f & (s + 1))

    def apply(k, eng=None, pair=None):
        """what happens in front of push k, to the engine or to the oracle pairs"""
        if k == RESET_AT:
            if eng is not None:
                flags = np.zeros(B, np.uint8)
                flags[CH] = 1
                eng.reset_channels(flags)
            else:
                pair[CH] = [oracle.Decoder("dmr"), oracle.Decoder("dmr")]
                set_pair(pair, CH, engine_filter[0])                      # a reset channel starts at the engine's filter
        if k in plan and plan[k][0] == "all":
            if eng is not None:
                eng.set_slot_filter(plan[k][1])
            else:
                engine_filter[0] = plan[k][1]
                for b in range(B):
                    set_pair(pair, b, plan[k][1])
        elif k in plan:
            if eng is not None:
                eng.set_slot_filter_channel(plan[k][1], plan[k][2])
            else:
                set_pair(pair, plan[k][1], plan[k][2])

    run = Run(ctx, syms, cuts_of(n, step), before_push=lambda eng, k, lo: apply(k, eng=eng))
    pair = [[oracle.Decoder("dmr"), oracle.Decoder("dmr")] for _ in range(B)]
    for b in range(B):
        set_pair(pair, b, 3)
    after_reset = [b"", b""]
    tags_seen = set()
    for k, lo in enumerate(range(0, n, step)):
        apply(k, pair=pair)
        for b in range(B):
            o = [d.process(syms[b, lo:lo + step]) for d in pair[b]]
            s0, s1 = split(run.pushes[b][k].tobytes())
            assert (s0, s1) == (o[0][0].tobytes(), o[1][0].tobytes()), (b, k)
            assert run.events[b][k].tobytes() == o[0][1].tobytes() == o[1][1].tobytes(), (b, k)
            tags_seen |= {(b, 0)} if s0 else set()
            tags_seen |= {(b, 1)} if s1 else set()
            if b == CH and k > RESET_AT + 3:              # (engine filter 3 again from push 12 on)
                after_reset[0] += s0; after_reset[1] += s1
    assert after_reset[0] and after_reset[1], "no voice on both slots behind the reset"
    assert len(tags_seen) >= 2 * sum(TWO)


# ------------------------------------------------------------------ 4. both passes
def test_both_passes(ctx, oracle):
    syms = streams()
    want = wanted(oracle, "streams", syms)
    cuts = cuts_of(syms.shape[1], 9300)
    run = Run(ctx, syms, cuts, scalar=False)
    twin = Run(ctx, syms, cuts, scalar=True)
    assert_both(run, want, 3, "lanes")
    assert run.frames == twin.frames and run.ev == twin.ev
    assert (twin.lanes == 0).all() and (twin.scalar > 0).all()
    assert (run.lanes + run.scalar == twin.scalar).all()                  # the same chunks either way
    # healthy two-slot traffic takes the lane pass: only the chunk behind the sync search (slot unknown) goes burst by burst
    assert (run.lanes[np.array(TWO)] > 0).all() and (run.scalar == 1).all(), (run.lanes, run.scalar)


def sync_loss_streams():
    """tests/test_chain.py::test_dmr_sync_loss_at_every_burst_index: channel c loses its signal from burst c on for 8 to 20 bursts of
    random dibits, scattered wrong dibits everywhere"""
    def make():
        rng = np.random.default_rng(2024)
        B, nb = 72, 150
        rows = []
        for c in range(B):
            s = synth.dmr_stream(300 + c, nb, two_slots=bool(c & 1), lead_in=int(rng.integers(0, 50))).copy()
            lead = len(s) - 144 * nb
            gap = int(rng.integers(8, 21))
            s[lead + 144 * c: lead + 144 * (c + gap)] = rng.integers(0, 4, 144 * gap)
            flips = rng.integers(0, len(s), len(s) // 150)
            s[flips] ^= rng.integers(1, 4, len(flips)).astype(np.uint8)
            rows.append(s)
        n = min(len(r) for r in rows)
        a = np.stack([r[:n] for r in rows])
        a.setflags(write=False)
        return a
    return shared("sync loss", make)


@pytest.mark.parametrize("step", [None, 1000])
def test_sync_loss_at_every_burst_index(ctx, oracle, step):
    syms = sync_loss_streams()
    want = wanted(oracle, "sync loss", syms)
    run = Run(ctx, syms, cuts_of(syms.shape[1], step))
    assert_both(run, want, 3, step)
    assert any(3 in set(np.frombuffer(w[3][1], api.EVENT_DTYPE)["type"].tolist()) for w in want)       # META_RESETs happened
    assert run.lanes.sum() > 0 and (run.scalar > 1).any()                 # declined and irregular chunks, and lane-parallel ones
    assert sum(len(w[1][0]) + len(w[2][0]) - len(w[3][0]) for w in want) > 27 * 100


# ------------------------------------------------------------------ 5. the full chain
def chain_inputs(oracle):
    def make():
        x = make_channels("dmr", [41, 43, 45, 47], 40)
        x.setflags(write=False)
        return x, {f: oracle.chain(x, proto=1, slot_filter=f) for f in (1, 2, 3)}
    return shared("chain", make)


@pytest.mark.parametrize("split_stages", [False, True])
@pytest.mark.parametrize("push", [4800, 10007])
def test_full_chain(ctx, oracle, push, split_stages):
    x, ref = chain_inputs(oracle)
    res = run_engine(ctx, x, "dmr", [push], dmr_both_slots=True, split_stages=split_stages)
    dropped = 0
    for b in range(x.shape[0]):
        s0, s1 = split(res["frames"][b].tobytes())
        out = {f: ref[f]["out"][b, :ref[f]["out_count"][b]].tobytes() for f in (1, 2, 3)}
        assert s0 == out[1] and s1 == out[2], b
        dropped += (len(out[1]) + len(out[2]) - len(out[3])) // 27
    print("payloads the one-pipe decoder drops on the chain's rows:", dropped)
    assert dropped > 0                                                    # the chain's streams overlap as well
    res["frames"] = [None] * x.shape[0]                                   # events and symbols: those at filter 3
    assert_matches_oracle(res, ref[3], x.shape[0], "both slots")
    for b in range(x.shape[0]):
        re = ref[3]["events"][b, :ref[3]["event_count"][b]]
        assert res["events"][b].tobytes() == re.tobytes(), b


# ------------------------------------------------------------------ 6. capacity
def busy_stream():
    """one long call on either slot, interleaved burst by burst: everything but the two LC headers and the two terminators is voice"""
    def make():
        rng = np.random.default_rng(77)
        q = [synth.dmr_call(rng, slot, dst=100 + slot, src=2000 + slot, n_superframes=17) for slot in (0, 1)]
        assert len(q[0]) == len(q[1]) == 104
        out = list(rng.integers(0, 4, 37))
        for i in range(208):
            out += q[i & 1][i >> 1]
        a = np.array(out, np.uint8)[None, :]
        a.setflags(write=False)
        return a
    return shared("busy", make)


def test_capacity(ctx, oracle):
    syms = busy_stream()
    want = wanted(oracle, "busy", syms)
    max_syms = 9300                                                       # 64 bursts and a little
    run = Run(ctx, syms, cuts_of(syms.shape[1], max_syms), max_syms=max_syms)          # sync() in Run raises on the overflow flag
    assert_both(run, want, 3, "busy")
    carry = 512                                                           # DH_SYM_CARRY_MAX: symbols a push may find left over
    assert run.stride >= REC * ((carry + max_syms) // 144 + 1) and run.stride % 64 == 0
    n = [len(p) // REC for p in run.pushes[0]]
    assert n[0] >= 60 and n[1] >= 63 and n[2] >= 63, n                    # the full pushes: (nearly) every burst position a record


# ------------------------------------------------------------------ 7. errors and the default
def test_errors_and_default(ctx, oracle):
    for kw in (dict(proto="ysf"), dict(proto="none"), dict(proto="nxdn", rrc="narrow", sps=20), dict(proto="scan")):
        with pytest.raises(_capi.DhError) as e:
            api.Engine(2, 4800, ctx=ctx, dmr_both_slots=True, **kw)
        assert e.value.code == _capi.DH_EINVAL, kw
    assert _capi.FLAG_DMR_BOTH_SLOTS == 0x400 and _capi.DMR_SLOT_RECORD_BYTES == REC
    # without the flag: the one-pipe decoder, records of 27 untagged bytes
    syms = streams()
    want = wanted(oracle, "streams", syms)
    run = Run(ctx, syms, cuts_of(syms.shape[1], 9300), both=False)
    for b, w in enumerate(want):
        assert run.frames[b] == w[3][0] and len(run.frames[b]) % 27 == 0 and run.ev[b] == w[3][1], b
    # only bits 0 and 1 of a caller's filter count: neither the configuration's value nor a filter call can switch the mode on
    high = Run(ctx, syms, cuts_of(syms.shape[1], 9300), both=False, slot_filter=7,
               before_push=lambda eng, k, lo: (eng.set_slot_filter(0xFF), eng.set_slot_filter_channel(2, 7)) if k == 1 else None)
    assert high.frames == run.frames and high.ev == run.ev
    with pytest.raises(ValueError):
        api.dmr_split_slots(np.zeros(27, np.uint8))
    bad = np.zeros(2 * REC, np.uint8)
    bad[2 * REC - 1] = 2
    with pytest.raises(ValueError):
        api.dmr_split_slots(bad)
    s0, s1 = api.dmr_split_slots(np.zeros(0, np.uint8))
    assert len(s0) == 0 and len(s1) == 0
    ok = np.arange(3 * REC, dtype=np.uint8)
    ok[REC - 1::REC] = (1, 0, 1)
    s0, s1 = api.dmr_split_slots(ok)
    assert s0.tobytes() == ok[REC:2 * REC - 1].tobytes() and s1.tobytes() == ok[:REC - 1].tobytes() + ok[2 * REC:3 * REC - 1].tobytes()


# ------------------------------------------------------------------ 8. read-out and monitors
def test_outpack(ctx):
    syms = streams()
    B = syms.shape[0]
    pack = api.OutPack(4 * B, 4096, 1 << 16, ctx=ctx)
    want = []
    with SymbolRun(ctx, "dmr", syms[:, :10000], 5000, capacity=5000, dmr_both_slots=True) as run:
        for k in run:
            pack.append(run.eng, user=k)
            got = [(b, k, run.frames_by_push[b][k].tobytes(), run.events_by_push[b][k].tobytes()) for b in range(B)]
            want += [g for g in got if g[2] or g[3]]
        header, entries, events, frames = pack.read()
    assert pack.rc == 0 and header["dropped"] == 0 and len(entries) == len(want) >= B
    assert (entries["n_frame_bytes"] % REC == 0).all() and entries["n_frame_bytes"].sum() > 20 * REC
    got = [(blk["channel"], blk["user"], blk["frames"].tobytes(), blk["events"].tobytes())
           for blk in api._packed_blocks(entries, events, frames, "user", "tag")]
    assert got == want
    pack.close()


class Three:
    """Monitor, DeviceMonitor and DeviceMonitor(packed=True) fed the same rounds: equal blocks, equal state"""

    def __init__(self, n_channels, max_samples, ctx, **kw):
        self.mons = [api.Monitor(n_channels, max_samples, ctx=ctx, **kw), api.DeviceMonitor(n_channels, max_samples, ctx=ctx, **kw),
                     api.DeviceMonitor(n_channels, max_samples, ctx=ctx, packed=True, **kw)]
        self.B, self.max_samples, self.ctx = n_channels, max_samples, ctx

    assigned = property(lambda self: self.mons[1].assigned)
    start = property(lambda self: self.mons[1].start)

    def push(self, rows, n=None, counts=None):
        if isinstance(rows, np.ndarray) and rows.shape[1]:
            rows = self.ctx.mem.from_numpy(np.ascontiguousarray(rows, np.float32))
        got = [m.push(rows, n=n, counts=counts) for m in self.mons]
        same_blocks(got[1], got[0])
        same_blocks(got[2], got[0])
        assert self.mons[0].assigned == self.mons[1].assigned == self.mons[2].assigned
        assert self.mons[0].start == self.mons[1].start == self.mons[2].start
        return got[2]

    def close(self):
        for m in self.mons:
            m.close()


def test_monitors(ctx, rows7):
    mon = Three(7, PUSH, ctx, depth=96000, dmr_both_slots=True)
    segs, trace = drive(mon, [(c, None) for c in chunks(rows7)])
    assert mon.assigned == WANT and mon.start == [0] * 5 + [None] * 2
    for b in range(1, 5):                                                 # the other protocols: as without the mode
        assert len(segs[b]) == 1 and segs[b][0]["proto"] == WANT[b]
        f, e = check(ctx, segs[b][0])
        assert len(e)
    assert not segs[5] and not segs[6]
    # the DMR row against a fresh both-slots engine fed the same samples in one push
    seg = segs[0][0]
    fed = np.concatenate(seg["fed"])
    assert seg["proto"] == "dmr" and len(fed) == N_SAMPLES
    eng = api.Engine(1, len(fed), proto="dmr", ctx=ctx, dmr_both_slots=True, **api.SCAN_FRONTS["wide10"])
    eng.push(np.ascontiguousarray(fed[None, :], np.float32))
    (f, fc), (e, ec) = eng.frames(), eng.events()
    eng.close()
    assert all(len(blk) % REC == 0 for blk in seg["frames"])
    got = np.concatenate(seg["frames"])
    assert split(got.tobytes()) == split(f[0, :fc[0]].tobytes()) and got.tobytes() == f[0, :fc[0]].tobytes()
    assert np.concatenate(seg["events"]).tobytes() == e[0, :ec[0]].tobytes()
    s0, s1 = split(got.tobytes())
    assert s0 and s1, "the scene's DMR row carries voice on one slot only"
    mon.close()


def test_monitor_config_of_the_old_size(ctx, rows7):
    """dh_monitor_config as it was before dmr_both_slots: the field is not read, the DMR engine is the one-pipe decoder"""
    lib, mem = ctx.lib, ctx.mem
    protos = 1 << _capi.PROTO["dmr"]
    old = _capi.MONITOR_CONFIG_V1_SIZE
    assert old == 48 and C.sizeof(_capi.MonitorConfig) > old

    def create(struct_size, both):
        cfg = _capi.MonitorConfig(struct_size, getattr(mem, "index", 0), 2, PUSH, 24000, 480, 2, 4, protos, mem.stream(), both)
        h = C.c_void_p()
        return lib.dh_monitor_create(C.byref(cfg), C.byref(h)), h

    def dmr_stride(h):
        e = api.Engine._borrowed(ctx, lib.dh_monitor_engine(h, _capi.PROTO["dmr"]), 2, PUSH)
        return e._view("frames")[1]

    strides = {}
    for name, size, both in (("old, field set", old, 1), ("new, off", C.sizeof(_capi.MonitorConfig), 0), ("new, on", C.sizeof(_capi.MonitorConfig), 1)):
        rc, h = create(size, both)
        assert rc == 0, name
        strides[name] = dmr_stride(h)
        lib.dh_monitor_destroy(h)
    assert strides["old, field set"] == strides["new, off"] <= strides["new, on"]          # (rows of 4 800 samples: 8 x 27 and 8 x 28 both round up to 256)
    for size in (old - 1, old + 4, C.sizeof(_capi.MonitorConfig) - 1):
        rc, h = create(size, 0)
        assert rc == _capi.DH_EINVAL and not h.value, size
    # and what comes out of it: the blocks of a monitor without the mode
    x = np.ascontiguousarray(rows7[[0, 6], :6 * PUSH])
    rc, h = create(old, 1)
    assert rc == 0
    plain = api.DeviceMonitor(2, PUSH, depth=24000, protos=("dmr",), ctx=ctx)
    pack = api.OutPack(64, 1 << 12, 1 << 18, ctx=ctx)
    n_bytes = 0
    for c in chunks(x):
        rows = mem.from_numpy(c)
        want = plain.push(rows)
        pack.clear()
        assert lib.dh_monitor_push_packed(h, mem.ptr(rows), c.shape[1], c.shape[1], None, pack._h) == 0
        header, entries, events, frames = pack.read()
        got = api._by_position(api._packed_blocks(entries, events, frames, "proto", "first_sample", api.PROTO_NAMES))
        same_blocks(got, want)
        n_bytes += sum(len(blk["frames"]) for blk in got)
        assert all(len(blk["frames"]) % 27 == 0 for blk in got)
    assert n_bytes > 0
    lib.dh_monitor_destroy(h)
    plain.close()
    pack.close()
