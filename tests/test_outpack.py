"""dh_outpack / api.OutPack: the packed read-out (include/digiham_amd.h, "Packed read-out").

The yardstick is always the engine's own dense read of the SAME push -- Engine.frames() / Engine.events() -- and the
specification's arithmetic on its counts: the pack must reproduce the rows byte for byte, in append order then channel
order, at the running offsets.  Nothing is asserted about what a decoder emits, except the stated sanity condition that at
least three channels produced output and at least three produced none.  Engines are decoder-only (push_symbols with
per-channel counts) wherever the test is not about the stages in front of the decoder."""
import ctypes as C

import numpy as np
import pytest

from digiham_amd import _capi, api, synth

SCAN_PASS = 256                     # channels one pass of k_outpack_scan covers (DH_OP_LANES, outpack_core.hpp): 4 wavefronts of 64
N_SYMS = 5000
# dibits per busy channel, taken in turn: 244 leaves events and no frame bytes, 4900 sixteen 27-byte frames (a multiple of 16)
COUNTS = (700, 244, 4900, 1500, 2200, 3000, 1000)
_SHARED = {}


def dibits(proto):
    if proto not in _SHARED:
        s = synth.dmr_stream(1, 40) if proto == "dmr" else synth.ysf_stream(2, 12)
        _SHARED[proto] = np.asarray(s, np.uint8)
        _SHARED[proto].setflags(write=False)
    return _SHARED[proto]


def seams(B):
    """the first and the last channel, both sides of every wavefront boundary and of every pass boundary"""
    at = {0, B - 1}
    for edge in range(64, B, 64):
        at |= {edge - 1, edge}
    return sorted(b for b in at if 0 <= b < B)


class Pushed:
    """a decoder-only engine, one push into it, and the dense read of that push"""

    def __init__(self, ctx, B, busy, proto="dmr", counts=COUNTS, **kw):
        self.ctx, self.B = ctx, B
        self.eng = api.Engine(B, N_SYMS, rrc="none", demod="none", proto=proto, ctx=ctx, **kw)
        self.pos = np.zeros(B, np.int64)
        self.busy, self.counts, self.src = list(busy), counts, dibits(proto)
        self.push()

    def push(self):
        rows, cnt = np.zeros((self.B, N_SYMS), np.uint8), np.zeros(self.B, np.uint32)
        for j, b in enumerate(self.busy):
            n = min(self.counts[j % len(self.counts)], len(self.src) - int(self.pos[b]))
            rows[b, :n] = self.src[self.pos[b]:self.pos[b] + n]
            cnt[b] = n
            self.pos[b] += n
        self.eng.push_symbols(rows, cnt)
        self.frames, self.fc = self.eng.frames()
        if self.eng_has_events():
            self.events, self.ec = self.eng.events()
        else:
            self.events, self.ec = np.zeros((self.B, 0), api.EVENT_DTYPE), np.zeros(self.B, np.uint32)
        return self

    def eng_has_events(self):
        p, stride, cnt = C.c_void_p(), C.c_size_t(), C.c_void_p()
        return self.ctx.lib.dh_engine_events(self.eng._h, C.byref(p), C.byref(stride), C.byref(cnt)) == 0

    def candidates(self, mask=None):
        return [b for b in range(self.B) if (mask is None or mask[b]) and (self.fc[b] or self.ec[b])]

    def want(self, mask=None, tag=None, tag_add=0, user=0):
        """(channel, user, tag, frame bytes, event bytes) per candidate, in channel order"""
        return [(b, user, ((int(tag[b]) if tag is not None else 0) + tag_add) % (1 << 64), self.frames[b, :self.fc[b]].tobytes(),
                 self.events[b, :self.ec[b]].tobytes()) for b in self.candidates(mask)]

    def sane(self):
        out = (self.fc != 0) | (self.ec != 0)
        assert out.sum() >= 3 and (~out).sum() >= 3, "the push does not meet the test's precondition"

    def close(self):
        self.eng.close()


def pad16(n):
    return (n + 15) // 16 * 16


def totals(want):
    return len(want), sum(len(w[4]) // 32 for w in want), sum(pad16(len(w[3])) for w in want)


def device_areas(ctx, pack):
    p = [C.c_void_p() for _ in range(4)]
    assert ctx.lib.dh_outpack_device(pack._h, *[C.byref(x) for x in p]) == 0
    return p[1:], (32 * pack.max_entries, 32 * pack.max_events, pack.max_frame_bytes)


def fill_areas(ctx, pack, byte=0xA5):
    ptrs, sizes = device_areas(ctx, pack)
    for p, n in zip(ptrs, sizes):
        a = np.full(n, byte, np.uint8)
        assert ctx.lib.dh_copy_to_device(p, a.ctypes.data_as(C.c_void_p), n) == 0


def dump_areas(ctx, pack):
    ptrs, sizes = device_areas(ctx, pack)
    out = []
    for p, n in zip(ptrs, sizes):
        a = np.zeros(n, np.uint8)
        assert ctx.lib.dh_copy_to_host(a.ctypes.data_as(C.c_void_p), p, n) == 0
        out.append(a)
    return out


def check_pack(got, want, dropped=0, appends=None):
    """got: OutPack.read(); want: the kept (channel, user, tag, frames, events) in order"""
    header, entries, events, frames = got
    E, V, F = totals(want)
    assert (header["n_entries"], header["n_events"], header["frame_bytes"], header["dropped"]) == (E, V, F, dropped)
    if appends is not None:
        assert header["appends"] == appends
    assert len(entries) == E and len(events) == V and len(frames) == F
    v = f = 0
    for en, (b, user, tag, wf, we) in zip(entries, want):
        assert (int(en["channel"]), int(en["user"]), int(en["tag"])) == (b, user, tag)
        assert (int(en["n_frame_bytes"]), int(en["n_events"])) == (len(wf), len(we) // 32)
        assert (int(en["frame_offset16"]), int(en["event_index"])) == (f // 16, v), b         # the running sums
        assert frames[f:f + len(wf)].tobytes() == wf, b
        assert not frames[f + len(wf):f + pad16(len(wf))].any(), b                            # pad bytes
        assert events[v:v + len(we) // 32].tobytes() == we, b
        v += len(we) // 32
        f += pad16(len(wf))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 70, SCAN_PASS + 1])
def test_equality(ctx, B):
    """one append, no mask: busy channels at the first and the last channel and on both sides of every wavefront and pass
    boundary, everything else silent.  (Three channels with output and three without need B >= 70: the sanity condition is
    asserted there.)"""
    busy = seams(B)
    p = Pushed(ctx, B, busy)
    if B >= 70:
        p.sane()
    else:
        assert p.candidates() and (B < 3 or len(p.candidates()) < B)
    want = p.want(user=7)
    assert [w[0] for w in want] == sorted(w[0] for w in want)
    E, V, F = totals(want)
    pack = api.OutPack(E + 3, V + 5, F + 64, ctx=ctx)
    fill_areas(ctx, pack)
    pack.append(p.eng, user=7)
    got = pack.read()
    check_pack(got, want, appends=1)
    assert pack.rc == 0 and list(got[1]["channel"]) == sorted(got[1]["channel"])
    entries, events, frames = dump_areas(ctx, pack)
    assert (entries[32 * E:] == 0xA5).all() and (events[32 * V:] == 0xA5).all() and (frames[F:] == 0xA5).all()       # nothing beyond the totals
    assert [(blk["channel"], blk["user"], blk["tag"], blk["frames"].tobytes(), blk["events"].tobytes()) for blk in pack.blocks()] == want
    pack.close()
    p.close()


def test_mask_and_tag(ctx):
    B = 70
    busy = seams(B) + [10, 11, 12]
    p = Pushed(ctx, B, busy)
    p.sane()
    cands = p.candidates()
    mask = np.zeros(B, np.uint32)
    mask[cands] = 5
    mask[cands[1]] = 0                                  # a busy channel left out
    mask[[20, 21, 22]] = 1                              # idle ones let in
    assert not p.fc[[20, 21, 22]].any() and not p.ec[[20, 21, 22]].any()
    tag = np.arange(B, dtype=np.uint64) * np.uint64(1000)
    tag[cands[0]] = np.uint64((1 << 64) - 5)            # + 10 wraps
    pack = api.OutPack(B, 4096, 1 << 16, ctx=ctx)
    pack.append(p.eng, mask=mask, tag=tag, tag_add=10, user=0x101)
    want = p.want(mask, tag, 10, 0x101)
    assert want[0][2] == 5 and cands[1] not in [w[0] for w in want] and len(want) == len(cands) - 1
    check_pack(pack.read(), want, appends=1)
    pack.clear()
    pack.append(p.eng, mask=mask, tag=None, tag_add=(1 << 64) - 1, user=9)           # d_tag = NULL
    check_pack(pack.read(), p.want(mask, None, (1 << 64) - 1, 9), appends=1)
    pack.clear()
    pack.append(p.eng, tag=tag, user=3)                                                # d_mask = NULL
    check_pack(pack.read(), p.want(None, tag, 0, 3), appends=1)
    pack.close()
    p.close()


def test_several_appends(ctx):
    dmr = Pushed(ctx, 70, seams(70))
    ysf = Pushed(ctx, 9, [0, 4, 8], proto="ysf", counts=(3000, 1500, 2500))
    dmr.sane()
    ysf.sane()
    pack = api.OutPack(256, 8192, 1 << 17, ctx=ctx)
    fill_areas(ctx, pack)
    pack.append(dmr.eng, user=1)
    want = dmr.want(user=1)
    pack.append(ysf.eng, tag_add=77, user=2 | 1 << 8)
    want += ysf.want(tag_add=77, user=2 | 1 << 8)
    dmr.push()                                          # the engine's rows are overwritten; what the pack took stays
    dmr.sane()
    pack.append(dmr.eng, user=3)
    want += dmr.want(user=3)
    got = pack.read()
    check_pack(got, want, appends=3)
    assert len({w[1] for w in want}) == 3
    before = dump_areas(ctx, pack)
    pack.clear()
    header, entries, events, frames = pack.read()
    assert header == dict(n_entries=0, n_events=0, frame_bytes=0, dropped=0, appends=0) and not len(entries) and not len(events) and not len(frames)
    after = dump_areas(ctx, pack)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))               # clear leaves the areas untouched
    pack.close()
    dmr.close()
    ysf.close()


@pytest.fixture
def capacity_push(ctx):
    p = Pushed(ctx, 70, seams(70) + [30, 31, 40])
    yield p
    p.close()


@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("limit", ["entries", "events", "frames"])
def test_capacity(ctx, capacity_push, limit, which):
    """The pack takes the append T once whole; in a second append of T candidate k is the first not to fit, because the
    capacity named by `limit` ends one entry / one event / one 16-byte piece short of it."""
    p = capacity_push
    p.sane()
    T = p.want(user=1)
    N, V, F = totals(T)
    assert any(not len(w[3]) and len(w[4]) for w in T), "no candidate with fc = 0, ec > 0"
    assert any(len(w[3]) and len(w[3]) % 16 == 0 for w in T), "no candidate whose fc is a multiple of 16"
    k = {"first": 0, "middle": N // 2, "last": N - 1}[which]
    assert len(T[k][3]) and len(T[k][4])                # the candidate that does not fit has frame bytes and events
    n_k, v_k, f_k = totals(T[:k])
    cap = {"entries": (N + n_k, 2 * V, 2 * F),
           "events": (2 * N, V + v_k + len(T[k][4]) // 32 - 1, 2 * F),
           "frames": (2 * N, 2 * V, F + f_k + pad16(len(T[k][3])) - 16)}[limit]
    pack = api.OutPack(*cap, ctx=ctx)
    fill_areas(ctx, pack)
    pack.append(p.eng, user=1)
    check_pack(pack.read(), T, appends=1)
    assert pack.rc == 0
    pack.append(p.eng, user=2)
    kept = T + [(b, 2, t, f, e) for b, _, t, f, e in T[:k]]
    got = pack.read()
    assert pack.rc == _capi.DH_ECAPACITY                # ... and the prefix is delivered
    check_pack(got, kept, dropped=N - k, appends=2)
    E2, V2, F2 = totals(kept)
    entries, events, frames = dump_areas(ctx, pack)
    assert (entries[32 * E2:] == 0xA5).all() and (events[32 * V2:] == 0xA5).all() and (frames[F2:] == 0xA5).all()
    pack.append(p.eng, user=3)                          # a further append: everything is dropped, also what would fit
    got = pack.read()
    assert pack.rc == _capi.DH_ECAPACITY
    check_pack(got, kept, dropped=N - k + N, appends=3)
    pack.clear()
    pack.append(p.eng, user=4)                          # after clear the same append is kept whole
    check_pack(pack.read(), [(b, 4, t, f, e) for b, _, t, f, e in T], appends=1)
    assert pack.rc == 0
    pack.close()


def test_other_engines(ctx):
    """An engine without events, a scan engine, a full chain.  (The sanity condition is on the test as a whole: the full
    chain has three channels.)"""
    with_out = without = 0
    # DH_FLAG_NO_EVENTS: n_events = 0 throughout
    p = Pushed(ctx, 70, seams(70), events=False)
    p.sane()
    assert not p.ec.any()
    pack = api.OutPack(70, 16, 1 << 16, ctx=ctx)
    fill_areas(ctx, pack)
    pack.append(p.eng, user=1)
    got = pack.read()
    check_pack(got, p.want(user=1), appends=1)
    assert got[0]["n_events"] == 0 and not got[1]["n_events"].any() and len(got[1]) >= 3
    assert (dump_areas(ctx, pack)[1] == 0xA5).all()
    with_out += len(got[1]); without += 70 - len(got[1])
    pack.close()
    p.close()

    # a scan engine: every masked channel is a candidate with 144 frame bytes
    s = Pushed(ctx, 70, seams(70), proto="scan")
    mask = np.zeros(70, np.uint32)
    mask[[0, 1, 63, 64, 69]] = 1
    pack = api.OutPack(70, 8192, 1 << 16, ctx=ctx)
    pack.append(s.eng, mask=mask, user=6)
    got = pack.read()
    check_pack(got, s.want(mask, user=6), appends=1)
    assert list(got[1]["channel"]) == [0, 1, 63, 64, 69] and (got[1]["n_frame_bytes"] == 144).all()
    pack.close()
    s.close()

    # a full chain: the append goes out behind a slicer launch
    x = np.zeros((3, 9600), np.float32)
    wave = np.asarray(synth.shape(synth.dmr_stream(31, 12)), np.float32)
    x[0], x[2] = wave[:9600], wave[1200:10800]
    eng = api.Engine(3, 4800, proto="dmr", ctx=ctx, **api.SCAN_FRONTS["wide10"])
    pack = api.OutPack(8, 512, 4096, ctx=ctx)
    want = []
    for k in range(2):
        eng.push(np.ascontiguousarray(x[:, 4800 * k:4800 * (k + 1)]))
        pack.append(eng, tag_add=4800 * k, user=k)
        (f, fc), (e, ec) = eng.frames(), eng.events()
        want += [(b, k, 4800 * k, f[b, :fc[b]].tobytes(), e[b, :ec[b]].tobytes()) for b in range(3) if fc[b] or ec[b]]
    check_pack(pack.read(), want, appends=2)
    assert {w[0] for w in want} == {0, 2} and any(len(w[3]) for w in want)
    with_out += 2; without += 1
    pack.close()
    eng.close()
    assert with_out >= 3 and without >= 3


def test_errors(ctx):
    lib, mem = ctx.lib, ctx.mem
    good = lambda: _capi.OutpackConfig(C.sizeof(_capi.OutpackConfig), getattr(mem, "index", 0), 4, 4, 64, mem.stream())
    h = C.c_void_p()
    for change in (dict(struct_size=C.sizeof(_capi.OutpackConfig) - 1), dict(max_entries=0), dict(max_frame_bytes=24),
                   dict(max_frame_bytes=1 << 36), dict(max_frame_bytes=(1 << 36) - 8)):
        cfg = good()
        for k, v in change.items():
            setattr(cfg, k, v)
        assert lib.dh_outpack_create(C.byref(cfg), C.byref(h)) == _capi.DH_EINVAL, change
        assert not h.value
    cfg = good()
    assert lib.dh_outpack_create(None, C.byref(h)) == _capi.DH_EINVAL and lib.dh_outpack_create(C.byref(cfg), None) == _capi.DH_EINVAL

    p = Pushed(ctx, 8, [0, 3, 7])
    pack = api.OutPack(8, 1024, 4096, ctx=ctx)
    none = api.Engine(8, 480, proto="none", ctx=ctx, **api.SCAN_FRONTS["wide10"])
    hdr, null = _capi.OutpackHeader(), None
    bad = [lib.dh_outpack_clear(null), lib.dh_outpack_append(null, p.eng._h, null, null, 0, 0), lib.dh_outpack_append(pack._h, null, null, null, 0, 0),
           lib.dh_outpack_read(null, C.byref(hdr), null, null, null), lib.dh_outpack_device(null, null, null, null, null),
           lib.dh_outpack_append(pack._h, none._h, null, null, 0, 0)]                  # proto == DH_PROTO_NONE
    assert bad == [_capi.DH_EINVAL] * len(bad)
    # a pack on another stream than the engine's
    torch = getattr(mem, "torch", None)
    side = torch.cuda.Stream(mem.device) if torch is not None else None
    cfg = good()
    cfg.max_entries, cfg.max_events, cfg.max_frame_bytes = 8, 1024, 4096
    cfg.stream = C.c_void_p(side.cuda_stream if side is not None else 64)
    assert lib.dh_outpack_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.dh_outpack_append(h, p.eng._h, null, null, 0, 0) == _capi.DH_EINVAL
    assert lib.dh_outpack_read(h, C.byref(hdr), null, null, null) == 0 and (hdr.n_entries, hdr.appends, hdr.dropped) == (0, 0, 0)
    lib.dh_outpack_destroy(h)
    if torch is None:                                   # ... or on another device (the emulation takes any index)
        cfg.stream, cfg.device = mem.stream(), 1
        assert lib.dh_outpack_create(C.byref(cfg), C.byref(h)) == 0
        assert lib.dh_outpack_append(h, p.eng._h, null, null, 0, 0) == _capi.DH_EINVAL
        lib.dh_outpack_destroy(h)
    # none of them appended anything; a read with every array NULL still tells the totals
    pack.append(p.eng)
    assert lib.dh_outpack_read(pack._h, C.byref(hdr), null, null, null) == 0 and hdr.n_entries == len(p.candidates()) == 3 and hdr.appends == 1
    assert lib.dh_outpack_read(pack._h, null, null, null, null) == 0 and lib.dh_outpack_device(pack._h, null, null, null, null) == 0
    lib.dh_outpack_destroy(null)
    none.close()
    pack.close()
    pack.close()
    p.close()


@pytest.mark.gpu
def test_2500_channels(gpu_ctx):
    """ten passes of the scan, more entries than a wavefront has lanes; against the dense read"""
    B = 2500
    busy = sorted({0, 63, 64, 1023, 1024, 2304, 2499} | {int(b) for b in np.linspace(5, 2490, 33).astype(int)})
    assert len(busy) == 40
    p = Pushed(gpu_ctx, B, busy)
    p.sane()
    want = p.want(user=1)
    E, V, F = totals(want)
    pack = api.OutPack(E, V, F, ctx=gpu_ctx)            # capacities that end exactly at the last kept byte
    pack.append(p.eng, user=1)
    check_pack(pack.read(), want, appends=1)
    assert pack.rc == 0 and E >= 30
    pack.close()
    p.close()
