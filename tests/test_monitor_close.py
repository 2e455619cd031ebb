"""Naming on close (api.Monitor / api.DeviceMonitor, on_close=...; include/digiham_amd.h "Band monitor", step C): a
transmission that ends before the scanner has confirmed it is named when its gate closes, from hits and their quality,
and replayed from the ring like any other.

The scene: eight keyed rows -- POCSAG preamble + 1 batch, POCSAG preamble + 2 batches, D-Star header + 1 superframe, 2 YSF
frames, 3 DMR bursts, 3 NXDN frames, noise, silence -- with the seeds and impairments of tests/test_scan.py::protocol_rows,
each behind one to three closed pushes and followed by noise of sigma 0.3.  A row's gate is open for every push that overlaps
its transmission and one more (the hang), then closed to the end.  The yardstick is tests/test_monitor.py's: a fresh
single-channel engine fed in one push what the rules say the channel's decoder got."""
import ctypes as C

import numpy as np
import pytest

from digiham_amd import _capi, _taps, api, synth
from test_monitor import check
from test_monitor_device import same_blocks
from test_scan import FAMILY, NAMES, SOURCE, STAT, model, run_front

PUSH, LEAD, RELEASE, DEPTH = 4800, 480, 4, 96000
ROWS = ["pocsag1", "pocsag2", "dstar", "ysf", "dmr", "nxdn", "noise", "silence"]
SHORT = {0: "pocsag", 1: "pocsag", 2: "dstar", 3: "ysf"}          # the rows only naming on close decodes
FRAME_BYTES = {0: 63, 1: 126, 2: 207, 3: 120}                    # what a fresh engine delivers of them
BEHIND = [1, 2, 3, 1, 2, 3, 1, 2]                                 # closed pushes in front of the row
OFFSET = [0, 240, 300, 120, 60, 400, 0, 0]                        # ... and where in its first open push the row begins: within one
                                                                  # power block of the squelch (noise in front detunes a slicer)
SILENCE_PUSHES = 3


def transmissions():
    """the six short transmissions and the noise, as their own front ends receive them"""
    rng = np.random.default_rng(99)
    dmr = synth.impair(synth.shape(synth.dmr_stream(31, 3)), 1, snr_db=24, dc=0.05, delay=3)
    ysf = synth.impair(synth.shape(synth.ysf_stream(32, 2)), 2, snr_db=22, dc=-0.05, delay=5, gain=0.8)
    nxdn = synth.impair(synth.shape(synth.nxdn_stream(33, 3), sps=20, taps=_taps.narrow()), 3, snr_db=24, delay=7)
    bits, _, _ = synth.dstar_transmission(np.random.default_rng(34), n_superframes=1)
    dstar = synth.impair(synth.fsk_shape(np.concatenate([rng.integers(0, 2, 41).astype(np.uint8), bits]), sps=10), 4, snr_db=22, dc=0.03)
    text = lambda n: "".join(chr(int(c)) for c in rng.integers(32, 127, n))
    # (an address of frame 0 and 39 characters: address, 14 message codewords and an idle one -- a message per batch)
    words = synth.pocsag_batches([(int(rng.integers(8, 1 << 21)) & ~7, 3, text(39)) for _ in range(2)])
    assert len(words) == 32
    pocsag = []
    for batches in (1, 2):
        pbits = [1, 0] * 288
        for i in range(0, 16 * batches, 16):
            for w in [synth.POCSAG_SYNC] + words[i:i + 16]:
                pbits += synth._bits_of(w, 32)
        pocsag.append(synth.impair(synth.fsk_shape(np.array(pbits, np.uint8), sps=40, invert=True), 5, snr_db=22, dc=0.02, delay=11))
    noise = rng.normal(0, 0.3, 90000).astype(np.float32)
    out = [pocsag[0], pocsag[1], dstar, ysf, dmr, nxdn, noise]
    assert [len(x) for x in out] == [44800, 66560, 30120, 10130, 4690, 13000, 90000]
    return out


class Scene:
    """x [8][rounds x PUSH], counts [rounds][8], and per row the first and the last open round"""

    def __init__(self, tx, behind=BEHIND, offset=OFFSET, tail=RELEASE + 1, gaps=None):
        B = len(tx)
        self.first = list(behind)
        self.last = []
        for b in range(B):
            end = behind[b] * PUSH + offset[b] + len(tx[b])
            self.last.append(-(-end // PUSH))                  # the pushes that overlap the row, and one push of hang
        self.rounds = max(self.last) + 1 + tail
        self.x = np.zeros((B, self.rounds * PUSH), np.float32)
        self.counts = np.zeros((self.rounds, B), np.uint32)
        for b in range(B):
            self.x[b] = np.random.default_rng(1000 + b).normal(0, 0.3, self.x.shape[1]).astype(np.float32)
            at = behind[b] * PUSH + offset[b]
            self.x[b, at:at + len(tx[b])] = tx[b]
            self.counts[self.first[b]:self.last[b] + 1, b] = PUSH
        for b, k in (gaps or {}).items():                      # a round in which the gate of row b is closed all the same
            self.counts[k, b] = 0
        self.B = B

    def pushes(self):
        return [(np.ascontiguousarray(self.x[:, k * PUSH:(k + 1) * PUSH]), self.counts[k].copy()) for k in range(self.rounds)]

    def start(self, b):
        return self.first[b] * PUSH - LEAD


_SHARED = {}                                  # computed once per session; never modified


@pytest.fixture(scope="module")
def scene():
    if "scene" not in _SHARED:
        tx = transmissions()
        s = Scene(tx + [np.zeros(0, np.float32)])
        s.x[7] = 0.0                                           # silence: a gate that opens on nothing for three pushes
        s.counts[:, 7] = 0
        s.counts[s.first[7]:s.first[7] + SILENCE_PUSHES, 7] = PUSH
        s.last[7] = s.first[7] + SILENCE_PUSHES - 1
        s.x.setflags(write=False)
        _SHARED["scene"] = s
    return _SHARED["scene"]


def family_sums(st):
    """per family (H, periodic, D) of a [9] statistics row"""
    out = []
    for f in range(5):
        ids = [i for i in range(9) if FAMILY[i] == f]
        out.append((int(st["hits"][ids].sum()), int(st["periodic"][ids].sum()), int(st["best_dist"][ids].min())))
    return out


def rules_statistics(emu_ctx, s):
    """the numpy statement of the scan rules (tests/test_scan.py::model) on the symbols of every row's open samples behind
    each front end (the slicer of an Engine(proto="none") on the CPU emulation, one push)"""
    if "want" not in _SHARED:
        want = np.zeros((s.B, 9), STAT)
        for b in range(s.B):
            row = np.ascontiguousarray(s.x[b:b + 1, s.first[b] * PUSH:(s.last[b] + 1) * PUSH])
            for f in api.SCAN_FRONTS:
                syms, _, _ = run_front(emu_ctx, row, f, "none", [row.shape[1]])
                st = model(syms[0])[1]
                for i in range(9):
                    if SOURCE[i] == f:
                        want[b, i] = st[i]
        _SHARED["want"] = want
    return _SHARED["want"]


def precondition(ctx, emu_ctx, s):
    """Before any monitor is asked: the scanner's statistics at every row's last open round are those of the rules, and
    they show the evidence the test is about."""
    want = rules_statistics(emu_ctx, s)
    key = ("scanned", id(ctx))
    if key not in _SHARED:
        sc = api.Scanner(s.B, PUSH, ctx=ctx)
        for chunk, counts in s.pushes():
            if counts.any():
                sc.push(chunk, counts=counts)              # (a closed row is not pushed: its statistics stay its last open round's)
        _SHARED[key] = sc.stats()
        sc.close()
    got = _SHARED[key]
    for b in range(s.B):
        assert got[b].tobytes() == want[b].view(api.SCAN_STAT_DTYPE).tobytes(), ROWS[b]
    fam = [family_sums(want[b]) for b in range(s.B)]
    for b, name in SHORT.items():
        assert fam[b][NAMES.index(name)][1] < 2, (ROWS[b], fam[b])          # not confirmed while open ...
        assert max(f[1] for f in fam[b]) < 2, (ROWS[b], fam[b])
    assert fam[0][4][0] == 1 and fam[0][4][2] == 0 and fam[1][4][0] == 2 and fam[1][4][2] == 0
    assert fam[2][3][0] >= 2 and fam[2][3][2] <= 1 and fam[3][1][0] >= 1 and fam[3][1][2] <= 1
    assert fam[2][0][0] >= 1 and fam[2][0][2] > 1, fam[2]                   # the D-Star row through wide10: DMR hits, none close
    assert fam[2][0][0] == fam[2][3][0], fam[2]                             # ... as many as D-Star's own (the tie of test_thresholds)
    assert fam[4][0][1] >= 2 and fam[5][2][1] >= 2                          # DMR and NXDN are confirmed while open
    for b in (6, 7):
        assert all(f[1] < 2 for f in fam[b]), (ROWS[b], fam[b])
        for f, (hits, dist) in zip(fam[b], api.CLOSE_DEFAULT.values()):
            assert hits == 0 or f[0] < hits or f[2] > dist, (ROWS[b], fam[b])
    return fam


def drive(mon, pushes):
    """Every round into `mon`.  Returns the trace of (assigned, start) after every round and all blocks."""
    trace, blocks, total = [], [], 0
    for chunk, counts in pushes:
        got = mon.push(chunk, counts=counts)
        total += chunk.shape[1]
        assert [(b["channel"], b["first_sample"]) for b in got] == sorted((b["channel"], b["first_sample"]) for b in got)
        for blk in got:
            assert blk["proto"] == mon.assigned[blk["channel"]] and mon.start[blk["channel"]] <= blk["first_sample"] < total
        blocks += got
        trace.append((list(mon.assigned), list(mon.start)))
    return trace, blocks


def segment(s, b, proto, start, named_at, blocks, later=()):
    """what test_monitor.check takes: the blocks of channel b, and what its decoder was fed"""
    mine = [blk for blk in blocks if blk["channel"] == b]
    fed = [s.x[b, start:named_at]] + [s.x[b, k * PUSH:(k + 1) * PUSH] for k in later]
    return dict(proto=proto, frames=[blk["frames"] for blk in mine], events=[blk["events"] for blk in mine], fed=fed,
                at=[blk["first_sample"] for blk in mine])


def named_while_open(s, trace, blocks, ctx):
    """the DMR and the NXDN row, as without naming on close: named in an open round, fed live while open, released"""
    for b, name in ((4, "dmr"), (5, "nxdn")):
        names = [t[0][b] for t in trace]
        k = names.index(name)
        assert s.first[b] <= k <= s.last[b] and trace[k][1][b] == s.start(b)
        assert names[k:s.last[b] + RELEASE] == [name] * (s.last[b] + RELEASE - k) and set(names[s.last[b] + RELEASE:]) == {None}
        seg = segment(s, b, name, s.start(b), (k + 1) * PUSH, blocks, later=range(k + 1, s.last[b] + 1))
        f, e = check(ctx, seg)
        assert len(e)


def key(blocks):
    return [(b["channel"], b["proto"], b["first_sample"], b["frames"].tobytes(), b["events"].tobytes()) for b in blocks]


def run_off(ctx, s):
    k = ("off", id(ctx))
    if k not in _SHARED:
        mon = api.Monitor(s.B, PUSH, depth=DEPTH, lead=LEAD, release=RELEASE, ctx=ctx)
        _SHARED[k] = drive(mon, s.pushes())
        mon.close()
    return _SHARED[k]


def test_off_is_today(ctx, emu_ctx, scene):
    s = scene
    precondition(ctx, emu_ctx, s)
    trace, blocks = run_off(ctx, s)
    mon = api.Monitor(s.B, PUSH, depth=DEPTH, lead=LEAD, release=RELEASE, ctx=ctx, on_close=None)
    trace2, blocks2 = drive(mon, s.pushes())
    mon.close()
    assert trace2 == trace and key(blocks2) == key(blocks)
    for b in list(SHORT) + [6, 7]:
        assert all(t[0][b] is None for t in trace), ROWS[b]
        assert not [blk for blk in blocks if blk["channel"] == b], ROWS[b]
    named_while_open(s, trace, blocks, ctx)


def check_default(s, trace, blocks, ctx):
    for b, name in SHORT.items():
        names = [t[0][b] for t in trace]
        k = s.last[b] + 1                                                  # the closing round, not earlier
        assert names[:k] == [None] * k and names[k:k + RELEASE - 1] == [name] * (RELEASE - 1), (ROWS[b], names)
        assert set(names[k + RELEASE - 1:]) == {None}, (ROWS[b], names)    # released in its `release`-th closed round, as any channel
        assert trace[k][1][b] == s.start(b), ROWS[b]
        seg = segment(s, b, name, s.start(b), (k + 1) * PUSH, blocks)
        assert seg["at"] and all(s.start(b) <= a < (k + 1) * PUSH for a in seg["at"])
        f, e = check(ctx, seg)                                             # = a fresh engine fed row[start:total at naming]
        assert len(f) == FRAME_BYTES[b] and len(e), (ROWS[b], len(f), len(e))
    for b in (6, 7):
        assert all(t[0][b] is None for t in trace) and not [blk for blk in blocks if blk["channel"] == b], ROWS[b]
    named_while_open(s, trace, blocks, ctx)


def test_default_names_the_short_rows(ctx, emu_ctx, scene):
    """the test that needs the feature"""
    s = scene
    precondition(ctx, emu_ctx, s)
    mon = api.Monitor(s.B, PUSH, depth=DEPTH, lead=LEAD, release=RELEASE, ctx=ctx, on_close="default")
    trace, blocks = drive(mon, s.pushes())
    mon.close()
    check_default(s, trace, blocks, ctx)
    off_trace, off_blocks = run_off(ctx, s)
    for b in (4, 5):                                                       # exactly as without the mode
        assert [t[0][b] for t in trace] == [t[0][b] for t in off_trace] and [t[1][b] for t in trace] == [t[1][b] for t in off_trace]
        assert key([blk for blk in blocks if blk["channel"] == b]) == key([blk for blk in off_blocks if blk["channel"] == b])


def sub_scene(s, rows):
    """the rows `rows` of the scene alone, up to the round after the last of them is released"""
    rounds = max(s.last[b] for b in rows) + 1 + RELEASE + 1
    return [(np.ascontiguousarray(s.x[rows, k * PUSH:(k + 1) * PUSH]), s.counts[k, rows].copy()) for k in range(rounds)]


@pytest.mark.parametrize("rule, protos, row, want", [
    ({"pocsag": (2, 1)}, None, 0, None),
    ({"pocsag": (1, 0)}, None, 0, "pocsag"),
    ({"dmr": (1, 3), "dstar": (2, 1)}, None, 2, "dmr"),                    # H is level: the first family in order
    ("default", ("dmr", "ysf", "nxdn", "pocsag"), 2, None),                # the winner is not configured
])
def test_thresholds(ctx, emu_ctx, scene, rule, protos, row, want):
    s = scene
    precondition(ctx, emu_ctx, s)
    kw = {} if protos is None else dict(protos=protos)
    mon = api.Monitor(1, PUSH, depth=DEPTH, lead=LEAD, release=RELEASE, ctx=ctx, on_close=rule, **kw)
    trace, blocks = drive(mon, sub_scene(s, [row]))
    mon.close()
    names = [t[0][0] for t in trace]
    k = s.last[row] + 1
    if want is None:
        assert set(names) == {None} and not blocks
    else:
        assert names[:k] == [None] * k and names[k] == want and trace[k][1][0] == s.start(row)


def reopening():
    """a POCSAG row of two batches whose gate is closed for the round that ends batch 1's hang, then open again"""
    tx = transmissions()[1]
    probe = Scene([tx], behind=[1], offset=[700])
    gap = -(-(PUSH + 700 + 44800) // PUSH) + 1                 # the round after the hang of preamble + batch 1
    assert probe.first[0] < gap < probe.last[0]
    return Scene([tx], behind=[1], offset=[700], gaps={0: gap}), gap


def check_reopening(s, gap, trace, blocks, ctx):
    names = [t[0][0] for t in trace]
    assert names[:gap] == [None] * gap and names[gap:s.last[0] + RELEASE] == ["pocsag"] * (s.last[0] + RELEASE - gap)
    assert set(names[s.last[0] + RELEASE:]) == {None} and trace[gap][1][0] == s.start(0) == trace[s.last[0]][1][0]
    seg = segment(s, 0, "pocsag", s.start(0), (gap + 1) * PUSH, blocks, later=range(gap + 1, s.last[0] + 1))
    f, e = check(ctx, seg)                                     # the replay plus the later open pushes, in one engine
    assert len(f) > FRAME_BYTES[0] and max(seg["at"]) >= (gap + 1) * PUSH


def test_reopening(ctx):
    s, gap = reopening()
    mon = api.Monitor(1, PUSH, depth=DEPTH, lead=LEAD, release=RELEASE, ctx=ctx, on_close="default")
    trace, blocks = drive(mon, s.pushes())
    mon.close()
    check_reopening(s, gap, trace, blocks, ctx)


class Both:
    """api.Monitor and api.DeviceMonitor fed the same pushes: after every round equal in assigned, start, total and in
    the list of blocks (channel, proto, first_sample, bytes)"""

    def __init__(self, n_channels, ctx, packed=False, **kw):
        self.ref = api.Monitor(n_channels, PUSH, ctx=ctx, **kw)
        self.dev = api.DeviceMonitor(n_channels, PUSH, ctx=ctx, packed=packed, **kw)
        self.B, self.ctx, self.packed, self.rounds = n_channels, ctx, packed, 0

    assigned = property(lambda self: self.dev.assigned)
    start = property(lambda self: self.dev.start)

    def push(self, rows, counts=None):
        mem = self.ctx.mem
        rows, counts = mem.from_numpy(np.ascontiguousarray(rows, np.float32)), mem.from_numpy(np.ascontiguousarray(counts, np.uint32))
        want = self.ref.push(rows, counts=counts)
        got = self.dev.push(rows, counts=counts)
        self.rounds += 1
        same_blocks(got, want)                                 # (packed: an entry's tag is the block's first_sample)
        assert self.dev.assigned == self.ref.assigned and self.dev.start == self.ref.start, self.rounds
        assert self.dev.total == self.ref.pre.total
        return got

    def close(self):
        self.ref.close()
        self.dev.close()


@pytest.mark.parametrize("packed", [False, True])
def test_device_monitor(ctx, emu_ctx, scene, packed):
    s = scene
    precondition(ctx, emu_ctx, s)
    mon = Both(s.B, ctx, packed=packed, depth=DEPTH, lead=LEAD, release=RELEASE, on_close="default")
    trace, blocks = drive(mon, s.pushes())
    mon.close()
    check_default(s, trace, blocks, ctx)
    r, gap = reopening()
    mon = Both(1, ctx, packed=packed, depth=DEPTH, lead=LEAD, release=RELEASE, on_close="default")
    trace, blocks = drive(mon, r.pushes())
    mon.close()
    check_reopening(r, gap, trace, blocks, ctx)


def test_device_monitor_off_and_subset(ctx, scene):
    """the mode off, and a winner that is not configured, behind the C ABI"""
    s = scene
    for kw in (dict(on_close=None), dict(on_close="default", protos=("dmr", "ysf", "nxdn", "pocsag"))):
        rows = [2, 4]
        mon = Both(len(rows), ctx, depth=DEPTH, lead=LEAD, release=RELEASE, **kw)
        trace, blocks = drive(mon, sub_scene(s, rows))
        mon.close()
        assert all(t[0][0] is None for t in trace) and "dmr" in [t[0][1] for t in trace]


def test_config_sizes_and_errors(ctx, scene):
    """dh_monitor_config of the sizes before dmr_both_slots, before close_hits and whole; a V2-size struct is the mode off"""
    lib, mem, s = ctx.lib, ctx.mem, scene
    v1, v2, full = _capi.MONITOR_CONFIG_V1_SIZE, _capi.MONITOR_CONFIG_V2_SIZE, C.sizeof(_capi.MonitorConfig)
    assert (v1, v2, full) == (48, 56, 96)
    protos = 1 << _capi.PROTO["pocsag"]
    hits, dist = (C.c_uint32 * 5)(0, 0, 0, 0, 1), (C.c_uint32 * 5)(0, 0, 0, 0, 1)

    def create(struct_size):
        cfg = _capi.MonitorConfig(struct_size, getattr(mem, "index", 0), 1, PUSH, DEPTH, LEAD, 2, RELEASE, protos, mem.stream(), 0, 0, hits, dist)
        h = C.c_void_p()
        return lib.dh_monitor_create(C.byref(cfg), C.byref(h)), h

    for size in (v1 - 1, v1 + 4, v2 - 1, v2 + 4, full - 4, full - 1):
        rc, h = create(size)
        assert rc == _capi.DH_EINVAL and not h.value, size
    assigned = {}
    for size in (v1, v2, full):
        rc, h = create(size)
        assert rc == 0 and h.value, size
        seen = set()
        for chunk, counts in sub_scene(s, [0]):
            rows, cnt = mem.from_numpy(chunk), mem.from_numpy(counts)
            assert lib.dh_monitor_push(h, mem.ptr(rows), PUSH, PUSH, mem.ptr(cnt), _capi.MONITOR_SINK(0), None) == 0
            a = np.zeros(1, np.uint8)
            assert lib.dh_monitor_state(h, a.ctypes.data_as(C.c_void_p), None) == 0
            seen.add(int(a[0]))
        assigned[size] = seen
        lib.dh_monitor_destroy(h)
    assert assigned == {v1: {0}, v2: {0}, full: {0, _capi.PROTO["pocsag"]}}
    with pytest.raises(ValueError):
        api.DeviceMonitor(1, PUSH, ctx=ctx, on_close={"p25": (1, 1)})
    with pytest.raises(ValueError):
        api.Monitor(1, PUSH, ctx=ctx, on_close="always")


# ----------------------------------------------------------------------------- many workgroups
def spread(s, B, at, rows, ctx):
    """the scene's rows `rows` at the channels `at` of a band of B, every other channel silent with its gate closed"""
    mon = Both(B, ctx, depth=DEPTH, lead=LEAD, release=RELEASE, on_close="default")
    rounds = max(s.last[r] for r in rows) + 2
    named = {}
    for k in range(rounds):
        x, counts = np.zeros((B, PUSH), np.float32), np.zeros(B, np.uint32)
        x[at] = s.x[rows, k * PUSH:(k + 1) * PUSH]
        counts[at] = s.counts[k, rows]
        blocks = mon.push(x, counts=counts)
        assert {blk["channel"] for blk in blocks} <= set(at)
        for b, name in enumerate(mon.assigned):
            if name is not None:
                named.setdefault(b, (name, k))
    assert named == {b: (SHORT[r], s.last[r] + 1) for b, r in zip(at, rows)}
    mon.close()


@pytest.mark.gpu
def test_300_channels(gpu_ctx, scene):
    spread(scene, 300, [0, 63, 64, 255, 256, 299], [0, 1, 2, 3, 2, 3], gpu_ctx)


@pytest.mark.gpu
def test_2500_channels(gpu_ctx, scene):
    """ten workgroups of step C, a closing channel in each"""
    at = list(range(0, 2500, 97))
    spread(scene, 2500, at, [0] * len(at), gpu_ctx)
