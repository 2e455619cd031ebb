"""dh_monitor / api.DeviceMonitor: the band monitor behind the C ABI, its per-round bookkeeping in kernels.

Two yardsticks, both from tests/test_monitor.py.  (1) The rules: a fresh single-channel engine fed in one push exactly
the samples the monitor's rules say a channel's decoder gets (`drive`, `check`).  (2) api.Monitor, the host version of the
same rules, fed the same pushes: after EVERY round `assigned` and `start` are equal, and the list of blocks is equal in
channel, proto, first_sample and bytes.  `Both` below is what `drive` takes for a monitor: it pushes into the two and
compares before it hands the device monitor's blocks on."""
import ctypes as C

import numpy as np
import pytest

from digiham_amd import _capi, api
from test_monitor import PUSH, WANT, _scene, check, chunks, drive
from test_scan import N_SAMPLES, rows7      # noqa: F401  (fixture)


def same_blocks(got, want):
    key = lambda blocks: [(b["channel"], b["proto"], b["first_sample"], b["frames"].tobytes(), b["events"].tobytes()) for b in blocks]
    assert [k[:3] for k in key(got)] == [k[:3] for k in key(want)]
    assert key(got) == key(want)


class Both:
    def __init__(self, n_channels, max_samples, ctx, **kw):
        self.ref = api.Monitor(n_channels, max_samples, ctx=ctx, **kw)
        self.dev = api.DeviceMonitor(n_channels, max_samples, ctx=ctx, **kw)
        self.B, self.max_samples, self.ctx, self.rounds = n_channels, max_samples, ctx, 0
        self.same_state()

    assigned = property(lambda self: self.dev.assigned)
    start = property(lambda self: self.dev.start)

    def same_state(self):
        assert self.dev.assigned == self.ref.assigned, self.rounds
        assert self.dev.start == self.ref.start, self.rounds
        assert self.dev.total == self.ref.pre.total

    def push(self, rows, n=None, counts=None):
        mem = self.ctx.mem
        if isinstance(rows, np.ndarray) and rows.shape[1]:            # one upload for the two of them
            rows = mem.from_numpy(np.ascontiguousarray(rows, np.float32))
        if counts is not None and isinstance(counts, np.ndarray):
            counts = mem.from_numpy(np.ascontiguousarray(counts, np.uint32))
        want = self.ref.push(rows, n=n, counts=counts)
        got = self.dev.push(rows, n=n, counts=counts)
        self.rounds += 1
        same_blocks(got, want)
        self.same_state()
        return got

    def close(self):
        self.ref.close()
        self.dev.close()


def test_all_open(ctx, rows7):
    mon = Both(7, PUSH, ctx, depth=96000)
    assert mon.push(np.zeros((7, 0), np.float32)) == [] and mon.dev.total == 0
    segs, trace = drive(mon, [(c, None) for c in chunks(rows7)])
    assert mon.assigned == WANT and mon.start == [0] * 5 + [None] * 2
    for b in range(5):
        assert len(segs[b]) == 1 and segs[b][0]["proto"] == WANT[b]
        assert len(np.concatenate(segs[b][0]["fed"])) == N_SAMPLES           # the decoder got the whole row, from sample 0
        f, e = check(ctx, segs[b][0])
        assert len(e), WANT[b]
    assert not segs[5] and not segs[6]
    assert segs[3][0]["named_at"] > 40000 and segs[4][0]["named_at"] > 60000       # ... the replay reached back that far
    mon.dev.reset()
    mon.ref.reset()
    mon.same_state()
    assert mon.assigned == [None] * 7 and mon.start == [None] * 7 and mon.dev.total == 0 and mon.dev.scanner.classify() == [None] * 7
    # ... and the round after a reset is the first round again
    blocks = mon.push(np.ascontiguousarray(rows7[:, :PUSH]))
    assert mon.assigned[0] == "dmr" and mon.start[0] == 0 and {b["channel"] for b in blocks} == {0}
    mon.close()


def test_keyed(ctx, rows7):
    """row b behind 4800 (b + 1) zeros, its gate closed for the pushes that lie wholly inside them"""
    B, body = 3, 7 * PUSH
    x = np.zeros((B, B * PUSH + body), np.float32)
    for b in range(B):
        x[b, PUSH * (b + 1):PUSH * (b + 1) + body] = rows7[b, :body][:x.shape[1] - PUSH * (b + 1)]
    pushes = [(c, np.array([PUSH if k >= b + 1 else 0 for b in range(B)], np.uint32)) for k, c in enumerate(chunks(x))]
    mon = Both(B, PUSH, ctx, depth=96000, lead=480)
    segs, trace = drive(mon, pushes)
    assert mon.assigned == WANT[:B]
    for b in range(B):
        assert len(segs[b]) == 1 and segs[b][0]["start"] == PUSH * (b + 1) - 480 == mon.start[b]
        f, e = check(ctx, segs[b][0])
        assert len(e) and len(f)
    mon.close()


def test_short_ring(ctx, rows7):
    """D-Star is named after 52 800 samples; a ring of 24 000 reaches back to 28 800, in five chunks across the seam"""
    x = np.ascontiguousarray(rows7[[0, 3]])
    mon = Both(2, PUSH, ctx, depth=24000)
    segs, trace = drive(mon, [(c, None) for c in chunks(x)])
    assert mon.assigned == ["dmr", "dstar"]
    d = segs[1][0]
    assert d["named_at"] == 52800 and d["start"] == d["named_at"] - 24000 == mon.start[1]
    assert (d["named_at"] - d["start"]) // mon.max_samples == 5 and d["at"][0] < d["named_at"]
    f, e = check(ctx, d)
    assert len(e)
    assert segs[0][0]["start"] == 0
    check(ctx, segs[0][0])
    mon.close()


def test_release(ctx, rows7):
    """channel 0: DMR, closed for `release` rounds, then YSF.  Channel 1: DMR, closed for release - 1 rounds, DMR again."""
    release, first, second = 4, 7, 10
    rounds = []
    for k in range(first + release + second):
        c, cnt = np.zeros((2, PUSH), np.float32), np.zeros(2, np.uint32)
        if k < first:
            c[0], c[1], cnt[:] = rows7[0, k * PUSH:(k + 1) * PUSH], rows7[0, k * PUSH:(k + 1) * PUSH], PUSH
        if k >= first + release:
            j = k - first - release
            c[0], cnt[0] = rows7[1, j * PUSH:(j + 1) * PUSH], PUSH
        if k >= first + release - 1:
            j = k - (release - 1)
            c[1], cnt[1] = rows7[0, j * PUSH:(j + 1) * PUSH], PUSH
        rounds.append((c, cnt))
    mon = Both(2, PUSH, ctx, depth=96000, lead=480, release=release)
    segs, trace = drive(mon, rounds)
    dedup = lambda names: [n for i, n in enumerate(names) if i == 0 or n != names[i - 1]]
    assert dedup([t[0] for t in trace]) == ["dmr", None, "ysf"]
    assert dedup([t[1] for t in trace]) == ["dmr"]
    assert trace[first + release - 2][0] == "dmr" and trace[first + release - 1][0] is None     # released in the release-th closed round
    assert [s["proto"] for s in segs[0]] == ["dmr", "ysf"] and [s["proto"] for s in segs[1]] == ["dmr"]
    assert segs[0][1]["start"] == (first + release) * PUSH - 480
    for s in segs[0] + segs[1]:
        f, e = check(ctx, s)
        assert len(e)
    assert len(np.concatenate(segs[1][0]["fed"])) == (first + second + 1) * PUSH
    mon.close()


def test_protocol_subset_and_scanner_counters(ctx, rows7):
    """protos = ysf, pocsag: only the wide10 and fsk40i scan engines exist; the DMR row wins its family every round and
    stays unassigned (the next-best family is not considered); the statistics of the YSF channel stop moving once it is
    assigned, and are those of a reset channel."""
    x = np.ascontiguousarray(rows7[[0, 1, 5], :6 * PUSH])     # YSF is named in the third round
    mon = Both(3, PUSH, ctx, protos=("ysf", "pocsag"))
    assert sorted(mon.dev.scanner_engines) == ["fsk40i", "wide10"] and sorted(mon.dev.engines) == ["pocsag", "ysf"]
    assert ctx.lib.dh_monitor_engine(mon.dev._h, _capi.PROTO["dmr"]) is None and ctx.lib.dh_monitor_scan_engine(mon.dev._h, 1) is None
    seen = []

    def after(k):
        st, want = mon.dev.scanner.stats(), mon.ref.scanner.stats()
        assert st.tobytes() == want.tobytes(), k
        seen.append((mon.assigned[1], st[1].tobytes(), st[0].tobytes()))
    segs, trace = drive(mon, [(c, None) for c in chunks(x)], after_round=after)
    assert mon.assigned == [None, "ysf", None] and all(t[0] is None for t in trace)
    assert mon.ref.scanner.classify(2)[0] == "dmr"            # ... not for want of a name
    i = [a for a, _, _ in seen].index("ysf")
    assert i >= 1 and seen[i - 1][1] != seen[i][1]
    assert len({s for _, s, _ in seen[i:]}) == 1 and len(seen) - i >= 3
    idle = np.zeros(9, api.SCAN_STAT_DTYPE)
    idle["best_dist"] = 255
    assert seen[-1][1] == idle.tobytes()
    assert seen[-1][2] != seen[i][2] != seen[0][2]            # the unassigned DMR channel goes on being scanned (no sync word in some rounds)
    check(ctx, segs[1][0])
    mon.close()


def spread(rows7, B, at, depth, ctx):
    """the seven rows at the channels `at` of a band of B, every other channel silent with its gate closed"""
    mon = Both(B, PUSH, ctx, depth=depth)
    counts = np.zeros(B, np.uint32)
    blocks = []
    for c in chunks(rows7):
        n = c.shape[1]
        x = np.zeros((B, n), np.float32)
        x[at] = c
        counts[at] = n
        blocks += mon.push(x, counts=counts)
    want = [None] * B
    for r, b in enumerate(at):
        want[b] = WANT[r]
    assert mon.assigned == want
    assert {b["channel"] for b in blocks} == {b for b in at if want[b] is not None}
    assert mon.start[at[0]] == 0 and all(mon.start[b] is not None for b in at[:5])
    if depth < 52800:
        assert mon.start[at[3]] == 52800 - depth              # D-Star is named after 52 800 samples (test_short_ring): as far back as the ring reaches
    silent = [b for b in range(B) if b not in at]
    assert (mon.dev.scanner.stats()["hits"][silent] == 0).all()
    mon.close()


def test_300_channels(ctx, rows7):
    spread(rows7, 300, [0, 63, 64, 255, 256, 298, 299], 96000, ctx)


@pytest.mark.gpu
def test_2500_channels(gpu_ctx, rows7):
    """more channels than one launch of the masked reset has workgroups, ten workgroups of steps A and B; a ring that the
    D-Star and POCSAG replays cross the seam of"""
    spread(rows7, 2500, [0, 63, 64, 1023, 1024, 2304, 2499], 24000, gpu_ctx)


def test_errors(ctx):
    lib, mem = ctx.lib, ctx.mem
    protos = sum(1 << _capi.PROTO[p] for p in ("dmr", "ysf"))
    good = lambda: _capi.MonitorConfig(C.sizeof(_capi.MonitorConfig), 0, 4, 100, 1000, 480, 2, 4, protos, mem.stream())
    h = C.c_void_p()
    for change in (dict(struct_size=C.sizeof(_capi.MonitorConfig) - 1), dict(protos=0), dict(protos=1), dict(protos=1 << 6), dict(n_channels=0),
                   dict(n_channels=65537), dict(max_samples=0), dict(depth=0), dict(depth=(1 << 24) + 1)):
        cfg = good()
        for k, v in change.items():
            setattr(cfg, k, v)
        assert lib.dh_monitor_create(C.byref(cfg), C.byref(h)) == _capi.DH_EINVAL, change
        assert not h.value
    cfg = good()
    assert lib.dh_monitor_create(None, C.byref(h)) == _capi.DH_EINVAL and lib.dh_monitor_create(C.byref(cfg), None) == _capi.DH_EINVAL
    with pytest.raises(_capi.DhError) as e:
        api.DeviceMonitor(4, 100, protos=(), ctx=ctx)
    assert e.value.code == _capi.DH_EINVAL

    mon = api.DeviceMonitor(4, 100, depth=1000, protos=("dmr", "ysf"), ctx=ctx)
    rows, cnt = mem.zeros((4, 128), np.float32), mem.zeros((4,), np.uint32)
    sink, null, total = _capi.MONITOR_SINK(lambda user, info: None), None, C.c_uint64(0)
    bad = [lib.dh_monitor_push(mon._h, mem.ptr(rows), 128, 101, mem.ptr(cnt), sink, null),        # n > max_samples
           lib.dh_monitor_push(mon._h, mem.ptr(rows), 63, 64, mem.ptr(cnt), sink, null),          # stride < n
           lib.dh_monitor_push(mon._h, null, 128, 64, mem.ptr(cnt), sink, null),
           lib.dh_monitor_push(null, mem.ptr(rows), 128, 64, mem.ptr(cnt), sink, null),
           lib.dh_monitor_reset(null), lib.dh_monitor_state(null, null, null),
           lib.dh_monitor_total(null, C.byref(total)), lib.dh_monitor_total(mon._h, null)]
    assert bad == [_capi.DH_EINVAL] * len(bad)
    assert lib.dh_monitor_engine(null, 1) is None and lib.dh_monitor_engine(mon._h, 0) is None and lib.dh_monitor_engine(mon._h, 6) is None
    assert lib.dh_monitor_scan_engine(null, 0) is None and lib.dh_monitor_scan_engine(mon._h, 4) is None and lib.dh_monitor_scan_engine(mon._h, -1) is None
    assert mon.total == 0 and mon.assigned == [None] * 4           # none of them appended anything
    with pytest.raises(_capi.DhError):
        mon.push(np.zeros((4, 101), np.float32))
    assert lib.dh_monitor_push(mon._h, null, 0, 0, null, sink, null) == 0 and mon.total == 0       # n = 0 needs nothing
    assert lib.dh_monitor_push(mon._h, mem.ptr(rows), 128, 64, null, _capi.MONITOR_SINK(0), null) == 0 and mon.total == 64     # no counts, no sink
    assert lib.dh_monitor_state(mon._h, null, null) == 0
    lib.dh_monitor_destroy(null)
    mon.close()
    mon.close()


def test_end_to_end_through_the_channelizer(ctx):
    """the scene and the squelch of tests/test_monitor.py::test_end_to_end_through_the_channelizer: a DMR carrier keyed on
    at 0.2 s, a YSF carrier at 0.4 s and an empty channel; the channelizer's rows and counts go to both monitors where they are"""
    L, hang, P = 480, 2, 4807
    D, rate, raster, x, meta = _scene("cpu")
    h = api.channel_taps(rate, D, 5500.0, 8000.0, 70.0)
    host = lambda a: np.array(ctx.mem.to_numpy(a))
    n = len(x)
    cz = api.Channelizer(rate, D, raster, h, input="cs16", output="fm", dcblock=True, max_input=P * D, ctx=ctx)
    cz.enable_power(block=L)
    power = []
    for pos in range(0, n, P * D):
        cz.push(x[pos:pos + P * D])
        power.append(host(cz.power_blocks()[0]).copy())
    pw = np.concatenate(power, axis=1)
    blk = np.arange(pw.shape[1])
    F = -(-len(h) // D)
    keyed = [pw[0, (blk * L >= 9600 + F)], pw[1, (blk * L >= 19200 + F)]]
    db = lambda v: 10.0 * np.log10(v)
    min_keyed, max_empty = min(float(k.min()) for k in keyed), float(pw[2].max())
    assert db(min_keyed) - db(max_empty) >= 8.0, "the scene does not meet the test's precondition"
    open_db = db(min_keyed) - 3.0
    cz.reset()
    cz.enable_power(block=L, open_db=open_db, close_db=open_db - 3.0, hang_blocks=hang)

    mon = Both(3, cz.out_stride, ctx, depth=96000, lead=480)
    hist, counts, fed, blocks, total = [], [], {}, [], 0
    for pos in range(0, n, P * D):
        rows, k = cz.push(x[pos:pos + P * D])
        was = list(mon.assigned)
        blocks += mon.push(rows, k, counts=cz.counts)
        total += k
        cnt = host(cz.counts).view(np.uint32).copy()
        hr = host(rows)[:, :k].copy()
        hist.append(hr); counts.append(cnt)
        for b in range(3):
            if mon.assigned[b] is not None and was[b] is None:
                fed[b] = [np.concatenate(hist, axis=1)[b, mon.start[b]:total]]
            elif mon.assigned[b] is not None and cnt[b]:
                fed[b].append(hr[b])
    counts = np.stack(counts)
    assert mon.assigned == ["dmr", "ysf", None] and (counts[:, 2] == 0).all()
    first_open = [int(np.flatnonzero(counts[:, b])[0]) * P for b in range(2)]
    for b, name in ((0, "dmr"), (1, "ysf")):
        assert mon.start[b] == first_open[b] - 480             # the decoder began `lead` samples before the squelch opened
        seg = dict(proto=name, frames=[blk_["frames"] for blk_ in blocks if blk_["channel"] == b],
                   events=[blk_["events"] for blk_ in blocks if blk_["channel"] == b], fed=fed[b], at=[])
        f, e = check(ctx, seg)
        assert len(e) and len(f)
    assert not [blk_ for blk_ in blocks if blk_["channel"] == 2]
    mon.close()
    cz.close()
