"""api.DeviceMonitor(packed=True) / dh_monitor_push_packed: a monitor round read back through one dh_outpack.

The yardstick is api.Monitor, the host version of the same rules, fed the same pushes (tests/test_monitor_device.py's
`Both`, here with the packed monitor in place of the sink-driven one): after EVERY round `assigned`, `start` and `total`
are equal and the list of blocks is equal in channel, proto, first_sample and bytes.  `drive`, `check` and the scenes are
those of tests/test_monitor.py and tests/test_monitor_device.py."""
import ctypes as C

import numpy as np
import pytest

import test_monitor_device
from digiham_amd import _capi, api
from test_monitor import PUSH, WANT, check, chunks, drive
from test_monitor_device import Both, same_blocks
from test_scan import N_SAMPLES, rows7      # noqa: F401  (fixture)


class BothPacked(Both):
    def __init__(self, n_channels, max_samples, ctx, **kw):
        self.ref = api.Monitor(n_channels, max_samples, ctx=ctx, **kw)
        self.dev = api.DeviceMonitor(n_channels, max_samples, ctx=ctx, packed=True, **kw)
        assert self.dev.pack is not None
        self.B, self.max_samples, self.ctx, self.rounds = n_channels, max_samples, ctx, 0
        self.same_state()


def test_all_open(ctx, rows7):
    mon = BothPacked(7, PUSH, ctx, depth=96000)
    assert mon.push(np.zeros((7, 0), np.float32)) == [] and mon.dev.total == 0
    segs, trace = drive(mon, [(c, None) for c in chunks(rows7)])
    assert mon.assigned == WANT and mon.start == [0] * 5 + [None] * 2
    for b in range(5):
        assert len(segs[b]) == 1 and segs[b][0]["proto"] == WANT[b]
        assert len(np.concatenate(segs[b][0]["fed"])) == N_SAMPLES
        f, e = check(ctx, segs[b][0])
        assert len(e), WANT[b]
    assert not segs[5] and not segs[6]               # at least three channels with output, two without (five protocols, seven rows)
    mon.close()


def test_keyed(ctx, rows7):
    """row b behind 4800 (b + 1) zeros, its gate closed for the pushes that lie wholly inside them; three more channels
    stay closed throughout"""
    K, B, body = 3, 6, 7 * PUSH
    x = np.zeros((B, K * PUSH + body), np.float32)
    for b in range(K):
        x[b, PUSH * (b + 1):PUSH * (b + 1) + body] = rows7[b, :body][:x.shape[1] - PUSH * (b + 1)]
    pushes = [(c, np.array([PUSH if b < K and k >= b + 1 else 0 for b in range(B)], np.uint32)) for k, c in enumerate(chunks(x))]
    mon = BothPacked(B, PUSH, ctx, depth=96000, lead=480)
    segs, trace = drive(mon, pushes)
    assert mon.assigned == WANT[:K] + [None] * (B - K)
    for b in range(K):
        assert len(segs[b]) == 1 and segs[b][0]["start"] == PUSH * (b + 1) - 480 == mon.start[b]
        f, e = check(ctx, segs[b][0])
        assert len(e) and len(f)
    assert not any(segs[K:])
    mon.close()


def test_short_ring(ctx, rows7):
    """D-Star is named after 52 800 samples; a ring of 24 000 reaches back to 28 800: five replay chunks appended to the
    pack in one round.  Three silent channels beside the three carriers."""
    x = np.zeros((6, N_SAMPLES), np.float32)
    x[[0, 2, 4]] = rows7[[0, 3, 1]]
    mon = BothPacked(6, PUSH, ctx, depth=24000)
    segs, trace = drive(mon, [(c, None) for c in chunks(x)])
    assert mon.assigned == ["dmr", None, "dstar", None, "ysf", None]
    d = segs[2][0]
    assert d["named_at"] == 52800 and d["start"] == d["named_at"] - 24000 == mon.start[2]
    assert (d["named_at"] - d["start"]) // mon.max_samples == 5 and d["at"][0] < d["named_at"]
    for b in (0, 2, 4):
        f, e = check(ctx, segs[b][0])
        assert len(e)
    assert not segs[1] and not segs[3] and not segs[5]
    mon.close()


def test_release(ctx, rows7):
    """channel 0: DMR, closed for `release` rounds, then YSF.  Channel 1: DMR, closed for release - 1 rounds, DMR again.
    Channel 2: YSF for as long as its row lasts.  Channels 3-5 never open."""
    release, first, second, B = 4, 7, 10, 6
    rounds = []
    for k in range(first + release + second):
        c, cnt = np.zeros((B, PUSH), np.float32), np.zeros(B, np.uint32)
        if k < N_SAMPLES // PUSH:
            c[2], cnt[2] = rows7[1, k * PUSH:(k + 1) * PUSH], PUSH
        if k < first:
            c[0], c[1], cnt[:2] = rows7[0, k * PUSH:(k + 1) * PUSH], rows7[0, k * PUSH:(k + 1) * PUSH], PUSH
        if k >= first + release:
            j = k - first - release
            c[0], cnt[0] = rows7[1, j * PUSH:(j + 1) * PUSH], PUSH
        if k >= first + release - 1:
            j = k - (release - 1)
            c[1], cnt[1] = rows7[0, j * PUSH:(j + 1) * PUSH], PUSH
        rounds.append((c, cnt))
    mon = BothPacked(B, PUSH, ctx, depth=96000, lead=480, release=release)
    segs, trace = drive(mon, rounds)
    dedup = lambda names: [n for i, n in enumerate(names) if i == 0 or n != names[i - 1]]
    assert dedup([t[0] for t in trace]) == ["dmr", None, "ysf"]
    assert dedup([t[1] for t in trace]) == ["dmr"]
    assert [s["proto"] for s in segs[0]] == ["dmr", "ysf"] and [s["proto"] for s in segs[1]] == ["dmr"] and [s["proto"] for s in segs[2]] == ["ysf"]
    assert segs[0][1]["start"] == (first + release) * PUSH - 480
    for s in segs[0] + segs[1] + segs[2]:
        f, e = check(ctx, s)
        assert len(e)
    assert not any(segs[3:])
    mon.close()


def test_300_channels(ctx, rows7, monkeypatch):
    monkeypatch.setattr(test_monitor_device, "Both", BothPacked)
    test_monitor_device.spread(rows7, 300, [0, 63, 64, 255, 256, 298, 299], 96000, ctx)


@pytest.mark.gpu
def test_2500_channels(gpu_ctx, rows7, monkeypatch):
    monkeypatch.setattr(test_monitor_device, "Both", BothPacked)
    test_monitor_device.spread(rows7, 2500, [0, 63, 64, 1023, 1024, 2304, 2499], 24000, gpu_ctx)


def pack_blocks(pack):
    """(rc, blocks as DeviceMonitor.push builds them) of one read"""
    header, entries, events, frames = pack.read()
    blocks = [{"channel": b, "proto": api.PROTO_NAMES[user & 255], "first_sample": tag, "frames": frames[16 * off:16 * off + fc], "events": events[ei:ei + ec]}
              for b, user, tag, fc, ec, off, ei in entries.tolist()]
    return pack.rc, header, blocks


def test_small_pack_from_c(ctx, rows7):
    """dh_monitor_push_packed from ctypes with a pack of two entries: the round that needs more reads back DH_ECAPACITY and
    a prefix; the monitor's state is what Monitor's is, and the next round, into a cleared large pack, agrees again."""
    lib, mem, B = ctx.lib, ctx.mem, 6
    x = np.zeros((B, 12 * PUSH), np.float32)
    x[:3] = rows7[:3, :12 * PUSH]
    ref = api.Monitor(B, PUSH, ctx=ctx, depth=96000)
    dev = api.DeviceMonitor(B, PUSH, ctx=ctx, depth=96000)
    small, large = api.OutPack(2, 4096, 1 << 16, ctx=ctx), api.OutPack(64, 1 << 14, 1 << 20, ctx=ctx)
    key = lambda blk: (blk["channel"], blk["first_sample"])
    state, seen = "small", []
    for c in chunks(x):
        rows = mem.from_numpy(c)
        want = ref.push(rows)
        pack = small if state == "small" else large
        pack.clear()
        assert lib.dh_monitor_push_packed(dev._h, mem.ptr(rows), c.shape[1], c.shape[1], None, pack._h) == 0
        rc, header, got = pack_blocks(pack)
        dev._state = None
        assert dev.assigned == ref.assigned and dev.start == ref.start and dev.total == ref.pre.total
        if state == "small" and rc == _capi.DH_ECAPACITY:
            assert len(want) > 2 and header["n_entries"] == 2 and header["dropped"] == len(want) - 2
            wanted = {key(w): w for w in want}
            for blk in got:                              # the prefix that was kept is made of blocks of this round
                w = wanted[key(blk)]
                assert blk["proto"] == w["proto"] and blk["frames"].tobytes() == w["frames"].tobytes() and blk["events"].tobytes() == w["events"].tobytes()
            state = "large"
        else:
            assert rc == 0 and header["dropped"] == 0
            same_blocks(sorted(got, key=key), want)
        seen.append((state, rc, len(want)))
    assert any(rc == _capi.DH_ECAPACITY for _, rc, _ in seen)
    after = [n for s, rc, n in seen if s == "large" and rc == 0]
    assert after and max(after) >= 3                    # rounds after the overflow with all three channels decoding
    assert dev.assigned == ["dmr", "ysf", "nxdn", None, None, None]
    # a pack on another stream or device is refused before the round begins
    torch = getattr(mem, "torch", None)
    side = torch.cuda.Stream(mem.device) if torch is not None else None
    cfg = _capi.OutpackConfig(C.sizeof(_capi.OutpackConfig), getattr(mem, "index", 0), 8, 8, 64, C.c_void_p(side.cuda_stream if side is not None else 64))
    h = C.c_void_p()
    assert lib.dh_outpack_create(C.byref(cfg), C.byref(h)) == 0
    total = dev.total
    rows = mem.from_numpy(np.zeros((B, PUSH), np.float32))
    assert lib.dh_monitor_push_packed(dev._h, mem.ptr(rows), PUSH, PUSH, None, h) == _capi.DH_EINVAL
    assert lib.dh_monitor_push_packed(dev._h, mem.ptr(rows), PUSH, PUSH, None, None) == _capi.DH_EINVAL
    assert lib.dh_monitor_push_packed(None, mem.ptr(rows), PUSH, PUSH, None, large._h) == _capi.DH_EINVAL
    assert dev.total == total
    lib.dh_outpack_destroy(h)
    for o in (small, large, dev, ref):
        o.close()
