"""api.Monitor: scanner + pre-roll ring + the five protocol engines, against dedicated engines.

The yardstick is always a fresh api.Engine(1, ..., proto=name, **front) on the same ctx, fed in ONE push exactly the
samples the monitor's rules say the channel's decoder gets: the ring from `start` to the end of the round in which the
channel was named, then every later push in which the channel was open.  The monitor's blocks of that channel,
concatenated, must equal the yardstick's frames and events byte for byte (engines do not depend on how a stream is cut).
The rows and front ends are those of tests/test_scan.py."""
import numpy as np
import pytest

from digiham_amd import api, wideband
from test_scan import FRONTS, N_SAMPLES, rows7      # noqa: F401  (fixture)

WANT = ["dmr", "ysf", "nxdn", "dstar", "pocsag", None, None]
PUSH = 4800
EV_DMR_LC, EV_DSTAR_HEADER = 4, 64


def test_constants():
    assert api.PROTO_FRONT == {"dmr": "wide10", "ysf": "wide10", "nxdn": "narrow20", "dstar": "fsk10", "pocsag": "fsk40i"}
    for name, ids in api.SCAN_FAMILIES:
        assert {api.SCAN_SOURCE[i] for i in ids} == {api.PROTO_FRONT[name]}
    assert api.SCAN_FRONTS == FRONTS


_YARD = {}                                    # yardsticks computed once per (tier, protocol, input); never modified


def yardstick(ctx, name, x):
    key = (id(ctx), name, x.tobytes())
    if key not in _YARD:
        eng = api.Engine(1, max(len(x), 1), proto=name, ctx=ctx, **api.SCAN_FRONTS[api.PROTO_FRONT[name]])
        eng.push(np.ascontiguousarray(x[None, :], np.float32))
        f, fc = eng.frames()
        e, ec = eng.events()
        eng.close()
        _YARD[key] = (f[0, :fc[0]].copy(), e[0, :ec[0]].copy())
    return _YARD[key]


def chunks(x, step=PUSH):
    return [np.ascontiguousarray(x[:, s:s + step]) for s in range(0, x.shape[1], step)]


def drive(mon, pushes, after_round=None):
    """pushes: (chunk [B][n] float32, counts or None) per round.  Returns per channel its list of segments -- one per
    assignment: proto, start, the samples its decoder must have been fed, the frames and events that came out -- and the
    trace of `assigned` after every round."""
    B = mon.B
    hist, segs, trace, total = [[] for _ in range(B)], [[] for _ in range(B)], [], 0
    for k, (chunk, counts) in enumerate(pushes):
        was = list(mon.assigned)
        blocks = mon.push(chunk, counts=counts)
        total += chunk.shape[1]
        for b in range(B):
            hist[b].append(chunk[b])
            now, opened = mon.assigned[b], counts is None or counts[b] != 0
            if now is not None and was[b] is None:
                assert opened and mon.start[b] is not None
                row = np.concatenate(hist[b])
                segs[b].append(dict(proto=now, start=mon.start[b], named_at=total, fed=[row[mon.start[b]:total]], frames=[], events=[], at=[]))
            elif now is not None and opened:
                assert now == was[b]
                segs[b][-1]["fed"].append(chunk[b])
            if now is None:
                assert mon.start[b] is None
        assert [(blk["channel"], blk["first_sample"]) for blk in blocks] == sorted((blk["channel"], blk["first_sample"]) for blk in blocks)
        for blk in blocks:
            s = segs[blk["channel"]][-1]
            assert blk["proto"] == s["proto"] == mon.assigned[blk["channel"]]
            assert s["start"] <= blk["first_sample"] < total and blk["events"].dtype == api.EVENT_DTYPE and blk["frames"].dtype == np.uint8
            s["frames"].append(blk["frames"]); s["events"].append(blk["events"]); s["at"].append(blk["first_sample"])
        trace.append(list(mon.assigned))
        if after_round is not None:
            after_round(k)
    return segs, trace


def outputs(seg):
    f = np.concatenate(seg["frames"]) if seg["frames"] else np.zeros(0, np.uint8)
    e = np.concatenate(seg["events"]) if seg["events"] else np.zeros(0, api.EVENT_DTYPE)
    return f, e


def check(ctx, seg):
    """the segment's output equals the yardstick's; returns (frames, events)"""
    f, e = outputs(seg)
    wf, we = yardstick(ctx, seg["proto"], np.concatenate(seg["fed"]))
    assert len(e) == len(we) and e.tobytes() == we.tobytes(), (seg["proto"], len(e), len(we))
    assert len(f) == len(wf) and f.tobytes() == wf.tobytes(), (seg["proto"], len(f), len(wf))
    assert seg["at"] == sorted(seg["at"])
    return f, e


def test_all_open(ctx, rows7):
    x = rows7
    mon = api.Monitor(7, PUSH, depth=96000, ctx=ctx)
    assert mon.push(np.zeros((7, 0), np.float32)) == [] and mon.pre.total == 0
    segs, trace = drive(mon, [(c, None) for c in chunks(x)])
    assert mon.assigned == WANT and mon.start == [0] * 5 + [None] * 2
    out = {}
    for b in range(5):
        assert len(segs[b]) == 1 and segs[b][0]["proto"] == WANT[b]
        assert len(np.concatenate(segs[b][0]["fed"])) == N_SAMPLES           # the decoder got the whole row, from sample 0
        out[b] = check(ctx, segs[b][0])
        assert len(out[b][1]), WANT[b]
    assert not segs[5] and not segs[6]
    # what the monitor is for: the call set-up that lies before the point of classification
    assert segs[3][0]["named_at"] > 40000 and segs[4][0]["named_at"] > 60000
    header = lambda e: ((e["type"] == EV_DSTAR_HEADER) & (e["b"] == 0)).sum()
    assert header(out[3][1]) >= 1 and len(out[4][0]) > 0
    mon.reset()
    assert mon.assigned == [None] * 7 and mon.start == [None] * 7 and mon.pre.total == 0 and mon.scanner.classify() == [None] * 7
    mon.close()

    # the recipe without pre-roll: a Scanner, and an engine fed from the push after the one that named the channel
    sc = api.Scanner(7, PUSH, ctx=ctx)
    engs, named, got = {}, {}, {3: [[], []], 4: [[], []]}
    for c in chunks(x):
        for b, eng in engs.items():
            eng.push(np.ascontiguousarray(c[b][None, :]))
            f, fc = eng.frames()
            e, ec = eng.events()
            got[b][0].append(f[0, :fc[0]].copy()); got[b][1].append(e[0, :ec[0]].copy())
        sc.push(c)
        names = sc.classify(2)
        for b in (3, 4):
            if b not in engs and names[b] is not None:
                assert names[b] == WANT[b]
                engs[b] = api.Engine(1, PUSH, proto=names[b], ctx=ctx, **api.SCAN_FRONTS[api.PROTO_FRONT[names[b]]])
    assert sorted(engs) == [3, 4]
    assert header(np.concatenate(got[3][1])) == 0, "the radio header lies before the classification point"
    assert sum(len(f) for f in got[4][0]) == 0
    for eng in engs.values():
        eng.close()
    sc.close()


def test_keyed(ctx, rows7):
    """row b behind 4800 (b + 1) zeros, its gate closed for the pushes that lie wholly inside them"""
    B, body = 3, 7 * PUSH
    x = np.zeros((B, B * PUSH + body), np.float32)
    for b in range(B):
        x[b, PUSH * (b + 1):PUSH * (b + 1) + body] = rows7[b, :body][:x.shape[1] - PUSH * (b + 1)]
    pushes = [(c, np.array([PUSH if k >= b + 1 else 0 for b in range(B)], np.uint32)) for k, c in enumerate(chunks(x))]
    mon = api.Monitor(B, PUSH, depth=96000, lead=480, ctx=ctx)
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
    mon = api.Monitor(2, PUSH, depth=24000, ctx=ctx)
    segs, trace = drive(mon, [(c, None) for c in chunks(x)])
    assert mon.assigned == ["dmr", "dstar"]
    d = segs[1][0]
    assert d["named_at"] == 52800 and d["start"] == d["named_at"] - 24000 == mon.start[1]
    assert (d["named_at"] - d["start"]) // mon.max_samples == 5 and d["at"][0] < d["named_at"]      # five replay chunks; output from the replay
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
    mon = api.Monitor(2, PUSH, depth=96000, lead=480, release=release, ctx=ctx)
    segs, trace = drive(mon, rounds)
    dedup = lambda names: [n for i, n in enumerate(names) if i == 0 or n != names[i - 1]]
    assert dedup([t[0] for t in trace]) == ["dmr", None, "ysf"]          # (DMR is named in its first round)
    assert dedup([t[1] for t in trace]) == ["dmr"]
    assert trace[first + release - 2][0] == "dmr" and trace[first + release - 1][0] is None     # released in the release-th closed round
    assert [s["proto"] for s in segs[0]] == ["dmr", "ysf"] and [s["proto"] for s in segs[1]] == ["dmr"]
    assert segs[0][1]["start"] == (first + release) * PUSH - 480
    for s in segs[0] + segs[1]:
        f, e = check(ctx, s)
        assert len(e)
    # channel 1 was fed its DMR row without the gap: the closed rounds brought its decoder nothing
    assert len(np.concatenate(segs[1][0]["fed"])) == (first + second + 1) * PUSH
    mon.close()


def test_two_of_forty_channels(ctx, rows7):
    """a wide monitor with two busy channels: the closed ones cost nothing, and the outputs of few channels are read row by row"""
    B, busy = 40, {3: 0, 20: 1}
    rounds = []
    for k in range(6):
        c, cnt = np.zeros((B, PUSH), np.float32), np.zeros(B, np.uint32)
        for b, r in busy.items():
            c[b], cnt[b] = rows7[r, k * PUSH:(k + 1) * PUSH], PUSH
        rounds.append((c, cnt))
    mon = api.Monitor(B, PUSH, ctx=ctx)
    segs, trace = drive(mon, rounds)
    assert mon.assigned == [("dmr" if b == 3 else "ysf" if b == 20 else None) for b in range(B)]
    for b in busy:
        assert segs[b][0]["start"] == 0
        f, e = check(ctx, segs[b][0])
        assert len(e) and len(f)
    assert (mon.scanner.stats()["hits"][[b for b in range(B) if b not in busy]] == 0).all()
    mon.close()


def test_assigned_channels_are_not_scanned(ctx, rows7):
    x = np.ascontiguousarray(rows7[[1, 5], :6 * PUSH])        # YSF is named in the third round
    mon = api.Monitor(2, PUSH, ctx=ctx)
    seen = []

    def after(k):
        seen.append((mon.assigned[0], mon.scanner.stats()[0].tobytes()))
    drive(mon, [(c, None) for c in chunks(x)], after_round=after)
    assert mon.assigned == ["ysf", None]
    i = [a for a, _ in seen].index("ysf")
    assert i >= 1 and seen[i - 1][1] != seen[i][1]            # the statistics moved while the channel was scanned ...
    assert len({s for _, s in seen[i:]}) == 1 and len(seen) - i >= 3      # ... and not once since
    idle = np.zeros(9, api.SCAN_STAT_DTYPE)
    idle["best_dist"] = 255
    assert seen[-1][1] == idle.tobytes()
    mon.close()


# ----------------------------------------------------------------------------- end to end through the channelizer
E2E_SEED = 7


def _scene(device):
    D, seconds = 10, 1.5
    rate = 48000.0 * D
    n = int(seconds * rate)
    dmr, meta = wideband.dmr_audio(101, n_calls=1)
    ysf = wideband.ysf_audio(102, 30)
    raster = [-12500.0, 0.0, 12500.0]
    x = wideband.composite(D, [(raster[0] + 60.0, 0.0, dmr), (raster[1] - 40.0, -6.0, ysf)], n, seed=E2E_SEED, device=device,
                           keying=[(0.2, seconds), (0.4, seconds)])
    return D, rate, raster, x, meta


def test_end_to_end_through_the_channelizer(ctx):
    """a DMR carrier keyed on at 0.2 s, a YSF carrier at 0.4 s and an empty channel, 1.5 s at 480 kS/s.  The squelch as in
    tests/test_channelizer_power.py: blocks of 480, hang 2, pushes of 4 807 outputs, the open level 3 dB below the weakest
    block of a keyed carrier and the close level 3 dB below that, the scene asserted to leave 8 dB between the weakest keyed
    block and the strongest block of the empty row -- the powers taken from a first, ungated pass."""
    L, hang, P = 480, 2, 4807
    D, rate, raster, x, meta = _scene("cpu")                  # (one fixture for both tiers: the noise is the CPU generator's)
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
    print("monitor scene: weakest keyed block %.1f dBFS, strongest block of the empty row %.1f dBFS" % (db(min_keyed), db(max_empty)))
    assert db(min_keyed) - db(max_empty) >= 8.0, "the scene does not meet the test's precondition"
    open_db = db(min_keyed) - 3.0
    cz.reset()
    cz.enable_power(block=L, open_db=open_db, close_db=open_db - 3.0, hang_blocks=hang)

    mon = api.Monitor(3, cz.out_stride, depth=96000, lead=480, ctx=ctx)
    hist, counts, fed = [], [], {}
    blocks, total = [], 0
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
    assert first_open[0] <= 9600 + 2 * P and first_open[1] <= 19200 + 2 * P and first_open[0] < first_open[1]
    for b, name in ((0, "dmr"), (1, "ysf")):
        assert mon.start[b] == first_open[b] - 480             # the decoder began `lead` samples before the squelch opened
        seg = dict(proto=name, frames=[blk_["frames"] for blk_ in blocks if blk_["channel"] == b],
                   events=[blk_["events"] for blk_ in blocks if blk_["channel"] == b], fed=fed[b], at=[])
        f, e = check(ctx, seg)
        assert len(e) and len(f)
        if b == 0:
            lcs = [api.parse_lc(p) for p in e[e["type"] == EV_DMR_LC]["payload"]]
            assert lcs, "no LC"
            assert all(l["source"] == meta["src"] and l["target"] == meta["dst"] for l in lcs), "wrong ids"
    assert not [blk_ for blk_ in blocks if blk_["channel"] == 2]
    mon.close()
    cz.close()
