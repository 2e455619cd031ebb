"""dh_engine_reset_channels / Engine.reset_channels: the masked reset of many channels in one launch, held to
dh_engine_reset_channel channel by channel.

Twin engines get the same 2 400 samples per channel; one twin then has six channels reset one call at a time, the other
the same six with one reset_channels; after 2 400 more samples everything a caller can read of all 300 channels -- symbols,
frames, events, every count, the slicer header words 0-31 and the decoder state words 100-163 of debug_header -- is the
same byte for byte.  A third twin gets all-zero flags: its channels go on as if nothing had been called -- the ones no
twin reset equal the first twin's, and the six equal a small engine that was never reset (a channel's output does not
depend on how many channels the engine has).  300 channels: more than one workgroup of channels for every kernel shape,
and no multiple of 64."""
import numpy as np
import pytest

from digiham_amd import api
from test_scan import FRONTS, rows7      # noqa: F401  (fixture)

B, N = 300, 2400
FLAGGED = [0, 63, 64, 255, 256, 299]
# engine kind -> (proto, front end, the rows of rows7 its channels carry)
KINDS = {"dmr": ("dmr", "wide10", [0]), "ysf": ("ysf", "wide10", [1]), "nxdn": ("nxdn", "narrow20", [2]), "dstar": ("dstar", "fsk10", [3]),
         "pocsag": ("pocsag", "fsk40i", [4]), "scan": ("scan", "wide10", [0, 1, 2, 3, 4]), "none": ("none", "wide10", [0])}


def signal(rows7, which):
    """[B][2 N]: channel b carries row which[b % len] of rows7 from an offset of its own"""
    return np.stack([np.roll(rows7[which[b % len(which)]], -(977 * b + 4800))[:2 * N] for b in range(B)]).astype(np.float32)


def snapshot(eng, proto):
    out = {}
    s, sc = eng.symbols()
    out["symbols"], out["symbol counts"] = s.tobytes(), sc.tobytes()
    valid = lambda rows, cnt: b"".join(rows[b, :cnt[b]].tobytes() for b in range(rows.shape[0]))
    if proto != "none":
        f, fc = eng.frames()
        e, ec = eng.events()
        out["frames"], out["frame counts"], out["events"], out["event counts"] = valid(f, fc), fc.tobytes(), valid(e, ec), ec.tobytes()
        out["decoder state"] = np.stack([eng.debug_header(w) for w in range(100, 164)]).tobytes()
    out["slicer header"] = np.stack([eng.debug_header(w) for w in range(32)]).tobytes()
    return out


def per_channel(eng, proto):
    """what snapshot() compares, as arrays indexed by channel (for comparing subsets of channels)"""
    out = {}
    s, sc = eng.symbols()
    out["symbols"], out["symbol counts"] = [s[b, :sc[b]].tobytes() for b in range(eng.B)], list(sc)
    if proto != "none":
        f, fc = eng.frames()
        e, ec = eng.events()
        out["frames"] = [f[b, :fc[b]].tobytes() for b in range(eng.B)]
        out["events"] = [e[b, :ec[b]].tobytes() for b in range(eng.B)]
        dec = np.stack([eng.debug_header(w) for w in range(100, 164)], axis=1)
        out["decoder state"] = [dec[b].tobytes() for b in range(eng.B)]
    hdr = np.stack([eng.debug_header(w) for w in range(32)], axis=1)
    out["slicer header"] = [hdr[b].tobytes() for b in range(eng.B)]
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_masked_reset_equals_reset_channel(ctx, rows7, kind):
    proto, front, which = KINDS[kind]
    x = signal(rows7, which)
    first, second = np.ascontiguousarray(x[:, :N]), np.ascontiguousarray(x[:, N:])
    make = lambda n: api.Engine(n, N, proto=proto, ctx=ctx, **FRONTS[front])
    one, masked, idle, never = make(B), make(B), make(B), make(len(FLAGGED))
    for eng in (one, masked, idle):
        eng.push(first)
    never.push(np.ascontiguousarray(first[FLAGGED]))
    for b in FLAGGED:
        one.reset_channel(b)
    flags = np.zeros(B, np.uint8)
    flags[FLAGGED] = 1
    masked.reset_channels(flags)
    idle.reset_channels(np.zeros(B, np.uint8))
    # right after the resets: the state words of the twins agree, and all-zero flags changed none
    a, m = snapshot(one, proto), snapshot(masked, proto)
    for key in ("slicer header", "decoder state"):
        if key in a:
            assert a[key] == m[key], (kind, key, "after the reset")
    for eng in (one, masked, idle):
        eng.push(second)
    never.push(np.ascontiguousarray(second[FLAGGED]))
    a, m = snapshot(one, proto), snapshot(masked, proto)
    for key in a:
        assert a[key] == m[key], (kind, key)
    assert sum(np.frombuffer(a["symbol counts"], np.uint32)) > 0
    pa, pi, pn = per_channel(one, proto), per_channel(idle, proto), per_channel(never, proto)
    rest = [b for b in range(B) if b not in FLAGGED]
    for key in pa:
        assert [pi[key][b] for b in rest] == [pa[key][b] for b in rest], (kind, key, "unflagged channels")
        assert [pi[key][b] for b in FLAGGED] == pn[key], (kind, key, "all-zero flags")
    if kind in ("dmr", "ysf", "nxdn"):          # the reset was no no-op: a reset channel lost its sync and its place in the stream
        assert [pa["decoder state"][b] for b in FLAGGED] != pn["decoder state"]
    for eng in (one, masked, idle, never):
        eng.close()


def test_errors(ctx):
    eng = api.Engine(4, 100, proto="dmr", ctx=ctx)
    assert ctx.lib.dh_engine_reset_channels(eng._h, None) == -1
    assert ctx.lib.dh_engine_reset_channels(None, ctx.mem.ptr(ctx.mem.zeros((4,), np.uint8))) == -1
    with pytest.raises(ValueError):
        eng.reset_channels(np.zeros(5, np.uint8))
    eng.close()
