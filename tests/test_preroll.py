"""dh_preroll / api.Preroll: the per-channel history ring against a numpy model of the text in include/digiham_amd.h
("Pre-roll").  Samples are compared as uint32 words: the ring moves bits, so NaN payloads, -0, subnormals and
infinities have to come back as they went in."""
import ctypes as C

import numpy as np
import pytest

from digiham_amd import _capi, api

NONE = _capi.PREROLL_NONE
NONE64 = np.uint64(NONE)
SPECIAL = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0], np.uint32)


def words(rng, shape):
    """random 32-bit patterns (every class of float among them) with the named special values sprinkled in"""
    w = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    pick = rng.random(shape) < 0.2
    w[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
    return w


class Model:
    """the header text, restated: whole streams are kept, the ring is what may be read of them"""

    def __init__(self, B, depth):
        self.B, self.depth = B, depth
        self.reset()

    def reset(self):
        self.x = np.zeros((self.B, 0), np.uint32)
        self.open_at = np.full(self.B, NONE, np.uint64)

    @property
    def total(self):
        return self.x.shape[1]

    @property
    def oldest(self):
        return self.total - self.depth if self.total > self.depth else 0

    def append(self, rows, counts=None):
        n = rows.shape[1]
        if n == 0:
            return
        base = self.total
        for b in range(self.B):
            if counts is None or counts[b] != 0:
                if int(self.open_at[b]) == NONE:
                    self.open_at[b] = base
            else:
                self.open_at[b] = NONE
        self.x = np.concatenate([self.x, rows], axis=1)

    def gather(self, from_, skip, max_n):
        out, start = [], []
        for b in range(self.B):
            if int(from_[b]) == NONE:
                out.append(None); start.append(NONE)
                continue
            s = max(int(from_[b]), self.oldest)
            first = s + skip
            count = min(max_n, self.total - first) if first < self.total else 0
            out.append(self.x[b, first:first + count]); start.append(s)
        return out, np.array(start, np.uint64)


def host(ctx, t, dtype):
    return np.array(ctx.mem.to_numpy(t)).view(dtype)


def append_slice(ctx, pre, w, n, counts=None, offset=1):
    """w [B][stride] words -> a device array; the append reads its columns [offset, offset + n): rows that start at an odd word"""
    base = ctx.mem.from_numpy(w.view(np.float32))
    pre.append(base[:, offset:offset + n], n=n, counts=counts)
    return w[:, offset:offset + n]


def check_gather(ctx, pre, m, from_, skip, max_n, sentinel=0x7FC0FFEE):
    out = ctx.mem.from_numpy(np.full((pre.B, max(max_n, 1) + 3), sentinel, np.uint32).view(np.float32))
    rows, counts, start = pre.gather(from_, skip, max_n, out=out)
    got, cnt = host(ctx, rows, np.uint32), host(ctx, counts, np.uint32)
    want, want_start = m.gather(from_, skip, max_n)
    assert start.tolist() == want_start.tolist()
    for b in range(pre.B):
        k = 0 if want[b] is None else len(want[b])
        assert cnt[b] == k, (b, cnt[b], k)
        assert (got[b, :k] == want[b]).all() if k else True, b
        assert (got[b, k:] == sentinel).all(), b              # nothing beyond the count, nothing at all in an unwanted row
    return want


@pytest.mark.parametrize("depth", [1000, 1003])
def test_ring_contents(ctx, depth):
    B, stride = 5, 2501
    rng = np.random.default_rng(depth)
    pre, m = api.Preroll(B, depth, ctx=ctx), Model(B, depth)
    assert pre.total == 0 and (pre.open_at() == np.uint64(NONE)).all()
    for n in (1, 7, 256, 999, 1000, 1001, 2500, 0, 64):
        m.append(append_slice(ctx, pre, words(rng, (B, stride)), n))
        assert pre.total == m.total
        want = check_gather(ctx, pre, m, np.zeros(B, np.uint64), 0, depth)
        for b in range(B):
            assert len(want[b]) == min(m.total, depth) and (want[b] == m.x[b, -min(m.total, depth):]).all()
    pre.close()


@pytest.mark.parametrize("max_n", [1, 63, 64, 1000])
def test_chunks_and_the_seam(ctx, max_n):
    B, depth = 6, 1000
    rng = np.random.default_rng(7)
    pre, m = api.Preroll(B, depth, ctx=ctx), Model(B, depth)
    for n in (700, 700, 700, 700, 701):                      # the ring has wrapped three times; the seam sits at 501
        m.append(append_slice(ctx, pre, words(rng, (B, 800)), n, offset=3))
    total = m.total
    back = 130 if max_n == 1 else 777
    # the middle, the middle again one sample on, before the oldest sample (clamped), not wanted, beyond the end, the very end
    from_ = np.array([total - back, total - back + 1, 5, NONE, total + 9, total], np.uint64)
    parts = [[] for _ in range(B)]
    skip = 0
    while True:
        want = check_gather(ctx, pre, m, from_, skip, max_n)
        if not any(w is not None and len(w) for w in want):
            break
        for b in range(B):
            if want[b] is not None:
                parts[b].append(want[b])
        skip += max_n
    # what the chunks add up to is the stream from start on (the model's chunks were each compared with the ring's)
    for b, s in ((0, total - back), (1, total - back + 1), (2, total - depth)):
        assert (np.concatenate(parts[b]) == m.x[b, s:]).all()
    assert not parts[3] and not len(np.concatenate(parts[4])) and not len(np.concatenate(parts[5]))
    check_gather(ctx, pre, m, from_, (1 << 64) - 1, max_n)     # a skip that start + skip cannot hold: nothing
    pre.close()


def test_open_at(ctx):
    B, depth, n = 4, 300, 100
    rng = np.random.default_rng(3)
    pre, m = api.Preroll(B, depth, ctx=ctx), Model(B, depth)
    pattern = np.array([[0, n, n, 0, 0, n], [n, n, n, n, n, n], [0, 0, 0, 0, 0, 0], [7, 0, 1, 0, n, n]], np.uint32)
    for k in range(6):
        counts = np.ascontiguousarray(pattern[:, k])
        m.append(append_slice(ctx, pre, words(rng, (B, n + 2)), n, counts=counts), counts)
        assert pre.open_at().tolist() == m.open_at.tolist(), k
        if k == 2:                                            # an empty append changes nothing, whatever its counts say
            pre.append(ctx.mem.from_numpy(np.zeros((B, 4), np.float32)), n=0, counts=np.zeros(B, np.uint32))
            assert pre.total == m.total and pre.open_at().tolist() == m.open_at.tolist()
    assert m.open_at.tolist() == [500, 0, NONE, 400]
    m.append(append_slice(ctx, pre, words(rng, (B, n + 2)), n))              # NULL counts: every channel is open
    assert pre.open_at().tolist() == m.open_at.tolist() == [500, 0, 600, 400]
    check_gather(ctx, pre, m, pre.open_at(), 0, depth)
    pre.reset()
    m.reset()
    assert pre.total == 0 and (pre.open_at() == np.uint64(NONE)).all()
    m.append(append_slice(ctx, pre, words(rng, (B, n + 2)), 50))
    assert pre.open_at().tolist() == [0] * B
    check_gather(ctx, pre, m, np.zeros(B, np.uint64), 0, depth)
    pre.close()


def test_channels_beyond_one_turn_of_grid_y(ctx):
    """The channels of an append or a gather sit on grid.y, 65 535 workgroups at most, each looping b += gridDim.y.  65 536
    channels is the most dh_preroll_create takes (65 537 is refused: test_errors): workgroup 0 then takes a second turn, for
    channel 65 535 -- the only second turn there can be.  depth = 8, appends of 3: the ring wraps in every channel."""
    B, depth, n = 65536, 8, 3
    rng = np.random.default_rng(65536)
    pre, m = api.Preroll(B, depth, ctx=ctx), Model(B, depth)
    counts = (np.arange(B) % 3 != 1).astype(np.uint32) * n
    for k in range(4):
        c = None if k == 1 else np.roll(counts, k)
        m.append(append_slice(ctx, pre, words(rng, (B, n + 2)), n, counts=c), c)
        assert pre.total == m.total and (pre.open_at() == m.open_at).all(), k
    from_ = np.where(np.arange(B) % 5 == 2, NONE64, (np.arange(B) % 7).astype(np.uint64))
    from_[[0, B - 1]] = 5, 6
    check_gather(ctx, pre, m, from_, 0, depth)
    check_gather(ctx, pre, m, from_, 2, n)
    pre.close()


def test_errors(ctx):
    lib, mem = ctx.lib, ctx.mem
    for kw in (dict(n_channels=4, depth=0), dict(n_channels=0, depth=10), dict(n_channels=65537, depth=10), dict(n_channels=1, depth=(1 << 24) + 1)):
        with pytest.raises(_capi.DhError) as e:
            api.Preroll(ctx=ctx, **kw)
        assert e.value.code == _capi.DH_EINVAL
    h = C.c_void_p()
    cfg = _capi.PrerollConfig(C.sizeof(_capi.PrerollConfig) - 1, 0, 4, 10, mem.stream())
    assert lib.dh_preroll_create(C.byref(cfg), C.byref(h)) == _capi.DH_EINVAL
    assert lib.dh_preroll_create(None, C.byref(h)) == _capi.DH_EINVAL
    cfg.struct_size += 1
    assert lib.dh_preroll_create(C.byref(cfg), None) == _capi.DH_EINVAL

    pre = api.Preroll(4, 10, ctx=ctx)
    rows, cnt = mem.zeros((4, 8), np.float32), mem.zeros((4,), np.uint32)
    from_ = np.zeros(4, np.uint64)
    fp, null = from_.ctypes.data_as(C.c_void_p), None
    total = C.c_uint64(0)
    bad = [lib.dh_preroll_append(pre._h, mem.ptr(rows), 5, 6, null),                     # stride < n
           lib.dh_preroll_append(pre._h, null, 8, 6, null),
           lib.dh_preroll_append(null, mem.ptr(rows), 8, 6, null),
           lib.dh_preroll_gather(pre._h, fp, 0, 8, mem.ptr(rows), 7, mem.ptr(cnt), null),  # out_stride < max_n
           lib.dh_preroll_gather(pre._h, null, 0, 8, mem.ptr(rows), 8, mem.ptr(cnt), null),
           lib.dh_preroll_gather(pre._h, fp, 0, 8, null, 8, mem.ptr(cnt), null),
           lib.dh_preroll_gather(pre._h, fp, 0, 8, mem.ptr(rows), 8, null, null),
           lib.dh_preroll_gather(null, fp, 0, 8, mem.ptr(rows), 8, mem.ptr(cnt), null),
           lib.dh_preroll_total(pre._h, null), lib.dh_preroll_total(null, C.byref(total)),
           lib.dh_preroll_open_at(pre._h, null), lib.dh_preroll_open_at(null, fp), lib.dh_preroll_reset(null)]
    assert bad == [_capi.DH_EINVAL] * len(bad)
    assert pre.total == 0                                     # none of them appended anything
    # n = 0 and max_n = 0 need no pointers
    assert lib.dh_preroll_append(pre._h, null, 0, 0, null) == 0
    assert lib.dh_preroll_gather(pre._h, null, 0, 0, null, 0, null, null) == 0
    lib.dh_preroll_destroy(null)
    pre.close()


@pytest.mark.gpu
def test_every_channel_behind_the_grid_cap(gpu_ctx):
    """65 536 channels: more than one launch's grid.y holds, and a wrap in every workgroup"""
    ctx, B, depth = gpu_ctx, 65536, 100
    rng = np.random.default_rng(11)
    pre = api.Preroll(B, depth, ctx=ctx)
    a, b = words(rng, (B, 40)), words(rng, (B, 70))
    c1 = (np.arange(B) % 3 != 0).astype(np.uint32)
    c2 = (np.arange(B) % 5 != 0).astype(np.uint32) * 70
    pre.append(ctx.mem.from_numpy(a.view(np.float32)), counts=c1)
    pre.append(ctx.mem.from_numpy(b.view(np.float32)), counts=c2)
    assert pre.total == 110
    want_open = np.where(c2 == 0, NONE64, np.where(c1 != 0, 0, 40).astype(np.uint64))
    assert (pre.open_at() == want_open).all()
    from_ = np.zeros(B, np.uint64)
    from_[1::7] = NONE
    from_[2::7] = 60
    rows, counts, start = pre.gather(from_, 0, depth)
    got, cnt = host(ctx, rows, np.uint32), host(ctx, counts, np.uint32)
    x = np.concatenate([a, b], axis=1)
    want_start = np.where(from_ == NONE64, NONE64, np.maximum(from_, np.uint64(10)))
    assert (start == want_start).all()
    want_cnt = np.where(from_ == NONE64, 0, 110 - np.minimum(want_start, 110).astype(np.int64))
    assert (cnt == want_cnt).all()
    for s in (10, 60):
        sel = want_start == s
        assert (got[sel, :110 - s] == x[sel, s:]).all()
    assert (got[from_ == NONE64] == 0).all()                    # a fresh array of zeros, left alone
    pre.close()


@pytest.mark.gpu
def test_two_seconds_of_64_channels(gpu_ctx):
    ctx, B, depth, n = gpu_ctx, 64, 96000, 48000
    rng = np.random.default_rng(12)
    pre = api.Preroll(B, depth, ctx=ctx)
    parts = [words(rng, (B, n)) for _ in range(3)]
    for p in parts:
        pre.append(ctx.mem.from_numpy(p.view(np.float32)))
    x = np.concatenate(parts, axis=1)
    got = []
    for skip in (0, n, 2 * n):
        rows, counts, start = pre.gather(np.zeros(B, np.uint64), skip, n)
        cnt = host(ctx, counts, np.uint32)
        assert (start == n).all() and (cnt == (n if skip < 2 * n else 0)).all()
        got.append(host(ctx, rows, np.uint32)[:, :cnt[0]].copy())
    assert (np.concatenate(got, axis=1) == x[:, n:]).all()
    pre.close()
