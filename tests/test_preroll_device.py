"""dh_preroll_gather_device / Preroll.gather_device: the gather with `from` on the device already, held to
dh_preroll_gather (rows as uint32 words, counts) for the `from` patterns of tests/test_preroll.py: the middle of a ring that
has wrapped, one sample on, before the oldest sample (clamped), not wanted, beyond the end, the very end."""
import ctypes as C

import numpy as np
import pytest

from digiham_amd import _capi
from digiham_amd import api
from test_preroll import NONE, append_slice, host, words

SENTINEL = 0x7FC0FFEE


@pytest.mark.parametrize("max_n", [1, 64, 1000])
def test_gather_device_equals_gather(ctx, max_n):
    B, depth = 6, 1003
    rng = np.random.default_rng(17)
    pre = api.Preroll(B, depth, ctx=ctx)
    for n in (700, 700, 700, 700, 701):                      # the ring has wrapped three times
        append_slice(ctx, pre, words(rng, (B, 800)), n, offset=3)
    total = pre.total
    back = 130 if max_n == 1 else 777
    from_ = np.array([total - back, total - back + 1, 5, NONE, total + 9, total], np.uint64)
    from_dev = ctx.mem.from_numpy(from_)
    fresh = lambda: ctx.mem.from_numpy(np.full((B, max_n + 3), SENTINEL, np.uint32).view(np.float32))
    skip, delivered = 0, 0
    while True:
        rows, counts, _ = pre.gather(from_, skip, max_n, out=fresh())
        want, want_cnt = host(ctx, rows, np.uint32).copy(), host(ctx, counts, np.uint32).copy()
        rows, counts = pre.gather_device(from_dev, skip, max_n, out=fresh())
        got, cnt = host(ctx, rows, np.uint32), host(ctx, counts, np.uint32)
        assert cnt.tolist() == want_cnt.tolist(), skip
        assert got.tobytes() == want.tobytes(), skip          # the sentinels beyond the counts and in unwanted rows included
        delivered += int(cnt.sum())
        if not cnt.any():
            break
        skip += max_n
    assert delivered == back + (back - 1) + depth             # channels 0, 1 and the clamped 2; nothing from 3, 4, 5
    for skip in ((1 << 64) - 1, 1 << 63):                     # skips that start + skip cannot hold: nothing
        rows, counts = pre.gather_device(from_dev, skip, max_n, out=fresh())
        assert not host(ctx, counts, np.uint32).any() and (host(ctx, rows, np.uint32) == SENTINEL).all()
    pre.close()


def test_errors(ctx):
    lib, mem = ctx.lib, ctx.mem
    pre = api.Preroll(4, 10, ctx=ctx)
    rows, cnt = mem.zeros((4, 8), np.float32), mem.zeros((4,), np.uint32)
    fd = mem.from_numpy(np.zeros(4, np.uint64))
    null = None
    bad = [lib.dh_preroll_gather_device(pre._h, mem.ptr(fd), 0, 8, mem.ptr(rows), 7, mem.ptr(cnt)),      # out_stride < max_n
           lib.dh_preroll_gather_device(pre._h, null, 0, 8, mem.ptr(rows), 8, mem.ptr(cnt)),
           lib.dh_preroll_gather_device(pre._h, mem.ptr(fd), 0, 8, null, 8, mem.ptr(cnt)),
           lib.dh_preroll_gather_device(pre._h, mem.ptr(fd), 0, 8, mem.ptr(rows), 8, null),
           lib.dh_preroll_gather_device(null, mem.ptr(fd), 0, 8, mem.ptr(rows), 8, mem.ptr(cnt))]
    assert bad == [_capi.DH_EINVAL] * len(bad)
    assert lib.dh_preroll_gather_device(pre._h, null, 0, 0, null, 0, null) == 0      # max_n = 0 needs no pointers
    with pytest.raises(ValueError):
        pre.gather_device(np.zeros(5, np.uint64), 0, 4)
    pre.close()
