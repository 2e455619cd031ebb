"""tests/dec_harness.py itself: the push plan and the pushed buffer as data, and what a failed comparison says (no engine, no oracle)."""
import numpy as np
import pytest

from dec_harness import assert_rows, event_record, first_differing_frame, push_buffer, push_plan


def _counts(plan):
    return [(lo, c.tolist()) for lo, c in plan]


def test_push_plan():
    assert _counts(push_plan((3, 10, 7), 4)) == [(0, [3, 4, 4]), (4, [0, 4, 3]), (8, [0, 2, 0])]
    cycled = _counts(push_plan((5, 12), [1, 7, 0, 3], cycle=True))
    assert cycled == [(0, [1, 1]), (1, [4, 7]), (8, [0, 0]), (8, [0, 3]), (11, [0, 1])]      # (a size of zero: a push all the same)
    assert _counts(push_plan((5, 12), [1, 7, 0, 3])) == cycled[:4]                           # runs out at 11 of 12: the run ends there
    assert _counts(push_plan((5, 12), None)) == [(0, [5, 12])]
    assert all(c.dtype == np.uint32 for _, c in push_plan((3, 10, 7), 4))


def test_assert_rows_says_where():
    want = [(np.arange(9, dtype=np.uint8), np.concatenate([event_record(29 + 480 * k, 16, a=k) for k in range(3)]))]
    assert_rows(want, want)
    late = want[0][1].copy()
    late["a"][2] = 7
    assert first_differing_frame(late, want[0][1], 29, 480) == 2 and first_differing_frame(late[:2], want[0][1], 29, 480) is None
    with pytest.raises(AssertionError, match="push 5 channel 0: event 2: got"):
        assert_rows([(want[0][0], late)], want, "push 5")
    with pytest.raises(AssertionError, match="2 events, expected 3"):
        assert_rows([(want[0][0], late[:2])], want)
    with pytest.raises(AssertionError, match="8 output bytes, expected 9; first difference at byte 8"):
        assert_rows([(want[0][0][:8], want[0][1])], want, ["one text per channel"])


def test_push_buffer():
    rows = np.arange(1, 31, dtype=np.uint8).reshape(3, 10)
    buf = push_buffer(rows, 4, [4, 4, 4])
    assert buf.shape == (3, 4) and buf.dtype == np.uint8 and buf.flags.c_contiguous and (buf == rows[:, 4:8]).all()
    ragged = [rows[0, :3], rows[1], rows[2, :7]]
    (lo, counts), = push_plan((3, 10, 7), 4)[1:2]
    for aligned in (False, True):
        buf = push_buffer(ragged, lo, counts, pitch=9, aligned=aligned)
        assert buf.shape == (3, 9) and buf.flags.c_contiguous and buf.strides == (9, 1)
        assert not buf[0].any() and (buf[1, :4] == rows[1, 4:8]).all() and not buf[1, 4:].any()
        assert (buf[2, :3] == rows[2, 4:7]).all() and not buf[2, 3:].any()
    assert buf.ctypes.data % 16 == 0 and buf[1].ctypes.data % 16 == 9                        # an odd pitch: row 1 is not aligned
    zero = push_buffer(rows, 8, [0, 0, 0], pitch=64)
    assert zero.shape == (3, 64) and not zero.any()
    with pytest.raises(AssertionError):
        push_buffer(rows, 8, [0, 0, 0])
