"""What the decoder tests share (test_dmr_*.py, test_ysf_elements.py, test_nxdn*.py, test_dstar*.py, test_pocsag*.py, test_elements.py,
test_chain.py, test_cli_meta.py, test_meta_oracle.py): symbol rows through a decoder-only engine.  The push loop is stated once, as
data (push_plan, push_buffer) plus one iterator (SymbolRun); around it the tier switch, the oracle's expectation, the comparison
with its account of the first difference, and the fixtures of the whole-frame tests."""
import os

import numpy as np

from digiham_amd import api


# ---- the tiers -------------------------------------------------------------------------------------------------------------
def is_emu(ctx):
    """the CPU wave emulation (host memory), not the device"""
    return type(ctx.mem).__name__ == "NumpyMemory"


def tier(ctx, full, small):
    """`full` on the device, `small` on the emulation"""
    return small if is_emu(ctx) else full


# ---- the pushes as data ----------------------------------------------------------------------------------------------------
def push_plan(lengths, sizes, cycle=False):
    """lengths[b]: symbols in channel b's row.  sizes: None (one push of everything), an int (every push), or a sequence taken in order
    -- repeated with `cycle`, else the run ends where it runs out, pushed or not.  A channel brings min(size, what its row has left);
    a size of zero still makes a push.  -> [(lo, counts [B] uint32)] per push"""
    lengths = np.asarray(lengths, np.int64)
    n = int(lengths.max())
    if sizes is None or isinstance(sizes, (int, np.integer)):
        sizes, cycle = [n if sizes is None else int(sizes)], True
        assert sizes[0] > 0 or n == 0
    plan, lo = [], 0
    while lo < n and (cycle or len(plan) < len(sizes)):
        size = int(sizes[len(plan) % len(sizes)])
        plan.append((lo, np.clip(lengths - lo, 0, size).astype(np.uint32)))
        lo += size
    return plan


def push_buffer(rows, lo, counts, pitch=None, aligned=False):
    """The uint8 array handed to push_symbols: rows[b][lo:lo + counts[b]] in row b of a zero-filled [B][pitch] block; pitch None: the
    contiguous [B][m] slice, m the push's size.  aligned: the block's first row starts at a multiple of 16 bytes (it has a meaning on
    host memory only).  rows: [B][n], or B rows of unequal length.
    The slice of an array that is contiguous as it lies -- a single row, or all of every row -- is that memory, not a copy: on host
    memory a one-channel run in pushes of an odd size hands the decoder every address modulo 16."""
    B, m = len(rows), int(max(counts))
    if pitch is None:
        assert m > 0, "a push of no symbols needs a pitch"
        if isinstance(rows, np.ndarray) and not aligned:
            buf = np.ascontiguousarray(rows[:, lo:lo + m], np.uint8)
            return buf if buf.flags.writeable else buf.copy()          # (torch.from_numpy warns about a read-only array)
        pitch = m
    raw = np.zeros(B * pitch + 16, np.uint8)
    off = (-raw.ctypes.data) & 15 if aligned else 0
    buf = raw[off:off + B * pitch].reshape(B, pitch)
    for b, c in enumerate(counts):
        buf[b, :c] = rows[b][lo:lo + int(c)]
    return buf


# ---- the run ---------------------------------------------------------------------------------------------------------------
class SymbolRun:
    """A decoder-only engine (rrc and demod "none") of len(rows) channels and the pushes of push_plan(row lengths, sizes, cycle), each
    laid out by push_buffer(pitch, aligned).  Iterating makes the pushes: `for k in run` hands over after push k is synced (sync()
    raises when it ran into the event or frame capacity) and its frames and events are collected, so the body of the `with` block in
    front of the loop is "before push 0" and the loop's body "after push k, before push k + 1"; `eng` is there to read or set.
    Leaving the block closes the engine.  capacity: the engine's max_samples (default: the pitch, else max(largest size, 64));
    env: {name: value or None} set in os.environ while the engine is created (the library reads DH_DMR_SCALAR_PASS_B there).
    -> frames[b] / events[b] (uint8 / api.EVENT_DTYPE, concatenated), frames_by_push[b][k] / events_by_push[b][k], results"""

    def __init__(self, ctx, proto, rows, sizes=None, capacity=None, pitch=None, aligned=False, cycle=False, env=None, **engine_kw):
        self.rows, self.pitch, self.aligned = rows, pitch, aligned
        self.plan = push_plan([len(r) for r in rows], sizes, cycle)
        if capacity is None:
            largest = max(len(r) for r in rows) if sizes is None else int(np.max(sizes))
            capacity = max(largest, 64) if pitch is None else pitch
        self.frames_by_push, self.events_by_push = [[] for _ in rows], [[] for _ in rows]
        saved = {k: os.environ.get(k) for k in env or {}}
        try:
            _set_env(env or {})
            self.eng = api.Engine(len(rows), capacity, rrc="none", demod="none", proto=proto, ctx=ctx, **engine_kw)
        finally:
            _set_env(saved)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()

    def __iter__(self):
        for k, (lo, counts) in enumerate(self.plan):
            self.eng.push_symbols(push_buffer(self.rows, lo, counts, self.pitch, self.aligned), counts)
            self.eng.sync()
            (f, fc), (e, ec) = self.eng.frames(), self.eng.events()
            for b in range(len(self.rows)):
                self.frames_by_push[b].append(f[b, :fc[b]].copy())
                self.events_by_push[b].append(e[b, :ec[b]].copy())
            yield k

    frames = property(lambda self: [np.concatenate(p) for p in self.frames_by_push])
    events = property(lambda self: [np.concatenate(p) for p in self.events_by_push])
    results = property(lambda self: list(zip(self.frames, self.events)))


def _set_env(env):
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def run_symbols(ctx, proto, rows, sizes=None, **kw):
    """a SymbolRun with all its pushes made, closed"""
    with SymbolRun(ctx, proto, rows, sizes, **kw) as run:
        for _ in run:
            pass
    return run


def run_dmr_pass_b(ctx, rows, sizes, scalar, **kw):
    """A DMR run whose pass B goes lane-parallel where a chunk allows it or, with `scalar`, burst after burst throughout
    -> the run, and per push the chunks counted as (lane-parallel [B], burst-serial [B]): int64 [pushes][2][B]"""
    seen, counts = np.zeros((2, len(rows)), np.int64), []
    with SymbolRun(ctx, "dmr", rows, sizes, env={"DH_DMR_SCALAR_PASS_B": "1" if scalar else None}, **kw) as run:
        for _ in run:
            now = np.stack([a.astype(np.int64) for a in run.eng.dmr_pass_b_stats()])
            counts.append(now - seen)
            seen = now
    return run, np.stack(counts)


# ---- what to expect, and whether it came -----------------------------------------------------------------------------------
def expected(oracle, proto, rows):
    """-> [(output bytes, events)] per row, from a fresh oracle decoder each"""
    return [oracle.Decoder(proto).process(r) for r in rows]


def first_differing(got, want):
    """index of the first event at which two event arrays part; None: at none that both have"""
    return next((i for i in range(min(len(got), len(want))) if got[i].tobytes() != want[i].tobytes()), None)


def first_differing_frame(got, want, lead, length):
    """the frame of the expected event at which they part, for frames of `length` symbols from symbol `lead` on (None as above)"""
    i = first_differing(got, want)
    return i if i is None else (int(want[i]["sym_index"]) - lead) // length


def first_difference(got, want):
    """a readable account of where two event arrays part (for assertion messages)"""
    i = first_differing(got, want)
    return "%d events, expected %d" % (len(got), len(want)) if i is None else "event %d: got %s, expected %s" % (i, got[i], want[i])


def assert_rows(got, want, what=""):
    """got: a SymbolRun or [(output bytes, events)] per channel; holds every channel's bytes and events to want's.  what: one text,
    or one per channel."""
    got = getattr(got, "results", got)
    assert len(got) == len(want), "%s: %d channels, expected %d" % (what, len(got), len(want))
    for b, ((go, ge), (wo, we)) in enumerate(zip(got, want)):
        at = "%s channel %d" % (what if isinstance(what, str) else what[b], b)
        assert ge.tobytes() == we.tobytes(), "%s: %s" % (at, first_difference(ge, we))
        go, wo = np.asarray(go, np.uint8), np.asarray(wo, np.uint8)
        m = min(len(go), len(wo))
        differ = np.flatnonzero(go[:m] != wo[:m])
        assert len(go) == len(wo) and not len(differ), "%s: %d output bytes, expected %d; first difference at byte %d" % (
            at, len(go), len(wo), differ[0] if len(differ) else m)


# ---- whole frames through a decoder-only engine (D-Star, POCSAG) ---------------------------------------------------------------
def frames_fixture():
    """tests/golden/frames_ref.npz (make_golden_frames.py): damaged D-Star radio headers and POCSAG codewords with what the
    reference's Header::parseFromHeader / Codeword::parse made of them"""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_ref.npz")) as z:
        return {k: z[k] for k in z.files}


def event_record(sym_index, typ, a=0, b=0, payload=b""):
    """one expected decoder event (api.EVENT_DTYPE), payload zero padded as dh_emit pads it"""
    e = np.zeros(1, api.EVENT_DTYPE)
    e["sym_index"], e["type"], e["a"], e["b"], e["len"] = sym_index, typ, a, b, len(payload)
    e["payload"][0, :len(payload)] = np.frombuffer(bytes(payload), np.uint8)
    return e


def stack_rows(rows):
    """rows of unequal length -> [B][n] uint8, zero padded"""
    n = max(len(r) for r in rows)
    return np.stack([np.concatenate([r, np.zeros(n - len(r), np.uint8)]) for r in rows]).astype(np.uint8)
