"""The sps-10 window phase on the slicer's symbol pairs (dsp_core.hpp: dh_shift_symbol0, dh_symbol_windows, DhWinPair): lane l takes
symbols 2 l and 2 l + 1 of a run from one grid -- in the block behind a timing step symbol 0's ten samples are moved by the step first --
and hands its volumes and mid-symbol sums to the AGC scan and the slicing phase in registers when the run opens its block.

Full DMR chains (wide filter, sps 10) against the oracle, dibits, frame bytes and events bit for bit.  Channel 0 is nominal; channels
1 and 2 are the same signal resampled by +0.3 % and -0.3 %, channels 3 and 4 by +0.1 % and -0.1 %.  Pushes of 2 403, 1 000, 1 507, 13
and 997 samples, in turn: blocks that open in the middle of a push, runs with an odd first ring slot, runs of one symbol, of an odd
number of symbols and of one pair; then the same sizes ragged, every channel at another place of the list in the same launch.

What proves that the move ran for both signs is asserted on the oracle's output alone.  A drift of 0.3 % is three samples per
variance block and the loop steps one sample per block: it cannot follow, the sampling point wanders through the symbol and the
steps of BOTH signs occur in each of the two channels (the oracle on this input: 9 up / 14 down and 13 up / 8 down) -- while the
symbol count stays within one of samples / 10, so the count says nothing there.  Those channels are held to the oracle's own step
counters.  At 0.1 % the loop follows with one step per block, all of one sign, and the count shows it: channel 3 yields at least
two symbols more than samples / 10 and channel 4 at least two fewer.

One more case on the kernel that also delivers the filtered samples (DH_FLAG_KEEP_FILTERED | DH_FLAG_ONE_LAUNCH): it copies a run's
samples out BEFORE symbol 0 moves, so the floats stay within the flag's 2.5e-6 of the reference's and the dibits are the reference's.
"""
import numpy as np
import pytest

from common import assert_matches_oracle, rel_err, rel_err_per_channel, run_engine
from digiham_amd import api, synth

PUSHES = [2403, 1000, 1507, 13, 997]
DRIFT = [0.0, 3e-3, -3e-3, 1e-3, -1e-3]


def _signals():
    s = synth.shape(synth.dmr_stream(31, 20))
    chans = []
    for i, r in enumerate(DRIFT):
        t = np.arange(int((len(s) - 1) / (1.0 + abs(r))) - 2) * (1.0 + r)
        c = np.interp(t, np.arange(len(s)), s).astype(np.float32)
        chans.append(synth.impair(c, 40 + i, snr_db=30, delay=3 * i))
    n = min(len(c) for c in chans)
    return np.stack([c[:n] for c in chans])


@pytest.fixture(scope="module")
def case(oracle):
    x = _signals()
    ref = oracle.chain(x, proto=1)
    return x, ref, oracle.chain(x, proto=0, keep_filtered=True)


def test_the_streams_step_both_ways(case):
    x, ref, _ = case
    n = x.shape[1]
    up, down, count = ref["steps_up"].astype(np.int64), ref["steps_down"].astype(np.int64), ref["sym_count"].astype(np.int64)
    print("samples", n, "symbols", count, "steps up", up, "down", down)
    for b in (1, 2):
        assert up[b] >= 2 and down[b] >= 2, (b, up, down)
    assert count[3] >= n // 10 + 2, (count, n)
    assert count[4] <= n // 10 - 2, (count, n)
    assert int(ref["out_count"].sum()) > 0 and int(ref["event_count"].sum()) > 0


def test_pushes(ctx, case):
    x, ref, _ = case
    res = run_engine(ctx, x, "dmr", PUSHES, rrc="wide", sps=10)
    assert_matches_oracle(res, ref, len(x), "pushes %s" % PUSHES)


def test_ragged_pushes(ctx, case):
    """the same sizes through the per-channel counts: in launch i channel b brings PUSHES[(i + b) % 5] samples"""
    x, ref, _ = case
    B, n = x.shape
    cap = max(PUSHES)
    eng = api.Engine(B, cap, rrc="wide", sps=10, proto="dmr", ctx=ctx)
    acc = [[[] for _ in range(B)] for _ in range(3)]
    pos = np.zeros(B, np.int64)
    i = 0
    while (pos < n).any():
        cnt = np.array([min(PUSHES[(i + b) % len(PUSHES)], n - pos[b]) for b in range(B)], np.uint32)
        buf = np.full((B, cap), np.nan, np.float32)
        for b in range(B):
            buf[b, :cnt[b]] = x[b, pos[b]:pos[b] + cnt[b]]
        eng.push(buf, n=int(cnt.max()), counts=cnt)
        pos += cnt
        i += 1
        for k, (rows, counts) in enumerate((eng.symbols(), eng.frames(), eng.events())):
            for b in range(B):
                acc[k][b].append(rows[b, :counts[b]].copy())
    eng.close()
    res = {"syms": [np.concatenate(a) for a in acc[0]], "frames": [np.concatenate(a) for a in acc[1]],
           "events": [np.concatenate(a) for a in acc[2]]}
    assert_matches_oracle(res, ref, B, "ragged")


def test_delivered_floats_across_a_timing_step(ctx, case):
    x, _, ref = case
    res = run_engine(ctx, x, "none", PUSHES, rrc="wide", sps=10, keep_filtered=True, one_launch=True)
    assert res["filtered"].shape == ref["filtered"].shape
    err, err_ch = rel_err(res["filtered"], ref["filtered"]).max(), rel_err_per_channel(res["filtered"], ref["filtered"]).max()
    print("floats: %.3g overall, %.3g per channel" % (err, err_ch))
    assert err <= 2.5e-6 and err_ch <= 2.5e-6
    assert_matches_oracle(res, {"syms": ref["syms"], "sym_count": ref["sym_count"]}, x.shape[0], "one launch")
