"""The two ends of a push in the chain kernels (dsp_core.hpp: dh_rrc_demod_channel).  The prologue fetches header, volume ring, variance
ring and taps in one batch of loads; the epilogue writes the raw tail back as whole 16-byte groups straight from the input row when the
push is longer than the tail, the last group being the last four samples wherever they start, and element by element through LDS when
the tail still reaches into the old one.  Full chains against the oracle with push lengths that take both routes in turn and leave
tails of every length modulo four: long pushes of odd sizes (the tail of the sps-10 kernels is up to 1 408 samples, one pass of groups;
of the sps-20 kernel 2 408, two passes), pushes shorter than a tail and pushes of a few samples between them.  Dibits, frame bytes and
events bit for bit.

The same write-back is what a part of a split push hands to the next part, or to the fix-up launch (engine.hip: k_chain, DH_TAIL_SPLIT).
The hand-over cases: 16 DMR and 16 YSF channels in two pushes of 70 000 samples with the later parts starting at 50 % and at 70 % + 92 %,
the same with every third channel's hand-over failing (DH_TAIL_SPLIT_FORCE_FAIL=3), ragged pushes with rows that end in front of, at and
behind the split point, and a part boundary swept sample by sample through a variance block of channels whose symbol clock drifts, so
that a timing step of +1 or -1 is pending across it.  The wave emulation splits at any size.  The device splits launches of at least
8 192 channels and 65 536 samples only: there the 16-channel cases run unsplit, and test_hand_over_on_a_launch_that_splits repeats them
8 208 channels wide, where debug word 202 shows that the fix-up launch really finished rows.
"""
import hashlib

import numpy as np
import pytest

from common import assert_matches_oracle, make_channels, run_engine
from digiham_amd import _taps, api, synth

CHUNKS = [[3001, 1409, 2, 1407, 700, 5, 4098, 1411], [1999, 1, 1, 2003, 3, 1410, 4101], [6007, 97, 1408, 2999]]
IDS = ["a", "b", "c"]


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}
    for proto, code in (("dmr", 1), ("ysf", 2)):
        x = make_channels(proto, [51, 52, 53, 54], 10 if proto == "dmr" else 6)[:, :14000].copy()
        assert x.shape[1] == 14000
        out[proto] = (x, oracle.chain(x, proto=code))
    chans = []
    for i, seed in enumerate((61, 62, 63)):
        s = synth.shape(synth.nxdn_stream(seed, 3), sps=20, taps=_taps.narrow())
        chans.append(synth.impair(s, seed, snr_db=[None, 22, 16][i], dc=[0, 0.1, -0.2][i], delay=7 * i, gain=[1, 0.5, 1.7][i]))
    n = min(min(len(c) for c in chans), 14000)
    x = np.stack([c[:n] for c in chans])
    out["nxdn"] = (x, oracle.chain(x, rrc=2, sps=20, proto=3))
    return out


@pytest.mark.parametrize("chunks", CHUNKS, ids=IDS)
@pytest.mark.parametrize("proto", ["dmr", "ysf"])
def test_wide_filter_chains(ctx, cases, proto, chunks):
    x, ref = cases[proto]
    res = run_engine(ctx, x, proto, chunks)
    assert_matches_oracle(res, ref, len(x), "%s %s" % (proto, chunks))
    assert int(ref["sym_count"].min()) > 1000


@pytest.mark.parametrize("chunks", CHUNKS, ids=IDS)
def test_nxdn_chain(ctx, cases, chunks):
    x, ref = cases["nxdn"]
    res = run_engine(ctx, x, "nxdn", chunks, rrc="narrow", sps=20)
    assert_matches_oracle(res, ref, len(x), "nxdn %s" % chunks)
    assert int(ref["sym_count"].min()) > 500


# ------------------------------------------------------------------ the hand-over between the parts of a split push
HN = 70000                                          # samples per push
SPLITS = ["50", "70,92"]


@pytest.fixture(scope="module")
def handover(oracle):
    out = {}
    for proto, code, units in (("dmr", 1, 100), ("ysf", 2, 31)):
        x = make_channels(proto, list(range(71, 87)), units)[:, :2 * HN].copy()
        assert x.shape == (16, 2 * HN)
        out[proto] = (x, oracle.chain(x, proto=code, threads=8))
    return out


def _split_env(monkeypatch, split, fail):
    monkeypatch.setenv("DH_TAIL_SPLIT", split)
    if fail:
        monkeypatch.setenv("DH_TAIL_SPLIT_FORCE_FAIL", "3")
    else:
        monkeypatch.delenv("DH_TAIL_SPLIT_FORCE_FAIL", raising=False)


def _push_counts(eng, cap, x, pos, cnt, acc):
    """one ragged push: channel b brings x[b, pos[b] : pos[b] + cnt[b]]"""
    B = len(x)
    cnt = np.asarray(cnt, np.uint32)
    buf = np.full((B, cap), np.nan, np.float32)
    for b in range(B):
        buf[b, :cnt[b]] = x[b, pos[b]:pos[b] + cnt[b]]
    eng.push(buf, n=int(cnt.max()), counts=cnt)
    pos += cnt
    for k, (rows, counts) in enumerate((eng.symbols(), eng.frames(), eng.events())):
        for b in range(B):
            acc[k][b].append(rows[b, :counts[b]].copy())


def _assert_acc(acc, ref, B, what):
    res = {"syms": [np.concatenate(a) for a in acc[0]], "frames": [np.concatenate(a) for a in acc[1]],
           "events": [np.concatenate(a) for a in acc[2]]}
    assert_matches_oracle(res, ref, B, what)


@pytest.mark.parametrize("fail", [False, True], ids=["", "fail3"])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("proto", ["dmr", "ysf"])
def test_hand_over(ctx, handover, monkeypatch, proto, split, fail):
    x, ref = handover[proto]
    _split_env(monkeypatch, split, fail)
    res = run_engine(ctx, x, proto, [HN])
    assert_matches_oracle(res, ref, len(x), "%s split %s fail %s" % (proto, split, fail))
    assert int(ref["out_count"].sum()) > 0 and int(ref["event_count"].sum()) > 0


@pytest.mark.parametrize("split", SPLITS)
def test_hand_over_ragged_rows(ctx, handover, monkeypatch, split):
    """One ragged push of up to 70 000 samples: rows that bring nothing, a few samples, less than the first part (split_n0 = 35 000 /
    49 000), exactly it, one more, and rows that end inside the last part; then every channel's rest."""
    x, ref = handover["dmr"]
    B, n = x.shape
    _split_env(monkeypatch, split, False)
    n0 = HN * int(split.split(",")[0]) // 100
    first = np.array([HN, 0, 3, 20000, n0 - 1, n0, n0 + 1, HN - 1, HN * 92 // 100 - 1, HN * 92 // 100, HN * 92 // 100 + 1, 1407, 1409, n0 - 1408, HN, HN], np.int64)
    eng = api.Engine(B, HN, proto="dmr", ctx=ctx)
    acc = [[[] for _ in range(B)] for _ in range(3)]
    pos = np.zeros(B, np.int64)
    _push_counts(eng, HN, x, pos, first, acc)
    while (pos < n).any():
        _push_counts(eng, HN, x, pos, np.minimum(HN, n - pos), acc)
    eng.close()
    _assert_acc(acc, ref, B, "ragged, split %s" % split)


def test_timing_step_across_the_part_boundary(emu_ctx, oracle, monkeypatch):
    """Two channels whose symbol clock drifts by a sample per variance block, one each way: every block ends with a step of +1 / -1 that
    is applied behind the first symbol of the next one.  A first push of 2 b samples with DH_TAIL_SPLIT=50 puts the part boundary at
    sample b; b = 1 500, 1 507, ... walks it through more than a block at every position modulo the symbol period, so it falls between
    the decision and the step, on the step and behind it.  (Emulation only: the device does not split a launch this small.)"""
    n = 4200
    chans = []
    for seed, r in ((91, 1e-3), (92, -1e-3)):
        s = synth.shape(synth.dmr_stream(seed, 4))
        t = np.arange(int(len(s) / (1.0 + r)) - 2) * (1.0 + r)
        chans.append(synth.impair(np.interp(t, np.arange(len(s)), s).astype(np.float32), seed, snr_db=30, delay=3 * seed % 10)[:n])
    x = np.stack(chans)
    assert x.shape == (2, n)
    ref = oracle.chain(x, proto=1)
    assert int(ref["steps_up"].sum()) >= 2 and int(ref["steps_down"].sum()) >= 2, (ref["steps_up"], ref["steps_down"])
    monkeypatch.setenv("DH_TAIL_SPLIT", "50")
    monkeypatch.delenv("DH_TAIL_SPLIT_FORCE_FAIL", raising=False)
    for b in range(1500, 2520, 7):
        res = run_engine(emu_ctx, x, "dmr", [2 * b, n])
        assert_matches_oracle(res, ref, len(x), "part boundary at %d" % b)


@pytest.mark.gpu
@pytest.mark.parametrize("proto", ["dmr", "ysf"])
def test_hand_over_on_a_launch_that_splits(gpu_ctx, handover, monkeypatch, proto):
    """The cases of test_hand_over 8 208 channels wide (16 signals, repeated): the launches split, and with DH_TAIL_SPLIT_FORCE_FAIL=3
    the fix-up launch finishes every third row (debug word 202 counts the hand-overs that did not come)."""
    import torch
    x16, ref = handover[proto]
    U, B = 16, 8192 + 16
    x = torch.from_numpy(x16).to(gpu_ctx.mem.device).repeat(B // U, 1).contiguous()
    for split in SPLITS:
        for fail in (False, True):
            _split_env(monkeypatch, split, fail)
            eng = api.Engine(B, HN, proto=proto, ctx=gpu_ctx)
            acc = [[[] for _ in range(B)] for _ in range(3)]
            for k in range(2):
                eng.push(x[:, k * HN:(k + 1) * HN].contiguous())
                for j, (rows, counts) in enumerate((eng.symbols(), eng.frames(), eng.events())):
                    for b in range(B):
                        acc[j][b].append(rows[b, :counts[b]].copy())
            gave_up = int(eng.debug_header(202)[0])
            eng.close()
            assert (gave_up > 0) == fail, (split, fail, gave_up)
            cat = [[np.concatenate(acc[j][b]) for b in range(B)] for j in range(3)]
            _assert_acc([[[cat[j][b]] for b in range(U)] for j in range(3)], ref, U, "%s split %s fail %s" % (proto, split, fail))
            for j in range(3):
                want = [hashlib.sha256(cat[j][b].tobytes()).hexdigest() for b in range(U)]
                assert all(hashlib.sha256(cat[j][b].tobytes()).hexdigest() == want[b % U] for b in range(U, B)), (split, fail, j)
