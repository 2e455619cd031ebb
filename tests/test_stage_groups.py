"""The edges of window staging in the chain kernels (dsp_core.hpp: DhWindowGroups, dh_stage_f16): a window of 1 024 + NZ samples is fetched as
four full 16-byte groups per lane and a partial last group behind their 1 024 samples (20 lanes of it for the wide filter, NZ = 80; 40 for
the narrow one, NZ = 160), zeroed beyond the input.  Full chains against the oracle at the smallest shapes where that group can go wrong:
pushes whose last window ends inside, at and just behind it (the zeros-beyond path with 1 024 < have < 1 024 + NZ), ragged pushes, an
all-zero channel (max |x| = 0) and non-finite samples inside the last 96 samples of a window (the reference-order FIR takes the run over
from the staged halves).  Dibits, decoder bytes, events and counts bit for bit; the one-launch mode's floats within its 2.5e-6.
"""
import numpy as np
import pytest

from common import assert_matches_oracle, make_channels, rel_err, rel_err_per_channel, run_engine
from digiham_amd import _taps, synth

LENGTHS = [1103, 1104, 1105, 1184, 2127, 2208]
N = 5002                                            # samples per channel: 2 000 + 1 + 3 001, five windows of the wide filter


def _special(x):
    """Rows 5..7: all zeros; a NaN and an infinity inside the last 96 samples of a window (windows start every 1 000 samples, give or take
    the timing steps: [1 008, 1 104) of the first, [2 008, 2 104) of the second ...)."""
    x = x.copy()
    x[5, :] = 0.0
    x[6, 1050] = np.nan
    x[6, 4060] = np.nan
    x[7, 2055] = np.inf
    x[7, 3090] = -np.inf
    return x


@pytest.fixture(scope="module")
def dmr_case(oracle):
    x = _special(make_channels("dmr", [1, 2, 3, 4, 5, 6, 7, 8], 5)[:, :N])
    assert x.shape == (8, N)
    return x, oracle.chain(x, proto=1), oracle.chain(x, proto=0, keep_filtered=True)


@pytest.fixture(scope="module")
def nxdn_case(oracle):
    chans = []
    for i, seed in enumerate(range(11, 19)):
        x = synth.shape(synth.nxdn_stream(seed, 3), sps=20, taps=_taps.narrow())
        chans.append(synth.impair(x, seed, snr_db=[None, 22, 16, 30][i % 4], dc=[0, 0.1, -0.2, 0.05][i % 4], delay=7 * i, gain=[1, 0.5, 1.7, 1][i % 4]))
    n = min(min(len(c) for c in chans), 2 * N)
    x = _special(np.stack([c[:n] for c in chans]))
    return x, oracle.chain(x, rrc=2, sps=20, proto=3)


@pytest.mark.parametrize("chunks", [[c] for c in LENGTHS] + [[2000, 1, 3001]], ids=lambda c: "x".join(map(str, c)))
def test_dmr_chain_bit_exact_around_the_last_group(ctx, dmr_case, chunks):
    x, ref, _ = dmr_case
    res = run_engine(ctx, x, "dmr", chunks)
    assert_matches_oracle(res, ref, len(x), "dmr %s" % chunks)
    assert int(ref["sym_count"][0]) > 400 and int(ref["sym_count"][5]) > 400          # (the all-zero channel slices too)


@pytest.mark.parametrize("length", LENGTHS)
def test_dmr_single_push_of_each_length(ctx, oracle, dmr_case, length):
    """One push of `length` samples into a fresh engine: its only windows are the first of a stream and the one that ends with the input."""
    x = np.ascontiguousarray(dmr_case[0][:, :length])
    ref = oracle.chain(x, proto=1)
    res = run_engine(ctx, x, "dmr", [length])
    assert_matches_oracle(res, ref, len(x), "dmr one push of %d" % length)


def test_nxdn_chain_bit_exact_at_the_same_lengths(ctx, nxdn_case):
    x, ref = nxdn_case
    for chunks in [[c] for c in LENGTHS] + [[2000, 1, 3001]]:
        res = run_engine(ctx, x, "nxdn", chunks, rrc="narrow", sps=20)
        assert_matches_oracle(res, ref, len(x), "nxdn %s" % chunks)


def test_one_launch_floats_at_the_same_lengths(ctx, dmr_case):
    """DH_FLAG_KEEP_FILTERED | DH_FLAG_ONE_LAUNCH: the split-f16 FIR's floats leave too -- within 2.5e-6 of the reference's relative to
    max(|ref|, rms), per batch and per channel (tests/test_chain.py).  The channels with a NaN or an infinity (rows 6, 7) are held to the
    same bound wherever the reference's output is finite (rms over those samples), and are non-finite exactly where the reference's is;
    the dibits of all channels bit for bit."""
    x, _, ref = dmr_case
    want = ref["filtered"]
    for chunks in [[c] for c in LENGTHS] + [[2000, 1, 3001]]:
        res = run_engine(ctx, x, "none", chunks, keep_filtered=True, one_launch=True)
        assert res["filtered"].shape == want.shape
        assert rel_err(res["filtered"][:5], want[:5]).max() <= 2.5e-6, chunks
        assert rel_err_per_channel(res["filtered"][:5], want[:5]).max() <= 2.5e-6, chunks
        assert (res["filtered"][5] == 0.0).all(), chunks
        for b in (6, 7):
            ok = np.isfinite(want[b])
            assert 0 < (~ok).sum() < 400 and (np.isfinite(res["filtered"][b]) == ok).all(), (chunks, b)
            assert rel_err(res["filtered"][b][ok], want[b][ok]).max() <= 2.5e-6, (chunks, b)
        assert_matches_oracle(res, {"syms": ref["syms"], "sym_count": ref["sym_count"]}, len(x), "one launch %s" % chunks)
