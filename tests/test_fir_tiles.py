"""The matrix-core FIRs' result tiles (dsp_core.hpp: dh_fir_f16, dh_fir_mfma, DH_F16_OUT, DH_MF_OUT): a run's 1 024 results come out of the
MFMAs in a tile layout and go back to the window block through DH_F16_OUT / DH_MF_OUT.  A sample that lands in the wrong word of that block
is a wrong dibit or a wrong float, so the layout is checked end to end against the oracle at the smallest shape that has every kind of
window: 2 600 samples are the first window of a stream, two whole runs and the window that ends with the input; pushes cut after 1, 9 and
1 003 samples move the run grid against the tiles; a NaN and a sample of 1e20 send their runs through the reference-order FIR from the same
staged block.  Dibits, frame bytes and events bit for bit; the floats of the one-launch modes within the bounds bench.py holds them to
(2.5e-6 split-f16, 1e-6 f32 FMA chain, of max(|ref|, rms))."""
import numpy as np
import pytest

from common import assert_matches_oracle, make_channels, rel_err, rel_err_per_channel, run_engine
from digiham_amd import _taps, synth

N = 2600
CUTS = [[N], [1, N - 1], [9, N - 9], [1003, N - 1003]]
IDS = ["whole", "cut1", "cut9", "cut1003"]
NAN_AT, HUGE_AT = 1337, 2011                        # channel 1 / channel 2: inside the second whole run / inside the last window


@pytest.fixture(scope="module")
def case(oracle):
    x = make_channels("dmr", [31, 32, 33], 2)[:, :N].copy()
    assert x.shape == (3, N)
    x[1, NAN_AT] = np.nan
    x[2, HUGE_AT] = 1e20
    return x, oracle.chain(x, proto=1), oracle.chain(x, proto=0, keep_filtered=True)


@pytest.mark.parametrize("chunks", CUTS, ids=IDS)
def test_dmr_chain_bit_exact(ctx, case, chunks):
    x, ref, _ = case
    res = run_engine(ctx, x, "dmr", chunks)
    assert_matches_oracle(res, ref, len(x), "dmr %s" % chunks)
    assert all(int(c) >= 200 for c in ref["sym_count"])             # (every channel slices all of its runs, the ones with a NaN or 1e20 too)


@pytest.mark.parametrize("fast,tol", [(False, 2.5e-6), (True, 1e-6)], ids=["f16", "fma"])
@pytest.mark.parametrize("chunks", CUTS, ids=IDS)
def test_one_launch_floats(ctx, case, chunks, fast, tol):
    """DH_FLAG_KEEP_FILTERED | DH_FLAG_ONE_LAUNCH, without and with DH_FLAG_FAST_FIR: what the tiles hold leaves as floats.  The clean
    channel per batch and per channel; the channels with a NaN or 1e20 are non-finite exactly where the reference's output is and held to
    the same bound elsewhere (rms over those samples)."""
    x, _, ref = case
    want = ref["filtered"]
    res = run_engine(ctx, x, "none", chunks, keep_filtered=True, one_launch=True, fast_fir=fast)
    got = res["filtered"]
    assert got.shape == want.shape
    assert rel_err(got[:1], want[:1]).max() <= tol
    assert rel_err_per_channel(got[:1], want[:1]).max() <= tol
    for b in (1, 2):
        ok = np.isfinite(want[b])
        assert (np.isfinite(got[b]) == ok).all(), b
        assert rel_err(got[b][ok], want[b][ok]).max() <= tol, b
    assert 0 < (~np.isfinite(want[1])).sum() <= 81 and np.isfinite(want[2]).all()
    # samples the NaN / the 1e20 never reaches are held against the channel's own level there (with the spike in it the rms is 1e18)
    for b, at in ((1, NAN_AT), (2, HUGE_AT)):
        far = np.ones(N, bool)
        far[max(0, at - 200):at + 200] = False
        assert rel_err(got[b][far], want[b][far]).max() <= tol, b
    assert_matches_oracle(res, {"syms": ref["syms"], "sym_count": ref["sym_count"]}, len(x), "one launch %s" % chunks)


def test_nxdn_narrow_filter_chain(ctx, oracle):
    """The 161-tap split-f16 FIR (six K steps per tile) on the NXDN chain: 2 channels x 2 100 samples, whole and cut at 1 003."""
    n = 2100
    chans = []
    for i, seed in enumerate((41, 42)):
        s = synth.shape(synth.nxdn_stream(seed, 3), sps=20, taps=_taps.narrow())
        chans.append(synth.impair(s, seed, snr_db=[None, 22][i], dc=[0, 0.1][i], delay=7 * i, gain=[1, 0.5][i])[:n])
    x = np.stack(chans)
    assert x.shape == (2, n)
    ref = oracle.chain(x, rrc=2, sps=20, proto=3)
    for chunks in ([n], [1003, n - 1003]):
        res = run_engine(ctx, x, "nxdn", chunks, rrc="narrow", sps=20)
        assert_matches_oracle(res, ref, len(x), "nxdn %s" % chunks)
    assert int(ref["sym_count"].min()) >= 80
