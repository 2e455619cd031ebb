"""Randomised parity soak: many small cases with drawn impairments and push patterns through the chain kernels, compared
bit for bit with the oracle (dibits, frame bytes, events).  Aimed at the error-bounded FIR (dsp_core.hpp): amplitudes from
1e-6 to 1e4 (the error radius scales with max |x|), DC offsets larger than the signal, signal-to-noise ratios from -3 dB
up, fades to silence and back, pushes from one sample to the whole stream -- a wrong bound or a lost history sample would
show up as a flipped dibit somewhere in here.  The case list is fixed by the seeds below (failures are reproducible)."""
import numpy as np
import pytest

from common import assert_matches_oracle, rel_err, rel_err_per_channel, run_engine
from digiham_amd import _taps, synth


def _case(rng, proto, big_dc=False):
    seed = int(rng.integers(1, 10 ** 6))
    kw, okw, sps, taps = {}, {}, 10, None
    if proto == "dmr":
        s = synth.dmr_stream(seed, int(rng.integers(6, 14)), two_slots=bool(rng.integers(0, 2)))
        okw = dict(proto=1)
    elif proto == "ysf":
        s = synth.ysf_stream(seed, int(rng.integers(3, 6)), mode=["vd2", "vd1", "fr", "datafr"][int(rng.integers(0, 4))])
        okw = dict(proto=2)
    elif proto == "nxdn":
        s = synth.nxdn_stream(seed, int(rng.integers(6, 12)))
        kw, okw, sps, taps = dict(rrc="narrow", sps=20), dict(rrc=2, sps=20, proto=3), 20, _taps.narrow()
    elif proto == "dstar":                                   # 2-level FSK at sps 10, no filter
        bits, _ = synth.dstar_stream(seed, 1, ber=float(rng.choice([0.0, 0.002])))
        kw, okw, sps = dict(rrc="none", demod="fsk", sps=10), dict(rrc=0, levels=2, sps=10, proto=5), 10
        s = None
        x = synth.fsk_shape(bits[:int(rng.integers(12000, 30000)) // 10], sps=10)
    else:                                                    # POCSAG: inverted 2-level FSK at sps 40
        bits, _ = synth.pocsag_stream(seed, 1)
        kw, okw, sps = dict(rrc="none", demod="fsk", sps=40, invert=True), dict(rrc=0, levels=2, sps=40, invert=True, proto=4), 40
        s = None
        x = synth.fsk_shape(bits[:int(rng.integers(400, 1200))], sps=40, invert=True)
    if s is not None:
        x = synth.shape(s, sps=sps, taps=taps) if taps is not None else synth.shape(s)
    gain = float(10.0 ** rng.uniform(-6, 4)) if rng.random() < 0.5 else float(rng.uniform(0.2, 3.0))
    snr = None if rng.random() < 0.2 else float(rng.uniform(-3, 40))
    dc = float(rng.uniform(-2, 2)) * (1.0 if rng.random() < 0.3 else 0.05)
    if big_dc:                                               # mean^2 / V from 1e2 to about 1e6: the estimate's cancellation
        dc = float(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(1, 3) * np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    x = synth.impair(x, seed, snr_db=snr, dc=dc, gain=1.0, delay=int(rng.integers(0, 40)))
    if rng.random() < 0.3:                                   # a fade to (near) silence and back
        a, b = sorted(rng.integers(0, len(x), 2))
        x[a:b] *= np.float32(rng.choice([0.0, 1e-4, 0.02]))
    x = (x * np.float32(gain)).astype(np.float32)
    n = len(x)
    kind = int(rng.integers(0, 4))
    chunks = ([n], [int(rng.integers(1, 50)), int(rng.integers(2000, 9000)), int(rng.integers(1, 400))],
              [int(rng.integers(900, 1100))], [int(rng.integers(100, 30000)) for _ in range(6)])[kind]
    return x, kw, okw, chunks, dict(seed=seed, gain=gain, snr=snr, chunks=chunks[:3])


@pytest.mark.parametrize("proto,batch", [("dmr", 0), ("dmr", 1), ("ysf", 0), ("ysf", 1), ("nxdn", 0)])
def test_randomised_cases_match_the_oracle(ctx, oracle, proto, batch):
    rng = np.random.default_rng(20260929 + 17 * batch + {"dmr": 0, "ysf": 1000, "nxdn": 2000}[proto])
    flips = 0
    for c in range(5 if proto != "nxdn" else 3):
        x, kw, okw, chunks, what = _case(rng, proto)
        ref = oracle.chain(x[None, :], **okw)
        res = run_engine(ctx, x[None, :], proto, chunks, **kw)
        assert_matches_oracle(res, ref, 1, "%s case %d %r" % (proto, c, what))
        flips += int(ref["sym_count"][0])
    assert flips > 0


# routes and draws the cases above do not reach: (proto, engine flags, DC up to 1e3 x the signal's rms, seed offset)
MORE = [("dstar", {}, False, 0), ("dstar", {}, True, 1), ("pocsag", {}, False, 0), ("pocsag", {}, True, 1),
        ("dmr", dict(one_launch=True, keep_filtered=True), False, 0), ("dmr", dict(one_launch=True, fast_fir=True, keep_filtered=True), False, 0),
        ("dmr", dict(one_launch=True, fast_fir=True, keep_filtered=True), True, 1),
        ("dmr", dict(split_stages=True), False, 0), ("dmr", dict(exact_symbols=True), False, 0),
        ("dmr", {}, True, 2), ("ysf", {}, True, 2), ("nxdn", {}, True, 2)]


@pytest.mark.parametrize("proto,flags,big_dc,batch", MORE, ids=["%s-%s%s-%d" % (p, "+".join(sorted(f)) or "default", "-dc" if d else "", b)
                                                                for p, f, d, b in MORE])
def test_randomised_cases_on_more_routes(ctx, oracle, proto, flags, big_dc, batch):
    """The soak on D-Star and POCSAG, on DH_FLAG_ONE_LAUNCH (with and without FAST_FIR; floats within 2.5e-6 / 1e-6 against
    every channel's own level as well as the batch's), SPLIT_STAGES and EXACT_SYMBOLS, and with DC offsets up to a thousand
    times the signal (mean^2 / V to about 1e6)."""
    rng = np.random.default_rng(20261016 + 101 * batch + {"dmr": 0, "ysf": 1000, "nxdn": 2000, "dstar": 3000, "pocsag": 4000}[proto])
    keep = bool(flags.get("keep_filtered"))
    tol = 1e-6 if flags.get("fast_fir") else 2.5e-6
    flips = 0
    for c in range(4 if proto not in ("nxdn", "pocsag") else 3):
        x, kw, okw, chunks, what = _case(rng, proto, big_dc=big_dc)
        ref = oracle.chain(x[None, :], keep_filtered=keep, **okw)
        res = run_engine(ctx, x[None, :], proto, chunks, **kw, **flags)
        what = "%s %s case %d %r" % (proto, sorted(flags), c, what)
        assert_matches_oracle(res, ref, 1, what)
        if keep:
            assert res["filtered"].shape == ref["filtered"].shape, what
            assert rel_err(res["filtered"], ref["filtered"]).max() <= tol, what
            assert rel_err_per_channel(res["filtered"], ref["filtered"]).max() <= tol, what
        flips += int(ref["sym_count"][0])
    assert flips > 0
