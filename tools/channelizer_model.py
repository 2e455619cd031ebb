#!/usr/bin/env python3
"""tools/channelizer_model.py [--interpolation L] [--decimation M] [--rows R] [--seconds S] [--seed N] [--device cuda|cpu]
[--raster HZ]:
a float64 model of the rational-rate channelizer on the end-to-end fixture of tests/test_channelizer_rational.py
(tests/cz_harness.py builds it), next to the library.

The model, per channel: mix the composite down by the channel's offset, convolve with each of the L phases
h_p[k] = h[r_p + k L] of the prototype (FFT, complex128), take z[j] = (h_p * x)[n_j] with p = j mod L (DESIGN.md section
4.6), then arg(z[j] conj z[j-1]) / pi and the DC blocker y = (x - x[-1]) + 0.995 y[-1], all in double.  Its rows and, with
--device cuda, the library's go through the CPU oracle's DMR chain.  Printed per row: level, generated superframes, and
(syncs, LCs, LCs with wrong ids) of the model and of the library, with the largest difference of the two FM rows after the
first 512 outputs.  The last line says whether the model decodes every row as test_end_to_end_wideband_gpu asks (ids in
every non-empty DMR row's LCs, at least as many syncs as superframes, no syncs in the empty rows); the exit status is 1 if
it does not.  A fixture for that test has to be one this model passes; --seed 8 is the test's.  --seed 7 on the device
gives row 10 a sixth LC with wrong ids in the model and in the library alike.

--raster HZ (with --decimation D; no interpolation): the fixture of tests/test_channelizer_raster.py instead -- 48 kS/s * D,
channels on multiples of HZ, Channelizer(raster_hz=HZ) -- and the model is the raster mode's own formula in double: the
polyphase fold v[r] = sum_p h[r + p K] x[n_j - r - p K], the K-point DFT over r and the rotation e^(-2 pi i c n_j / K), then
the discriminator and the DC blocker as above.  That fixture's noise comes from the CPU generator whatever --device is, so
a seed checked here with --device cpu names the noise test_end_to_end_raster_gpu gets."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def model_rows(x, rate, raster, h, L, M):
    """float64 FM + DC rows [len(raster)][L n // M] of the int16 composite x [n][2]."""
    from scipy.signal import lfilter
    n = len(x)
    xs = (x[:, 0].astype(np.float64) + 1j * x[:, 1]) / 32768.0
    n_out = L * n // M
    nj = (np.arange(n_out) * M + M - 1) // L
    h64 = h.astype(np.float64)
    size = 1 << int(np.ceil(np.log2(n + len(h) // L + 2)))
    Hp = [np.fft.fft(h64[(p * M + M - 1) % L::L], size) for p in range(L)]
    nn = np.arange(n)
    out = np.zeros((len(raster), n_out), np.float64)
    for r, f in enumerate(raster):
        X = np.fft.fft(xs * np.exp(-2j * np.pi * ((f / rate * nn) % 1.0)), size)
        z = np.zeros(n_out, complex)
        for p in range(L):
            z[p::L] = np.fft.ifft(X * Hp[p])[nj[p::L]]
        w = z * np.conj(np.concatenate([[0], z[:-1]]))
        out[r] = lfilter([1.0, -1.0], [1.0, -0.995], np.angle(w) / np.pi)
    return out


def model_rows_raster(x, rate, raster_hz, raster, h, D, block=8192):
    """float64 FM + DC rows [len(raster)][n // D] of the int16 composite x [n][2]: fold + DFT + rotation."""
    from scipy.signal import lfilter
    K = int(round(rate / raster_hz))
    P = -(-len(h) // K)
    hp = np.zeros(P * K)
    hp[:len(h)] = h
    hp = hp.reshape(P, K)
    n = len(x)
    n_out = n // D
    H = P * K
    xs = np.concatenate([np.zeros(H, complex), (x[:, 0].astype(np.float64) + 1j * x[:, 1]) / 32768.0])
    c = np.mod(np.round(np.array(raster) / raster_hz).astype(np.int64), K)
    r = np.arange(K)
    E = np.exp(2j * np.pi * np.outer(r, c) / K)                 # [K][rows]
    z = np.zeros((len(raster), n_out), complex)
    for j0 in range(0, n_out, block):
        j1 = min(n_out, j0 + block)
        nj = np.arange(j0, j1) * D + D - 1
        v = np.zeros((j1 - j0, K), complex)
        for p in range(P):                                      # x[n_j - r - p K]: rows D apart, r descending
            first = xs[H + nj[0] - p * K:]
            a = np.lib.stride_tricks.as_strided(first, shape=(j1 - j0, K), strides=(D * xs.itemsize, -xs.itemsize), writeable=False)
            v += hp[p][None, :] * a
        z[:, j0:j1] = (v @ E).T * np.exp(-2j * np.pi * np.outer(c, nj % K) / K)
    out = np.zeros((len(raster), n_out), np.float64)
    for i in range(len(raster)):
        w = z[i] * np.conj(np.concatenate([[0], z[i, :-1]]))
        out[i] = lfilter([1.0, -1.0], [1.0, -0.995], np.angle(w) / np.pi)
    return out


def decode(audio, meta, O, api):
    """per row: (syncs, LCs, LCs with wrong ids) of the oracle's DMR chain."""
    ref = O.chain(np.ascontiguousarray(audio, np.float32), proto=1)
    res = []
    for r in range(len(audio)):
        e = ref["events"][r, :ref["event_count"][r]]
        lcs = [api.parse_lc(p) for p in e[e["type"] == 4]["payload"]]
        bad = [l for l in lcs if r in meta and not (l["source"] == meta[r]["src"] and l["target"] == meta[r]["dst"])]
        res.append((int((e["type"] == 1).sum()), len(lcs), len(bad)))
    return res


def passes(res, f):
    for r, (syncs, lcs, bad) in enumerate(res):
        if r in f["meta"]:
            if bad or not lcs or syncs < f["meta"][r]["superframes"]:
                return False
        elif r in f["empty"] and syncs:
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--interpolation", type=int, default=3)
    ap.add_argument("--decimation", type=int, default=128)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--raster", type=float, default=0.0)
    a = ap.parse_args()
    from digiham_amd import api
    from oracle import oracle as O
    from cz_harness import end_to_end_fixture
    O.build()
    L, M = a.interpolation, a.decimation
    if a.raster:
        L = 1
        f = end_to_end_fixture(1, M, a.rows, a.seconds, a.device, a.seed, raster_hz=a.raster, noise_device="cpu")
    else:
        f = end_to_end_fixture(L, M, a.rows, a.seconds, a.device, a.seed)
    on_device = a.device != "cpu"
    x = f["x"].cpu().numpy() if on_device else f["x"]
    lib = None
    if on_device:
        cz = api.Channelizer(f["rate"], M, f["raster"], f["h"], input="cs16", output="fm", dcblock=True, max_input=f["n"],
                             **(dict(raster_hz=a.raster) if a.raster else dict(interpolation=L)))
        rows, k = cz.push(f["x"])
        lib = rows[:, :k].cpu().numpy().astype(np.float64)
        cz.close()
    model = model_rows_raster(x, f["rate"], a.raster, f["raster"], f["h"], M) if a.raster else model_rows(x, f["rate"], f["raster"], f["h"], L, M)
    rm = decode(model, f["meta"], O, api)
    rl = decode(lib, f["meta"], O, api) if lib is not None else None
    start = 512                                                 # outputs skipped: the filter's and the DC blocker's start-up
    for r in range(a.rows):
        kind = "ysf" if r == f["ysf_row"] else "empty" if r in f["empty"] else "dmr %6.1f dB, %d superframes" % (f["meta"][r]["level_db"], f["meta"][r]["superframes"])
        line = "row %2d  %-30s model (syncs, LCs, wrong) %s" % (r, kind, rm[r])
        if lib is not None:
            line += "  library %s  max |FM difference| %.3g" % (rl[r], float(np.abs(lib[r] - model[r])[start:].max()))
        print(line, flush=True)
    ok = passes(rm, f)
    print("%sseed %d, %s noise: the model %s every row%s" % ("raster %g Hz, D %d, %d rows, %g s: " % (a.raster, M, a.rows, a.seconds) if a.raster else "", a.seed,
             "cpu" if a.raster else a.device, "decodes" if ok else "does NOT decode",
          "" if rl is None else "; the library %s; counts %s" % ("does too" if passes(rl, f) else "does NOT", "agree" if rl == rm else "differ")))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
