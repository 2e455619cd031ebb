"""The one-chain form of the split-f16 FIR (dsp_core.hpp: dh_f16_one_chain, dh_fir_f16, dh_stage_f16) and the NaN-propagating
max |x| of staging (wave_ops.hpp: dh_max_abs_groups, DH_WAVE_MAX_NAN).

The wide filter's kernels that do not hand out their floats add all nine MFMAs of a tile into ONE accumulator on a common 2^11
scale -- taps g1' = 2^11 g1, second halves h2' = f16(x_s - h1) -- and multiply once.  What that changes is the error radius
(six MFMAs at the main sum's magnitude instead of three), never an output: undecided comparisons take the reference's arithmetic.

* the radius, restated here, against a brute-force comparison through the matrix cores;
* what the host hands the kernels: g1' exact and finite, the other engines' fragments and coefficients as they were;
* DMR and YSF chains against the oracle over amplitudes, a spike among quiet samples and a large DC, in one push and in ragged
  ones -- with no run through the reference-order FIR, so the matrix-core path is what ran;
* NaN and infinity: caught where max |x| is taken, the clean channel beside them untouched.
"""
import os
import subprocess

import numpy as np
import pytest

from common import make_channels, assert_matches_oracle
from digiham_amd import api, _taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _split_taps(taps):
    g1 = taps.astype(np.float16)
    g2 = ((taps.astype(np.float64) - g1.astype(np.float64)) * 2048).astype(np.float32).astype(np.float16)
    delta = taps.astype(np.float64) - g1.astype(np.float64) - g2.astype(np.float64) / 2048
    return g1, g2, delta


def _kl1(taps, one_chain):
    """dh_f16_error_coefficient without its 1.44 (the slicer's head room) and without u / gain, restated"""
    g1, g2, delta = _split_taps(taps)
    l1, l1g1, l1g2 = (np.abs(v.astype(np.float64)).sum() for v in (taps, g1, g2))
    ks = (len(taps) + 15 + 31) // 32
    if one_chain:          # 2 KS MFMAs at the main sum's magnitude; L1(g2) inside all 3 KS; the g1' h2' sum inside the last KS; one rounding of the combine
        mfma = 82.0 * ks * l1g1 * (1 + 2.0 ** -11) + 41.0 * ks / 2048 * (3 * l1g2 * (1 + 2.0 ** -11) + l1g1)
        combine = 2.1 * l1
    else:
        mfma = 41.0 * ks * l1g1 * (1 + 2.0 ** -11) + 82.0 * ks / 2048 * (l1g2 + 0.5 * l1g1)
        combine = 3.1 * l1
    return ((len(taps) + 1 + 0.01) * l1 + 1.0001 * l1 + mfma
            + 2.0 * (0.5 * l1g2 / 2 ** 22 + np.abs(delta).sum() * (1 + 2.0 ** -12) + U * l1) / U + combine)


def test_one_chain_radius_covers_a_brute_force_comparison(ctx):
    """The method of test_numerics.test_f16_fir_error_radius_covers_a_brute_force_comparison with the one-chain operands (g1', g2, h1,
    h2'), the nine MFMAs in the kernel's order in one accumulator, and y = A kc -- against the reference's rounded-product chain.
    The distance stays inside the radius (the fraction observed is printed: DESIGN.md section 3 quotes it)."""
    rng = np.random.default_rng(3)
    taps = _taps.wide().astype(np.float32); gain = _taps.WIDE_GAIN
    g1, g2, _ = _split_taps(taps)
    g1s = (g1.astype(np.float32) * np.float32(2048)).astype(np.float16)
    assert np.isfinite(g1s).all() and np.array_equal(g1s.astype(np.float64), g1.astype(np.float64) * 2048)
    radius_per_xmax = _kl1(taps, True) * U / gain
    T = 96

    def toeplitz(g):                       # B[p][n] = g[p - n]
        B = np.zeros((96, 16), np.float16)
        for n in range(16):
            B[n:n + 81, n] = g
        return B
    B1s, B2 = toeplitz(g1s), toeplitz(g2)
    worst = {}
    for name in ("1", "3e-4", "700", "spike"):
        if name == "spike":                # one sample at 1.0 among samples around 1e-4: nearly every h2' is subnormal or zero
            x = (rng.normal(0, 1e-4, (T, 16, 16 + 95))).astype(np.float32)
            x[np.arange(T), rng.integers(0, 16, T), rng.integers(0, 111, T)] = 1.0
        else:
            x = (rng.normal(0, 0.4, (T, 16, 16 + 95)) * float(name)).astype(np.float32)
        xmax = np.abs(x).max(axis=(1, 2), keepdims=True)
        ex = np.floor(np.log2(xmax)).astype(np.int64)
        scale = (2.0 ** (-1 - ex)).astype(np.float32)                                # max |x s| in [0.5, 1)
        xs = x * scale
        h1 = xs.astype(np.float16); h2 = (xs - h1.astype(np.float32)).astype(np.float16)
        if name == "spike":
            tiny = np.abs(h2.astype(np.float64)) < 2.0 ** -14
            assert tiny.mean() > 0.99 and (h2 != 0).any()
        acc = np.zeros((T, 16, 16), np.float32)
        for h, B in ((h1, B2), (h1, B1s), (h2, B1s)):
            for s in range(3):
                acc = ctx.debug_mfma_f16(h[:, :, 32 * s:32 * s + 32], np.broadcast_to(B[32 * s:32 * s + 32], (T, 32, 16)), acc)
        kc = (np.float32(1.0 / gain) / scale * np.float32(2.0 ** -11)).astype(np.float32)      # powers of two: exact
        y = (acc.astype(np.float32) * kc).astype(np.float32)
        ref = np.zeros((T, 16, 16), np.float32)                                      # rounded products, rounded sums in tap order, double division
        for k in range(81):
            win = np.stack([x[:, :, n + k] for n in range(16)], axis=2)
            ref = (ref + (np.float32(taps[k]) * win).astype(np.float32)).astype(np.float32)
        ref = (ref.astype(np.float64) / gain).astype(np.float32)
        worst[name] = float((np.abs(y.astype(np.float64) - ref.astype(np.float64)) / (radius_per_xmax * xmax)).max())
    print("one-chain radius, worst distance as a fraction of it:", worst)
    assert max(worst.values()) <= 1.0, worst


def _fragments(g_main, g_second, nz, ks):
    """DhF16Taps::frag as dh_f16_tap_fragments lays it out: frag[f][lane][d] = halves 32 s + 8 q + 2 d + (0, 1) - n of slice s = f % KS"""
    out = np.zeros((2 * ks, 64, 4), np.uint32)
    for f in range(2 * ks):
        g = (g_main if f < ks else g_second).view(np.uint16)
        for lane in range(64):
            n, q = lane & 15, lane >> 4
            for d in range(4):
                w = 0
                for hh in range(2):
                    t = 32 * (f % ks) + 8 * q + 2 * d + hh - n
                    w |= (int(g[t]) if 0 <= t <= nz else 0) << (16 * hh)
                out[f, lane, d] = w
    return out.ravel()


def test_fragments_and_coefficients_per_engine_kind(tmp_path):
    """tests/host_cpp/f16_fragments.cpp prints what an engine builds.  One chain (wide filter, floats not kept): the main-sum fragments
    hold 2^11 g1 -- exact, finite -- and the coefficient is the restated one.  An engine that keeps its filtered samples and the narrow
    filter: fragments from g1 itself and the coefficients these engines had before the one-chain form existed (their float bits)."""
    exe = str(tmp_path / "f16_fragments")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-Wno-unknown-pragmas", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "host_cpp", "f16_fragments.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        p = line.split()
        rows[p[0]] = (int(p[1]), int(p[2]), np.array([int(p[3], 16)], np.uint32).view(np.float32)[0], np.array([int(v, 16) for v in p[5:]], np.uint32))
        assert len(p) == 5 + int(p[4])
    wide, narrow = _taps.wide().astype(np.float32), _taps.narrow().astype(np.float32)
    w1, w2, _ = _split_taps(wide)
    n1, n2, _ = _split_taps(narrow)
    w1s = (w1.astype(np.float32) * np.float32(2048)).astype(np.float16)
    assert np.isfinite(w1s).all() and np.array_equal(w1s.astype(np.float64), 2048 * w1.astype(np.float64)) and np.abs(w1s.astype(np.float64)).max() == 2160
    one, ok, coef, words = rows["wide"]
    assert one == 1 and ok == 1 and np.array_equal(words, _fragments(w1s, w2, 80, 3))
    want = 1.44 * _kl1(wide, True) * U / _taps.WIDE_GAIN * 1.0001
    assert want <= coef <= want * (1 + 1e-6)
    for name in ("wide_keep", "wide_keep_fast"):
        one, ok, coef, words = rows[name]
        assert one == 0 and ok == 1 and np.array_equal(words, _fragments(w1, w2, 80, 3))
        assert np.float32(coef).view(np.uint32) == 0x37E07058
    one, ok, coef, words = rows["narrow"]
    assert one == 0 and ok == 1 and np.array_equal(words, _fragments(n1, n2, 160, 6))
    assert np.float32(coef).view(np.uint32) == 0x385A187E
    assert abs(rows["wide"][2] / rows["wide_keep"][2] - 1.57) < 0.01          # what the one accumulator costs the radius


# ---------------------------------------------------------------------------------------------- chains against the oracle
N = 4000                 # four variance blocks of 1 000 samples
_cache = {}


def _inputs(proto):
    """five channels of N samples: the signal as it is, at 1e-20 and at 1e12, a spike among quiet samples, a DC far above the deviation"""
    base = make_channels(proto, [61, 62, 63, 64, 65], 3 if proto == "dmr" else 1)[:, :N].copy()
    x = base.copy()
    x[1] *= np.float32(1e-20)
    x[2] *= np.float32(1e12)
    x[3] *= np.float32(1e-4); x[3, 350::700] = 1.0
    x[4] = x[4] * np.float32(0.01) + np.float32(5.0)
    return x


def _oracle(oracle, proto, key, x):
    if (proto, key) not in _cache:
        with np.errstate(all="ignore"):
            _cache[(proto, key)] = oracle.chain(x, proto=1 if proto == "dmr" else 2)
    return _cache[(proto, key)]


def _run(ctx, x, proto, chunks):
    """the pushes of common.run_engine, plus DH_ST_EXACT_RUNS per channel"""
    B, n = x.shape
    eng = api.Engine(B, max(chunks), proto=proto, ctx=ctx)
    syms, frames, evs = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    pos = i = 0
    while pos < n:
        c = min(chunks[i % len(chunks)], n - pos); i += 1
        eng.push(np.ascontiguousarray(x[:, pos:pos + c])); pos += c
        s, sc = eng.symbols(); f, fc = eng.frames(); e, ec = eng.events()
        for b in range(B):
            syms[b].append(s[b, :sc[b]].copy()); frames[b].append(f[b, :fc[b]].copy()); evs[b].append(e[b, :ec[b]].copy())
    exact_runs = eng.debug_header(17).astype(np.int64)
    eng.close()
    cat = lambda parts, dt: [np.concatenate(p) if p else np.zeros(0, dt) for p in parts]
    return {"syms": cat(syms, np.uint8), "frames": cat(frames, np.uint8), "events": cat(evs, api.EVENT_DTYPE), "filtered": None}, exact_runs


@pytest.mark.parametrize("chunks", [[N], [1500, 1, 777, 1203, 519]], ids=["one_push", "ragged"])
@pytest.mark.parametrize("proto", ["dmr", "ysf"])
def test_chain_is_the_oracles_and_runs_on_the_matrix_cores(ctx, oracle, proto, chunks):
    """(the ragged pushes: a one-sample push, and pushes that end inside a run)"""
    x = _inputs(proto)
    ref = _oracle(oracle, proto, "finite", x)
    assert int(ref["sym_count"].min()) > 300
    res, exact_runs = _run(ctx, x, proto, chunks)
    assert_matches_oracle(res, ref, x.shape[0], "%s %s" % (proto, chunks[:2]))
    assert (exact_runs == 0).all(), exact_runs


@pytest.mark.parametrize("proto", ["dmr", "ysf"])
def test_nan_and_infinity_are_caught_at_staging(ctx, oracle, proto):
    """A NaN as the first sample the first run's window takes from the input (channel 0: the 80 before it are the filter's zero
    history), a NaN inside the last, partial 16-byte load group of a window that is loaded in groups (channel 1: the second run's
    window starts within a few samples of input sample 920, so sample 2 000 sits at its offset 1 024 .. 1 103 -- and at offset 80 or
    so of the third: two runs), an infinity (channel 2), and a clean channel beside them."""
    x = make_channels(proto, [71, 72, 73, 74], 3 if proto == "dmr" else 1)[:, :N].copy()
    # Run k = 1, 2, .. of a stream takes a timing block (100 symbols of 10 samples) and starts k - 1 blocks in, moved by the timing
    # recovery by at most one sample per block; the stream begins with the filter's 80 zeros, so the window of run k begins at input
    # sample 1000 (k - 1) - 80 + d, |d| <= k - 1, and is fetched as 16-byte groups of 256 samples, the last one at offsets 1024 .. 1103.
    block, history, last_group, window = 100 * 10, 80, 1024, 1024 + 80
    pos = 2000
    for d in (-1, 0, 1):                       # run 2: inside the last, partial group
        assert last_group <= pos - (block - history + d) < window
    for d in (-2, -1, 0, 1, 2):                # run 3: inside its window too (first group)
        assert 0 <= pos - (2 * block - history + d) < 256
    x[0, 0] = np.nan
    x[1, pos] = np.nan
    x[2, 2500] = np.inf
    ref = _oracle(oracle, proto, "poisoned", x)
    res, exact_runs = _run(ctx, x, proto, [N])
    assert_matches_oracle(res, ref, x.shape[0], proto)
    assert exact_runs[0] >= 1 and exact_runs[1] >= 2 and exact_runs[2] >= 1 and exact_runs[3] == 0, exact_runs
