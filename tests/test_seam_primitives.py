"""Every primitive of the device / CPU seam (dh_portable.hpp, wave_ops.hpp) and the AGC scan pair, each run ALONE through the
probe kernel (dh_debug_seam_probe, seam_probe_core.hpp): once on the CPU restatement (the emulation) and once, with -m gpu, on
the gfx950 form -- inline assembly the compiler does not check.  Both are held to the primitive's written statement, computed
here in numpy (float32 operations; float64 or exact arithmetic where a fused form needs it), never to each other.

Comparison: bit patterns are equal; where the reference is NaN the result is a NaN (payload free); where a minimum or maximum
ties between +0 and -0 either zero passes.  Signalling NaNs bind the primitives that take raw samples (dh_max3_abs,
dh_max_abs_groups, DH_WAVE_MAX_NAN, dh_f16_split4_plain); for the NaN-skipping minima and maxima, whose operands are arithmetic
results and so quiet, rows with a signalling NaN are reported (run with -s) and do not fail.  One launch per op."""
import os
import re

import numpy as np
import pytest

from digiham_amd import _capi, api

OP = _capi.PROBE_OPS
HDR, WAVE = 4, 64
LDS_WORDS, BASE_MAX, RAMP, MARK = 5632, 1720, 0x3F000000, 0x4B000000
FLT_MAX, FLT_MIN = np.float32(3.402823466e+38), np.float32(1.175494351e-38)
u32, f32, f64 = np.uint32, np.float32, np.float64


def bits(x):
    return np.ascontiguousarray(x, f32).view(u32)


def flt(b):
    return np.ascontiguousarray(b, u32).view(f32)


def word(x):
    """the bit pattern of one float"""
    return int(np.float32(x).view(np.uint32))


QNAN, SNAN = [0x7FC00000, 0xFFC00001], [0x7F800001, 0xFFA00000]
_POS = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000] + [word(f32(1.5) * f32(2.0) ** k) for k in (-60, -1, 30, 90)] + [0x7F7FFFFF, 0x7F800000]
E = np.array(_POS + [p | 0x80000000 for p in _POS] + QNAN + SNAN, u32)      # the operand table: 26 values


def is_nan(b):
    b = np.asarray(b, u32)
    return (b & 0x7FFFFFFF) > 0x7F800000


def is_snan(b):
    b = np.asarray(b, u32)
    return is_nan(b) & ((b & 0x00400000) == 0)


def quieted(b):
    b = np.asarray(b, u32).copy()
    b[is_snan(b)] |= 0x00400000
    return b


def rand_bits(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(u32)


def product(*tables):
    g = np.meshgrid(*tables, indexing="ij")
    return [x.ravel() for x in g]


def operands(k, seed, table=E, n_random=4096):
    """table^k followed by n_random random bit patterns per operand"""
    rng = np.random.default_rng(seed)
    return [np.concatenate([t, rand_bits(rng, n_random)]) for t in product(*([table] * k))]


# ------------------------------------------------------------------------------------------------------------------ running
def run_lanes(ctx, op, args, hdr=None):
    """args: per-operand uint32 arrays of one length n (item j is lane j % 64 of case j // 64); hdr: [cases][<= 4] header words.
    Returns the per-result arrays of length n."""
    n = len(args[0]) if args else WAVE * len(hdr)
    cases = -(-n // WAVE)
    w = np.zeros((cases, HDR + WAVE * len(args)), u32)
    if hdr is not None:
        h = np.asarray(hdr, u32).reshape(cases, -1)
        w[:, :h.shape[1]] = h
    for i, a in enumerate(args):
        buf = np.full(cases * WAVE, 0x3F800000, u32)
        buf[:n] = a
        w[:, HDR + WAVE * i:HDR + WAVE * (i + 1)] = buf.reshape(cases, WAVE)
    out = ctx.debug_seam_probe(OP[op], w)
    assert out.shape[1] % WAVE == 0
    return [out[:, WAVE * i:WAVE * (i + 1)].reshape(-1)[:n] for i in range(out.shape[1] // WAVE)]


def hold(what, got, ref, args=(), tie=None, free=None):
    """got (uint32 bits) against ref (float32, or uint32 bits): equal bits, or both NaN, or (tie) any zero; `free` rows are reported only"""
    got = np.asarray(got, u32)
    refb = ref if np.asarray(ref).dtype == u32 else bits(ref)
    ok = got == refb
    ok |= is_nan(refb) & is_nan(got)
    if tie is not None:
        ok |= tie & ((got & 0x7FFFFFFF) == 0)
    if free is not None and free.any():
        g = got[free]
        print("%s: %d rows with a signalling NaN operand (not binding): %d gave a NaN, %d the statement's value, %d something else"
              % (what, int(free.sum()), int(is_nan(g).sum()), int(ok[free].sum()), int((~ok[free] & ~is_nan(g)).sum())))
        ok |= free
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d differ; first at %d: got %#010x, statement %#010x, operands %s" % (
        what, bad.size, got.size, bad[0], got[bad[0]], refb[bad[0]], ["%#010x" % a[bad[0]] for a in args])


def zero_tie(*ops):
    """rows where the operands hold both a +0 and a -0 (a minimum / maximum of 0 may be either)"""
    pz = np.zeros(ops[0].shape, bool); nz = pz.copy()
    for o in ops:
        pz |= o == 0; nz |= o == 0x80000000
    return pz & nz


def any_snan(*ops):
    m = np.zeros(ops[0].shape, bool)
    for o in ops:
        m |= is_snan(o)
    return m


def skip_nan_reduce(fn, *xs):
    """min / max that skip a NaN operand: NaN only when every operand is NaN"""
    out = xs[0].copy()
    for x in xs[1:]:
        with np.errstate(invalid="ignore"):
            out = np.where(np.isnan(out), x, np.where(np.isnan(x), out, fn(out, x)))
    return out


def fma_exact(a, b, c):
    """RN32(a b + c) with ONE rounding: the product is exact in float64 (48 bits), the sum is rounded to odd in float64 (two-sum
    gives its error exactly), and 53 - 24 >= 2 spare bits make the final rounding to float32 the correct one -- subnormal results
    included.  Non-finite operands go through the same float64 operations, which have float32's rules for them."""
    with np.errstate(all="ignore"):
        p = flt(a).astype(f64) * flt(b).astype(f64)
        c64 = flt(c).astype(f64)
        s = p + c64
        t = s - p
        err = (p - (s - t)) + (c64 - t)
        inexact = np.isfinite(s) & (err != 0) & np.isfinite(err)
        even = (s.view(np.uint64) & np.uint64(1)) == 0
        toward = np.where((err > 0), np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)
        return s.astype(f32)


# ------------------------------------------------------------------------------------------------------------------ the entry
def test_probe_entry_checks_its_arguments(ctx):
    with pytest.raises(api.DhError) as e:
        ctx.seam_probe_words(len(OP))
    assert e.value.code == -1
    with pytest.raises(api.DhError):
        ctx.seam_probe_words(-1)
    rc = ctx.lib.dh_debug_seam_probe(len(OP), None, None, 0, ctx.mem.stream())
    assert rc == -1
    for name, op in OP.items():
        nin, nout = ctx.seam_probe_words(op)
        assert nin >= HDR and nout >= 1, name
        assert ctx.debug_seam_probe(op, np.zeros((0, nin), u32)).shape == (0, nout)      # no cases: DH_OK, nothing launched


def test_op_table_is_the_headers_enum():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "digiham_amd.h")).read()
    body = re.search(r"enum dh_probe_op \{(.*?)\}", text, re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.replace("\n", " ").split(",") if n.strip()]
    assert names == ["DH_PROBE_" + n for n in OP] + ["DH_PROBE_OP_COUNT"]
    assert list(OP.values()) == list(range(len(OP)))


# ---------------------------------------------------------------------------------------------------------- lane-wise floats
@pytest.mark.parametrize("op", ["VMIN", "VMAX"])
def test_min_max_skip_a_nan_operand(ctx, op):
    a, b = operands(2, 1)
    got, = run_lanes(ctx, op, [a, b])
    ref = skip_nan_reduce(np.minimum if op == "VMIN" else np.maximum, flt(a), flt(b))
    hold("dh_" + op.lower(), got, ref, (a, b), tie=zero_tie(a, b), free=any_snan(a, b))


def test_min3_abs_skips_nan_operands(ctx):
    a, b, c = operands(3, 2)
    got, = run_lanes(ctx, "MIN3_ABS", [a, b, c])
    ref = skip_nan_reduce(np.minimum, np.abs(flt(a)), np.abs(flt(b)), np.abs(flt(c)))
    hold("dh_min3_abs", got, ref, (a, b, c), free=any_snan(a, b, c))


def test_max3_abs_hands_on_any_nan(ctx):
    """max(|a|, |b|, c), c >= 0 or NaN; NaN when ANY operand is NaN, a signalling one included"""
    c_table = E[((E & 0x80000000) == 0) | is_nan(E) | (E == 0x80000000)]
    rng = np.random.default_rng(3)
    a, b, c = product(E, E, c_table)
    rc = rand_bits(rng, 4096); rc = np.where(is_nan(rc), rc, rc & 0x7FFFFFFF).astype(u32)
    a, b, c = np.concatenate([a, rand_bits(rng, 4096)]), np.concatenate([b, rand_bits(rng, 4096)]), np.concatenate([c, rc])
    got, = run_lanes(ctx, "MAX3_ABS", [a, b, c])
    with np.errstate(invalid="ignore"):
        ref = np.maximum(np.maximum(np.abs(flt(a)), np.abs(flt(b))), flt(c))
    ref = np.where(is_nan(a) | is_nan(b) | is_nan(c), f32(np.nan), ref)
    hold("dh_max3_abs", got, ref, (a, b, c), tie=zero_tie(a & 0x7FFFFFFF, b & 0x7FFFFFFF, c))


def test_max_abs_groups_sees_every_position(ctx):
    """the distinguished value -- the largest magnitude of either sign, an infinity, a quiet or a signalling NaN -- at each of the
    20 positions; none (all zero); random groups"""
    rng = np.random.default_rng(4)
    rows = []
    for pos in range(20):
        for special in (0x7F000000, 0xFF000000, 0x7F800000, 0xFF800000) + tuple(QNAN) + tuple(SNAN):
            r = bits(rng.uniform(-2, 2, 20).astype(f32)).copy()
            r[pos] = special
            rows.append(r)
    rows.append(np.zeros(20, u32)); rows.append(np.full(20, 0x80000000, u32))
    rows += list(rand_bits(rng, 20 * 1024).reshape(1024, 20))
    rows = np.array(rows, u32)
    got, = run_lanes(ctx, "MAX_ABS_GROUPS5", [rows[:, i] for i in range(20)])
    ref = np.where(is_nan(rows).any(axis=1), f32(np.nan), np.abs(flt(rows)).max(axis=1, initial=0.0)).astype(f32)
    hold("dh_max_abs_groups<5>", got, ref, [rows[:, i] for i in range(20)])


def _uniform_cases(seed, n_uniform):
    """64 cases of 64 lanes: the wave-uniform operand(s) of case i from E and random patterns, the lanes' operands likewise"""
    rng = np.random.default_rng(seed)
    uni = [np.concatenate([E, rand_bits(rng, WAVE - E.size)])[rng.permutation(WAVE)] for _ in range(n_uniform)]
    return rng, uni


def test_mul_uniform_is_one_rounded_product(ctx):
    rng, (s,) = _uniform_cases(5, 1)
    v = np.concatenate([np.concatenate([E, rand_bits(rng, WAVE - E.size)]) for _ in range(WAVE)])
    got, = run_lanes(ctx, "MUL_UNIFORM", [v], hdr=s[:, None])
    with np.errstate(all="ignore"):
        ref = flt(v) * np.repeat(flt(s), WAVE)
    hold("dh_mul_uniform", got, ref, (np.repeat(s, WAVE), v))


@pytest.mark.parametrize("d", [5, 6, 10, 20, 40])
def test_div_const2_is_div_const_of_each_half(ctx, d):
    """each half the IEEE quotient x / d, bit for bit -- also for a pair with one half inside and one outside [2^-100, 2^100], in
    both positions (the device tests the larger word once and takes the real division for both)"""
    rng = np.random.default_rng(60 + d)
    edge = np.concatenate([np.arange(b - 16, b + 16, dtype=u32) for b in (0x0D800000, 0x71800000, 0x00800000, 0x7F800000)] + [np.arange(0, 16, dtype=u32)])
    edge = np.concatenate([edge, edge | u32(0x80000000)])
    inside = bits((rng.normal(0, 1, edge.size) * 10.0 ** rng.uniform(-6, 3, edge.size)).astype(f32))
    ex, ey = product(E, E)
    x = np.concatenate([ex, edge, inside, rand_bits(rng, 4096), bits(rng.normal(0, 3, 4096).astype(f32))])
    y = np.concatenate([ey, inside, edge, rand_bits(rng, 4096), bits(rng.normal(0, 3, 4096).astype(f32))])
    cases = -(-x.size // WAVE)
    hdr = np.tile(np.array([word(f32(d)), word(f32(1) / f32(d))], u32), (cases, 1))
    gx, gy = run_lanes(ctx, "DIV_CONST2", [x, y], hdr=hdr)
    with np.errstate(all="ignore"):
        hold("dh_div_const2 / %d, first half" % d, gx, flt(x) / f32(d), (x, y))
        hold("dh_div_const2 / %d, second half" % d, gy, flt(y) / f32(d), (x, y))


def _mac_operands(seed):
    """(c, w, acc) triples: E^3, random patterns, signal-sized values, products that cancel against the addend (acc = -RN(c w): the
    fused form leaves the product's rounding error, the rounded one 0) and results in the subnormal range"""
    rng = np.random.default_rng(seed)
    c, w, a = product(E, E, E)
    n = 2048
    sc, sw = rng.normal(0, 1, n).astype(f32), rng.normal(0, 1, n).astype(f32)
    tiny_c, tiny_w = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-80, -60, n)).astype(f32), (rng.uniform(-2, 2, n) * 2.0 ** rng.integers(-75, -60, n)).astype(f32)
    with np.errstate(all="ignore"):
        cancel = -(sc * sw)
    c = np.concatenate([c, rand_bits(rng, n), bits(sc), bits(sc), bits(tiny_c), bits(tiny_c)])
    w = np.concatenate([w, rand_bits(rng, n), bits(sw), bits(sw), bits(tiny_w), bits(tiny_w)])
    a = np.concatenate([a, rand_bits(rng, n), bits(rng.normal(0, 1, n).astype(f32)), bits(cancel), np.zeros(n, u32), rng.integers(0, 1 << 23, n).astype(u32)])
    return c, w, a


def _mac_ref(fast, c, w, a):
    if fast:
        return fma_exact(c, w, a)
    with np.errstate(all="ignore"):
        return flt(a) + (flt(c) * flt(w)).astype(f32)


@pytest.mark.parametrize("fast", [False, True])
def test_f2_mac_rounds_as_stated(ctx, fast):
    """a + c w per half: product and sum rounded separately; FAST: one fused rounding (exact reference)"""
    c, wx, ax = _mac_operands(7)
    wy, ay = np.roll(wx, 1), np.roll(ax, 3)
    gx, gy = run_lanes(ctx, "F2_MAC_FAST" if fast else "F2_MAC", [c, wx, wy, ax, ay])
    hold("dh_f2_mac<%d>.x" % fast, gx, _mac_ref(fast, c, wx, ax), (c, wx, ax))
    hold("dh_f2_mac<%d>.y" % fast, gy, _mac_ref(fast, c, wy, ay), (c, wy, ay))


@pytest.mark.parametrize("fast,half", [(False, 0), (False, 1), (True, 0), (True, 1)])
def test_f2_mac_pair_takes_the_named_half_of_the_tap_pair(ctx, fast, half):
    """the tap is ONE half of a scalar pair (op_sel): the other half -- always a different value here -- must not take part"""
    c, wx, ax = _mac_operands(8)
    n = c.size - c.size % WAVE
    c, wx, ax = c[:n], wx[:n], ax[:n]
    wy, ay = np.roll(wx, 1), np.roll(ax, 3)
    tap = c.reshape(-1, WAVE)[:, 0]                                    # one tap per case
    other = np.roll(tap, 1) ^ u32(0x00010000)
    assert (other != tap).all()
    hdr = np.stack([other, tap] if half else [tap, other], axis=1)
    cc = np.repeat(tap, WAVE)
    gx, gy = run_lanes(ctx, "F2_MAC_PAIR_%s%s" % ("FAST_" if fast else "", "HI" if half else "LO"), [wx, wy, ax, ay], hdr=hdr)
    hold("dh_f2_mac_pair<%d, %d>.x" % (fast, half), gx, _mac_ref(fast, cc, wx, ax), (cc, wx, ax))
    hold("dh_f2_mac_pair<%d, %d>.y" % (fast, half), gy, _mac_ref(fast, cc, wy, ay), (cc, wy, ay))


def test_f2_fma_is_one_rounding_per_half(ctx):
    a, b, c = _mac_operands(9)
    a2, b2, c2 = np.roll(a, 5), np.roll(b, 7), np.roll(c, 11)
    gx, gy = run_lanes(ctx, "F2_FMA", [a, a2, b, b2, c, c2])
    hold("dh_f2_fma.x", gx, fma_exact(a, b, c), (a, b, c))
    hold("dh_f2_fma.y", gy, fma_exact(a2, b2, c2), (a2, b2, c2))


def test_f2_scale_is_one_rounded_product_per_half(ctx):
    x, y, s = operands(3, 10)
    gx, gy = run_lanes(ctx, "F2_SCALE", [x, y, s])
    with np.errstate(all="ignore"):
        hold("dh_f2_scale.x", gx, flt(x) * flt(s), (x, s))
        hold("dh_f2_scale.y", gy, flt(y) * flt(s), (y, s))


def test_sqrt_upper_is_an_upper_bound_within_two_to_the_minus_19(ctx):
    """s = sqrt(max(x, 1e-30)) in float64: s <= r <= s (1 + 2^-19) -- 1 ulp of v_sqrt_f32, the factor 1 + 2^-20 and one rounding.
    The two builds may differ in the last bit; both are bounds."""
    rng = np.random.default_rng(12)
    e_pos = E[((E & 0x80000000) == 0) & ~is_nan(E)]
    x = np.concatenate([e_pos, bits((rng.uniform(1, 2, 100_000) * 2.0 ** rng.integers(-126, 127, 100_000)).astype(f32)), rng.integers(1, 1 << 23, 1000).astype(u32)])
    got, = run_lanes(ctx, "SQRT_UPPER", [x])
    r = flt(got).astype(f64)
    s = np.sqrt(np.maximum(flt(x).astype(f64), 1e-30))
    print("dh_sqrt_upper: r / s in [1 + %.3g, 1 + %.3g]" % ((r[np.isfinite(s)] / s[np.isfinite(s)]).min() - 1, (r[np.isfinite(s)] / s[np.isfinite(s)]).max() - 1))
    bad = np.flatnonzero(~((s <= r) & (r <= s * (1 + 2.0 ** -19))))
    assert bad.size == 0, "x = %r: r = %r, s = %r" % (flt(x)[bad[0]], r[bad[0]], s[bad[0]])


def test_f16_split_plain_is_round_to_nearest_with_subnormals(ctx):
    """h1 = f16(x s), h2 = f16(x s - h1): numpy's IEEE conversions (round to nearest even, subnormal halves kept), the difference
    exact in float32; x s = h1 + h2 to within 2^-24 for |x s| <= 1.  Infinite samples give an infinite h1 (and a NaN h2:
    inf - inf), NaN samples -- quiet or signalling -- NaN halves."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-1, 1, 20_000), rng.uniform(-1, 1, 10_000) * 10.0 ** rng.uniform(-9, 0, 10_000),
                        [0.0, -0.0, 1.0, -1.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 0.99999994, 6.1e-5, 5.96e-8]]).astype(f32)
    special = np.array([0x7F800000, 0xFF800000] + QNAN + SNAN, u32)
    xin, scales = [], []
    for scale in (1.0, 0.5, 2.0 ** -7, 2.0 ** 20):
        v = np.concatenate([bits((x / f32(scale)).astype(f32)), special])             # so that x s covers [-1, 1] again
        v = np.concatenate([v, np.zeros(-v.size % (4 * WAVE), u32)])
        xin.append(v); scales += [scale] * (v.size // (4 * WAVE))
    xin = np.concatenate(xin)
    hdr = bits(np.array(scales, f32))[:, None]
    quads = xin.reshape(-1, WAVE, 4)                                                     # a lane's four samples
    out = run_lanes(ctx, "F16_SPLIT4_PLAIN", [quads[:, :, i].reshape(-1) for i in range(4)], hdr=hdr)
    halves = np.stack(out, axis=1).reshape(-1, 4).copy().view(np.uint16).reshape(-1, 2, 4)   # [lane][h1 | h2][4]
    h1, h2 = halves[:, 0, :].reshape(-1), halves[:, 1, :].reshape(-1)
    with np.errstate(all="ignore"):
        xs = flt(xin) * np.repeat(flt(hdr[:, 0]), 4 * WAVE)
        r1 = xs.astype(np.float16)
        r2 = (xs - r1.astype(f32)).astype(np.float16)
    for name, g, r in (("h1", h1, r1), ("h2", h2, r2)):
        rb = r.view(np.uint16)
        nan = np.isnan(r)
        assert (np.isnan(g.view(np.float16)) == nan).all(), name
        bad = np.flatnonzero((g != rb) & ~nan)
        assert bad.size == 0, "%s: x s = %r: got %#06x, want %#06x" % (name, xs[bad[0]], g[bad[0]], rb[bad[0]])
    fin = np.isfinite(xs) & (np.abs(xs) <= 1)
    rec = h1.view(np.float16).astype(f64) + h2.view(np.float16).astype(f64)
    assert np.abs(rec - xs.astype(f64))[fin].max() <= 2.0 ** -24
    assert fin.sum() > 100_000


# ------------------------------------------------------------------------------------------------------- reductions and sums
def run_reduce(ctx, op, rows):
    rows = np.asarray(rows, u32)
    w = np.zeros((rows.shape[0], HDR + WAVE), u32)
    w[:, HDR:] = rows
    return ctx.debug_seam_probe(OP[op], w)[:, 0]


def _reduce_rows(rng, lanes, lo_is_special, domain):
    """the cases of a reduction over `lanes` lanes: the distinguished lane at every position, among ordinary values and as the only
    lane that is not NaN; all equal; 256 random vectors (quiet NaNs among them).  Every lane NaN: test_reductions_of_all_nan_lanes."""
    rows = []
    for pos in range(lanes):
        r = rng.uniform(1, 2, lanes).astype(f32)
        r[pos] = -1000.0 if lo_is_special else 1000.0
        rows.append(bits(domain(r)))
        r = np.full(lanes, QNAN[pos & 1], u32); r[pos] = word(1.5 + pos)
        rows.append(r)
    rows.append(np.full(lanes, word(f32(3.25)), u32))
    rows.append(np.zeros(lanes, u32))
    rows += list(quieted(bits(domain(flt(rand_bits(rng, 256 * lanes))))).reshape(256, lanes))
    return np.array(rows, u32)


def _nan_skipping(fn, rows):
    f = flt(rows)
    with np.errstate(all="ignore"):
        return fn(f, axis=1).astype(f32)


def _report_snan_rows(ctx, op, rng, make):
    rows = []
    for pos in (0, 15, 16, 37, 63):
        for s in SNAN:
            r = make(); r[pos % r.size] = s
            rows.append(r)
    full = np.array([_pad_row0(r) for r in rows], u32)
    got = run_reduce(ctx, op, full)
    print("%s with one signalling NaN lane (not binding): %s" % (op, ", ".join("%#010x" % g for g in got)))


def _pad_row0(r):
    """a DH_ROW0_MIN vector from its ten values: lanes 10 .. 15 hold FLT_MAX, as the caller leaves them, lanes 16 .. 63 values BELOW
    the row's minimum, which must not be looked at"""
    if r.size == WAVE:
        return r
    out = np.full(WAVE, word(f32(-3e38)), u32)
    out[:r.size] = r
    out[r.size:16] = word(FLT_MAX)
    return out


def test_wave_max_skips_nan_lanes(ctx):
    """DH_WAVE_MAX: values >= 0"""
    rng = np.random.default_rng(20)
    rows = _reduce_rows(rng, WAVE, False, np.abs)
    hold("DH_WAVE_MAX", run_reduce(ctx, "WAVE_MAX", rows), _nan_skipping(np.nanmax, rows), tie=None)
    _report_snan_rows(ctx, "WAVE_MAX", rng, lambda: bits(rng.uniform(1, 2, WAVE).astype(f32)))


def test_wave_max_nan_hands_on_any_nan(ctx):
    """DH_WAVE_MAX_NAN: magnitudes (sign bit clear); NaN when ANY lane is NaN -- quiet or signalling, at every position, alone
    among numbers and everywhere"""
    rng = np.random.default_rng(21)
    rows = list(_reduce_rows(rng, WAVE, False, np.abs) & u32(0x7FFFFFFF))
    for pos in range(WAVE):
        for nan in (QNAN[0], SNAN[0], 0x7FFFFFFF):
            r = bits(rng.uniform(0, 2, WAVE).astype(f32)).copy(); r[pos] = nan
            rows.append(r)
    rows.append(np.full(WAVE, QNAN[0], u32)); rows.append(np.full(WAVE, SNAN[0], u32))
    r = bits(rng.uniform(0, 2, WAVE).astype(f32)).copy(); r[7] = 0x7F800000; rows.append(r)           # an infinity is a number
    rows = np.array(rows, u32)
    ref = np.where(is_nan(rows).any(axis=1), f32(np.nan), flt(rows).max(axis=1, initial=0.0)).astype(f32)
    hold("DH_WAVE_MAX_NAN", run_reduce(ctx, "WAVE_MAX_NAN", rows), ref)


def _min_domain(r):
    return np.where(r > FLT_MAX, FLT_MAX, r).astype(f32)            # values <= FLT_MAX (-inf is one); NaN stays


def test_wave_min_skips_nan_lanes(ctx):
    """DH_WAVE_MIN: values <= FLT_MAX (-inf is one)"""
    rng = np.random.default_rng(22)
    rows = _reduce_rows(rng, WAVE, True, _min_domain)
    ref = _nan_skipping(np.nanmin, rows)
    hold("DH_WAVE_MIN", run_reduce(ctx, "WAVE_MIN", rows), ref, tie=(flt(rows) == 0).any(axis=1) & (ref == 0))
    _report_snan_rows(ctx, "WAVE_MIN", rng, lambda: bits(rng.uniform(1, 2, WAVE).astype(f32)))


def test_row0_min_looks_at_lanes_0_to_15_only(ctx):
    rng = np.random.default_rng(23)
    rows = np.array([_pad_row0(r) for r in _reduce_rows(rng, 10, True, _min_domain)], u32)
    # (the row's minimum must stay above what lanes 16 .. 63 hold)
    rows[:, :10] = np.where(flt(rows[:, :10]) < -2e38, word(-2e38), rows[:, :10])
    ref = _nan_skipping(np.nanmin, rows[:, :16])
    hold("DH_ROW0_MIN", run_reduce(ctx, "ROW0_MIN", rows), ref, tie=(flt(rows[:, :16]) == 0).any(axis=1) & (ref == 0))
    _report_snan_rows(ctx, "ROW0_MIN", rng, lambda: bits(rng.uniform(1, 2, 10).astype(f32)))


def test_reductions_of_all_nan_lanes(ctx):
    """Every lane NaN: nothing to skip to, the result is NaN (DH_WAVE_MAX_NAN: above).  The callers never depend on it: they keep
    the lanes that hold no phase at FLT_MAX, which is what ROW0_MIN's second vector here does -- ten NaN phases, the result FLT_MAX."""
    for op in ("WAVE_MAX", "WAVE_MIN", "ROW0_MIN"):
        rows = np.array([np.full(WAVE, QNAN[0], u32), np.full(WAVE, QNAN[1], u32), np.where(np.arange(WAVE) & 1, QNAN[0], QNAN[1])], u32)
        if op == "ROW0_MIN":
            rows[:, 16:] = word(-1.0)
        hold("DH_%s, every lane NaN" % op, run_reduce(ctx, op, rows), np.full(3, np.nan, f32))
    row = _pad_row0(np.full(10, QNAN[0], u32))
    hold("DH_ROW0_MIN, ten NaN phases", run_reduce(ctx, "ROW0_MIN", row[None, :]), np.array([FLT_MAX], f32))
    row = np.full(WAVE, QNAN[1], u32); row[40] = word(FLT_MAX)
    hold("DH_WAVE_MIN, NaN but one FLT_MAX", run_reduce(ctx, "WAVE_MIN", row[None, :]), np.array([FLT_MAX], f32))


def test_row_sum5_pair_order_and_row_ends(ctx):
    """((x[l] + x[l-1]) + (x[l-2] + x[l-3])) + x[l-4] inside each row of sixteen, a missing neighbour 0: magnitudes spread over
    2^+-20 so that another order changes the float result; a large value in lanes 15, 31 and 47 must not leak into the next row"""
    rng = np.random.default_rng(24)
    def spread(n):
        return (rng.choice([-1.0, 1.0], (n, WAVE)) * rng.uniform(1, 2, (n, WAVE)) * 2.0 ** rng.integers(-20, 21, (n, WAVE))).astype(f32)
    s, q = spread(256), spread(256)
    for k, lane in enumerate((15, 31, 47)):
        s[k] = rng.uniform(-1, 1, WAVE); s[k, lane] = 1e30
        q[k] = rng.uniform(-1, 1, WAVE); q[k, lane] = -1e30
    s[3, ::7] = 0.0; q[3, ::5] = -0.0
    gs, gq = run_lanes(ctx, "ROW_SUM5_PAIR", [bits(s).reshape(-1), bits(q).reshape(-1)])
    def at(x, d):
        y = np.zeros_like(x)
        y[:, d:] = x[:, :WAVE - d]
        y[:, (np.arange(WAVE) & 15) < d] = 0.0
        return y
    def ref(x):
        return (((at(x, 0) + at(x, 1)).astype(f32) + (at(x, 2) + at(x, 3)).astype(f32)).astype(f32) + at(x, 4)).astype(f32)
    hold("dh_row_sum5_pair, s", gs, ref(s).reshape(-1), (bits(s).reshape(-1),))
    hold("dh_row_sum5_pair, q", gq, ref(q).reshape(-1), (bits(q).reshape(-1),))
    # (the operands tell the stated order from a left-to-right chain: the check would not see another order otherwise)
    chain = ((((at(s, 0) + at(s, 1)).astype(f32) + at(s, 2)).astype(f32) + at(s, 3)).astype(f32) + at(s, 4)).astype(f32)
    assert (bits(chain) != bits(ref(s))).mean() > 0.05


# ------------------------------------------------------------------------------------------------------------ the AGC scan
def _agc_tables(old, new):
    """mn[k0][k], mx[k0][k]: the extremes over the ring as it stands after slot k was written, slots k0 .. k new, the others old,
    100 slots; seeds FLT_MAX and FLT_MIN (gfsk_demodulator.cpp:109-116); a NaN entry is skipped"""
    mn = np.zeros((100, 100), f32); mx = np.zeros((100, 100), f32)
    for k0 in range(100):
        ring = old[:100].copy()
        for k in range(k0, 100):
            ring[k] = new[k]
            mn[k0, k] = np.fmin.reduce(ring, initial=FLT_MAX)
            mx[k0, k] = np.fmax.reduce(ring, initial=FLT_MIN)
    return mn, mx


def _agc_run(ctx, pairs, rings, spans, from_win):
    """rings: list of (old[128], new[128]) float32; spans: per case (ring index, k0, k1); from_win per case.  The source the case does not
    use (the LDS rings or the DhWinPair values) and the ring slots from 100 on hold junk."""
    rng = np.random.default_rng(31)
    n = len(spans)
    w = np.zeros((n, HDR + WAVE * 10), u32)
    lane = np.arange(WAVE)
    for c, ((ri, k0, k1), fw) in enumerate(zip(spans, from_win)):
        old, new = rings[ri]
        junk = bits(rng.uniform(-5e4, 5e4, 6 * WAVE + 256).astype(f32))
        w[c, :3] = (k0, k1, int(fw))
        lds_old, lds_new = (junk[:128], junk[128:256]) if fw else (bits(old), bits(new))
        words = [lds_old[:64], lds_old[64:], lds_new[:64], lds_new[64:]]
        if fw:
            words += [bits(new[2 * lane]), bits(new[2 * lane + 1]), junk[256:320], junk[320:384], bits(old[126 - 2 * lane]), bits(old[127 - 2 * lane])]
        else:
            words += list(junk[256:].reshape(6, WAVE))
        w[c, HDR:] = np.concatenate(words)
    out = ctx.debug_seam_probe(OP["AGC_SCAN_PAIRS" if pairs else "AGC_SCAN"], w)
    mn = out[:, :128]; mx = out[:, 128:256]
    agc = out[:, 256:].reshape(n, 4, WAVE)                             # mn0, mx0, mn1, mx1 per lane
    return mn, mx, agc


def _agc_check(what, rings, tables, spans, mn, mx, agc):
    bad = []
    for c, (ri, k0, k1) in enumerate(spans):
        rmn, rmx = tables[ri][0][k0, k0:k1], tables[ri][1][k0, k0:k1]
        k = np.arange(k0, k1)
        slot_mn = np.where(k & 1, agc[c, 2, k >> 1], agc[c, 0, k >> 1])
        slot_mx = np.where(k & 1, agc[c, 3, k >> 1], agc[c, 1, k >> 1])
        for name, g, r in (("S.mn", mn[c, k0:k1], rmn), ("S.mx", mx[c, k0:k1], rmx), ("agc.mn", slot_mn, rmn), ("agc.mx", slot_mx, rmx)):
            ok = (g == bits(r)) | ((r == 0) & ((g & 0x7FFFFFFF) == 0))
            if not ok.all():
                j = int(np.flatnonzero(~ok)[0])
                bad.append("%s ring %d k0 %d k1 %d: %s[%d] = %#010x, statement %#010x" % (what, ri, k0, k1, name, k0 + j, g[j], bits(r)[j]))
    assert not bad, "%d differ; first: %s" % (len(bad), bad[0])


def _agc_rings():
    rng = np.random.default_rng(30)
    def ring(fn):
        return fn(128).astype(f32), fn(128).astype(f32)
    positive = ring(lambda n: rng.uniform(0.01, 3, n) * 10.0 ** rng.uniform(-3, 3, n))
    mixed = ring(lambda n: rng.normal(0, 1, n))
    negative = ring(lambda n: -rng.uniform(0.01, 3, n))
    constant = (np.full(128, 0.75, f32), np.full(128, 0.75, f32))
    def with_nans(n):
        v = rng.uniform(0.01, 3, n).astype(f32)
        v[rng.random(n) < 0.3] = flt(np.array(QNAN, u32))[rng.integers(0, 2)]
        return v
    nans = ring(with_nans)
    all_nan = (flt(np.full(128, QNAN[0], u32)), flt(np.full(128, QNAN[1], u32)))
    return [positive, mixed, negative, constant, nans, all_nan]


@pytest.fixture(scope="module")
def agc_cases():
    """the rings, their reference tables (computed once) and the spans: every (k0, k1) on the positive ring, 64 random spans on each
    of the others"""
    rng = np.random.default_rng(32)
    rings = _agc_rings()
    tables = [_agc_tables(o, n) for o, n in rings]
    upper = np.triu(np.ones((100, 100), bool))
    assert (tables[2][1][upper] == FLT_MIN).all()                              # the all-negative ring: mx stays at its seed
    assert (tables[5][0][upper] == FLT_MAX).all() and (tables[5][1][upper] == FLT_MIN).all()
    spans = [(0, k0, k1) for k0 in range(100) for k1 in range(k0 + 1, 101)]
    for ri in range(1, len(rings)):
        for _ in range(64):
            k0 = int(rng.integers(0, 100)); k1 = int(rng.integers(k0 + 1, 101))
            spans.append((ri, k0, k1))
    return rings, tables, spans


def test_agc_scan_extremes_of_every_span(ctx, agc_cases):
    rings, tables, spans = agc_cases
    mn, mx, agc = _agc_run(ctx, False, rings, spans, [False] * len(spans))
    _agc_check("dh_agc_scan<false>", rings, tables, spans, mn, mx, agc)


def test_agc_scan_pairs_from_lds_and_from_the_window_phase(ctx, agc_cases):
    """dh_agc_scan<true>: from_win false on every span (the sources in LDS), from_win true on every span that opens its block (k0 = 0:
    the sources in the lanes' DhWinPair, the LDS rings hold junk)"""
    rings, tables, spans = agc_cases
    opening = [(ri, 0, k1) for ri in range(len(rings)) for k1 in (range(1, 101) if ri == 0 else (1, 2, 37, 99, 100))]
    all_spans = spans + opening
    mn, mx, agc = _agc_run(ctx, True, rings, all_spans, [False] * len(spans) + [True] * len(opening))
    _agc_check("dh_agc_scan<true>", rings, tables, all_spans, mn, mx, agc)


# ---------------------------------------------------------------------------------------------------------- the LDS movers
def _lds_bases():
    """per case a base for every lane: every dword alignment modulo 16 bytes for lane 0, lane strides that keep or rotate it"""
    lane = np.arange(WAVE)
    return [(a + s * lane).astype(u32) for a in range(4) for s in (4, 9, 10, 21)]


def _ramp(seed, idx):
    return (RAMP + seed + np.asarray(idx, np.int64)).astype(u32)


@pytest.mark.parametrize("op,n", [("LDS_RUN20", 20), ("LDS_RUN40", 40)])
def test_lds_run_reads_its_consecutive_words(ctx, op, n):
    bases = _lds_bases()
    hdr = np.arange(len(bases), dtype=u32)[:, None] * 7
    out = run_lanes(ctx, op, [np.concatenate(bases)], hdr=hdr)
    base = np.concatenate(bases).astype(np.int64); seed = np.repeat(hdr[:, 0], WAVE)
    for i in range(n):
        hold("%s v[%d]" % (op, i), out[i], _ramp(seed, base + i), (base.astype(u32),))


def test_lds_run20_with_pair(ctx):
    bases = _lds_bases()
    pair = [(2 * ((np.arange(WAVE) * 5 + a) % 700)).astype(u32) for a in range(len(bases))]
    out = run_lanes(ctx, "LDS_RUN20_WITH_PAIR", [np.concatenate(bases), np.concatenate(pair)])
    base, p = np.concatenate(bases).astype(np.int64), np.concatenate(pair).astype(np.int64)
    for i in range(20):
        hold("run20_with_pair v[%d]" % i, out[i], _ramp(0, base + i), (base.astype(u32),))
    hold("run20_with_pair p0", out[20], _ramp(0, p)); hold("run20_with_pair p1", out[21], _ramp(0, p + 1))


def test_lds_pairs3_now_and_raw_reads(ctx):
    bases = _lds_bases()
    b = np.concatenate(bases).astype(np.int64)
    pb, pc = (b * 3 + 1) % 1700, (b * 7 + 2) % 1700
    out = run_lanes(ctx, "LDS_PAIRS3_NOW", [b.astype(u32), pb.astype(u32), pc.astype(u32)])
    for i, src in enumerate((b, b + 1, pb, pb + 1, pc, pc + 1)):
        hold("dh_lds_pairs3_now word %d" % i, out[i], _ramp(0, src), (b.astype(u32),))
    p8 = 2 * ((b * 5 + 3) % 800)
    out = run_lanes(ctx, "LDS_READS", [b.astype(u32), p8.astype(u32)])
    for i, src in enumerate((b, b + 1, p8, p8 + 1, b, b + 1)):
        hold("raw LDS reads word %d" % i, out[i], _ramp(0, src), (b.astype(u32),))


def _store_case(ctx, op, bases, writes):
    """bases: per case the lanes' bases; writes(base) -> [(word offset from the base, value index j)].  The whole block afterwards
    against the ramp with exactly those words replaced."""
    w = np.zeros((len(bases), HDR + WAVE), u32)
    for c, b in enumerate(bases):
        w[c, 0] = 11 * c; w[c, HDR:] = b
    out = ctx.debug_seam_probe(OP[op], w)
    assert out.shape == (len(bases), LDS_WORDS)
    for c, b in enumerate(bases):
        ref = _ramp(11 * c, np.arange(LDS_WORDS))
        for lane in range(WAVE):
            for off, j in writes:
                at = int(b[lane]) + off
                assert ref[at] < MARK, "%s: the test's own lanes overlap at word %d" % (op, at)
                ref[at] = MARK + WAVE * lane + j
        bad = np.flatnonzero(out[c] != ref)
        assert bad.size == 0, "%s, lane 0 at word %d: %d words differ; first: word %d holds %#010x, should hold %#010x" % (
            op, int(b[0]), bad.size, bad[0], out[c][bad[0]], ref[bad[0]])


def test_lds_store4_at_the_window_offsets(ctx):
    lane = np.arange(WAVE)
    for op, G, pad in (("LDS_STORE4_AT", 272, lane >> 2), ("LDS_STORE4_AT_PLAIN", 256, 0 * lane)):
        bases = [(a + 4 * lane + pad).astype(u32) for a in range(4)] + [(101 + 4 * lane + pad).astype(u32)]
        _store_case(ctx, op, bases, [(G * g + i, 4 * g + i) for g in range(5) for i in range(4)])


@pytest.mark.parametrize("K", [0, 1000, 2000, 3000])
def test_lds_store_row10_columns(ctx, K):
    lane = np.arange(WAVE)
    bases = [(a + lane).astype(u32) for a in range(4)] + [(33 + lane).astype(u32), (BASE_MAX - 63 + lane).astype(u32)]
    _store_case(ctx, "LDS_STORE_ROW10_%d" % K, bases, [(K + 100 * i, i) for i in range(10)])


def test_lds_store_pair_and_rows10_pair(ctx):
    lane = np.arange(WAVE)
    _store_case(ctx, "LDS_STORE_PAIR", [(a + 2 * lane).astype(u32) for a in range(4)] + [(a + 3 * lane).astype(u32) for a in range(4)], [(0, 0), (1, 1)])
    # a row of the ring holds fifty pairs: lanes 50 .. 63 go ten rows further
    bases = [np.where(lane < 48, a + 2 * lane, 1000 + a + 2 * (lane - 48)).astype(u32) for a in range(4)]
    _store_case(ctx, "LDS_STORE_ROWS10_PAIR", bases, [(100 * i, i) for i in range(10)] + [(100 * i + 1, 10 + i) for i in range(10)])


# ------------------------------------------------------------------------------------------------------- the lane vocabulary
def test_lv_read_and_lv_down(ctx):
    rng = np.random.default_rng(40)
    v = rand_bits(rng, 8 * WAVE)
    got, = run_lanes(ctx, "LV_READ", [v])
    hold("DH_LV_READ", got, v)
    out = run_lanes(ctx, "LV_DOWN", [v])
    lane = np.arange(WAVE)
    for g, d in zip(out, (0, 1, 5, 63)):
        src = np.where(lane + d > 63, lane, lane + d)                  # a lane without a source keeps its own value
        hold("DH_LV_DOWN d = %d" % d, g, v.reshape(-1, WAVE)[:, src].reshape(-1))


def test_ls_write_then_read_leaves_m0_and_the_other_field_alone(ctx):
    rng = np.random.default_rng(41)
    v, a, b, val = (rand_bits(rng, 8 * WAVE) for _ in range(4))
    after, read, other, b_out, m0 = run_lanes(ctx, "LS_WRITE_READ", [v, a, b, val])
    hold("DH_LS_WRITE: the field afterwards", after, val)
    hold("DH_LS_READ behind each write", read, val)
    hold("DH_LV_READ behind each write", other, v.reshape(-1, WAVE)[:, ::-1].reshape(-1))
    hold("m0 behind each write: what it held in front of it", m0, np.tile(0x00A50000 + np.arange(WAVE), 8).astype(u32))
    hold("the field DH_LS_WRITE does not name", b_out, b)


def test_ls_gather(ctx):
    rng = np.random.default_rng(42)
    a = rand_bits(rng, 4 * WAVE).reshape(4, WAVE)
    j = np.stack([rng.permutation(WAVE), np.full(WAVE, 17), np.full(WAVE, 63), rng.integers(0, WAVE, WAVE)]).astype(u32)
    got, = run_lanes(ctx, "LS_GATHER", [np.zeros(4 * WAVE, u32), a.reshape(-1), j.reshape(-1)])
    hold("DH_LS_GATHER", got, np.take_along_axis(a, j.astype(np.int64), axis=1).reshape(-1))


def test_lanes_below_counts_the_vote_below_each_lane(ctx):
    rng = np.random.default_rng(43)
    masks = [0, (1 << 64) - 1] + [1 << i for i in range(64)] + [int(x) for x in rng.integers(0, 1 << 63, 64, dtype=np.uint64) * 2 + rng.integers(0, 2, 64, dtype=np.uint64)]
    hdr = np.array([[m & 0xFFFFFFFF, m >> 32] for m in masks], u32)
    got, = run_lanes(ctx, "LANES_BELOW", [], hdr=hdr)
    ref = np.array([[bin(m & ((1 << l) - 1)).count("1") for l in range(WAVE)] for m in masks], u32).reshape(-1)
    hold("DH_LANES_BELOW", got, ref)


def test_state_register_get_set_store(ctx):
    rng = np.random.default_rng(44)
    n = 16
    words = rand_bits(rng, n * WAVE).reshape(n, WAVE)
    sets = np.zeros((n, WAVE), u32)
    sets[:, 0:16:2] = rng.integers(0, WAVE, (n, 8)); sets[:, 1:16:2] = rand_bits(rng, n * 8).reshape(n, 8)
    sets[0, 0:16:2] = 5                                                # eight writes to one word: the last one stays
    first = rng.integers(0, WAVE, n); count = np.array([int(rng.integers(0, WAVE - f + 1)) for f in first])
    first[1], count[1] = 0, 64; first[2], count[2] = 63, 1; count[3] = 0
    got, stored, part = run_lanes(ctx, "STATE", [words.reshape(-1), sets.reshape(-1)], hdr=np.stack([first, count], axis=1))
    hold("DhState::get", got, words.reshape(-1))
    after = words.copy()
    for c in range(n):
        for i in range(8):
            after[c, sets[c, 2 * i]] = sets[c, 2 * i + 1]
    hold("DhState::set, store", stored, after.reshape(-1))
    ref = np.full((n, WAVE), 0xA5A5A5A5, u32)
    for c in range(n):
        ref[c, :count[c]] = after[c, first[c]:first[c] + count[c]]
    hold("DhState::store_words", part, ref.reshape(-1))


def test_bit_primitives(ctx):
    rng = np.random.default_rng(45)
    x = np.concatenate([np.array([0, 1, (1 << 64) - 1, 1 << 63, 1 << 32, 1 << 31, 0xFFFFFFFF, 0xFFFFFFFF00000000], np.uint64),
                        np.uint64(1) << np.arange(64, dtype=np.uint64), rng.integers(0, 1 << 63, 1024, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 1024, dtype=np.uint64),
                        rng.integers(0, 1 << 63, 256, dtype=np.uint64) >> rng.integers(0, 63, 256, dtype=np.uint64)])
    lo, hi = (x & np.uint64(0xFFFFFFFF)).astype(u32), (x >> np.uint64(32)).astype(u32)
    brev, ffs, top, p32, p64 = run_lanes(ctx, "BITS", [lo, hi])
    ints = [int(v) for v in x]
    hold("dh_brev32", brev, np.array([int("{:032b}".format(v & 0xFFFFFFFF)[::-1], 2) for v in ints], u32))
    hold("dh_ffs64", ffs, np.array([(v & -v).bit_length() - 1 if v else 0xFFFFFFFF for v in ints], u32))
    hold("dh_top64", top, np.array([v.bit_length() - 1 if v else 0xFFFFFFFF for v in ints], u32))
    hold("dh_popc32", p32, np.array([bin(v & 0xFFFFFFFF).count("1") for v in ints], u32))
    hold("dh_popc64", p64, np.array([bin(v).count("1") for v in ints], u32))
