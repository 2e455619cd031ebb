// wave_ops.hpp -- the float-vector, LDS and DPP primitives of the kernel bodies: the second half of the device / CPU seam.
//
// dh_portable.hpp ("THE SEAM") holds the lane loops, the per-lane value vocabularies and the integer primitives; this header
// holds what needs the short float vectors (dh_f2, dh_v4f, dh_h4, dh_f4), under the same rule: every primitive states ONCE what
// it computes, has its gfx950 form and its CPU restatement side by side under DH_ON_GPU, and one name and signature.
#pragma once

#include "dh_portable.hpp"

#define DH_FLT_MAX 3.402823466e+38f
#define DH_DBL_MAX 1.7976931348623157e+308
#define DH_FLT_MIN 1.175494351e-38f

// ---------------------------------------------------------------------------------------------
// Short vectors.  dh_f2: an aligned register pair, the operand of the packed f32 instructions (v_pk_mul_f32 / v_pk_add_f32 /
// v_pk_fma_f32); dh_v4f: sixteen bytes, one ds_read_b128; dh_h4 / dh_h8: four / eight IEEE halves (the CPU build keeps their
// bit patterns); dh_u4: four words; dh_f32x4: an MFMA accumulator.
#if DH_ON_GPU
typedef float dh_f2 __attribute__((ext_vector_type(2)));
typedef float dh_v4f __attribute__((ext_vector_type(4)));
typedef float dh_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 dh_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 dh_h4 __attribute__((ext_vector_type(4)));
typedef uint32_t dh_u4 __attribute__((ext_vector_type(4)));
#else
struct dh_f2 { float x, y; };
typedef uint16_t dh_h4[4];
#endif
// four consecutive floats from a 4-byte-aligned address (global_load_dwordx4: gfx950 allows dword alignment)
struct __attribute__((aligned(4))) dh_f4 { float x, y, z, w; };
struct alignas(16) dh_f4a { float x, y, z, w; };     // 16-byte aligned: one ds_read_b128
DH_HD dh_f4 dh_load4_unaligned(const float* p) { dh_f4 v; __builtin_memcpy(&v, p, sizeof(v)); return v; }
DH_HD void dh_store4(float* q, const dh_f4& v) { q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
DH_HD void dh_store4_unaligned(float* q, const dh_f4& v) { __builtin_memcpy(q, &v, sizeof(v)); }   // global_store_dwordx4

// ---------------------------------------------------------------------------------------------
// Pair arithmetic: element-wise, every operation rounded once, as the scalar operation on each half would be (the library is
// built with -ffp-contract=off; only the *_fma and FAST forms fuse, and they say so).  NaN and infinity propagate as in IEEE.
//   dh_f2_make(a, b)          (a, b)
//   dh_f2_mac<FAST>(c, w, a)  a + c w: product and sum rounded separately (v_pk_mul_f32, v_pk_add_f32); FAST: one fused rounding
//   dh_f2_add / _sub / _fma   a + b, a - b, fma(a, b, c)
//   dh_f2_scale(a, s)         a s
#if DH_ON_GPU
__device__ __forceinline__ dh_f2 dh_f2_make(float a, float b) { dh_f2 v; v.x = a; v.y = b; return v; }
template <bool FAST> __device__ __forceinline__ dh_f2 dh_f2_mac(float c, dh_f2 w, dh_f2 acc) {
    if (FAST) { const dh_f2 cc = dh_f2_make(c, c); return __builtin_elementwise_fma(cc, w, acc); }   // v_pk_fma_f32
    const dh_f2 p = c * w;                                 // v_pk_mul_f32, rounded
    return acc + p;                                        // v_pk_add_f32, rounded (-ffp-contract=off)
}
__device__ __forceinline__ dh_f2 dh_f2_add(dh_f2 a, dh_f2 b) { return a + b; }
__device__ __forceinline__ dh_f2 dh_f2_sub(dh_f2 a, dh_f2 b) { return a - b; }
__device__ __forceinline__ dh_f2 dh_f2_fma(dh_f2 a, dh_f2 b, dh_f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ dh_f2 dh_f2_scale(dh_f2 a, float s) { const dh_f2 ss = { s, s }; return a * ss; }
#else
inline dh_f2 dh_f2_make(float a, float b) { dh_f2 v; v.x = a; v.y = b; return v; }
template <bool FAST> inline dh_f2 dh_f2_mac(float c, dh_f2 w, dh_f2 acc) {
    if (FAST) return dh_f2_make(__builtin_fmaf(c, w.x, acc.x), __builtin_fmaf(c, w.y, acc.y));
    const float px = c * w.x, py = c * w.y;
    return dh_f2_make(acc.x + px, acc.y + py);
}
inline dh_f2 dh_f2_add(dh_f2 a, dh_f2 b) { return dh_f2_make(a.x + b.x, a.y + b.y); }
inline dh_f2 dh_f2_sub(dh_f2 a, dh_f2 b) { return dh_f2_make(a.x - b.x, a.y - b.y); }
inline dh_f2 dh_f2_fma(dh_f2 a, dh_f2 b, dh_f2 c) { return dh_f2_make(__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)); }
inline dh_f2 dh_f2_scale(dh_f2 a, float s) { return dh_f2_make(a.x * s, a.y * s); }
#endif
#if DH_ON_GPU
// dh_f2_mac with the tap as ONE HALF of a 64-bit scalar register pair (two taps per pair, chosen with op_sel): the
// packed multiply takes the pair as its scalar operand, so the taps occupy 41 / 81 SGPRs instead of as many VGPRs.
// Left to the compiler a scalar tap becomes a (c, c) pair -- two SGPRs per tap, which spills SGPRs into VGPR lanes
// in the slicer kernel -- hence the explicit instruction.  (Device only: where the operands come from, not what is
// computed -- the CPU form of its one user, dh_fir_lane, is dh_f2_mac.)
template <bool FAST, int HALF> __device__ __forceinline__ dh_f2 dh_f2_mac_pair(dh_f2 cc, dh_f2 w, dh_f2 acc) {
    dh_f2 p;
    if (FAST) {
        if (HALF == 0) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(p) : "s"(cc), "v"(w), "v"(acc));
        else           asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(p) : "s"(cc), "v"(w), "v"(acc));
        return p;
    }
    if (HALF == 0) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(p) : "s"(cc), "v"(w));
    else           asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(p) : "s"(cc), "v"(w));
    return acc + p;                                        // v_pk_add_f32, rounded (-ffp-contract=off)
}
#endif

// s v for a wave-uniform s, one rounding.  Device: one v_mul_f32 that takes s from its scalar register and writes where the
// caller wants the result: left to itself the compiler packs a lane's sixteen such multiplies and pays for it with ~29
// register moves (halves gathered into pairs before, results copied into the outputs' registers after)
DH_HD float dh_mul_uniform(float s, float v) {
#if DH_ON_GPU
    float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(v)); return r;
#else
    return v * s;
#endif
}

// x / d for a float constant d (the samples per symbol: `volume_sum / samplesPerSymbol`, gfsk_demodulator.cpp:83), r =
// RN(1 / d): q0 = RN(x r) is within 1 ulp of x / d, the FMA delivers the residual x - d q0 exactly, and
// RN(q0 + residual * r) is then the correctly rounded quotient (Markstein's theorem; it needs r correctly rounded and
// no underflow / overflow on the way).  Three instructions instead of the eleven of an IEEE division; 0, tiny, huge
// and non-finite x (anything outside 2^-100 <= |x| <= 2^100) take the real division.  tests/test_numerics.py runs all
// 2^32 floats through it for d = 10 (and the other sps values on a sample).
DH_HD float dh_div_const(float x, float d, float r) {
    union { float f; uint32_t u; } a; a.f = x;
    const uint32_t t = (a.u << 1) - 2u * 0x0D800000u;                   // bits(2^-100) = (127 - 100) << 23
    if (t > 2u * (0x71800000u - 0x0D800000u)) return x / d;             // bits(2^100) = (127 + 100) << 23
    const float q0 = x * r;
    const float rem = __builtin_fmaf(-q0, d, x);
    return __builtin_fmaf(rem, r, q0);
}
// the same for a pair of operands: each half is dh_div_const of that half, bit for bit (device: v_pk_mul_f32 + two
// v_pk_fma_f32 for both; one range test on the larger of the two words)
#if DH_ON_GPU
__device__ __forceinline__ dh_f2 dh_div_const2(dh_f2 x, float d, float r) {
    const uint32_t ta = (__float_as_uint(x.x) << 1) - 2u * 0x0D800000u, tb = (__float_as_uint(x.y) << 1) - 2u * 0x0D800000u;
    if (__builtin_expect((ta > tb ? ta : tb) > 2u * (0x71800000u - 0x0D800000u), 0)) { dh_f2 q; q.x = dh_div_const(x.x, d, r); q.y = dh_div_const(x.y, d, r); return q; }
    const dh_f2 rr = { r, r }, dd = { -d, -d };
    const dh_f2 q0 = x * rr;
    const dh_f2 rem = __builtin_elementwise_fma(q0, dd, x);
    return __builtin_elementwise_fma(rem, rr, q0);
}
#else
inline dh_f2 dh_div_const2(dh_f2 x, float d, float r) { return dh_f2_make(dh_div_const(x.x, d, r), dh_div_const(x.y, d, r)); }
#endif

// an upper bound of sqrt(x), x >= 0 (a tolerance may be generous, never short): the hardware's v_sqrt_f32 (1 ulp, one
// instruction -- the correctly rounded square root this file is compiled for is twenty) on an argument kept away from
// the denormals, times 1 + 2^-20.  The two builds may differ in the last bit; both are upper bounds.
DH_HD float dh_sqrt_upper(float x) {
    const float a = x > 1e-30f ? x : 1e-30f;
    return DH_GPU_ELSE(__builtin_amdgcn_sqrtf(a), __builtin_sqrtf(a)) * 1.00000095367431640625f;
}

// ---------------------------------------------------------------------------------------------
// Minima and maxima that SKIP a NaN operand (the result is the other operand; NaN only when every operand is NaN) -- and
// the one that does not: dh_max3_abs, whose callers take max |x| of a window and want to SEE a NaN sample.
//   dh_fmin_ / dh_fmax_(a, b)   `if (b < a) a = b`, the reference's own statement: a NaN b is skipped, a NaN a stays
//   dh_vmin / dh_vmax(a, b)     v_min_f32 / v_max_f32: the operand that is not NaN -- for a NaN ENTRY b exactly what
//                               `if (v < min) min = v` does -- at one VALU instruction where compare + select cost two
//                               (a QUIET NaN, that is.  The kernels run in IEEE mode, where v_min_f32 / v_max_f32 / v_min3_f32 and
//                               their DPP forms answer a SIGNALLING NaN operand with a quiet NaN instead of skipping it -- measured
//                               through the seam probe on an MI355X: all 115 rows of the operand table with one, none skipped; a
//                               wave reduction then drops that NaN at its next step, unless the step was the last.  The operands
//                               here are sums, differences and earlier minima, never raw samples: arithmetic results, quiet.)
//   dh_min3_abs(a, b, c)        min(|a|, |b|, |c|) in one instruction (v_min3_f32).  Callers that must notice a NaN
//                               distance make sure ALL THREE are NaN then (they are: every distance of a symbol hangs
//                               on the same average and extremes) -- see P5
//   dh_max3_abs(a, b, c)        max(|a|, |b|, c), c >= 0 or NaN, in one instruction; NaN when ANY operand is NaN (v_maximum3_f32,
//                               the gfx950 form that propagates a NaN where v_max3_f32 drops it)
DH_HD float dh_fmin_(float a, float b) { return b < a ? b : a; }
DH_HD float dh_fmax_(float a, float b) { return b > a ? b : a; }
#if DH_ON_GPU
__device__ __forceinline__ float dh_vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float dh_vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float dh_min3_abs(float a, float b, float c) { float r; asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float dh_max3_abs(float a, float b, float c) { float r; asm("v_maximum3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
#else
inline float dh_vmin(float a, float b) { return __builtin_fminf(a, b); }
inline float dh_vmax(float a, float b) { return __builtin_fmaxf(a, b); }
inline float dh_min3_abs(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(__builtin_fabsf(a), __builtin_fabsf(b)), __builtin_fabsf(c)); }
inline float dh_max3_abs(float a, float b, float c) {
    if (a != a || b != b || c != c) return __builtin_nanf("");
    return __builtin_fmaxf(c, __builtin_fmaxf(__builtin_fabsf(a), __builtin_fabsf(b)));
}
#endif
// max |x| over a lane's N groups of four, 0 for none; NaN when one of them is NaN (dh_max3_abs).  Device: 2 N v_maximum3_f32 in
// ONE statement (as separate statements the compiler put an s_nop behind each)
template <int N> DH_HD float dh_max_abs_groups(const dh_f4 (&w)[N]) {
#if DH_ON_GPU
    static_assert(N == 5, "five groups of four");
    float mx;
    const dh_f4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    asm("v_maximum3_f32 %0, |%1|, |%2|, 0\n\tv_maximum3_f32 %0, |%3|, |%4|, %0\n\tv_maximum3_f32 %0, |%5|, |%6|, %0\n\tv_maximum3_f32 %0, |%7|, |%8|, %0\n\t"
        "v_maximum3_f32 %0, |%9|, |%10|, %0\n\tv_maximum3_f32 %0, |%11|, |%12|, %0\n\tv_maximum3_f32 %0, |%13|, |%14|, %0\n\tv_maximum3_f32 %0, |%15|, |%16|, %0\n\t"
        "v_maximum3_f32 %0, |%17|, |%18|, %0\n\tv_maximum3_f32 %0, |%19|, |%20|, %0"
        : "=&v"(mx) : "v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y), "v"(w1.z), "v"(w1.w), "v"(w2.x), "v"(w2.y), "v"(w2.z), "v"(w2.w),
                      "v"(w3.x), "v"(w3.y), "v"(w3.z), "v"(w3.w), "v"(w4.x), "v"(w4.y), "v"(w4.z), "v"(w4.w));
    return mx;
#else
    float mx = 0.0f;
    for (int r = 0; r < N; r++) { mx = dh_max3_abs(w[r].x, w[r].y, mx); mx = dh_max3_abs(w[r].z, w[r].w, mx); }
    return mx;
#endif
}

// ---------------------------------------------------------------------------------------------
// IEEE binary16 <-> binary32 in integer arithmetic (host and harness; the device converts in hardware): round to nearest even
DH_HD uint16_t dh_f16_bits(float f) {
    union { float f; uint32_t u; } v; v.f = f;
    const uint32_t sign = (v.u >> 16) & 0x8000u, a = v.u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t) (sign | (a > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (a >= 0x477FF000u) return (uint16_t) (sign | 0x7C00u);                         // >= 65520 rounds to infinity
    if (a < 0x33000001u) return (uint16_t) sign;                                      // <= 2^-25: zero (the tie goes to even = 0)
    const int e = (int) (a >> 23) - 127;
    uint32_t man = (a & 0x7FFFFFu) | 0x800000u, shift = e < -14 ? (uint32_t) (13 + (-14 - e)) : 13u;
    uint32_t q = man >> shift; const uint32_t rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (q & 1u))) q++;
    const uint32_t bits = e < -14 ? q : ((uint32_t) (e + 15 - 1) << 10) + q;           // (the implicit bit of q carries into the exponent)
    return (uint16_t) (sign | bits);
}
DH_HD float dh_f16_value(uint16_t h) {
    const uint32_t sign = (uint32_t) (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    union { float f; uint32_t u; } v;
    if (e == 31u) v.u = sign | 0x7F800000u | (m << 13);
    else if (e == 0u) { v.f = (float) m * 5.9604644775390625e-08f; v.u |= sign; }     // m 2^-24
    else v.u = sign | ((e + 112u) << 23) | (m << 13);
    return v.f;
}
// The split of four samples into halves for the split-f16 FIR (dsp_core.hpp): with x_s = x scale (a power of two: exact),
// h1 = f16(x_s) and h2 = f16((x_s - h1) 2^11), both conversions rounded to nearest even, x_s - h1 exact in f32.  Infinite
// and NaN samples give infinite / NaN halves; subnormal halves are kept.
// (Round 4 tried the second half as ONE fused operation per sample, h2 = f16(fma(x, 2^11 scale, -2^11 h1)) with v_fma_mixlo / mixhi_f16
// reading 2^11 h1 as a half: bit-identical, two and a half instructions per sample instead of three and a half -- and no faster,
// because v_fma_mix* issues at 8.2 cycles per wavefront against 4.2 for the conversions and packed operations it replaces
// (tools/microbench/valu_rate.hip).  Dropped.)
DH_HD void dh_f16_split4(const dh_f4& v, float scale, dh_h4& h1, dh_h4& h2) {
    const float x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float xs = x[i] * scale;                            // exact (power of two)
#if DH_ON_GPU
        const _Float16 a = (_Float16) xs;                         // v_cvt_f16_f32: round to nearest even
        const float r = xs - (float) a;                           // exact
        h1[i] = a; h2[i] = (_Float16) (r * 2048.0f);
#else
        h1[i] = dh_f16_bits(xs);
        const float r = xs - dh_f16_value(h1[i]);
        h2[i] = dh_f16_bits(r * 2048.0f);
#endif
    }
}
// The same split with the second half left on the first one's scale: h2 = f16(x_s - h1).  For |x_s| <= 1 the residual is at most
// 2^-12 in magnitude, where a half's spacing is 2^-24 (subnormals, and normals below 2^-13) or 2^-23: h2 is within 2^-24 of it, the
// same x_s = h1 + h2 + eps, |eps| <= 2^-24, as above -- without the multiplication.  The FIR that reads these halves carries the
// 2^11 in its taps instead (dsp_core.hpp: the one-chain form of dh_fir_f16).
// Device: the difference as two v_pk_add_f32 with the second operand negated, written out -- left to the compiler, the
// subtraction and the conversion behind it became one v_fma_mixlo_f16 per sample (8 cycles a wavefront against 4) with scalar
// multiplications and subtractions around it, nine instructions per window MORE than the scaled split: four samples are two packed
// multiplications, two packed conversions, four conversions back, two packed additions and two packed conversions.
DH_HD void dh_f16_split4_plain(const dh_f4& v, float scale, dh_h4& h1, dh_h4& h2) {
#if DH_ON_GPU
    dh_v4f xs; xs.x = v.x; xs.y = v.y; xs.z = v.z; xs.w = v.w;
    xs = xs * scale;                                              // exact (power of two)
    const dh_h4 a = __builtin_convertvector(xs, dh_h4);           // v_cvt_pk_f16_f32: round to nearest even
    const dh_v4f af = __builtin_convertvector(a, dh_v4f);
    const dh_f2 x01 = xs.xy, x23 = xs.zw, a01 = af.xy, a23 = af.zw;
    dh_f2 r01, r23;                                               // xs - a: exact
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r01) : "v"(x01), "v"(a01));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r23) : "v"(x23), "v"(a23));
    dh_v4f r; r.xy = r01; r.zw = r23;
    h1 = a; h2 = __builtin_convertvector(r, dh_h4);
#else
    const float x[4] = { v.x, v.y, v.z, v.w };
    for (int i = 0; i < 4; i++) {
        const float xs = x[i] * scale;                            // exact (power of two)
        h1[i] = dh_f16_bits(xs);
        h2[i] = dh_f16_bits(xs - dh_f16_value(h1[i]));
    }
#endif
}
// *dst = v for four halves: one 8-byte store (the CPU build's dh_h4 is an array of four bit patterns, which has no assignment)
DH_HD void dh_h4_store(dh_h4* dst, const dh_h4& v) { __builtin_memcpy(dst, &v, sizeof(dh_h4)); }

// ---------------------------------------------------------------------------------------------
// LDS reads the compiler does not track.  A read issued from inline asm is in flight until an `s_waitcnt lgkmcnt(0)` that
// names its destination registers; nothing may touch them in between (tests/test_isa_contract.py checks the generated code).
#if DH_ON_GPU
// dh_lds_read2<O0, O1>(addr): the words at byte address addr + 4 O0 and addr + 4 O1 as a pair (one ds_read2_b32)
template <int O0, int O1> __device__ __forceinline__ dh_f2 dh_lds_read2(uint32_t addr) {
    static_assert(O0 < 256 && O1 < 256, "ds_read2_b32 offsets are 8-bit dword counts");
    dh_f2 v;
    asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(v) : "v"(addr), "n"(O0), "n"(O1) : "memory");
    return v;
}
// (eight bytes from a four-byte aligned address: the queue's LDS alignment mode is "unaligned" on this target)
template <int OFF_BYTES> __device__ __forceinline__ dh_f2 dh_lds_read_b64(uint32_t addr) {
    dh_f2 v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF_BYTES) : "memory");
    return v;
}
template <int OFF_BYTES> __device__ __forceinline__ float dh_lds_read_b32(uint32_t addr) {
    float v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF_BYTES) : "memory");
    return v;
}
// the wait that settles such reads: names their destinations (the compiler knows nothing of the reads and adds no wait of its own --
// where a value is wanted only phases later, a wait of the compiler's at the first use would drain every LDS store issued since)
__device__ __forceinline__ void dh_lds_reads_done(float& a, float& b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b) :: "memory"); }
__device__ __forceinline__ uint32_t dh_lds_addr(const float* p) { return (uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) p; }
template <int OFF_BYTES> __device__ __forceinline__ dh_v4f dh_lds_read_b128(uint32_t addr) {
    dh_v4f v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF_BYTES) : "memory");
    return v;
}
#endif
// This lane's N consecutive floats from a 4-byte-aligned LDS address: v[i] = src[i].  Device: N / 4 ds_read_b128 (sixteen
// bytes from a four-byte aligned address) at compile-time offsets from one base, all in flight together, ONE wait.  N = 20, 40.
template <int N> DH_HD void dh_lds_run(const float* src, float (&v)[N]) {
#if DH_ON_GPU
    static_assert(N == 20 || N == 40, "five or ten 16-byte reads");
    const uint32_t a = (uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) src;
    dh_v4f x0 = dh_lds_read_b128<0>(a), x1 = dh_lds_read_b128<16>(a), x2 = dh_lds_read_b128<32>(a), x3 = dh_lds_read_b128<48>(a), x4 = dh_lds_read_b128<64>(a);
    if constexpr (N == 20) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4) :: "memory");
        v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w; v[8] = x2.x; v[9] = x2.y;
        v[10] = x2.z; v[11] = x2.w; v[12] = x3.x; v[13] = x3.y; v[14] = x3.z; v[15] = x3.w; v[16] = x4.x; v[17] = x4.y; v[18] = x4.z; v[19] = x4.w;
    } else {
        dh_v4f x5 = dh_lds_read_b128<80>(a), x6 = dh_lds_read_b128<96>(a), x7 = dh_lds_read_b128<112>(a), x8 = dh_lds_read_b128<128>(a), x9 = dh_lds_read_b128<144>(a);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(x8), "+v"(x9) :: "memory");
        const dh_v4f x[10] = { x0, x1, x2, x3, x4, x5, x6, x7, x8, x9 };
#pragma unroll
        for (int i = 0; i < 10; i++) { v[4 * i] = x[i].x; v[4 * i + 1] = x[i].y; v[4 * i + 2] = x[i].z; v[4 * i + 3] = x[i].w; }
    }
#else
    for (int i = 0; i < N; i++) v[i] = src[i];
#endif
}
// dh_lds_run<20> and, requested in front of it and settled by the same wait, the two floats at `pair` (8-byte aligned): p0 =
// pair[0], p1 = pair[1].  Device: a read the compiler does not track -- one it tracks it waits for at the first use, and where that
// is phases later the wait drains every LDS store issued in between.
DH_HD void dh_lds_run20_with_pair(const float* src, float (&v)[20], const float* pair, float& p0, float& p1) {
#if DH_ON_GPU
    dh_f2 q = dh_lds_read_b64<0>((uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) pair);
    dh_lds_run<20>(src, v);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q) :: "memory");
    p0 = q.x; p1 = q.y;
#else
    dh_lds_run<20>(src, v);
    p0 = pair[0]; p1 = pair[1];
#endif
}
// Three pairs of neighbouring floats from LDS, here and now: a = (pa[0], pa[1]), b and c likewise.  Device: three ds_read2_b32 the
// compiler does not track, in flight together, and their wait -- for a rare path that joins a usual one which loads nothing:
// the wait for a tracked load is placed behind the join and drains, on the usual path, every LDS store still in flight.
DH_HD void dh_lds_pairs3_now(const float* pa, const float* pb, const float* pc, dh_f2& a, dh_f2& b, dh_f2& c) {
#if DH_ON_GPU
    a = dh_lds_read2<0, 1>((uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) pa);
    b = dh_lds_read2<0, 1>((uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) pb);
    c = dh_lds_read2<0, 1>((uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) pc);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c) :: "memory");
#else
    a = dh_f2_make(pa[0], pa[1]); b = dh_f2_make(pb[0], pb[1]); c = dh_f2_make(pc[0], pc[1]);
#endif
}

// LDS stores the compiler does not track: dh_lds_stores_done() must come before the barrier that publishes them (where one does:
// a block that is ONE wavefront's needs neither, its LDS instructions complete in the order they were issued).
//   dh_lds_store4_at<OFF_WORDS>(base, v)   base[OFF_WORDS .. OFF_WORDS + 3] = v
//   dh_lds_store_row10<K>(base, a0 .. a9)  base[100 i + K] = a_i: ten floats into one column of the transposed variance
//                                          ring (row i is DH_VARIANCE_SYMBOLS = 100 words further; K = column offset)
// Four consecutive floats to LDS at `base` + a compile-time offset (the padded window is only dword aligned, so the
// widest store the hardware takes is a dword pair; the compiler adds the offset to the base with one VALU instruction
// per pair because a ds_write2_b32 offset only reaches 255 dwords -- four ds_write_b32 with 16-bit byte offsets cost
// LDS issue slots, which this kernel has to spare, and no VALU at all).  The row stores likewise: ten ds_write_b32 with
// immediate offsets from one address, no vector arithmetic.
#if DH_ON_GPU
template <int OFF_WORDS> __device__ __forceinline__ void dh_lds_store4_at(float* base, const dh_f4& v) {
    static_assert(4 * OFF_WORDS + 12 < 65536, "ds_write_b32 offsets are 16-bit byte counts");
    const uint32_t addr = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) float*) base;
    asm volatile("ds_write_b32 %0, %1 offset:%5\n\tds_write_b32 %0, %2 offset:%6\n\tds_write_b32 %0, %3 offset:%7\n\tds_write_b32 %0, %4 offset:%8"
                 :: "v"(addr), "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w), "n"(4 * OFF_WORDS), "n"(4 * OFF_WORDS + 4), "n"(4 * OFF_WORDS + 8), "n"(4 * OFF_WORDS + 12) : "memory");
}
__device__ __forceinline__ void dh_lds_stores_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int K> __device__ __forceinline__ void dh_lds_store_row10(float* base, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7, float a8, float a9) {
    const uint32_t addr = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) float*) base;
    asm volatile("ds_write_b32 %0, %1 offset:%11\n\tds_write_b32 %0, %2 offset:%12\n\tds_write_b32 %0, %3 offset:%13\n\tds_write_b32 %0, %4 offset:%14\n\t"
                 "ds_write_b32 %0, %5 offset:%15\n\tds_write_b32 %0, %6 offset:%16\n\tds_write_b32 %0, %7 offset:%17\n\tds_write_b32 %0, %8 offset:%18\n\t"
                 "ds_write_b32 %0, %9 offset:%19\n\tds_write_b32 %0, %10 offset:%20"
                 :: "v"(addr), "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7), "v"(a8), "v"(a9),
                    "n"(4 * K), "n"(4 * (K + 100)), "n"(4 * (K + 200)), "n"(4 * (K + 300)), "n"(4 * (K + 400)), "n"(4 * (K + 500)), "n"(4 * (K + 600)),
                    "n"(4 * (K + 700)), "n"(4 * (K + 800)), "n"(4 * (K + 900)) : "memory");
}
//   dh_lds_store_pair(base, a, b)          base[0] = a, base[1] = b
//   dh_lds_store_rows10_pair(base, a, b)   base[100 i] = a[i], base[100 i + 1] = b[i]: two neighbouring columns of the ring
// Two neighbouring words from two registers of their own: one ds_write2_b32 (offset1 = offset0 + 1).  A ds_write_b64 wants its
// two words in an aligned register pair -- the columns' values come out of different 16-byte reads, a v_mov per pair -- and
// an 8-byte aligned address; this form takes any registers and any dword address.  Its offsets are 8-bit dword counts: three
// rows per base, one VALU addition per further base.
__device__ __forceinline__ void dh_lds_store_pair(float* base, float a, float b) {
    const uint32_t addr = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) float*) base;
    asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" :: "v"(addr), "v"(a), "v"(b) : "memory");
}
__device__ __forceinline__ void dh_lds_store_rows3_pair_(uint32_t addr, float a0, float b0, float a1, float b1, float a2, float b2) {
    asm volatile("ds_write2_b32 %0, %1, %2 offset1:1\n\tds_write2_b32 %0, %3, %4 offset0:100 offset1:101\n\tds_write2_b32 %0, %5, %6 offset0:200 offset1:201"
                 :: "v"(addr), "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2) : "memory");
}
__device__ __forceinline__ void dh_lds_store_rows10_pair(float* base, const float (&a)[10], const float (&b)[10]) {
    const uint32_t addr = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) float*) base;
    dh_lds_store_rows3_pair_(addr, a[0], b[0], a[1], b[1], a[2], b[2]);
    dh_lds_store_rows3_pair_(addr + 1200u, a[3], b[3], a[4], b[4], a[5], b[5]);
    dh_lds_store_rows3_pair_(addr + 2400u, a[6], b[6], a[7], b[7], a[8], b[8]);
    asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" :: "v"(addr + 3600u), "v"(a[9]), "v"(b[9]) : "memory");
}
#else
template <int OFF_WORDS> inline void dh_lds_store4_at(float* base, const dh_f4& v) { dh_store4(base + OFF_WORDS, v); }
inline void dh_lds_stores_done() {}
inline void dh_lds_store_pair(float* base, float a, float b) { base[0] = a; base[1] = b; }
inline void dh_lds_store_rows10_pair(float* base, const float (&a)[10], const float (&b)[10]) {
    for (int i = 0; i < 10; i++) { base[i * 100] = a[i]; base[i * 100 + 1] = b[i]; }
}
template <int K> inline void dh_lds_store_row10(float* base, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7, float a8, float a9) {
    const float a[10] = { a0, a1, a2, a3, a4, a5, a6, a7, a8, a9 };
    for (int i = 0; i < 10; i++) base[i * 100 + K] = a[i];
}
#endif

// ---------------------------------------------------------------------------------------------
// dh_l2_touch_lines(base, n, sink): lane l with 32 l < n requests the dword at base + 32 l, one per 128-byte line, which
// pulls the lines into L2; the values are not wanted.  Device: global_load_lds_dword drops them (lane l -> sink + l) into
// 64 words of LDS that are dead meanwhile, so no vector register is tied to a load the compiler does not know about; the
// LDS base goes through m0, which belongs to the compiler -- saved and restored.  The lane id is taken afresh (not
// loop-invariant: a hoisted address is spilled).  dh_global_loads_done() waits for the last of them (s_waitcnt vmcnt(0)).
// The CPU build has no cache to warm: both do nothing.
DH_HD void dh_l2_touch_lines(const float* base, uint32_t n, float* sink) {
#if DH_ON_GPU
    const uint32_t pf_lane = (uint32_t) dh_fresh_lane_id_();
    const float* line = base + 32u * pf_lane;
    const uint32_t sink_addr = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) float*) sink;
    uint32_t keep_m0;
    if (32u * pf_lane < n)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tglobal_load_lds_dword %2, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep_m0) : "s"(sink_addr), "v"(line) : "memory");
#endif
}
DH_HD void dh_global_loads_done() { DH_GPU_ELSE(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"), (void) 0); }

// A lane's tap fragments of the split-f16 FIR (dsp_core.hpp: dh_fir_f16), N 16-byte pieces out of a table [N][DH_WAVE][4]:
//   DH_TAPFRAG_REGS(name, N, table)         declares them
//   DH_TAPFRAG_LOAD(name, N, table, on)     requests them (16-byte loads, 1 KiB per instruction), one iteration ahead of their use
//   DH_TAPFRAG_SETTLE(name, N, on)          makes the compiler see them landed
// (`on`: a compile-time switch -- kernels without that FIR declare the registers and never fill them.)  Every path through the FIR phase must leave these loads landed, also the rare ones that never look at the fragments: otherwise
// the compiler's wait-count bookkeeping still sees them in flight further down, and the first instruction that reuses one of
// their registers -- in the slicing phase -- gets an s_waitcnt vmcnt(0), which also waits for the NEXT window's loads,
// requested after P3 precisely so that they can stay in flight through P4 - P6 (it cost 1 ms of a 6.8 ms step).  The CPU build
// reads the table in place: `name` is a pointer to it, load and settle do nothing.
#if DH_ON_GPU
#define DH_TAPFRAG_REGS(name, N, table) dh_u4 name[N]
#define DH_TAPFRAG_LOAD(name, N, table, on) do { if constexpr (on) { const dh_u4* tf_ = reinterpret_cast<const dh_u4*>(table) + dh_fresh_lane_id_(); \
        _Pragma("unroll") for (int f_ = 0; f_ < (N); f_++) name[f_] = tf_[DH_WAVE * f_]; } } while (0)
#define DH_TAPFRAG_SETTLE(name, N, on) do { if constexpr (on) { _Pragma("unroll") for (int f_ = 0; f_ < (N); f_++) \
        asm volatile("" :: "v"(name[f_])); } } while (0)
#else
#define DH_TAPFRAG_REGS(name, N, table) const uint32_t (* const name)[DH_WAVE][4] = reinterpret_cast<const uint32_t (*)[DH_WAVE][4]>(table)
#define DH_TAPFRAG_LOAD(name, N, table, on) ((void) 0)
#define DH_TAPFRAG_SETTLE(name, N, on) ((void) 0)
#endif

// ---------------------------------------------------------------------------------------------
// Wave-wide scans, shifts and reductions of per-lane floats, on the VALU's DPP network.  A DPP read needs two wait states
// after the VALU write of its source, and a VALU write of EXEC just before would need five: inline asm gets no hazard
// handling from the compiler, hence the s_nop padding and the interleaved streams.  All skip NaN operands as dh_vmin / dh_vmax do.
#if DH_ON_GPU
// Inclusive wave64 prefix min (mn, mn2) and max (mx, mx2) in lane order, two pairs at once (prefix and suffix scans of the AGC):
// row_shr 1/2/4/8 inside each row of 16, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.  Lanes without
// a source keep their value.  Four streams interleaved: a DPP read always finds its source written three instructions earlier -- no s_nop between the steps.
__device__ __forceinline__ void dh_wave_prefix_minmax2(float& mn, float& mx, float& mn2, float& mx2) {
#define DH_SCAN_STEP4(ctrl) \
    "v_min_f32_dpp %0, %0, %0 " ctrl "\n\tv_max_f32_dpp %1, %1, %1 " ctrl "\n\tv_min_f32_dpp %2, %2, %2 " ctrl "\n\tv_max_f32_dpp %3, %3, %3 " ctrl "\n\t"
    asm volatile("s_nop 4\n\t"
                 DH_SCAN_STEP4("row_shr:1 row_mask:0xf bank_mask:0xf")
                 DH_SCAN_STEP4("row_shr:2 row_mask:0xf bank_mask:0xf")
                 DH_SCAN_STEP4("row_shr:4 row_mask:0xf bank_mask:0xf")
                 DH_SCAN_STEP4("row_shr:8 row_mask:0xf bank_mask:0xf")
                 DH_SCAN_STEP4("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 DH_SCAN_STEP4("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 1"
                 : "+v"(mn), "+v"(mx), "+v"(mn2), "+v"(mx2));
#undef DH_SCAN_STEP4
}
// the previous lane's value of four registers at once (lane 0 keeps the identities it is given)
__device__ __forceinline__ void dh_wave_prev4(float& a, float& b, float& c, float& d, float va, float vb, float vc, float vd) {
    asm volatile("s_nop 4\n\tv_mov_b32_dpp %0, %4 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %5 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b32_dpp %2, %6 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %3, %7 wave_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(va), "v"(vb), "v"(vc), "v"(vd));
}

// maximum over the wavefront of a per-lane value, wave-uniform (row_shr 1/2/4/8 inside each row of 16, row_bcast:15 / :31
// across rows -- the running maximum ends up in lane 63; v_max_f32 skips a NaN operand.  max |x| of a window, which must
// not lose a NaN, goes through dh_wave_max_nan below)
__device__ __forceinline__ float dh_wave_max(float v) {
#define DH_MAX_STEP(ctrl) "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 " ctrl "\n\t"
    asm volatile("s_nop 4\n\t"
                 DH_MAX_STEP("row_shr:1 row_mask:0xf bank_mask:0xf") DH_MAX_STEP("row_shr:2 row_mask:0xf bank_mask:0xf")
                 DH_MAX_STEP("row_shr:4 row_mask:0xf bank_mask:0xf") DH_MAX_STEP("row_shr:8 row_mask:0xf bank_mask:0xf")
                 DH_MAX_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf") DH_MAX_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 1" : "+v"(v));
#undef DH_MAX_STEP
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// The same reduction for a maximum that must not lose a NaN (max |x| of a window: dh_max3_abs hands a NaN on, this does too):
// on the BIT PATTERNS, v_max_u32.  The values are magnitudes -- sign bit clear -- so unsigned order is float order, with every
// NaN above infinity; a NaN in any lane is the result.
__device__ __forceinline__ float dh_wave_max_nan(float f) {
    uint32_t v = __float_as_uint(f);
#define DH_MAX_STEP(ctrl) "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 " ctrl "\n\t"
    asm volatile("s_nop 4\n\t"
                 DH_MAX_STEP("row_shr:1 row_mask:0xf bank_mask:0xf") DH_MAX_STEP("row_shr:2 row_mask:0xf bank_mask:0xf")
                 DH_MAX_STEP("row_shr:4 row_mask:0xf bank_mask:0xf") DH_MAX_STEP("row_shr:8 row_mask:0xf bank_mask:0xf")
                 DH_MAX_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf") DH_MAX_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 1" : "+v"(v));
#undef DH_MAX_STEP
    return __int_as_float(__builtin_amdgcn_readlane((int) v, 63));
}
// minimum of lanes 0..15 (one DPP row), valid in lane 15 and returned wave-uniform: four v_min_f32 with row_shr
__device__ __forceinline__ float dh_row_min_to_lane15(float v) {
    asm volatile("s_nop 4\n\tv_min_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
                 : "+v"(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15));
}
#else
inline float dh_wave_max_lanes(const float (&a)[DH_WAVE][1]) {
    float m = 0.0f; bool any = false;
    for (int l = 0; l < DH_WAVE; l++) { m = __builtin_fmaxf(m, a[l][0]); any |= a[l][0] == a[l][0]; }
    return any ? m : __builtin_nanf("");
}
inline float dh_wave_max_nan_lanes(const float (&a)[DH_WAVE][1]) {
    uint32_t m = 0;
    for (int l = 0; l < DH_WAVE; l++) { union { float f; uint32_t u; } b; b.f = a[l][0]; if (b.u > m) m = b.u; }
    union { float f; uint32_t u; } r; r.u = m;
    return r.f;
}
inline float dh_wave_min_lanes(const float (&a)[DH_WAVE][1], int lanes) {
    float m = DH_FLT_MAX; bool any = false;
    for (int l = 0; l < lanes; l++) { m = dh_fmin_(m, a[l][0]); any |= a[l][0] == a[l][0]; }
    return any ? m : __builtin_nanf("");
}
#endif
// Reductions of a DH_LANE_ARRAY(float, a, 1), wave-uniform results; NaN lanes are skipped, except by DH_WAVE_MAX_NAN.  When EVERY
// lane they look at is NaN there is nothing to skip to and the three skipping ones give NaN (v_max_f32 / v_min_f32 of two NaNs; until
// the seam probe ran them alone the restatements gave their seeds, 0 and FLT_MAX, and DH_WAVE_MAX's statement said 0).  No caller
// depends on it: the sps-10 votes keep lanes that hold no phase at FLT_MAX (dsp_core.hpp: `own`, "lanes 10 .. 15 hold FLT_MAX"),
// and where all 64 lanes hold phases (a run-time sps of 64 or more) a NaN interval clears its lane's bit in v_ok, which every
// verdict that looks at the minimum requires to be full.
//   DH_WAVE_MAX(a)   the largest value of the 64 lanes, of values >= 0
//   DH_WAVE_MAX_NAN(a)   the same of magnitudes (sign bit clear), but NaN when ANY lane is NaN
//   DH_WAVE_MIN(a)   the smallest value of the 64 lanes, of values <= FLT_MAX (device: -max(-a), exact)
//   DH_ROW0_MIN(a)   the smallest value of lanes 0..15, of values <= FLT_MAX
#if DH_ON_GPU
#define DH_WAVE_MAX(a) dh_wave_max((a)[0])
#define DH_WAVE_MAX_NAN(a) dh_wave_max_nan((a)[0])
#define DH_WAVE_MIN(a) (-dh_wave_max(-(a)[0]))
#define DH_ROW0_MIN(a) dh_row_min_to_lane15((a)[0])
#else
#define DH_WAVE_MAX(a) dh_wave_max_lanes(a)
#define DH_WAVE_MAX_NAN(a) dh_wave_max_nan_lanes(a)
#define DH_WAVE_MIN(a) dh_wave_min_lanes(a, DH_WAVE)
#define DH_ROW0_MIN(a) dh_wave_min_lanes(a, 16)
#endif

// s and q (DH_LANE_ARRAY(float, , 1)) each replaced by the sum over the lane and its four lower neighbours INSIDE its row of
// sixteen, a missing neighbour counting as 0, in the order ((x[l] + x[l-1]) + (x[l-2] + x[l-3])) + x[l-4]: three roundings.
// Defined in every lane.  Device: row_shr with bound_ctrl (lanes without a source read 0), the two streams interleaved.
DH_HD void dh_row_sum5_pair(DH_LANE_ARRAY(float, (&gs), 1), DH_LANE_ARRAY(float, (&gq), 1)) {
#if DH_ON_GPU
    float s = gs[0], q = gq[0], t1, t2, u1, u2;
    asm volatile("s_nop 4\n\t"               // (a VALU write of EXEC just before would need 5 wait states ahead of a DPP op)
                 "v_add_f32_dpp %0, %4, %4 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %2, %5, %5 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "s_nop 0\n\t"                // (a DPP read needs two wait states after the write of its source: the other stream's add + this)
                 "v_add_f32_dpp %1, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %3, %2, %2 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %1, %4, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %3, %5, %3 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0"
                 : "=&v"(t1), "=&v"(t2), "=&v"(u1), "=&v"(u2) : "v"(s), "v"(q));
    gs[0] = t2; gq[0] = u2;
#else
    float ts[DH_WAVE], tq[DH_WAVE];
    for (int l = 0; l < DH_WAVE; l++) {
        const int c = l & 15;
        auto at = [&](float (*arr)[1], int d) { return c - d >= 0 ? arr[l - d][0] : 0.0f; };
        ts[l] = ((at(gs, 0) + at(gs, 1)) + (at(gs, 2) + at(gs, 3))) + at(gs, 4);
        tq[l] = ((at(gq, 0) + at(gq, 1)) + (at(gq, 2) + at(gq, 3))) + at(gq, 4);
    }
    for (int l = 0; l < DH_WAVE; l++) { gs[l][0] = ts[l]; gq[l][0] = tq[l]; }
#endif
}
