// dsp_core.hpp -- RRC FIR + GFSK/FSK symbol slicer, one channel per wavefront.
//
// Arithmetic contract (bit-exact dibits need bit-exact floats):
//   FIR      y[n] = (float)((double)(((0 + c0*x[n-N]) + c1*x[n-N+1]) + ... + cN*x[n]) / gain)
//            every product and every sum separately rounded to float, taps in order
//            (src/rrc_filter/rrc_filter.cpp:22-34).  Built with -ffp-contract=off; the only
//            fused variant is the explicitly requested DH_FLAG_FAST_FIR path (__builtin_fmaf).
//   slicer   window sums in sample order, float; AGC thresholds in double, stored to float;
//            timing variance in double, 100-term sums in order
//            (src/gfsk_demodulator/gfsk_demodulator.cpp:24-122).
//
// Block-parallel formulation of the symbol loop: the +-1 sample timing step is
// decided only at the 100th symbol of a variance block and applied after the first symbol of
// the next block, so inside one block every symbol window position is known up front:
//   start[k] = p + (k - k0)*sps + (k0 == 0 && k > 0 ? pending_offset : 0)
// Lanes take symbols; the 100-entry sliding AGC min/max becomes
//   min_k = min( prefix-min over {old[0..k0), new[k0..k]}, suffix-min over old(k..99] )
// (two wave scans: min/max are exact in any order), and the per-phase variance runs on `sps`
// lanes at the end of the block.
#pragma once

#include "dh_portable.hpp"
#include "wave_ops.hpp"

#define DH_VARIANCE_SYMBOLS 100      // include/gfsk_demodulator.hpp:5
#define DH_VOLUME_RB_SIZE 100        // include/gfsk_demodulator.hpp:6
#define DH_FTILE 1024                // filtered samples produced per FIR pass (64 lanes x 16)
#define DH_FIR_L 16                  // consecutive outputs per lane
#define DH_PF_N 5                    // 16-byte prefetch loads per lane covering 1024 + 160 samples
#define DH_PF_SINK 512               // word offset inside the window block where the L2-touch loads drop their dwords (64 words)
#define DH_MAX_NZ 160
#define DH_MAX_SPS 40
// raw samples kept BEHIND the read position by the error-bounded kernels (see "Error-bounded FIR"): the 100 symbols of the
// rings + slack; and the most the tail carries between pushes: history + the last nz inputs + not yet consumed ones
DH_HD uint32_t dh_history(uint32_t sps) { return DH_VARIANCE_SYMBOLS * (sps > 10u ? sps : 10u) + 152u; }
DH_HD uint32_t dh_tail_max(uint32_t sps) { return 256u + dh_history(sps); }
#define DH_STATE_HDR 32              // u32 words of per-channel header

// per-channel state block in HBM (floats / u32 words, AoS, `state_stride` words apart):
//   [0..15]                      header: k, pending offset, tail count, symbols produced (lo),
//                                timing blocks decided by the ordered chain, timing blocks total, ...
//   [16 .. 16+100)               volume ring  (volume_rb)
//   [116 .. 116+100*sps)         variance ring (variance_rb), phase-major: [sample i][symbol k]
//   [.. + dh_tail_max(sps))      raw-sample tail: the last nz inputs + not yet consumed samples
enum { DH_ST_K = 0, DH_ST_OFF = 1, DH_ST_TAIL = 2, DH_ST_NSYM = 3, DH_ST_ORDERED = 4, DH_ST_BLOCKS = 5,
       DH_ST_P0 = 6,                 // read position inside the tail at the start of the next push (= history samples in front of it)
       DH_ST_CUR_START = 7, DH_ST_CUR_OFF = 8, DH_ST_PREV_START = 9, DH_ST_PREV_OFF = 10,   // filtered positions of symbol 0 of the current / previous variance block, their offsets
       DH_ST_BLOCK_FLAGS = 11,       // bit 0: the current block's start is known, bit 1: the previous block's
       DH_ST_E_CUR = 12, DH_ST_E_PREV = 13, DH_ST_E_COUNT = 14, DH_ST_E_BLOCK = 15,          // error radii of the ring entries (floats), symbols in the current bucket
       DH_ST_UNCERTAIN = 16, DH_ST_EXACT_RUNS = 17, DH_ST_EXACT_BLOCKS = 18,                    // statistics: symbols / runs / timing blocks decided by exact arithmetic
       DH_ST_PART = 19,              // tail split: the hand-over flag word of the last split push (chain_core.hpp: dh_pf_pack)
       DH_ST_DIAG = 20 };            // 20..31: diagnostic builds (phase clocks 20..27, wave timeline 28..31)
#define DH_ST_VOL DH_STATE_HDR
#define DH_ST_VAR (DH_STATE_HDR + DH_VOLUME_RB_SIZE)

struct DhDspParams {
    const float* in; size_t in_stride; uint32_t n;     // n new samples per channel (ragged pushes: the most any channel brings)
    const uint32_t* n_per;                             // ragged pushes (dh_engine_push_ragged): [B] samples of each channel, <= n; or null
    float* state; size_t state_stride;                 // per-channel state (see above), in 4-byte words
    uint8_t* syms; size_t sym_stride;                  // symbol output [B][sym_stride]
    uint32_t* sym_count;                               // [B] symbols produced by this push
    uint32_t sym_cap;                                  // max symbols a push may append per channel
    uint32_t* overflow;                                // set to 1 if sym_cap was hit
    uint32_t n_channels;
    uint32_t ch_base;                                  // first channel of this launch (a push may go out as two launches, engine.hip)
    uint32_t sps, lo, hi;                              // samples/symbol, [lo,hi) = mid-symbol evaluation window
    int32_t levels, invert;                            // 4 = GFSK, 2 = FSK
    uint32_t nz;                                       // FIR order (0 = no RRC stage)
    int32_t fast;                                      // 1 = FMA FIR
    int32_t ordered_timing;                            // 1 = always run the ordered variance chain (DH_FLAG_ORDERED_TIMING)
    int32_t exact_mode;                                // error-bounded kernels: 0 normal, 1 every symbol decided by exact arithmetic, 2 exact FIR in every run
    float err_coef;                                    // error radius of a filtered sample per unit of max |x| (dh_fir_error_coefficient)
    double gain, rgain; float inv_gain;                // rgain = 1/gain rounded to double
    float taps[DH_MAX_NZ / 2 + 1];                     // first half + centre of the symmetric response
    const uint32_t* tapfrag;                           // split-f16 FIR: the per-lane tap fragments (DhF16Taps::frag), or null
    float err_coef_f16;                                // its error radius per unit of max |x| (dh_f16_error_coefficient)
    // tail split (engine.hip, HipBackend::go_chain): the launch has two or three workgroups per channel; workgroup
    // k * split_pad + channel takes the samples [0, split_n0), [split_n0, split_n1 or the end), [split_n1, end) of the
    // channel's row for k = 0, 1, 2.  split_n0 = 0: one workgroup per channel; split_n1 = 0: two.
    uint32_t split_n0, split_n1, split_pad, part_epoch;
    // split_fixup = 1: the launch BEHIND a split launch, one workgroup per channel -- a channel whose later parts did not get
    // their hand-over (flag never came, or came from another XCD) is finished here, unsplit, from where its last completed part
    // stopped; every other workgroup leaves at once.  split_force_fail = k > 0 (tests: DH_TAIL_SPLIT_FORCE_FAIL): the SECOND parts
    // of the channels with ch % k == 1 give up without looking.
    uint32_t split_fixup, split_force_fail;
    // DH_FLAG_KEEP_FILTERED | DH_FLAG_ONE_LAUNCH on the wide filter at sps 10 (else null): the error-bounded slicer also delivers the filtered
    // samples of the push it has in LDS anyway -- filt_out[ch][t] for every new sample t -- in ONE launch.  Without DH_FLAG_FAST_FIR (KEEPF = 1) the
    // split-f16 FIR's: within 2.5e-6 of the reference's (measured 1.0e-6); with it (KEEPF = 2) the f32 FMA chain's: the 1e-6 of BASELINE configs[1]
    float* filt_out; size_t filt_stride;
};

// (behind the tail: two words per phase that round 4's ring-less experiment kept there; the layout is unchanged)
#define DH_PART_WORDS(sps) ((2u * (sps) + 4u + 3u) & ~3u)
DH_HD uint32_t dh_state_part_offset(uint32_t sps) { return DH_ST_VAR + DH_VARIANCE_SYMBOLS * sps + dh_tail_max(sps); }
DH_HD uint32_t dh_state_words(uint32_t sps) { return dh_state_part_offset(sps) + DH_PART_WORDS(sps); }

// LDS block of one wavefront.  `xf` holds the raw-sample window during the FIR (padded one word
// per 16 so that the per-lane sliding windows, 16 words apart, hit 32 different banks) and is then
// overwritten in place by the filtered samples of the run.
#define DH_XPAD(i) ((i) + ((i) >> 4))
#define DH_SCAN_N 128
// The LDS block of one wavefront, carved by dh_dsp_carve():
//   vol_old[128] vol_new[128]                                fixed part, then
//   wide filter / no filter:  tap table[112] bound[12] stats[2] pad[2] (clk[8] in DH_PHASE_CLOCKS builds)
//   narrow filter:            tapsf[84] stats[2] clk[8] pad[2] bound[16]
//   var_rb[100 * sps]     variance ring, phase-major: row i holds sample i of the last 100 symbols
//   xf[...]               raw-sample window during the FIR (padded one word per 16 so that the per-lane sliding
//                         windows, 16 words apart, hit 32 different banks), then overwritten by the filtered samples
// The wide filter's tap table is the WHOLE response between two runs of 15 zeros (tap k at word 15 + k): the matrix-pipe
// FIR (dh_fir_mfma) reads its Toeplitz operand c[p - n], p = 0..95, n = 0..15, straight out of it; `tapsf` points at tap 0,
// so everything that indexes the first half + centre still works.
// Everything that only lives between the window phase (P3) and the next staging (P7) sits INSIDE the window block,
// which is idle then: the AGC extremes mn / mx (also the scratch of the timing estimate) in its first 256 words
// (the filtered samples there are dead once P3 has copied them into the ring), the ordered-chain variances behind
// them, and the mid-symbol sums behind the last filtered sample.  10 240 bytes per wavefront for the wide filter at
// sps 10: exactly 16 wavefronts per CU.
struct DhDspShared {
    float* xf;
    float* vol_old;                                    // ring content before the current run (+ identity padding)
    float* vol_new;                                    // entries written by the current run
    float* mn; float* mx;                              // AGC window min / max per symbol of the block
    float* sum;                                        // mid-symbol window sums of the current run
    double* variance;                                  // [DH_MAX_SPS] per-phase variances of the ordered chain
    uint32_t* stats;                                   // timing blocks of this push: all / decided by the ordered chain
    uint32_t* clk;                                     // DH_PHASE_CLOCKS builds only
    float* tapsf;                                      // FIR taps (first half + centre; the wide filter: all of them, see above)
    float* var_rb;
    float* bound;                                      // bookkeeping of the error-bounded kernels (DhBoundState, 16 words)
};

#define DH_TAP_LEAD 15                                 // zeros in front of (and behind) the wide filter's tap table
// words in front of the variance ring (a multiple of 4: keeps var_rb 16-byte aligned)
DH_HD uint32_t dh_lds_fixed_words(uint32_t nz) { return nz > 80u ? 352u + 16u : 384u; }
DH_HD uint32_t dh_dsp_xf_words(uint32_t nz) {
    const uint32_t padded = DH_XPAD(DH_FTILE + nz) + 1u, with_sums = DH_FTILE + 4u + DH_SCAN_N;
    return ((padded > with_sums ? padded : with_sums) + 3u) & ~3u;
}
#define DH_RING_WORDS(sps) (DH_VARIANCE_SYMBOLS * (sps))
// (Round 4 measured kernels WITHOUT the variance ring in LDS -- per-phase sums carried instead, 6.3 KB per wavefront: the sums cost the window
// phase more than the ring costs, +4 % on the DMR chain, and a fifth wavefront per SIMD at 96 registers spills across the FIR.  Removed in
// round 5; profiles/r04_b_ab_logs.txt.)
DH_HD size_t dh_dsp_shared_bytes(uint32_t sps, uint32_t nz) {
    return sizeof(float) * (size_t) (dh_lds_fixed_words(nz) + DH_RING_WORDS(sps) + dh_dsp_xf_words(nz));
}
DH_HD DhDspShared dh_dsp_carve(void* base, uint32_t sps, uint32_t nz = 0) {          // base: 16-byte aligned
    float* f = reinterpret_cast<float*>(base);
    DhDspShared S;
    S.vol_old = f; S.vol_new = f + 128;
    if (nz > 80u) {
        S.tapsf = f + 256;
        S.stats = reinterpret_cast<uint32_t*>(f + 340); S.clk = S.stats + 2;
        S.bound = f + 352;
    } else {
        S.tapsf = f + 256 + DH_TAP_LEAD;
        S.bound = f + 256 + 112;
        S.stats = reinterpret_cast<uint32_t*>(f + 256 + 124); S.clk = reinterpret_cast<uint32_t*>(f + 384);
    }
    S.var_rb = f + dh_lds_fixed_words(nz);
    S.xf = S.var_rb + DH_RING_WORDS(sps);
    S.mn = S.xf; S.mx = S.xf + DH_SCAN_N;
    S.variance = reinterpret_cast<double*>(S.xf + 2 * DH_SCAN_N);
    S.sum = S.xf + DH_FTILE + 4;
    return S;
}

// (Wave priorities -- s_setprio around the FIR and in the decoder half -- were worth 2 % in round 2 and nothing since the FIR moved to
// the matrix cores: removed in round 5; the policies and their A/B logs are in git history and profiles/r03_b_ab_logs.txt.)

// ---------------------------------------------------------------------------------------------
// (float)((double)acc / gain), the reference's `sum / gain` with a double gain, without paying an
// IEEE double division per sample: q' = fl64(acc * fl64(1/gain)) is within 3 ulp of fl64(acc / gain);
// both round to the same float unless a float rounding boundary (mantissa bits 28..0 = 0x10000000)
// lies within that distance, or the result is a float subnormal.  Only then (p ~ 2e-8) the real
// division runs.  dh_div_gain_exact() is what the fast path must always equal (tested over 2^31
// operands in tests/test_numerics.py).
DH_HD float dh_div_gain_exact(float acc, double gain) { return (float) ((double) acc / gain); }

// fast part: returns (float) q' and sets `suspect` when the exact division has to decide.
// Both tests are "an unsigned word is small":
//   tie    t = (low word of q' << 3) + 0x80000020 <= 64: the low 29 mantissa bits of q' are within 4 ulp(double) of a
//          float midpoint (0x0FFFFFFC .. 0x10000004; the shift drops the three bits above them);
//   range  r = (bits(acc) << 1) - 1 < 2 * bits(2^-118) - 1: acc is non-zero and |acc| < 2^-118.  Results that may be
//          float subnormals round at other bit positions: with 1 < gain < 128 they need |acc| < 2^-118; the quotient of
//          a finite acc cannot overflow.  0, inf and nan are fine: acc * rgain is then acc / gain bit for bit.
// One v_lshl_add_u32 each; a lane's sixteen outputs share ONE decision, so the words are min-reduced (v_min3_u32,
// half an instruction per word) and compared once (dh_fir_finish).
#define DH_DIV_TIE_MAX 64u
#define DH_DIV_RANGE_MAX (2u * 0x04800000u - 1u)             /* bits(2^-118) = (127 - 118) << 23 */
DH_HD float dh_div_gain_words(float acc, double rgain, uint32_t& tie, uint32_t& range) {
    const double q = (double) acc * rgain;
    union { double d; uint64_t u; } b; b.d = q;
    union { float f; uint32_t u; } a; a.f = acc;
    tie = ((uint32_t) b.u << 3) + 0x80000020u;
    range = (a.u << 1) + 0xFFFFFFFFu;
    return (float) q;
}
DH_HD float dh_div_gain_fast(float acc, double rgain, bool& suspect) {
    uint32_t tie, range;
    const float y = dh_div_gain_words(acc, rgain, tie, range);
    suspect = tie <= DH_DIV_TIE_MAX || range < DH_DIV_RANGE_MAX;
    return y;
}

DH_HD float dh_div_gain(float acc, double gain, double rgain) {
    bool suspect;
    const float y = dh_div_gain_fast(acc, rgain, suspect);
    return suspect ? dh_div_gain_exact(acc, gain) : y;
}

// ---------------------------------------------------------------------------------------------
// FIR pass: lane computes outputs [base, base+16) of the tile from the padded LDS window.
//   x[e] = xs[DH_XPAD(e)] holds input sample (tile_start - NZ + e);  out[j] = sum_i c[i]*x[base+j+i]
//
// Register layout chosen for packed fp32 (v_pk_mul_f32 / v_pk_add_f32 work on aligned VGPR pairs):
// the 16 outputs are two groups of 8, and output j of group A shares a register pair with output j
// of group B.  The sliding window then holds pairs (x[t], x[t+8]); sliding by one tap renames
// pairs instead of re-aligning them, and one ds_read2_b32 fills a pair.  Straight-line after
// unrolling: 8 window pairs + 8 accumulator pairs + the taps (one VGPR each).
#define DH_FIR_H (DH_FIR_L / 2)
#define DH_XLOFF(e) ((e) + ((e) >> 4))                 // dword offset of window element e from the lane's base

// (float)((double)acc / gain) for the 16 accumulators of a lane, see dh_div_gain_fast
template <bool FAST>
DH_HD void dh_fir_finish(const float* acc, double gain, double rgain, float inv_gain, float* out16, bool* nonfinite = nullptr) {
    if (FAST) {
#pragma unroll
        for (int j = 0; j < DH_FIR_L; j++) out16[j] = dh_mul_uniform(inv_gain, acc[j]);
        if (nonfinite) {                                  // NaN or infinity in any accumulator: 0 * acc is then NaN
            float t = 0.0f;
#pragma unroll
            for (int j = 0; j < DH_FIR_L; j++) t = __builtin_fmaf(acc[j], 0.0f, t);
            *nonfinite = !(t == 0.0f);
        }
    } else {
        uint32_t tmin = 0xFFFFFFFFu, rmin = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < DH_FIR_L; j++) {
            uint32_t t, r;
            out16[j] = dh_div_gain_words(acc[j], rgain, t, r);
            tmin = dh_min<uint32_t>(tmin, t); rmin = dh_min<uint32_t>(rmin, r);
        }
        const bool any = tmin <= DH_DIV_TIE_MAX || rmin < DH_DIV_RANGE_MAX;
        if (any) {                                        // ~2e-8 per sample: one copy of the IEEE division, not sixteen
#pragma unroll 1
            for (int j = 0; j < DH_FIR_L; j++) {
                bool s;
                (void) dh_div_gain_fast(acc[j], rgain, s);
                if (s) out16[j] = dh_div_gain_exact(acc[j], gain);
            }
        }
    }
}

#if DH_ON_GPU
// Window pairs come from LDS through inline asm: every sample is needed twice, 8 taps apart -- first as the high
// half of a pair, then as the low half of another.  Given ordinary loads the compiler keeps the first copy, pairs
// up adjacent addresses instead, and shuffles halves with ~2 v_mov per tap on the VALU, which is the bottleneck
// of this kernel; the LDS pipe is idle.  One ds_read2_b32 per tap delivers (x[t], x[t+8]) straight into an aligned
// register pair.  The loads run one batch of DH_FIR_G taps ahead of the arithmetic; the compiler does not track
// them, so each batch passes through an explicit `s_waitcnt lgkmcnt(0)` (robust against any other LDS / scalar
// memory operation the compiler may have in flight) before its first use.
#define DH_FIR_G 4
// pair i of the slide sequence: (x[8 + i], x[16 + i]), consumed when tap i has been accumulated
template <int NZ, int I> __device__ __forceinline__ void dh_fir_issue_one(uint32_t addr, dh_f2& d) {
    if constexpr (I < NZ) d = dh_lds_read2<DH_XLOFF(DH_FIR_H + I), DH_XLOFF(2 * DH_FIR_H + I)>(addr);
    else d = dh_f2_make(0.0f, 0.0f);
}
template <int NZ, int B> __device__ __forceinline__ void dh_fir_issue(uint32_t addr, dh_f2 (&d)[DH_FIR_G]) {
    dh_fir_issue_one<NZ, B * DH_FIR_G + 0>(addr, d[0]); dh_fir_issue_one<NZ, B * DH_FIR_G + 1>(addr, d[1]);
    dh_fir_issue_one<NZ, B * DH_FIR_G + 2>(addr, d[2]); dh_fir_issue_one<NZ, B * DH_FIR_G + 3>(addr, d[3]);
}
// The same batch, issued AND waited for inside one asm statement: nothing of the compiler's (a spill of a destination
// pair, say) can come between a load and its wait.  For the FIR bodies that are rare paths of a kernel at its register
// limit -- the reference-order FIR of the error-bounded chain kernels, which the compiler is told is cold and which it
// therefore spills around freely (tests/test_isa_contract.py caught a destination pair stored to scratch ahead of its wait).
template <int NZ, int B> __device__ __forceinline__ void dh_fir_issue_wait(uint32_t addr, dh_f2 (&d)[DH_FIR_G]) {
    if constexpr (B * DH_FIR_G < NZ) {
        static_assert(NZ % DH_FIR_G == 0, "a batch is all taps or all padding");
        asm volatile("ds_read2_b32 %0, %4 offset0:%5 offset1:%6\n\tds_read2_b32 %1, %4 offset0:%7 offset1:%8\n\t"
                     "ds_read2_b32 %2, %4 offset0:%9 offset1:%10\n\tds_read2_b32 %3, %4 offset0:%11 offset1:%12\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]) : "v"(addr),
                       "n"(DH_XLOFF(DH_FIR_H + B * DH_FIR_G + 0)), "n"(DH_XLOFF(2 * DH_FIR_H + B * DH_FIR_G + 0)),
                       "n"(DH_XLOFF(DH_FIR_H + B * DH_FIR_G + 1)), "n"(DH_XLOFF(2 * DH_FIR_H + B * DH_FIR_G + 1)),
                       "n"(DH_XLOFF(DH_FIR_H + B * DH_FIR_G + 2)), "n"(DH_XLOFF(2 * DH_FIR_H + B * DH_FIR_G + 2)),
                       "n"(DH_XLOFF(DH_FIR_H + B * DH_FIR_G + 3)), "n"(DH_XLOFF(2 * DH_FIR_H + B * DH_FIR_G + 3)) : "memory");
    } else {
        d[0] = dh_f2_make(0.0f, 0.0f); d[1] = d[0]; d[2] = d[0]; d[3] = d[0];
    }
}
__device__ __forceinline__ void dh_fir_arrived(dh_f2 (&d)[DH_FIR_G]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]) :: "memory");
}
// SG: the taps are read as 64-bit scalar pairs from the kernel arguments (dh_f2_mac_pair) instead of from a register
// array.  A packed multiply with a scalar operand issues a little slower (slicer kernels: +5 %), so this only pays
// where the 41 / 81 tap registers cost a wavefront per SIMD -- the stand-alone RRC kernel (168 -> 105 VGPRs).
// ZINIT = false: the accumulators start as the first product instead of 0 + product -- the same float except that a
// product of -0 stays -0 where the reference's `sum = 0; sum += c * x` gives +0.  The sign of a zero cannot reach a
// dibit (the slicer only adds, subtracts and compares filtered samples), so the slicer kernels drop the eight packed
// adds and the zeroing; the materialised RRC output (k_rrc_tile) keeps the reference's bits.
template <int NZ, bool FAST, int B, bool SG = false, bool ZINIT = true, bool SAFE = false> struct DhFirBatch {
    // tap I = B * DH_FIR_G + G: accumulate it on the eight window pairs, then slide the window by one sample
    template <int G> static __device__ __forceinline__ void tap(const float* taps, dh_f2 (&accp)[DH_FIR_H], dh_f2 (&w)[DH_FIR_H], dh_f2 (&cur)[DH_FIR_G]) {
        constexpr int I = B * DH_FIR_G + G;
        if constexpr (I <= NZ) {
            constexpr int TI = I <= NZ / 2 ? I : NZ - I;
            if constexpr (SG) {
                const dh_f2 cc = reinterpret_cast<const dh_f2*>(taps)[TI >> 1];     // wave-uniform 64-bit load
#pragma unroll
                for (int j = 0; j < DH_FIR_H; j++) accp[j] = dh_f2_mac_pair<FAST, TI & 1>(cc, w[j], accp[j]);
            } else if constexpr (I == 0 && !ZINIT) {
                const float c = taps[TI];
#pragma unroll
                for (int j = 0; j < DH_FIR_H; j++) accp[j] = c * w[j];              // v_pk_mul_f32
            } else {
                const float c = taps[TI];
#pragma unroll
                for (int j = 0; j < DH_FIR_H; j++) accp[j] = dh_f2_mac<FAST>(c, w[j], accp[j]);
            }
            if constexpr (I < NZ) {
#pragma unroll
                for (int j = 0; j < DH_FIR_H - 1; j++) w[j] = w[j + 1];
                w[DH_FIR_H - 1] = cur[G];
            }
        }
    }
    static __device__ __forceinline__ void run(const float* taps, uint32_t addr, dh_f2 (&accp)[DH_FIR_H], dh_f2 (&w)[DH_FIR_H], dh_f2 (&cur)[DH_FIR_G]) {
        if constexpr (B * DH_FIR_G <= NZ) {
            dh_f2 nxt[DH_FIR_G];
            if constexpr (SAFE) dh_fir_issue_wait<NZ, B + 1>(addr, nxt); else dh_fir_issue<NZ, B + 1>(addr, nxt);
            tap<0>(taps, accp, w, cur); tap<1>(taps, accp, w, cur); tap<2>(taps, accp, w, cur); tap<3>(taps, accp, w, cur);
            static_assert(DH_FIR_G == 4, "four taps per batch");
            if constexpr (!SAFE && (B + 1) * DH_FIR_G < NZ) dh_fir_arrived(nxt);
            DhFirBatch<NZ, FAST, B + 1, SG, ZINIT, SAFE>::run(taps, addr, accp, w, nxt);
        }
    }
};

template <int NZ, bool FAST, bool SG = false, bool SAFE = false>
__device__ __forceinline__ void dh_fir_lane(const float* taps, double gain, double rgain, float inv_gain, const float* xs_all, int lane, float* out16, bool* nonfinite = nullptr) {
    constexpr bool ZINIT = SG;                             // the stand-alone RRC kernel (scalar taps) materialises its output
    // element e of this lane's window sits at DH_XPAD(16*lane + e) = 17*lane + e + (e >> 4): static offsets from one base
    const uint32_t addr = (uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) (xs_all + (DH_FIR_L + 1) * lane);
    dh_f2 accp[DH_FIR_H], w[DH_FIR_H], cur[DH_FIR_G];
    if constexpr (SAFE) {
        // (the first eight window pairs as two batches of the slide sequence shifted by -8: pair i = (x[i], x[8 + i]))
        asm volatile("ds_read2_b32 %0, %8 offset0:%9 offset1:%10\n\tds_read2_b32 %1, %8 offset0:%11 offset1:%12\n\t"
                     "ds_read2_b32 %2, %8 offset0:%13 offset1:%14\n\tds_read2_b32 %3, %8 offset0:%15 offset1:%16\n\t"
                     "ds_read2_b32 %4, %8 offset0:%17 offset1:%18\n\tds_read2_b32 %5, %8 offset0:%19 offset1:%20\n\t"
                     "ds_read2_b32 %6, %8 offset0:%21 offset1:%22\n\tds_read2_b32 %7, %8 offset0:%23 offset1:%24\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7]) : "v"(addr),
                       "n"(DH_XLOFF(0)), "n"(DH_XLOFF(8)), "n"(DH_XLOFF(1)), "n"(DH_XLOFF(9)), "n"(DH_XLOFF(2)), "n"(DH_XLOFF(10)), "n"(DH_XLOFF(3)), "n"(DH_XLOFF(11)),
                       "n"(DH_XLOFF(4)), "n"(DH_XLOFF(12)), "n"(DH_XLOFF(5)), "n"(DH_XLOFF(13)), "n"(DH_XLOFF(6)), "n"(DH_XLOFF(14)), "n"(DH_XLOFF(7)), "n"(DH_XLOFF(15)) : "memory");
        dh_fir_issue_wait<NZ, 0>(addr, cur);
    } else {
    w[0] = dh_lds_read2<DH_XLOFF(0), DH_XLOFF(8)>(addr);  w[1] = dh_lds_read2<DH_XLOFF(1), DH_XLOFF(9)>(addr);
    w[2] = dh_lds_read2<DH_XLOFF(2), DH_XLOFF(10)>(addr); w[3] = dh_lds_read2<DH_XLOFF(3), DH_XLOFF(11)>(addr);
    w[4] = dh_lds_read2<DH_XLOFF(4), DH_XLOFF(12)>(addr); w[5] = dh_lds_read2<DH_XLOFF(5), DH_XLOFF(13)>(addr);
    w[6] = dh_lds_read2<DH_XLOFF(6), DH_XLOFF(14)>(addr); w[7] = dh_lds_read2<DH_XLOFF(7), DH_XLOFF(15)>(addr);
    dh_fir_issue<NZ, 0>(addr, cur);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]) :: "memory");
    dh_fir_arrived(cur);
    }
    if constexpr (ZINIT) {
#pragma unroll
        for (int j = 0; j < DH_FIR_H; j++) accp[j] = dh_f2_make(0.0f, 0.0f);
    }
    DhFirBatch<NZ, FAST, 0, SG, ZINIT, SAFE>::run(taps, addr, accp, w, cur);
    float acc[DH_FIR_L];
#pragma unroll
    for (int j = 0; j < DH_FIR_H; j++) { acc[j] = accp[j].x; acc[j + DH_FIR_H] = accp[j].y; }
    if (FAST && nonfinite) {                               // 0 * acc is NaN for a NaN or infinite accumulator: eight packed FMAs
        dh_f2 t = dh_f2_make(0.0f, 0.0f);
        const dh_f2 zero = dh_f2_make(0.0f, 0.0f);
#pragma unroll
        for (int j = 0; j < DH_FIR_H; j++) t = __builtin_elementwise_fma(accp[j], zero, t);
        *nonfinite = !(t.x + t.y == 0.0f);
        dh_fir_finish<FAST>(acc, gain, rgain, inv_gain, out16, nullptr);
    } else dh_fir_finish<FAST>(acc, gain, rgain, inv_gain, out16, nonfinite);
}
#else
template <int NZ, bool FAST, bool SG = false, bool SAFE = false>         // (SG, SAFE: how the device form gets and waits for its operands)
inline void dh_fir_lane(const float* taps, double gain, double rgain, float inv_gain, const float* xs_all, int lane, float* out16, bool* nonfinite = nullptr) {
    const float* xs = xs_all + (DH_FIR_L + 1) * lane;
#define DH_XL(e) xs[DH_XLOFF(e)]
    dh_f2 accp[DH_FIR_H], w[DH_FIR_H];
    for (int j = 0; j < DH_FIR_H; j++) {
        accp[j] = dh_f2_make(0.0f, 0.0f);
        w[j] = dh_f2_make(DH_XL(j), DH_XL(j + DH_FIR_H));
    }
    for (int i = 0; i <= NZ; i++) {
        const float c = taps[i <= NZ / 2 ? i : NZ - i];
        for (int j = 0; j < DH_FIR_H; j++) accp[j] = dh_f2_mac<FAST>(c, w[j], accp[j]);
        if (i < NZ) {
            for (int j = 0; j < DH_FIR_H - 1; j++) w[j] = w[j + 1];
            w[DH_FIR_H - 1] = dh_f2_make(DH_XL(DH_FIR_H + i), DH_XL(2 * DH_FIR_H + i));
        }
    }
    float acc[DH_FIR_L];
    for (int j = 0; j < DH_FIR_H; j++) { acc[j] = accp[j].x; acc[j + DH_FIR_H] = accp[j].y; }
    dh_fir_finish<FAST>(acc, gain, rgain, inv_gain, out16, nonfinite);
}
#endif

// ---------------------------------------------------------------------------------------------
// The fused FIR on the matrix pipe (error-bounded and FAST wide-filter kernels): v_mfma_f32_16x16x4_f32 is bit for bit a
// k-ordered chain of f32 FMAs, at the same FLOP rate as v_pk_fma_f32 -- but it issues beside the VALU, which the rest
// of the slicer keeps busy, and takes one register per operand instead of a ds_read2 per packed FMA.
//
// Toeplitz form.  The 1024 outputs of a pass are 64 blocks of 16: y[16 b + n] = sum_p x[16 b + p] c[p - n], p = 0..NZ+15,
// with c = 0 outside 0..NZ.  One MFMA tile takes 16 blocks as its rows (A operand: the raw samples) and the 16 samples of
// a block as its columns (B operand: the taps, the same for every block and tile); K runs over p in (NZ + 16) / 4 slices
// of 4.  Multiplying by an exact zero changes nothing, so each output is the (NZ + 1)-term fused chain in tap order --
// the value the VALU form (dh_fir_lane<NZ, true>) produces, and the one the bound of "Error-bounded FIR" is proven for
// (a non-finite sample under a zero tap turns into a NaN, which is exactly what sends the run to the reference's
// arithmetic anyway).
//   A: lane (m = l & 15, q = l >> 4) holds x[16 b(m) + 4 s + q];   B: lane (n = l & 15, q = l >> 4) holds c[4 s + q - n]
//   D: lane (n = l & 15, g = l >> 4), register r holds y[16 b(4 g + r) + n]
// Blocks of tile T: b(m) = 2 m + (T & 1) + 32 (T >> 1).  In the padded window (one word per 16) block b starts at word
// 17 b, so the sixteen rows of a tile are 34 words apart: with the q = 0 / 1 (2 / 3) lanes of a ds_read_b32's lane group
// one word apart that is 32 different banks.  Tiles T and T + 1 interleave their blocks, so slice s of the odd tile IS
// slice s + 4 of the even one: 28 window reads serve the 48 MFMAs of a tile pair.  Results go back unpadded (sample o at
// word o): sixteen ds_write_b32 at compile-time offsets from one per-lane base (2-way bank conflicts, which a 4-byte
// store hides behind its own issue time).
#define DH_MF_OUT(T, r, g, n) (128u * (uint32_t) (g) + (uint32_t) (n) + 32u * (uint32_t) (r) + 16u * ((uint32_t) (T) & 1u) + 512u * ((uint32_t) (T) >> 1))
#if DH_ON_GPU
// acc[4 T + r] of lane (n, g) = sum over the chain for output DH_MF_OUT(T, r, g, n); `tapsf` points at tap 0 of the
// zero-framed table, `xs` at the padded window
template <int NZ>
__device__ __forceinline__ void dh_fir_mfma(const float* tapsf, const float* xs, int lane, float* acc16) {
    static_assert((NZ + 16) % 4 == 0 && NZ <= 80, "K = NZ + 16 in slices of four; the zero-framed tap table exists for the wide filter");
    constexpr int NS = (NZ + 16) / 4;
    const int m = lane & 15, q = lane >> 4;
    const float* xb = xs + 34 * m + q;
    const float* tb = tapsf + (q - m);
    float tap[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) tap[s] = tb[4 * s];
    dh_f32x4 a0 = { 0.0f, 0.0f, 0.0f, 0.0f }, a1 = a0, a2 = a0, a3 = a0;
#pragma unroll
    for (int s = 0; s < NS + 4; s++) {
        const int off = 4 * s + (s >> 2);
        const float x01 = xb[off], x23 = xb[544 + off];
        if (s < NS) { a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x01, tap[s], a0, 0, 0, 0); a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(x23, tap[s], a2, 0, 0, 0); }
        if (s >= 4) { a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x01, tap[s - 4], a1, 0, 0, 0); a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(x23, tap[s - 4], a3, 0, 0, 0); }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) { acc16[r] = a0[r]; acc16[4 + r] = a1[r]; acc16[8 + r] = a2[r]; acc16[12 + r] = a3[r]; }
}
#else
template <int NZ>
inline void dh_fir_mfma(const float* tapsf, const float* xs, int lane, float* acc16) {
    const int n = lane & 15, g = lane >> 4;
    for (int T = 0; T < 4; T++) for (int r = 0; r < 4; r++) {
        const uint32_t o = DH_MF_OUT(T, r, g, n), b16 = o - (uint32_t) n;
        float acc = 0.0f;
        for (int p = 0; p < NZ + 16; p++) acc = __builtin_fmaf(xs[DH_XPAD(b16 + (uint32_t) p)], tapsf[p - n], acc);
        acc16[4 * T + r] = acc;
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// The fused FIR as a SPLIT-f16 product on the matrix cores (the error-bounded kernels).
//
// f32 arithmetic -- v_pk_fma_f32 and v_mfma_f32_16x16x4_f32 alike -- runs at 64 flop / clock / SIMD, and an f32 MFMA keeps
// the vector ALU as busy as the packed FMAs it replaces (tools/microbench/mfma_valu_overlap.hip: MFMA wave + VALU wave on one
// SIMD take the SUM of their times): 81 taps x 1024 outputs are 2 600 SIMD cycles per run whichever instruction does them.
// v_mfma_f32_16x16x32_f16 does 16 times the work per cycle.  The error-bounded scheme does not need the reference's floats,
// only values with a KNOWN distance from them, so the filter runs there:
//   samples   x_s = x 2^-k  (k from the run's max |x|, which staging computes anyway: max |x_s| in [0.5, 1))
//             h1 = f16(x_s), h2 = f16((x_s - h1) 2^11):   x_s = h1 + 2^-11 h2 + eps,  |eps| <= 2^-24   (both conversions round to
//             nearest; x_s - h1 is exact in f32; f16 subnormals are honoured by the MFMA -- tools/microbench/mfma_f16_numerics.hip)
//   taps      c = g1 + 2^-11 g2 + delta, g1 = f16(c), g2 = f16((c - g1) 2^11)   (host, once per engine; delta known exactly)
//   products  M = sum g1 h1  (3 MFMAs of K = 32 per tile of 256 outputs),  R = sum (g2 h1 + g1 h2)  (6 MFMAs),
//             y = (M + 2^-11 R) / (gain 2^-k)  as  fma(R, k2, M k1);   the g2 h2 products (2^-22) are dropped
//   ONE CHAIN (dh_f16_one_chain: the wide filter's kernels that do not hand out their floats).  The two scales are a convention,
//             and the two accumulators, the 2^11 of h2 and the fma they cost buy nothing: there the main sum's tap fragments
//             hold g1' = 2^11 g1 (exact in f16 for the table: the host checks it), staging stores h2' = f16(x_s - h1) as it
//             stands (dh_f16_split4_plain: the same |eps| <= 2^-24), and all nine MFMAs of a tile add into ONE accumulator on the
//             2^11 scale, smallest first:  A = sum g2 h1 (3), + sum g1' h1 (3), + sum g1' h2' (3);  y = A kc,  kc = k1 2^-11 (exact).
//             One multiplication per output, one accumulator quad per tile.  The price is in the radius: the six MFMAs that
//             follow the small ones run at the main sum's magnitude, where the two-chain form had three (below).
// f16 x f16 products are exact in f32; what the hardware does to their sum is not documented, so the bound rests on a
// stated assumption, checked on the device by tests/test_numerics.py (known-answer probes + 10^6 random dot products):
//   (H1) inside one MFMA every addend (32 products and C) enters the sum with an alignment error below 2^-24 mu, and each
//        of its four passes rounds with a relative error <= 2^-23, where mu bounds every addend and partial sum:
//        |D - (C + sum a b)| <= 41 u mu,  u = 2^-24.  (Observed on gfx950: products are truncated to 2^-24 of the largest
//        product of their group of eight, groups are added in order with a final round to nearest; worst case over 10^6
//        random sums 3.5 u (|C| + sum |a b|) -- a tenth of what (H1) allows.)
// dh_f16_error_coefficient() adds it all up (reference chain gamma_82 + its division; 123 u for the three chained MFMAs of
// M; the split residuals; the dropped products; the two roundings of the combine -- in the one-chain form 246 u for the six
// MFMAs at full magnitude and one rounding of the combine) and keeps the 1.44 of head room for the
// slicer's own roundings that the f32 bound has.  Toeplitz layout as in dh_fir_mfma, natural block order:
//   A: lane (m = l & 15, q = l >> 4) holds h[16 (16 T + b(m)) + 32 s + 8 q + j], j = 0..7 -- ONE ds_read_b128 from the plain f16
//      window (32 bytes per row, 16 per q: conflict-free in every lane group of a b128 read); b(m) = DH_F16_ROW_BLOCK(m), a
//      permutation of the tile's sixteen blocks inside each half of the rows (see DH_F16_OUT)
//   B: lane (n = l & 15, q = l >> 4) holds g[32 s + 8 q + j - n]: per-lane fragments precomputed on the host (6 x 1 KiB,
//      dh_f16_tap_fragments), fetched with the samples
//   D: lane (n, g), register r holds y[256 T + 16 b(4 g + r) + n] = y[DH_F16_OUT(T, r, g, n)]
#define DH_EXACT_BATCH 2                     // exact evaluations of the 81-tap kernels: this many products at a time, their LDS reads in flight together (the 161-tap ones: 8)
// K = taps + 15 rounded up to whole MFMAs of 32: three for the wide filter (96), six for the narrow one (192; taps beyond the
// response are zeros in the fragments, and the halves beyond the window are stored as zeros)
#define DH_F16_KSTEPS_OF(nz) (((nz) + 16 + 31) / 32)
#define DH_F16_MAX_KSTEPS DH_F16_KSTEPS_OF(DH_MAX_NZ)
#define DH_F16_HALVES_OF(nz) (1008 + 32 * DH_F16_KSTEPS_OF(nz))     // halves per array: the last block (63) reads up to here
#define DH_F16_H2_OFFSET_OF(nz) (DH_F16_HALVES_OF(nz) / 2)           // word offset of the h2 array inside the window block
// Row m = 4 g + r of a tile (the block of sixteen outputs an A row produces) is block 2 r + (g & 1) + 8 (g >> 1) of the tile, not block m:
// register r of the lanes of ONE store pass (32 lanes: g = 0, 1 or g = 2, 3) then covers 32 consecutive words -- in natural order the
// two groups of a pass were 64 words apart and every result store ran into a two-way bank conflict.
#define DH_F16_ROW_BLOCK(m) (2u * ((uint32_t) (m) & 3u) + (((uint32_t) (m) >> 2) & 1u) + 8u * ((uint32_t) (m) >> 3))
#define DH_F16_OUT(T, r, g, n) (256u * (uint32_t) (T) + 128u * ((uint32_t) (g) >> 1) + 32u * (uint32_t) (r) + 16u * ((uint32_t) (g) & 1u) + (uint32_t) (n))

// Which kernels filter in the one-chain form (above): the wide filter's, unless they also deliver their filtered samples
// (`keepf`: KEEPF of dh_rrc_demod_channel, fused_keep of an engine -- that path promises 2.5e-6 on its floats and keeps the form
// it was measured with).  An engine launches either the KEEPF slicer or the others, so the host builds the fragments and
// the coefficient ONCE, by the predicate the kernel is compiled with.
constexpr bool dh_f16_one_chain(uint32_t nz, int keepf) { return nz == 80 && !keepf; }

// the split of a tap and the per-lane B operands (host, once per engine): frag[f][lane][d], f = 0..2 the g1 slices (one chain:
// of g1' = 2^11 g1), 3..5 the g2 slices
struct DhF16Taps {
    uint32_t frag[2 * DH_F16_MAX_KSTEPS][DH_WAVE][4];        // the first 2 * DH_F16_KSTEPS_OF(nz) are used
    uint32_t ksteps;
    bool one_chain;
    double l1, l1_g1, l1_g2, sum_delta;                      // (l1_g1: of g1 itself in either form)
};
// false: a one-chain table whose 2^11 g1 is not a finite half equal to it (neither built-in table; nothing is usable then)
inline bool dh_f16_tap_fragments(const float* taps_half, uint32_t nz, bool one_chain, DhF16Taps& F) {
    uint16_t g1[DH_MAX_NZ + 1], g2[DH_MAX_NZ + 1];
    F.l1 = F.l1_g1 = F.l1_g2 = F.sum_delta = 0.0;
    F.one_chain = one_chain;
    bool ok = true;
    for (uint32_t i = 0; i <= nz; i++) {
        const float c = taps_half[i <= nz / 2 ? i : nz - i];
        g1[i] = dh_f16_bits(c);
        const double r = (double) c - (double) dh_f16_value(g1[i]);
        g2[i] = dh_f16_bits((float) (r * 2048.0));                                     // (r has at most 13 significant bits: exact)
        const double v2 = (double) dh_f16_value(g2[i]);
        const double delta = r - v2 / 2048.0;
        F.l1 += c < 0 ? -(double) c : (double) c; F.l1_g1 += __builtin_fabs((double) dh_f16_value(g1[i]));
        F.l1_g2 += __builtin_fabs(v2); F.sum_delta += __builtin_fabs(delta);
        if (one_chain) {                                                               // g1 becomes g1' = 2^11 g1
            const float v1 = dh_f16_value(g1[i]);
            g1[i] = dh_f16_bits(v1 * 2048.0f);
            const float s1 = dh_f16_value(g1[i]);
            if (!(s1 == v1 * 2048.0f) || (g1[i] & 0x7C00u) == 0x7C00u) ok = false;     // exact and finite (the product itself is exact in f32)
        }
    }
    const int KS = (int) DH_F16_KSTEPS_OF(nz);
    F.ksteps = (uint32_t) KS;
    for (int f = 0; f < 2 * KS; f++) for (int lane = 0; lane < DH_WAVE; lane++) for (int d = 0; d < 4; d++) {
        const int n = lane & 15, q = lane >> 4, s = f % KS;
        uint32_t w = 0;
        for (int hh = 0; hh < 2; hh++) {
            const int t = 32 * s + 8 * q + 2 * d + hh - n;
            const uint16_t v = (t >= 0 && t <= (int) nz) ? (f < KS ? g1[t] : g2[t]) : 0;
            w |= (uint32_t) v << (16 * hh);
        }
        F.frag[f][lane][d] = w;
    }
    return ok;
}
// error radius of a filtered sample per unit of max |x| for this path (see above; everything in units of u / gain):
//   reference: (taps + 1) (gamma, + second order) L1 + 1.0001 L1 (its division and rounding): 82 for the wide filter
//   main sum:  41 KS L1(g1) (1 + 2^-11) ((H1), KS chained MFMAs -- 123 for the wide filter; |h1| <= max |x_s| (1 + 2^-11))
//   second sum: 2^-11 82 KS (L1(g2) + L1(g1) / 2)
//   residuals (absolute in the scaled domain, where max |x_s| >= 1/2: twice as much per unit of max |x|):
//              2 (2^-22 L1(g2) / 2 + sum |delta| (1 + 2^-12) + u L1) / u
//   combine:   3.1 L1 (fl32(1 / gain), the multiply, the fma)
// times 1.44 for the slicer's own roundings, as in dh_fir_error_coefficient.
// One chain (everything divided by the 2^11 the accumulator carries; mu of (H1) is what the accumulator can hold BY THEN):
//   MFMAs 1..KS, g2 h1:        mu = L1(g2) (1 + 2^-11)                                    -> 2^-11 41 KS L1(g2) (1 + 2^-11)
//   MFMAs KS+1..2KS, g1' h1:   mu = (2^11 L1(g1) + L1(g2)) (1 + 2^-11)                    -> 41 KS (L1(g1) + 2^-11 L1(g2)) (1 + 2^-11)
//   MFMAs 2KS+1..3KS, g1' h2': the same + 2^11 L1(g1) 2^-12, per unit of max |x_s| >= 1/2 at most 2^-11 of the main sum more
//                                                                                         -> the same + 2^-11 41 KS L1(g1)
//   together  82 KS L1(g1) (1 + 2^-11)  [246 for the wide filter, where the two chains had 123]
//           + 2^-11 41 KS (3 L1(g2) (1 + 2^-11) + L1(g1))
//   residuals: as above (h2' is within 2^-24 of x_s - h1 like 2^-11 h2; the dropped g2 h2' products are the same numbers)
//   combine:   2.1 L1 (fl32(1 / gain) and ONE multiplication; kc = k1 2^-11 is exact)
// Any other order -- the main sums between the small ones -- puts up to eight MFMAs at full magnitude.
inline float dh_f16_error_coefficient(const DhF16Taps& F, uint32_t nz, double gain) {
    const double u = 5.9604644775390625e-08;
    const double ks = (double) F.ksteps, nref = 2.0 + (double) nz;                     // gamma_(taps + 1) for the reference's chain
    const double mfma = F.one_chain ? 82.0 * ks * F.l1_g1 * (1.0 + 1.0 / 2048.0) + 41.0 * ks / 2048.0 * (3.0 * F.l1_g2 * (1.0 + 1.0 / 2048.0) + F.l1_g1)
                                    : 41.0 * ks * F.l1_g1 * (1.0 + 1.0 / 2048.0) + 82.0 * ks / 2048.0 * (F.l1_g2 + 0.5 * F.l1_g1);
    const double kl1 = (nref + 0.01) * F.l1 + 1.0001 * F.l1 + mfma
                     + 2.0 * (0.5 * F.l1_g2 / 4194304.0 + F.sum_delta * (1.0 + 1.0 / 4096.0) + u * F.l1) / u + (F.one_chain ? 2.1 : 3.1) * F.l1;
    const double coef = 1.44 * kl1 * u / (gain < 0 ? -gain : gain) * 1.0001;
    float f = (float) coef;
    if ((double) f < coef) { union { float f; uint32_t u; } b; b.f = f; b.u++; f = b.f; }
    return f;
}

#if DH_ON_GPU
// acc16[4 T + r] of lane (n, g) = y-before-gain of output DH_F16_OUT(T, r, g, n) in the scaled domain: main + 2^-11 second sum
// is formed by the caller's fma (k1, k2).  `hw` = the window block (h1 at byte 0, h2 at DH_F16_H2_OFFSET words), G = the six
// tap fragments of this lane.  ONE: the one-chain form -- G[0..2] hold g1', the h2 array holds h2', k1 is kc and k2 is not used.
template <int NZ, bool ONE>
__device__ __forceinline__ void dh_fir_f16(const float* hw, const dh_u4 (&G)[2 * DH_F16_KSTEPS_OF(NZ)], int lane, float k1, float k2, float* out16) {
    constexpr int DH_F16_KSTEPS = DH_F16_KSTEPS_OF(NZ), DH_F16_FRAGS = 2 * DH_F16_KSTEPS, DH_F16_H2_OFFSET = DH_F16_H2_OFFSET_OF(NZ);
    const int m = lane & 15, q = lane >> 4;
    const char* base = reinterpret_cast<const char*>(hw) + 32 * (int) DH_F16_ROW_BLOCK(m) + 16 * q;
    dh_h8 g[DH_F16_FRAGS];
#pragma unroll
    for (int f = 0; f < DH_F16_FRAGS; f++) g[f] = __builtin_bit_cast(dh_h8, G[f]);
    // Two tiles at a time, so that four accumulation chains (main and second sum of each) alternate and no MFMA waits for
    // the one before it.  Only six 16-byte fragments of the window are live at once: the h2 fragment of a K step is read
    // into the registers of the h1 fragment the step has just finished with, two steps before it is needed.
#pragma unroll
    for (int TT = 0; TT < 4; TT += 2) {
        dh_h8 a1[2][DH_F16_KSTEPS], a2[2][DH_F16_KSTEPS];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++) a1[t][s] = *reinterpret_cast<const dh_h8*>(base + 512 * (TT + t) + 64 * s);
        if constexpr (ONE) {
            // one accumulator per tile, two tiles alternating; the order is the one the radius was derived for (dh_f16_error_coefficient):
            // the small sum first, then the two at the main sum's magnitude
            dh_f32x4 acc[2] = { { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } };
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++)
#pragma unroll
                for (int t = 0; t < 2; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[t][s], g[DH_F16_KSTEPS + s], acc[t], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++) {
#pragma unroll
                for (int t = 0; t < 2; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[t][s], g[s], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 2; t++) a2[t][s] = *reinterpret_cast<const dh_h8*>(base + 512 * (TT + t) + 64 * s + 4 * DH_F16_H2_OFFSET);
            }
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++)
#pragma unroll
                for (int t = 0; t < 2; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[t][s], g[s], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) out16[4 * (TT + t) + r] = acc[t][r] * k1;
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * DH_F16_KSTEPS, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * DH_F16_KSTEPS, 0);
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++) { __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 2, 0); }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * DH_F16_KSTEPS, 0);
            (void) k2;
        } else {
            dh_f32x4 mn[2] = { { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } }, sc[2] = { { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } };
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++) {
#pragma unroll
                for (int t = 0; t < 2; t++) sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[t][s], g[DH_F16_KSTEPS + s], sc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 2; t++) mn[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[t][s], g[s], mn[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 2; t++) a2[t][s] = *reinterpret_cast<const dh_h8*>(base + 512 * (TT + t) + 64 * s + 4 * DH_F16_H2_OFFSET);
            }
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++)
#pragma unroll
                for (int t = 0; t < 2; t++) sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[t][s], g[s], sc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) out16[4 * (TT + t) + r] = __builtin_fmaf(sc[t][r], k2, mn[t][r] * k1);
            // scheduling groups (DS read = 0x100, MFMA = 0x008): the order written above
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * DH_F16_KSTEPS, 0);
#pragma unroll
            for (int s = 0; s < DH_F16_KSTEPS; s++) { __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); __builtin_amdgcn_sched_group_barrier(0x100, 2, 0); }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * DH_F16_KSTEPS, 0);
        }
    }
}
#else
// harness: the same split and the same sums as plain f32 chains (products of halves are exact in f32; a sequential chain of
// 96 rounded additions stays inside what (H1) allows the hardware, so the decisions downstream are the same)
// (ONE: one chain in the device's order -- the taps' second halves, the main sum, the samples' second halves; 288 rounded additions
// at the magnitudes the nine MFMAs see are inside the 369 u (H1) allows those)
template <int NZ, bool ONE>
inline void dh_fir_f16(const float* hw, const uint32_t (*G)[DH_WAVE][4], int lane, float k1, float k2, float* out16) {
    constexpr int DH_F16_KSTEPS = DH_F16_KSTEPS_OF(NZ), DH_F16_H2_OFFSET = DH_F16_H2_OFFSET_OF(NZ);
    const uint16_t* h1 = reinterpret_cast<const uint16_t*>(hw);
    const uint16_t* h2 = reinterpret_cast<const uint16_t*>(hw + DH_F16_H2_OFFSET);
    const int n = lane & 15, g = lane >> 4;
    for (int T = 0; T < 4; T++) for (int r = 0; r < 4; r++) {
        const uint32_t o = DH_F16_OUT(T, r, g, n), b16 = o - (uint32_t) n;
        float mn = 0.0f, sc = 0.0f;
        for (int i = 0; i < 3; i++) {                              // two chains: main (0); taps' second halves (1); samples' second halves (2).  ONE: 1, 0, 2 -- the device's order either way
            const int pass = ONE ? (i == 0 ? 1 : i == 1 ? 0 : 2) : i;
            for (int s = 0; s < DH_F16_KSTEPS; s++) for (int qq = 0; qq < 4; qq++) for (int j = 0; j < 8; j++) {
                const int kk = 8 * qq + j;                         // B fragment of lane (n, qq): element j
                const uint32_t w = G[(pass == 1 ? DH_F16_KSTEPS : 0) + s][16 * qq + n][j >> 1];
                const float tap = dh_f16_value((uint16_t) (w >> (16 * (j & 1))));
                const uint16_t hv = (pass == 2 ? h2 : h1)[b16 + 32u * (uint32_t) s + (uint32_t) kk];
                if (pass == 0 && !ONE) mn = __builtin_fmaf(dh_f16_value(hv), tap, mn); else sc = __builtin_fmaf(dh_f16_value(hv), tap, sc);
            }
        }
        out16[4 * T + r] = ONE ? sc * k1 : __builtin_fmaf(sc, k2, mn * k1);
    }
}
#endif

// virtual input stream of a channel for this push: carried tail followed by the new samples
DH_HD float dh_virtual_sample(const float* tail, uint32_t tc, const float* in, uint32_t idx) {
    return idx < tc ? tail[idx] : in[idx - tc];
}

// ---------------------------------------------------------------------------------------------
// AGC window extremes for the symbols k0..k1-1 of the current block (calibrateAudio,
// gfsk_demodulator.cpp:109-116): S.mn[k] / S.mx[k] = min / max over the volume ring as it stands
// right after symbol k was written.  The reference seeds min with FLT_MAX and max with FLT_MIN
// (sic: the smallest positive float), which are exactly the identities used for padding here.
// `agc`: the extremes of ring slots 2 l and 2 l + 1 once more, as a per-lane value -- what the scan hands to the slicing phase in
// registers.  Defined for the slots k0 .. k1 - 1 (the others: some value of the block, never looked at).
struct DhAgcPair { float mn0, mx0, mn1, mx1; };
// What the sps-10 window phase hands on in registers: the volumes (`from_win`: the scan's sources for ring slots 2 l, 2 l + 1 of a
// run that opens its block, k0 = 0 -- S.vol_new then holds the same values, for the runs and paths that look there) and the
// mid-symbol sums of the lane's symbols 2 l and 2 l + 1 of the run.
struct DhWinPair { float vol0, vol1, sum0, sum1, old0, old1; };

#if DH_ON_GPU
// lane l owns ring slots 2l and 2l+1 for the prefix part; the suffix part is the same scan over the ring read
// backwards (lane l takes slots 126-2l and 127-2l), handed back to the owning lanes -- lane 63 - l -- by four ds_bpermute
// (until round 5 through S.mn / S.mx: four stores, a barrier, four loads, a barrier -- one LDS round trip more).  The lane's
// results (slots 2l and 2l+1) also stay in registers: the slicing phase of a run that starts its block takes them from there.
template <bool PAIRS>                                   // PAIRS: behind the sps-10 window phase (DhWinPair; `from_win` only there)
__device__ __forceinline__ void dh_agc_scan(DhDspShared& S, uint32_t k0, uint32_t k1, DH_LANE_STRUCT_REF(DhAgcPair, agc), DH_LANE_STRUCT_IN(DhWinPair, win), bool from_win) {
    const int lane = dh_fresh_lane_id_();
    const uint32_t e0 = 2u * (uint32_t) lane, e1 = e0 + 1u;
    // prefix source: old below k0, new in [k0, k1), identity above
    float c0, c1;
    if (!PAIRS) { c0 = e0 < k0 ? S.vol_old[e0] : S.vol_new[e0]; c1 = e1 < k0 ? S.vol_old[e1] : S.vol_new[e1]; }
    else if (DH_LIKELY(from_win)) { c0 = win.vol0; c1 = win.vol1; }              // (wave-uniform; k0 = 0: nothing of the window phase's is loaded back)
    else {
        // (reads the compiler does not track, settled here: a tracked load's wait would be placed where the two paths join, and on
        // the usual one it drains the window phase's stores in front of the scan)
        c0 = dh_lds_read_b32<0>(dh_lds_addr((e0 < k0 ? S.vol_old : S.vol_new) + e0));
        c1 = dh_lds_read_b32<0>(dh_lds_addr((e1 < k0 ? S.vol_old : S.vol_new) + e1));
        dh_lds_reads_done(c0, c1);
    }
    const bool v0 = e0 < k1, v1 = e1 < k1;
    const float pmn0 = v0 ? c0 : DH_FLT_MAX, pmn1 = v1 ? c1 : DH_FLT_MAX;
    const float pmx0 = v0 ? c0 : DH_FLT_MIN, pmx1 = v1 ? c1 : DH_FLT_MIN;
    float pmn = dh_vmin(pmn0, pmn1), pmx = dh_vmax(pmx0, pmx1);
    // suffix source: the old ring backwards (slots >= 100 hold the identity)
    const uint32_t r0 = 126u - e0, r1 = r0 + 1u;
    float o0, o1;
    if (!PAIRS) { o0 = S.vol_old[r0]; o1 = S.vol_old[r1]; }
    else if (DH_LIKELY(from_win)) { o0 = win.old0; o1 = win.old1; }
    else { o0 = dh_lds_read_b32<0>(dh_lds_addr(S.vol_old + r0)); o1 = dh_lds_read_b32<0>(dh_lds_addr(S.vol_old + r1)); dh_lds_reads_done(o0, o1); }
    const float omn0 = r0 < DH_VOLUME_RB_SIZE ? o0 : DH_FLT_MAX, omn1 = r1 < DH_VOLUME_RB_SIZE ? o1 : DH_FLT_MAX;
    const float omx0 = r0 < DH_VOLUME_RB_SIZE ? o0 : DH_FLT_MIN, omx1 = r1 < DH_VOLUME_RB_SIZE ? o1 : DH_FLT_MIN;
    float smn = dh_vmin(omn0, omn1), smx = dh_vmax(omx0, omx1);
    dh_wave_prefix_minmax2(pmn, pmx, smn, smx);
    // exclusive parts: everything before this lane's pair (prefix), everything after slot r1 (suffix)
    float epmn = DH_FLT_MAX, epmx = DH_FLT_MIN, esmn = DH_FLT_MAX, esmx = DH_FLT_MIN;
    dh_wave_prev4(epmn, epmx, esmn, esmx, pmn, pmx, smn, smx);
    // suffix (exclusive of the slot itself) for slots r1 (esmn / esmx) and r0; slot e of lane l is slot r of lane 63 - l
    const int from = (63 - lane) << 2;
    const float s1n = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(esmn)));
    const float s1x = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(esmx)));
    const float s0n = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(dh_vmin(omn1, esmn))));
    const float s0x = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(dh_vmax(omx1, esmx))));
    // slot e0: prefix through e0 = before this lane + own e0; slot e1: inclusive prefix of the lane
    DhAgcPair r;
    r.mn0 = dh_vmin(dh_vmin(epmn, pmn0), s0n); r.mx0 = dh_vmax(dh_vmax(epmx, pmx0), s0x);
    r.mn1 = dh_vmin(pmn, s1n); r.mx1 = dh_vmax(pmx, s1x);
    S.mn[e0] = r.mn0; S.mx[e0] = r.mx0; S.mn[e1] = r.mn1; S.mx[e1] = r.mx1;
    agc = r;
}
#else
template <bool PAIRS>
inline void dh_agc_scan(DhDspShared& S, uint32_t k0, uint32_t k1, DH_LANE_STRUCT_REF(DhAgcPair, agc), DH_LANE_STRUCT_IN(DhWinPair, win), bool from_win) {
    // plain sequential statement of the same thing (harness only)
    float pmn = DH_FLT_MAX, pmx = DH_FLT_MIN;
    for (uint32_t j = 0; j < k0; j++) { pmn = dh_fmin_(pmn, S.vol_old[j]); pmx = dh_fmax_(pmx, S.vol_old[j]); }
    for (uint32_t k = k0; k < k1; k++) {
        const float vk = !from_win ? S.vol_new[k] : (k & 1u) ? win[k >> 1].vol1 : win[k >> 1].vol0;      // (from_win: k0 = 0, slot k is symbol k of lane k / 2)
        pmn = dh_fmin_(pmn, vk); pmx = dh_fmax_(pmx, vk);
        float smn = DH_FLT_MAX, smx = DH_FLT_MIN;
        for (uint32_t j = k + 1; j < DH_VOLUME_RB_SIZE; j++) {
            // (from_win: the old ring too as the window phase handed it on -- slot j is old0 of lane (126 - j) / 2 for an even j, old1 of lane (127 - j) / 2 for an odd one)
            const float oj = !from_win ? S.vol_old[j] : (j & 1u) ? win[(127u - j) >> 1].old1 : win[(126u - j) >> 1].old0;
            smn = dh_fmin_(smn, oj); smx = dh_fmax_(smx, oj);
        }
        S.mn[k] = dh_fmin_(pmn, smn); S.mx[k] = dh_fmax_(pmx, smx);
    }
    for (uint32_t l = 0; l < DH_WAVE; l++) {
        const uint32_t e0 = 2u * l, e1 = e0 + 1u, a = e0 >= k0 && e0 < k1 ? e0 : k0, b = e1 >= k0 && e1 < k1 ? e1 : k0;
        agc[l] = DhAgcPair{ S.mn[a], S.mx[a], S.mn[b], S.mx[b] };
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// Error-bounded FIR (the exact wide-filter kernels at sps 10, i.e. the DMR / YSF pipes).
//
// The reference's dibits and timing steps depend on the filtered samples only through comparisons.  The kernel therefore
// filters with the fused multiply-add FIR (half the vector instructions of the rounded-product chain), carries a proven
// bound on how far each value can be from the reference's, decides every comparison that the bound leaves no doubt about,
// and evaluates the rest -- a few symbols in ten thousand on noise, none on a clean signal -- with the reference's own
// arithmetic (dh_exact_filtered: rounded products, rounded sums in tap order, the double division).  Outputs are the
// reference's bits; only values that never leave the kernel (AGC ring, variance ring) are approximations.
//
// Bound.  u = 2^-24, A = sum |c_i| |x_i| <= ||c||_1 max|x| over the run's raw window, y = value the reference computes.
//   reference chain: |acc_ref - sum c_i x_i| <= g82 A;  FMA chain: |acc_fma - sum c_i x_i| <= g81 A   (g_k = k u / (1 - k u))
//   y_ref = acc_ref / gain (1 + d1), |d1| <= u (1 + 2^-29) (double division, then one rounding to float)
//   y_fma = acc_fma fl32(1 / gain) (1 + d3) = acc_fma / gain (1 + d2)(1 + d3), |d2|, |d3| <= u (1 + 2^-29)
//   => |y_fma - y_ref| <= (g82 + g81 + 3.1 u (1 + g82)) A / gain <= 167 u A / gain           (no overflow, no underflow:
//   runs whose max |x| is 0 are exact, runs with max |x| outside [1e-25, 1e15] or a non-finite sample use the exact FIR)
// The slicer's own float operations (window sums, /10, (max + min) / 2, the 0.625 thresholds) run on both sides with the
// same operation sequence; on perturbed operands they add at most 62 u A / gain between a mid-symbol average and a
// threshold (counted operation by operation in DESIGN.md section 3: 39.8 u A / gain for both sides together).  With
//   e = 240 u (||c||_1 / gain) max|x|      (dh_fir_error_coefficient: 240 u ||c||_1 / gain, rounded up)
// an average and a threshold computed from values with radii <= e differ from the reference's difference by at most
// (1 + 2.25) 167/240 e + 62/240 e < 2.53 e; a comparison is DECIDED when they are further apart than T = 3.5 e.
// e of a ring entry is the e of the run that produced it: kept as two maxima over >= 100-symbol buckets (DH_ST_E_*).
// The same scheme serves the narrow filter at a run-time samples-per-symbol (the NXDN pipe).
template <int NZ, bool FAST, int SPS> struct DhIsBounded {
    static constexpr bool value = !FAST && ((NZ == 80 && SPS == 10) || (NZ == 160 && SPS != 10));
};
// Diagnostic builds only (tools/phase_budget.sh): -DDH_STOP_AFTER=n leaves out the phases after Pn of every run (the
// results are then wrong; the instruction counters of such builds, subtracted from each other, give the per-phase budget)
#ifndef DH_STOP_AFTER
#define DH_STOP_AFTER 99
#endif
#define DH_BOUND_T_FACTOR 3.5f
#define DH_BOUND_XMAX_LO 1e-25f
#define DH_BOUND_XMAX_HI 1e15f

// kappa u ||c||_1 / gain, rounded up (host side, once per engine).  kappa = 240 for the 81 taps the bound above was written
// for (gamma_82 + gamma_81 + 3.1 u = 167 u, times 1.44 of head room for the slicer's own roundings); for n taps the two
// accumulation chains give (2 n + 5) u, and the same proportion is kept: kappa = 1.44 (2 n + 5).  The slicer's roundings
// grow with the samples per symbol (sums of sps terms): both sides together <= 2 (avg + umid) u A / gain with
//   vol = (sps (sps + 1) / 2 - 1) / sps + 1,  centre = vol + 1,  umid = (vol + centre + 1) 0.625 + centre + 1,
//   avg = (w (w + 1) / 2 - 1) / w + 1 for a mid-symbol window of w samples
// = 68 at sps 20 (w 6), 119 at sps 40 (w 14): (3.25 (2 n + 5) + that) / kappa stays below 2.8 for every filter and sps the
// engine accepts, under the decision threshold T = 3.5 e.
inline float dh_fir_error_coefficient(const float* taps_half, uint32_t nz, double gain) {
    double l1 = 0.0;
    for (uint32_t i = 0; i <= nz; i++) { const double c = taps_half[i <= nz / 2 ? i : nz - i]; l1 += c < 0 ? -c : c; }
    const double kappa = nz == 80 ? 240.0 : 1.44 * (2.0 * (nz + 1) + 5.0);
    const double coef = kappa * 5.9604644775390625e-08 * l1 / (gain < 0 ? -gain : gain) * 1.0001;
    float f = (float) coef;
    if ((double) f < coef) { union { float f; uint32_t u; } b; b.f = f; b.u++; f = b.f; }
    return f;
}

// The reference's filtered sample at filtered position f of this push's virtual stream V = tail ++ in
// (rrc_filter.cpp:22-34 for one output): needs V[f .. f + NZ].  Per lane, no barriers.  tapsf = first half + centre.
template <int NZ>
DH_HD float dh_exact_filtered(const float* tail, uint32_t tc, const float* in, uint32_t nv, const float* tapsf, double gain, double rgain, int32_t f) {
    if (f < 0 || (uint32_t) f + (uint32_t) NZ >= nv) return 0.0f;       // not available (callers only ask for positions they hold)
    float acc = 0.0f;
    for (int i = 0; i <= NZ; i++) {
        const float c = tapsf[i <= NZ / 2 ? i : NZ - i];
        const float x = dh_virtual_sample(tail, tc, in, (uint32_t) f + (uint32_t) i);
        const float prod = c * x;
        acc = acc + prod;
    }
    return dh_div_gain(acc, gain, rgain);
}

// The rare paths of the error-bounded kernels (inlined: as real calls they would force the kernel's argument block into
// scratch memory).  What they need to know lives in LDS between runs (DhBoundState), not in vector registers: all 128 are
// taken across the FIR, and a value parked there is a spill in the hot loop.  (The seven words the run loop itself reads and
// writes in every run fit the scalar file without one -- tools/asm_census.py -- and are carried there, see the struct.)
#define DH_COLD DH_HD

// bookkeeping of the error-bounded kernels between runs, in LDS (words 48.. of the tap block: the wide filter uses 41)
struct DhBoundState {
    int32_t cur_start, cur_off, prev_start, prev_off;   // filtered positions of symbol 0 of the current / previous variance block, their offsets
    uint32_t blk_flags;                                 // bit 0: the current block's start is known, bit 1: the previous block's
    uint32_t n_uncertain, n_exact_runs, n_exact_blocks;
    // (what only the run loop itself reads and writes in every run -- the error radii of the current variance block and of the current /
    // previous >= 100-symbol bucket, the bucket's symbol count, and its own copies of blk_flags, cur_start and cur_off -- is carried in
    // scalar registers there: dh_rrc_demod_channel)
};
#define DH_BOUND_STATE(S) (reinterpret_cast<DhBoundState*>((S).bound))
DH_HD float dh_uniform_f(float x) { union { float f; uint32_t u; } b; b.f = x; b.u = dh_uniform(b.u); return b.f; }

// What the exact evaluation of one symbol needs to know about the stream (error-bounded kernels)
struct DhExactCtx {
    const float* tail; uint32_t tc; const float* in; uint32_t nv;      // the virtual stream V = tail ++ in
    const float* tapsf; double gain, rgain; float sps_rcp;
    int32_t cur_start, cur_off, prev_start, prev_off; uint32_t blk_flags;
    uint32_t k0;                                                        // ring slots [k0, k] hold this run's volumes (S.vol_new)
    float e_eff; int32_t levels, invert;
};
// filtered position of sample 0 of ring slot j as seen from symbol k of the current block: slots <= k belong to the
// current block, the others still hold the previous block's symbols; INT32_MIN = a slot never written (exact zero)
DH_HD int32_t dh_slot_position(const DhExactCtx& C, uint32_t j, uint32_t k, uint32_t sps) {
    if (j <= k) return (C.blk_flags & 1u) ? C.cur_start + (int32_t) (j * sps) + (j ? C.cur_off : 0) : INT32_MIN;
    return (C.blk_flags & 2u) ? C.prev_start + (int32_t) (j * sps) + (j ? C.prev_off : 0) : INT32_MIN;
}

// ---- the same two exact evaluations with the raw samples staged through LDS (generic sps; used by the narrow filter, whose
// 161-tap chains would otherwise fetch every sample with a dependent load of its own from HBM / L2)
// raw[0 ..] = V[base ..]: the reference's filtered sample at filtered position f (rrc_filter.cpp:22-34), 0 where the stream
// does not hold all of V[f .. f + NZ]
template <int NZ>
DH_HD float dh_exact_filtered_lds(const float* raw, int32_t base, uint32_t nv, const float* tapsf, double gain, double rgain, int32_t f) {
    if (f < 0 || (uint32_t) f + (uint32_t) NZ >= nv) return 0.0f;
    const float* x = raw + (f - base);
    float acc = 0.0f;
    // eight products at a time, their sixteen LDS reads in flight together, then the eight additions in tap order (written
    // tap by tap this compiled to a read - wait - multiply - add per tap: 110 cycles each, 620 000 for a variance ring)
    // (the 161-tap kernels only: in the 81-tap ones, at 128 registers, the eight products push spills into the hot loop --
    // 24 scratch accesses in the commit phase, DMR chain 6.8 -> 11.9 ms -- and their exact evaluations are 4x rarer and 2x shorter)
    int i = 0;
    constexpr int B = NZ > 80 ? 8 : DH_EXACT_BATCH;
    for (; B > 1 && i + B <= NZ + 1; i += B) {
        float prod[B];
#pragma unroll
        for (int j = 0; j < B; j++) { const int t = i + j; prod[j] = tapsf[t <= NZ / 2 ? t : NZ - t] * x[t]; }
#pragma unroll
        for (int j = 0; j < B; j++) acc = acc + prod[j];
    }
    for (; i <= NZ; i++) {
        const float prod = tapsf[i <= NZ / 2 ? i : NZ - i] * x[i];
        acc = acc + prod;
    }
    return dh_div_gain(acc, gain, rgain);
}
// V[base .. base + count) into raw[] (zeros outside the stream); barriers on both sides
DH_HD void dh_stage_raw(float* raw, const float* tail, uint32_t tc, const float* in, uint32_t nv, int32_t base, uint32_t count) {
    DH_BARRIER();
    DH_FOR_LANES_FRESH(lane) {
        // four loads per lane in flight (one address each: the tail or the input), then their stores
        for (uint32_t e0 = (uint32_t) lane; e0 < count; e0 += 4u * DH_WAVE) {
            float v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
                const uint32_t e = e0 + u * DH_WAVE;
                const int32_t idx = base + (int32_t) e;
                const bool have = e < count && idx >= 0 && (uint32_t) idx < nv;
                const uint32_t at = have ? (uint32_t) idx : tc;                  // (any valid address for the lanes that store a zero)
                const float* src = at < tc ? tail + at : in + (at - tc);
                v[u] = (have || nv > tc) ? *src : 0.0f;
                if (!have) v[u] = 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) { const uint32_t e = e0 + u * DH_WAVE; if (e < count) raw[e] = v[u]; }
        }
    }
    DH_BARRIER();
}
// `stage`: `cap` LDS floats free at the caller's phase.  The mid-symbol window of symbol k and the ten (sps) samples of every
// candidate slot are evaluated TOGETHER: their raw samples are staged side by side (areas of STRIDE words), all chains run at once
// on different lanes, one round of two barriers for the window and up to A - 1 slots -- one after the other (a staging round trip
// to HBM / L2 and an 81-long dependent chain each, three or four times per doubtful symbol) these evaluations were 3 % of the DMR
// chain kernel's time for 0.008 % of its symbols.
template <int NZ>
DH_COLD uint8_t dh_exact_symbol_staged(const DhExactCtx& C, DhDspShared& S, uint32_t k, float* stage, uint32_t cap, uint32_t sps, uint32_t LO, uint32_t HI) {
    const uint32_t W = HI - LO;
    const uint32_t STRIDE = ((W > sps ? W : sps) + (uint32_t) NZ + 1u + 3u) & ~3u;
    const uint32_t A = (cap - 80u) / STRIDE;                          // areas in front of 64 result words + 16 words of slot table (A >= 2: area 0 is the window's)
    // (per_round >= 1 -- or the loop below would never clear its bits -- needs sps + W <= DH_WAVE, W = round(2 sps / 3) - round(sps / 3)
    // <= sps / 3 + 1, and two areas in `stage`: both hold for every sps up to DH_MAX_SPS with the window blocks of dh_dsp_xf_words().
    // The staging areas run over S.sum, behind the filtered samples: the slicing phase has consumed it by the time this is called.)
    static_assert(DH_MAX_SPS + DH_MAX_SPS / 3 + 2 <= DH_WAVE, "a candidate slot's samples and the evaluation window fit one round of lanes");
    static_assert(DH_MAX_SPS + DH_MAX_NZ + 1 <= 4 * DH_WAVE, "an area is staged with four elements per lane");
    uint32_t per_round = dh_min<uint32_t>(A - 1u, (DH_WAVE - W) / sps);
    if (per_round > 8u) per_round = 8u;
    float* scratch = stage + A * STRIDE;
    int32_t* tbl_pos = reinterpret_cast<int32_t*>(scratch + DH_WAVE);  // [8] filtered position of the round's slots (INT32_MIN: never written)
    uint32_t* tbl_slot = reinterpret_cast<uint32_t*>(scratch + DH_WAVE + 8);
    const float mn_a = S.mn[k], mx_a = S.mx[k];
    const float lo_thr = mn_a + 2.5f * C.e_eff, hi_thr = mx_a - 2.5f * C.e_eff;
    uint64_t cand_lo[2] = { 0, 0 }, cand_hi[2] = { 0, 0 };
    for (int h = 0; h < 2; h++) {
        uint64_t vlo = 0, vhi = 0;
        DH_FOR_LANES_FRESH(lane) {
            const uint32_t j = (uint32_t) lane + 64u * (uint32_t) h;
            bool lo = false, hi = false;
            if (j < DH_VOLUME_RB_SIZE) {
                const float v = (j >= C.k0 && j <= k) ? S.vol_new[j] : S.vol_old[j];
                lo = v <= lo_thr; hi = v >= hi_thr;
            }
            DH_BALLOT_ACC(vlo, lo, lane); DH_BALLOT_ACC(vhi, hi, lane);
        }
        cand_lo[h] = vlo; cand_hi[h] = vhi;
    }
    const int32_t mid_base = dh_slot_position(C, k, k, sps) + (int32_t) LO;
    float exact_min = DH_FLT_MAX, exact_max = DH_FLT_MIN;            // the reference's seeds (gfsk_demodulator.cpp:110-111)
    float avg_sum = 0.0f;
    bool first = true;
    uint64_t todo[2] = { cand_lo[0] | cand_hi[0], cand_lo[1] | cand_hi[1] };
    while (first || todo[0] || todo[1]) {
        // this round's slots: the first `ns` set bits of todo, their positions into the table
        const uint32_t pending = (uint32_t) (dh_popc64(todo[0]) + dh_popc64(todo[1]));
        const uint32_t ns = dh_min<uint32_t>(pending, per_round);
        DH_BARRIER();                                                  // the previous round's results and table have been read
        DH_FOR_LANES_FRESH(lane) {
            if ((uint32_t) lane < ns) {
                uint64_t t0 = todo[0], t1 = todo[1];
                for (uint32_t b = 0; b < (uint32_t) lane; b++) { if (t0) t0 &= t0 - 1; else t1 &= t1 - 1; }
                const uint32_t j = t0 ? (uint32_t) dh_ffs64(t0) : 64u + (uint32_t) dh_ffs64(t1);
                tbl_slot[lane] = j; tbl_pos[lane] = dh_slot_position(C, j, k, sps);
            }
        }
        for (uint32_t b = 0; b < ns; b++) { if (todo[0]) todo[0] &= todo[0] - 1; else todo[1] &= todo[1] - 1; }
        DH_BARRIER();
        // raw samples, area by area (wave-uniform loop: area 0 = V[mid_base ..), first round only; area 1 + c = V[pos_c ..)): a lane takes
        // elements lane, lane + 64, ... of the area, its (up to four) loads in flight together.  (As ONE loop over all areas' elements
        // every element paid a division by the area stride, a run-time value wherever the evaluation window is.)
        for (uint32_t a = first ? 0u : 1u; a <= ns; a++) {
            const int32_t base = a == 0u ? mid_base : (int32_t) dh_uniform((uint32_t) tbl_pos[a - 1u]);
            const uint32_t count = (a == 0u ? W : sps) + (uint32_t) NZ + 1u;
            float* const area = stage + a * STRIDE;
            DH_FOR_LANES_FRESH(lane) {
                float v[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; u++) {
                    const uint32_t i = (uint32_t) lane + u * DH_WAVE;
                    const int32_t idx = base + (int32_t) i;
                    const bool have = i < count && base != INT32_MIN && idx >= 0 && (uint32_t) idx < C.nv;
                    const uint32_t at = have ? (uint32_t) idx : C.tc;            // (any valid address for the lanes that store a zero)
                    const float* src = at < C.tc ? C.tail + at : C.in + (at - C.tc);
                    v[u] = (have || C.nv > C.tc) ? *src : 0.0f;
                    if (!have) v[u] = 0.0f;
                }
#pragma unroll
                for (uint32_t u = 0; u < 4u; u++) { const uint32_t i = (uint32_t) lane + u * DH_WAVE; if (i < count) area[i] = v[u]; }
            }
        }
        DH_BARRIER();
        DH_FOR_LANES_FRESH(lane) {
            // lanes 0 .. W - 1: the evaluation window (first round); W + c sps + i: sample i of the round's slot c -- one chain per lane,
            // from ONE call site (area, position and sample index are per-lane values)
            float y = 0.0f;
            uint32_t area = 0; int32_t s0 = mid_base, f = mid_base + lane; bool run = (uint32_t) lane < W && first;
            if ((uint32_t) lane >= W) {
                const uint32_t c = ((uint32_t) lane - W) / sps, i = ((uint32_t) lane - W) - c * sps;
                if (c < ns) { s0 = tbl_pos[c]; f = s0 + (int32_t) i; area = 1u + c; run = s0 != INT32_MIN; }
            }
            if (run) y = dh_exact_filtered_lds<NZ>(stage + area * STRIDE, s0, C.nv, C.tapsf, C.gain, C.rgain, f);
            scratch[lane] = y;
        }
        DH_BARRIER();
        if (first) { for (uint32_t i = 0; i < W; i++) avg_sum += scratch[i]; first = false; }
        for (uint32_t c = 0; c < ns; c++) {
            float vol = 0.0f;                                        // (a slot never written holds an exact zero: ten zeros above)
            for (uint32_t i = 0; i < sps; i++) vol += scratch[W + c * sps + i];
            vol = dh_div_const(vol, (float) sps, C.sps_rcp);
            const uint32_t j = dh_uniform(tbl_slot[c]);
            if ((cand_lo[j >> 6] >> (j & 63u)) & 1u) exact_min = dh_fmin_(exact_min, vol);
            if ((cand_hi[j >> 6] >> (j & 63u)) & 1u) exact_max = dh_fmax_(exact_max, vol);
        }
    }
    const float center = (exact_max + exact_min) / 2.0f;
    const float average = avg_sum / (float) W;
    if (C.levels == 4) {
        const float umid = __builtin_fmaf(exact_max - center, 0.625f, center);
        const float lmid = __builtin_fmaf(exact_min - center, 0.625f, center);
        if (average > center) return average > umid ? 1 : 0;
        return average < lmid ? 3 : 2;
    }
    return average > center ? (uint8_t) !C.invert : (uint8_t) (C.invert != 0);
}
// the variance ring of the block that just ended, recomputed exactly, a chunk of symbols at a time through `stage` (cap floats)
// `rows`: the phases (rows of the transposed ring) to recompute -- all of them, or only those the float estimate could not
// rule out as the arg-min (the others keep their approximate values and are not looked at: see P6)
template <int NZ>
DH_COLD void dh_exact_var_ring_staged(const DhExactCtx& C, DhDspShared& S, uint32_t sps, float* stage, uint32_t cap, uint64_t rows) {
    const uint32_t spc = (cap - (uint32_t) NZ - 3u) / sps;            // symbols per chunk
    const uint64_t all = sps >= 64u ? ~0ull : ((1ull << sps) - 1ull);
    const bool full = (rows & all) == all;
    const uint32_t nrows = full ? sps : (uint32_t) (dh_popc32((uint32_t) (rows & all)) + dh_popc32((uint32_t) ((rows & all) >> 32)));
    for (uint32_t j0 = 0; j0 < DH_VARIANCE_SYMBOLS; j0 += spc) {
        const uint32_t nj = dh_min<uint32_t>(spc, DH_VARIANCE_SYMBOLS - j0);
        const int32_t base = C.cur_start + (int32_t) (j0 * sps) - 1;      // one sample of slack for the block's +-1 step
        dh_stage_raw(stage, C.tail, C.tc, C.in, C.nv, base, nj * sps + (uint32_t) NZ + 3u);
        for (uint32_t r = 0; r * DH_WAVE < nj * nrows; r++) {
            DH_FOR_LANES_FRESH(lane) {
                const uint32_t e = r * DH_WAVE + (uint32_t) lane;
                if (e < nj * nrows) {
                    uint32_t jj, i;
                    if (full) { jj = e / sps; i = e - jj * sps; }
                    else {
                        const uint32_t c = e / nj;                     // the c-th phase of the set
                        jj = e - c * nj;
                        uint64_t m = rows & all;
                        for (uint32_t b = 0; b < c; b++) m &= m - 1;
                        i = (uint32_t) dh_ffs64(m);
                    }
                    const uint32_t j = j0 + jj;
                    const int32_t f = C.cur_start + (int32_t) (j * sps) + (j ? C.cur_off : 0) + (int32_t) i;
                    S.var_rb[i * DH_VARIANCE_SYMBOLS + j] = dh_exact_filtered_lds<NZ>(stage, base, C.nv, C.tapsf, C.gain, C.rgain, f);
                }
            }
        }
    }
    DH_BARRIER();
}

// the rounded-product FIR over the staged window (runs the bound does not cover): outputs into fo[16] per lane
template <int NZ>
DH_COLD void dh_exact_fir_pass(const DhDspParams& P, DhDspShared& S, uint32_t need, DH_LANE_ARRAY(float, (&fo), DH_FIR_L)) {
    float tv[NZ / 2 + 1];
    for (int i = 0; i <= NZ / 2; i++) tv[i] = S.tapsf[i];
    DH_FOR_LANES_FRESH(lane) {
        if ((uint32_t) (lane * DH_FIR_L) < need) {
            // (device: a rare path next to the split-f16 FIR, loads waited for where they are issued)
            dh_fir_lane<NZ, false, false, true>(tv, P.gain, P.rgain, P.inv_gain, S.xf, lane, DH_LA(fo, lane));
        }
    }
}

// One grid for a sps-10 run: the block after a timing step has symbol 0 at 0 and symbol q >= 1 at 10 q + step_off.  Symbol 0's ten
// filtered samples move by step_off (+-1) in place -- all ten read, then written; word -1 of the window block is the last word of
// the variance ring, slot 99 of row 9, which this block stores before anything reads it -- and every symbol q sits at 10 q + step_off.
// Cold and wave-uniform: step_off != 0 only in the run that opens the block behind a timing step.  A kernel that delivers the
// filtered samples has copied this run's out before (dh_rrc_demod_channel: the KEEPF copy precedes this call).
DH_COLD void dh_shift_symbol0(float* fbuf, int32_t step_off) {
    DH_LANE_VALUE(float, t);
    DH_FOR_LANES_FRESH(lane) { DH_LV(t, lane) = fbuf[lane < 10 ? lane : 0]; }
    DH_FOR_LANES_FRESH(lane) { if (lane < 10) fbuf[lane + step_off] = DH_LV(t, lane); }
}

// ---------------------------------------------------------------------------------------------
// ---- P3: symbol windows (gfsk_demodulator.cpp:28-35, 82-83)
// sps 10: the slicer's pairs -- lane l (0..49) takes symbols 2 l and 2 l + 1 of the run, twenty consecutive words on the run's one
// grid (dh_shift_symbol0), read as five ds_read_b128 at compile-time offsets from one per-lane base (dh_lds_run<20>, the sps-20
// body's read: a twenty-word lane stride read four words at a time touches every bank once per eight lanes).  The ring takes
// row i of both symbols, neighbouring slots, as ONE ds_write2_b32 -- ten stores per lane where the two columns took twenty -- and
// S.sum / S.vol_new one each; the last symbol of an odd run goes word by word behind a wave-uniform branch.  The lane keeps its
// two volumes and mid-symbol sums (DhWinPair): the scan and the slicing phase work on the same pairs and, on a run that opens its
// block, take them from there -- the LDS copies are for the other runs and the rare paths.  Until this form a lane held symbols
// l + 1 and l + 65 (ten ds_read_b64, twenty ring stores) and every volume and sum changed lane through LDS.  Each symbol's sums
// run in sample order, as the reference's do.  Lanes beyond the run read words of the window block that nothing will look at and
// store nothing.
// `fbuf`: the run's filtered samples (the window block); sps 10: symbol q of the run (ring slot k0 + q) starts at q sps + step_off;
// the other bodies: at q sps (+ step_off behind symbol 0).
// Leaves S.sum[q], S.vol_new[k0 + q] and column k0 + q of the transposed ring; the caller's barrier publishes them (sps 10: its
// stores are left in flight -- the block is one wavefront's and its LDS instructions complete in order, see the call).
// `win` (sps 10 only): the lane's pair once more, for dh_agc_scan and dh_slice_symbols.
template <int SPS>
DH_HD void dh_symbol_windows(DhDspShared& S, const float* fbuf, uint32_t k0, uint32_t m, int32_t step_off, uint32_t sps, uint32_t ev_lo, uint32_t ev_hi, float sps_rcp,
                             DH_LANE_STRUCT_REF(DhWinPair, win)) {
#define DH_FB(n) fbuf[n]
    if (SPS == 10 && DH_STOP_AFTER >= 3) DH_FOR_LANES_FRESH(lane) {
        const uint32_t l = (uint32_t) lane;
        const uint32_t qa = 2u * l, qb = qa + 1u;
        const bool vb = qb < m;                                                                            // both of the lane's symbols belong to the run
        const float* src = l < 50u ? fbuf + (int32_t) (l * 20u) + step_off : fbuf;                        // (lanes beyond a block read symbols 0 and 1 and store nothing)
        // (the scan's suffix source, ring slots 126 - 2 l and 127 - 2 l as they stood before this run: requested in front of the
        // window, so that it arrives with it and the scan starts without a load of its own)
        float x[20], v[10], w[10], old0, old1;
        dh_lds_run20_with_pair(src, x, S.vol_old + (126u - qa), old0, old1);
#pragma unroll
        for (int i = 0; i < 10; i++) { v[i] = x[i]; w[i] = x[10 + i]; }
        float vola = v[0], volb = w[0];
#pragma unroll
        for (int i = 1; i < 10; i++) { vola += v[i]; volb += w[i]; }
        // samples ev_lo .. ev_hi - 1 = 3 .. 6 (the first chain's steps kept apart from the second's: as one pair of chains the
        // compiler packed them -- three v_pk_add_f32 behind six v_mov that bring the operands into register pairs)
        float mida = v[3] + v[4]; DH_TO_VGPR(mida); mida += v[5]; DH_TO_VGPR(mida); mida += v[6]; DH_TO_VGPR(mida);
        const float midb = ((w[3] + w[4]) + w[5]) + w[6];
        const float volume_a = dh_div_const(vola, 10.0f, sps_rcp), volume_b = dh_div_const(volb, 10.0f, sps_rcp);
        const uint32_t ka = k0 + qa;
        if (vb) {
            dh_lds_store_rows10_pair(S.var_rb + ka, v, w);                                                 // transposed ring: phase-major
            dh_lds_store_pair(S.sum + qa, mida, midb); dh_lds_store_pair(S.vol_new + ka, volume_a, volume_b);
        }
        if (DH_UNLIKELY((m & 1u) != 0u)) {                                                                 // (wave-uniform: the last symbol of an odd run stands alone)
            if (qb == m) {
                dh_lds_store_row10<0>(S.var_rb + ka, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
                S.sum[qa] = mida; S.vol_new[ka] = volume_a;
            }
        }
        DH_LS(win, lane) = DhWinPair{ volume_a, volume_b, mida, midb, old0, old1 };
    }
    // sps 20 (a FIR pass holds at most 51 symbols): one symbol per lane, q = lane + 1, lane 63: symbol 0; its twenty samples as five
    // ds_read_b128 (sixteen bytes from a four-byte aligned address).  Twenty words per lane read in fours touch every bank once per
    // eight lanes; read one word at a time (the general form below) every read was a four-way conflict.
    if (SPS == 20 && DH_STOP_AFTER >= 3) DH_FOR_LANES_FRESH(lane) {
        const uint32_t l = (uint32_t) lane;
        const uint32_t q = l < 63u ? l + 1u : 0u;
        const bool valid = q < m;
        const float* src = valid && q > 0u ? fbuf + (int32_t) (q * 20u) + step_off : fbuf;       // (lanes beyond the run read symbol 0 and store nothing)
        float v[20];
        dh_lds_run<20>(src, v);
        float vol = v[0];
#pragma unroll
        for (int i = 1; i < 20; i++) vol += v[i];
        const float mid = ((((v[7] + v[8]) + v[9]) + v[10]) + v[11]) + v[12];                    // samples ev_lo .. ev_hi - 1 = 7 .. 12
        const float volume = dh_div_const(vol, 20.0f, sps_rcp);
        if (valid) {
            const uint32_t k = k0 + q;
            dh_lds_store_row10<0>(S.var_rb + k, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);      // transposed ring: phase-major
            dh_lds_store_row10<1000>(S.var_rb + k, v[10], v[11], v[12], v[13], v[14], v[15], v[16], v[17], v[18], v[19]);
            S.sum[q] = mid; S.vol_new[k] = volume;
        }
        dh_lds_stores_done();
    }
    // sps 40 (a pass holds at most 25 symbols): the same with ten ds_read_b128 per symbol (a forty-word lane stride read one word at a
    // time reaches four banks: eight-way conflicts in the general loop).  (Folded into the sps-20 body with the window bounds as
    // constants, the sps-20 kernels came out with another instruction order: two bodies.)
    if (SPS == 40 && DH_STOP_AFTER >= 3) DH_FOR_LANES_FRESH(lane) {
        const uint32_t l = (uint32_t) lane;
        const uint32_t q = l < 63u ? l + 1u : 0u;
        const bool valid = q < m;
        const float* src = valid && q > 0u ? fbuf + (int32_t) (q * 40u) + step_off : fbuf;       // (lanes beyond the run read symbol 0 and store nothing)
        float v[40];
        dh_lds_run<40>(src, v);
        float vol = v[0], mid = v[13];
#pragma unroll
        for (int i = 1; i < 40; i++) vol += v[i];
#pragma unroll
        for (int i = 14; i < 27; i++) mid += v[i];                                               // samples ev_lo .. ev_hi - 1 = 13 .. 26
        const float volume = dh_div_const(vol, 40.0f, sps_rcp);
        if (valid) {
            const uint32_t k = k0 + q;
            dh_lds_store_row10<0>(S.var_rb + k, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);      // transposed ring: phase-major
            dh_lds_store_row10<1000>(S.var_rb + k, v[10], v[11], v[12], v[13], v[14], v[15], v[16], v[17], v[18], v[19]);
            dh_lds_store_row10<2000>(S.var_rb + k, v[20], v[21], v[22], v[23], v[24], v[25], v[26], v[27], v[28], v[29]);
            dh_lds_store_row10<3000>(S.var_rb + k, v[30], v[31], v[32], v[33], v[34], v[35], v[36], v[37], v[38], v[39]);
            S.sum[q] = mid; S.vol_new[k] = volume;
        }
        dh_lds_stores_done();
    }
    if (SPS != 10 && SPS != 20 && SPS != 40 && DH_STOP_AFTER >= 3) DH_FOR_LANES_FRESH(lane) {
        for (uint32_t q = lane; q < m; q += DH_WAVE) {
            const uint32_t k = k0 + q;
            const uint32_t s = q * sps + (q > 0 ? (uint32_t) step_off : 0u);   // relative to p
            float sum = 0.0f, volume_sum = 0.0f;
            {
                // (the ring stores below may alias the samples as far as the compiler knows: read one by one, every sample would wait out
                // its own LDS round trip before the next is even requested)
                // four samples at a time, all four requested before the first is used; sums in sample order
                uint32_t i = 0;
                for (; i + 4u <= sps; i += 4u) {
                    float value[4];
#pragma unroll
                    for (uint32_t j = 0; j < 4u; j++) value[j] = DH_FB(s + i + j);
#pragma unroll
                    for (uint32_t j = 0; j < 4u; j++) {
                        if (i + j >= ev_lo && i + j < ev_hi) sum += value[j];
                        volume_sum += value[j];
                        S.var_rb[(i + j) * DH_VARIANCE_SYMBOLS + k] = value[j];       // transposed ring: phase-major
                    }
                }
                for (; i < sps; i++) {
                    const float value = DH_FB(s + i);
                    if (i >= ev_lo && i < ev_hi) sum += value;
                    volume_sum += value;
                    S.var_rb[i * DH_VARIANCE_SYMBOLS + k] = value;
                }
            }
            S.sum[q] = sum;
            S.vol_new[k] = dh_div_const(volume_sum, (float) sps, sps_rcp);
        }
    }
#undef DH_FB
}

// ---------------------------------------------------------------------------------------------
// ---- P6: end of a variance block -> timing decision (gfsk_demodulator.cpp:41-80)
// The reference's result depends on the per-phase variances only through (arg-min position, vmin <= 0,
// vmin > 5e6).  Its sums run in symbol order (float total, then double sum of squared deviations): a
// 100-long dependent chain on `sps` lanes.  For sps = 10 a float estimate V' with a proven error bound is
// taken first: 50 lanes = 10 phases x 5 groups of 20 symbols, partials combined through LDS.  With
// u = 2^-24, mu / sigma^2 the exact mean / variance of the phase, A = mean |x|, F(m) = sum (m - x)^2 / 100
// = sigma^2 + (m - mu)^2:
//   |mean_ref - mu| <= 100.1 u A,  |mean' - mu| <= 25.2 u A   =>  |F(mean') - F(mean_ref)| <= (100.1 u A)^2
//   (the estimate's sums run as two interleaved chains of ten per lane -- packed adds / FMAs -- plus one add, so
//   they are shorter than the 20-long chains these constants were derived for: 16 u A and 18 u below)
//   A^2 <= mean x^2 = sigma^2 + mu^2 <= 1.01 (F(mean') + 2 mean'^2)   =>  that difference < 1e-10 (V' + mean'^2)
//   V_ref = F(mean_ref)(1 + 1.2e-14);  V' = F(mean')(1 + 28 u) up to 25 subnormal roundings (< 1e-42)
// so |V' - V_ref| <= tol = 4e-6 V' + 1.2e-10 (V' + mean'^2) + 1e-42, provided nothing overflows (max |x|
// < 1e16 is checked).  If the intervals [V' - tol, V' + tol] separate the smallest phase from all others,
// from 0 and from 5e6, the reference's decision is known; an all-zero phase gives vmin = 0 exactly.
// Anything else (ties, constant input, non-finite or huge samples) is decided by the ordered chain.
// `V`: the virtual stream of the push (for the exact recomputation of the ring); k0: the run's first slot (for the exact context only).
// Returns the step the reference would take: +1, -1 or 0.
struct DhStreamView { const float* tail; uint32_t tc; const float* in; uint32_t nv; float sps_rcp; };
template <int NZ, int SPS, bool BOUNDED>
DH_HD int32_t dh_timing_decision(const DhDspParams& P, DhDspShared& S, DhBoundState* const BS, const DhStreamView& V, uint32_t sps, uint32_t k0, float e_blk) {
    const float* const tail = V.tail; const uint32_t tc = V.tc; const float* const in = V.in; const uint32_t nv = V.nv; const float sps_rcp = V.sps_rcp;
    int32_t new_off = 0;
    {
        bool ordered = true;
        // Phases that can still be the reference's arg-min once an estimate has been taken and could not decide: those whose
        // interval [V' - tol, V' + tol] reaches below the smallest upper end.  Every other phase has V_ref > that upper end
        // >= the smallest V_ref, strictly, so neither the minimum nor a tie: the ordered chain (and, in the error-bounded
        // kernels, the exact recomputation of the ring in front of it) only has to look at these rows.  All rows when no
        // valid set of intervals exists (no estimate, NaN / overflow, an estimate of exactly 0).
        uint64_t chain_rows = ~0ull;
        bool est_done = false;
        // The same estimate without its LDS exchange and with two votes instead of six.  Lane 16 r + 5 j + g takes piece g (20
        // symbols) of phase i = 3 r + j -- three phases per DPP row, so that the five partial sums of a phase are five neighbouring
        // lanes of one row and meet through row_shr (lane g = 4 of each group: ((s4 + s3) + (s2 + s1)) + s0, three roundings
        // where the exchange form has four: the tolerance derived below covers it).  The ten lanes that then hold a phase form
        // its interval; `above` (ruled out by the smallest upper end) and the two kinds of `fine` (guard holds and estimate not exactly
        // 0: fine when ruled out; also positive and below 5e6: fine as a candidate) are the only votes: one candidate and every lane fine is the case
        // decided here -- everything else (an estimate of exactly 0, NaN / overflow, ties) is left to the full form below, which
        // starts over.  ~100 instructions instead of ~260 per block.
        if (SPS == 10 && !P.ordered_timing) {
            DH_LANE_ARRAY(float, gs, 1); DH_LANE_ARRAY(float, gq, 1);
            DH_FOR_LANES_FRESH(lane) {
                const uint32_t r = (uint32_t) lane >> 4, c = (uint32_t) lane & 15u;
                const uint32_t j = (c * 205u) >> 10, g = c - 5u * j, i = 3u * r + j;      // c / 5, c % 5
                const bool act = c < 15u && i < 10u;
                const dh_f4a* row = reinterpret_cast<const dh_f4a*>(S.var_rb + (act ? i * DH_VARIANCE_SYMBOLS + g * 20u : 0u));
                dh_f2 s2 = dh_f2_make(0.0f, 0.0f), q2 = dh_f2_make(0.0f, 0.0f);
#pragma unroll
                for (int q = 0; q < 5; q++) {
                    const dh_f4a v = row[q];
                    const dh_f2 a = dh_f2_make(v.x, v.y), b = dh_f2_make(v.z, v.w);
                    s2 = dh_f2_add(s2, a); s2 = dh_f2_add(s2, b);
                    q2 = dh_f2_fma(a, a, q2); q2 = dh_f2_fma(b, b, q2);
                }
                DH_LA(gs, lane)[0] = act ? s2.x + s2.y : 0.0f; DH_LA(gq, lane)[0] = act ? q2.x + q2.y : 0.0f;
            }
            DH_LANE_ARRAY(float, lo, 1); DH_LANE_ARRAY(float, hi, 1);
            uint64_t vote_above = 0, fine_cand = 0, fine_out = 0;
            dh_row_sum5_pair(gs, gq);
            DH_FOR_LANES_FRESH(lane) {
                const uint32_t r = (uint32_t) lane >> 4, c = (uint32_t) lane & 15u;
                const bool own = (((r == 3u ? 0x0010u : 0x4210u) >> c) & 1u) != 0u;      // this lane holds a phase: lane 4, 9 or 14 of its row (row 3: phase 9 only)
                const float total = DH_LA(gs, lane)[0], e = DH_LA(gq, lane)[0] * 0.01f;      // e = mean x^2
                const float mean = total * 0.01f;
                const float v = __builtin_fmaf(-mean, mean, e);
                float tol = __builtin_fmaf(e, 4e-6f, 1e-42f);
                if (BOUNDED && e_blk > 0.0f) tol += 8.0f * e_blk * dh_sqrt_upper(__builtin_fmaxf(v, 0.0f) + 4.0f * e_blk * e_blk) + 8.0f * e_blk * e_blk;      // (see the full form below)
                const float l = own ? v - tol : DH_FLT_MAX, h = own ? v + tol : DH_FLT_MAX;
                DH_LA(lo, lane)[0] = l; DH_LA(hi, lane)[0] = h;
                const bool sane = e < 1e30f && v != 0.0f;
                DH_BALLOT_ACC(fine_cand, !own || (sane && l > 0.0f && h < 4999999.0f), lane);      // fine as a candidate
                DH_BALLOT_ACC(fine_out, !own || sane, lane);                                       // fine when ruled out
            }
            const float hmin = DH_WAVE_MIN(hi);
            DH_FOR_LANES_FRESH(lane) {
                DH_BALLOT_ACC(vote_above, DH_LA(lo, lane)[0] > hmin, lane);
            }
            // The verdict is scalar logic on the three ballots: every lane fine for what it is (ruled out / candidate) and exactly
            // one candidate.  A lone candidate is one of the ten lanes that hold a phase (the other lanes share one interval: all of
            // them candidates or none), lane 16 r + 5 j + 4 for phase 3 r + j: phases 1 .. 4 step up, 5 .. 8 down, 0 and 9 stay.
            const uint64_t cand = ~vote_above;
            const uint64_t unfit = (vote_above & ~fine_out) | (cand & ~fine_cand);
            if (DH_LIKELY((unfit | (cand & (cand - 1))) == 0 && cand != 0)) {
                est_done = true; ordered = false;
                constexpr uint64_t UP = (1ull << 9) | (1ull << 14) | (1ull << 20) | (1ull << 25), DOWN = (1ull << 30) | (1ull << 36) | (1ull << 41) | (1ull << 46);
                new_off = (cand & UP) ? +1 : (cand & DOWN) ? -1 : 0;
            }
        }
        if (SPS == 10 && !P.ordered_timing && !est_done) {
            DH_BARRIER();                                   // mn / mx are dead from here: scratch
            float* psum = S.mn; float* pd = S.mx;
            // ONE pass over the ring: sum and sum of squares together, two interleaved chains per lane (packed adds / FMAs).
            // V' = Q' / 100 - mean'^2 loses more to cancellation than the reference's two passes, and its tolerance says
            // so: with S', Q' the float sums (chains of 10 + 1 + 4 roundings: 15 u), 0.01f for 1 / 100 (0.4 u) and m2 =
            // mean x^2 = sigma^2 + mu^2 >= A^2:
            //   |Q' 0.01f - m2| <= 16.4 u m2,  |mean' - mu| <= 16.4 u A  =>  |mean'^2 - mu^2| <= 32.8 u m2,  the final fma 1 u m2
            //   |V' - sigma^2| <= 50.2 u m2 = 3.0e-6 m2;  V_ref within (100.1 u A)^2 + 1.2e-14 V of sigma^2: 3.6e-11 m2
            // so tol = 4e-6 m2' + 1e-42 (m2' = Q' 0.01f, within 1e-6 of m2; 1e-42 for up to ~120 subnormal roundings).
            // A strong DC component (mu^2 >> sigma^2) widens the intervals; what they cannot separate goes to the ordered
            // chain as before.
            DH_FOR_LANES_FRESH(lane) {
                if (lane < 50) {
                    // lane = 5 i + g: eight consecutive lanes then read 16-byte pieces 20 or 40 words apart, which fall into
                    // eight different groups of four banks (with lane = 10 g + i two of every eight collided: 50 LDS cycles
                    // per block, all of this phase's bank conflicts)
                    const uint32_t i = ((uint32_t) lane * 205u) >> 10, g = (uint32_t) lane - 5u * i;      // lane / 5, lane % 5
                    const uint32_t ro = i * DH_VARIANCE_SYMBOLS + g * 20u;
                    const dh_f4a* row = reinterpret_cast<const dh_f4a*>(S.var_rb + ro);
                    dh_f2 s2 = dh_f2_make(0.0f, 0.0f), q2 = dh_f2_make(0.0f, 0.0f);
#pragma unroll
                    for (int q = 0; q < 5; q++) {
                        const dh_f4a v = row[q];
                        const dh_f2 a = dh_f2_make(v.x, v.y), b = dh_f2_make(v.z, v.w);
                        s2 = dh_f2_add(s2, a); s2 = dh_f2_add(s2, b);
                        q2 = dh_f2_fma(a, a, q2); q2 = dh_f2_fma(b, b, q2);
                    }
                    psum[lane] = s2.x + s2.y; pd[lane] = q2.x + q2.y;
                }
            }
            DH_BARRIER();
            // lanes 0..9 hold one phase each; the others hold neutral values
            DH_LANE_ARRAY(float, lo, 1); DH_LANE_ARRAY(float, hi, 1);
            uint64_t vote_guard = 0, vote_vzero = 0, vote_zero = 0, vote_pos = 0, vote_small = 0, vote_above = 0;
            DH_FOR_LANES_FRESH(lane) {
                float l = DH_FLT_MAX, h = DH_FLT_MAX;
                bool guard = true, vzero = false;
                if (lane < 10) {
                    const int i = lane;
                    const float total = (((psum[5 * i] + psum[5 * i + 1]) + psum[5 * i + 2]) + psum[5 * i + 3]) + psum[5 * i + 4];
                    const float e = ((((pd[5 * i] + pd[5 * i + 1]) + pd[5 * i + 2]) + pd[5 * i + 3]) + pd[5 * i + 4]) * 0.01f;      // mean x^2
                    const float mean = total * 0.01f;
                    const float v = __builtin_fmaf(-mean, mean, e);
                    float tol = __builtin_fmaf(e, 4e-6f, 1e-42f);
                    // error-bounded mode: the ring holds values within e_blk of the reference's; moving every sample by
                    // up to e_blk moves the mean by <= e_blk, every deviation by <= 2 e_blk and the variance by
                    // <= 4 e_blk sqrt(V) + 4 e_blk^2 (Cauchy-Schwarz); taken twice over for the float mean's own rounding
                    if (BOUNDED && e_blk > 0.0f) tol += 8.0f * e_blk * dh_sqrt_upper(__builtin_fmaxf(v, 0.0f) + 4.0f * e_blk * e_blk) + 8.0f * e_blk * e_blk;
                    guard = e < 1e30f;                           // false for NaN, and for samples beyond ~1e15 (e overflows first)
                    vzero = v == 0.0f;
                    l = v - tol; h = v + tol;
                }
                DH_LA(lo, lane)[0] = l; DH_LA(hi, lane)[0] = h;
                DH_BALLOT_ACC(vote_guard, guard, lane);
                DH_BALLOT_ACC(vote_vzero, vzero, lane);
                DH_BALLOT_ACC(vote_pos, l > 0.0f, lane);
                DH_BALLOT_ACC(vote_small, h < 4999999.0f, lane);
            }
            const uint32_t ten = 0x3FFu;
            if (((uint32_t) vote_vzero & ten) && !(BOUNDED && e_blk > 0.0f)) {       // (approximate samples prove nothing about exact zeros)
                // an estimate of exactly 0: only a phase whose hundred samples are all (+-)0 has vmin == 0 for sure (tiny
                // samples square to 0 in float, not in the reference's double) -- look at the bits
                uint64_t vote_nz = 0;
                DH_FOR_LANES_FRESH(lane) {
                    uint32_t any = 0;
                    if (lane < 50) {
                        const uint32_t g = ((uint32_t) lane * 205u) >> 11, i = (uint32_t) lane - 10u * g;
                        const uint32_t* row = reinterpret_cast<const uint32_t*>(S.var_rb + i * DH_VARIANCE_SYMBOLS + g * 20u);
#pragma unroll
                        for (int q = 0; q < 20; q++) any |= row[q];
                    }
                    DH_BALLOT_ACC(vote_nz, (any << 1) != 0u, lane);
                }
                const uint32_t nz = (uint32_t) (vote_nz | (vote_nz >> 10) | (vote_nz >> 20) | (vote_nz >> 30) | (vote_nz >> 40));
                vote_zero = ~nz & ten;
            }
            const float hmin = DH_ROW0_MIN(hi);                 // (lanes 10 .. 15 hold FLT_MAX)
            DH_FOR_LANES_FRESH(lane) { DH_BALLOT_ACC(vote_above, DH_LA(lo, lane)[0] > hmin, lane); }
            const uint32_t above = (uint32_t) vote_above & ten;
            const uint32_t cand = ~above & ten;                 // phases whose interval reaches below hmin
            if (((uint32_t) vote_guard & ten) != ten) {
            } else if ((uint32_t) vote_zero & ten) {
                ordered = false;                                // vmin == 0 exactly: no step
            } else if (dh_popc32(cand) == 1 && ((uint32_t) vote_pos & cand) && ((uint32_t) vote_small & cand)) {
                ordered = false;
                const uint32_t vmin_pos = (uint32_t) dh_ffs64((uint64_t) cand);
                if (vmin_pos > 0 && vmin_pos < 5) new_off = +1;
                else if (vmin_pos >= 5 && vmin_pos < 9) new_off = -1;
            }
            // (the candidates are not handed on here: one more live value costs the 81-tap kernels four scratch accesses in
            // their hot loop, and they reach this point in 0.02 % of the blocks -- the 161-tap, sps-20 kernel in 1.3 %)
        }
        if (ordered && SPS != 10 && sps <= DH_WAVE && !P.ordered_timing && (!BOUNDED || P.exact_mode == 0)) {
            // (sps 33 .. 64, e.g. POCSAG's 40: one lane per phase, chains of 100 + 1 fused terms -- (1 + u)^102 - 1 < 6.1e-6, still
            // inside the 8e-6 V' below; the float mean is then the reference's own chain, within 100.1 u A of the true one.  The
            // in-order double chain cost that slicer a fifth of its time, every block.)
            // Run-time sps with at least one lane per phase: a float estimate like the sps-10 one.  G = 64 / sps groups
            // per phase, lane g sps + i takes a contiguous piece of row i -- `seg` = 4 ceil(25 / G) ring entries, read 16
            // bytes at a time -- and the partial sums meet in LDS.  The bound of the sps-10 estimate holds with 8e-6 V'
            // for 4e-6 V' (chains of up to 52 fused terms + G partials); in the error-bounded kernels the ring holds
            // values within e_blk of the reference's, which moves a variance by |2 cov(x, d) + var(d)| <= 2 e sigma +
            // e^2 with sigma <= sqrt(V) + e, i.e. <= 2 e sqrt(V) + 3 e^2 (taken as 2.5 e sqrt(V) + 4 e^2).  An estimate
            // of exactly 0, a NaN or an overflow is left to the chain below.
            DH_BARRIER();                                   // mn / mx are dead from here: scratch
            float* psum = S.mn; float* pd = S.mx; float* pmean = S.mn + 64;
            const uint32_t G = DH_WAVE / sps, active = G * sps, quads = (25u + G - 1u) / G;
            for (int pass = 0; pass < 2; pass++) {
                DH_FOR_LANES_FRESH(lane) {
                    if ((uint32_t) lane < active) {
                        const uint32_t g = (uint32_t) lane / sps, i = (uint32_t) lane - g * sps;
                        const uint32_t q0 = g * quads;                                 // first 16-byte piece of this lane
                        const dh_f4a* row = reinterpret_cast<const dh_f4a*>(S.var_rb + i * DH_VARIANCE_SYMBOLS);
                        float mean = 0.0f;
                        if (pass == 1) {
                            float total = 0.0f;
                            for (uint32_t gg = 0; gg < G; gg++) total += psum[gg * sps + i];
                            mean = total * 0.01f;
                            if (g == 0) pmean[i] = mean;
                        }
                        float acc = 0.0f;
                        for (uint32_t q = 0; q < quads; q += 3u) {                     // three pieces in flight
                            dh_f4a v[3];
#pragma unroll
                            for (uint32_t j = 0; j < 3u; j++) v[j] = row[dh_min<uint32_t>(q0 + q + j, 24u)];
#pragma unroll
                            for (uint32_t j = 0; j < 3u; j++) {
                                if (q + j < quads && q0 + q + j < 25u) {
                                    if (pass == 0) { acc += v[j].x; acc += v[j].y; acc += v[j].z; acc += v[j].w; }
                                    else {
                                        const float d0 = mean - v[j].x, d1 = mean - v[j].y, d2 = mean - v[j].z, d3 = mean - v[j].w;
                                        acc = __builtin_fmaf(d0, d0, acc); acc = __builtin_fmaf(d1, d1, acc);
                                        acc = __builtin_fmaf(d2, d2, acc); acc = __builtin_fmaf(d3, d3, acc);
                                    }
                                }
                            }
                        }
                        if (pass == 0) psum[lane] = acc; else pd[lane] = acc;
                    }
                }
                DH_BARRIER();
            }
            DH_LANE_ARRAY(float, iv_lo, 1); DH_LANE_ARRAY(float, iv_hi, 1);
            uint64_t v_ok = 0, v_pos = 0, v_small = 0, v_big = 0, v_above = 0;
            DH_FOR_LANES_FRESH(lane) {
                float l = DH_FLT_MAX, h = DH_FLT_MAX;
                bool ok = true;
                if ((uint32_t) lane < sps) {
                    float v = 0.0f;
                    for (uint32_t gg = 0; gg < G; gg++) v += pd[gg * sps + (uint32_t) lane];
                    v *= 0.01f;
                    const float mean = pmean[lane];
                    const float e = __builtin_fmaf(mean, mean, v);
                    float tol = __builtin_fmaf(v, 8e-6f, __builtin_fmaf(e, 1.2e-10f, 1e-42f));
                    if (BOUNDED && e_blk > 0.0f) tol += 2.5f * e_blk * __builtin_sqrtf(v) + 4.0f * e_blk * e_blk;
                    ok = e < 1e30f && v != 0.0f;
                    l = v - tol; h = v + tol;
                }
                DH_LA(iv_lo, lane)[0] = l; DH_LA(iv_hi, lane)[0] = h;
                DH_BALLOT_ACC(v_ok, ok, lane);
                DH_BALLOT_ACC(v_pos, l > 0.0f, lane);
                DH_BALLOT_ACC(v_small, h < 4999999.0f, lane);
                DH_BALLOT_ACC(v_big, l > 5000001.0f, lane);
            }
            const float hmin = DH_WAVE_MIN(iv_hi);
            DH_FOR_LANES_FRESH(lane) { DH_BALLOT_ACC(v_above, DH_LA(iv_lo, lane)[0] > hmin, lane); }
            const uint64_t phases = sps >= 64u ? ~0ull : ((1ull << sps) - 1ull);
            const uint64_t cand = ~v_above & phases;                          // phases whose interval reaches below the smallest upper end
            const bool one = cand != 0 && (cand & (cand - 1)) == 0;
            if (one && (v_ok & phases) == phases && (((v_pos & cand) && (v_small & cand)) || (v_big & cand))) {
                ordered = false;
                const uint32_t vmin_pos = (uint32_t) dh_ffs64(cand);
                if (v_big & cand) {
                } else if (vmin_pos > 0 && vmin_pos < sps / 2) new_off = +1;
                else if (vmin_pos >= sps / 2 && vmin_pos < sps - 1) new_off = -1;
            } else if (cand != 0 && (v_ok & phases) == phases) {
                chain_rows = cand;
            }
        }
        if (DH_UNLIKELY(ordered)) {
            // both sums of a phase in symbol order: one phase per lane, its 100 samples contiguous in the transposed
            // ring and fetched 16 bytes at a time.
            // Error-bounded kernels: the ring holds values within e_blk of the reference's.  At sps 10 the estimate above
            // has already failed, so the chain runs on the reference's samples -- all thousand of this block, recomputed
            // exactly.  At a run-time sps there is no estimate: the chain first runs on the ring as it is (attempt 0) and
            // its result stands if the intervals [V - tol, V + tol] separate the smallest phase from all others, from 0 and
            // from 5e6; otherwise attempt 1 recomputes the ring exactly.  tol: samples moved by <= e move the variance
            // by |2 cov(x, d) + var(d)| <= 2 e sigma + e^2 with sigma <= sqrt(V) + e, i.e. <= 2 e sqrt(V) + 3 e^2 (taken
            // as 2.5 e sqrt(V) + 4 e^2); each chain's float mean is within 100.1 u A of the true one, which moves its
            // sum of squared deviations by (that)^2 <= 1e-10 (V + mean^2); the double arithmetic adds 1e-14 V.
            const bool approx_ring = BOUNDED && e_blk > 0.0f;
            for (int attempt = (approx_ring && SPS != 10 && sps > DH_WAVE && !P.ordered_timing && P.exact_mode == 0) ? 0 : 1; attempt < 2; attempt++) {      // (attempt 0 only where the estimate above does not run)
                DH_BARRIER();
                if (approx_ring && attempt == 1) {
                    DhExactCtx C;
                    C.tail = tail; C.tc = tc; C.in = in; C.nv = nv; C.tapsf = S.tapsf; C.gain = P.gain; C.rgain = P.rgain; C.sps_rcp = sps_rcp;
                    C.cur_start = (int32_t) dh_uniform((uint32_t) BS->cur_start); C.cur_off = (int32_t) dh_uniform((uint32_t) BS->cur_off);
                    C.prev_start = 0; C.prev_off = 0; C.blk_flags = dh_uniform(BS->blk_flags);
                    C.k0 = k0; C.e_eff = 0.0f; C.levels = P.levels; C.invert = P.invert;
                    // (the window block is dead here except words 512..575, where the L2 touch of the next window may
                    // still be dropping its dwords: the staged variant uses the words behind them)
                    dh_exact_var_ring_staged<NZ>(C, S, sps, S.xf + 576, dh_dsp_xf_words(NZ) - 576u, chain_rows);
                    BS->n_exact_blocks++;
                    DH_BARRIER();
                }
                DH_LANE_ARRAY(float, iv_lo, 1); DH_LANE_ARRAY(float, iv_hi, 1); DH_LANE_ARRAY(uint32_t, iv_ok, 1);
                DH_FOR_LANES_FRESH(lane) {
                    if ((uint32_t) lane < sps && !((chain_rows >> (uint32_t) lane) & 1ull)) {
                        S.variance[lane] = DH_DBL_MAX;               // ruled out by its interval: never the smallest
                        if (BOUNDED && SPS != 10 && attempt == 0) { DH_LA(iv_lo, lane)[0] = DH_FLT_MAX; DH_LA(iv_hi, lane)[0] = DH_FLT_MAX; DH_LA(iv_ok, lane)[0] = 1u; }
                    } else if ((uint32_t) lane < sps) {
                        const dh_f4a* row = reinterpret_cast<const dh_f4a*>(S.var_rb + lane * DH_VARIANCE_SYMBOLS);
                        float total = 0.0f;
#pragma unroll 5
                        for (int q = 0; q < DH_VARIANCE_SYMBOLS / 4; q++) {
                            const dh_f4a v = row[q];
                            total += v.x; total += v.y; total += v.z; total += v.w;
                        }
                        const double mean = (double) (total / (float) DH_VARIANCE_SYMBOLS);
                        double dsum = 0.0;
#pragma unroll 5
                        for (int q = 0; q < DH_VARIANCE_SYMBOLS / 4; q++) {
                            const dh_f4a v = row[q];
                            const double d0 = mean - (double) v.x, d1 = mean - (double) v.y, d2 = mean - (double) v.z, d3 = mean - (double) v.w;
                            const double s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s3 = d3 * d3;
                            dsum += s0; dsum += s1; dsum += s2; dsum += s3;
                        }
                        const double var = dsum / (double) DH_VARIANCE_SYMBOLS;
                        S.variance[lane] = var;
                        if (BOUNDED && SPS != 10 && attempt == 0) {
                            // this phase's interval, as floats rounded outwards (2e-7 V covers the two conversions)
                            const double eb = (double) e_blk;
                            const double tol = 2.5 * eb * __builtin_sqrt(var) + 4.0 * eb * eb + 2e-10 * (var + mean * mean) + 2e-7 * var + 1e-40;
                            DH_LA(iv_lo, lane)[0] = (float) (var - tol); DH_LA(iv_hi, lane)[0] = (float) (var + tol);
                            DH_LA(iv_ok, lane)[0] = (var + mean * mean < 1e30) ? 1u : 0u;      // false for NaN / overflow, as in the estimate
                        }
                    } else if (BOUNDED && SPS != 10 && attempt == 0) {
                        DH_LA(iv_lo, lane)[0] = DH_FLT_MAX; DH_LA(iv_hi, lane)[0] = DH_FLT_MAX; DH_LA(iv_ok, lane)[0] = 1u;
                    }
                }
                DH_BARRIER();
                if (BOUNDED && SPS != 10 && attempt == 0) {
                    // is the reference's (arg-min, vmin <= 0, vmin > 5e6) beyond doubt?  One vote per question.
                    const float hmin = DH_WAVE_MIN(iv_hi);
                    uint64_t v_above = 0, v_ok = 0, v_pos = 0, v_small = 0, v_big = 0;
                    DH_FOR_LANES_FRESH(lane) {
                        const float l = DH_LA(iv_lo, lane)[0], h = DH_LA(iv_hi, lane)[0];
                        DH_BALLOT_ACC(v_above, l > hmin, lane);
                        DH_BALLOT_ACC(v_ok, DH_LA(iv_ok, lane)[0] != 0u, lane);
                        DH_BALLOT_ACC(v_pos, l > 0.0f, lane);
                        DH_BALLOT_ACC(v_small, h < 4999999.0f, lane);
                        DH_BALLOT_ACC(v_big, l > 5000001.0f, lane);
                    }
                    const uint64_t phases = sps >= 64u ? ~0ull : ((1ull << sps) - 1ull);
                    const uint64_t cand = ~v_above & phases;                  // phases whose interval reaches below the smallest upper end
                    const bool one = cand != 0 && (cand & (cand - 1)) == 0;
                    const bool sure = one && (v_ok & phases) == phases && (((v_pos & cand) && (v_small & cand)) || (v_big & cand));
                    if (!sure) continue;                                      // attempt 1: the exact ring
                    DH_FOR_LANES_FRESH(lane) { if (DH_IS_LANE0(lane)) S.stats[1]++; }
                    const uint32_t vmin_pos = (uint32_t) dh_ffs64(cand);
                    if (v_big & cand) {
                    } else if (vmin_pos > 0 && vmin_pos < sps / 2) new_off = +1;
                    else if (vmin_pos >= sps / 2 && vmin_pos < sps - 1) new_off = -1;
                    break;
                }
                double vmin = S.variance[0]; uint32_t vmin_pos = 0;
                for (uint32_t i = 1; i < sps; i++) if (S.variance[i] < vmin) { vmin = S.variance[i]; vmin_pos = i; }
                DH_FOR_LANES_FRESH(lane) { if (DH_IS_LANE0(lane)) S.stats[1]++; }
                if (vmin <= 0 || vmin > 5000000) {
                } else if (vmin_pos > 0 && vmin_pos < sps / 2) new_off = +1;
                else if (vmin_pos >= sps / 2 && vmin_pos < sps - 1) new_off = -1;
                break;
            }
        }
    }
    return new_off;
}

// ---------------------------------------------------------------------------------------------
// ---- P5: thresholds + slice (gfsk_demodulator.cpp:88-106 / fsk_demodulator.cpp:89-99)
// error-bounded mode: a comparison whose two sides are closer than T cannot be trusted to come out as the
// reference's; those symbols are decided exactly below, and that decision replaces the dibit stored here
// TWO symbols per lane, q = 2 lane and 2 lane + 1 (a run has at most 100): their AGC extremes, window sums and everything
// derived from them are pairs, so centre, average, the two thresholds and the three distances are packed operations for
// both symbols -- one pass of ~40 vector instructions instead of two of ~37.  Every operation is the one the one-symbol
// form performs (same operands, same order), so the dibits and the doubts are the same.
// `out`: where symbol 0 of the run goes; `agc`: the scan's own results for the lane's two symbols, used when the run starts its
// block.  Doubtful symbols are stored provisionally and overwritten by dh_settle_doubts; their votes come back in vote_a (symbols 2 l)
// and vote_b (2 l + 1).
struct DhSliceSetup { bool four_levels, e_pos, width_pow2, pair_store; float T_eff, inv_width; };
template <int SPS, int LV, bool BOUNDED>
DH_HD void dh_slice_symbols(const DhDspParams& P, DhDspShared& S, DH_LANE_STRUCT_IN(DhAgcPair, agc), DH_LANE_STRUCT_IN(DhWinPair, win), uint8_t* out, uint32_t k0, uint32_t m, uint32_t ev_lo, uint32_t ev_hi,
                            const DhSliceSetup& U, uint64_t& vote_a, uint64_t& vote_b) {
    const bool four_levels = U.four_levels, e_pos = U.e_pos, width_pow2 = U.width_pow2, pair_store = U.pair_store;
    const float T_eff = U.T_eff, inv_width = U.inv_width;
    DH_FOR_LANES_FRESH(lane) {
        const uint32_t qa = 2u * (uint32_t) lane;
        const bool va = qa < m, vb = qa + 1u < m;
        const uint32_t qq = va ? qa : 0u, k = k0 + qq;                            // (lanes beyond the run recompute symbols 0 / 1: in-range reads, no store)
        // (a run that starts its block: the lane's symbols 2 l, 2 l + 1 are the ring slots the AGC scan left in its registers)
        const DhAgcPair& own = DH_LS(agc, lane);
        // (sps 10 likewise: the lane's two mid-symbol sums are the ones the window phase left in its registers; the other runs load all
        // three pairs and wait for them where they stand, dh_lds_pairs3_now)
        const DhWinPair& own_win = DH_LS(win, lane);
        dh_f2 mn, mx, sumq;
        if (SPS == 10) {
            if (DH_LIKELY(k0 == 0u)) { mn = dh_f2_make(own.mn0, own.mn1); mx = dh_f2_make(own.mx0, own.mx1); sumq = dh_f2_make(own_win.sum0, own_win.sum1); }
            else dh_lds_pairs3_now(S.mn + k, S.mx + k, S.sum + qq, mn, mx, sumq);
        } else {
            if (k0 == 0u) { mn = dh_f2_make(own.mn0, own.mn1); mx = dh_f2_make(own.mx0, own.mx1); }
            else { mn = dh_f2_make(S.mn[k], S.mn[k + 1u]); mx = dh_f2_make(S.mx[k], S.mx[k + 1u]); }
            sumq = dh_f2_make(S.sum[qq], S.sum[qq + 1u]);
        }
        const dh_f2 center = dh_f2_scale(dh_f2_add(mx, mn), 0.5f);                // (max + min) / 2.0f: the division by two is exact
        // (sps 20: the division by the window's six samples as reciprocal product + exact residual + correction, dh_div_const; tests/test_numerics.py)
        const dh_f2 average = width_pow2 ? dh_f2_scale(sumq, inv_width) : SPS == 20 ? dh_div_const2(sumq, 6.0f, inv_width)
                                                                                    : dh_f2_make(sumq.x / (float) (ev_hi - ev_lo), sumq.y / (float) (ev_hi - ev_lo));
        const dh_f2 c625 = dh_f2_make(0.625f, 0.625f);
        const dh_f2 umid = dh_f2_fma(dh_f2_sub(mx, center), c625, center);        // one float FMA each: see the one-symbol form below
        const dh_f2 lmid = dh_f2_fma(dh_f2_sub(mn, center), c625, center);
        const bool above_a = average.x > center.x, above_b = average.y > center.y;
        const uint8_t sym4a = above_a ? (average.x > umid.x ? 1 : 0) : (average.x < lmid.x ? 3 : 2);
        const uint8_t sym4b = above_b ? (average.y > umid.y ? 1 : 0) : (average.y < lmid.y ? 3 : 2);
        const uint8_t sym2a = LV == 4 ? (uint8_t) 0 : above_a ? (uint8_t) !P.invert : (uint8_t) (P.invert != 0);
        const uint8_t sym2b = LV == 4 ? (uint8_t) 0 : above_b ? (uint8_t) !P.invert : (uint8_t) (P.invert != 0);
        const uint8_t sa = four_levels ? sym4a : sym2a, sb = four_levels ? sym4b : sym2b;
        bool doubt_a = false, doubt_b = false;
        if (BOUNDED) {
            const dh_f2 du = dh_f2_sub(average, umid), dl = dh_f2_sub(average, lmid), dc = dh_f2_sub(average, center);
            const float da = dh_min3_abs(four_levels ? du.x : DH_FLT_MAX, four_levels ? dl.x : DH_FLT_MAX, dc.x);
            const float db = dh_min3_abs(four_levels ? du.y : DH_FLT_MAX, four_levels ? dl.y : DH_FLT_MAX, dc.y);
            doubt_a = va && e_pos && !(da > T_eff);                               // (!(d > T): a NaN distance is a doubt)
            doubt_b = vb && e_pos && !(db > T_eff);
        }
#ifdef DH_IGNORE_DOUBT
        doubt_a = false; doubt_b = false;
#endif
        // Every valid symbol's dibit is stored, doubtful or not: dh_settle_doubts stores out[q] again for every vote it is handed --
        // later in program order, from this wavefront, to the same address (and behind waits for its own loads, which this store
        // precedes in the memory counter).  The lane's two dibits are neighbours: one 16-bit store when the row position is even
        // (wave-uniform); an odd last symbol of such a run (m odd: wave-uniform too) goes as a byte.
        if (DH_LIKELY(pair_store)) {
            if (vb) *reinterpret_cast<uint16_t*>(out + qa) = (uint16_t) ((uint32_t) sa | ((uint32_t) sb << 8));
            if (DH_UNLIKELY((m & 1u) != 0u)) { if (qa + 1u == m) out[qa] = sa; }
        } else {
            if (va) out[qa] = sa;
            if (vb) out[qa + 1u] = sb;
        }
        DH_BALLOT_ACC(vote_a, doubt_a, lane);
        DH_BALLOT_ACC(vote_b, doubt_b, lane);
    }
}

// the doubtful symbols of a run (votes of dh_slice_symbols), one exact evaluation at a time -- the even symbols' votes first (the evaluations do
// not depend on one another); ONE call site: the evaluation is a thousand instructions of text
template <int NZ>
DH_COLD void dh_settle_doubts(const DhDspParams& P, DhDspShared& S, DhBoundState* const BS, const DhStreamView& V, uint8_t* out, uint32_t k0, float e_eff,
                              uint32_t sps, uint32_t ev_lo, uint32_t ev_hi, uint64_t vote_a, uint64_t vote_b) {
    const float* const tail = V.tail; const uint32_t tc = V.tc; const float* const in = V.in; const uint32_t nv = V.nv; const float sps_rcp = V.sps_rcp;
        DhExactCtx C;
        C.tail = tail; C.tc = tc; C.in = in; C.nv = nv; C.tapsf = S.tapsf; C.gain = P.gain; C.rgain = P.rgain; C.sps_rcp = sps_rcp;
        C.cur_start = (int32_t) dh_uniform((uint32_t) BS->cur_start); C.cur_off = (int32_t) dh_uniform((uint32_t) BS->cur_off);
        C.prev_start = (int32_t) dh_uniform((uint32_t) BS->prev_start); C.prev_off = (int32_t) dh_uniform((uint32_t) BS->prev_off);
        C.blk_flags = dh_uniform(BS->blk_flags);
        C.k0 = k0; C.e_eff = e_eff; C.levels = P.levels; C.invert = P.invert;
        // one evaluation at a time, the even symbols' votes first (the evaluations do not depend on one another); ONE call site:
        // the evaluation is a thousand instructions of text
        uint64_t ta = vote_a, tb = vote_b;
        while ((ta | tb) != 0) {
            uint32_t q;
            if (ta) { q = 2u * (uint32_t) dh_ffs64(ta); ta &= ta - 1; } else { q = 2u * (uint32_t) dh_ffs64(tb) + 1u; tb &= tb - 1; }
            // (the raw samples behind each evaluation are staged through the dead part of the window block: fetched one by one from
            // HBM / L2 by the 81-tap chains, a doubtful symbol cost as much as several whole runs)
            const uint8_t sym = dh_exact_symbol_staged<NZ>(C, S, k0 + q, S.xf + 576, dh_dsp_xf_words(NZ) - 576u, sps, ev_lo, ev_hi);
            DH_FOR_LANES_FRESH(lane) { if (DH_IS_LANE0(lane)) out[q] = sym; }
            BS->n_uncertain++;
        }
}

// ---------------------------------------------------------------------------------------------
// ---- P1 / P2 / P7: what staging a run's raw window and putting its filtered samples back are made of, each stated once.
// Staging itself (P1), the FIR with its store-back layouts (P2) and the P7 half of the fetch ahead are written out in
// dh_rrc_demod_channel: moved behind a call -- a function or an always_inline lambda, arguments by value or by reference --
// every slicer kernel comes out of the compiler with other registers.
// the last window of a push: zeros beyond the input (`w` holds the elements e .. e + 3 of a window with `have` samples)
DH_HD dh_f4 dh_zero_beyond(dh_f4 w, uint32_t e, uint32_t have) {
    w.x = e + 0u < have ? w.x : 0.0f; w.y = e + 1u < have ? w.y : 0.0f;
    w.z = e + 2u < have ? w.z : 0.0f; w.w = e + 3u < have ? w.w : 0.0f;
    return w;
}
// raw-sample window layout: padded one word per 16 for the FIR's lane-strided reads; plain without an RRC stage
// (the samples are then used where they were staged, and the window sums sit right behind them)
#define DH_XP(e) (NZ > 0 ? DH_XPAD(e) : (e))
// the window V[p .. p + DH_FTILE + NZ) sample by sample out of the carried tail and the input, zeros beyond the stream
template <int NZ>
DH_HD void dh_gather_window(DhDspShared& S, const float* tail, uint32_t tc, const float* in, uint32_t nv, uint32_t p) {
    DH_FOR_LANES_FRESH(lane) {
        for (uint32_t e = lane; e < DH_FTILE + NZ; e += DH_WAVE)
            S.xf[DH_XP(e)] = p + e < nv ? dh_virtual_sample(tail, tc, in, p + e) : 0.0f;
    }
}
// A window of DH_FTILE + NZ samples as DH_PF_N groups of 16 bytes per lane: group r holds the elements 4 lane + 256 r ...
// Only the last group is partial: LAST_LANES of its lanes lie inside the window.  GSTEP: words between two groups of a lane
// in the (padded) window block.  STORE_LANES: lanes of the last group that the arrays of halves of the split-f16 FIR reach
// (they are as long as the last block's K range).
template <int NZ> struct DhWindowGroups {
    static constexpr uint32_t GSTEP = NZ > 0 ? DH_XPAD(4u * DH_WAVE) : 4u * DH_WAVE;
    static constexpr uint32_t LAST_LANES = (DH_FTILE + NZ - 4u * DH_WAVE * (DH_PF_N - 1)) / 4u;
    static constexpr uint32_t STORE_LANES = (DH_F16_HALVES_OF(NZ) - 4u * DH_WAVE * (DH_PF_N - 1)) / 4u;
    static_assert((DH_FTILE + NZ) % 4u == 0 && (DH_FTILE + NZ) >= 4u * DH_WAVE * (DH_PF_N - 1) && LAST_LANES <= DH_WAVE, "four full groups + a partial one cover the window");
    static_assert(STORE_LANES >= LAST_LANES && STORE_LANES <= DH_WAVE, "the partial group covers the padded arrays");
};
// a lane's 16 consecutive filtered samples back into the window block, unpadded: four 16-byte stores
// (a macro: as a function the error-bounded sps-10 kernels came out with other registers)
#define DH_STORE_FIR_OUT(xf, lane, fo) do { \
        dh_f4a* dst_ = reinterpret_cast<dh_f4a*>((xf) + DH_FIR_L * (lane)); \
        _Pragma("unroll") for (int j_ = 0; j_ < DH_FIR_L / 4; j_++) { \
            dh_f4a v_; v_.x = DH_LA(fo, lane)[4 * j_]; v_.y = DH_LA(fo, lane)[4 * j_ + 1]; \
            v_.z = DH_LA(fo, lane)[4 * j_ + 2]; v_.w = DH_LA(fo, lane)[4 * j_ + 3]; \
            dst_[j_] = v_; \
        } } while (0)
// split-f16 FIR: the window held in `varr` (five 16-byte groups per lane, as loaded) -> zeros beyond `have`, max |x| of the
// wavefront, the power-of-two scale that puts it into [0.5, 1), the two arrays of halves in the window block.  Returns
// false (nothing stored) when max |x| is outside the range the bound covers -- or NaN: the maximum is taken so that ONE NaN sample
// makes it NaN (dh_max_abs_groups, DH_WAVE_MAX_NAN), and a NaN fails every comparison below.  An infinite sample is above the
// range.  So what reaches the FIR is finite and at most 1e15, and with L1(taps) / gain about 1.45 nothing in it can overflow:
// there is no look at its outputs afterwards.
// ONE (dh_f16_one_chain): the second halves on the scale of the first (dh_f16_split4_plain), k1_out is the one factor kc of
// y = A kc, and k2_out is not used.
template <int NZ, bool ONE>
DH_HD bool dh_stage_f16(const DhDspParams& P, DhDspShared& S, DH_LANE_ARRAY(dh_f4, (&varr), DH_PF_N), uint32_t have, float& e_out, float& k1_out, float& k2_out) {
    constexpr uint32_t LAST_LANES = DhWindowGroups<NZ>::LAST_LANES, STORE_LANES = DhWindowGroups<NZ>::STORE_LANES;
    DH_LANE_ARRAY(float, xm, 1);
    DH_FOR_LANES_FRESH(lane) {
        const uint32_t l4 = 4u * (uint32_t) lane;
        if (DH_UNLIKELY(have < DH_FTILE + NZ)) {   // the last window of the push: zeros beyond the input
#pragma unroll
            for (int r = 0; r < DH_PF_N; r++) {
                const uint32_t e = l4 + 4u * DH_WAVE * (uint32_t) r;
                DH_LA(varr, lane)[r] = dh_zero_beyond(DH_LA(varr, lane)[r], e, have);
            }
        }
        const float mx = dh_max_abs_groups(DH_LA(varr, lane));
        DH_LA(xm, lane)[0] = mx;
    }
    const float xmax = DH_WAVE_MAX_NAN(xm);
    float scale = 1.0f;
    if (xmax == 0.0f) { e_out = 0.0f; k1_out = P.inv_gain; }                       // all zeros in, all zeros out
    else if (xmax >= DH_BOUND_XMAX_LO && xmax <= DH_BOUND_XMAX_HI) {
        union { float f; uint32_t u; } b; b.f = xmax;
        const uint32_t ex = b.u >> 23;                                              // xmax in [2^(ex - 127), 2^(ex - 126))
        b.u = (253u - ex) << 23; scale = b.f;                                       // 2^(126 - ex)
        b.u = (ex + 1u - (ONE ? 11u : 0u)) << 23; k1_out = P.inv_gain * b.f;        // fl32(1 / gain) 2^(ex - 126) (one chain: 2^-11 of it): exact scaling (ex >= 43)
        e_out = P.err_coef_f16 * xmax;
    } else return false;                                                            // tiny, huge, infinite or NaN samples: outside the bound's assumptions
    k2_out = ONE ? 0.0f : k1_out * 0.00048828125f;                                  // 2^-11
    // (the arrays are as long as the last block's K range reaches: the halves behind the window, under zero taps, must be
    // finite -- the lanes of the last group beyond the window store zeros there)
    DH_FOR_LANES_FRESH(lane) {
        const bool in_last = (uint32_t) lane < LAST_LANES, in_store = (uint32_t) lane < STORE_LANES;
        if (STORE_LANES > LAST_LANES && !in_last) { dh_f4 z; z.x = 0.0f; z.y = 0.0f; z.z = 0.0f; z.w = 0.0f; DH_LA(varr, lane)[DH_PF_N - 1] = z; }
        dh_h4* d1 = reinterpret_cast<dh_h4*>(S.xf) + lane;                          // halves 4 lane .. 4 lane + 3 of group 0; group r is 256 halves on
        dh_h4* d2 = reinterpret_cast<dh_h4*>(S.xf + DH_F16_H2_OFFSET_OF(NZ)) + lane;
#pragma unroll
        for (int r = 0; r < DH_PF_N; r++) {
            dh_h4 a, b;
            if constexpr (ONE) dh_f16_split4_plain(DH_LA(varr, lane)[r], scale, a, b); else dh_f16_split4(DH_LA(varr, lane)[r], scale, a, b);
            if (r < DH_PF_N - 1 || in_store) { dh_h4_store(d1 + DH_WAVE * r, a); dh_h4_store(d2 + DH_WAVE * r, b); }
        }
    }
    return true;
}

// ---- the fetch ahead: the raw window of the NEXT run.  Its start is already known (the timing decision of this
// block only moves symbols 1.. of the next one), the window block is idle from here to the end of the
// iteration, and P4-P6 are latency-bound with few live registers: the HBM latency of these loads hides
// behind them.  Five 16-byte loads per lane, parked in registers until P7.
// (arguments by reference, as the lambda this used to be captured them: by value the PF_REG kernels come out with other registers)
template <int NZ, bool PF_REG>
DH_HD void dh_issue_next_window(DhDspShared& S, const float* const& in, const uint32_t& tc, const uint32_t& p_next, const bool& pf_plain, const bool& pf_reg, DH_LANE_ARRAY(dh_f4, (&pfr), PF_REG ? DH_PF_N : 1)) {
    (void) S; (void) pfr;
    if (DH_LIKELY(pf_reg)) {
        // The split-f16 FIR leaves registers free where the packed-FMA FIR had none: the next window's five 16-byte loads
        // per lane are issued here, straight from HBM, land while P4 - P6 run, and P7 turns them into the two arrays of
        // halves -- the next iteration starts at the matrix cores.
        constexpr uint32_t LAST_LANES = DhWindowGroups<NZ>::LAST_LANES;
        const float* src = in + (p_next - tc);
        DH_FOR_LANES_FRESH(lane) {
            const float* lsrc = src + 4u * (uint32_t) lane;
            const bool in_last = (uint32_t) lane < LAST_LANES;
#pragma unroll
            for (int r = 0; r < DH_PF_N - 1; r++) DH_LA(pfr, lane)[PF_REG ? r : 0] = dh_load4_unaligned(lsrc + 4 * DH_WAVE * r);
            if constexpr (LAST_LANES > 0) DH_LA(pfr, lane)[PF_REG ? DH_PF_N - 1 : 0] = dh_load4_unaligned(lsrc + (in_last ? 4 * DH_WAVE * (DH_PF_N - 1) : 0));
            else (void) in_last;
        }
    } else {
        // Register-free variant: one dword per 128-byte line of the next window is requested now, which pulls the
        // lines into L2; the next iteration's P1 then stages from L2 instead of HBM.  The dwords themselves are not
        // wanted: they are dropped into a part of the window block that is dead until the next staging (dh_l2_touch_lines).
        // They have landed before the next P1 stores anything there (its own, younger loads are waited for first), and
        // an explicit wait follows the loop for the last one.
        if (pf_plain) dh_l2_touch_lines(in + (p_next - tc), DH_FTILE + NZ, S.xf + DH_PF_SINK);
    }
}

#define DH_TAIL_GROUPS 8              // write-back of the raw tail: 16-byte groups per lane and pass (dh_rrc_demod_channel)
#define DH_RING_GROUPS 16             // the sps-10 variance ring (1 000 words) as words per lane: the prologue's loads, all in flight together

// ---------------------------------------------------------------------------------------------
// One channel, one push.  `S` is this wavefront's LDS block.  Called by all 64 lanes (device) or
// once (host harness; the DH_FOR_LANES loops then iterate the lanes).
// SPS = 10 bakes the DMR / YSF samples-per-symbol (and its evaluation window 3..6) into the code so the
// per-symbol loops unroll; SPS = 0 takes them from the parameters.
// part_lo / part_hi / sym_base: the tail split of the chain kernels -- this call takes the samples [part_lo, part_hi) of the
// push and appends its symbols behind the sym_base symbols the earlier parts produced (a part is a push: results do not
// depend on where pushes end).
// LV = 4 / 2: the number of levels is known where the kernel is instantiated (the chain kernels: 4 for DMR / YSF / NXDN, 2 for
// D-Star; dh_plan_chain, launch_plan.hpp, checks P.levels against it) and the other slicer's selects, its invert mask and two scalar register
// pairs drop out of the slicing phase; 0 = taken from P.levels.
// KEEPF (DH_FLAG_KEEP_FILTERED | DH_FLAG_ONE_LAUNCH): the run's filtered samples also leave, from where they stand in LDS -- 1: those of the
// split-f16 product (2.5e-6 of the reference's); 2 (with DH_FLAG_FAST_FIR): the error-bounded kernel filters with the f32 FMA chain instead
// (v_mfma_f32_16x16x4_f32: the arithmetic of DH_FLAG_FAST_FIR, 1e-6 -- BASELINE configs[1] in ONE launch, dibits still the reference's).
template <int NZ, bool FAST, int SPS, int LV = 0, int KEEPF = 0>
DH_HD void dh_rrc_demod_channel(const DhDspParams& P, uint32_t ch, DhDspShared& S, uint32_t part_lo = 0, uint32_t part_hi = 0xFFFFFFFFu, uint32_t sym_base = 0) {
    static_assert(SPS == 0 || SPS == 10 || SPS == 20 || SPS == 40, "0 = run-time samples per symbol; 10 has its own window and timing code, 20 / 40 are the generic code with the constant folded in");
    constexpr bool BOUNDED = DhIsBounded<NZ, FAST, SPS>::value;                      // see "Error-bounded FIR" above
    constexpr bool MF16 = BOUNDED && (NZ == 80 || NZ == 160) && KEEPF != 2;           // its fused FIR as a split-f16 product on the matrix cores
    constexpr bool ONE_CHAIN = dh_f16_one_chain(NZ, KEEPF);                           // ... in the one-chain form (the host built the fragments by the same predicate)
    constexpr bool F16_KEEPS_VOTE = MF16 && NZ == 160;                                // ... still followed by the vote on its outputs: the narrow filter's kernels, for their register allocation's sake (P2)
    DhBoundState* const BS = DH_BOUND_STATE(S);
    float* st = P.state + (size_t) ch * P.state_stride;
    uint32_t* sth = (uint32_t*) st;
    const uint32_t sps = SPS ? (uint32_t) SPS : P.sps;
    const uint32_t ev_lo = SPS == 10 ? 3u : SPS == 20 ? 7u : SPS == 40 ? 13u : P.lo, ev_hi = SPS == 10 ? 7u : SPS == 20 ? 13u : SPS == 40 ? 27u : P.hi;        // (round(sps / 3), round(2 sps / 3): engine_impl.hpp)
    const float sps_rcp = 1.0f / (float) sps;           // correctly rounded (IEEE division, once per push)
    float* tail = st + DH_ST_VAR + DH_VARIANCE_SYMBOLS * sps;
    const float* in = P.in + (size_t) ch * P.in_stride + part_lo;
    uint8_t* syms = P.syms + (size_t) ch * P.sym_stride;
    const float* in_end = P.in + (size_t) (P.n_channels - 1u) * P.in_stride + P.n;    // end of the readable input
    // a whole window (DH_FTILE + NZ samples) from input index i lies inside the readable input iff i < win_lim: the pointer compare
    // in + i + (DH_FTILE + NZ) <= in_end, taken once per push (an index is below n_new <= 2^32 - 1, so the clamp loses nothing)
    const ptrdiff_t in_room = (in_end - in) - (ptrdiff_t) (DH_FTILE + NZ);
    const uint32_t win_lim = dh_uniform(in_room < 0 ? 0u : in_room >= (ptrdiff_t) 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t) in_room + 1u);

    DH_PHASE_MARK_BEGIN();
    // ---- load carried state.  Every global load of the prologue -- header, volume ring, variance ring, taps -- is issued before
    // the first of them is waited for: taken one loop after the other they were nine round trips in a row at the start of every
    // part of a push (the rings of the kernels with a run-time or larger samples-per-symbol keep their loops).
    // (A ragged push adds one full wait: n_per[ch] is wanted as a scalar for the part's bounds, and the wait for it is a wait for
    // everything issued before it.  All of the loads are in flight by then.)
    uint32_t k0 = sth[DH_ST_K];
    int32_t off = (int32_t) sth[DH_ST_OFF];
    const uint32_t tc = sth[DH_ST_TAIL];
    const uint32_t h_p0 = BOUNDED ? sth[DH_ST_P0] : 0u;
    uint32_t h_cur_start = 0, h_cur_off = 0, h_prev_start = 0, h_prev_off = 0, h_blk_flags = 0, h_e_count = 0;
    float h_e_cur = 0.0f, h_e_prev = 0.0f, h_e_block = 0.0f;
    if (BOUNDED) {
        h_cur_start = sth[DH_ST_CUR_START]; h_cur_off = sth[DH_ST_CUR_OFF]; h_prev_start = sth[DH_ST_PREV_START]; h_prev_off = sth[DH_ST_PREV_OFF];
        h_blk_flags = sth[DH_ST_BLOCK_FLAGS]; h_e_count = sth[DH_ST_E_COUNT];
        h_e_cur = st[DH_ST_E_CUR]; h_e_prev = st[DH_ST_E_PREV]; h_e_block = st[DH_ST_E_BLOCK];
    }
    constexpr bool RING_REGS = SPS == 10;               // DH_VARIANCE_SYMBOLS * 10 words: DH_RING_GROUPS per lane
    constexpr bool TAPS_REGS = NZ > 0 && NZ <= 80;      // NZ + 1 + 2 DH_TAP_LEAD words: two per lane
    static_assert(DH_VOLUME_RB_SIZE > DH_WAVE && DH_SCAN_N == 2 * DH_WAVE && DH_VARIANCE_SYMBOLS * 10 <= DH_WAVE * DH_RING_GROUPS && 80 + 1 + 2 * DH_TAP_LEAD <= 2 * DH_WAVE, "words per lane of the prologue's loads");
    DH_LANE_ARRAY(float, vol_v, 2);
    DH_LANE_ARRAY(float, ring_v, RING_REGS ? DH_RING_GROUPS : 1);
    DH_LANE_ARRAY(float, tap_v, 2);
    DH_FOR_LANES(lane) {
        // (a lane beyond the end of a table reads its last word and drops it)
        DH_LA(vol_v, lane)[0] = st[DH_ST_VOL + (uint32_t) lane];
        DH_LA(vol_v, lane)[1] = st[DH_ST_VOL + dh_min<uint32_t>((uint32_t) lane + DH_WAVE, DH_VOLUME_RB_SIZE - 1u)];
        if constexpr (RING_REGS) {
#pragma unroll
            for (int r = 0; r < DH_RING_GROUPS; r++) DH_LA(ring_v, lane)[r] = st[DH_ST_VAR + dh_min<uint32_t>((uint32_t) lane + DH_WAVE * (uint32_t) r, DH_VARIANCE_SYMBOLS * 10u - 1u)];
        }
        if constexpr (TAPS_REGS) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int k = lane + DH_WAVE * i - DH_TAP_LEAD, kc = k < 0 ? 0 : k > NZ ? NZ : k;
                DH_LA(tap_v, lane)[i] = P.taps[kc <= NZ / 2 ? kc : NZ - kc];
            }
        }
    }
    const uint32_t n_push = P.n_per ? dh_min<uint32_t>(dh_uniform(P.n_per[ch]), P.n) : P.n;
    const uint32_t n_new = dh_min<uint32_t>(n_push, part_hi) > part_lo ? dh_min<uint32_t>(n_push, part_hi) - part_lo : 0u;
    const uint32_t nv = tc + n_new;                     // length of the virtual input stream
    const uint32_t nf = nv >= NZ ? nv - NZ : 0u;        // filtered samples available this push
    const uint32_t pf_lim = dh_uniform(dh_min<uint32_t>(win_lim, n_new));        // the next window may be fetched ahead from input indices below this
    DH_FOR_LANES(lane) {
        S.vol_old[lane] = DH_LA(vol_v, lane)[0];
        S.vol_old[lane + DH_WAVE] = (uint32_t) lane + DH_WAVE < DH_VOLUME_RB_SIZE ? DH_LA(vol_v, lane)[1] : 0.0f;
        S.vol_new[lane] = 0.0f; S.vol_new[lane + DH_WAVE] = 0.0f;
        if constexpr (RING_REGS) {
#pragma unroll
            for (int r = 0; r < DH_RING_GROUPS; r++) {
                const uint32_t j = (uint32_t) lane + DH_WAVE * (uint32_t) r;
                if (DH_WAVE * (r + 1) <= DH_VARIANCE_SYMBOLS * 10 || j < DH_VARIANCE_SYMBOLS * 10u) S.var_rb[j] = DH_LA(ring_v, lane)[r];      // (only the last group is partial)
            }
        } else {
            for (uint32_t j = lane; j < DH_VARIANCE_SYMBOLS * sps; j += DH_WAVE) S.var_rb[j] = st[DH_ST_VAR + j];
        }
    }
    DH_BARRIER();

    // FIR taps are parked in LDS and pulled into VGPRs at the start of every FIR pass (see P2): their live range
    // must end with the FIR, or they pin ~80 registers through the latency-bound phases where the prefetch lives.
    // (error radii of the current variance block and of the current / previous >= 100-symbol bucket, the current bucket's symbols, the
    // block flags and the current block's start: wave-uniform, and read and written by every run -- carried in scalar registers across
    // the loop, as k0, off, p and nsym are: read back from LDS they cost every run a ds_read, a wait and a v_readfirstlane each;
    // blk_flags, cur_start and cur_off are also written through to DhBoundState, where the rare paths read them)
    uint32_t blk_flags = 0, e_count = 0; float e_cur = 0.0f, e_prev = 0.0f, e_blk_run = 0.0f;
    int32_t cur_start = 0, cur_off = 0;
    if (BOUNDED) {
        cur_start = (int32_t) dh_uniform(h_cur_start); cur_off = (int32_t) dh_uniform(h_cur_off);
        BS->cur_start = cur_start; BS->cur_off = cur_off;
        BS->prev_start = (int32_t) h_prev_start; BS->prev_off = (int32_t) h_prev_off;
        blk_flags = dh_uniform(h_blk_flags); e_count = dh_uniform(h_e_count);
        e_cur = dh_uniform_f(h_e_cur); e_prev = dh_uniform_f(h_e_prev); e_blk_run = dh_uniform_f(h_e_block);
        BS->blk_flags = blk_flags; BS->n_uncertain = 0; BS->n_exact_runs = 0; BS->n_exact_blocks = 0;
    }
    DH_FOR_LANES(lane) {
        if (NZ > 80) { for (int i = lane; i <= NZ / 2; i += DH_WAVE) S.tapsf[i] = P.taps[i]; }
        else if (NZ > 0) {                              // the whole response between two runs of zeros (see DhDspShared)
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int j = lane + DH_WAVE * i, k = j - DH_TAP_LEAD;
                if (j < NZ + 1 + 2 * DH_TAP_LEAD) S.tapsf[k] = (k >= 0 && k <= NZ) ? DH_LA(tap_v, lane)[i] : 0.0f;
            }
        }
        if (lane < 2) S.stats[lane] = 0;
    }

    // error-bounded mode (see "Error-bounded FIR" above): the tail then starts with DH_ST_P0 samples of HISTORY, so that the
    // raw samples behind every entry of the 100-symbol rings are still at hand when a comparison has to be settled exactly
    uint32_t p = h_p0;                                  // read position in the filtered stream
    uint32_t staged_p = 0xFFFFFFFFu;                    // the LDS window already holds V[staged_p ...) (prefetch); 0xFFFFFFFF: it does not (no run starts there: p < nv)
    // the next window fetched into registers behind P3 and put into the window block in P7: the split-f16 kernels (as two arrays of
    // halves, with the constants of its run below) and the kernels without an RRC stage (as it is: they have the registers, and staged
    // from L2 at the start of the next run every run waited out an L2 round trip: POCSAG slicer 4.86 -> 4.34 ms, D-Star chain 3.94 -> 3.65,
    // r05_a_ab_logs.txt pf1)
    const DhStreamView V = { tail, tc, in, nv, sps_rcp };
    constexpr bool PF_PLAIN = NZ == 0 && !BOUNDED && !KEEPF;
    constexpr bool PF_REG = MF16 || PF_PLAIN;
    float st_e_run = 0.0f, st_k1 = 0.0f, st_k2 = 0.0f;
    uint32_t nsym = sym_base;                           // symbols of this push so far (a later part of a split push starts behind the earlier ones')
    bool overflow = false;
    const uint32_t max_run = (DH_FTILE - 2) / sps;      // symbols whose windows fit one FIR pass
    // (run planning, sps 10: a whole block fits from every position up to fast_p_end while the symbol count is at most fast_sym_end; -1 = never)
    const int32_t fast_p_end = (nf >= 1003u && nf < 0x40000000u) ? (int32_t) (nf - 1003u) : -1;
    const int32_t fast_sym_end = (P.sym_cap >= (uint32_t) DH_VARIANCE_SYMBOLS && P.sym_cap < 0x40000000u) ? (int32_t) (P.sym_cap - DH_VARIANCE_SYMBOLS) : -1;

    DH_PHASE_MARK(7);
    // split-f16 FIR: this lane's six tap fragments -- the same 6 KiB for every wavefront of the chip (L1 / L2 hits).  Requested one
    // iteration ahead (here, and again at the end of every iteration, when the staging registers are free), so they have landed
    // when P2 wants them; every path through P2 leaves them settled (wave_ops.hpp: DH_TAPFRAG_*).
    constexpr int NFRAG = 2 * DH_F16_KSTEPS_OF(NZ > 0 ? NZ : 80);
    DH_TAPFRAG_REGS(tapfrag_regs, NFRAG, P.tapfrag);
    DH_TAPFRAG_LOAD(tapfrag_regs, NFRAG, P.tapfrag, MF16);
    for (;;) {
        // ---- run planning (wave-uniform): symbols k0 .. k0+m-1 of the current variance block.
        // A symbol at filtered position s is produced iff nf - s > sps + 1 (gfsk_demodulator.cpp:18-22);
        // s_0 = p, s_q = p + q*sps + step_off for q >= 1.
        const int32_t step_off = (k0 == 0) ? off : 0;   // applied after the first symbol of a block
        uint32_t m = 0;
        if (SPS == 10 && DH_LIKELY(k0 == 0 && (int32_t) p <= fast_p_end && (int32_t) nsym <= fast_sym_end)) {
            // the usual run: it starts a variance block and holds all of it -- the stream has the samples whatever the pending step
            // is (nf - p >= 1003 >= 1002 + step_off) and the symbol buffer the room: what the general form below comes to, in three
            // compares instead of forty-five scalar instructions and a load of the symbol capacity from the argument block
            m = DH_VARIANCE_SYMBOLS;
        } else {
            uint32_t lim = dh_min<uint32_t>(DH_VARIANCE_SYMBOLS - k0, max_run);
            lim = dh_min<uint32_t>(lim, P.sym_cap - nsym);
            const int64_t room = (int64_t) nf - (int64_t) p - (int64_t) sps - 2;     // >= 0  <=>  symbol 0 fits
            if (DH_LIKELY(nf >= p && nf - p < 0x40000000u)) {
                // (the same in 32 bits -- every push but an absurdly long one: there is no 64-bit scalar compare or divide, the
                // general form below costs two vector compares and twenty scalar instructions per run)
                const int32_t room32 = (int32_t) (nf - p) - (int32_t) sps - 2;
                if (room32 >= 0 && lim > 0) {
                    const int32_t r1 = room32 - step_off;
                    const uint32_t qmax = r1 >= (int32_t) sps ? (uint32_t) r1 / sps : 0u;
                    m = dh_min<uint32_t>(lim, qmax + 1u);
                }
            } else if (room >= 0 && lim > 0) {
                const int64_t r1 = room - step_off;                                   // q*sps <= r1 for q >= 1
                const uint32_t qmax = r1 >= (int64_t) sps ? (uint32_t) (r1 / sps) : 0u;
                m = dh_min<uint32_t>(lim, qmax + 1u);
            }
            if (m == 0) {
                if (lim == 0 && room >= 0) overflow = true;
                break;
            }
        }
        const uint32_t last_start = p + (m - 1) * sps + (m > 1 ? (uint32_t) step_off : 0u);
        const uint32_t need = last_start + sps - p;     // filtered samples [p, p+need) feed this run
        const uint32_t need_fir = KEEPF ? (uint32_t) DH_FTILE : need;      // (a kernel that also delivers the filtered samples wants the whole pass)
        if (BOUNDED && k0 == 0) { cur_start = (int32_t) p; cur_off = step_off; BS->cur_start = cur_start; BS->cur_off = cur_off; blk_flags = (blk_flags & 3u) | 1u; BS->blk_flags = blk_flags; e_blk_run = 0.0f; }   // symbol k of this block sits at cur_start + k sps + (k ? cur_off : 0)
        bool use_exact = BOUNDED && P.exact_mode == 2;  // this run through the exact FIR (odd samples, odd staging path)
        DH_LANE_ARRAY(float, xmax_lane, 1);
        float e_run = 0.0f;                             // error radius of this run's filtered samples (0: exact)
        bool f16_staged = false, xmax_done = false;     // split-f16 FIR: the window block holds the two arrays of halves
        float k1 = 0.0f, k2 = 0.0f;                     // ... and its outputs are fma(second sum, k2, main sum * k1)

        // ---- P1: stage raw samples V[p .. p+need+NZ) into the padded LDS window (zeros beyond)
        // After the first run of a push the whole window comes straight from `in`: 16 B per lane per load,
        // 16 B per LDS store (a group of four never straddles a pad slot: pads sit every 16 elements).
        // From the second run on, the window was already put there by the previous iteration's prefetch (the kernels that fetch it into
        // registers: PF_REG; the others have had it pulled into L2).
        if (DH_LIKELY(staged_p == p)) {
            if (PF_REG && MF16) { f16_staged = true; xmax_done = true; e_run = st_e_run; k1 = st_k1; k2 = st_k2; }      // (put there by P7 of the previous run)
        } else if (p - tc < pf_lim) {                   // (p < nv in every run: its first symbol fits)
            // whole window inside the input buffer: unconditional loads (all in flight together, see the prefetch
            // below for why that matters), samples past the end of the stream zeroed afterwards
            const float* src = in + (p - tc);
            const uint32_t have = dh_min<uint32_t>(DH_FTILE + NZ, nv - p);
            // Per lane ONE global base and ONE LDS base: group r sits 1024 bytes further in memory (immediate offset of
            // the load) and DH_XP(4 lane + 256 r) = DH_XP(4 lane) + 272 r words further in the padded window -- written
            // out, because the compiler otherwise rebuilds every address from the lane id (6 VALU per group).  Only the
            // last group is partial (elements < DH_FTILE + NZ): its lanes beyond the window re-read group 0.
            constexpr uint32_t GSTEP = DhWindowGroups<NZ>::GSTEP, LAST_LANES = DhWindowGroups<NZ>::LAST_LANES;
            DH_LANE_ARRAY(dh_f4, v, DH_PF_N);
            DH_FOR_LANES_FRESH(lane) {
                const uint32_t l4 = 4u * (uint32_t) lane;
                const bool in_last = (uint32_t) lane < LAST_LANES;
                const float* lsrc = src + l4;          // one 64-bit address per lane; the groups are immediate offsets of it
#pragma unroll
                for (int r = 0; r < DH_PF_N - 1; r++) DH_LA(v, lane)[r] = dh_load4_unaligned(lsrc + 4 * DH_WAVE * r);
                if constexpr (LAST_LANES > 0) DH_LA(v, lane)[DH_PF_N - 1] = dh_load4_unaligned(lsrc + (in_last ? 4 * DH_WAVE * (DH_PF_N - 1) : 0));
                else DH_LA(v, lane)[DH_PF_N - 1] = DH_LA(v, lane)[0];
                if (!MF16 || use_exact) {
                    if (have < DH_FTILE + NZ) {        // the last window of the push: zeros beyond the input
#pragma unroll
                        for (int r = 0; r < DH_PF_N; r++) {
                            const uint32_t e = l4 + 4u * DH_WAVE * (uint32_t) r;
                            DH_LA(v, lane)[r] = dh_zero_beyond(DH_LA(v, lane)[r], e, have);
                        }
                    }
                    if (BOUNDED) {                     // max |x| of the window (NaN when a sample is NaN)
                        float mx = 0.0f;
#pragma unroll
                        for (int r = 0; r < DH_PF_N; r++) {
                            const dh_f4 w = DH_LA(v, lane)[r];
                            mx = dh_max3_abs(w.x, w.y, mx); mx = dh_max3_abs(w.z, w.w, mx);
                        }
                        DH_LA(xmax_lane, lane)[0] = mx;
                    }
                }
            }
            if (MF16 && !use_exact) {
                // split-f16 FIR: the window goes to LDS as two arrays of halves (dh_stage_f16)
                xmax_done = true;
                if (dh_stage_f16<NZ, ONE_CHAIN>(P, S, v, have, e_run, k1, k2)) f16_staged = true; else use_exact = true;
            }
            if (!f16_staged) {
                DH_FOR_LANES_FRESH(lane) {
                    const uint32_t l4 = 4u * (uint32_t) lane;
                    const bool in_last = (uint32_t) lane < LAST_LANES;
                    float* ldst = &S.xf[DH_XP(l4)];
                    dh_lds_store4_at<0>(ldst, DH_LA(v, lane)[0]); dh_lds_store4_at<GSTEP>(ldst, DH_LA(v, lane)[1]);
                    dh_lds_store4_at<2 * GSTEP>(ldst, DH_LA(v, lane)[2]); dh_lds_store4_at<3 * GSTEP>(ldst, DH_LA(v, lane)[3]);
                    static_assert(DH_PF_N == 5, "four full groups + a partial one");
                    if constexpr (LAST_LANES > 0) { if (in_last) dh_lds_store4_at<4 * GSTEP>(ldst, DH_LA(v, lane)[4]); }
                    dh_lds_stores_done();
                }
            }
        } else if (MF16 && !use_exact) {
            // The first window of a push (it starts in the carried tail) and the last ones (they end within DH_FTILE + NZ of
            // the input buffer's end): gathered sample by sample, then the same two arrays of halves as everywhere else.  These
            // runs used to go through the reference-order FIR -- one or two of every push, which is most of a push of a few
            // thousand samples (tools/push_size.py).
            const uint32_t have = dh_min<uint32_t>(DH_FTILE + NZ, nv - p);
            DH_LANE_ARRAY(dh_f4, v, DH_PF_N);
            DH_FOR_LANES_FRESH(lane) {
#pragma unroll
                for (int r = 0; r < DH_PF_N; r++) {
                    const uint32_t e = 4u * (uint32_t) lane + 4u * DH_WAVE * (uint32_t) r;
                    dh_f4 w;
                    w.x = e + 0u < have ? dh_virtual_sample(tail, tc, in, p + e + 0u) : 0.0f;
                    w.y = e + 1u < have ? dh_virtual_sample(tail, tc, in, p + e + 1u) : 0.0f;
                    w.z = e + 2u < have ? dh_virtual_sample(tail, tc, in, p + e + 2u) : 0.0f;
                    w.w = e + 3u < have ? dh_virtual_sample(tail, tc, in, p + e + 3u) : 0.0f;
                    DH_LA(v, lane)[r] = w;
                }
            }
            xmax_done = true;
            if (dh_stage_f16<NZ, ONE_CHAIN>(P, S, v, have, e_run, k1, k2)) f16_staged = true;
            else {
                use_exact = true;
                dh_gather_window<NZ>(S, tail, tc, in, nv, p);
            }
        } else if (p >= tc) {
            use_exact = BOUNDED;
            const float* src = in + (p - tc);
            const uint32_t have = dh_min<uint32_t>(DH_FTILE + NZ, nv - p);
            DH_FOR_LANES_FRESH(lane) {
                for (uint32_t e = 4u * (uint32_t) lane; e < DH_FTILE + NZ; e += 4u * DH_WAVE) {
                    dh_f4 v;
                    if (e + 4u <= have) v = dh_load4_unaligned(src + e);
                    else {
                        v.x = e + 0u < have ? src[e + 0u] : 0.0f; v.y = e + 1u < have ? src[e + 1u] : 0.0f;
                        v.z = e + 2u < have ? src[e + 2u] : 0.0f; v.w = e + 3u < have ? src[e + 3u] : 0.0f;
                    }
                    dh_store4(&S.xf[DH_XP(e)], v);
                }
            }
        } else {
            use_exact = BOUNDED;
            dh_gather_window<NZ>(S, tail, tc, in, nv, p);
        }
        DH_BARRIER();
        if (BOUNDED && !use_exact && !xmax_done) {
            const float xmax = DH_WAVE_MAX_NAN(xmax_lane);
            if (xmax == 0.0f) e_run = 0.0f;             // all zeros in, all zeros out of either FIR
            else if (xmax >= DH_BOUND_XMAX_LO && xmax <= DH_BOUND_XMAX_HI) e_run = P.err_coef * xmax;
            else use_exact = true;                      // tiny, huge, infinite or NaN samples: outside the bound's assumptions
        }
        DH_PHASE_MARK(0);

        // ---- P2: FIR into registers, then (after every lane has read its window) back into the window block.
        // The filtered samples go back UNPADDED (element n at word n, four 16-byte stores per lane): the symbol
        // windows of P3 then sit at compile-time offsets from one per-lane base, which saves two address
        // instructions per sample on the VALU; the bank conflicts of the 16-words-apart stores cost LDS cycles
        // only, and the LDS pipe has slack.  Without an RRC stage the staged (padded) samples are used as they are.
        if (NZ > 0 && DH_STOP_AFTER >= 2) {
            DH_LANE_ARRAY(float, fo, DH_FIR_L);
            DH_COMPILER_FENCE();                        // forces the tap loads below to stay inside this pass
            // (taps from the LDS copy into vector registers: as scalar operands they free 40 VGPRs but cost this kernel 5 %,
            // see DhFirBatch)
            constexpr bool MFMA = NZ > 0 && NZ <= 80 && (BOUNDED || FAST) && !MF16;      // the fused FIR as f32 MFMAs (dh_fir_mfma)
            int mf_layout = 0;                          // fo[] holds a matrix-core output layout: 1 = DH_MF_OUT, 2 = DH_F16_OUT
            if (BOUNDED) {
                uint64_t vote_bad = 0;
                if (DH_LIKELY(!use_exact)) {
                    if constexpr (MF16) {
                        // (f16_staged holds: every staging path that does not fill the two arrays of halves sets use_exact)
                        // Nothing looks at the outputs: staging has seen max |x| of exactly these samples, NaN included, and lets only
                        // finite windows of at most 1e15 through (dh_stage_f16), which cannot overflow in here.
                        // (The narrow filter's kernels keep the vote behind the FIR they had -- sixteen v_fma and a ballot: without it
                        // the NXDN chain kernel came out with a scratch load on the run loop's hot path, tools/asm_census.py.)
                        DH_FOR_LANES_FRESH(lane) {
                            dh_fir_f16<MF16 ? NZ : 80, ONE_CHAIN>(S.xf, tapfrag_regs, lane, k1, k2, DH_LA(fo, lane));
                            if constexpr (F16_KEEPS_VOTE) {
                                float t = 0.0f;
#pragma unroll
                                for (int j = 0; j < DH_FIR_L; j++) t = __builtin_fmaf(DH_LA(fo, lane)[j], 0.0f, t);       // NaN or infinity anywhere: 0 * y is NaN
                                DH_BALLOT_ACC(vote_bad, !(t == 0.0f), lane);
                            }
                        }
                        mf_layout = 2;
                    } else if constexpr (MFMA) {
                        DH_FOR_LANES_FRESH(lane) {
                            bool bad = false;
                            float acc[DH_FIR_L];
                            dh_fir_mfma<MFMA ? NZ : 80>(S.tapsf, S.xf, lane, acc);
                            dh_fir_finish<true>(acc, P.gain, P.rgain, P.inv_gain, DH_LA(fo, lane), &bad);
                            DH_BALLOT_ACC(vote_bad, bad, lane);
                        }
                        mf_layout = 1;
                    } else static_assert(!BOUNDED, "every error-bounded kernel filters on the matrix cores (launch_plan.hpp instantiates none without MF16 or MFMA)");
                }
                if (DH_UNLIKELY(use_exact || vote_bad)) {            // samples outside the bound's range, a NaN / infinity among them: the reference's arithmetic decides
                    use_exact = true; e_run = 0.0f; BS->n_exact_runs++; mf_layout = 0;
                    if (MF16 && f16_staged) {           // the window block holds halves: the reference's FIR wants the raw samples back
                        DH_BARRIER();
                        dh_gather_window<NZ>(S, tail, tc, in, nv, p);
                        DH_BARRIER();
                    }
                    dh_exact_fir_pass<NZ>(P, S, need_fir, fo);
                }
            } else if constexpr (MFMA) {
                DH_FOR_LANES_FRESH(lane) {
                    float acc[DH_FIR_L];
                    dh_fir_mfma<MFMA ? NZ : 80>(S.tapsf, S.xf, lane, acc);
                    dh_fir_finish<true>(acc, P.gain, P.rgain, P.inv_gain, DH_LA(fo, lane), nullptr);
                }
                mf_layout = 1;
            } else {
                float tv[NZ / 2 + 1];
#pragma unroll
                for (int i = 0; i <= NZ / 2; i++) tv[i] = S.tapsf[i];
                DH_FOR_LANES_FRESH(lane) {
                    if ((uint32_t) (lane * DH_FIR_L) < need_fir)
                        dh_fir_lane<NZ, FAST>(tv, P.gain, P.rgain, P.inv_gain, S.xf, lane, DH_LA(fo, lane));
                }
            }
            DH_BARRIER();
            if (MF16 && mf_layout == 2) {
                DH_FOR_LANES_FRESH(lane) {
                    float* dst = S.xf + DH_F16_OUT(0, 0, lane >> 4, lane & 15);
#pragma unroll
                    for (int T = 0; T < 4; T++)
#pragma unroll
                        for (int r = 0; r < 4; r++) dst[DH_F16_OUT(T, r, 0, 0)] = DH_LA(fo, lane)[4 * T + r];
                }
            } else if (MFMA && mf_layout == 1) {
                // sample DH_MF_OUT(T, r, g, n) of the run from register 4 T + r of lane 16 g + n: compile-time offsets
                DH_FOR_LANES_FRESH(lane) {
                    float* dst = S.xf + DH_MF_OUT(0, 0, lane >> 4, lane & 15);
#pragma unroll
                    for (int T = 0; T < 4; T++)
#pragma unroll
                        for (int r = 0; r < 4; r++) dst[DH_MF_OUT(T, r, 0, 0)] = DH_LA(fo, lane)[4 * T + r];
                }
            } else {
                DH_FOR_LANES_FRESH(lane) {
                    if ((uint32_t) (lane * DH_FIR_L) < need_fir) DH_STORE_FIR_OUT(S.xf, lane, fo);
                }
            }
            DH_BARRIER();
        }
        DH_TAPFRAG_SETTLE(tapfrag_regs, NFRAG, MF16);
        DH_PHASE_MARK(1);
        const float* fbuf = S.xf;

        // ---- the raw window of the NEXT run: planned here, fetched behind P3 (dh_issue_next_window), stored in P7 (dh_store_next_window)
        const uint32_t p_next = last_start + sps + ((k0 == 0 && m == 1) ? (uint32_t) step_off : 0u);
        const uint32_t pf_have = dh_min<uint32_t>(DH_FTILE + NZ, nv - p_next);        // (read in P7, under pf_reg only: p_next < nv there)
        DH_LANE_ARRAY(dh_f4, pfr, PF_REG ? DH_PF_N : 1);  // split-f16 kernels: the next window, parked in registers through P4 - P6
        // Only when the whole window lies inside the input buffer (every run but the last ones of the last
        // channel): the loads are then unconditional, there is nothing to merge, and all five are in flight
        // together; samples past pf_have are zeroed in P7.  Otherwise the next iteration stages in P1.
        // (tc <= p_next < nv and the window inside the input, as one unsigned compare: p_next - tc wraps past every n_new when p_next < tc)
        const bool pf_plain = p_next - tc < pf_lim;
        const bool pf_reg = PF_REG && pf_plain && P.exact_mode != 2;
        if constexpr (KEEPF) {
            // This run's filtered samples [p, p_next) leave as they stand in LDS (each store instruction a run of 64 consecutive
            // words); what the previous push already delivered -- positions in front of tc - NZ, the first new sample's -- is
            // skipped, and nothing is delivered beyond the last complete output.
            const uint32_t f_lo = tc > (uint32_t) NZ ? tc - (uint32_t) NZ : 0u;
            const uint32_t s0 = p < f_lo ? f_lo - p : 0u;
            const uint32_t s1 = dh_min<uint32_t>(p_next - p, nf > p ? nf - p : 0u);
            float* orow = P.filt_out + (size_t) ch * P.filt_stride + ((ptrdiff_t) p + (ptrdiff_t) NZ - (ptrdiff_t) tc);
            DH_FOR_LANES_FRESH(lane) {
                for (uint32_t e = s0 + (uint32_t) lane; e < s1; e += DH_WAVE) orow[e] = fbuf[e];
            }
        }

        DH_COMPILER_FENCE();                            // what the slicing phases read from LDS is read here, not hoisted across the FIR (the run's own bookkeeping is in scalar registers, see above)
        float e_blk = 0.0f;
        if (BOUNDED) { e_blk = dh_uniform_f(__builtin_fmaxf(e_blk_run, e_run)); e_blk_run = e_blk; }
        const float e_eff = BOUNDED ? dh_uniform_f(__builtin_fmaxf(e_run, __builtin_fmaxf(e_cur, e_prev))) : 0.0f;
        const float T = DH_BOUND_T_FACTOR * e_eff;
        uint64_t vote_a = 0, vote_b = 0;                // doubtful symbols of the run: bit l of vote_a = symbol 2 l, of vote_b = symbol 2 l + 1
        // Straight-line per half of the run (m <= 100 symbols: lanes 0..63, then 0..35): every lane computes, a predicate
        // guards the store -- written as a loop over the lane's symbols this compiled to a real loop with exec-mask
        // bookkeeping (half of this phase's instructions were scalar).  The wave-uniform choices (4 / 2 levels, invert,
        // exact_mode) are selects, not branches.
        const bool four_levels = LV ? LV == 4 : P.levels == 4;
        // (DH_FLAG_EXACT_SYMBOLS -- every symbol decided exactly -- is an infinite threshold, not another mask)
        const bool force_doubt = BOUNDED && P.exact_mode == 1;
        const bool e_pos = e_eff > 0.0f || force_doubt;
        const float T_eff = force_doubt ? __builtin_inff() : T;
        const float inv_width = 1.0f / (float) (ev_hi - ev_lo);                       // (a power of two for sps 10: the product below is the division)
        const bool width_pow2 = ((ev_hi - ev_lo) & (ev_hi - ev_lo - 1u)) == 0u;
        const bool pair_store = ((uint32_t) (uintptr_t) syms + nsym) % 2u == 0u;      // (paired slicing phases: symbols 2 l, 2 l + 1 of the run as one 16-bit store)

        // ---- P3: symbol windows (gfsk_demodulator.cpp:28-35, 82-83): dh_symbol_windows
        // (sps 10: one grid first -- behind the KEEPF copy above, which delivers the samples where the FIR put them)
        DH_LANE_STRUCT(DhWinPair, win) = {};
        if (SPS == 10 && DH_STOP_AFTER >= 3 && DH_UNLIKELY(step_off != 0)) dh_shift_symbol0(S.xf, step_off);
        dh_symbol_windows<SPS>(S, fbuf, k0, m, step_off, sps, ev_lo, ev_hi, sps_rcp, win);
        // (sps 10: no drain here.  The block is one wavefront's, and a wavefront's LDS instructions complete in the order it issued them:
        // what the scan below loads -- on a run with k0 != 0 the volumes other lanes stored -- was stored by older instructions, and
        // the window words it stores S.mn / S.mx over have arrived in every lane's registers, dh_lds_run waits for them.  The
        // scan's vector work runs while the window phase's twelve stores drain; the barrier behind the scan waits for both.)
        if (SPS != 10) DH_BARRIER();
        DH_PHASE_MARK(2);

        dh_issue_next_window<NZ, PF_REG>(S, in, tc, p_next, pf_plain, pf_reg, pfr);

        // ---- P4: sliding AGC min/max as two wave scans
        DH_LANE_STRUCT(DhAgcPair, agc) = {};
        if (DH_STOP_AFTER >= 4) dh_agc_scan<SPS == 10>(S, k0, k0 + m, agc, win, SPS == 10 && k0 == 0u);
        // (sps 10, as above: on a run that opens its block the slicing phase takes extremes and sums from registers and loads nothing;
        // on the others its loads of S.mn / S.mx / S.sum are younger than the stores.  Whoever next reads what these phases stored -- the
        // timing decision, P7 -- waits for its own loads, which return behind them.)
        if (SPS != 10) DH_BARRIER();
        DH_PHASE_MARK(3);

        // ---- P5: thresholds + slice (gfsk_demodulator.cpp:88-106 / fsk_demodulator.cpp:89-99): dh_slice_symbols; what it leaves in doubt: dh_settle_doubts
        if (DH_STOP_AFTER >= 5) {
            const DhSliceSetup U = { four_levels, e_pos, width_pow2, pair_store, T_eff, inv_width };
            dh_slice_symbols<SPS, LV, BOUNDED>(P, S, agc, win, syms + nsym, k0, m, ev_lo, ev_hi, U, vote_a, vote_b);
        }
        if (BOUNDED && DH_UNLIKELY((vote_a | vote_b) != 0)) {
            dh_settle_doubts<NZ>(P, S, BS, V, syms + nsym, k0, e_eff, sps, ev_lo, ev_hi, vote_a, vote_b);
        }

        DH_PHASE_MARK(4);
        // ---- P6: end of a variance block -> timing decision (gfsk_demodulator.cpp:41-80): dh_timing_decision
        int32_t new_off = 0;
        const bool block_done = (k0 + m == DH_VARIANCE_SYMBOLS);
        if (block_done && DH_STOP_AFTER >= 6) {
            new_off = dh_timing_decision<NZ, SPS, BOUNDED>(P, S, BS, V, sps, k0, e_blk);
        }

        DH_PHASE_MARK(5);
        // ---- P7: commit the run (wave-uniform bookkeeping) and fold new volumes into the ring
        DH_FOR_LANES_FRESH(lane) {
            // a run has at most 100 symbols: two copies per lane, both loads in flight together (as a loop this was two trips of
            // exec-mask bookkeeping with a wait in each).  A lane beyond the run copies the run's first slot again -- the value lane 0
            // writes there -- so the stores need no predicate: no exec-mask region, no skip branch.
            const uint32_t ka = k0 + (uint32_t) lane, kb = ka + DH_WAVE, ke = k0 + m;
            const uint32_t ia = ka < ke ? ka : k0, ib = kb < ke ? kb : k0;
            const float va_ = S.vol_new[ia], vb_ = S.vol_new[ib];
            S.vol_old[ia] = va_;
            S.vol_old[ib] = vb_;
        }
        staged_p = 0xFFFFFFFFu;
        if (DH_LIKELY(pf_reg)) {
            if constexpr (PF_REG && MF16) { if (DH_LIKELY((dh_stage_f16<NZ, ONE_CHAIN>(P, S, pfr, pf_have, st_e_run, st_k1, st_k2)))) staged_p = p_next; }
            else if constexpr (PF_PLAIN) {
                // no RRC stage: the window is the 1 024 samples themselves (four groups of four per lane, unpadded), zeros beyond the stream's end
                static_assert(!PF_PLAIN || (DH_FTILE == 4u * DH_WAVE * (DH_PF_N - 1)), "four full groups cover the window");
                DH_FOR_LANES_FRESH(lane) {
                    const uint32_t l4 = 4u * (uint32_t) lane;
                    float* ldst = &S.xf[l4];
#pragma unroll
                    for (int r = 0; r < DH_PF_N - 1; r++) {
                        dh_f4 w = DH_LA(pfr, lane)[PF_REG ? r : 0];
                        if (DH_UNLIKELY(pf_have < DH_FTILE)) w = dh_zero_beyond(w, l4 + 4u * DH_WAVE * (uint32_t) r, pf_have);
                        dh_store4(ldst + 4 * DH_WAVE * r, w);
                    }
                }
                staged_p = p_next;
            }
        }
        DH_BARRIER();
        p = p_next;
        nsym += m;
        if (k0 == 0) off = 0;                           // the pending step has been consumed (:36-38)
        k0 += m;
        if (block_done) { k0 = 0; off = new_off; }
        if (BOUNDED) {
            // radii of the ring entries: the last 100 symbols always lie inside the current bucket + the one before it
            const float ec = dh_uniform_f(__builtin_fmaxf(e_cur, e_run));
            const uint32_t cnt = e_count + m;
            if (cnt >= DH_VOLUME_RB_SIZE) { e_prev = ec; e_cur = 0.0f; e_count = 0; }
            else { e_cur = ec; e_count = cnt; }
            if (block_done) { BS->prev_start = cur_start; BS->prev_off = cur_off; blk_flags = (blk_flags & 1u) ? 2u : 0u; BS->blk_flags = blk_flags; }
        }
        DH_TAPFRAG_LOAD(tapfrag_regs, NFRAG, P.tapfrag, MF16);      // for the next run
        DH_PHASE_MARK(6);
    }

    dh_global_loads_done();                             // a last L2-touch load may still be writing into the window block
    if constexpr (KEEPF) {
        // the outputs behind the last run (less than a symbol's worth, unless the symbol buffer is full): the reference's arithmetic,
        // sample by sample, while the tail it reads is still the old one
        const uint32_t f_lo = tc > (uint32_t) NZ ? tc - (uint32_t) NZ : 0u;
        float* orow = P.filt_out + (size_t) ch * P.filt_stride;
        DH_FOR_LANES(lane) {
            for (uint32_t f = dh_max<uint32_t>(p, f_lo) + (uint32_t) lane; f < nf; f += DH_WAVE)
                orow[f + (uint32_t) NZ - tc] = dh_exact_filtered<NZ>(tail, tc, in, nv, S.tapsf, P.gain, P.rgain, (int32_t) f);
        }
    }
    // ---- write back state: rings, header, and the raw tail V[base .. nv): the unread samples (from p) and, in the
    // error-bounded kernels, up to dh_history(sps) samples behind them
    const uint32_t tail_max = dh_tail_max(sps);
    const uint32_t keep = BOUNDED ? dh_min<uint32_t>(dh_history(sps), p) : 0u;
    const uint32_t base = p - keep;
    const uint32_t new_tc = nv - base;                 // = history + unread filtered samples + NZ
    DH_FOR_LANES(lane) {
        for (uint32_t j = lane; j < DH_VOLUME_RB_SIZE; j += DH_WAVE) st[DH_ST_VOL + j] = S.vol_old[j];
        for (uint32_t j = lane; j < DH_VARIANCE_SYMBOLS * sps; j += DH_WAVE) st[DH_ST_VAR + j] = S.var_rb[j];
    }
    const uint32_t tail_n = new_tc < tail_max ? new_tc : tail_max;
    if (base >= tc && tail_n >= 4u) {
        // Every push longer than a tail: the new tail lies in the input row, which nothing writes.  Whole 16-byte groups, the
        // loads of a pass (DH_TAIL_GROUPS per lane, 2 048 samples) unconditional and all in flight before the first store --
        // element by element through LDS (below) every pair of loads was waited for, eleven round trips to L2 in a row at the
        // end of every part.  The last group is the last four samples, wherever they start: it may overlap the one before
        // it (the same values twice); a lane beyond the tail loads that group once more and stores nothing.
        const float* src = in + (base - tc);
        for (uint32_t c0 = 0; c0 < tail_n; c0 += 4u * DH_WAVE * DH_TAIL_GROUPS) {
            DH_LANE_ARRAY(dh_f4, tv, DH_TAIL_GROUPS);
            DH_FOR_LANES(lane) {
#pragma unroll
                for (int r = 0; r < DH_TAIL_GROUPS; r++) {
                    const uint32_t e = c0 + 4u * ((uint32_t) lane + DH_WAVE * (uint32_t) r);
                    DH_LA(tv, lane)[r] = dh_load4_unaligned(src + dh_min<uint32_t>(e, tail_n - 4u));
                }
            }
            dh_global_loads_done();
            DH_FOR_LANES(lane) {
#pragma unroll
                for (int r = 0; r < DH_TAIL_GROUPS; r++) {
                    const uint32_t e = c0 + 4u * ((uint32_t) lane + DH_WAVE * (uint32_t) r);
                    if (e < tail_n) dh_store4_unaligned(tail + dh_min<uint32_t>(e, tail_n - 4u), DH_LA(tv, lane)[r]);
                }
            }
        }
    }
    // otherwise the tail overlaps its own source: in chunks through LDS (a chunk is read completely before any of
    // it is written, and later chunks only read further ahead)
    else for (uint32_t c0 = 0; c0 < new_tc && c0 < tail_max; c0 += DH_FTILE) {
        DH_BARRIER();
        DH_FOR_LANES(lane) {
            for (uint32_t j = c0 + lane; j < new_tc && j < tail_max && j < c0 + DH_FTILE; j += DH_WAVE) S.xf[j - c0] = dh_virtual_sample(tail, tc, in, base + j);
        }
        DH_BARRIER();
        DH_FOR_LANES(lane) {
            for (uint32_t j = c0 + lane; j < new_tc && j < tail_max && j < c0 + DH_FTILE; j += DH_WAVE) tail[j] = S.xf[j - c0];
        }
    }
    DH_FOR_LANES(lane) {
        if (DH_IS_LANE0(lane)) {
            // (timing blocks completed by this call: the symbol counter of the block wraps at 100 exactly when one ends -- counted here,
            // from the counter as the call found it, not with a read-modify-write of LDS by one lane in every run)
            // (sym_base is not kept through the loop: a later part finds it where it read it, until P.sym_count is stored below)
            // (the counters below are read again here and written back, not carried through the loop in registers: the compiler issues
            // these loads together and stores the header as dwordx4 -- one more batch of loads per part)
            const uint32_t produced = nsym - (part_lo ? P.sym_count[ch] : 0u);
            sth[DH_ST_BLOCKS] += (sth[DH_ST_K] + produced) / DH_VARIANCE_SYMBOLS;
            sth[DH_ST_K] = k0;
            sth[DH_ST_OFF] = (uint32_t) off;
            sth[DH_ST_TAIL] = new_tc < tail_max ? new_tc : tail_max;
            sth[DH_ST_NSYM] += produced;
            if (BOUNDED) {
                sth[DH_ST_P0] = keep;
                sth[DH_ST_CUR_START] = (uint32_t) (cur_start - (int32_t) base); sth[DH_ST_CUR_OFF] = (uint32_t) cur_off;
                sth[DH_ST_PREV_START] = (uint32_t) (BS->prev_start - (int32_t) base); sth[DH_ST_PREV_OFF] = (uint32_t) BS->prev_off;
                sth[DH_ST_BLOCK_FLAGS] = blk_flags; sth[DH_ST_E_COUNT] = e_count;
                st[DH_ST_E_CUR] = e_cur; st[DH_ST_E_PREV] = e_prev; st[DH_ST_E_BLOCK] = e_blk_run;
                sth[DH_ST_UNCERTAIN] += BS->n_uncertain; sth[DH_ST_EXACT_RUNS] += BS->n_exact_runs; sth[DH_ST_EXACT_BLOCKS] += BS->n_exact_blocks;
            }

            sth[DH_ST_ORDERED] += S.stats[1];
            P.sym_count[ch] = nsym;
            if ((overflow || new_tc > tail_max) && P.overflow) *P.overflow = 1u;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Stand-alone RRC stage (materialised output, BASELINE config 2): one 1024-sample tile of one
// channel per wavefront.  `hist` holds the last NZ inputs of the previous push ([B][NZ]).
struct DhRrcParams {
    const float* in; size_t in_stride;
    float* out; size_t out_stride;
    const float* hist;                                  // [B][nz] previous inputs (zeros after reset)
    const uint32_t* n_per;                              // ragged pushes: [B] samples of each channel (<= n), or null
    uint32_t n, n_channels, nz;
    int32_t fast;
    double gain, rgain; float inv_gain;
    float taps[DH_MAX_NZ / 2 + 1];
};

template <int NZ, bool FAST>
DH_HD void dh_rrc_tile(const DhRrcParams& R, uint32_t ch, uint32_t tile, DhDspShared& S) {
    const float* in = R.in + (size_t) ch * R.in_stride;
    const float* hist = R.hist + (size_t) ch * NZ;
    float* out = R.out + (size_t) ch * R.out_stride;
    const uint32_t t0 = tile * DH_FTILE;
    const uint32_t n_ch = R.n_per ? dh_min<uint32_t>(dh_uniform(R.n_per[ch]), R.n) : R.n;
    if (t0 >= n_ch) return;                             // (ragged pushes: the grid covers the longest row)
    const uint32_t cnt = dh_min<uint32_t>(DH_FTILE, n_ch - t0);
    // virtual stream = hist (NZ samples) ++ in; output t needs virtual [t, t+NZ]
    if (t0 >= (uint32_t) NZ) {
        // every tile but the first reads `in` only: 16 bytes per lane per load
        const float* src = in + (t0 - NZ);
        const uint32_t have = cnt + NZ;
        if (have >= DH_FTILE + NZ) {
            // a full tile: the loads are issued unconditionally (clamped addresses) so that all of them are in flight
            // together -- under a branch each would be waited for before the next starts
            constexpr int NV = (DH_FTILE + NZ + 4 * DH_WAVE - 1) / (4 * DH_WAVE);
            DH_FOR_LANES(lane) {
                dh_f4 v[NV];
#pragma unroll
                for (int r = 0; r < NV; r++) {
                    const uint32_t e = 4u * (uint32_t) lane + 4u * DH_WAVE * (uint32_t) r;
                    v[r] = dh_load4_unaligned(src + dh_min<uint32_t>(e, DH_FTILE + NZ - 4u));
                }
#pragma unroll
                for (int r = 0; r < NV; r++) {
                    const uint32_t e = 4u * (uint32_t) lane + 4u * DH_WAVE * (uint32_t) r;
                    if (e < DH_FTILE + NZ) dh_store4(&S.xf[DH_XPAD(e)], v[r]);
                }
            }
        } else {
            DH_FOR_LANES(lane) {
                for (uint32_t e = 4u * (uint32_t) lane; e < DH_FTILE + NZ; e += 4u * DH_WAVE) {
                    dh_f4 v; v.x = 0.0f; v.y = 0.0f; v.z = 0.0f; v.w = 0.0f;
                    if (e + 4u <= have) v = dh_load4_unaligned(src + e);
                    else if (e < have) {
                        v.x = src[e];
                        if (e + 1u < have) v.y = src[e + 1u];
                        if (e + 2u < have) v.z = src[e + 2u];
                    }
                    dh_store4(&S.xf[DH_XPAD(e)], v);
                }
            }
        }
    } else {
        DH_FOR_LANES(lane) {
            for (uint32_t e = lane; e < DH_FTILE + NZ; e += DH_WAVE) {
                const uint32_t v = t0 + e;
                float x = 0.0f;
                if (e < cnt + NZ) x = v < (uint32_t) NZ ? hist[v] : in[v - NZ];
                S.xf[DH_XPAD(e)] = x;
            }
        }
    }
    DH_BARRIER();
    DH_COMPILER_FENCE();                                // the taps become live after the staging registers are dead
    // (the taps straight from the parameter block: the GPU reads R.taps as scalar pairs, DhFirBatch SG)
    // Each lane produces 16 consecutive outputs.  Stored straight from registers, one store instruction would touch
    // 64 separate 64-byte pieces of the row; instead the tile goes through the (now idle) window block and leaves
    // as four fully coalesced 1 KB stores.
    DH_LANE_ARRAY(float, fo, DH_FIR_L);
    DH_FOR_LANES(lane) {
        if ((uint32_t) lane * DH_FIR_L < cnt) dh_fir_lane<NZ, FAST, true>(R.taps, R.gain, R.rgain, R.inv_gain, S.xf, lane, DH_LA(fo, lane));
    }
    DH_BARRIER();                                       // every lane has read its window
    DH_FOR_LANES(lane) {
        if ((uint32_t) lane * DH_FIR_L < cnt) DH_STORE_FIR_OUT(S.xf, lane, fo);
    }
    DH_BARRIER();
    DH_FOR_LANES(lane) {
        float* dst = out + t0;
#pragma unroll
        for (int r = 0; r < DH_FTILE / (4 * DH_WAVE); r++) {
            const uint32_t e = 4u * (uint32_t) lane + 4u * DH_WAVE * (uint32_t) r;
            const dh_f4a v = *reinterpret_cast<const dh_f4a*>(S.xf + e);
            if (e + 4u <= cnt) { dh_f4 w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; dh_store4_unaligned(dst + e, w); }
            else {
                if (e + 0u < cnt) dst[e + 0u] = v.x;
                if (e + 1u < cnt) dst[e + 1u] = v.y;
                if (e + 2u < cnt) dst[e + 2u] = v.z;
            }
        }
    }
    DH_BARRIER();
}
