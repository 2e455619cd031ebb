// seam_probe_core.hpp -- the probe kernel of the device / CPU seam (dh_portable.hpp, "THE SEAM"): every primitive of the layer,
// and every whole-function pair a test can drive alone, called ONCE, by itself, on operands the caller chooses -- with exactly the
// template arguments the kernels instantiate.  tests/test_seam_primitives.py runs it on the device and on the CPU tier and holds
// both to a plain reference that is neither form.  Not part of any path; include/digiham_amd.h (dh_debug_seam_probe) has the ops
// and their word layouts.
//
// One workgroup = one wavefront = one case: blockIdx.x selects it, its input words are in + case * in_words(op), its output
// words out + case * out_words(op).  The first DH_PROBE_HDR input words are the case's header (wave-uniform operands), then
// come the lanes' words, word i of lane l at [DH_PROBE_HDR + 64 i + l]; results likewise, word i of lane l at [64 i + l].
#pragma once

#include "../../include/digiham_amd.h"
#include "dsp_core.hpp"

#define DH_PROBE_HDR 4u
#define DH_PROBE_LDS_WORDS 5632u                        // the LDS block of the movers: 22 KiB
#define DH_PROBE_BASE_MAX 1720u                         // largest base (in words) a mover takes: the furthest reach is base + 3900 + 1 (dh_lds_store_row10<3000>)
#define DH_PROBE_RAMP 0x3F000000u                       // the block before a mover runs: word i holds the bits RAMP + seed + i
#define DH_PROBE_MARK 0x4B000000u                       // what a lane stores: its j-th value is MARK + 64 lane + j

struct DhProbeShape { uint32_t in_words, out_words; };
// (lane words in, lane words out) of an op; false for an op that does not exist
inline bool dh_probe_shape(int op, DhProbeShape& s) {
    uint32_t in = 0, out = 0, flat_out = 0;
    switch (op) {
    case DH_PROBE_VMIN: case DH_PROBE_VMAX: in = 2; out = 1; break;
    case DH_PROBE_MIN3_ABS: case DH_PROBE_MAX3_ABS: in = 3; out = 1; break;
    case DH_PROBE_MAX_ABS_GROUPS5: in = 20; out = 1; break;
    case DH_PROBE_MUL_UNIFORM: case DH_PROBE_SQRT_UPPER: in = 1; out = 1; break;
    case DH_PROBE_DIV_CONST2: in = 2; out = 2; break;
    case DH_PROBE_F2_MAC: case DH_PROBE_F2_MAC_FAST: in = 5; out = 2; break;
    case DH_PROBE_F2_MAC_PAIR_LO: case DH_PROBE_F2_MAC_PAIR_HI: case DH_PROBE_F2_MAC_PAIR_FAST_LO: case DH_PROBE_F2_MAC_PAIR_FAST_HI: in = 4; out = 2; break;
    case DH_PROBE_F2_FMA: in = 6; out = 2; break;
    case DH_PROBE_F2_SCALE: in = 3; out = 2; break;
    case DH_PROBE_F16_SPLIT4_PLAIN: in = 4; out = 4; break;
    case DH_PROBE_WAVE_MAX: case DH_PROBE_WAVE_MAX_NAN: case DH_PROBE_WAVE_MIN: case DH_PROBE_ROW0_MIN: in = 1; flat_out = 1; break;
    case DH_PROBE_ROW_SUM5_PAIR: in = 2; out = 2; break;
    case DH_PROBE_AGC_SCAN: case DH_PROBE_AGC_SCAN_PAIRS: in = 4 + 6; out = 4 + 4; break;
    case DH_PROBE_LDS_RUN20: in = 1; out = 20; break;
    case DH_PROBE_LDS_RUN40: in = 1; out = 40; break;
    case DH_PROBE_LDS_RUN20_WITH_PAIR: in = 2; out = 22; break;
    case DH_PROBE_LDS_PAIRS3_NOW: in = 3; out = 6; break;
    case DH_PROBE_LDS_READS: in = 2; out = 6; break;
    case DH_PROBE_LDS_STORE4_AT: case DH_PROBE_LDS_STORE4_AT_PLAIN: case DH_PROBE_LDS_STORE_ROW10_0: case DH_PROBE_LDS_STORE_ROW10_1000:
    case DH_PROBE_LDS_STORE_ROW10_2000: case DH_PROBE_LDS_STORE_ROW10_3000: case DH_PROBE_LDS_STORE_PAIR: case DH_PROBE_LDS_STORE_ROWS10_PAIR:
        in = 1; flat_out = DH_PROBE_LDS_WORDS; break;
    case DH_PROBE_LV_READ: in = 1; out = 1; break;
    case DH_PROBE_LV_DOWN: in = 1; out = 4; break;
    case DH_PROBE_LS_WRITE_READ: in = 4; out = 5; break;
    case DH_PROBE_LS_GATHER: in = 3; out = 1; break;
    case DH_PROBE_LANES_BELOW: in = 0; out = 1; break;
    case DH_PROBE_STATE: in = 2; out = 3; break;
    case DH_PROBE_BITS: in = 2; out = 5; break;
    default: return false;
    }
    s.in_words = DH_PROBE_HDR + DH_WAVE * in; s.out_words = flat_out ? flat_out : DH_WAVE * out;
    return true;
}

DH_HD float dh_probe_f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
DH_HD uint32_t dh_probe_u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// dh_f2_mac_pair exists on the device only (where the tap comes from, not what is computed): its restatement is dh_f2_mac with the
// half of the pair that HALF names
#if DH_ON_GPU
template <bool FAST, int HALF> __device__ __forceinline__ dh_f2 dh_probe_mac_pair(dh_f2 cc, dh_f2 w, dh_f2 acc) { return dh_f2_mac_pair<FAST, HALF>(cc, w, acc); }
#else
template <bool FAST, int HALF> inline dh_f2 dh_probe_mac_pair(dh_f2 cc, dh_f2 w, dh_f2 acc) { return dh_f2_mac<FAST>(HALF ? cc.y : cc.x, w, acc); }
#endif
// the raw LDS reads likewise (dh_agc_scan's rare path and the slicing phase use them directly): two words at dword offsets 0 and 1
// of p as one ds_read2_b32, the same two as one ds_read_b64 (p 8-byte aligned) and as two ds_read_b32, settled by their own waits
#if DH_ON_GPU
__device__ __forceinline__ void dh_probe_lds_reads(const float* p, const float* p8, dh_f2& two, dh_f2& wide, float& a, float& b) {
    two = dh_lds_read2<0, 1>(dh_lds_addr(p));
    wide = dh_lds_read_b64<0>(dh_lds_addr(p8));
    a = dh_lds_read_b32<0>(dh_lds_addr(p)); b = dh_lds_read_b32<4>(dh_lds_addr(p));
    dh_lds_reads_done(a, b);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(two), "+v"(wide) :: "memory");
}
#else
inline void dh_probe_lds_reads(const float* p, const float* p8, dh_f2& two, dh_f2& wide, float& a, float& b) {
    two = dh_f2_make(p[0], p[1]); wide = dh_f2_make(p8[0], p8[1]); a = p[0]; b = p[1];
}
#endif

// ---------------------------------------------------------------------------------------------------------- lane-wise floats
DH_HD void dh_probe_lanewise(int op, const uint32_t* in, uint32_t* out) {
    const float h0 = dh_probe_f(dh_uniform(in[0])), h1 = dh_probe_f(dh_uniform(in[1]));      // the case's wave-uniform operands
    const dh_f2 hh = dh_f2_make(h0, h1);
    DH_FOR_LANES(lane) {
        const uint32_t* a = in + DH_PROBE_HDR + lane;
        uint32_t* r = out + lane;
#define DH_PA(i) dh_probe_f(a[DH_WAVE * (i)])
#define DH_PR(i, v) r[DH_WAVE * (i)] = dh_probe_u(v)
#define DH_PR2(v) do { const dh_f2 v_ = (v); DH_PR(0, v_.x); DH_PR(1, v_.y); } while (0)
        switch (op) {
        case DH_PROBE_VMIN: DH_PR(0, dh_vmin(DH_PA(0), DH_PA(1))); break;
        case DH_PROBE_VMAX: DH_PR(0, dh_vmax(DH_PA(0), DH_PA(1))); break;
        case DH_PROBE_MIN3_ABS: DH_PR(0, dh_min3_abs(DH_PA(0), DH_PA(1), DH_PA(2))); break;
        case DH_PROBE_MAX3_ABS: DH_PR(0, dh_max3_abs(DH_PA(0), DH_PA(1), DH_PA(2))); break;
        case DH_PROBE_MAX_ABS_GROUPS5: {
            dh_f4 w[5];
            for (int g = 0; g < 5; g++) { w[g].x = DH_PA(4 * g); w[g].y = DH_PA(4 * g + 1); w[g].z = DH_PA(4 * g + 2); w[g].w = DH_PA(4 * g + 3); }
            DH_PR(0, dh_max_abs_groups(w));
            break;
        }
        case DH_PROBE_MUL_UNIFORM: DH_PR(0, dh_mul_uniform(h0, DH_PA(0))); break;
        case DH_PROBE_SQRT_UPPER: DH_PR(0, dh_sqrt_upper(DH_PA(0))); break;
        case DH_PROBE_DIV_CONST2: DH_PR2(dh_div_const2(dh_f2_make(DH_PA(0), DH_PA(1)), h0, h1)); break;            // h0 = d, h1 = RN(1 / d)
        case DH_PROBE_F2_MAC: DH_PR2(dh_f2_mac<false>(DH_PA(0), dh_f2_make(DH_PA(1), DH_PA(2)), dh_f2_make(DH_PA(3), DH_PA(4)))); break;
        case DH_PROBE_F2_MAC_FAST: DH_PR2(dh_f2_mac<true>(DH_PA(0), dh_f2_make(DH_PA(1), DH_PA(2)), dh_f2_make(DH_PA(3), DH_PA(4)))); break;
        case DH_PROBE_F2_MAC_PAIR_LO: DH_PR2((dh_probe_mac_pair<false, 0>(hh, dh_f2_make(DH_PA(0), DH_PA(1)), dh_f2_make(DH_PA(2), DH_PA(3))))); break;
        case DH_PROBE_F2_MAC_PAIR_HI: DH_PR2((dh_probe_mac_pair<false, 1>(hh, dh_f2_make(DH_PA(0), DH_PA(1)), dh_f2_make(DH_PA(2), DH_PA(3))))); break;
        case DH_PROBE_F2_MAC_PAIR_FAST_LO: DH_PR2((dh_probe_mac_pair<true, 0>(hh, dh_f2_make(DH_PA(0), DH_PA(1)), dh_f2_make(DH_PA(2), DH_PA(3))))); break;
        case DH_PROBE_F2_MAC_PAIR_FAST_HI: DH_PR2((dh_probe_mac_pair<true, 1>(hh, dh_f2_make(DH_PA(0), DH_PA(1)), dh_f2_make(DH_PA(2), DH_PA(3))))); break;
        case DH_PROBE_F2_FMA: DH_PR2(dh_f2_fma(dh_f2_make(DH_PA(0), DH_PA(1)), dh_f2_make(DH_PA(2), DH_PA(3)), dh_f2_make(DH_PA(4), DH_PA(5)))); break;
        case DH_PROBE_F2_SCALE: DH_PR2(dh_f2_scale(dh_f2_make(DH_PA(0), DH_PA(1)), DH_PA(2))); break;
        case DH_PROBE_F16_SPLIT4_PLAIN: {
            dh_f4 v; v.x = DH_PA(0); v.y = DH_PA(1); v.z = DH_PA(2); v.w = DH_PA(3);
            dh_h4 p, q;
            dh_f16_split4_plain(v, h0, p, q);
            uint32_t t[4];
            __builtin_memcpy(t, &p, 8); __builtin_memcpy(t + 2, &q, 8);      // the four halves as the kernels store them (one 8-byte vector each)
            for (int i = 0; i < 4; i++) r[DH_WAVE * i] = t[i];
            break;
        }
        default: break;
        }
#undef DH_PA
#undef DH_PR
#undef DH_PR2
    }
}

// ------------------------------------------------------------------------------------------- wave reductions and the row sums
DH_HD void dh_probe_reduce(int op, const uint32_t* in, uint32_t* out) {
    DH_LANE_ARRAY(float, a, 1); DH_LANE_ARRAY(float, b, 1);
    DH_FOR_LANES(lane) {
        DH_LA(a, lane)[0] = dh_probe_f(in[DH_PROBE_HDR + lane]);
        DH_LA(b, lane)[0] = op == DH_PROBE_ROW_SUM5_PAIR ? dh_probe_f(in[DH_PROBE_HDR + DH_WAVE + lane]) : 0.0f;
    }
    if (op == DH_PROBE_ROW_SUM5_PAIR) {
        dh_row_sum5_pair(a, b);
        DH_FOR_LANES(lane) { out[lane] = dh_probe_u(DH_LA(a, lane)[0]); out[DH_WAVE + lane] = dh_probe_u(DH_LA(b, lane)[0]); }
        return;
    }
    const float r = op == DH_PROBE_WAVE_MAX ? DH_WAVE_MAX(a) : op == DH_PROBE_WAVE_MAX_NAN ? DH_WAVE_MAX_NAN(a) : op == DH_PROBE_WAVE_MIN ? DH_WAVE_MIN(a) : DH_ROW0_MIN(a);
    if (dh_is_writer_lane()) out[0] = dh_probe_u(r);
}

// ------------------------------------------------------------------------------------------------------------ the AGC scan
// header: k0, k1, from_win.  Lane words 0 .. 3: vol_old[l], vol_old[64 + l], vol_new[l], vol_new[64 + l]; 4 .. 9: the lane's DhWinPair.
// Out, lane words 0 .. 3: S.mn[l], S.mn[64 + l], S.mx[l], S.mx[64 + l] (a slot the scan did not write: 0xA5A5A5A5); 4 .. 7: the DhAgcPair.
DH_HD void dh_probe_agc(int op, const uint32_t* in, uint32_t* out, float* lds) {
    DhDspShared S = {};
    S.vol_old = lds; S.vol_new = lds + DH_SCAN_N; S.mn = lds + 2 * DH_SCAN_N; S.mx = lds + 3 * DH_SCAN_N;
    const uint32_t k1 = dh_min(dh_uniform(in[1]), (uint32_t) DH_VOLUME_RB_SIZE), k0 = dh_min(dh_uniform(in[0]), k1);
    const bool from_win = op == DH_PROBE_AGC_SCAN_PAIRS && k0 == 0u && dh_uniform(in[2]) != 0u;
    DH_LANE_STRUCT(DhWinPair, win) = {};
    DH_LANE_STRUCT(DhAgcPair, agc) = {};
    DH_FOR_LANES(lane) {
        const uint32_t* a = in + DH_PROBE_HDR + lane;
        for (int i = 0; i < 4; i++) { lds[DH_WAVE * i + lane] = dh_probe_f(a[DH_WAVE * i]); lds[2 * DH_SCAN_N + DH_WAVE * i + lane] = dh_probe_f(0xA5A5A5A5u); }
        DH_LS(win, lane) = DhWinPair{ dh_probe_f(a[DH_WAVE * 4]), dh_probe_f(a[DH_WAVE * 5]), dh_probe_f(a[DH_WAVE * 6]), dh_probe_f(a[DH_WAVE * 7]),
                                      dh_probe_f(a[DH_WAVE * 8]), dh_probe_f(a[DH_WAVE * 9]) };
    }
    DH_BARRIER();
    if (k0 < k1) {
        if (op == DH_PROBE_AGC_SCAN) dh_agc_scan<false>(S, k0, k1, agc, win, false);
        else dh_agc_scan<true>(S, k0, k1, agc, win, from_win);
    }
    DH_BARRIER();
    DH_FOR_LANES(lane) {
        uint32_t* r = out + lane;
        for (int i = 0; i < 4; i++) r[DH_WAVE * i] = dh_probe_u(lds[2 * DH_SCAN_N + DH_WAVE * i + lane]);
        const DhAgcPair& p = DH_LS(agc, lane);
        r[DH_WAVE * 4] = dh_probe_u(p.mn0); r[DH_WAVE * 5] = dh_probe_u(p.mx0); r[DH_WAVE * 6] = dh_probe_u(p.mn1); r[DH_WAVE * 7] = dh_probe_u(p.mx1);
    }
}

// ---------------------------------------------------------------------------------------------------------- the LDS movers
// header word 0: the ramp's seed.  Lane word 0: the lane's base, in words from the start of the block (clamped to
// DH_PROBE_BASE_MAX); word 1 (run20_with_pair): where the pair is (made even); words 1, 2 (pairs3_now): the other two bases.
// Loads: out = the lane's registers in order.  Stores: out = the whole block afterwards.
DH_HD void dh_probe_lds(int op, const uint32_t* in, uint32_t* out, float* lds) {
    const uint32_t seed = dh_uniform(in[0]) & 0xFFFFu;
    DH_FOR_LANES(lane) { for (uint32_t i = lane; i < DH_PROBE_LDS_WORDS; i += DH_WAVE) lds[i] = dh_probe_f(DH_PROBE_RAMP + seed + i); }
    DH_BARRIER();
    const bool stores = op >= DH_PROBE_LDS_STORE4_AT;
    DH_FOR_LANES(lane) {
        const uint32_t* a = in + DH_PROBE_HDR + lane;
        uint32_t* r = out + lane;
        float* base = lds + dh_min(a[0], DH_PROBE_BASE_MAX);
        float m[20];                                            // what a store writes
        for (int j = 0; j < 20; j++) m[j] = dh_probe_f(DH_PROBE_MARK + (uint32_t) (DH_WAVE * lane + j));
        switch (op) {
        case DH_PROBE_LDS_RUN20: { float v[20]; dh_lds_run<20>(base, v); for (int i = 0; i < 20; i++) r[DH_WAVE * i] = dh_probe_u(v[i]); break; }
        case DH_PROBE_LDS_RUN40: { float v[40]; dh_lds_run<40>(base, v); for (int i = 0; i < 40; i++) r[DH_WAVE * i] = dh_probe_u(v[i]); break; }
        case DH_PROBE_LDS_RUN20_WITH_PAIR: {
            float v[20], p0, p1;
            dh_lds_run20_with_pair(base, v, lds + (dh_min(a[DH_WAVE], DH_PROBE_BASE_MAX) & ~1u), p0, p1);
            for (int i = 0; i < 20; i++) r[DH_WAVE * i] = dh_probe_u(v[i]);
            r[DH_WAVE * 20] = dh_probe_u(p0); r[DH_WAVE * 21] = dh_probe_u(p1);
            break;
        }
        case DH_PROBE_LDS_PAIRS3_NOW: {
            dh_f2 x, y, z;
            dh_lds_pairs3_now(base, lds + dh_min(a[DH_WAVE], DH_PROBE_BASE_MAX), lds + dh_min(a[2 * DH_WAVE], DH_PROBE_BASE_MAX), x, y, z);
            r[0] = dh_probe_u(x.x); r[DH_WAVE] = dh_probe_u(x.y); r[DH_WAVE * 2] = dh_probe_u(y.x); r[DH_WAVE * 3] = dh_probe_u(y.y);
            r[DH_WAVE * 4] = dh_probe_u(z.x); r[DH_WAVE * 5] = dh_probe_u(z.y);
            break;
        }
        case DH_PROBE_LDS_READS: {
            dh_f2 two, wide; float x, y;
            dh_probe_lds_reads(base, lds + (dh_min(a[DH_WAVE], DH_PROBE_BASE_MAX) & ~1u), two, wide, x, y);
            r[0] = dh_probe_u(two.x); r[DH_WAVE] = dh_probe_u(two.y); r[DH_WAVE * 2] = dh_probe_u(wide.x); r[DH_WAVE * 3] = dh_probe_u(wide.y);
            r[DH_WAVE * 4] = dh_probe_u(x); r[DH_WAVE * 5] = dh_probe_u(y);
            break;
        }
        case DH_PROBE_LDS_STORE4_AT: case DH_PROBE_LDS_STORE4_AT_PLAIN: {            // the five groups of a lane's window, as dh_window_to_lds stores them
            dh_f4 g[5];
            for (int i = 0; i < 5; i++) { g[i].x = m[4 * i]; g[i].y = m[4 * i + 1]; g[i].z = m[4 * i + 2]; g[i].w = m[4 * i + 3]; }
            if (op == DH_PROBE_LDS_STORE4_AT) {
                constexpr uint32_t G = DhWindowGroups<80>::GSTEP;
                dh_lds_store4_at<0>(base, g[0]); dh_lds_store4_at<G>(base, g[1]); dh_lds_store4_at<2 * G>(base, g[2]); dh_lds_store4_at<3 * G>(base, g[3]); dh_lds_store4_at<4 * G>(base, g[4]);
            } else {
                constexpr uint32_t G = DhWindowGroups<0>::GSTEP;
                dh_lds_store4_at<0>(base, g[0]); dh_lds_store4_at<G>(base, g[1]); dh_lds_store4_at<2 * G>(base, g[2]); dh_lds_store4_at<3 * G>(base, g[3]); dh_lds_store4_at<4 * G>(base, g[4]);
            }
            break;
        }
        case DH_PROBE_LDS_STORE_ROW10_0: dh_lds_store_row10<0>(base, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9]); break;
        case DH_PROBE_LDS_STORE_ROW10_1000: dh_lds_store_row10<1000>(base, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9]); break;
        case DH_PROBE_LDS_STORE_ROW10_2000: dh_lds_store_row10<2000>(base, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9]); break;
        case DH_PROBE_LDS_STORE_ROW10_3000: dh_lds_store_row10<3000>(base, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9]); break;
        case DH_PROBE_LDS_STORE_PAIR: dh_lds_store_pair(base, m[0], m[1]); break;
        case DH_PROBE_LDS_STORE_ROWS10_PAIR: {
            float x[10], y[10];
            for (int i = 0; i < 10; i++) { x[i] = m[i]; y[i] = m[10 + i]; }
            dh_lds_store_rows10_pair(base, x, y);
            break;
        }
        default: break;
        }
    }
    if (!stores) return;
    dh_lds_stores_done();
    DH_BARRIER();
    DH_FOR_LANES(lane) { for (uint32_t i = lane; i < DH_PROBE_LDS_WORDS; i += DH_WAVE) out[i] = dh_probe_u(lds[i]); }
}

// ------------------------------------------------------------------------------------- the lane vocabulary of dh_portable.hpp
struct DhProbePair { uint32_t a, b; };
// m0 around a DH_LS_WRITE, whose device form routes the lane select through it and must hand it back as it was (m0 belongs to
// the compiler): dh_probe_m0_swap(st, v) puts v there and returns what it held -- once in front of the write with a value of the
// probe's, once behind it with the compiler's own.  The register operand ties each swap to the write between them.  (The CPU
// build has no m0: a word that nothing but the swaps touches.)
#if DH_ON_GPU
__device__ __forceinline__ uint32_t dh_probe_m0_swap(DhProbePair& st, uint32_t v) {
    uint32_t old;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2" : "=&s"(old), "+v"(st.a) : "s"(v));
    return old;
}
#else
inline uint32_t dh_probe_m0_swap(DhProbePair*, uint32_t v) { static thread_local uint32_t m0 = 0; const uint32_t old = m0; m0 = v; return old; }
#endif
DH_HD void dh_probe_lanes(int op, const uint32_t* in, uint32_t* out) {
    const uint32_t h0 = dh_uniform(in[0]), h1 = dh_uniform(in[1]);
    DH_LANE_VALUE(uint32_t, v);
    DH_LANE_STRUCT(DhProbePair, st);
    DH_FOR_LANES(lane) {
        DH_LV(v, lane) = op == DH_PROBE_LANES_BELOW ? 0u : in[DH_PROBE_HDR + lane];
        DH_LS(st, lane) = op == DH_PROBE_LS_WRITE_READ || op == DH_PROBE_LS_GATHER ? DhProbePair{ in[DH_PROBE_HDR + DH_WAVE + lane], in[DH_PROBE_HDR + 2 * DH_WAVE + lane] } : DhProbePair{ 0u, 0u };
    }
    switch (op) {
    case DH_PROBE_LV_READ:
        for (uint32_t k = 0; k < DH_WAVE; k++) { const uint32_t x = DH_LV_READ(v, k); if (dh_is_writer_lane()) out[k] = x; }
        break;
    case DH_PROBE_LV_DOWN:
        DH_FOR_LANES(lane) {
            out[lane] = DH_LV_DOWN(v, lane, 0); out[DH_WAVE + lane] = DH_LV_DOWN(v, lane, 1);
            out[2 * DH_WAVE + lane] = DH_LV_DOWN(v, lane, 5); out[3 * DH_WAVE + lane] = DH_LV_DOWN(v, lane, 63);
        }
        break;
    case DH_PROBE_LS_WRITE_READ:
        // lane words: v, st.a, st.b, and the value written to st.a of lane k in word 3 of lane k.  Out, lane words: st.a afterwards; what
        // DH_LS_READ(st, a, k) gave right after the write (word k); what DH_LV_READ(v, 63 - k) gave right behind the write; st.b, untouched;
        // what m0 held behind the write (word k), having held 0x00A50000 + k in front of it
        for (uint32_t k = 0; k < DH_WAVE; k++) {
            const uint32_t val = dh_uniform(in[DH_PROBE_HDR + 3 * DH_WAVE + k]);
            const uint32_t keep = dh_probe_m0_swap(st, 0x00A50000u + k);
            DH_LS_WRITE(st, a, k, val);
            const uint32_t m0_seen = dh_probe_m0_swap(st, keep);
            const uint32_t y = DH_LV_READ(v, 63u - k), x = DH_LS_READ(st, a, k);
            if (dh_is_writer_lane()) { out[DH_WAVE + k] = x; out[2 * DH_WAVE + k] = y; out[4 * DH_WAVE + k] = m0_seen; }
        }
        DH_FOR_LANES(lane) { out[lane] = DH_LS(st, lane).a; out[3 * DH_WAVE + lane] = DH_LS(st, lane).b; }
        break;
    case DH_PROBE_LS_GATHER:
        DH_FOR_LANES(lane) { out[lane] = DH_LS_GATHER(st, a, DH_LS(st, lane).b & 63u); }
        break;
    case DH_PROBE_LANES_BELOW: {
        const uint64_t mask = (uint64_t) h0 | (uint64_t) h1 << 32;
        DH_FOR_LANES(lane) { out[lane] = DH_LANES_BELOW(mask, lane); }
        break;
    }
    default: break;
    }
}
// DhState.  header: first, n of store_words.  Lane word 0: the state; word 1, lanes 0 .. 15: eight (index, value) pairs to set.
// Out, lane word 0: get(k) for every k; word 1: store() after the sets; word 2: store_words(first, n) (the rest: untouched)
DH_HD void dh_probe_state(const uint32_t* in, uint32_t* out) {
    const uint32_t first = dh_uniform(in[0]) & 63u, n = dh_min(dh_uniform(in[1]), DH_WAVE - first);
    DhState s;
    s.load(in + DH_PROBE_HDR);
    for (uint32_t k = 0; k < DH_WAVE; k++) { const uint32_t x = s.get(k); if (dh_is_writer_lane()) out[k] = x; }
    for (uint32_t i = 0; i < 8; i++) {
        const uint32_t at = dh_uniform(in[DH_PROBE_HDR + DH_WAVE + 2 * i]) & 63u, val = dh_uniform(in[DH_PROBE_HDR + DH_WAVE + 2 * i + 1]);
        if (i & 1u) s[at] = val; else s.set(at, val);
    }
    s.store(out + DH_WAVE);
    s.store_words(out + 2 * DH_WAVE, first, n);
}
DH_HD void dh_probe_bits(const uint32_t* in, uint32_t* out) {
    DH_FOR_LANES(lane) {
        const uint32_t lo = in[DH_PROBE_HDR + lane], hi = in[DH_PROBE_HDR + DH_WAVE + lane];
        const uint64_t x = (uint64_t) lo | (uint64_t) hi << 32;
        out[lane] = dh_brev32(lo);
        out[DH_WAVE + lane] = x ? (uint32_t) dh_ffs64(x) : ~0u;
        out[2 * DH_WAVE + lane] = x ? (uint32_t) dh_top64(x) : ~0u;
        out[3 * DH_WAVE + lane] = (uint32_t) dh_popc32(lo);
        out[4 * DH_WAVE + lane] = (uint32_t) dh_popc64(x);
    }
}

DH_HD void dh_seam_probe_case(int op, const uint32_t* in, uint32_t* out, float* lds) {
    if (op <= DH_PROBE_F16_SPLIT4_PLAIN) dh_probe_lanewise(op, in, out);
    else if (op <= DH_PROBE_ROW_SUM5_PAIR) dh_probe_reduce(op, in, out);
    else if (op <= DH_PROBE_AGC_SCAN_PAIRS) dh_probe_agc(op, in, out, lds);
    else if (op <= DH_PROBE_LDS_STORE_ROWS10_PAIR) dh_probe_lds(op, in, out, lds);
    else if (op <= DH_PROBE_LANES_BELOW) dh_probe_lanes(op, in, out);
    else if (op == DH_PROBE_STATE) dh_probe_state(in, out);
    else dh_probe_bits(in, out);
}

// ---------------------------------------------------------------------------------------------------------------- the launch
namespace {

__global__ __launch_bounds__(DH_WAVE) void k_seam_probe(int op, const uint32_t* in, uint32_t* out, uint32_t in_words, uint32_t out_words) {
    __shared__ dh_f4a lds[DH_PROBE_LDS_WORDS / 4];
    dh_seam_probe_case(op, in + (size_t) blockIdx.x * in_words, out + (size_t) blockIdx.x * out_words, reinterpret_cast<float*>(lds));
}

}  // namespace

static int dh_be_seam_probe(int op, const uint32_t* in, uint32_t* out, size_t cases, void* stream) {
    DhProbeShape s;
    if (!dh_probe_shape(op, s) || cases > 0x7FFFFFFFu) return DH_EINVAL;
    if (!cases) return DH_OK;
    return dh_launch(k_seam_probe, dim3((unsigned) cases), dh_workgroup(DH_WAVE), 0, stream, "k_seam_probe", op, in, out, s.in_words, s.out_words) ? DH_EDEVICE : DH_OK;
}
