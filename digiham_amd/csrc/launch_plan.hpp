// launch_plan.hpp -- which template instantiation serves which configuration: the one statement of the routing.
//
// Both backends (HipBackend in engine.hip, the lane-loop HostBackend of tests/host_harness) go through these ladders; each
// passes a callable that runs ONE instantiation, called as go(Tag{}) and returning the backend's status.  Nothing here
// launches, allocates or emulates anything.  Also here, once: the protocol switch behind a slicer and the host-side
// arithmetic of the tail split (grammar of DH_TAIL_SPLIT, parameters of a split launch; the parts themselves and the chain
// workgroup: chain_core.hpp, which this header brings with it, at its end).  When to split is each backend's own policy.
// tests/host_cpp/plan_test.cpp holds the routes as a literal table: a route changed here is changed there, on purpose.
#pragma once

#include <stdlib.h>

#include "dsp_core.hpp"
#include "decoder_core.hpp"

// the template arguments of one instantiation (k_rrc_demod / k_chain / k_rrc_tile and the harness's loops over the same bodies)
template <int NZ_, bool FAST_, int SPS_, int KEEPF_ = 0> struct DhDemodInst {
    static constexpr int NZ = NZ_, SPS = SPS_, KEEPF = KEEPF_; static constexpr bool FAST = FAST_;
};
template <int NZ_, bool FAST_, int PROTO_, int SPS_ = 10, bool MAY_SPLIT_ = false> struct DhChainInst {
    static constexpr int NZ = NZ_, PROTO = PROTO_, SPS = SPS_; static constexpr bool FAST = FAST_, MAY_SPLIT = MAY_SPLIT_;
    static constexpr int LV = PROTO_ == DH_PROTO_DSTAR ? 2 : 4;         // the chain kernels' slicer knows its pipe's levels (dh_rrc_demod_channel)
};
template <int NZ_, bool FAST_> struct DhTilesInst { static constexpr int NZ = NZ_; static constexpr bool FAST = FAST_; };

template <class Go> int dh_plan_rrc_demod(const DhDspParams& P, uint32_t nz, bool fast, Go&& go) {
    // (engine_impl.hpp: only this pipe asks for it; `fast` here = the floats of the f32 FMA chain, dsp_core.hpp KEEPF = 2)
    if (P.filt_out) return (P.sps == 10 && nz == 80) ? (fast ? go(DhDemodInst<80, false, 10, 2>{}) : go(DhDemodInst<80, false, 10, 1>{})) : -1;
    if (P.sps == 10) {                      // DMR / YSF: specialised symbol loops
        if (nz == 0) return go(DhDemodInst<0, false, 10>{});
        if (nz == 80) return fast ? go(DhDemodInst<80, true, 10>{}) : go(DhDemodInst<80, false, 10>{});
    }
    if (nz == 0 && P.sps == 40) return go(DhDemodInst<0, false, 40>{});       // fsk_demodulator -s 40 (POCSAG): the generic code with the constant folded in
    if (nz == 160 && P.sps == 20 && !fast) return go(DhDemodInst<160, false, 20>{});      // rrc_filter -n | gfsk_demodulator -s 20 (NXDN48)
    if (nz == 0) return go(DhDemodInst<0, false, 0>{});
    if (nz == 80) return fast ? go(DhDemodInst<80, true, 0>{}) : go(DhDemodInst<80, false, 0>{});
    if (nz == 160) return fast ? go(DhDemodInst<160, true, 0>{}) : go(DhDemodInst<160, false, 0>{});
    return -1;
}

// 1 = not available for this configuration (the caller launches the two stages separately), otherwise what go returned
template <class Go> int dh_plan_chain(const DhDspParams& P, uint32_t nz, bool fast, int proto, Go&& go) {
    if (P.levels != (proto == DH_PROTO_DSTAR ? 2 : 4)) return 1;        // the chain kernels are built for their pipe's slicer (DhChainInst::LV); anything else runs as two launches
    if (proto == DH_PROTO_NXDN && nz == 160 && !fast && P.sps == 20) return go(DhChainInst<160, false, DH_PROTO_NXDN, 20, true>{});   // rrc_filter -n | gfsk_demodulator -s 20 | nxdn_decoder
    if (proto == DH_PROTO_NXDN && nz == 160 && !fast) return go(DhChainInst<160, false, DH_PROTO_NXDN, 0, true>{});    // (any other samples-per-symbol)
    // (POCSAG stays on two launches: measured 9.5 ms chained against 8.9 ms split at 16 384 channels)
    if (P.sps != 10) return 1;
    if (proto == DH_PROTO_DSTAR && nz == 0) return go(DhChainInst<0, false, DH_PROTO_DSTAR, 10, true>{});    // fsk_demodulator -s 10 | dstar_decoder
    if ((nz != 0 && nz != 80) || (proto != DH_PROTO_DMR && proto != DH_PROTO_YSF)) return 1;
    const bool dmr = proto == DH_PROTO_DMR;
    if (nz == 0) return dmr ? go(DhChainInst<0, false, DH_PROTO_DMR>{}) : go(DhChainInst<0, false, DH_PROTO_YSF>{});
    if (fast) return dmr ? go(DhChainInst<80, true, DH_PROTO_DMR>{}) : go(DhChainInst<80, true, DH_PROTO_YSF>{});
    return dmr ? go(DhChainInst<80, false, DH_PROTO_DMR, 10, true>{}) : go(DhChainInst<80, false, DH_PROTO_YSF, 10, true>{});     // the headline pipes
}

template <class Go> int dh_plan_rrc_tiles(uint32_t nz, bool fast, Go&& go) {
    if (nz == 80) return fast ? go(DhTilesInst<80, true>{}) : go(DhTilesInst<80, false>{});
    if (nz == 160) return fast ? go(DhTilesInst<160, true>{}) : go(DhTilesInst<160, false>{});
    return -1;
}

// The decoder of one channel; sym_base / append are the tail split's (POCSAG and the protocol scan are never chained and take neither).
// dh_chain_workgroup (chain_core.hpp) calls it with its PROTO template constant, so the switch folds.
DH_HD void dh_decode_channel(int proto, const DhDecParams& D, uint32_t ch, DhDecShared& S, uint32_t sym_base = 0, bool append = false) {
    if (proto == DH_PROTO_DMR) dh_dmr_channel(D, ch, S, sym_base, append);
    else if (proto == DH_PROTO_DSTAR) dh_dstar_channel(D, ch, S, sym_base, append);
    else if (proto == DH_PROTO_NXDN) dh_nxdn_channel(D, ch, S, sym_base, append);
    else if (proto == DH_PROTO_POCSAG) dh_pocsag_channel(D, ch, S);
    else if (proto == DH_PROTO_SCAN) dh_scan_channel(D, ch, S);
    else dh_ysf_channel(D, ch, S, sym_base, append);
}

// ---- tail split (chain_core.hpp): how a push is cut and launched
// DH_TAIL_SPLIT = "80" or "75,93": percent of a push where the second / third part of a channel starts, "0" = off.
// DH_TAIL_SPLIT_FORCE_FAIL = k (tests): see DhDspParams::split_force_fail.
struct DhTailSplitEnv { bool set; uint32_t pct, pct2, force_fail; };
inline DhTailSplitEnv dh_tail_split_env() {
    DhTailSplitEnv E = { false, 0u, 0u, 0u };
    if (const char* e = getenv("DH_TAIL_SPLIT_FORCE_FAIL")) E.force_fail = (uint32_t) strtoul(e, nullptr, 10);
    if (const char* e = getenv("DH_TAIL_SPLIT")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10), w = end && *end == ',' ? strtol(end + 1, nullptr, 10) : 0;
        E.set = true;
        E.pct = v > 0 && v < 100 ? (uint32_t) v : 0u;
        E.pct2 = E.pct && w > v && w < 100 ? (uint32_t) w : 0u;
    }
    return E;
}
// DhDspParams::split_n0 / split_n1 of a push of n samples (split_n1 = 0: two parts)
inline void dh_tail_split_points(uint32_t n, uint32_t pct, uint32_t pct2, uint32_t& n0, uint32_t& n1) {
    n0 = (uint32_t) ((uint64_t) n * pct / 100u);
    n1 = pct2 > pct ? (uint32_t) ((uint64_t) n * pct2 / 100u) : 0u;
}
// The parameters of a split launch of Q's push, stated once for both backends (when to split is theirs): the parts' bounds
// (a first part of at least one sample, a third that does not start in front of the second: nothing to clamp at the device's
// thresholds), the pad between the parts of the grid -- a multiple of 8, so that the workgroups of a channel land on one XCD --
// and the next epoch of the engine's counter.  Returns the grid of the split launch and of the fix-up launch behind it
// (the same Q with split_fixup = 1).
inline uint32_t dh_next_epoch(uint32_t e) { return (e % 0x00FFFFFEu) + 1u; }         // 24 bits, never 0
struct DhSplitGrids { uint32_t split, fixup; };
inline DhSplitGrids dh_plan_split(DhDspParams& Q, uint32_t pct, uint32_t pct2, uint32_t& epoch, uint32_t force_fail) {
    dh_tail_split_points(Q.n, pct, pct2, Q.split_n0, Q.split_n1);
    if (Q.split_n0 < 1u) Q.split_n0 = 1u;
    if (pct2 > pct && Q.split_n1 < Q.split_n0) Q.split_n1 = Q.split_n0;
    Q.split_pad = (Q.n_channels + 7u) & ~7u;
    Q.part_epoch = epoch = dh_next_epoch(epoch);
    Q.split_fixup = 0u;
    Q.split_force_fail = force_fail;
    return { (Q.split_n1 ? 2u : 1u) * Q.split_pad + Q.n_channels, Q.n_channels };
}

// The chain workgroup the chain routes launch, and the parts of a split push (dh_part_lo / dh_part_hi, the flag word): whoever
// has the plan has them.  At the end: chain_core.hpp uses DhChainInst and dh_decode_channel above (either header may come first).
#include "chain_core.hpp"
