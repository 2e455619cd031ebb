// chain_core.hpp -- the chain workgroup: one channel's slicer, then its decoder, and the hand-over of the tail split.
//
// One text for k_chain (engine.hip) and the CPU wave emulation (tests/host_harness), which calls dh_chain_workgroup for the
// blocks of the planned grids in ascending order -- the order the hand-over rests on.
//
// Tail split (when and how far: each backend's policy; the launch's parameters: dh_plan_split, launch_plan.hpp): two (or
// three) workgroups per channel.  Workgroup c takes the first split_n0 samples of channel c's push, workgroup split_pad + c
// the rest (up to split_n1, where workgroup 2 split_pad + c takes over), each starting from the state the one before wrote
// back -- a part is a push, and results do not depend on where pushes end.  Workgroups are dispatched in index order, so every
// first part is on the machine (most have long finished) before any second part is; the short later parts are what the launch
// drains with.  Hand-over: the workgroups of a channel run on the same XCD (workgroup i goes to XCD i mod 8, split_pad is a
// multiple of 8), so a part's stores only have to reach that XCD's L2 (dh_release_before_flag) and the next part only has to
// drop its CU's L1 / scalar cache (dh_acquire_behind_flag); the flag word carries the epoch of the push, the number of parts
// written back and the XCC id.  None of this is promised by HIP: HipBackend::open probes the placement once per device and
// switches the split off where it does not hold, and a part that finds another XCC id, or no flag within its patience, touches
// nothing and leaves -- the fix-up launch that follows every split launch (split_fixup) then finishes that channel's row.
#pragma once

#include "launch_plan.hpp"

// ---- the hand-over flag word of a split push (DH_ST_PART of a channel's state):
// epoch of the push (24 bits, never 0) | parts written back << 24 | a later part gave up << 26 | XCC id << 28
#define DH_PF_GAVE_UP (1u << 26)
DH_HD uint32_t dh_pf_pack(uint32_t epoch, uint32_t part, uint32_t xcc) { return epoch | (part + 1u) << 24 | xcc << 28; }    // part 0..2 has been written back
DH_HD bool dh_pf_of_push(uint32_t v, uint32_t epoch) { return (v & 0x00FFFFFFu) == epoch; }
DH_HD uint32_t dh_pf_done(uint32_t v) { return (v >> 24) & 3u; }
DH_HD uint32_t dh_pf_xcc(uint32_t v) { return v >> 28; }
// Merges `mine` into the flag word: of a word of this push the bits of keep_mask stay, a word of an older push is replaced.
// (Compare-and-swap, not a store: the part in front and the part that gives up behind it write the same word, in either order.)
DH_HD void dh_pf_publish(uint32_t* flag, uint32_t epoch, uint32_t mine, uint32_t keep_mask) {
    uint32_t seen = dh_agent_load(flag);
    for (;;) {
        const uint32_t want = mine | (dh_pf_of_push(seen, epoch) ? (seen & keep_mask) : 0u);
        if (dh_agent_cas(flag, seen, want)) break;
    }
}

// ---- the parts of a push
// part p = 0, 1, 2 takes the samples [lo, hi) of the row; the fix-up behind a failed hand-over takes [lo of the first
// unfinished part, dh_part_hi(2, ...) = the end of the row)
DH_HD uint32_t dh_part_lo(uint32_t part, uint32_t n0, uint32_t n1) { return part == 0 ? 0u : part == 1 ? n0 : n1; }
DH_HD uint32_t dh_part_hi(uint32_t part, uint32_t n0, uint32_t n1) { return part == 0 ? n0 : (part == 1 && n1) ? n1 : 0xFFFFFFFFu; }
DH_HD uint32_t dh_last_part(const DhDspParams& P) { return P.split_n0 ? (P.split_n1 ? 2u : 1u) : 0u; }
// Which part of which channel block `bid` of a split launch is: `bid` comes back channel-local (channel = bid + ch_base),
// padding = one of the blocks between the parts of the grid.  Block b of an unsplit or a fix-up launch is part 0 of channel b.
struct DhBlockPart { uint32_t part, bid; bool padding; };
DH_HD DhBlockPart dh_part_of_block(const DhDspParams& P, uint32_t bid) {
    DhBlockPart B = { 0u, bid, false };
    if (P.split_n0 && !P.split_fixup) {
        const uint32_t last = dh_last_part(P);
        while (B.part < last && B.bid >= P.split_pad) { B.part++; B.bid -= P.split_pad; }
        B.padding = B.bid >= P.n_channels;
    }
    return B;
}
DH_HD uint32_t* dh_part_flag(const DhDspParams& P, uint32_t ch) { return reinterpret_cast<uint32_t*>(P.state) + (size_t) ch * P.state_stride + DH_ST_PART; }

// ---- everything in front of the slicer: what this workgroup is to do, if anything
struct DhChainPart { uint32_t ch, part, lo, hi, sym_base; bool run; };
DH_HD DhChainPart dh_chain_enter(const DhDspParams& P, uint32_t bid) {
    DhChainPart E = { 0u, 0u, 0u, 0xFFFFFFFFu, 0u, false };
    const DhBlockPart B = dh_part_of_block(P, bid);
    if (B.padding) return E;
    E.part = B.part;
    if (P.split_n0 && !P.split_fixup) { E.lo = dh_part_lo(E.part, P.split_n0, P.split_n1); E.hi = dh_part_hi(E.part, P.split_n0, P.split_n1); }
    E.ch = B.bid + P.ch_base;
    uint32_t* const part_flag = dh_part_flag(P, E.ch);
    if (P.split_n0 && P.split_fixup) {
        // The launch behind a split launch, one workgroup per channel.  The kernel boundary in front of it has made everything
        // the split launch stored visible; a channel whose flag word says that all parts were written back -- every channel,
        // unless a hand-over failed -- is left alone.  Otherwise the rest of the row is done here in one piece, starting behind
        // the last part that was completed.
        const uint32_t v = dh_uniform(dh_agent_load(part_flag));
        const uint32_t done = dh_pf_of_push(v, P.part_epoch) ? dh_pf_done(v) : 0u;
        if (done > dh_last_part(P)) return E;
        E.part = done;
        E.lo = dh_part_lo(E.part, P.split_n0, P.split_n1);
        if (E.part) E.sym_base = dh_uniform(dh_agent_load(P.sym_count + E.ch));
    } else if (E.part) {
        const uint32_t xcc = dh_xcc_id();
        bool ok = false, told = false;
        const bool forced = P.split_force_fail && E.part == 1u && E.ch % P.split_force_fail == 1u;     // (tests: this hand-over "fails"; a third part then has to notice)
        for (uint32_t spin = 0; spin < (1u << 16) && !forced; spin++) {                 // (a first part takes ~1.5 ms; 2^16 x ~2 us)
            const uint32_t v = dh_uniform(dh_agent_load(part_flag));
            if (dh_pf_of_push(v, P.part_epoch)) {
                if (v & DH_PF_GAVE_UP) { told = true; break; }                              // the part in front of this one gave up
                if (dh_pf_done(v) >= E.part) { ok = dh_pf_xcc(v) == xcc; break; }
            }
            dh_nap();
        }
        dh_acquire_behind_flag();
        if (!ok) {
            // No hand-over (never seen on an MI355X in SPX mode, where the probe of HipBackend::open holds): nothing of this
            // channel has been touched by this workgroup, the fix-up launch behind this one finishes the row.
            if (dh_is_writer_lane()) {
                // "gave up" is published as a word of THIS push (the whole word kept if it is one, the bare epoch otherwise): when the
                // part in front has not published yet the word still carries an older epoch, and a bit set on that would be dropped by
                // that part's publish (it only keeps the bit of a word of its own push) -- the part behind this one would then spin
                // through its whole patience instead of leaving at once
                dh_pf_publish(part_flag, P.part_epoch, P.part_epoch | DH_PF_GAVE_UP, 0xFFFFFFFFu);
                if (P.overflow) dh_agent_add(P.overflow + 2, 1u);               // (a statistic: dh_engine_debug_header(202))
                if (P.overflow && told) dh_agent_add(P.overflow + 3, 1u);       // ... of which: told so by the part in front (203)
            }
            return E;
        }
        E.sym_base = dh_uniform(dh_agent_load(P.sym_count + E.ch));
    }
    E.run = true;
    return E;
}

// ---- ... and behind the decoder: this part has been written back.  (The last part publishes too: the fix-up launch reads how
// far the row got.)  `bid` is worked out into part and flag word again, from an opaque copy of the block index: nothing of
// the hand-over stays live through the two halves.
DH_HD void dh_chain_leave(const DhDspParams& P, uint32_t bid) {
    if (!P.split_n0) return;
    const DhBlockPart B = dh_part_of_block(P, bid);
    const uint32_t part = P.split_fixup ? dh_last_part(P) : B.part;                   // the fix-up launch finishes the row
    uint32_t* const flag = dh_part_flag(P, B.bid + P.ch_base);
    dh_release_before_flag();
    // (a later part that has given up meanwhile set bit 26: a plain store would wipe it out and leave the part behind that one
    // spinning through its whole patience -- the bit of a word of this push is kept)
    if (dh_is_writer_lane()) dh_pf_publish(flag, P.part_epoch, dh_pf_pack(P.part_epoch, part, dh_xcc_id()), DH_PF_GAVE_UP);
}

// The whole chain of one channel in one wavefront: slice this part's samples, then run the protocol decoder over the symbols
// just produced.  The two stages use the block `smem` (max(dh_dsp_shared_bytes, sizeof(DhDecShared)) bytes, 16-byte aligned)
// one after the other.
template <int NZ, bool FAST, int PROTO, int SPS>
DH_HD void dh_chain_workgroup(const DhDspParams& P, const DhDecParams& D, uint32_t bid, void* smem) {
    const DhChainPart E = dh_chain_enter(P, bid);
    if (!E.run) return;
    {
        DhDspShared L = dh_dsp_carve(smem, SPS ? (uint32_t) SPS : P.sps, NZ);
        constexpr int LV = DhChainInst<NZ, FAST, PROTO, SPS>::LV;
        dh_rrc_demod_channel<NZ, FAST, SPS, LV>(P, E.ch, L, E.lo, E.hi, E.sym_base);      // (dh_plan_chain checked P.levels)
    }
    // This wavefront's symbol / count stores are read back by its own decoder half below: a WORKGROUP-scope fence orders
    // them.  A device-scope fence here made every wavefront write back its XCD's L2 -- 16 384 times per launch, 0.7 ms of a
    // push of 4 752 samples (tools/push_size.py).
    dh_barrier_global();
    DhDecShared& S = *reinterpret_cast<DhDecShared*>(smem);
#ifdef DH_SKIP_DECODER                      // diagnostic builds (tools/phase_budget.sh): the slicer half alone (the hand-over of the tail split still takes place)
    if (!P.n_channels)
#endif
    dh_decode_channel(PROTO, D, E.ch, S, E.sym_base, E.part != 0);
    dh_chain_leave(P, dh_opaque_scalar(bid));
}
