// outpack_core.hpp -- the packed read-out (include/digiham_amd.h, "Packed read-out"): what one engine push produced, moved
// from the engine's dense [B][out_cap] / [B][ev_cap] rows into three compact device areas behind one header, appendable
// across the pushes and engines of a round.  Bodies of the kernels k_outpack_scan and
// k_outpack_copy (at the end of this file), which both builds compile.  No arithmetic on the data: counts are added up, bytes move as 16-byte
// pieces.
//
// The scan is ONE workgroup of DH_OP_LANES lanes (four wavefronts) that walks the B channels DH_OP_LANES at a time, in
// phases as dh_portable.hpp describes them -- here the phases span the whole workgroup, so the lane loop of the harness
// runs over 256 lanes and a per-lane value is an array of 256:
//   1. lane l reads channel base + l: is it a candidate, its event count ec, its frame bytes fc; the wavefront votes on
//      "candidate" and adds up ec and pad16(fc) by an inclusive shuffle scan; lane 63 leaves the wavefront's three totals in LDS;
//   2. a candidate's place is the running carry + the totals of the wavefronts below + its place inside its own wavefront
//      (votes below the lane; the scan less its own share).  The sums run over ALL candidates, kept or not: they only grow, so
//      once a candidate does not fit no later one does, and "fits" may be decided by every lane for itself -- the kept set
//      is a prefix without anybody looking for its end.  A kept candidate writes its entry;
//   3. every lane adds the four wavefront totals to its copy of the carry.
// After the last pass the kept candidate with the largest n_entries-after-it is the last one: its lane writes the totals
// into the header; lane 0 adds the candidates beyond it to `dropped`, counts the append and leaves (n_entries before,
// entries added) in the scratch words for the copy.  All sums are 64 bits wide: nothing wraps below 2^32 channels.
#pragma once

#include "dh_portable.hpp"
#include "../../include/digiham_amd.h"      // dh_outpack_header, dh_outpack_entry, dh_event

// (DH_OP_LANES, DH_OP_WAVES and the DH_OP_* vocabulary of a 256-lane phase: dh_portable.hpp)

struct DhOutpack {
    dh_outpack_header* hdr; dh_outpack_entry* entries; dh_event* events; uint8_t* frames;      // the pack
    uint32_t* scratch;                      // [2]: n_entries before this append, entries it added
    uint32_t max_entries, max_events; uint64_t max_frame_bytes;
    const uint8_t* src_frames; const uint32_t* src_fc; uint32_t out_cap;         // the engine's rows; out_cap a multiple of 64
    const dh_event* src_events; const uint32_t* src_ec; uint32_t ev_cap;         // src_events null: DH_FLAG_NO_EVENTS
    const uint32_t* mask; const uint64_t* tag;                                    // [B] each, or null
    uint64_t tag_add; uint32_t user, B;
};

struct DhOpShared { uint64_t wave_v[DH_OP_WAVES], wave_f[DH_OP_WAVES]; uint32_t wave_c[DH_OP_WAVES], wave_best[DH_OP_WAVES]; };

struct alignas(16) DhOpQuad { uint32_t w[4]; };

DH_HD uint64_t dh_op_pad16(uint32_t n) { return ((uint64_t) n + 15u) & ~(uint64_t) 15u; }

// One append: candidates, fit rule, entries, header, scratch.  One workgroup of DH_OP_LANES lanes.
DH_D void dh_outpack_scan(const DhOutpack& P, DhOpShared& S) {
    // the totals the append starts from: read before anything is written (the header's stores come behind the last barrier)
    const uint64_t E0 = P.hdr->n_entries, V0 = P.hdr->n_events, F0 = P.hdr->frame_bytes;
    const bool open = P.hdr->dropped == 0u;
    uint64_t cE = E0, cV = V0, cF = F0;                         // the carry: totals over every candidate so far (the same in every lane)
    DH_OP_VAL(uint32_t, best); DH_OP_VAL(uint64_t, best_v); DH_OP_VAL(uint64_t, best_f);       // the totals behind the lane's last kept candidate
    DH_OP_FOR(lane) { DH_OP_V(best, lane) = (uint32_t) E0; DH_OP_V(best_v, lane) = V0; DH_OP_V(best_f, lane) = F0; }

    for (uint32_t base = 0; base < P.B; base += DH_OP_LANES) {
        DH_OP_VAL(uint32_t, fc); DH_OP_VAL(uint32_t, ec); DH_OP_VAL(uint64_t, sv); DH_OP_VAL(uint64_t, sf);
        DH_OP_WAVE_VAL(uint64_t, vote);
        DH_OP_CLEAR_VOTES(vote);
        DH_OP_FOR(lane) {                                       // 1
            const uint32_t b = base + lane;
            uint32_t f = 0, e = 0;
            if (b < P.B && (!P.mask || P.mask[b] != 0u)) {
                f = dh_min(P.src_fc[b], P.out_cap);
                e = P.src_events ? dh_min(P.src_ec[b], P.ev_cap) : 0u;
            }
            DH_OP_V(fc, lane) = f; DH_OP_V(ec, lane) = e;
            DH_OP_V(sv, lane) = e; DH_OP_V(sf, lane) = dh_op_pad16(f);
            DH_OP_VOTE(vote, (f | e) != 0u, lane);
        }
        DH_OP_WAVE_SCAN(sv);
        DH_OP_WAVE_SCAN(sf);
        DH_OP_FOR(lane) {
            if ((lane & (DH_WAVE - 1u)) == DH_WAVE - 1u) {
                const uint32_t w = lane / DH_WAVE;
                S.wave_c[w] = (uint32_t) dh_popc64(DH_OP_W(vote, lane)); S.wave_v[w] = DH_OP_V(sv, lane); S.wave_f[w] = DH_OP_V(sf, lane);
            }
        }
        DH_BARRIER();
        DH_OP_FOR(lane) {                                       // 2
            const uint32_t w = lane / DH_WAVE, wl = lane & (DH_WAVE - 1u);
            const uint64_t votes = DH_OP_W(vote, lane);
            if ((votes >> wl) & 1u) {
                uint64_t E = cE, V1 = cV, F1 = cF;
                for (uint32_t k = 0; k < w; k++) { E += S.wave_c[k]; V1 += S.wave_v[k]; F1 += S.wave_f[k]; }
                E += (uint32_t) dh_popc64(votes & (((uint64_t) 1 << wl) - 1u));
                V1 += DH_OP_V(sv, lane); F1 += DH_OP_V(sf, lane);           // the totals behind this candidate
                const uint32_t f = DH_OP_V(fc, lane), e = DH_OP_V(ec, lane);
                if (open && E + 1u <= P.max_entries && V1 <= P.max_events && F1 <= P.max_frame_bytes) {
                    const uint32_t b = base + lane;
                    dh_outpack_entry en;
                    en.channel = b; en.user = P.user; en.tag = (P.tag ? P.tag[b] : 0u) + P.tag_add;
                    en.n_frame_bytes = f; en.n_events = e;
                    en.frame_offset16 = (uint32_t) ((F1 - dh_op_pad16(f)) / 16u); en.event_index = (uint32_t) (V1 - e);
                    P.entries[E] = en;
                    DH_OP_V(best, lane) = (uint32_t) (E + 1u); DH_OP_V(best_v, lane) = V1; DH_OP_V(best_f, lane) = F1;
                }
            }
        }
        for (uint32_t k = 0; k < DH_OP_WAVES; k++) { cE += S.wave_c[k]; cV += S.wave_v[k]; cF += S.wave_f[k]; }       // 3
        DH_BARRIER();                                       // (the next pass writes the totals again)
    }

    DH_OP_VAL(uint32_t, wave_best);
    DH_OP_WAVE_MAX(wave_best, best);
    DH_OP_FOR(lane) { if ((lane & (DH_WAVE - 1u)) == 0u) S.wave_best[lane / DH_WAVE] = DH_OP_V(wave_best, lane); }
    DH_BARRIER();
    DH_OP_FOR(lane) {
        uint32_t last = S.wave_best[0];
        for (uint32_t k = 1; k < DH_OP_WAVES; k++) last = dh_max(last, S.wave_best[k]);
        if (last > (uint32_t) E0 && DH_OP_V(best, lane) == last) {              // one lane: n_entries after a kept candidate is its own
            P.hdr->n_entries = last; P.hdr->n_events = (uint32_t) DH_OP_V(best_v, lane); P.hdr->frame_bytes = DH_OP_V(best_f, lane);
        }
        if (lane == 0u) {
            P.hdr->dropped += (uint32_t) (cE - last);
            P.hdr->appends += 1u;
            P.scratch[0] = (uint32_t) E0; P.scratch[1] = last - (uint32_t) E0;
        }
    }
}

// Entry idx of the pack: the share of lane `lane` of `lanes` in copying its events and its frame bytes.  16 bytes per
// store: an event row starts at a multiple of 32 bytes and a record is two pieces; a frame row starts at a multiple of
// 64 bytes (out_cap), its place in the pack at a multiple of 16.  The piece that holds the row's last fc mod 16 bytes is
// read whole -- it lies inside the row -- and stored with the bytes behind them cleared.
DH_HD void dh_outpack_copy_entry(const DhOutpack& P, uint32_t idx, uint32_t lane, uint32_t lanes) {
    const dh_outpack_entry en = P.entries[idx];
    const uint32_t pieces = 2u * en.n_events;
    if (pieces) {
        const DhOpQuad* src = (const DhOpQuad*) (P.src_events + (size_t) en.channel * P.ev_cap);
        DhOpQuad* dst = (DhOpQuad*) (P.events + en.event_index);
        for (uint32_t i = lane; i < pieces; i += lanes) dst[i] = src[i];
    }
    const uint32_t whole = en.n_frame_bytes / 16u, rem = en.n_frame_bytes & 15u;
    if (whole | rem) {
        const DhOpQuad* src = (const DhOpQuad*) (P.src_frames + (size_t) en.channel * P.out_cap);
        DhOpQuad* dst = (DhOpQuad*) (P.frames + (uint64_t) en.frame_offset16 * 16u);
        for (uint32_t i = lane; i < whole; i += lanes) dst[i] = src[i];
        if (rem && lane == whole % lanes) {
            DhOpQuad q = src[whole];
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t keep = rem > 4u * k ? dh_min(rem - 4u * k, 4u) : 0u;       // bytes of word k that are the row's
                if (keep < 4u) q.w[k] &= keep ? (1u << (8u * keep)) - 1u : 0u;
            }
            dst[whole] = q;
        }
    }
}

// ---------------------------------------------------------------------------------- packed read-out (outpack_core.hpp)
// k_outpack_scan: ONE workgroup of 256 lanes walks the engine's B channels 256 at a time -- B is at most a few tens of
// thousands of 8-byte reads -- so that the order rule is exact without any hand-over between workgroups: candidate vote
// and popcount below the lane, two shuffle scans per wavefront, the wavefronts' totals through 48 bytes of LDS, a running
// carry across passes.  Ordinary vector stores only.
// k_outpack_copy: a fixed grid, workgroup i takes entries i, i + gridDim.x, ... of THIS append while i < n_new; n_new and
// the first entry's index are the two scratch words the scan left, the same for every lane.
namespace {

__global__ __launch_bounds__(DH_OP_LANES) void k_outpack_scan(const DhOutpack P) {
    __shared__ DhOpShared S;
    dh_outpack_scan(P, S);
}

__global__ __launch_bounds__(256) void k_outpack_copy(const DhOutpack P) {
    const uint32_t first = P.scratch[0], n_new = P.scratch[1];
    for (uint32_t i = blockIdx.x; i < n_new; i += gridDim.x) dh_outpack_copy_entry(P, first + i, threadIdx.x, 256u);
}

}  // namespace

template <class BE> static int dh_be_outpack_scan(BE& be, const DhOutpack& P) {
    return dh_launch(k_outpack_scan, dim3(1), dh_workgroup(DH_OP_LANES), 0, dh_be_stream(be, 0), "k_outpack_scan", P);
}
template <class BE> static int dh_be_outpack_copy(BE& be, const DhOutpack& P) {
    return dh_launch(k_outpack_copy, dim3(P.B < 1024u ? P.B : 1024u), dim3(256), 0, dh_be_stream(be, 0), "k_outpack_copy", P);
}
