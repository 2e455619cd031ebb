// monitor_core.hpp -- the band monitor's per-round bookkeeping (include/digiham_amd.h, "Band monitor"): which channels
// the scanner sees, which one is named and from where its decoder is fed, which ones an engine forgets.  Bodies shared by
// the gfx950 build and the CPU test harness (kernels of steps B and C: the end of this file; k_monitor_open, k_reset_channels: engine.hip).  No arithmetic on samples: three small words of state per
// channel (a fourth, `opened`, for naming on close), nine statistics records read per scanned or closing channel, and one
// fixed-size summary block that is all the host reads per round.
#pragma once

#include "dh_portable.hpp"
#include "preroll_core.hpp"

#define DH_MON_PROTOS 6u            /* arrays indexed by DH_PROTO_*: [0] (DH_PROTO_NONE) stays unused */
#define DH_MON_FRONTS 4u            /* wide10, narrow20, fsk10, fsk40i */
#define DH_MON_FAMILIES 5u
#define DH_MON_STAT_BYTES 144u      /* DH_SCAN_PATTERNS x sizeof(dh_scan_stat) */
#define DH_MON_RUN_MAX 0xFFFFFFFFu

// the block the host reads after step A (n_scan, n_reset, n_live) and after steps B and C (n_new, min_start); the host
// re-initialises it in front of step A: counts 0, every min_start DH_PREROLL_NONE
struct DhMonSummary {
    uint32_t n_scan;                        // channels with scan_counts != 0
    uint32_t n_reset;                       // channels with scan_reset set by step A: the CLOSING channels, step C's
    uint32_t n_live[DH_MON_PROTOS];         // channels with live_counts[p] != 0
    uint32_t n_new[DH_MON_PROTOS];          // channels assigned to p by step B or step C
    uint64_t min_start[DH_MON_PROTOS];      // the smallest start among them
};

struct DhMonOpen {                          // step A
    const uint64_t* open_at;                // [B] the ring's, after this round's append
    uint8_t* assigned; uint32_t* closed_run; uint64_t* start;        // [B] the state
    uint64_t* opened;                       // [B] open_at of the last open round (step C's); null: not kept
    uint8_t* scan_reset; uint32_t* scan_counts;                      // [B]
    uint32_t* live_counts[DH_MON_PROTOS];   // [B] each; null: the protocol is not configured
    DhMonSummary* sum;
    uint32_t B, n, release;
};

struct DhMonStats {                         // where steps B and C read the scanner's evidence
    const uint8_t* stats[DH_MON_FRONTS];    // the "frames" rows of the scan engine of a front end; null: not configured
    const uint32_t* stat_count[DH_MON_FRONTS];
    size_t stat_stride[DH_MON_FRONTS];
};

struct DhMonAssign : DhMonStats {           // step B
    const uint32_t* scan_counts; const uint64_t* open_at;
    uint8_t* assigned; uint64_t* start; uint8_t* scan_reset;
    uint8_t* new_flags[DH_MON_PROTOS]; uint64_t* from[DH_MON_PROTOS];        // [B] each; null: not configured
    DhMonSummary* sum;
    uint32_t B, lead, depth, confirm;
    uint64_t total;
};

struct DhMonClose : DhMonStats {            // step C
    const uint8_t* scan_reset;              // [B] step A's: 1 marks the closing channels
    const uint64_t* opened;
    uint8_t* assigned; uint64_t* start;
    uint8_t* new_flags[DH_MON_PROTOS]; uint64_t* from[DH_MON_PROTOS];        // [B] each; null: not configured
    DhMonSummary* sum;
    uint32_t B, lead, depth;
    uint32_t close_hits[DH_MON_FAMILIES], close_dist[DH_MON_FAMILIES];
    uint64_t total;
};

#define DH_RST_MAX_BUFS 12u
struct DhResetChannels {
    const uint8_t* flags;                   // [B]
    struct { void* p; uint32_t row_bytes; } buf[DH_RST_MAX_BUFS];    // what the engine declared ZERO_PER_CHANNEL
    uint32_t n_bufs;
    uint32_t* dsp_state; size_t state_words; uint32_t tail0; uint32_t* dec_state; uint32_t slot_filter;      // k_init_state's
    uint32_t B;
};

// the front end pattern i is read from (api.SCAN_SOURCE), its family, and the protocol a family stands for, in the
// order ties are broken: DMR, YSF, NXDN, D-Star, POCSAG
DH_HD uint32_t dh_mon_pattern_front(uint32_t i) { return i < 5u ? 0u : i == 5u ? 1u : i < 8u ? 2u : 3u; }
DH_HD uint32_t dh_mon_pattern_family(uint32_t i) { return i < 4u ? 0u : i == 4u ? 1u : i == 5u ? 2u : i < 8u ? 3u : 4u; }
DH_HD uint32_t dh_mon_family_proto(uint32_t f) { return f < 3u ? f + 1u : f == 3u ? 5u : 4u; }     // DH_PROTO_DMR, _YSF, _NXDN, _DSTAR, _POCSAG

// Step A for channel b.  Returns the bits the caller adds up into the summary: bit 0 scanned, bit 1 scan_reset,
// bits 8.. the protocol it is live in (0: none).
DH_HD uint32_t dh_mon_open_channel(const DhMonOpen& A, uint32_t b) {
    const bool open = A.open_at[b] != DH_PR_NONE;
    const uint32_t was = A.closed_run[b];
    const uint32_t run = open ? 0u : (was == DH_MON_RUN_MAX ? was : was + 1u);
    A.closed_run[b] = run;
    if (open && A.opened) A.opened[b] = A.open_at[b];
    uint32_t a = A.assigned[b];
    uint32_t reset = 0;
    if (!open) {
        if (a == 0u) reset = run == 1u ? 1u : 0u;
        else if (run >= A.release) { a = 0u; A.assigned[b] = 0; A.start[b] = DH_PR_NONE; }
    }
    A.scan_reset[b] = (uint8_t) reset;
    const bool scanned = open && a == 0u;
    A.scan_counts[b] = scanned ? A.n : 0u;
    for (uint32_t p = 1; p < DH_MON_PROTOS; p++)
        if (A.live_counts[p]) A.live_counts[p][b] = open && a == p ? A.n : 0u;
    const uint32_t live = open && a != 0u && A.live_counts[a] ? a : 0u;
    return (scanned ? 1u : 0u) | (reset << 1) | (live << 8);
}

// The statistics record of pattern i of channel b (dh_scan_stat as four words: hits, periodic, last_sym, best_dist in the
// low byte), from the scan engine of the pattern's front end.  Null -- a front end that is not configured, a row of fewer
// than 144 bytes -- reads as zeros and best_dist 255.
DH_HD const uint32_t* dh_mon_stat(const DhMonStats& S, uint32_t b, uint32_t i) {
    const uint32_t f = dh_mon_pattern_front(i);
    if (!S.stats[f] || S.stat_count[f][b] < DH_MON_STAT_BYTES) return nullptr;
    return (const uint32_t*) (S.stats[f] + (size_t) b * S.stat_stride[f]) + 4u * i;            // rows are 64-byte multiples apart
}

// where the decoder of a channel named now begins: max(open_at - lead, total - depth, 0), both differences saturating
DH_HD uint64_t dh_mon_start(uint64_t open_at, uint32_t lead, uint32_t depth, uint64_t total) {
    const uint64_t lo = open_at > lead ? open_at - lead : 0u;
    const uint64_t oldest = total > depth ? total - depth : 0u;
    return lo > oldest ? lo : oldest;
}

// Step B for channel b.  Returns the protocol the channel was assigned to in this round (0: none) and its start.
DH_HD uint32_t dh_mon_assign_channel(const DhMonAssign& S, uint32_t b, uint64_t& start) {
    uint32_t won = 0;
    start = DH_PR_NONE;
    // a channel that step A marked as closing and that is assigned all the same was named by step C in this round: its
    // new_flags and from entries are step C's (without naming on close there is no such channel)
    const bool named_on_close = S.scan_reset[b] != 0u && S.assigned[b] != 0u;
    if (S.scan_counts[b] != 0u) {
        uint64_t sums[DH_MON_FAMILIES] = { 0, 0, 0, 0, 0 };
        for (uint32_t i = 0; i < 9u; i++) {
            const uint32_t* r = dh_mon_stat(S, b, i);
            if (r) sums[dh_mon_pattern_family(i)] += r[1];
        }
        uint32_t best = 0;
        for (uint32_t f = 1; f < DH_MON_FAMILIES; f++) if (sums[f] > sums[best]) best = f;       // (the first of equal sums)
        const uint32_t p = dh_mon_family_proto(best);
        if (sums[best] >= S.confirm && S.new_flags[p]) {
            start = dh_mon_start(S.open_at[b], S.lead, S.depth, S.total);
            won = p;
            S.assigned[b] = (uint8_t) p;
            S.start[b] = start;
        }
    }
    if (!named_on_close)
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++)
            if (S.new_flags[p]) { S.new_flags[p][b] = won == p ? 1 : 0; S.from[p][b] = won == p ? start : DH_PR_NONE; }
    S.scan_reset[b] = won ? 1 : 0;
    return won;
}

// Step C for channel b: naming on close.  Of a closing channel, per family, H = the sum of `hits` and D = the smallest
// best_dist over the family's patterns; a family is eligible with close_hits != 0, H >= close_hits and D <= close_dist; the
// eligible family with the largest H wins, the first in order where two are level.  Returns the protocol the channel was
// assigned to (0: none) and its start.  scan_reset stays as step A left it.
DH_HD uint32_t dh_mon_close_channel(const DhMonClose& C, uint32_t b, uint64_t& start) {
    uint32_t cand = 0, won = 0;                                            // (no array is indexed by a lane's value: registers only)
    start = DH_PR_NONE;
    if (C.scan_reset[b] != 0u) {
        uint64_t H[DH_MON_FAMILIES] = { 0, 0, 0, 0, 0 };
        uint32_t D[DH_MON_FAMILIES] = { 255u, 255u, 255u, 255u, 255u };
        for (uint32_t i = 0; i < 9u; i++) {
            const uint32_t* r = dh_mon_stat(C, b, i);
            if (!r) continue;
            const uint32_t f = dh_mon_pattern_family(i), d = r[3] & 255u;
            H[f] += r[0];
            if (d < D[f]) D[f] = d;
        }
        uint64_t most = 0;
        for (uint32_t f = 0; f < DH_MON_FAMILIES; f++) {
            const bool eligible = C.close_hits[f] != 0u && H[f] >= C.close_hits[f] && D[f] <= C.close_dist[f];
            if (eligible && (cand == 0u || H[f] > most)) { cand = dh_mon_family_proto(f); most = H[f]; }
        }
        if (cand) start = dh_mon_start(C.opened[b], C.lead, C.depth, C.total);
    }
    for (uint32_t p = 1; p < DH_MON_PROTOS; p++)
        if (C.new_flags[p]) {                                              // (a winner that is not configured wins nothing)
            const bool w = cand == p;
            if (w) won = p;
            C.new_flags[p][b] = w ? 1 : 0; C.from[p][b] = w ? start : DH_PR_NONE;
        }
    if (won) { C.assigned[b] = (uint8_t) won; C.start[b] = start; }
    return won;
}

// Masked reset, channel b: the share of lane `lane` of `lanes` in zeroing row b of every declared buffer.  16 bytes per
// store where the row starts on a 16-byte boundary and is a multiple of 16 long (the slicer state, the symbol rows, the
// decoder state, the carried symbols), otherwise 4 bytes (the per-channel counters); lane 0 takes a tail of fewer than
// four bytes, which no buffer of today has.
struct alignas(16) DhRstQuad { uint32_t w[4]; };
DH_HD void dh_rst_zero_rows(const DhResetChannels& R, uint32_t b, uint32_t lane, uint32_t lanes) {
    for (uint32_t k = 0; k < R.n_bufs; k++) {
        const uint32_t bytes = R.buf[k].row_bytes;
        char* row = (char*) R.buf[k].p + (size_t) b * bytes;
        if ((((uintptr_t) row | bytes) & 15u) == 0u) {
            const DhRstQuad z = { { 0u, 0u, 0u, 0u } };
            for (uint32_t i = lane; i < bytes / 16u; i += lanes) ((DhRstQuad*) row)[i] = z;
        } else if (((uintptr_t) row & 3u) == 0u) {
            for (uint32_t i = lane; i < bytes / 4u; i += lanes) ((uint32_t*) row)[i] = 0u;
            if (lane == 0u) for (uint32_t i = bytes & ~3u; i < bytes; i++) row[i] = 0;
        } else {
            for (uint32_t i = lane; i < bytes; i += lanes) row[i] = 0;
        }
    }
}
// ... and then, by one lane once the zeros are in memory, what k_init_state does for a channel (kernels_core.hpp)
DH_HD void dh_rst_init(const DhResetChannels& R, uint32_t b) {
    dh_init_state_channel(R.dsp_state, R.state_words, R.tail0, R.dec_state, R.slot_filter, b);
}

#if !DH_DEVICE_BUILD
// ---- CPU restatements of the masked reset (a barrier between its two steps) and of step A (counted per wavefront with
// votes); engine.hip has the gfx950 kernels; the monitor's other launches follow, one text for both builds ---------------
template <class BE>
static int dh_be_reset_channels(BE&, const DhResetChannels& R) {
    for (uint32_t b = R.B; b-- > 0;)
        if (R.flags[b]) { dh_rst_zero_rows(R, b, 0u, 1u); dh_rst_init(R, b); }
    return 0;
}
static int dh_be_monitor_open(const DhMonOpen& A, void*) {
    for (uint32_t b = A.B; b-- > 0;) {                                      // (the lanes of a launch have no order)
        const uint32_t r = dh_mon_open_channel(A, b);
        A.sum->n_scan += r & 1u; A.sum->n_reset += (r >> 1) & 1u;
        if (r >> 8) A.sum->n_live[r >> 8] += 1u;
    }
    return 0;
}
#endif

// ---------------------------------------------------------------------------------- band monitor (monitor_core.hpp)
// Steps B and C of a round: one lane per channel, 256-thread workgroups.  Ordinary vector stores for the state and the
// per-channel outputs; the summary block takes one vector atomic per newly named channel.  (Step A, k_monitor_open, counts per
// wavefront with votes: engine.hip, its CPU restatement in monitor_core.hpp.)
namespace {

__global__ __launch_bounds__(256) void k_monitor_assign(const DhMonAssign S) {
    for (uint32_t b = blockIdx.x * 256u + threadIdx.x; b < S.B; b += gridDim.x * 256u) {
        uint64_t start;
        const uint32_t p = dh_mon_assign_channel(S, b, start);
        if (p) {
            atomicAdd(&S.sum->n_new[p], 1u);
            atomicMin((unsigned long long*) &S.sum->min_start[p], (unsigned long long) start);
        }
    }
}

__global__ __launch_bounds__(256) void k_monitor_close(const DhMonClose C) {
    for (uint32_t b = blockIdx.x * 256u + threadIdx.x; b < C.B; b += gridDim.x * 256u) {
        uint64_t start;
        const uint32_t p = dh_mon_close_channel(C, b, start);
        if (p) {
            atomicAdd(&C.sum->n_new[p], 1u);
            atomicMin((unsigned long long*) &C.sum->min_start[p], (unsigned long long) start);
        }
    }
}

}  // namespace

static int dh_be_monitor_assign(const DhMonAssign& S, void* stream) {
    return dh_launch(k_monitor_assign, dim3(grid_for(S.B, 256)), dim3(256), 0, stream, "k_monitor_assign", S) ? DH_EDEVICE : DH_OK;
}
static int dh_be_monitor_close(const DhMonClose& C, void* stream) {
    return dh_launch(k_monitor_close, dim3(grid_for(C.B, 256)), dim3(256), 0, stream, "k_monitor_close", C) ? DH_EDEVICE : DH_OK;
}
