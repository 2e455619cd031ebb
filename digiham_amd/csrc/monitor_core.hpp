// monitor_core.hpp -- the band monitor's per-round bookkeeping (include/digiham_amd.h, "Band monitor"): which channels
// the scanner sees, which one is named and from where its decoder is fed, which ones an engine forgets.  Bodies shared by
// the gfx950 kernels in engine.hip and by the CPU test harness.  No arithmetic on samples: three small words of state per
// channel, nine counters read per scanned channel, and one fixed-size summary block that is all the host reads per round.
#pragma once

#include "dh_portable.hpp"
#include "preroll_core.hpp"

#define DH_MON_PROTOS 6u            /* arrays indexed by DH_PROTO_*: [0] (DH_PROTO_NONE) stays unused */
#define DH_MON_FRONTS 4u            /* wide10, narrow20, fsk10, fsk40i */
#define DH_MON_FAMILIES 5u
#define DH_MON_STAT_BYTES 144u      /* DH_SCAN_PATTERNS x sizeof(dh_scan_stat) */
#define DH_MON_RUN_MAX 0xFFFFFFFFu

// the block the host reads after step A (n_scan, n_reset, n_live) and after step B (n_new, min_start); the host
// re-initialises it in front of step A: counts 0, every min_start DH_PREROLL_NONE
struct DhMonSummary {
    uint32_t n_scan;                        // channels with scan_counts != 0
    uint32_t n_reset;                       // channels with scan_reset set by step A
    uint32_t n_live[DH_MON_PROTOS];         // channels with live_counts[p] != 0
    uint32_t n_new[DH_MON_PROTOS];          // channels assigned to p by step B
    uint64_t min_start[DH_MON_PROTOS];      // the smallest start among them
};

struct DhMonOpen {                          // step A
    const uint64_t* open_at;                // [B] the ring's, after this round's append
    uint8_t* assigned; uint32_t* closed_run; uint64_t* start;        // [B] the state
    uint8_t* scan_reset; uint32_t* scan_counts;                      // [B]
    uint32_t* live_counts[DH_MON_PROTOS];   // [B] each; null: the protocol is not configured
    DhMonSummary* sum;
    uint32_t B, n, release;
};

struct DhMonAssign {                        // step B
    const uint8_t* stats[DH_MON_FRONTS];    // the "frames" rows of the scan engine of a front end; null: not configured
    const uint32_t* stat_count[DH_MON_FRONTS];
    size_t stat_stride[DH_MON_FRONTS];
    const uint32_t* scan_counts; const uint64_t* open_at;
    uint8_t* assigned; uint64_t* start; uint8_t* scan_reset;
    uint8_t* new_flags[DH_MON_PROTOS]; uint64_t* from[DH_MON_PROTOS];        // [B] each; null: not configured
    DhMonSummary* sum;
    uint32_t B, lead, depth, confirm;
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

// `periodic` of pattern i of channel b: from the scan engine of the pattern's front end
DH_HD uint32_t dh_mon_periodic(const DhMonAssign& S, uint32_t b, uint32_t i) {
    const uint32_t f = dh_mon_pattern_front(i);
    if (!S.stats[f] || S.stat_count[f][b] < DH_MON_STAT_BYTES) return 0u;
    const uint32_t* row = (const uint32_t*) (S.stats[f] + (size_t) b * S.stat_stride[f]);      // rows are 64-byte multiples apart
    return row[4u * i + 1u];                                                                // dh_scan_stat: hits, periodic, last_sym, best_dist
}

// Step B for channel b.  Returns the protocol the channel was assigned to in this round (0: none) and its start.
DH_HD uint32_t dh_mon_assign_channel(const DhMonAssign& S, uint32_t b, uint64_t& start) {
    uint32_t won = 0;
    start = DH_PR_NONE;
    if (S.scan_counts[b] != 0u) {
        uint64_t sums[DH_MON_FAMILIES] = { 0, 0, 0, 0, 0 };
        for (uint32_t i = 0; i < 9u; i++) sums[dh_mon_pattern_family(i)] += dh_mon_periodic(S, b, i);
        uint32_t best = 0;
        for (uint32_t f = 1; f < DH_MON_FAMILIES; f++) if (sums[f] > sums[best]) best = f;       // (the first of equal sums)
        const uint32_t p = dh_mon_family_proto(best);
        if (sums[best] >= S.confirm && S.new_flags[p]) {
            const uint64_t open_at = S.open_at[b];
            const uint64_t lo = open_at > S.lead ? open_at - S.lead : 0u;
            const uint64_t oldest = S.total > S.depth ? S.total - S.depth : 0u;
            start = lo > oldest ? lo : oldest;
            won = p;
            S.assigned[b] = (uint8_t) p;
            S.start[b] = start;
        }
    }
    for (uint32_t p = 1; p < DH_MON_PROTOS; p++)
        if (S.new_flags[p]) { S.new_flags[p][b] = won == p ? 1 : 0; S.from[p][b] = won == p ? start : DH_PR_NONE; }
    S.scan_reset[b] = won ? 1 : 0;
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
// ---- host backends of the CPU test harness (engine.hip defines the gfx950 ones) --------------------------------------
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
static int dh_be_monitor_assign(const DhMonAssign& S, void*) {
    for (uint32_t b = S.B; b-- > 0;) {
        uint64_t start;
        const uint32_t p = dh_mon_assign_channel(S, b, start);
        if (p) { S.sum->n_new[p] += 1u; if (start < S.sum->min_start[p]) S.sum->min_start[p] = start; }
    }
    return 0;
}
#endif
