// monitor_seams.cpp -- the host back ends of the band monitor's three kernel bodies (digiham_amd/csrc/monitor_core.hpp:
// step A, step B, the masked reset) over their seam cases, as a stand-alone program meant to be built with
// -fsanitize=address,undefined: one channel, 257 channels (one more than a workgroup of lanes), flags at the first and the
// last channel.  Every array is a heap block of exactly the size the body may touch, so a stray index is an error report.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/digiham_amd.h"
#include "../../digiham_amd/csrc/kernels_core.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

template <class T> static T* block(size_t n, int fill = 0) {
    T* p = (T*) malloc(sizeof(T) * n);
    memset(p, fill, sizeof(T) * n);
    return p;
}

struct NoBackend {};

static void round_trip(uint32_t B) {
    const uint32_t first = 0, last = B - 1, n = 4800, release = 2;
    uint64_t* open_at = block<uint64_t>(B, 0xFF);                  // every gate closed
    DhMonOpen A{};
    A.open_at = open_at; A.assigned = block<uint8_t>(B); A.closed_run = block<uint32_t>(B); A.start = block<uint64_t>(B, 0xFF);
    A.scan_reset = block<uint8_t>(B, 0x5A); A.scan_counts = block<uint32_t>(B, 0x5A);
    A.live_counts[DH_PROTO_DMR] = block<uint32_t>(B, 0x5A); A.live_counts[DH_PROTO_YSF] = block<uint32_t>(B, 0x5A);
    DhMonSummary* sum = block<DhMonSummary>(1);
    A.sum = sum; A.B = B; A.n = n; A.release = release;
    auto fresh = [&] { memset(sum, 0, sizeof(*sum)); for (uint32_t p = 0; p < DH_MON_PROTOS; p++) sum->min_start[p] = DH_PR_NONE; };

    // round 1: the first and the last channel open at 100, everything else closes for the first time
    open_at[first] = 100; open_at[last] = 100;
    A.closed_run[last] = DH_MON_RUN_MAX;                           // (an open round clears a saturated run)
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(sum->n_scan == (B > 1 ? 2u : 1u) && sum->n_reset == (B > 2 ? B - 2 : 0u));
    CHECK(A.scan_counts[first] == n && A.scan_counts[last] == n && A.closed_run[last] == 0 && A.scan_reset[first] == 0);
    if (B > 2) CHECK(A.scan_counts[1] == 0 && A.scan_reset[1] == 1 && A.closed_run[1] == 1 && A.live_counts[DH_PROTO_DMR][1] == 0);

    // step B: DMR statistics for the first channel, YSF for the last (where they are one channel, DMR: the first family of a tie)
    DhMonAssign S{};
    const size_t stride = 192;
    uint8_t* stats = block<uint8_t>(B * stride);
    uint32_t* stat_count = block<uint32_t>(B);
    S.stats[0] = stats; S.stat_count[0] = stat_count; S.stat_stride[0] = stride;
    S.scan_counts = A.scan_counts; S.open_at = open_at; S.assigned = A.assigned; S.start = A.start; S.scan_reset = A.scan_reset;
    for (int p : { DH_PROTO_DMR, DH_PROTO_YSF }) { S.new_flags[p] = block<uint8_t>(B, 0x5A); S.from[p] = block<uint64_t>(B, 0x5A); }
    S.sum = sum; S.B = B; S.lead = 480; S.depth = 24000; S.confirm = 2; S.total = 30000;
    dh_scan_stat* st0 = (dh_scan_stat*) (stats + first * stride);
    dh_scan_stat* st1 = (dh_scan_stat*) (stats + last * stride);
    st1[DH_SCAN_YSF].periodic = 2;
    st0[DH_SCAN_DMR_BS_DATA].periodic = 1; st0[DH_SCAN_DMR_MS_VOICE].periodic = 1;
    stat_count[first] = stat_count[last] = DH_MON_STAT_BYTES;
    fresh();
    CHECK(dh_be_monitor_assign(S, nullptr) == 0);
    const uint64_t start = 30000 - 24000;                          // the ring does not reach back to 100 - 480
    CHECK(A.assigned[first] == DH_PROTO_DMR && A.start[first] == start && S.new_flags[DH_PROTO_DMR][first] == 1 && S.from[DH_PROTO_DMR][first] == start);
    CHECK(sum->n_new[DH_PROTO_DMR] == 1 && sum->min_start[DH_PROTO_DMR] == start && A.scan_reset[first] == 1);
    if (B > 1) {
        CHECK(A.assigned[last] == DH_PROTO_YSF && S.from[DH_PROTO_YSF][last] == start && S.from[DH_PROTO_DMR][last] == DH_PR_NONE);
        CHECK(sum->n_new[DH_PROTO_YSF] == 1 && S.new_flags[DH_PROTO_DMR][last] == 0 && S.new_flags[DH_PROTO_YSF][first] == 0);
    }
    if (B > 2) CHECK(A.assigned[1] == 0 && A.scan_reset[1] == 0 && S.new_flags[DH_PROTO_DMR][1] == 0 && S.from[DH_PROTO_YSF][1] == DH_PR_NONE);

    // round 2: both are live; rounds 3 and 4: closed, released in the second closed round
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(sum->n_scan == 0 && sum->n_live[DH_PROTO_DMR] == 1 && A.live_counts[DH_PROTO_DMR][first] == n);
    if (B > 1) CHECK(sum->n_live[DH_PROTO_YSF] == 1 && A.live_counts[DH_PROTO_YSF][last] == n && A.live_counts[DH_PROTO_DMR][last] == 0);
    open_at[first] = open_at[last] = DH_PR_NONE;
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(A.assigned[first] == DH_PROTO_DMR && A.closed_run[first] == 1 && sum->n_live[DH_PROTO_DMR] == 0 && sum->n_reset == 0);
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(A.assigned[first] == 0 && A.assigned[last] == 0 && A.start[first] == DH_PR_NONE && A.start[last] == DH_PR_NONE && sum->n_reset == 0);

    for (void* p : { (void*) open_at, (void*) A.assigned, (void*) A.closed_run, (void*) A.start, (void*) A.scan_reset, (void*) A.scan_counts,
                     (void*) A.live_counts[DH_PROTO_DMR], (void*) A.live_counts[DH_PROTO_YSF], (void*) sum, (void*) stats, (void*) stat_count,
                     (void*) S.new_flags[DH_PROTO_DMR], (void*) S.new_flags[DH_PROTO_YSF], (void*) S.from[DH_PROTO_DMR], (void*) S.from[DH_PROTO_YSF] })
        free(p);
}

static void masked_reset(uint32_t B) {
    const uint32_t state_words = 48, rows[3] = { 64, 4, 20 };      // a 16-byte row, a counter, a row of words that is no multiple of 16
    DhResetChannels R{};
    uint8_t* flags = block<uint8_t>(B);
    flags[0] = 1; flags[B - 1] = 1;
    R.flags = flags; R.B = B;
    for (uint32_t k = 0; k < 3; k++) { R.buf[k].p = block<uint8_t>((size_t) B * rows[k], 0xA5); R.buf[k].row_bytes = rows[k]; }
    R.dsp_state = block<uint32_t>((size_t) B * state_words, 0xA5); R.state_words = state_words; R.tail0 = 80;
    R.dec_state = block<uint32_t>((size_t) B * DH_DEC_STATE_WORDS, 0xA5); R.slot_filter = 3;
    R.buf[3].p = R.dsp_state; R.buf[3].row_bytes = state_words * 4; R.buf[4].p = R.dec_state; R.buf[4].row_bytes = DH_DEC_STATE_WORDS * 4;
    R.n_bufs = 5;
    NoBackend be;
    CHECK(dh_be_reset_channels(be, R) == 0);
    for (uint32_t b = 0; b < B; b++) {
        const bool hit = b == 0 || b == B - 1;
        for (uint32_t k = 0; k < 3; k++)
            for (uint32_t i = 0; i < rows[k]; i++) CHECK(((uint8_t*) R.buf[k].p)[(size_t) b * rows[k] + i] == (hit ? 0 : 0xA5));
        const uint32_t* s = R.dsp_state + (size_t) b * state_words;
        const uint32_t* d = R.dec_state + (size_t) b * DH_DEC_STATE_WORDS;
        for (uint32_t i = 0; i < state_words; i++) CHECK(s[i] == (hit ? (i == DH_ST_TAIL ? 80u : 0u) : 0xA5A5A5A5u));
        for (uint32_t i = 0; i < DH_DEC_STATE_WORDS; i++)
            CHECK(d[i] == (hit ? (i == DS_SLOT_FILTER || i == DS_SLOT_FILTER_DECODER ? 3u : 0u) : 0xA5A5A5A5u));
    }
    for (uint32_t k = 0; k < 3; k++) free(R.buf[k].p);
    free(flags); free(R.dsp_state); free(R.dec_state);
}

int main() {
    for (uint32_t B : { 1u, 257u }) { round_trip(B); masked_reset(B); }
    printf(failures ? "monitor seams: %d checks failed\n" : "monitor seams: clean\n", failures);
    return failures ? 1 : 0;
}
