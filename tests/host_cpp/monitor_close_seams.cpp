// monitor_close_seams.cpp -- the host back ends of steps A and C of the band monitor (digiham_amd/csrc/monitor_core.hpp:
// the `opened` word, naming on close) over their seam cases, as a stand-alone program meant to be built with
// -fsanitize=address,undefined: one channel, 257 channels (one more than a workgroup of lanes), closing channels at the
// first and the last index, a front end that is not configured.  Every array is a heap block of exactly the size the body
// may touch, so a stray index is an error report.
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

static void round_trip(uint32_t B) {
    const uint32_t first = 0, last = B - 1, n = 4800, release = 2;
    uint64_t* open_at = block<uint64_t>(B, 0xFF);                  // every gate closed
    DhMonOpen A{};
    A.open_at = open_at; A.assigned = block<uint8_t>(B); A.closed_run = block<uint32_t>(B); A.start = block<uint64_t>(B, 0xFF);
    A.opened = block<uint64_t>(B, 0xFF);
    A.scan_reset = block<uint8_t>(B, 0x5A); A.scan_counts = block<uint32_t>(B, 0x5A);
    A.live_counts[DH_PROTO_POCSAG] = block<uint32_t>(B, 0x5A); A.live_counts[DH_PROTO_DSTAR] = block<uint32_t>(B, 0x5A);
    DhMonSummary* sum = block<DhMonSummary>(1);
    A.sum = sum; A.B = B; A.n = n; A.release = release;
    auto fresh = [&] { memset(sum, 0, sizeof(*sum)); for (uint32_t p = 0; p < DH_MON_PROTOS; p++) sum->min_start[p] = DH_PR_NONE; };

    // the scan engines of fsk10 (D-Star) and fsk40i (POCSAG); wide10 and narrow20 are not configured
    DhMonClose C{};
    const size_t stride = 192;
    uint8_t* stats[2] = { block<uint8_t>(B * stride), block<uint8_t>(B * stride) };
    uint32_t* stat_count[2] = { block<uint32_t>(B), block<uint32_t>(B) };
    for (uint32_t k = 0; k < 2; k++) { C.stats[2 + k] = stats[k]; C.stat_count[2 + k] = stat_count[k]; C.stat_stride[2 + k] = stride; }
    C.scan_reset = A.scan_reset; C.opened = A.opened; C.assigned = A.assigned; C.start = A.start;
    for (int p : { DH_PROTO_POCSAG, DH_PROTO_DSTAR }) { C.new_flags[p] = block<uint8_t>(B, 0x5A); C.from[p] = block<uint64_t>(B, 0x5A); }
    C.sum = sum; C.B = B; C.lead = 480; C.depth = 96000;
    const uint32_t hits[5] = { 1, 1, 0, 2, 1 }, dist[5] = { 1, 1, 0, 1, 1 };
    memcpy(C.close_hits, hits, sizeof hits); memcpy(C.close_dist, dist, sizeof dist);

    // round 1: the first and the last channel open at 4800 and 9600 - 1; every other channel closes with nothing seen
    open_at[first] = 4800; open_at[last] = B > 1 ? 9599 : 4800;
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(A.opened[first] == 4800 && A.opened[last] == open_at[last] && sum->n_reset == (B > 2 ? B - 2 : 0u));
    if (B > 2) CHECK(A.opened[1] == DH_PR_NONE && A.scan_reset[1] == 1);
    C.total = 14400;
    CHECK(dh_be_monitor_close(C, nullptr) == 0);                   // closing channels without a statistics row: nobody is named
    for (uint32_t p = 1; p < DH_MON_PROTOS; p++) CHECK(sum->n_new[p] == 0 && sum->min_start[p] == DH_PR_NONE);
    for (uint32_t b = 0; b < B; b++)
        CHECK(A.assigned[b] == 0 && C.new_flags[DH_PROTO_POCSAG][b] == 0 && C.from[DH_PROTO_DSTAR][b] == DH_PR_NONE);

    // round 2: both close.  First: one POCSAG hit at distance 1.  Last: two D-Star hits (header and voice) at distance 0
    // and 1 -- and, where they are one channel, D-Star's larger H wins.  Distance 2 would not do (checked on a copy below).
    dh_scan_stat* pf = (dh_scan_stat*) (stats[1] + first * stride);
    dh_scan_stat* dl = (dh_scan_stat*) (stats[0] + last * stride);
    for (uint32_t k = 0; k < 2; k++)
        for (uint32_t b : { first, last })
            for (uint32_t i = 0; i < DH_SCAN_PATTERNS; i++) ((dh_scan_stat*) (stats[k] + b * stride))[i].best_dist = 255;
    pf[DH_SCAN_POCSAG].hits = 1; pf[DH_SCAN_POCSAG].best_dist = 1;
    dl[DH_SCAN_DSTAR_HEADER].hits = 1; dl[DH_SCAN_DSTAR_HEADER].best_dist = 0; dl[DH_SCAN_DSTAR_VOICE].hits = 1; dl[DH_SCAN_DSTAR_VOICE].best_dist = 1;
    stat_count[0][first] = stat_count[1][first] = stat_count[0][last] = stat_count[1][last] = DH_MON_STAT_BYTES;
    open_at[first] = open_at[last] = DH_PR_NONE;
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(sum->n_reset == (B > 1 ? 2u : 1u) && A.scan_reset[first] == 1 && A.scan_reset[last] == 1 && A.opened[first] == 4800);
    C.total = 19200;
    CHECK(dh_be_monitor_close(C, nullptr) == 0);
    if (B > 1) {
        CHECK(A.assigned[first] == DH_PROTO_POCSAG && A.start[first] == 4800 - 480 && C.new_flags[DH_PROTO_POCSAG][first] == 1);
        CHECK(C.from[DH_PROTO_POCSAG][first] == 4320 && C.from[DH_PROTO_DSTAR][first] == DH_PR_NONE && sum->n_new[DH_PROTO_POCSAG] == 1);
        CHECK(A.assigned[last] == DH_PROTO_DSTAR && A.start[last] == 9599 - 480 && C.new_flags[DH_PROTO_DSTAR][last] == 1 && C.new_flags[DH_PROTO_POCSAG][last] == 0);
        CHECK(sum->n_new[DH_PROTO_DSTAR] == 1 && sum->min_start[DH_PROTO_DSTAR] == 9119 && sum->min_start[DH_PROTO_POCSAG] == 4320);
    } else {
        CHECK(A.assigned[first] == DH_PROTO_DSTAR && A.start[first] == 4320 && sum->n_new[DH_PROTO_DSTAR] == 1 && sum->n_new[DH_PROTO_POCSAG] == 0);
    }
    CHECK(A.scan_reset[first] == 1 && A.scan_reset[last] == 1 && A.closed_run[first] == 1);                  // as step A left them
    if (B > 2) CHECK(A.assigned[1] == 0 && C.new_flags[DH_PROTO_POCSAG][1] == 0 && C.from[DH_PROTO_POCSAG][1] == DH_PR_NONE);

    // rounds 3 and 4: closed; released in the second closed round, `opened` stays
    fresh();
    CHECK(dh_be_monitor_open(A, nullptr) == 0);
    CHECK(A.assigned[first] == 0 && A.assigned[last] == 0 && A.start[first] == DH_PR_NONE && sum->n_reset == 0 && A.opened[first] == 4800);

    // a best distance above the limit, a short row, too few hits: nobody is named; the ring's reach bounds the start
    open_at[first] = 100; fresh(); CHECK(dh_be_monitor_open(A, nullptr) == 0);
    open_at[first] = DH_PR_NONE; fresh(); CHECK(dh_be_monitor_open(A, nullptr) == 0);
    C.total = 200000;
    if (B > 1) {
        pf[DH_SCAN_POCSAG].best_dist = 2;
        CHECK(dh_be_monitor_close(C, nullptr) == 0 && A.assigned[first] == 0);
        pf[DH_SCAN_POCSAG].best_dist = 0; stat_count[1][first] = DH_MON_STAT_BYTES - 1;
        CHECK(dh_be_monitor_close(C, nullptr) == 0 && A.assigned[first] == 0);
        stat_count[1][first] = DH_MON_STAT_BYTES;
        CHECK(dh_be_monitor_close(C, nullptr) == 0 && A.assigned[first] == DH_PROTO_POCSAG && A.start[first] == 200000 - 96000);
    } else {
        dl[DH_SCAN_DSTAR_VOICE].hits = 0;
        CHECK(dh_be_monitor_close(C, nullptr) == 0 && A.assigned[first] == DH_PROTO_POCSAG && A.start[first] == 200000 - 96000);
    }

    for (void* p : { (void*) open_at, (void*) A.assigned, (void*) A.closed_run, (void*) A.start, (void*) A.opened, (void*) A.scan_reset,
                     (void*) A.scan_counts, (void*) A.live_counts[DH_PROTO_POCSAG], (void*) A.live_counts[DH_PROTO_DSTAR], (void*) sum,
                     (void*) stats[0], (void*) stats[1], (void*) stat_count[0], (void*) stat_count[1], (void*) C.new_flags[DH_PROTO_POCSAG],
                     (void*) C.new_flags[DH_PROTO_DSTAR], (void*) C.from[DH_PROTO_POCSAG], (void*) C.from[DH_PROTO_DSTAR] })
        free(p);
}

int main() {
    for (uint32_t B : { 1u, 257u }) round_trip(B);
    printf(failures ? "monitor close seams: %d checks failed\n" : "monitor close seams: clean\n", failures);
    return failures ? 1 : 0;
}
