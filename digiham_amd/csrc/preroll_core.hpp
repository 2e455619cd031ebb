// preroll_core.hpp -- the pre-roll ring (include/digiham_amd.h, "Pre-roll"): every channel's last `depth` samples, kept on
// the device so that a channel that has just been named is decoded from where its squelch opened.  Index arithmetic
// shared by the gfx950 build and the CPU test harness, as are the kernels and their launches at the end of this file; no arithmetic on the samples at all -- they move
// as 32-bit words, so NaN payloads, -0 and subnormals arrive as they were sent.
//
// Stream index t of a channel lives at ring[b][t mod depth].  The host knows `total` (the same for every channel), so the
// two positions a launch needs -- where an append starts writing, where the oldest sample sits -- arrive reduced mod depth
// and the kernels wrap with one compare.
#pragma once

#include "../../include/digiham_amd.h"
#include "dh_portable.hpp"

#define DH_PR_NONE 0xFFFFFFFFFFFFFFFFull      /* DH_PREROLL_NONE */
#define DH_PR_TILE 1024u                      /* samples per workgroup: 256 lanes x 4, lane l takes l, l + 256, ... */

struct DhPrAppend {
    uint32_t* ring;             // [B][depth]
    uint64_t* open_at;          // [B]
    const uint32_t* rows;       // the caller's [B][stride] floats, as words, from the first column that is kept
    size_t stride;
    const uint32_t* counts;     // [B] or null (every channel open)
    uint32_t B, depth;
    uint32_t n;                 // samples kept of this append: min(n, depth), the LAST ones of each row
    uint32_t w0;                // ring position of the first of them
    uint64_t base;              // total before the append
};

struct DhPrGather {
    const uint32_t* ring;
    const uint64_t* from;       // [B] device copy of h_from
    uint32_t* out; size_t out_stride;
    uint32_t* counts;           // [B]
    uint32_t B, depth, max_n;
    uint32_t r0;                // ring position of the oldest sample: oldest mod depth
    uint64_t total, oldest, skip;
};

// open_at of channel b after a push that began at stream index base (tile 0 of the channel, one lane)
DH_HD void dh_pr_append_open(const DhPrAppend& A, uint32_t b) {
    const bool open = !A.counts || A.counts[b] != 0;
    if (!open) A.open_at[b] = DH_PR_NONE;
    else if (A.open_at[b] == DH_PR_NONE) A.open_at[b] = A.base;
}

// kept sample i (< A.n) of channel b
DH_HD void dh_pr_append_item(const DhPrAppend& A, uint32_t b, uint32_t i) {
    uint32_t p = A.w0 + i;                                      // w0 < depth, i < n <= depth <= 2^24
    if (p >= A.depth) p -= A.depth;
    A.ring[(size_t) b * A.depth + p] = A.rows[(size_t) b * A.stride + i];
}

DH_HD uint64_t dh_pr_start(uint64_t from, uint64_t oldest) { return from > oldest ? from : oldest; }

// samples channel b delivers, and the ring position `pos` of the first of them
DH_HD uint32_t dh_pr_count(const DhPrGather& G, uint32_t b, uint32_t& pos) {
    pos = 0;
    const uint64_t from = G.from[b];
    if (from == DH_PR_NONE) return 0;
    const uint64_t start = dh_pr_start(from, G.oldest);
    const uint64_t avail = start < G.total ? G.total - start : 0;           // <= depth
    if (G.skip >= avail) return 0;                                          // (start + skip itself may not fit 64 bits)
    const uint64_t left = avail - G.skip;
    pos = G.r0 + (uint32_t) (start + G.skip - G.oldest);                    // r0 < depth, the offset < depth
    if (pos >= G.depth) pos -= G.depth;
    return left < G.max_n ? (uint32_t) left : G.max_n;
}

// output sample i (< count) of channel b
DH_HD void dh_pr_gather_item(const DhPrGather& G, uint32_t b, uint32_t pos, uint32_t i) {
    uint32_t p = pos + i;
    if (p >= G.depth) p -= G.depth;
    G.out[(size_t) b * G.out_stride + i] = G.ring[(size_t) b * G.depth + p];
}

// ---------------------------------------------------------------------------------- pre-roll ring (preroll_core.hpp)
// One workgroup per (1 024-sample tile, channel), blockIdx.y looping over the channels as in k_cz_fm.  Lane l of the 256
// takes samples l, l + 256, l + 512, l + 768 of the tile: every wave instruction moves one contiguous 256-byte piece on
// both sides, except the one piece per tile that may straddle the ring's seam.  The tile-0 workgroup of a channel is
// the only one that touches that channel's open_at (append) or count (gather).
namespace {

__global__ __launch_bounds__(256) void k_preroll_append(const DhPrAppend A) {
    const uint32_t i0 = blockIdx.x * DH_PR_TILE + threadIdx.x;
    for (uint32_t b = blockIdx.y; b < A.B; b += gridDim.y) {
        if (blockIdx.x == 0 && threadIdx.x == 0) dh_pr_append_open(A, b);
#pragma unroll
        for (uint32_t k = 0; k < DH_PR_TILE / 256u; k++) {
            const uint32_t i = i0 + 256u * k;
            if (i < A.n) dh_pr_append_item(A, b, i);
        }
    }
}

__global__ __launch_bounds__(256) void k_preroll_gather(const DhPrGather G) {
    const uint32_t i0 = blockIdx.x * DH_PR_TILE + threadIdx.x;
    for (uint32_t b = blockIdx.y; b < G.B; b += gridDim.y) {
        uint32_t pos;
        const uint32_t count = dh_pr_count(G, b, pos);
        if (blockIdx.x == 0 && threadIdx.x == 0) G.counts[b] = count;
#pragma unroll
        for (uint32_t k = 0; k < DH_PR_TILE / 256u; k++) {
            const uint32_t i = i0 + 256u * k;
            if (i < count) dh_pr_gather_item(G, b, pos, i);
        }
    }
}

}  // namespace

static int dh_be_preroll_append(const DhPrAppend& A, void* stream) {
    if (!A.n) return DH_OK;
    return dh_launch(k_preroll_append, dim3((A.n + DH_PR_TILE - 1) / DH_PR_TILE, A.B < 65535u ? A.B : 65535u), dim3(256), 0, stream, "k_preroll_append", A) ? DH_EDEVICE : DH_OK;
}
static int dh_be_preroll_gather(const DhPrGather& G, void* stream) {
    if (!G.max_n) return DH_OK;
    return dh_launch(k_preroll_gather, dim3((G.max_n + DH_PR_TILE - 1) / DH_PR_TILE, G.B < 65535u ? G.B : 65535u), dim3(256), 0, stream, "k_preroll_gather", G) ? DH_EDEVICE : DH_OK;
}
