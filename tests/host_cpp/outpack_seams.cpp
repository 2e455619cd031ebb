// outpack_seams.cpp -- the host back ends of the packed read-out's two kernel bodies (digiham_amd/csrc/outpack_core.hpp:
// the scan, the copy) over their seam cases, as a stand-alone program meant to be built with
// -fsanitize=address,undefined: one channel, 257 channels (one more than a pass of the scan covers), busy channels at the
// first and the last channel and on both sides of every wavefront boundary, capacities that end exactly at the last kept
// byte.  Every array is a heap block of exactly the size the bodies may touch, so a stray index is an error report.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/digiham_amd.h"
#include "../../digiham_amd/csrc/outpack_core.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

template <class T> static T* block(size_t n, int fill = 0) {
    T* p = (T*) malloc(sizeof(T) * (n ? n : 1));       // (a capacity of 0 is an area nobody may touch: one byte that stays as it is)
    memset(p, fill, sizeof(T) * (n ? n : 1));
    return p;
}

struct NoBackend {};

struct Cand { uint32_t b, fc, ec; };

// `keep` candidates fit exactly; the areas end at the last kept byte
static void run(uint32_t B, const std::vector<Cand>& busy, size_t keep, bool with_mask) {
    const uint32_t out_cap = 64, ev_cap = 2;
    uint8_t* rows = block<uint8_t>((size_t) B * out_cap);
    for (size_t i = 0; i < (size_t) B * out_cap; i++) rows[i] = (uint8_t) (i * 7u) | 1u;      // no byte of a row is 0
    dh_event* evs = block<dh_event>((size_t) B * ev_cap, 0xEE);
    uint32_t* fc = block<uint32_t>(B); uint32_t* ec = block<uint32_t>(B); uint32_t* mask = block<uint32_t>(B); uint64_t* tag = block<uint64_t>(B);
    for (uint32_t b = 0; b < B; b++) { tag[b] = 1000u + b; fc[b] = with_mask ? 9u : 0u; ec[b] = 0; }       // (masked-out channels are busy)
    for (const Cand& c : busy) { fc[c.b] = c.fc; ec[c.b] = c.ec; mask[c.b] = 1; }
    uint64_t nf = 0; uint32_t nv = 0;
    for (size_t k = 0; k < keep; k++) { nf += dh_op_pad16(busy[k].fc); nv += busy[k].ec; }

    DhOutpack P{};
    P.hdr = block<dh_outpack_header>(1); P.scratch = block<uint32_t>(2, 0x5A);
    P.entries = block<dh_outpack_entry>(keep, 0x5A); P.events = block<dh_event>(nv, 0x5A); P.frames = block<uint8_t>((size_t) nf, 0x5A);
    P.max_entries = (uint32_t) keep; P.max_events = nv; P.max_frame_bytes = nf;
    P.src_frames = rows; P.src_fc = fc; P.out_cap = out_cap; P.src_events = evs; P.src_ec = ec; P.ev_cap = ev_cap;
    P.mask = with_mask ? mask : nullptr; P.tag = tag; P.tag_add = ~(uint64_t) 0; P.user = 77; P.B = B;
    NoBackend be;
    CHECK(dh_be_outpack_scan(be, P) == 0 && dh_be_outpack_copy(be, P) == 0);
    CHECK(P.hdr->n_entries == keep && P.hdr->n_events == nv && P.hdr->frame_bytes == nf && P.hdr->appends == 1);
    CHECK(P.hdr->dropped == busy.size() - keep && P.hdr->reserved[0] == 0 && P.hdr->reserved[1] == 0);
    CHECK(P.scratch[0] == 0 && P.scratch[1] == keep);
    uint64_t F = 0; uint32_t V = 0;
    for (size_t k = 0; k < keep; k++) {
        const Cand& c = busy[k];
        const dh_outpack_entry& en = P.entries[k];
        CHECK(en.channel == c.b && en.user == 77 && en.tag == 999u + c.b && en.n_frame_bytes == c.fc && en.n_events == c.ec);
        CHECK(en.frame_offset16 == F / 16 && en.event_index == V);
        CHECK(memcmp(P.frames + F, rows + (size_t) c.b * out_cap, c.fc) == 0);
        for (uint64_t i = F + c.fc; i < F + dh_op_pad16(c.fc); i++) CHECK(P.frames[i] == 0);
        if (c.ec) CHECK(memcmp(P.events + V, evs + (size_t) c.b * ev_cap, sizeof(dh_event) * c.ec) == 0);
        F += dh_op_pad16(c.fc); V += c.ec;
    }
    // a second append onto the full pack: everything is dropped, nothing is written
    const uint32_t more = (uint32_t) busy.size();
    CHECK(dh_be_outpack_scan(be, P) == 0 && dh_be_outpack_copy(be, P) == 0);
    CHECK(P.hdr->n_entries == keep && P.hdr->n_events == nv && P.hdr->frame_bytes == nf && P.hdr->appends == 2);
    CHECK(P.hdr->dropped == busy.size() - keep + more && P.scratch[0] == keep && P.scratch[1] == 0);
    for (void* p : { (void*) rows, (void*) evs, (void*) fc, (void*) ec, (void*) mask, (void*) tag, (void*) P.hdr, (void*) P.scratch,
                     (void*) P.entries, (void*) P.events, (void*) P.frames })
        free(p);
}

int main() {
    // fc = 5: a masked last piece; 16 and 64: whole pieces only (64: the whole row); 0 with events; 33 without events
    const std::vector<Cand> one = { { 0, 5, 2 } };
    const std::vector<Cand> many = { { 0, 5, 2 }, { 63, 16, 1 }, { 64, 0, 2 }, { 127, 64, 0 }, { 128, 33, 1 }, { 191, 1, 0 }, { 192, 15, 2 },
                                     { 255, 17, 1 }, { 256, 64, 2 } };
    for (bool with_mask : { false, true }) {
        run(1, one, 1, with_mask);
        run(257, many, many.size(), with_mask);
        run(257, many, many.size() - 1, with_mask);     // the channel behind the pass boundary is the one that does not fit
        run(257, many, 4, with_mask);
    }
    printf(failures ? "outpack seams: %d checks failed\n" : "outpack seams: clean\n", failures);
    return failures ? 1 : 0;
}
