// plan_test.cpp -- the routes of digiham_amd/csrc/launch_plan.hpp against a table written out by hand.
//
// Which instantiation served a push cannot be seen through the ABI (two launches and one chained launch give the same
// bytes), so the plan itself is asked: for every (nz, sps, fast, proto, levels, filt_out) an engine can hand to a backend
// (engine_impl.hpp, make_layout) a recording callable notes the tag it was called with, and the note is compared with the
// first matching row below (-1 = any; no row = no instantiation).  A route that changes in launch_plan.hpp changes here
// too: this is the one place where that has to be done twice.  Also here: the host-visible pieces of the tail split
// (digiham_amd/csrc/chain_core.hpp) -- the locator, the bounds, the flag word and its merge, the parameters of a split launch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../digiham_amd/csrc/chain_core.hpp"

namespace {

struct Row { int proto, levels, nz, fast, sps, keep; const char* route; };

// chain<NZ,FAST,PROTO,SPS,MAY_SPLIT;LV>; anything not listed runs as two launches (dh_plan_chain returns 1)
const Row CHAIN[] = {
    { DH_PROTO_DMR, 4, 0, -1, 10, -1, "chain<0,0,1,10,0;4>" },          // fsk / unfiltered input | dmr_decoder
    { DH_PROTO_DMR, 4, 80, 1, 10, -1, "chain<80,1,1,10,0;4>" },         // DH_FLAG_FAST_FIR
    { DH_PROTO_DMR, 4, 80, 0, 10, -1, "chain<80,0,1,10,1;4>" },         // the headline pipe: split
    { DH_PROTO_YSF, 4, 0, -1, 10, -1, "chain<0,0,2,10,0;4>" },
    { DH_PROTO_YSF, 4, 80, 1, 10, -1, "chain<80,1,2,10,0;4>" },
    { DH_PROTO_YSF, 4, 80, 0, 10, -1, "chain<80,0,2,10,1;4>" },
    { DH_PROTO_NXDN, 4, 160, 0, 20, -1, "chain<160,0,3,20,1;4>" },      // NXDN48
    { DH_PROTO_NXDN, 4, 160, 0, -1, -1, "chain<160,0,3,0,1;4>" },       // any other samples-per-symbol
    { DH_PROTO_DSTAR, 2, 0, -1, 10, -1, "chain<0,0,5,10,1;2>" },
    // POCSAG, the wrong number of levels, any other filter / rate: two launches
};
// demod<NZ,FAST,SPS,KEEPF>; keep = 0 no filt_out, 1 filt_out (`fast` then chooses KEEPF 2); does not look at proto / levels
const Row DEMOD[] = {
    { -1, -1, 80, 0, 10, 1, "demod<80,0,10,1>" },
    { -1, -1, 80, 1, 10, 1, "demod<80,0,10,2>" },
    { -1, -1, -1, -1, -1, 1, "none" },                                  // filtered samples from the slicer: <80, 10> only
    { -1, -1, 0, -1, 10, 0, "demod<0,0,10,0>" },
    { -1, -1, 80, 0, 10, 0, "demod<80,0,10,0>" },
    { -1, -1, 80, 1, 10, 0, "demod<80,1,10,0>" },
    { -1, -1, 0, -1, 40, 0, "demod<0,0,40,0>" },                        // POCSAG
    { -1, -1, 160, 0, 20, 0, "demod<160,0,20,0>" },                     // NXDN48
    { -1, -1, 0, -1, -1, 0, "demod<0,0,0,0>" },
    { -1, -1, 80, 0, -1, 0, "demod<80,0,0,0>" },
    { -1, -1, 80, 1, -1, 0, "demod<80,1,0,0>" },
    { -1, -1, 160, 0, -1, 0, "demod<160,0,0,0>" },
    { -1, -1, 160, 1, -1, 0, "demod<160,1,0,0>" },
};
const Row TILES[] = {
    { -1, -1, 80, 0, -1, -1, "tiles<80,0>" }, { -1, -1, 80, 1, -1, -1, "tiles<80,1>" },
    { -1, -1, 160, 0, -1, -1, "tiles<160,0>" }, { -1, -1, 160, 1, -1, -1, "tiles<160,1>" },
};

template <size_t N> const char* expect(const Row (&rows)[N], int proto, int levels, int nz, int fast, int sps, int keep) {
    for (const Row& r : rows)
        if ((r.proto < 0 || r.proto == proto) && (r.levels < 0 || r.levels == levels) && (r.nz < 0 || r.nz == nz) &&
            (r.fast < 0 || r.fast == fast) && (r.sps < 0 || r.sps == sps) && (r.keep < 0 || r.keep == keep)) return r.route;
    return "none";
}

struct Recorder {
    std::string got = "none";
    template <int NZ, bool FAST, int SPS, int KEEPF> int operator()(DhDemodInst<NZ, FAST, SPS, KEEPF>) {
        char b[64]; snprintf(b, sizeof b, "demod<%d,%d,%d,%d>", NZ, (int) FAST, SPS, KEEPF); got = b; return 0;
    }
    template <int NZ, bool FAST, int PROTO, int SPS, bool SPLIT> int operator()(DhChainInst<NZ, FAST, PROTO, SPS, SPLIT> i) {
        char b[64]; snprintf(b, sizeof b, "chain<%d,%d,%d,%d,%d;%d>", NZ, (int) FAST, PROTO, SPS, (int) SPLIT, decltype(i)::LV); got = b; return 0;
    }
    template <int NZ, bool FAST> int operator()(DhTilesInst<NZ, FAST>) {
        char b[64]; snprintf(b, sizeof b, "tiles<%d,%d>", NZ, (int) FAST); got = b; return 0;
    }
};

int failures = 0;
void check(bool ok, const char* what) { if (!ok) { failures++; fprintf(stderr, "FAIL %s\n", what); } }
void compare(const std::string& got, int rc, const char* want, int rc_none, const char* what, int proto, int levels, int nz, int fast, int sps, int keep) {
    const bool none = !strcmp(want, "none");
    if (got == want && rc == (none ? rc_none : 0)) return;
    failures++;
    fprintf(stderr, "FAIL %s proto %d levels %d nz %d fast %d sps %d filt_out %d: got %s (rc %d), table says %s\n", what, proto, levels, nz, fast, sps, keep, got.c_str(), rc, want);
}

}  // namespace

int main() {
    float dummy = 0.0f;
    int routes = 0;
    // make_layout: nz = 0 (no fused filter), 80 (wide), 160 (narrow); sps 3 .. DH_MAX_SPS; levels = 2 / 4; every protocol
    for (int nz : { 0, 80, 160 }) for (int sps = 3; sps <= DH_MAX_SPS; sps++) for (int fast = 0; fast < 2; fast++) {
        for (int keep = 0; keep < 2; keep++) {
            DhDspParams P{}; P.sps = (uint32_t) sps; P.filt_out = keep ? &dummy : nullptr;
            Recorder r;
            const int rc = dh_plan_rrc_demod(P, (uint32_t) nz, fast != 0, r);
            compare(r.got, rc, expect(DEMOD, -1, -1, nz, fast, sps, keep), -1, "dh_plan_rrc_demod", 0, 0, nz, fast, sps, keep);
            routes++;
        }
        for (int proto = DH_PROTO_DMR; proto <= DH_PROTO_DSTAR; proto++) for (int levels : { 2, 4 }) {
            DhDspParams P{}; P.sps = (uint32_t) sps; P.levels = (uint32_t) levels;
            Recorder r;
            const int rc = dh_plan_chain(P, (uint32_t) nz, fast != 0, proto, r);
            compare(r.got, rc, expect(CHAIN, proto, levels, nz, fast, sps, -1), 1, "dh_plan_chain", proto, levels, nz, fast, sps, 0);
            routes++;
        }
    }
    for (int nz : { 0, 37, 80, 160 }) for (int fast = 0; fast < 2; fast++) {
        Recorder r;
        const int rc = dh_plan_rrc_tiles((uint32_t) nz, fast != 0, r);
        compare(r.got, rc, expect(TILES, -1, -1, nz, fast, -1, -1), -1, "dh_plan_rrc_tiles", 0, 0, nz, fast, 0, 0);
        routes++;
    }

    // the tail split's grammar and bounds
    const struct { const char* text; bool set; uint32_t pct, pct2; } ENV[] = {
        { nullptr, false, 0, 0 }, { "80", true, 80, 0 }, { "75,93", true, 75, 93 }, { "0", true, 0, 0 }, { "100", true, 0, 0 },
        { "93,75", true, 93, 0 }, { "40,100", true, 40, 0 }, { "x", true, 0, 0 },
    };
    for (const auto& e : ENV) {
        if (e.text) setenv("DH_TAIL_SPLIT", e.text, 1); else unsetenv("DH_TAIL_SPLIT");
        unsetenv("DH_TAIL_SPLIT_FORCE_FAIL");
        const DhTailSplitEnv E = dh_tail_split_env();
        check(E.set == e.set && E.pct == e.pct && E.pct2 == e.pct2 && E.force_fail == 0u, e.text ? e.text : "(DH_TAIL_SPLIT unset)");
    }
    setenv("DH_TAIL_SPLIT_FORCE_FAIL", "3", 1);
    check(dh_tail_split_env().force_fail == 3u, "DH_TAIL_SPLIT_FORCE_FAIL");
    uint32_t n0, n1;
    dh_tail_split_points(70000u, 80u, 0u, n0, n1);
    check(n0 == 56000u && n1 == 0u, "points 80");
    check(dh_part_lo(0, n0, n1) == 0u && dh_part_hi(0, n0, n1) == 56000u && dh_part_lo(1, n0, n1) == 56000u && dh_part_hi(1, n0, n1) == 0xFFFFFFFFu, "two parts");
    dh_tail_split_points(70000u, 75u, 93u, n0, n1);
    check(n0 == 52500u && n1 == 65100u, "points 75,93");
    check(dh_part_hi(0, n0, n1) == 52500u && dh_part_lo(1, n0, n1) == 52500u && dh_part_hi(1, n0, n1) == 65100u &&
          dh_part_lo(2, n0, n1) == 65100u && dh_part_hi(2, n0, n1) == 0xFFFFFFFFu, "three parts");
    dh_tail_split_points(0xFFFFFFFFu, 99u, 0u, n0, n1);
    check(n0 == 4252017622u, "points: 64-bit product");

    // which part of which channel a block of a split launch is; the blocks between the parts are padding
    const struct { uint32_t channels, pad; } GRIDS[] = { { 1, 8 }, { 7, 8 }, { 8, 8 }, { 9, 16 } };
    for (const auto& g : GRIDS) for (uint32_t parts = 2; parts <= 3; parts++) {
        DhDspParams Q{}; Q.n = 1000u; Q.n_channels = g.channels; Q.ch_base = 0u;
        uint32_t epoch = 41u;
        const DhSplitGrids G = dh_plan_split(Q, 40u, parts == 3 ? 90u : 0u, epoch, 5u);
        check(Q.split_pad == g.pad && Q.split_pad % 8u == 0u && Q.split_pad >= g.channels, "pad: the next multiple of 8");
        check(G.split == (parts - 1u) * g.pad + g.channels && G.fixup == g.channels, "grids of the split and the fix-up launch");
        check(Q.split_n0 == 400u && Q.split_n1 == (parts == 3 ? 900u : 0u) && Q.part_epoch == 42u && epoch == 42u &&
              Q.split_force_fail == 5u && Q.split_fixup == 0u, "parameters of a split launch");
        uint32_t real = 0;
        for (uint32_t bid = 0; bid < G.split; bid++) {
            const DhBlockPart B = dh_part_of_block(Q, bid);
            const uint32_t part = bid / g.pad, local = bid % g.pad;       // (no block lies beyond the last part's channels)
            check(B.part == part && B.bid == local && B.padding == (local >= g.channels), "dh_part_of_block");
            real += B.padding ? 0u : 1u;
        }
        check(real == parts * g.channels, "every part of every channel has one block");
        Q.split_fixup = 1u;                                             // the fix-up launch: block b is channel b
        for (uint32_t bid = 0; bid < G.fixup; bid++) {
            const DhBlockPart B = dh_part_of_block(Q, bid);
            check(B.part == 0u && B.bid == bid && !B.padding, "dh_part_of_block (fix-up)");
        }
    }
    {   // (the harness's pushes: a first part of at least one sample, a third not in front of the second)
        DhDspParams Q{}; Q.n = 2u; Q.n_channels = 4u;
        uint32_t epoch = 0u;
        const DhSplitGrids G = dh_plan_split(Q, 1u, 40u, epoch, 0u);
        check(Q.split_n0 == 1u && Q.split_n1 == 1u && G.split == 20u && epoch == 1u, "bounds of a two-sample push");
    }
    // the epoch: 24 bits, never 0
    check(dh_next_epoch(0u) == 1u && dh_next_epoch(1u) == 2u && dh_next_epoch(0x00FFFFFDu) == 0x00FFFFFEu && dh_next_epoch(0x00FFFFFEu) == 1u, "epoch step");
    // the flag word
    for (uint32_t epoch : { 1u, 0x00ABCDEFu, 0x00FFFFFEu }) for (uint32_t part = 0; part < 3; part++) for (uint32_t xcc = 0; xcc < 16; xcc++) {
        const uint32_t v = dh_pf_pack(epoch, part, xcc);
        check(dh_pf_of_push(v, epoch) && !dh_pf_of_push(v, dh_next_epoch(epoch)) && dh_pf_done(v) == part + 1u && dh_pf_xcc(v) == xcc &&
              !(v & DH_PF_GAVE_UP), "flag word round trip");
        check(dh_pf_of_push(v | DH_PF_GAVE_UP, epoch) && dh_pf_done(v | DH_PF_GAVE_UP) == part + 1u && dh_pf_xcc(v | DH_PF_GAVE_UP) == xcc, "flag word with the give-up bit");
    }
    {   // its merge, both keep rules, on a word of this push (epoch 7) and on words of older pushes
        const uint32_t E = 7u, gave_up = E | DH_PF_GAVE_UP;
        const uint32_t done1 = dh_pf_pack(E, 0u, 5u), old = dh_pf_pack(6u, 1u, 3u) | DH_PF_GAVE_UP;
        uint32_t w;
        // the give-up write: the whole word of this push stays, an older one is replaced by the bare epoch
        w = done1; dh_pf_publish(&w, E, gave_up, 0xFFFFFFFFu); check(w == (done1 | DH_PF_GAVE_UP), "give-up on a word of this push");
        w = old; dh_pf_publish(&w, E, gave_up, 0xFFFFFFFFu); check(w == gave_up, "give-up on a word of an older push");
        w = 0u; dh_pf_publish(&w, E, gave_up, 0xFFFFFFFFu); check(w == gave_up, "give-up on a fresh word");
        // the done write: only the give-up bit of a word of this push stays
        const uint32_t done2 = dh_pf_pack(E, 1u, 2u);
        w = done1; dh_pf_publish(&w, E, done2, DH_PF_GAVE_UP); check(w == done2, "done over a done word of this push");
        w = done1 | DH_PF_GAVE_UP; dh_pf_publish(&w, E, done2, DH_PF_GAVE_UP); check(w == (done2 | DH_PF_GAVE_UP), "done keeps the give-up bit of this push");
        w = gave_up; dh_pf_publish(&w, E, done1, DH_PF_GAVE_UP); check(w == (done1 | DH_PF_GAVE_UP), "done behind an early give-up");
        w = old; dh_pf_publish(&w, E, done1, DH_PF_GAVE_UP); check(w == done1, "done drops everything of an older push");
    }

    printf("%d routes checked, %d failures\n", routes, failures);
    return failures ? 1 : 0;
}
