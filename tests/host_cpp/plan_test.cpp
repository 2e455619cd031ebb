// plan_test.cpp -- the routes of digiham_amd/csrc/launch_plan.hpp against a table written out by hand.
//
// Which instantiation served a push cannot be seen through the ABI (two launches and one chained launch give the same
// bytes), so the plan itself is asked: for every (nz, sps, fast, proto, levels, filt_out) an engine can hand to a backend
// (engine_impl.hpp, make_layout) a recording callable notes the tag it was called with, and the note is compared with the
// first matching row below (-1 = any; no row = no instantiation).  A route that changes in launch_plan.hpp changes here
// too: this is the one place where that has to be done twice.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../digiham_amd/csrc/launch_plan.hpp"

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

    printf("%d routes checked, %d failures\n", routes, failures);
    return failures ? 1 : 0;
}
