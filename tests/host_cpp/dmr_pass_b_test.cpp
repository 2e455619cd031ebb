// dmr_pass_b_test.cpp -- the lane-parallel pass B of the DMR decoder (dh_dmr_pass_b_lanes) against the burst-serial one
// (dh_dmr_pass_b), which is its definition.  Stand-alone: g++ -std=c++17 -O2 tests/host_cpp/dmr_pass_b_test.cpp && ./a.out
// (it may be built with -fsanitize=address,undefined as it is).
//
// Both passes get identical summaries, fragments, entry state, slot filter, room and n.  Where the lane-parallel pass takes the
// chunk, everything it leaves is compared bit for bit with what the serial pass leaves: the 64 flag words, all of
// S.dmr.emb_words, all 64 state words (s[DS_EMB_DATA*] among them), the machine M, room, and the serial pass's nflag = consumed = n,
// to_sync = overflow = false.  Where it declines, it must have written nothing (the caller then runs the serial pass on the same
// input, so the outcome is the serial pass's by construction).  And it must take a chunk exactly when the chunk is regular,
// which is read off the serial pass's own result: entry slot != -1, every TACT names the expected slot, every burst got a SYNC or EMB
// flag and none a reset flag, nothing overflowed, no return to the SyncPhase.
//
// Cases: 100 000 random chunks (n from 1, 2, 63, 64 and random; traffic-shaped summaries with none to all bursts disturbed);
// the entry states enumerated -- every value of the global members (slot x stab x sync_count x active x filter, 43 848) against a
// set of slot words, and every ordered pair of slot words (st x ss x sf x eo, 540 x 540) against active: the slot words meet the global
// members only through `slot` and `active`, so the two products cover every interaction without walking the 10^10 full product;
// and regular chunks with one irregularity planted at every lane index (see plant()).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "../../digiham_amd/csrc/decoder_core.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t) (rng_state >> 16); }
static uint32_t rnd(uint32_t n) { return rnd() % n; }
static bool chance(uint32_t pct) { return rnd(100) < pct; }

struct Case {
    DhDmrLane L[DH_WAVE];
    DhDmrMachine M;
    uint32_t emb[8];
    uint32_t room, n;
};

static DhDecShared* SA; static DhDecShared* SB;
static long n_lanes = 0, n_scalar = 0, n_fail = 0;

#define FAIL(...) do { if (n_fail++ < 20) { printf("FAIL %s: ", what); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool same_machine(const DhDmrMachine& a, const DhDmrMachine& b) {
    return a.slot == b.slot && a.stab == b.stab && a.sync_count == b.sync_count && a.st0 == b.st0 && a.st1 == b.st1 && a.ss0 == b.ss0 && a.ss1 == b.ss1 &&
           a.active == b.active && a.filter == b.filter && a.sf0 == b.sf0 && a.sf1 == b.sf1 && a.eo0 == b.eo0 && a.eo1 == b.eo1;
}

// runs both passes on the case; returns whether the lane-parallel pass took it
static bool check(const Case& c, const char* what) {
    static DhDmrLane la[DH_WAVE], lb[DH_WAVE];
    memcpy(la, c.L, sizeof la); memcpy(lb, c.L, sizeof lb);
    DhState sa, sb;
    for (int i = 0; i < DH_DEC_STATE_WORDS; i++) sa.w[i] = sb.w[i] = 0xA5000000u + (uint32_t) i;
    for (int i = 0; i < 8; i++) sa.w[DS_EMB_DATA0 + i] = sb.w[DS_EMB_DATA0 + i] = c.emb[i];
    for (int k = 0; k < DH_DMR_CHUNK; k++) for (int i = 0; i < 4; i++) SA->dmr.emb_words[k][i] = SB->dmr.emb_words[k][i] = 0xC3000000u + (uint32_t) (4 * k + i);
    DhDmrMachine ma = c.M, mb = c.M;
    uint32_t room_a = c.room, room_b = c.room, nflag = 0;
    bool to_sync = false, ovf = false;
    const uint32_t ncons = dh_dmr_pass_b(ma, sa, *SA, la, c.n, room_a, nflag, to_sync, ovf);
    const bool took = dh_dmr_pass_b_lanes(mb, sb, *SB, lb, c.n, room_b);
    // regular, by the serial pass's own account
    bool regular = c.M.slot != -1 && nflag == c.n && ncons == c.n && !to_sync && !ovf;
    for (uint32_t k = 0; k < c.n && regular; k++) {
        const uint32_t sm = c.L[k].summary, fl = la[k].flags;
        const uint32_t expect = (uint32_t) (c.M.slot ^ 1 ^ (int) k) & 1u;
        regular = (sm & DH_DS_HAS_TACT) && ((sm >> DH_DS_TACT_SLOT_SHIFT) & 1u) == expect && (fl & (DH_DF_SYNC | DH_DF_EMB)) &&
                  !(fl & (DH_DF_RESET_OTHER | DH_DF_SLOT_RESET | DH_DF_META_RESET));
    }
    if (took != regular) FAIL("took %d but regular %d (n %u)", (int) took, (int) regular, c.n);
    if (took) {
        n_lanes++;
        for (int k = 0; k < DH_WAVE; k++) if (la[k].flags != lb[k].flags) { FAIL("flags of burst %d: serial %x lanes %x (n %u)", k, la[k].flags, lb[k].flags, c.n); break; }
        if (memcmp(la, lb, sizeof la)) FAIL("lane structs differ");
        if (memcmp(SA->dmr.emb_words, SB->dmr.emb_words, sizeof SA->dmr.emb_words)) FAIL("emb_words differ");
        if (memcmp(sa.w, sb.w, sizeof sa.w)) FAIL("state words differ");
        if (!same_machine(ma, mb)) FAIL("machine differs: slot %d/%d stab %d/%d sc %d/%d st %d,%d/%d,%d ss %d,%d/%d,%d sf %d,%d/%d,%d eo %d,%d/%d,%d active %d/%d",
            ma.slot, mb.slot, ma.stab, mb.stab, ma.sync_count, mb.sync_count, ma.st0, ma.st1, mb.st0, mb.st1, ma.ss0, ma.ss1, mb.ss0, mb.ss1,
            ma.sf0, ma.sf1, mb.sf0, mb.sf1, ma.eo0, ma.eo1, mb.eo0, mb.eo1, ma.active, mb.active);
        if (room_a != room_b) FAIL("room %u / %u", room_a, room_b);
    } else {
        n_scalar++;
        bool clean = memcmp(lb, c.L, sizeof lb) == 0 && same_machine(mb, c.M) && room_b == c.room;
        for (int i = 0; i < DH_DEC_STATE_WORDS; i++) clean = clean && sb.w[i] == ((i >= DS_EMB_DATA0 && i < DS_EMB_DATA0 + 8) ? c.emb[i - DS_EMB_DATA0] : 0xA5000000u + (uint32_t) i);
        for (int k = 0; k < DH_DMR_CHUNK; k++) for (int i = 0; i < 4; i++) clean = clean && SB->dmr.emb_words[k][i] == 0xC3000000u + (uint32_t) (4 * k + i);
        if (!clean) FAIL("declined the chunk but wrote something");
    }
    return took;
}

// ---- traffic-shaped chunks
static uint32_t sm_common(uint32_t slot) {
    return DH_DS_HAS_TACT | slot << DH_DS_TACT_SLOT_SHIFT | rnd(16) << DH_DS_EMB_CC_SHIFT | rnd(16) << DH_DS_ST_CC_SHIFT | rnd(16) << DH_DS_DT_SHIFT |
           (rnd(16) & 0xDu) << DH_DS_DFLAGS_SHIFT | (chance(50) ? (uint32_t) DH_DS_ST_OK : 0u) | (chance(50) ? (uint32_t) DH_DS_BPTC_OK : 0u);
}
static uint32_t sm_sync(uint32_t slot, int type) { return sm_common(slot) | (uint32_t) type << DH_DS_SYNC_SHIFT | (chance(10) ? (uint32_t) DH_DS_EMB_OK | rnd(4) << DH_DS_LCSS_SHIFT : 0u); }
static uint32_t sm_emb(uint32_t slot, uint32_t lcss) { return sm_common(slot) | DH_DS_EMB_OK | lcss << DH_DS_LCSS_SHIFT; }

struct Gen { int voice; int sf, limit; };      // one slot's traffic: inside a voice superframe (sf bursts behind its sync, a sync is due at `limit`) or between syncs

// a chunk of regular traffic on both slots that continues the entry state it makes up; lcss_noise = percent of EMBs with a random LCSS
static void regular_case(Case& c, uint32_t n, uint32_t lcss_noise, int voice_pct = 60) {
    memset(&c, 0, sizeof c);
    DhDmrMachine& M = c.M;
    M.slot = (int) rnd(2); M.stab = (int) rnd(202) - 101; M.sync_count = (int) rnd(6); M.active = (int) rnd(3) - 1; M.filter = chance(70) ? 3 : (int) rnd(4);
    Gen g[2];
    for (int p = 0; p < 2; p++) {
        const int st = chance(voice_pct) ? DH_SYNCTYPE_VOICE : chance(70) ? DH_SYNCTYPE_DATA : -1;
        const int ss = (int) rnd(6), sf = (int) rnd(6), eo = (int) rnd(5);
        g[p].voice = st == DH_SYNCTYPE_VOICE; g[p].sf = sf; g[p].limit = sf >= 4 ? 5 : 4 + (int) rnd(2);
        if (p) { M.st1 = st; M.ss1 = ss; M.sf1 = sf; M.eo1 = eo; } else { M.st0 = st; M.ss0 = ss; M.sf0 = sf; M.eo0 = eo; }
    }
    for (int i = 0; i < 8; i++) c.emb[i] = rnd() ^ rnd() << 16;
    static const uint32_t pattern[5] = { 1, 3, 3, 2, 0 };
    for (int k = 0; k < DH_WAVE; k++) {
        const uint32_t slot = (uint32_t) (M.slot ^ 1 ^ k) & 1u;
        Gen& q = g[slot];
        uint32_t sm;
        if (q.voice && q.sf < q.limit) { sm = sm_emb(slot, chance(lcss_noise) ? rnd(4) : pattern[q.sf]); q.sf++; }
        else if (chance(voice_pct)) { sm = sm_sync(slot, DH_SYNCTYPE_VOICE); q.voice = 1; q.sf = 0; q.limit = 4 + (int) rnd(2); }
        else { sm = sm_sync(slot, DH_SYNCTYPE_DATA); q.voice = 0; }
        c.L[k].summary = sm; c.L[k].frag = rnd() ^ rnd() << 16; c.L[k].flags = 0;
        for (int i = 0; i < 5; i++) { c.L[k].hw[i] = rnd(); c.L[k].lw[i] = rnd(); }
        for (int i = 0; i < 3; i++) c.L[k].bptc[i] = rnd();
    }
    c.n = n; c.room = 100000u;
}

static void disturb(uint32_t& sm) {
    switch (rnd(7)) {
    case 0: sm &= ~(uint32_t) DH_DS_HAS_TACT; break;
    case 1: sm ^= 1u << DH_DS_TACT_SLOT_SHIFT; break;
    case 2: sm &= ~(3u << DH_DS_SYNC_SHIFT); break;
    case 3: sm = (sm & ~(3u << DH_DS_SYNC_SHIFT)) | (1u + rnd(2)) << DH_DS_SYNC_SHIFT; break;
    case 4: sm &= ~(uint32_t) DH_DS_EMB_OK; break;
    case 5: sm ^= rnd(4) << DH_DS_LCSS_SHIFT; break;
    default: { uint32_t r = rnd() ^ rnd() << 16; if (((r >> DH_DS_SYNC_SHIFT) & 3u) == 3u) r ^= 1u << DH_DS_SYNC_SHIFT; sm = r; } break;      // (a summary never carries sync type 3)
    }
}

static uint32_t pick_n() { static const uint32_t fixed[4] = { 1, 2, 63, 64 }; const uint32_t r = rnd(8); return r < 4 ? fixed[r] : 1u + rnd(64); }

static void random_chunks(long count) {
    const char* what = "random";
    static const uint32_t rates[6] = { 0, 0, 1, 5, 30, 100 };
    for (long it = 0; it < count; it++) {
        Case c;
        regular_case(c, pick_n(), chance(50) ? 15 : 0, (int) rnd(101));
        const uint32_t rate = rates[rnd(6)];
        for (int k = 0; k < DH_WAVE; k++) if (chance(rate)) disturb(c.L[k].summary);
        if (chance(30)) {                      // an entry state that the traffic does not continue
            c.M.slot = (int) rnd(3) - 1;
            c.M.st0 = (int) rnd(3) == 0 ? -1 : 1 + (int) rnd(2); c.M.st1 = (int) rnd(3) == 0 ? -1 : 1 + (int) rnd(2);
            c.M.sf0 = (int) rnd(6); c.M.sf1 = (int) rnd(6); c.M.eo0 = (int) rnd(5); c.M.eo1 = (int) rnd(5);
        }
        if (chance(25)) c.room = rnd(27 * 70);
        check(c, what);
    }
}

static void set_word(DhDmrMachine& M, int p, int st, int ss, int sf, int eo) {
    if (p) { M.st1 = st; M.ss1 = ss; M.sf1 = sf; M.eo1 = eo; } else { M.st0 = st; M.ss0 = ss; M.sf0 = sf; M.eo0 = eo; }
}

static void entry_states() {
    const char* what = "entry states";
    static const int sts[3] = { -1, DH_SYNCTYPE_DATA, DH_SYNCTYPE_VOICE };
    Case base[4];
    for (int i = 0; i < 4; i++) regular_case(base[i], i == 0 ? 64u : pick_n(), 15);
    // the global members in full, against six pairs of slot words
    static const int words[6][2][4] = { { { 2, 3, 0, 0 }, { 1, 5, 0, 0 } }, { { 2, 0, 4, 3 }, { 2, 5, 2, 1 } }, { { -1, 0, 0, 0 }, { 2, 1, 5, 4 } },
                                        { { 1, 2, 0, 0 }, { -1, 0, 0, 0 } }, { { 2, 5, 1, 2 }, { 2, 0, 0, 0 } }, { { 1, 0, 0, 0 }, { 1, 5, 0, 0 } } };
    long id = 0;
    for (int slot = -1; slot <= 1; slot++) for (int stab = -101; stab <= 100; stab++) for (int sc = 0; sc <= 5; sc++)
        for (int active = -1; active <= 1; active++) for (int filter = 0; filter <= 3; filter++) for (int w = 0; w < 6; w++, id++) {
            Case c = base[id & 3];
            // (the traffic of the base chunk is laid out for the slot of its own entry state: keep the parity, so that the TACTs fit)
            if (slot >= 0 && slot != c.M.slot) for (int k = 0; k < DH_WAVE; k++) c.L[k].summary ^= 1u << DH_DS_TACT_SLOT_SHIFT;
            c.M.slot = slot; c.M.stab = stab; c.M.sync_count = sc; c.M.active = active; c.M.filter = filter;
            for (int p = 0; p < 2; p++) set_word(c.M, p, words[w][p][0], words[w][p][1], words[w][p][2], words[w][p][3]);
            check(c, what);
        }
    // every pair of slot words, against slot and active
    // (the pair (a, b) entered in slot 0 is the pair (b, a) entered in slot 1: the slot goes along with the pair's index)
    for (int a = 0; a < 540; a++) for (int b = 0; b < 540; b++) for (int active = -1; active <= 1; active++, id++) {
        const int slot = (a + b) & 1;
        Case c = base[id & 3];
        if (slot != c.M.slot) for (int k = 0; k < DH_WAVE; k++) c.L[k].summary ^= 1u << DH_DS_TACT_SLOT_SHIFT;
        c.M.slot = slot; c.M.active = active; c.M.filter = 3;
        set_word(c.M, 0, sts[a % 3], a / 3 % 6, a / 18 % 6, a / 108);
        set_word(c.M, 1, sts[b % 3], b / 3 % 6, b / 18 % 6, b / 108);
        if (id % 7 == 0) c.n = 1u + (uint32_t) (id % 64);
        check(c, what);
    }
}

// ---- one irregularity (or edge of the embedded-LC collector) planted at lane k of a regular chunk
enum { TACT_MISSING, TACT_WRONG_STAB4, TACT_WRONG_STAB5, SYNC_MISSING, EMB_BAD, START_NO_STOP, STOP_NO_START, FIVE_CONT, STOP_FROM_BEFORE,
       VOICE_FILTERED, BOTH_CLAIM, ROOM_OUT, TO_SYNCPHASE, N_PLANTS };
static const char* plant_names[N_PLANTS] = { "TACT missing", "TACT slot wrong, stab 4", "TACT slot wrong, stab 5", "sync missing at sf 4 / 5", "EMB bad",
    "START without STOP", "STOP without START", "five continuations", "STOP of a segment from before the chunk", "voice on a filtered slot",
    "both slots claim active", "room runs out", "back to the SyncPhase" };

static bool is_sync(uint32_t sm) { return ((sm >> DH_DS_SYNC_SHIFT) & 3u) != 0u; }
static void set_lcss(uint32_t& sm, uint32_t v) { sm = (sm & ~(3u << DH_DS_LCSS_SHIFT)) | v << DH_DS_LCSS_SHIFT; }

// returns false when the base chunk does not offer the situation at lane k (the caller draws another one)
static bool plant(Case& c, int kind, int k) {
    uint32_t& sm = c.L[k].summary;
    switch (kind) {
    case TACT_MISSING: sm &= ~(uint32_t) DH_DS_HAS_TACT; return true;
    case TACT_WRONG_STAB4: case TACT_WRONG_STAB5:                 // the slot stability in front of burst k on both sides of 5 (dmr_phase.cpp:72-90)
        sm ^= 1u << DH_DS_TACT_SLOT_SHIFT; c.M.stab = (kind == TACT_WRONG_STAB4 ? 4 : 5) - k; return true;
    case SYNC_MISSING:                                            // the sync that ends a superframe of 5 or 6 bursts does not come: sf 4 goes on, sf 5 is lost
        if (!is_sync(sm) || (k >= 2 && is_sync(c.L[k - 2].summary))) return false;
        if (k < 2) set_word(c.M, (c.M.slot ^ 1 ^ k) & 1, DH_SYNCTYPE_VOICE, (int) rnd(6), 4 + (int) rnd(2), (int) rnd(5));      // (the superframe began before the chunk)
        sm = (sm & ~(3u << DH_DS_SYNC_SHIFT)) | DH_DS_EMB_OK; set_lcss(sm, 0); return true;
    case EMB_BAD:
        if (is_sync(sm)) return false;
        sm &= ~(uint32_t) DH_DS_EMB_OK; return true;
    case START_NO_STOP: case STOP_NO_START: case FIVE_CONT: {
        if (is_sync(sm)) return false;
        int lo = k, hi = k;                                       // the superframe around burst k
        while (lo - 2 >= 0 && !is_sync(c.L[lo - 2].summary)) lo -= 2;
        while (hi + 2 < DH_WAVE && !is_sync(c.L[hi + 2].summary)) hi += 2;
        for (int j = lo; j <= hi; j += 2) {
            uint32_t& x = c.L[j].summary;
            if (kind == FIVE_CONT) set_lcss(x, 3);
            else if (kind == START_NO_STOP) set_lcss(x, j < k ? 0u : j == k ? 1u : 3u);
            else set_lcss(x, j < k ? 0u : j == k ? 2u : 0u);
        }
        return true; }
    case STOP_FROM_BEFORE: {                                      // the slot's bursts in front of k collect on from the entry state, k stops
        if (k > 7) return false;
        const int p = (c.M.slot ^ 1 ^ k) & 1, q = k >> 1;
        const int sf = (int) rnd((uint32_t) (5 - q)), eo = (int) rnd(5);
        set_word(c.M, p, DH_SYNCTYPE_VOICE, (int) rnd(6), sf, eo);
        for (int j = k & 1; j <= k; j += 2) { c.L[j].summary = sm_emb((uint32_t) p, j == k ? 2u : chance(70) ? 3u : 0u); }
        c.n = (uint32_t) k + 1u + (k < 63 ? rnd(2) : 0u);         // (behind burst k the base chunk's traffic no longer continues the slot's state)
        return true; }
    case VOICE_FILTERED: {                                        // burst k is a voice burst of a slot the filter does not let through
        if (is_sync(sm) && ((sm >> DH_DS_SYNC_SHIFT) & 3u) != DH_SYNCTYPE_VOICE) return false;
        const uint32_t p = (uint32_t) (c.M.slot ^ 1 ^ k) & 1u;
        c.M.filter = chance(50) ? (int) (2u - p) : 0;             // the filter lets the OTHER slot through, or none
        return true; }
    case BOTH_CLAIM: {                                            // voice on both slots from k on, superframes of five bursts, a release now and then
        c.M.filter = 3;
        int vo[2] = { 0, 0 };
        for (int j = k; j < DH_WAVE; j++) {
            const uint32_t p = (uint32_t) (c.M.slot ^ 1 ^ j) & 1u;
            if (!vo[p] || ((j - k) >> 1) % 5 == 0) { const int type = j < k + 2 || chance(75) ? DH_SYNCTYPE_VOICE : DH_SYNCTYPE_DATA; c.L[j].summary = sm_sync(p, type); vo[p] = type == DH_SYNCTYPE_VOICE; }
            else c.L[j].summary = sm_emb(p, rnd(4));
        }
        return true; }
    case ROOM_OUT: return true;                                   // (room is set by the caller from the serial pass's voice flags)
    default: {                                                    // TO_SYNCPHASE: the signal ends at burst k
        for (int j = k; j < DH_WAVE; j++) c.L[j].summary &= ~((3u << DH_DS_SYNC_SHIFT) | DH_DS_EMB_OK);
        c.M.sync_count = (int) rnd(6);
        return true; }
    }
}

static void planted() {
    long took[N_PLANTS] = { 0 }, declined[N_PLANTS] = { 0 };
    for (int kind = 0; kind < N_PLANTS; kind++) for (int k = 0; k < DH_WAVE; k++) {
        const char* what = plant_names[kind];
        int done = 0;
        for (int tries = 0; tries < 4000 && done < 12; tries++) {
            Case c;
            regular_case(c, 64u, 0, 75);
            if (done % 3 == 1) c.n = (uint32_t) k + 1u;           // the planted burst is the chunk's last
            if (done % 3 == 2 && k < 63) c.n = (uint32_t) k + 2u;
            if (!check(c, "regular base chunk")) { const char* what = "regular base chunk"; FAIL("not taken lane-parallel"); }
            if (!plant(c, kind, k)) continue;
            if (kind == ROOM_OUT) {                               // room for the voice payloads in front of burst k and 0, 26 or 27 bytes more
                static DhDmrLane l[DH_WAVE]; memcpy(l, c.L, sizeof l);
                DhState s; memset(&s, 0, sizeof s); DhDmrMachine m = c.M; uint32_t room = 100000u, nflag; bool ts, ov = false;
                dh_dmr_pass_b(m, s, *SA, l, c.n, room, nflag, ts, ov);
                uint32_t before = 0; for (int j = 0; j < k; j++) before += (l[j].flags & DH_DF_VOICE) ? 27u : 0u;
                static const uint32_t extra[3] = { 0, 26, 27 };
                c.room = before + extra[done % 3]; c.n = done % 3 == 2 ? (uint32_t) k + 1u : 64u;      // (27 more: burst k is the last and fits)
            }
            (check(c, what) ? took : declined)[kind]++;
            done++;
        }
        if (done < 12 && !(kind == STOP_FROM_BEFORE && k > 7)) { n_fail++; printf("FAIL %s: no base chunk for lane %d\n", what, k); }
    }
    for (int kind = 0; kind < N_PLANTS; kind++) printf("  %-42s lane-parallel %5ld  serial %5ld\n", plant_names[kind], took[kind], declined[kind]);
    // what each plant must come to: the irregular ones are never taken, the collector's edges and the filter / claim cases always, the
    // missing sync and the room on both sides
    static const int must[N_PLANTS] = { -1, -1, -1, 0, -1, 1, 1, 1, 1, 1, 1, 0, -1 };
    for (int kind = 0; kind < N_PLANTS; kind++) {
        const bool ok = must[kind] < 0 ? took[kind] == 0 : must[kind] > 0 ? declined[kind] == 0 : (took[kind] > 0 && declined[kind] > 0);
        if (!ok) { n_fail++; printf("FAIL %s: lane-parallel %ld, serial %ld\n", plant_names[kind], took[kind], declined[kind]); }
    }
}

int main() {
    SA = new DhDecShared; SB = new DhDecShared;
    memset(SA, 0, sizeof *SA); memset(SB, 0, sizeof *SB);
    random_chunks(100000);
    printf("random chunks: lane-parallel %ld, serial %ld\n", n_lanes, n_scalar);
    if (n_lanes < 10000 || n_scalar < 10000) { n_fail++; printf("FAIL: the random chunks do not exercise both outcomes\n"); }
    long a = n_lanes, b = n_scalar;
    entry_states();
    printf("entry states: lane-parallel %ld, serial %ld\n", n_lanes - a, n_scalar - b);
    planted();
    delete SA; delete SB;
    if (n_fail) { printf("dmr pass b: %ld FAILURES\n", n_fail); return 1; }
    printf("dmr pass b: identical\n");
    return 0;
}
