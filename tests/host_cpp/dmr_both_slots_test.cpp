// dmr_both_slots_test.cpp -- pass B of the DMR decoder in the both-slots mode (DH_FLAG_DMR_BOTH_SLOTS: DH_DMR_BOTH_SLOTS_BIT in the slot
// filter word), lane-parallel (dh_dmr_pass_b_lanes) against burst-serial (dh_dmr_pass_b), which is its definition.  Stand-alone, host
// only: g++ -std=c++17 -O1 -fsanitize=address,undefined tests/host_cpp/dmr_both_slots_test.cpp && ./a.out
//
// Every case is run three times on identical input: the serial pass with room for everything (what the chunk IS: regular or not, which
// bursts are voice), then both passes with the case's room.  Checked:
//   * the lane pass takes the chunk exactly when the serial pass's flags call it regular (entry slot known, every TACT names the expected
//     slot, every burst got a SYNC or an EMB flag and none a reset flag, no return to the SyncPhase) and 28 bytes per voice burst fit;
//   * where it takes it: all 64 flag words, the lane structs, S.dmr.emb_words, all state words (the carried embedded words among them),
//     the machine and room are the serial pass's; where it declines, nothing was written;
//   * `active` is -1 behind every chunk, whichever pass ran it, regular or not;
//   * on regular chunks the voice flags are exactly "the slot's sync type behind the burst is VOICE and the filter has the slot's bit",
//     read off the serial flags (SYNC with a voice sync in the summary, or EMB), and the room shrinks by 28 for each.
// Cases: 240 000 random chunks (own generator: traffic on both slots that continues a made-up entry state, none to all summaries
// disturbed, n = 1..64, filters 0..3, room on both sides of 28 x voice count), and the entry states enumerated: every value of the global
// members (slot x stab x sync_count x filter) and every slot word (st x ss x sf x eo) of either slot.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "../../digiham_amd/csrc/decoder_core.hpp"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t) (rng_state >> 20); }
static uint32_t rnd(uint32_t n) { return rnd() % n; }
static bool chance(uint32_t pct) { return rnd(100) < pct; }

struct Case {
    DhDmrLane L[DH_WAVE];
    DhDmrMachine M;
    uint32_t emb[8];
    uint32_t n;
};

static DhDecShared* SA; static DhDecShared* SB;
static long n_taken = 0, n_declined = 0, n_short = 0, n_fail = 0, n_voice = 0, n_both_voice = 0;

#define FAIL(...) do { if (n_fail++ < 20) { printf("FAIL %s: ", what); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool same_machine(const DhDmrMachine& a, const DhDmrMachine& b) {
    return a.slot == b.slot && a.stab == b.stab && a.sync_count == b.sync_count && a.st0 == b.st0 && a.st1 == b.st1 && a.ss0 == b.ss0 && a.ss1 == b.ss1 &&
           a.active == b.active && a.filter == b.filter && a.sf0 == b.sf0 && a.sf1 == b.sf1 && a.eo0 == b.eo0 && a.eo1 == b.eo1;
}

static void fresh(DhState& s, DhDecShared& S, const Case& c) {
    for (int i = 0; i < DH_DEC_STATE_WORDS; i++) s.w[i] = 0x5A000000u + (uint32_t) i;
    for (int i = 0; i < 8; i++) s.w[DS_EMB_DATA0 + i] = c.emb[i];
    for (int k = 0; k < DH_DMR_CHUNK; k++) for (int i = 0; i < 4; i++) S.dmr.emb_words[k][i] = 0x3C000000u + (uint32_t) (4 * k + i);
}

enum { ROOM_PLENTY, ROOM_EXACT, ROOM_ONE_SHORT, ROOM_OLD_RECORDS, ROOM_RANDOM_BELOW, ROOM_ABOVE, ROOM_KINDS };

static void check(const Case& c, int room_kind, const char* what) {
    static DhDmrLane l0[DH_WAVE], la[DH_WAVE], lb[DH_WAVE];
    // what the chunk is: the serial pass with room for everything
    memcpy(l0, c.L, sizeof l0);
    DhState s0; fresh(s0, *SA, c);
    DhDmrMachine m0 = c.M;
    uint32_t room0 = 1u << 20, nflag0 = 0; bool ts0 = false, ov0 = false;
    const uint32_t ncons0 = dh_dmr_pass_b(m0, s0, *SA, l0, c.n, room0, nflag0, ts0, ov0);
    bool regular = c.M.slot != -1 && nflag0 == c.n && ncons0 == c.n && !ts0 && !ov0;
    for (uint32_t k = 0; k < c.n && regular; k++) {
        const uint32_t sm = c.L[k].summary, fl = l0[k].flags;
        const uint32_t expect = (uint32_t) (c.M.slot ^ 1 ^ (int) k) & 1u;
        regular = (sm & DH_DS_HAS_TACT) && ((sm >> DH_DS_TACT_SLOT_SHIFT) & 1u) == expect && (fl & (DH_DF_SYNC | DH_DF_EMB)) &&
                  !(fl & (DH_DF_RESET_OTHER | DH_DF_SLOT_RESET | DH_DF_META_RESET));
    }
    uint32_t nv = 0, slots_seen = 0;
    for (uint32_t k = 0; k < nflag0; k++) if (l0[k].flags & DH_DF_VOICE) { nv++; slots_seen |= (l0[k].flags & DH_DF_SLOT) ? 2u : 1u; }
    if (room0 != (1u << 20) - 28u * nv) FAIL("serial pass: room went down by %u for %u voice bursts", (1u << 20) - room0, nv);
    if (m0.active != -1) FAIL("serial pass left active = %d", m0.active);
    if (regular) {
        n_voice += nv; if (slots_seen == 3u) n_both_voice++;
        for (uint32_t k = 0; k < c.n; k++) {
            const uint32_t sm = c.L[k].summary, fl = l0[k].flags;
            const bool st_voice = (fl & DH_DF_SYNC) ? ((sm >> DH_DS_SYNC_SHIFT) & 3u) == DH_SYNCTYPE_VOICE : (fl & DH_DF_EMB) != 0u;
            const uint32_t slot = (fl & DH_DF_SLOT) ? 1u : 0u;
            const bool want = st_voice && ((slot + 1u) & (uint32_t) c.M.filter & 3u) != 0u;
            if (want != ((fl & DH_DF_VOICE) != 0u)) { FAIL("burst %u: voice flag %d, sync type / filter say %d (filter %d)", k, (int) !want, (int) want, c.M.filter); break; }
        }
    }
    uint32_t room;
    switch (room_kind) {
    case ROOM_EXACT: room = 28u * nv; break;
    case ROOM_ONE_SHORT: room = nv ? 28u * nv - 1u : 0u; break;
    case ROOM_OLD_RECORDS: room = 27u * nv; break;                 // (what 27-byte records would need)
    case ROOM_RANDOM_BELOW: room = nv ? rnd(28u * nv) : 0u; break;
    case ROOM_ABOVE: room = 28u * nv + rnd(64); break;
    default: room = 100000u; break;
    }
    const bool fits = 28u * nv <= room;
    if (regular && !fits) n_short++;
    // both passes with the case's room
    memcpy(la, c.L, sizeof la); memcpy(lb, c.L, sizeof lb);
    DhState sa, sb; fresh(sa, *SA, c); fresh(sb, *SB, c);
    DhDmrMachine ma = c.M, mb = c.M;
    uint32_t room_a = room, room_b = room, nflag = 0; bool to_sync = false, ovf = false;
    const uint32_t ncons = dh_dmr_pass_b(ma, sa, *SA, la, c.n, room_a, nflag, to_sync, ovf);
    const bool took = dh_dmr_pass_b_lanes(mb, sb, *SB, lb, c.n, room_b);
    if (ma.active != -1) FAIL("serial pass left active = %d (room %u)", ma.active, room);
    if (regular && ovf != !fits) FAIL("serial pass: overflow %d with room %u for %u voice bursts", (int) ovf, room, nv);
    if (took != (regular && fits)) FAIL("took %d but regular %d, fits %d (n %u, %u voice, room %u)", (int) took, (int) regular, (int) fits, c.n, nv, room);
    if (took) {
        n_taken++;
        if (ncons != c.n || nflag != c.n || to_sync || ovf) FAIL("taken, but the serial pass consumed %u of %u", ncons, c.n);
        for (int k = 0; k < DH_WAVE; k++) if (la[k].flags != lb[k].flags) { FAIL("flags of burst %d: serial %x lanes %x (n %u)", k, la[k].flags, lb[k].flags, c.n); break; }
        if (memcmp(la, lb, sizeof la)) FAIL("lane structs differ");
        if (memcmp(SA->dmr.emb_words, SB->dmr.emb_words, sizeof SA->dmr.emb_words)) FAIL("emb_words differ");
        if (memcmp(sa.w, sb.w, sizeof sa.w)) FAIL("state words differ");
        if (!same_machine(ma, mb)) FAIL("machine differs (slot %d/%d stab %d/%d sync count %d/%d active %d/%d)", ma.slot, mb.slot, ma.stab, mb.stab, ma.sync_count, mb.sync_count, ma.active, mb.active);
        if (mb.active != -1) FAIL("lane pass left active = %d", mb.active);
        if (room_a != room_b || room_b != room - 28u * nv) FAIL("room %u / %u behind %u voice bursts from %u", room_a, room_b, nv, room);
    } else {
        n_declined++;
        bool clean = memcmp(lb, c.L, sizeof lb) == 0 && same_machine(mb, c.M) && room_b == room;
        for (int i = 0; i < DH_DEC_STATE_WORDS; i++) clean = clean && sb.w[i] == ((i >= DS_EMB_DATA0 && i < DS_EMB_DATA0 + 8) ? c.emb[i - DS_EMB_DATA0] : 0x5A000000u + (uint32_t) i);
        for (int k = 0; k < DH_DMR_CHUNK; k++) for (int i = 0; i < 4; i++) clean = clean && SB->dmr.emb_words[k][i] == 0x3C000000u + (uint32_t) (4 * k + i);
        if (!clean) FAIL("declined the chunk but wrote something");
    }
}

// ---- the generator: summaries as pass A leaves them
static uint32_t sm_rest(uint32_t slot) {
    return DH_DS_HAS_TACT | slot << DH_DS_TACT_SLOT_SHIFT | rnd(16) << DH_DS_EMB_CC_SHIFT | rnd(16) << DH_DS_ST_CC_SHIFT | rnd(16) << DH_DS_DT_SHIFT |
           (rnd(16) & 0xDu) << DH_DS_DFLAGS_SHIFT | (chance(50) ? (uint32_t) DH_DS_ST_OK : 0u) | (chance(50) ? (uint32_t) DH_DS_BPTC_OK : 0u);
}
static uint32_t sm_sync(uint32_t slot, int type) { return sm_rest(slot) | (uint32_t) type << DH_DS_SYNC_SHIFT | (chance(10) ? (uint32_t) DH_DS_EMB_OK | rnd(4) << DH_DS_LCSS_SHIFT : 0u); }
static uint32_t sm_emb(uint32_t slot, uint32_t lcss) { return sm_rest(slot) | DH_DS_EMB_OK | lcss << DH_DS_LCSS_SHIFT; }

static void set_word(DhDmrMachine& M, int p, int st, int ss, int sf, int eo) {
    if (p) { M.st1 = st; M.ss1 = ss; M.sf1 = sf; M.eo1 = eo; } else { M.st0 = st; M.ss0 = ss; M.sf0 = sf; M.eo0 = eo; }
}

// traffic on both slots that continues the entry state it makes up: a slot is inside a voice superframe (EMBs until a sync is due) or
// between syncs; voice_pct = how much of the traffic is voice, lcss_noise = percent of EMBs with a random LCSS
static void traffic(Case& c, uint32_t n, uint32_t voice_pct, uint32_t lcss_noise) {
    memset(&c, 0, sizeof c);
    DhDmrMachine& M = c.M;
    M.slot = (int) rnd(2); M.stab = (int) rnd(202) - 101; M.sync_count = (int) rnd(6); M.active = -1;
    M.filter = (int) ((chance(60) ? 3u : rnd(4)) | DH_DMR_BOTH_SLOTS_BIT);
    int voice[2], sf[2], due[2];
    for (int p = 0; p < 2; p++) {
        const int st = chance(voice_pct) ? DH_SYNCTYPE_VOICE : chance(70) ? DH_SYNCTYPE_DATA : -1;
        voice[p] = st == DH_SYNCTYPE_VOICE; sf[p] = (int) rnd(6); due[p] = sf[p] >= 4 ? 5 : 4 + (int) rnd(2);
        set_word(M, p, st, (int) rnd(6), sf[p], (int) rnd(5));
    }
    for (int i = 0; i < 8; i++) c.emb[i] = rnd() ^ rnd() << 16;
    static const uint32_t lcss_of[5] = { 1, 3, 3, 2, 0 };
    for (int k = 0; k < DH_WAVE; k++) {
        const uint32_t p = (uint32_t) (M.slot ^ 1 ^ k) & 1u;
        uint32_t sm;
        if (voice[p] && sf[p] < due[p]) { sm = sm_emb(p, chance(lcss_noise) ? rnd(4) : lcss_of[sf[p]]); sf[p]++; }
        else if (chance(voice_pct)) { sm = sm_sync(p, DH_SYNCTYPE_VOICE); voice[p] = 1; sf[p] = 0; due[p] = 4 + (int) rnd(2); }
        else { sm = sm_sync(p, DH_SYNCTYPE_DATA); voice[p] = 0; }
        c.L[k].summary = sm; c.L[k].frag = rnd() ^ rnd() << 16; c.L[k].flags = 0;
        for (int i = 0; i < 5; i++) { c.L[k].hw[i] = rnd(); c.L[k].lw[i] = rnd(); }
        for (int i = 0; i < 3; i++) c.L[k].bptc[i] = rnd();
    }
    c.n = n;
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
    static const uint32_t rates[6] = { 0, 0, 0, 2, 30, 100 };
    for (long it = 0; it < count; it++) {
        Case c;
        traffic(c, pick_n(), chance(50) ? 85u : rnd(101), chance(50) ? 15u : 0u);
        const uint32_t rate = rates[rnd(6)];
        for (int k = 0; k < DH_WAVE; k++) if (chance(rate)) disturb(c.L[k].summary);
        if (chance(25)) {                      // an entry state that the traffic does not continue
            c.M.slot = (int) rnd(3) - 1;
            for (int p = 0; p < 2; p++) set_word(c.M, p, rnd(3) == 0 ? -1 : 1 + (int) rnd(2), (int) rnd(6), (int) rnd(6), (int) rnd(5));
        }
        check(c, (int) (it % ROOM_KINDS), what);
    }
}

static void entry_states() {
    const char* what = "entry states";
    static const int sts[3] = { -1, DH_SYNCTYPE_DATA, DH_SYNCTYPE_VOICE };
    Case base[4];
    for (int i = 0; i < 4; i++) traffic(base[i], i == 0 ? 64u : pick_n(), 85, 15);
    long id = 0;
    // the global members in full, the slot words as the base chunk made them up or drawn
    for (int slot = -1; slot <= 1; slot++) for (int stab = -101; stab <= 100; stab++) for (int sc = 0; sc <= 5; sc++) for (int filter = 0; filter <= 3; filter++, id++) {
        Case c = base[id & 3];
        // (the traffic of the base chunk is laid out for the slot of its own entry state: keep the parity, so that the TACTs fit)
        if (slot >= 0 && slot != c.M.slot) for (int k = 0; k < DH_WAVE; k++) c.L[k].summary ^= 1u << DH_DS_TACT_SLOT_SHIFT;
        c.M.slot = slot; c.M.stab = stab; c.M.sync_count = sc; c.M.filter = filter | DH_DMR_BOTH_SLOTS_BIT;
        if (id % 3 == 0) for (int p = 0; p < 2; p++) set_word(c.M, p, sts[rnd(3)], (int) rnd(6), (int) rnd(6), (int) rnd(5));
        check(c, (int) (id % ROOM_KINDS), what);
    }
    // every slot word of either slot, entered in either slot, under every filter; the other slot's word drawn
    for (int p = 0; p < 2; p++) for (int w = 0; w < 540; w++) for (int slot = 0; slot <= 1; slot++) for (int filter = 0; filter <= 3; filter++, id++) {
        Case c = base[id & 3];
        if (slot != c.M.slot) for (int k = 0; k < DH_WAVE; k++) c.L[k].summary ^= 1u << DH_DS_TACT_SLOT_SHIFT;
        c.M.slot = slot; c.M.filter = filter | DH_DMR_BOTH_SLOTS_BIT;
        set_word(c.M, p ^ 1, sts[rnd(3)], (int) rnd(6), (int) rnd(6), (int) rnd(5));
        set_word(c.M, p, sts[w % 3], w / 3 % 6, w / 18 % 6, w / 108);
        if (id % 5 == 0) c.n = 1u + (uint32_t) (id % 64);
        check(c, (int) (id % ROOM_KINDS), what);
    }
}

int main() {
    SA = new DhDecShared; SB = new DhDecShared;
    memset(SA, 0, sizeof *SA); memset(SB, 0, sizeof *SB);
    random_chunks(240000);
    printf("random chunks: lane-parallel %ld, declined %ld (of them regular but short of room: %ld); %ld voice bursts on regular chunks, %ld regular chunks with voice on both slots\n",
           n_taken, n_declined, n_short, n_voice, n_both_voice);
    if (n_taken < 20000 || n_declined < 20000 || n_short < 5000 || n_both_voice < 5000) { n_fail++; printf("FAIL: the random chunks do not exercise every outcome\n"); }
    const long a = n_taken, b = n_declined;
    entry_states();
    printf("entry states: lane-parallel %ld, declined %ld\n", n_taken - a, n_declined - b);
    if (n_taken - a < 1000 || n_declined - b < 1000) { n_fail++; printf("FAIL: the entry states do not exercise both outcomes\n"); }
    delete SA; delete SB;
    if (n_fail) { printf("dmr both slots: %ld FAILURES\n", n_fail); return 1; }
    printf("dmr both slots: identical\n");
    return 0;
}
