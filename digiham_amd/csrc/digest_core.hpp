// digest_core.hpp -- the call digest (DH_FLAG_CALL_DIGEST; include/digiham_amd.h, "Call digest"): a launch of its own behind the
// last launch of a push folds the channel's event row into its call record and rewrites the row in place -- one DH_EV_CALL
// event where the record changed, the pass-through events, nothing else.  One channel per wavefront, no LDS, no scratch.
//
// The raw row is taken in chunks of 64 events, one per lane.  The record is a handful of FIELD WORDS in GROUPS that are always
// written together (DMR: sync and type/source/target of either slot; NXDN: sync, type/source/destination; YSF: mode, target,
// source), carried between chunks in wave-uniform registers.  Phase 1: every lane loads its event and states which groups it
// writes and with what.  Phase 2: the value of a group in front of lane i is the one written by the last writer below i -- a vote
// of the group's writers, masked to the lanes below, dh_top64, DH_LS_GATHER -- or the carried one; an event changed the record
// where what it writes differs from that.  Phase 3: a stable compaction, positions from DH_LANES_BELOW of the keep vote.  Every
// load of a chunk is in registers before any lane stores, and an output index never exceeds its input index: the rewrite is
// safe in place, across chunks too.
#pragma once

#include "decoder_core.hpp"

#define DS_CALL_RECORD 56             // the call record in the channel's decoder state: six words that no decoder touches (zeroed by every reset path)
#define DH_CALL_RECORD_WORDS 6
#define DH_DIGEST_MAX_FIELDS 7
#define DH_DIGEST_MAX_GROUPS 4

// Digiham::Dmr::Lc opcodes (include/digiham/lc.hpp: LC_OPCODE_GROUP, LC_OPCODE_UNIT_TO_UNIT, LC_TALKER_ALIAS_HDR .. LC_GPS_INFO)
#define DH_LC_GROUP 0u
#define DH_LC_UNIT_TO_UNIT 3u
#define DH_LC_TALKER_ALIAS_HDR 4u
#define DH_LC_GPS_INFO 8u
// nxdn_meta.hpp: NXDN_MESSAGE_TYPE_VCALL, NXDN_CALL_TYPE_CONFERENCE, NXDN_CALL_TYPE_INDIVIDUAL
#define DH_NXDN_VCALL 1u
#define DH_NXDN_CONFERENCE 1u
#define DH_NXDN_INDIVIDUAL 4u

struct DhDigestParams {
    dh_event* events; size_t ev_stride; uint32_t ev_cap; uint32_t* ev_count;     // [B][ev_stride], [B]: rewritten in place
    uint32_t* state; size_t state_stride;                                       // [B][DH_DEC_STATE_WORDS]
    uint32_t n_channels;
};

// a lane's event (eight words), the field words it writes (zeros where it writes none), the groups it writes (bit g), pass-through
struct DhDigestLane { uint32_t e[8]; uint32_t v[DH_DIGEST_MAX_FIELDS]; uint32_t wr, pass; };

// What a protocol states: its field words and their groups, the record's bytes from the field words and back (the record in memory
// is the specification's, byte for byte), which parts changed (the `a` of a DH_EV_CALL), and the update one event applies.
template <int PROTO> struct DhDigest;

// DMR.  Slot s: field 3 s = sync (byte 0), 3 s + 1 = bytes 1-3 in place (type, source high and middle), 3 s + 2 = bytes 4-7 (source
// low, target).  The update is Dmr::MetaCollector's on its identity fields (include/digiham/dmr_meta.hpp:109-143).
template <> struct DhDigest<DH_PROTO_DMR> {
    static constexpr int FIELDS = 6, GROUPS = 4, WORDS = 4, LEN = 16;
    static DH_HD int group_of(int f) { return f == 0 ? 0 : f < 3 ? 1 : f == 3 ? 2 : 3; }
    static DH_HD void unpack(const uint32_t* w, uint32_t* F) {
        F[0] = w[0] & 0xFFu; F[1] = w[0] & ~0xFFu; F[2] = w[1];
        F[3] = w[2] & 0xFFu; F[4] = w[2] & ~0xFFu; F[5] = w[3];
    }
    static DH_HD void pack(const uint32_t* F, uint32_t* w) { w[0] = F[0] | F[1]; w[1] = F[2]; w[2] = F[3] | F[4]; w[3] = F[5]; w[4] = 0; w[5] = 0; }
    static DH_HD uint32_t parts(uint32_t changed) { return ((changed & 7u) ? 1u : 0u) | ((changed & 0x38u) ? 2u : 0u); }
    static DH_HD void classify(const uint32_t* e, uint32_t* v, uint32_t& wr, uint32_t& pass) {
        const uint32_t type = e[1] & 0xFFu, s = (e[1] >> 8) & 1u, b = (e[1] >> 16) & 0xFFu, len = e[1] >> 24, op = e[2] & 0x3Fu;
        uint32_t sync = 0, ida = 0, idb = 0;
        bool w_sync = false, w_id = false, both = false;
        if (type == DH_EV_DMR_SYNC) {
            w_sync = true; sync = b == DH_SYNCTYPE_DATA ? 1u : b == DH_SYNCTYPE_VOICE ? 2u : 3u;
            w_id = len > 0 && (e[2] & 0xFFu);                                  // voice -> data on this slot: the call ends
        } else if (type == DH_EV_DMR_SLOT_RESET) { w_sync = true; w_id = true; }
        else if (type == DH_EV_DMR_META_RESET) both = true;
        else if (type == DH_EV_DMR_SOFT_RESET) w_id = true;
        else if (type == DH_EV_DMR_LC) {
            if (len >= 9 && (op == DH_LC_GROUP || op == DH_LC_UNIT_TO_UNIT)) {
                // Lc::getSource: bytes 6-8, getTarget: bytes 3-5 of the word (lc.hpp:26-27); record bytes 2-4 and 5-7
                w_id = true;
                ida = (op == DH_LC_GROUP ? 1u : 2u) << 8 | (e[3] & 0xFFFF0000u);
                idb = (e[4] & 0xFFu) | (e[2] >> 24) << 8 | (e[3] & 0xFFFFu) << 16;
            } else pass = op >= DH_LC_TALKER_ALIAS_HDR && op <= DH_LC_GPS_INFO;
        }
        v[0] = s ? 0u : sync; v[1] = s ? 0u : ida; v[2] = s ? 0u : idb;
        v[3] = s ? sync : 0u; v[4] = s ? ida : 0u; v[5] = s ? idb : 0u;
        wr = both ? 15u : ((w_sync ? 1u : 0u) | (w_id ? 2u : 0u)) << (2u * s);
    }
};

// NXDN.  Field 0 = sync (byte 0), 1 = bytes 1-3 in place (type, source), 2 = bytes 4-5 (destination).  nxdn_meta.hpp:22-40.
template <> struct DhDigest<DH_PROTO_NXDN> {
    static constexpr int FIELDS = 3, GROUPS = 2, WORDS = 2, LEN = 8;
    static DH_HD int group_of(int f) { return f == 0 ? 0 : 1; }
    static DH_HD void unpack(const uint32_t* w, uint32_t* F) { F[0] = w[0] & 0xFFu; F[1] = w[0] & ~0xFFu; F[2] = w[1]; }
    static DH_HD void pack(const uint32_t* F, uint32_t* w) { w[0] = F[0] | F[1]; w[1] = F[2]; w[2] = 0; w[3] = 0; w[4] = 0; w[5] = 0; }
    static DH_HD uint32_t parts(uint32_t) { return 1u; }
    static DH_HD void classify(const uint32_t* e, uint32_t* v, uint32_t& wr, uint32_t& pass) {
        const uint32_t type = e[1] & 0xFFu, len = e[1] >> 24;
        v[0] = 0; v[1] = 0; v[2] = 0; wr = 0; pass = 0;
        if (type == DH_EV_NXDN_SYNC_VOICE) { v[0] = 1u; wr = 1u; }
        else if (type == DH_EV_NXDN_META_RESET) wr = 3u;
        else if (type == DH_EV_NXDN_SACCH_SF && len >= 9 && (e[2] & 0x3Fu) == DH_NXDN_VCALL) {
            const uint32_t ct = (e[2] >> 21) & 7u;                             // payload[2] >> 5
            // source: payload bytes 3, 4; destination: 5, 6 (nxdn_meta.hpp:32-33); record bytes 2-3 and 4-5
            v[1] = (ct == DH_NXDN_CONFERENCE ? 1u : ct == DH_NXDN_INDIVIDUAL ? 2u : 0u) << 8 | (e[2] >> 24) << 16 | (e[3] & 0xFFu) << 24;
            v[2] = (e[3] >> 8) & 0xFFFFu;
            wr = 2u;
        }
    }
};

// YSF.  Field 0 = mode, 1-3 = the ten target bytes, 4-6 = the ten source bytes, each group in words of its own; the record's 21
// bytes are put together from them.  ysf_meta.hpp:58-101 (mode, destination, source).
template <> struct DhDigest<DH_PROTO_YSF> {
    static constexpr int FIELDS = 7, GROUPS = 3, WORDS = 6, LEN = 21;
    static DH_HD int group_of(int f) { return f == 0 ? 0 : f < 4 ? 1 : 2; }
    static DH_HD void unpack(const uint32_t* w, uint32_t* F) {
        F[0] = w[0] & 0xFFu;
        F[1] = w[0] >> 8 | w[1] << 24; F[2] = w[1] >> 8 | w[2] << 24; F[3] = (w[2] >> 8) & 0xFFFFu;
        F[4] = w[2] >> 24 | w[3] << 8; F[5] = w[3] >> 24 | w[4] << 8; F[6] = w[4] >> 24 | (w[5] & 0xFFu) << 8;
    }
    static DH_HD void pack(const uint32_t* F, uint32_t* w) {
        w[0] = F[0] | F[1] << 8; w[1] = F[1] >> 24 | F[2] << 8; w[2] = F[2] >> 24 | F[3] << 8 | F[4] << 24;
        w[3] = F[4] >> 8 | F[5] << 24; w[4] = F[5] >> 8 | F[6] << 24; w[5] = (F[6] >> 8) & 0xFFu;
    }
    static DH_HD uint32_t parts(uint32_t) { return 1u; }
    static DH_HD void classify(const uint32_t* e, uint32_t* v, uint32_t& wr, uint32_t& pass) {
        const uint32_t type = e[1] & 0xFFu, a = (e[1] >> 8) & 0xFFu, b = (e[1] >> 16) & 0xFFu, len = e[1] >> 24;
        for (int f = 0; f < FIELDS; f++) v[f] = 0;
        wr = 0; pass = 0;
        if (type == DH_EV_YSF_MODE) { v[0] = 1u + (b & 3u); wr = 1u; }
        else if (type == DH_EV_YSF_META_RESET) wr = 7u;
        else if (type == DH_EV_YSF_DCH) {
            if (len >= 10 && a < 2u) {
                const int at = a ? 4 : 1;
                v[at] = e[2]; v[at + 1] = e[3]; v[at + 2] = e[4] & 0xFFFFu;
                wr = a ? 4u : 2u;
            } else pass = a >= 2u;
        } else if (type == DH_EV_YSF_HEADER_DCH) {
            if (len >= 20 && a == 0u) {                                        // CSD1: destination, source
                v[1] = e[2]; v[2] = e[3]; v[3] = e[4] & 0xFFFFu;
                v[4] = e[4] >> 16 | e[5] << 16; v[5] = e[5] >> 16 | e[6] << 16; v[6] = e[6] >> 16;
                wr = 6u;
            } else pass = a == 1u;
        }
    }
};

template <int PROTO>
DH_D void dh_call_digest_channel(const DhDigestParams& P, uint32_t ch) {
    using D = DhDigest<PROTO>;
    const uint32_t n = dh_uniform(dh_min(P.ev_count[ch], P.ev_cap));
    if (n == 0) return;                                                        // a channel that brought no events leaves at once
    uint32_t* const rec = P.state + (size_t) ch * P.state_stride + DS_CALL_RECORD;
    DhU4* const row = reinterpret_cast<DhU4*>(P.events + (size_t) ch * P.ev_stride);      // an event is two of them
    uint32_t w[DH_CALL_RECORD_WORDS] = { 0, 0, 0, 0, 0, 0 }, carry[DH_DIGEST_MAX_FIELDS];
    for (int i = 0; i < D::WORDS; i++) w[i] = dh_uniform(rec[i]);
    D::unpack(w, carry);
    uint32_t nout = 0;
    for (uint32_t base = 0; base < n; base += DH_WAVE) {
        DH_LANE_STRUCT(DhDigestLane, L);
        uint64_t writers[DH_DIGEST_MAX_GROUPS] = { 0, 0, 0, 0 }, keep = 0;
        // phase 1: the chunk into registers; what every event writes
        DH_FOR_LANES(lane) {
            DhDigestLane& me = DH_LS(L, lane);
            const bool valid = base + (uint32_t) lane < n;
            DhU4 lo = { 0, 0, 0, 0 }, hi = { 0, 0, 0, 0 };
            if (valid) { lo = row[2 * (size_t) (base + lane)]; hi = row[2 * (size_t) (base + lane) + 1]; }
            me.e[0] = lo.x; me.e[1] = lo.y; me.e[2] = lo.z; me.e[3] = lo.w; me.e[4] = hi.x; me.e[5] = hi.y; me.e[6] = hi.z; me.e[7] = hi.w;
            for (int f = 0; f < DH_DIGEST_MAX_FIELDS; f++) me.v[f] = 0;
            me.wr = 0; me.pass = 0;
            if (valid) D::classify(me.e, me.v, me.wr, me.pass);
#pragma unroll
            for (int g = 0; g < D::GROUPS; g++) DH_BALLOT_ACC(writers[g], (me.wr >> g) & 1u, lane);
        }
        // phase 2: the record in front of and behind every event; the output event where it differs
        DH_FOR_LANES(lane) {
            DhDigestLane& me = DH_LS(L, lane);
            const uint64_t below = ((uint64_t) 1 << lane) - 1u;
            uint32_t after[DH_DIGEST_MAX_FIELDS], changed = 0;
#pragma unroll
            for (int f = 0; f < D::FIELDS; f++) {
                const int g = D::group_of(f);
                const uint64_t m = writers[g] & below;
                const uint32_t x = DH_LS_GATHER(L, v[f], m ? dh_top64(m) : lane);
                const uint32_t before = m ? x : carry[f];
                after[f] = ((me.wr >> g) & 1u) ? me.v[f] : before;
                if (after[f] != before) changed |= 1u << f;
            }
            if (changed) {
                uint32_t r[DH_CALL_RECORD_WORDS];
                D::pack(after, r);
                me.e[1] = (uint32_t) DH_EV_CALL | D::parts(changed) << 8 | (uint32_t) D::LEN << 24;
                for (int i = 0; i < DH_CALL_RECORD_WORDS; i++) me.e[2 + i] = r[i];
            }
            DH_BALLOT_ACC(keep, changed != 0u || me.pass != 0u, lane);
        }
        // the record behind the chunk: every group as its last writer left it
#pragma unroll
        for (int f = 0; f < D::FIELDS; f++) {
            const uint64_t m = writers[D::group_of(f)];
            if (m) carry[f] = DH_LS_READ(L, v[f], dh_uniform((uint32_t) dh_top64(m)));
        }
        // phase 3: stable compaction
        DH_FOR_LANES(lane) {
            const DhDigestLane& me = DH_LS(L, lane);
            if ((keep >> lane) & 1ull) {
                const size_t at = nout + DH_LANES_BELOW(keep, lane);
                const DhU4 lo = { me.e[0], me.e[1], me.e[2], me.e[3] }, hi = { me.e[4], me.e[5], me.e[6], me.e[7] };
                row[2 * at] = lo; row[2 * at + 1] = hi;
            }
        }
        nout += (uint32_t) dh_popc64(keep);
    }
    if (dh_is_writer_lane()) {
        P.ev_count[ch] = nout;
        D::pack(carry, w);
        for (int i = 0; i < D::WORDS; i++) rec[i] = w[i];
    }
}

// ---------------------------------------------------------------------------------- the launch
namespace {

template <int PROTO>
__global__ __launch_bounds__(DH_WAVE) void k_call_digest(const DhDigestParams P) {
    dh_call_digest_channel<PROTO>(P, blockIdx.x);
}

}  // namespace

template <class BE> static int dh_be_call_digest(BE& be, const DhDigestParams& P, int proto) {
    void (*const k)(const DhDigestParams) = proto == DH_PROTO_DMR ? k_call_digest<DH_PROTO_DMR> : proto == DH_PROTO_YSF ? k_call_digest<DH_PROTO_YSF> : k_call_digest<DH_PROTO_NXDN>;
    return dh_launch(k, dim3(P.n_channels), dh_workgroup(DH_WAVE), 0, dh_be_stream(be, 0), "k_call_digest", P);
}
