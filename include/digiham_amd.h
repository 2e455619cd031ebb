/*
 * digiham_amd.h -- C ABI of the MI355X-native many-channel digital-voice
 * demodulation / FEC engine (libdigiham_amd.so).
 *
 * This is the drop-in boundary for digiham's hot path
 *     rrc_filter -> gfsk_demodulator / fsk_demodulator -> dmr_decoder / ysf_decoder
 * (+ digitalvoice_filter).  Plain C types, caller-owned buffers, `int` return
 * (0 = ok, negative = DH_E*), no exceptions across the ABI.  The host-side
 * C++ classes in include/digiham/ (same names and constructor signatures as
 * the reference's include/ headers) and the Python binding in digiham_amd/ sit on
 * top of exactly these entry points.
 *
 * Pointer conventions
 *   d_*   device pointers (HBM; hipMalloc / torch CUDA tensors)
 *   h_*   host pointers
 *   stream: a hipStream_t passed as void* (NULL = the HIP default stream)
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the reference root, jketterl/digiham v0.7.0-dev).
 */
#ifndef DIGIHAM_AMD_H
#define DIGIHAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_OK        0
#define DH_EINVAL   -1   /* bad argument */
#define DH_ENOMEM   -2   /* device allocation failed */
#define DH_EDEVICE  -3   /* HIP runtime error (see dh_last_error) */
#define DH_ENODEV   -4   /* no gfx950 device visible */
#define DH_ECAPACITY -5  /* an output buffer overflowed; results truncated */

const char* dh_version(void);
/* last HIP error string recorded on this thread ("" if none) */
const char* dh_last_error(void);
/* number of visible HIP devices, or a negative DH_E* code */
int dh_device_count(void);

/* small memory helpers so that C / C++ hosts need no HIP headers (synchronous) */
int dh_device_alloc(int device, size_t bytes, void** d_out);
int dh_device_free(void* d_ptr);
int dh_copy_to_host(void* h_dst, const void* d_src, size_t bytes);
int dh_copy_to_device(void* d_dst, const void* h_src, size_t bytes);

/* ------------------------------------------------------------------------
 * Stateless batch FEC kernels (one codeword / block per lane).
 * Replace the C functions under src/dmr_decoder and src/ysf_decoder.
 * All arrays are device pointers; `ok` receives 1/0 per item.
 * ---------------------------------------------------------------------- */
/* bool hamming_7_4(uint8_t*)      src/dmr_decoder/hamming_7_4.c:56-72  */
int dh_hamming_7_4(uint8_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool hamming_13_9(uint16_t*)    src/dmr_decoder/hamming_13_9.c:70-84 */
int dh_hamming_13_9(uint16_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool hamming_15_11(uint16_t*)   src/dmr_decoder/hamming_15_11.c:74-88 */
int dh_hamming_15_11(uint16_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool hamming_16_11(uint16_t*)   src/dmr_decoder/hamming_16_11.c:79-93 */
int dh_hamming_16_11(uint16_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool quadratic_residue(uint16_t*) src/dmr_decoder/quadratic_residue.c:321-335 */
int dh_quadratic_residue(uint16_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool golay_20_8(uint32_t*)      src/dmr_decoder/golay_20_8.c:1421-1435 */
int dh_golay_20_8(uint32_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool golay_24_12(uint32_t*)     src/ysf_decoder/golay_24_12.c:2401-2415 */
int dh_golay_24_12(uint32_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool bch_31_21(uint32_t*)       src/pocsag_decoder/bch_31_21.c:545-561 (31-bit words, up to 2 errors) */
int dh_bch_31_21(uint32_t* d_words, uint8_t* d_ok, size_t n, void* stream);
/* bool bptc_196_96(uint8_t payload[25], uint8_t output[12])  src/dmr_decoder/bptc_196_96.c:5-59
 * d_in [n][25] -> d_out [n][12] (zero-filled when ok == 0) */
int dh_bptc_196_96(const uint8_t* d_in, uint8_t* d_out, uint8_t* d_ok, size_t n, void* stream);
/* uint8_t decode_trellis(uint8_t* input, uint8_t size, uint8_t* output)  src/ysf_decoder/trellis.c:32-109
 * d_in [n][in_stride] dibits packed 4 per byte MSB first; n_dibits <= 192;
 * d_out [n][out_stride] decoded bits (ceil(n_dibits/8) bytes used); d_metric [n] */
int dh_trellis(const uint8_t* d_in, size_t in_stride, int n_dibits,
               uint8_t* d_out, size_t out_stride, uint8_t* d_metric, size_t n, void* stream);
/* uint16_t crc16_checksum(uint8_t* data, int count)  src/ysf_decoder/crc16.c:3-18 */
int dh_crc16(const uint8_t* d_in, size_t stride, int count, uint16_t* d_out, size_t n, void* stream);
/* void decode_whitening(uint8_t* in, uint8_t* out, uint8_t num)  src/ysf_decoder/whitening.c:6-22
 * in/out [n][stride]; ceil(n_bits/8) bytes per row are written */
int dh_whitening(const uint8_t* d_in, uint8_t* d_out, size_t stride, int n_bits, size_t n, void* stream);

/* ------------------------------------------------------------------------
 * Streaming engine: B independent channels, per-channel state resident in HBM.
 * Replaces one `rrc_filter | gfsk_demodulator | dmr_decoder` process chain
 * per channel (examples/dmr-decoder.sh:19-23, examples/ysf-decoder.sh:19-23):
 *   Digiham::RrcFilter::{Wide,Narrow}RrcFilter::process   src/rrc_filter/rrc_filter.cpp:16-34
 *   Digiham::Fsk::GfskDemodulator::process                src/gfsk_demodulator/gfsk_demodulator.cpp:24-122
 *   Digiham::Fsk::FskDemodulator::process                 src/fsk_demodulator/fsk_demodulator.cpp:25-112
 *   Digiham::Decoder::process + Dmr/Ysf phases            src/lib/decoder.cpp:21-47,
 *                                                         src/dmr_decoder/dmr_phase.cpp:18-302,
 *                                                         src/ysf_decoder/ysf_phase.cpp:16-349
 * ---------------------------------------------------------------------- */
typedef struct dh_engine dh_engine;

enum { DH_RRC_NONE = 0, DH_RRC_WIDE = 1, DH_RRC_NARROW = 2,
       DH_RRC_CUSTOM = 3 };   /* the caller's coefficient table: RrcFilter(nZeros, gain, coeffs[]), include/rrc_filter.hpp:12 */
enum { DH_DEMOD_NONE = 0, DH_DEMOD_FSK2 = 2, DH_DEMOD_GFSK4 = 4 };
enum { DH_PROTO_NONE = 0, DH_PROTO_DMR = 1, DH_PROTO_YSF = 2, DH_PROTO_NXDN = 3, DH_PROTO_POCSAG = 4, DH_PROTO_DSTAR = 5,
       DH_PROTO_SCAN = 6 };   /* no decoder: the sync words of all five protocols, counted ("Protocol scan" below) */

/* flags */
#define DH_FLAG_FAST_FIR        0x1   /* FMA FIR: float outputs within 1e-6 of the reference, dibits NOT guaranteed bit-exact */
#define DH_FLAG_KEEP_FILTERED   0x2   /* also materialise the RRC output [B][n] (unfused path; BASELINE config 2) */
#define DH_FLAG_FSK_INVERT      0x4   /* FskDemodulator(sps, invert = true) */
#define DH_FLAG_NO_EVENTS       0x8   /* do not record decoder events */
#define DH_FLAG_SPLIT_STAGES    0x20  /* launch slicer and decoder as two kernels even where the one-wavefront chain kernel exists */
#define DH_FLAG_ORDERED_TIMING  0x10  /* always run the in-order variance chain of the timing recovery (diagnostic; results are identical) */
#define DH_FLAG_EXACT_SYMBOLS   0x40  /* error-bounded kernels: decide EVERY symbol with the reference's arithmetic (diagnostic; results are identical) */
#define DH_FLAG_EXACT_FIR       0x80  /* error-bounded kernels: run the rounded-product FIR in every run (diagnostic / A-B; results are identical) */
#define DH_FLAG_ONE_LAUNCH      0x200 /* with DH_FLAG_KEEP_FILTERED on the wide filter at 10 samples per symbol: `rrc_filter | gfsk_demodulator` as ONE kernel per push -- the
                                         error-bounded slicer kernel (dibits bit-exact, as without the flag) also stores the filtered samples it holds in LDS.  They come from
                                         its split-f16 matrix-core FIR: within 2.5e-6 of the reference's floats relative to max(|ref|, rms(ref)) (measured 1.0e-6), which is
                                         NOT the 1e-6 of DH_FLAG_FAST_FIR and not bit-exact.  With DH_FLAG_FAST_FIR set as well the one kernel filters with the f32 FMA chain
                                         instead (on the matrix cores, v_mfma_f32_16x16x4_f32: the floats of DH_FLAG_FAST_FIR, within 1e-6, measured 5e-7) and -- unlike
                                         DH_FLAG_FAST_FIR alone -- still delivers the reference's dibits bit for bit (error radius + exact re-evaluation of what it leaves in
                                         doubt): BASELINE configs[1] in one launch.  (The reference's own 81-term float chain is 8e-7 away from the exact
                                         convolution and the split-f16 FIR 1.3e-7: most of the distance is the reference's rounding, which only its own order of operations reproduces.) */
#define DH_FLAG_OVERLAP_PUSHES  0x100 /* engines of >= 8192 channels on the one-launch chains (DMR, YSF, NXDN, D-Star): a push goes out as two launches on two streams of the engine's
                                         own (three quarters of the channels at high priority, the rest at normal priority) which are ordered
                                         after the caller's stream at the moment of the push and joined with it again only when results are
                                         read, the engine is reset / synchronised or another kind of work is queued -- so the drain of one
                                         launch is filled by the next, across pushes.  CONTRACT: the input buffer of a push must stay
                                         untouched until dh_engine_sync() (or any read) returns, and the raw device
                                         views of the outputs (dh_engine_symbols / _frames / _events) are only valid after dh_engine_sync().
                                         Results are identical. */
#define DH_FLAG_DMR_BOTH_SLOTS  0x400 /* proto == DH_PROTO_DMR only (DH_EINVAL otherwise, before anything is allocated): the voice of BOTH timeslots of a
                                         channel leaves the decoder, as slot-tagged records ("DMR: both timeslots" below).  Off: the reference's one output
                                         pipe, one active slot at a time, records of 27 untagged bytes. */

/* ----------------------------------------------------------------------
 * DMR: both timeslots (DH_FLAG_DMR_BOTH_SLOTS).  Own specification, held to the reference through its slot filter.
 *
 * The reference's FramePhase has one output pipe and therefore one activeSlot (dmr_phase.cpp:207-231): while a call holds
 * it, the voice bursts of the other slot are dropped.  In this mode, fixed when the engine is created:
 *
 * Gate.  A voice burst -- one whose slot has syncTypes[slot] == VOICE after the burst's own bookkeeping (:207) -- is emitted
 * iff (slot + 1) & slot_filter.  activeSlot takes no part and is never claimed: it stays -1.
 *
 * Records.  The frames row of a channel is a sequence of DH_DMR_SLOT_RECORD_BYTES = 28 byte records in burst order: the 27
 * payload bytes of :213-226, then one tag byte, the slot (0 or 1; its upper seven bits are 0).
 *
 * Contract.  For every channel, every slot filter f in 0..3 and any way the stream is cut into pushes, the payloads of the
 * records tagged s, in order, are byte for byte the frames of the decoder without the flag on the same input at slot
 * filter f & (s + 1); the events are the decoder's at any filter (they never depended on it); the symbols are untouched.
 * Concatenated over a stream, the frames bytes do not depend on how the stream is cut into pushes.
 *
 * Capacity.  The frames row holds (max_syms / 144 + 1) * 28 bytes, rounded up to 64: a voice burst in every burst position
 * of a push fits, so the row cannot overflow in this mode.
 *
 * dh_engine_set_slot_filter and _channel keep their meaning (bits 0 and 1 of the filter; higher bits are ignored) and do
 * not switch the mode; dh_engine_reset, _reset_channel and _reset_channels keep it.
 * ---------------------------------------------------------------------- */
#define DH_DMR_SLOT_RECORD_BYTES 28

#define DH_FLAG_CALL_DIGEST     0x800 /* proto DH_PROTO_DMR, DH_PROTO_YSF or DH_PROTO_NXDN only, and neither with DH_FLAG_NO_EVENTS nor with
                                         DH_FLAG_OVERLAP_PUSHES (DH_EINVAL otherwise, before anything is allocated): every push ends with one more
                                         launch, k_call_digest, that folds the channel's events into its call record and rewrites the event row in
                                         place ("Call digest" below).  Off: the raw events, no extra launch, allocation or state word. */

/* ----------------------------------------------------------------------
 * Call digest (DH_FLAG_CALL_DIGEST).  Own specification; the updates are those of the reference's MetaCollectors on their
 * identity fields (src/dmr_decoder/dmr_meta.cpp:11-179 with its call sites dmr_phase.cpp:80, :109-114, :178-184, :196-202,
 * :279-282, :304-339 and lc.cpp:26-43; src/nxdn_decoder/nxdn_meta.cpp:52-75 with nxdn_phase.cpp:51, :115-121, :141, :157;
 * src/ysf_decoder/ysf_meta.cpp:47-93 with ysf_phase.cpp:73-163, :270-287), as include/digiham/{dmr,nxdn,ysf}_meta.hpp replay them.
 *
 * Records.  Every channel owns one call record in its decoder state.  It is zero after create and after any reset
 * (dh_engine_reset, _reset_channel, _reset_channels); a reset raises no event.
 *   DMR, 16 bytes, slot s at bytes [8 s, 8 s + 8): byte 0 sync (0 none, 1 data, 2 voice, 3 any other sync type), byte 1 type
 *     (0 none, 1 group, 2 direct), bytes 2-4 source, bytes 5-7 target (24 bits each, big endian).
 *   NXDN, 8 bytes: byte 0 sync (0 none, 1 voice), byte 1 type (0 none, 1 conference, 2 individual), bytes 2-3 source, bytes
 *     4-5 destination (big endian), bytes 6-7 zero.
 *   YSF, 21 bytes: byte 0 mode (0 none, otherwise 1 + (b & 3) of the MODE event), bytes 1-10 target, bytes 11-20 source (the
 *     ten raw bytes as carried).
 *
 * Fold.  The raw events of a push are visited in row order; each applies one update.
 *   DMR, s = a & 1.  SYNC: sync of s = b (1, 2; anything else: 3), and if len > 0 && payload[0], type, source and target of s
 *     become 0.  SLOT_RESET (either b): all four fields of s become 0.  META_RESET: both slots become 0.  SOFT_RESET: type,
 *     source and target of s become 0.  LC with len >= 9 and opcode group (0) or unit-to-unit (3): type = 1 or 2, target =
 *     payload bytes 3-5, source = payload bytes 6-8 (Digiham::Dmr::Lc).  Every other event leaves the record alone.
 *   NXDN.  SYNC_VOICE: sync = 1.  SACCH_SF with len >= 9 and (payload[0] & 0x3F) == 1 (VCALL): type from payload[2] >> 5
 *     (1 conference -> 1, 4 individual -> 2, others 0), source = payload bytes 3-4, destination = bytes 5-6.  META_RESET: all 0.
 *   YSF.  MODE: mode = 1 + (b & 3).  DCH with len >= 10: a = 0 sets target = payload[0, 10), a = 1 sets source.  HEADER_DCH with
 *     len >= 20 and a = 0: target = payload[0, 10), source = payload[10, 20).  META_RESET: all 0.
 *
 * Output.  Every raw event yields at most one output event at its place, order kept (a stable compaction):
 *   - the update changed a byte of the record: one DH_EV_CALL event, sym_index the raw event's, a = which parts changed (DMR:
 *     bit s for slot s, so a META_RESET may give 3; NXDN and YSF: 1), b = 0, len = 16, 8 or 21, payload = the whole record
 *     after the update, 0 beyond len;
 *   - otherwise the event is copied bit for bit if it is a pass-through event -- DMR: LC whose opcode is a talker-alias block
 *     or GPS info (4 .. 8: LC_TALKER_ALIAS_HDR .. LC_GPS_INFO of include/digiham/lc.hpp); YSF: DCH with a >= 2, HEADER_DCH with
 *     a = 1; NXDN: none;
 *   - otherwise it is dropped (EMB, SLOTTYPE, BPTC, FICH, LICH, SACCH fragments, FACCH1, and every event that repeats what the
 *     record already says).
 *
 * Properties.  The new count never exceeds the old one (row capacities are unchanged); no byte beyond the new count is
 * defined.  Concatenated over a stream, the digested events do not depend on how the stream is cut into pushes: the record
 * carries over.  A row the decoder truncated (DH_ECAPACITY) is digested as far as it was kept.  Frames, symbols, statistics
 * and the slot filter are untouched.  Combines freely with DH_FLAG_DMR_BOTH_SLOTS, DH_FLAG_SPLIT_STAGES and decoder-only
 * engines (dh_engine_push_symbols); dh_engine_events, dh_engine_read_events and dh_outpack_append see the digested row.
 * (dh_monitor creates its engines itself and has no field for the flag: its configuration struct keeps its size.)
 * ---------------------------------------------------------------------- */
#define DH_CALL_RECORD_DMR_BYTES 16
#define DH_CALL_RECORD_NXDN_BYTES 8
#define DH_CALL_RECORD_YSF_BYTES 21

typedef struct {
    uint32_t struct_size;     /* = sizeof(dh_engine_config) */
    int32_t  device;          /* HIP device ordinal */
    uint32_t n_channels;      /* B */
    uint32_t max_samples;     /* largest n a single push may carry (per channel) */
    int32_t  rrc;             /* DH_RRC_* */
    int32_t  demod;           /* DH_DEMOD_* */
    uint32_t sps;             /* samples per symbol (GfskDemodulator / FskDemodulator ctor argument) */
    int32_t  proto;           /* DH_PROTO_* */
    uint32_t flags;
    uint32_t slot_filter;     /* Dmr::Decoder::setSlotFilter initial value (3 = both slots) */
    void*    stream;          /* hipStream_t all work is enqueued on (NULL: default stream) */
    /* rrc == DH_RRC_CUSTOM only (struct_size must cover these fields): y[n] = (float)((double) sum_i rrc_taps[i] x[n - nZeros + i] / rrc_gain),
     * products and sums rounded to float one by one in tap order (src/rrc_filter/rrc_filter.cpp:22-34).  The table
     * (host memory, rrc_nzeros + 1 floats, 1 <= rrc_nzeros <= 160, any shape) is copied at create time.  A custom filter
     * is never fused into the slicer: the filtered signal is materialised and the demodulator (if any) reads it. */
    const float* rrc_taps;
    uint32_t rrc_nzeros;
    double   rrc_gain;
} dh_engine_config;
/* sizeof(dh_engine_config) before the custom-filter fields were added: still accepted as struct_size */
#define DH_ENGINE_CONFIG_V1_SIZE offsetof(dh_engine_config, rrc_taps)

/* Decoder event: one record per call the reference makes into its MetaCollector,
 * plus the FEC-corrected words feeding it (BPTC LC, slot type, EMB, FICH, DCH). */
typedef struct {
    uint32_t sym_index;       /* absolute symbol index of the frame start (mod 2^32): the first symbol of the burst, frame or
                               * codeword that raises the event.  The events raised between frames carry the first symbol not
                               * yet consumed: D-Star HEADER (radio header) and VOICE_START, raised once the 660 header bits /
                               * the voice sync pattern are behind, carry the first symbol of the first voice frame */
    uint8_t  type;            /* DH_EV_* */
    uint8_t  a;               /* DMR slot / YSF frame number or CSD index */
    uint8_t  b;               /* sub-type (sync type, data type, lcss, reset cause) */
    uint8_t  len;             /* valid payload bytes */
    uint8_t  payload[24];
} dh_event;

enum {
    /* DMR (src/dmr_decoder/dmr_phase.cpp): SLOT_RESET b = 1 when it is the OTHER slot that is reset after a TACT slot switch
     * (:80 -- the reference leaves that slot's talker alias collector alone until its next burst), 0 otherwise */
    DH_EV_DMR_SYNC = 1, DH_EV_DMR_SLOT_RESET = 2, DH_EV_DMR_META_RESET = 3, DH_EV_DMR_LC = 4,
    DH_EV_DMR_SOFT_RESET = 5, DH_EV_DMR_BPTC = 6, DH_EV_DMR_SLOTTYPE = 7, DH_EV_DMR_EMB = 8,
    DH_EV_YSF_FICH = 16, DH_EV_YSF_MODE = 17, DH_EV_YSF_DCH = 18, DH_EV_YSF_HEADER_DCH = 19,
    DH_EV_YSF_META_RESET = 20,
    /* NXDN48 (src/nxdn_decoder/nxdn_phase.cpp): LICH byte; SACCH fragment (a = structure index, 5 bytes); complete SACCH
     * superframe (9 bytes); setSync("voice"); FACCH1 (a = block, 12 bytes); MetaCollector::reset (b = 0 sync loss, 1 TX_RELEASE) */
    DH_EV_NXDN_LICH = 32, DH_EV_NXDN_SACCH = 33, DH_EV_NXDN_SACCH_SF = 34, DH_EV_NXDN_SYNC_VOICE = 35,
    DH_EV_NXDN_FACCH1 = 36, DH_EV_NXDN_META_RESET = 37,
    /* POCSAG (src/pocsag_decoder/pocsag_phase.cpp:56-57): a = position in the batch, payload = BCH-corrected codeword (big endian) */
    DH_EV_POCSAG_CODEWORD = 48,
    /* D-Star (src/dstar_decoder/dstar_phase.cpp): HEADER = setFromHeader of a CRC-valid voice header, 41 bytes over two
     * events (a = 0: bytes 0-23, a = 1: bytes 24-40; b = 0 radio header (:50), 1 slow-data header (:214)); VOICE_START =
     * a new VoicePhase (b = 1 after a header, 0 after a voice sync); SYNC_VOICE = setSync("voice") (:110); MESSAGE = the
     * 20-character slow-data message (:207); SIMPLE = len simple-data bytes appended (:178); FRAME_SYNC = parseFrameData
     * (:113): the consumer now parses its simple-data lines (DPRS / NMEA, :218-245); META_RESET = MetaCollector::reset
     * (b = 0 terminator, 1 sync lost) */
    DH_EV_DSTAR_HEADER = 64, DH_EV_DSTAR_VOICE_START = 65, DH_EV_DSTAR_SYNC_VOICE = 66, DH_EV_DSTAR_MESSAGE = 67,
    DH_EV_DSTAR_SIMPLE = 68, DH_EV_DSTAR_FRAME_SYNC = 69, DH_EV_DSTAR_META_RESET = 70,
    /* protocol scan: a sync pattern found (sym_index = its first symbol, a = DH_SCAN_* pattern, b = distance, len = 0) */
    DH_EV_SCAN_HIT = 80,
    /* call digest (DH_FLAG_CALL_DIGEST): the channel's call record changed (a = parts changed, len = 16 / 8 / 21 for DMR / NXDN /
     * YSF, payload = the record after the change) */
    DH_EV_CALL = 96
};

/* ----------------------------------------------------------------------
 * Protocol scan (DH_PROTO_SCAN): which protocol does a channel carry?  Own specification; the reference has no
 * counterpart (there one person picks one mode for one channel).  The decoder stage of such an engine is a free-running
 * correlator with no frame state machine: behind whatever front end the engine was created with, EVERY symbol position
 * is tested against the nine sync patterns the five decoders search for, with the decoders' own tests:
 *
 *   DH_SCAN_DMR_BS_DATA .. DH_SCAN_DMR_MS_VOICE   24 dibits   distance <= 3   Dmr::SyncPhase (dmr_phase.cpp:18-33), each of the four on its own
 *   DH_SCAN_YSF                                   20 dibits   distance <= 3   ysf_phase.cpp:16-18
 *   DH_SCAN_NXDN                                  10 dibits   distance <= 2   nxdn_phase.cpp:21
 *   DH_SCAN_DSTAR_HEADER                          24 bits     distance <= 2   dstar_phase.cpp:17-34
 *   DH_SCAN_DSTAR_VOICE                           24 bits     distance <= 1   dstar_phase.cpp:17-34 (also where the header pattern hits)
 *   DH_SCAN_POCSAG                                32 bits     distance <= 3   pocsag_phase.cpp:18-28
 *
 * The distance is the number of differing bits; against a pattern of bits a symbol 2 or 3 counts one more.  All nine are
 * tested whatever the front end; there is no configuration word.
 *
 * Positions.  p counts the channel's symbols since create or reset, modulo 2^32.  Position p is examined, for all nine
 * patterns, in the push that brings symbol p + 31, and never again: at most 31 symbols are carried between pushes, and
 * the last 31 positions of a stream stay unexamined until more symbols arrive.  Nothing depends on how the stream is
 * cut into pushes.
 *
 * Events.  A hit is one dh_event: type DH_EV_SCAN_HIT, sym_index = p, a = pattern, b = distance, len = 0; in ascending p,
 * then ascending pattern.  When the event row is full the push reports DH_ECAPACITY and the events are truncated; the
 * statistics still count every hit.
 *
 * Statistics.  The "frames" row of the channel (dh_engine_frames / dh_engine_read_frames: 144 bytes) holds
 * dh_scan_stat[DH_SCAN_PATTERNS], cumulative since create or reset and rewritten by every push: hits, the hits that
 * were periodic, the position of the last hit, the smallest distance seen (255 before the first hit).
 *
 * Periodic hits.  The patterns form five families with the distances, in symbols, between sync words of a running
 * transmission: DMR (the four DMR patterns) {144, 288}; YSF {480}; NXDN {192}; D-Star (header, voice) {2016} -- 21
 * frames of 96 bits; POCSAG {544} -- the sync word and 16 codewords.  Every family remembers the two most recent
 * distinct positions at which one of its patterns hit.  A hit at p counts as periodic when p - q (unsigned) is one of
 * the family's distances for a remembered q; all patterns that hit at p are judged against the positions before p, then
 * p is remembered, once.  A single hit says little -- the NXDN test passes on random dibits about once in 5 000
 * positions -- a hit one frame behind another says a lot.
 * ---------------------------------------------------------------------- */
enum { DH_SCAN_DMR_BS_DATA = 0, DH_SCAN_DMR_BS_VOICE = 1, DH_SCAN_DMR_MS_DATA = 2, DH_SCAN_DMR_MS_VOICE = 3, DH_SCAN_YSF = 4,
       DH_SCAN_NXDN = 5, DH_SCAN_DSTAR_HEADER = 6, DH_SCAN_DSTAR_VOICE = 7, DH_SCAN_POCSAG = 8, DH_SCAN_PATTERNS = 9 };
typedef struct { uint32_t hits, periodic, last_sym; uint8_t best_dist, pad[3]; } dh_scan_stat;

int  dh_engine_create(const dh_engine_config* cfg, dh_engine** out);
void dh_engine_destroy(dh_engine* e);
/* back to the freshly-constructed state of every module (zeroed delay lines, SyncPhase) */
int  dh_engine_reset(dh_engine* e);
/* Dmr::Decoder::setSlotFilter (src/dmr_decoder/dmr_decoder.cpp:9-15) for every channel */
int  dh_engine_set_slot_filter(dh_engine* e, uint32_t filter);

/* Feed n new samples per channel (n <= max_samples).  d_samples is [B][stride]
 * float32, channel-major, resident in HBM.  Asynchronous on the engine stream.
 * Outputs of this push replace those of the previous push.  n = 0 is a valid (empty) push; d_samples may then be NULL. */
int  dh_engine_push(dh_engine* e, const float* d_samples, size_t stride, size_t n);
/* same, from host memory (staged through an engine-owned device buffer) */
int  dh_engine_push_host(dh_engine* e, const float* h_samples, size_t stride, size_t n);
/* One channel of a many-channel engine: back to the freshly-constructed state / Dmr::Decoder::setSlotFilter for it alone
 * (the other channels keep streaming).  What a module instance attached to a shared engine needs. */
int  dh_engine_reset_channel(dh_engine* e, uint32_t channel);
int  dh_engine_set_slot_filter_channel(dh_engine* e, uint32_t channel, uint32_t filter);
/* dh_engine_reset_channel for every channel b with d_flags[b] != 0 (n_channels bytes on the device), in ONE launch however
 * many are flagged: a flagged channel ends in exactly the state dh_engine_reset_channel leaves it in, the others are not
 * touched.  Asynchronous on the engine stream; the flags are read when the launch runs. */
int  dh_engine_reset_channels(dh_engine* e, const uint8_t* d_flags);
/* Ragged pushes: channel b brings d_counts[b] (<= max_n) new samples of its row; the others stay where they are.  One launch
 * for N module instances whose ring buffers hold different amounts (include/digiham/shared_engine.hpp); a real-time receiver
 * whose channels arrive in blocks of unequal length.  Engines with a foreign tap table (DH_RRC_CUSTOM) take whole pushes only. */
int  dh_engine_push_ragged(dh_engine* e, const float* d_in, size_t stride, const uint32_t* d_counts, size_t max_n);
int  dh_engine_push_host_ragged(dh_engine* e, const float* h_in, size_t stride, const uint32_t* h_counts, size_t max_n);

/* Device views of the current push's outputs (valid until the next push).
 * Any out-pointer may be NULL. counts are uint32 [B]. */
int  dh_engine_filtered(dh_engine* e, const float** d_filtered, size_t* stride);           /* needs DH_FLAG_KEEP_FILTERED */
int  dh_engine_symbols(dh_engine* e, const uint8_t** d_syms, size_t* stride, const uint32_t** d_count);
int  dh_engine_frames(dh_engine* e, const uint8_t** d_bytes, size_t* stride, const uint32_t** d_count);
int  dh_engine_events(dh_engine* e, const dh_event** d_events, size_t* stride, const uint32_t** d_count);
/* Host copies for one channel (synchronises the engine stream). *n in: capacity, out: count */
int  dh_engine_read_symbols(dh_engine* e, uint32_t channel, uint8_t* h_out, size_t* n);
int  dh_engine_read_frames(dh_engine* e, uint32_t channel, uint8_t* h_out, size_t* n);
int  dh_engine_read_events(dh_engine* e, uint32_t channel, dh_event* h_out, size_t* n);
int  dh_engine_read_filtered(dh_engine* e, uint32_t channel, float* h_out, size_t* n);
/* Per-stage device timing (HIP events recorded on the engine stream around each stage of a push):
 * enable once with the number of pushes to keep; read returns, for each recorded push, the
 * milliseconds spent in the stand-alone RRC stage (0 when fused), the slicer (fused RRC+GFSK)
 * kernel and the decoder kernel.  *n in: capacity of the arrays, out: pushes recorded. */
int  dh_engine_timing_enable(dh_engine* e, uint32_t max_pushes);
int  dh_engine_timing_read(dh_engine* e, float* rrc_ms, float* slicer_ms, float* decoder_ms, uint32_t* n);
/* For pushes that went out as two launches (DH_FLAG_OVERLAP_PUSHES): duration of the FIRST launch alone (events on the
 * engine's high-priority stream) and the number of channels it covered (0 / 0 for a push with one launch).  Call BEFORE
 * dh_engine_timing_read, which starts a new series; the stage times of such a push on the caller's stream are ~0. */
int  dh_engine_timing_read_split(dh_engine* e, float* first_ms, uint32_t* first_channels, uint32_t* n);
/* Timing-recovery statistics since create/reset, per channel (host arrays of n_channels, either may be NULL):
 * blocks = 100-symbol variance blocks evaluated (gfsk_demodulator.cpp:41-80), ordered = those in which the
 * error-bounded estimate could not separate the phases and the reference's in-order sums decided. Synchronises. */
int  dh_engine_timing_stats(dh_engine* e, uint32_t* h_blocks, uint32_t* h_ordered);
/* Diagnostic: word `word` (0..31) of every channel's slicer state header, or word `word - 100` (0..63) of its
 * decoder state, or word `word - 200` (0..15) of the engine's own flag block (the same value for every channel; 202 =
 * hand-overs inside split launches that did not come and were finished by the fix-up launch), into h_out[n_channels].
 * Synchronises. */
int  dh_engine_debug_header(dh_engine* e, uint32_t word, uint32_t* h_out);
/* wait for all enqueued work; returns DH_ECAPACITY if any channel overflowed an output buffer */
int  dh_engine_sync(dh_engine* e);

/* Standalone decoder stage over symbols (for pipes that already have dibits):
 * d_syms [B][stride] uint8 dibits (values 0..3), d_count[B] valid symbols per channel. Requires
 * proto != NONE and an engine created with rrc = NONE, demod = DH_DEMOD_NONE (max_samples then
 * bounds the symbols per push). */
int  dh_engine_push_symbols(dh_engine* e, const uint8_t* d_syms, size_t stride, const uint32_t* d_count);

/* ------------------------------------------------------------------------
 * Digital voice post-filter, B independent int16 streams, state carried.
 * Replaces Digiham::DigitalVoice::DigitalVoiceFilter::process
 * (src/digitalvoice_filter/digitalvoice_filter.cpp:6-10,34-45).
 * d_state: [B][22] floats (xv[11], yv[11]) zero-initialised by the caller.
 * ---------------------------------------------------------------------- */
int dh_dvfilter_s16(const int16_t* d_in, int16_t* d_out, float* d_state, size_t n_channels, size_t stride, size_t n, void* stream);

/* ------------------------------------------------------------------------
 * Receiver front-end, B independent streams, state carried: what examples/dmr-decoder.sh:13-17 runs in front of
 * rrc_filter -- `rtl_fm -M fm -s 48000 | csdr convert -i s16 -o float | csdr dcblock` (third-party tools, no source in the
 * reference: the arithmetic is this library's own specification, digiham_amd/csrc/frontend_core.hpp).
 *   mode DH_FE_AUDIO_S16  d_in [B][in_stride] int16 FM-discriminator audio            -> x = s16 / 32768
 *   mode DH_FE_IQ_S16     d_in [B][in_stride] int16, interleaved I / Q (2 n values)    -> x = arg(z[n] conj(z[n-1])) / pi
 *   dcblock != 0          y[n] = (x[n] - x[n-1]) + 0.995 y[n-1]
 * d_out [B][out_stride] float32 is what dh_engine_push takes.  d_state: [B][4] floats, zero-initialised by the caller.
 * ---------------------------------------------------------------------- */
enum { DH_FE_AUDIO_S16 = 1, DH_FE_IQ_S16 = 2 };
int dh_frontend_s16(const int16_t* d_in, size_t in_stride, float* d_out, size_t out_stride, float* d_state,
                    size_t n_channels, size_t n, int mode, int dcblock, void* stream);

/* ------------------------------------------------------------------------
 * Channelizer: ONE wideband complex stream -> n_channels rows at input_rate / decimation, a bank of digital down-converters
 * (this library's own stage; the arithmetic, bit for bit, is specified in digiham_amd/csrc/channelizer_core.hpp).
 * Channel b: NCO increment increments[b] = offset_b / input_rate * 2^32 (two's complement for negative offsets), the real
 * low-pass taps[0..n_taps) rotated to the channel, output j at input index j * decimation + decimation - 1.
 *   input_format  DH_CZ_CS16 interleaved int16 I / Q (scaled by 2^-15), DH_CZ_CF32 interleaved float32
 *   output_mode   DH_CZ_IQ_F32 interleaved complex float rows, DH_CZ_FM arg(z[j] conj(z[j-1])) / pi (what dh_engine_push takes),
 *                 dcblock != 0 (FM only): y = (x - x[-1]) + 0.995 y[-1] as in dh_frontend_s16
 * Limits: 1 <= decimation <= 1024, 1 <= n_taps <= 16384 (finite), 1 <= n_channels <= 65536, 1 <= max_input <= 2^28.
 * Rational rates: interpolation = L > 1 gives rows at input_rate * L / decimation (2.048 MS/s -> 48 kS/s is 3 / 128).  taps is
 * then the low-pass at the virtual rate L * input_rate, with about L at DC for unity gain; output j sits at input index
 * floor((j * decimation + decimation - 1) / L), and after N input samples exactly floor(L N / decimation) outputs exist.
 * Limits: L <= 64, L <= decimation, gcd(L, decimation) = 1, n_taps <= 16384 L.  Wherever "max_input / decimation" sizes
 * something below, read max_input * L / decimation.
 * Uniform raster: raster = K != 0 puts every channel on a multiple of input_rate / K -- channel b at bins[b] * input_rate / K,
 * bins taken mod K, any subset in any order, duplicates allowed -- and computes all of them as ONE polyphase fold of the
 * prototype followed by a K-point DFT on the matrix cores: the matrix work per output is 8 B K instead of 8 B n_taps.
 * increments is then ignored and may be NULL; bins must not be.  Phases are the integers (c m) mod K mapped through
 * Phi(q) = ((q << 32) + K / 2) / K, so the arithmetic (channelizer_core.hpp, "Uniform raster") is not bit for bit that of
 * the same channels given as increments; both are the same converter bank to within rounding.  The fixed-offset form stays
 * the general case, for channels off any raster.  Limits: 2 <= raster <= 16384, 1 <= n_taps <= 64 raster and <= 2^20 (in
 * place of 16384).  raster together with interpolation > 1 is DH_EINVAL: a raster has no rational rates yet.
 * ---------------------------------------------------------------------- */
enum { DH_CZ_CS16 = 1, DH_CZ_CF32 = 2 };
enum { DH_CZ_IQ_F32 = 1, DH_CZ_FM = 2 };
typedef struct dh_channelizer dh_channelizer;
typedef struct {
    uint32_t struct_size;          /* sizeof(dh_channelizer_config) */
    int32_t  device;
    uint32_t n_channels;
    uint32_t decimation;
    const float* taps;             /* host, copied at create */
    uint32_t n_taps;
    const uint32_t* increments;    /* host [n_channels], copied at create */
    int32_t  input_format;         /* DH_CZ_* */
    int32_t  output_mode;          /* DH_CZ_* */
    int32_t  dcblock;
    uint32_t max_input;            /* complex samples per push */
    void*    stream;               /* hipStream_t; NULL = default stream */
    uint32_t interpolation;        /* L of a rational rate; 0 and 1 (and a struct_size that ends before this field): L = 1 */
    uint32_t raster;               /* K of a uniform raster; 0 (and every struct_size below the whole struct): fixed offsets */
    const int32_t* bins;           /* raster != 0: host [n_channels], copied at create */
} dh_channelizer_config;
/* raster took the place of the tail padding that the struct had when it ended with interpolation: that struct's size covers
 * it, and its callers never wrote it.  raster is therefore read only when struct_size covers bins as well, i.e. is at least
 * sizeof(dh_channelizer_config); every smaller struct_size means fixed offsets whatever bytes follow interpolation. */

int  dh_channelizer_create(const dh_channelizer_config* cfg, dh_channelizer** out);
void dh_channelizer_destroy(dh_channelizer* c);
/* back to sample 0: zero input history and channel states (taps and increments stay) */
int  dh_channelizer_reset(dh_channelizer* c);
/* channel `channel` takes `increment` from the next push on; its FM / DC-blocker state restarts, the input history stays.
 * On a uniform raster `increment` is the channel's new bin, read as a two's-complement int32 (pass (uint32_t) bin). */
int  dh_channelizer_retune(dh_channelizer* c, uint32_t channel, uint32_t increment);
/* n_in (<= max_input, any length, 0 included) complex samples; *n_out = outputs completed by this push, known without a
 * sync.  d_out [n_channels][out_stride] (out_stride in output samples: complex pairs for IQ_F32, floats for FM, >= *n_out)
 * receives them.  Asynchronous on the channelizer's stream.  With block power enabled every push writes d_counts, so even
 * a push of n_in = 0 launches one small kernel. */
int  dh_channelizer_push(dh_channelizer* c, const void* d_in, size_t n_in, float* d_out, size_t out_stride, size_t* n_out);
/* the same from host memory (staged through a device buffer; returns once the input has been read) */
int  dh_channelizer_push_host(dh_channelizer* c, const void* h_in, size_t n_in, float* d_out, size_t out_stride, size_t* n_out);
/* Block power and squelch gate (optional; bit for bit specified in channelizer_core.hpp).  Block m of a channel covers the
 * outputs [m block, (m + 1) block) counted from create / reset, whatever the push lengths; power = the in-order sum of |z|^2
 * over the block times (float) (1 / block), z the rotated output (the same in both output modes).  The gate of a channel opens
 * with a block >= open_level and closes after more than hang_blocks consecutive blocks < close_level.  After every push
 * d_counts[b] = n_out if the gate of channel b was open when the push began or in any block the push completed, else 0:
 * the d_counts argument of dh_engine_push_ragged.  Whole pushes pass or do not; a transmission that begins inside the last,
 * unfinished block of a push loses at most block - 1 outputs.  The three arrays are the caller's device memory, like push's
 * d_out, and are written by every push from the enable on.  Legal only while no sample has been pushed since create / reset.
 * A retune zeroes the channel's sum and gate; a reset zeroes all of them and keeps this configuration.
 * DH_EINVAL: null pointers, block 0 or > 65536, stride too small, levels not finite or negative, close_level > open_level,
 * hang_blocks > 65535, samples already pushed. */
typedef struct {
    uint32_t struct_size;          /* sizeof(dh_channelizer_power_config) */
    uint32_t block;                /* L: outputs per block, 1 .. 65536 (480 = 10 ms at 48 kS/s) */
    float    open_level, close_level;      /* |z|^2 units: a full-scale CS16 tone through unity-gain taps is 1.0 */
    uint32_t hang_blocks;
    float*    d_power;             /* [n_channels][stride] */
    uint8_t*  d_gate;              /* [n_channels][stride] */
    uint32_t* d_counts;            /* [n_channels] */
    size_t   stride;               /* >= (max_input * L / decimation + 1) / block + 1 */
    float*    d_ferr;              /* [n_channels][stride] frequency-error blocks (below); NULL: off */
} dh_channelizer_power_config;
/* Frequency-error blocks (optional; bit for bit specified in channelizer_core.hpp): how far off its channel a carrier sits.
 * d_ferr was appended to the struct.  struct_size = DH_CHANNELIZER_POWER_CONFIG_V1_SIZE (a caller built against the older
 * header): the field is not read, whatever bytes follow, and the feature is off.  struct_size = sizeof(the struct): d_ferr =
 * NULL is off -- nothing more is allocated, launched or written than before -- and otherwise every push that completes
 * outputs launches one more kernel, and column i of d_ferr is block *first_block + i of dh_channelizer_power_last, as for
 * d_power.  Any other struct_size is DH_EINVAL.
 * Value: with w[j] = z[j] conj(z[j-1]) (the discriminator's product, z[-1] = 0 after create / reset), Ar and Ai the in-order
 * sums of re w and im w over the block from +0, ferr = atan2(Ai, Ar) / pi with dh_frontend_s16's polynomial; (0, 0) -> 0.
 * The unit is half the output rate: Hz = ferr * output_rate / 2.  It is the |z|^2-weighted mean frequency of the block:
 * strong samples dominate, an empty channel gives noise around 0.  The same value in both output modes and all three kinds
 * of bank.  A push that ends inside a block carries (Ar, Ai) and its last z; a retune zeroes the channel's sums and carried z
 * (the block in progress keeps its index and holds the outputs after the retune); a reset zeroes all of them.  Power, gate,
 * counts and the rows are byte for byte what they are without d_ferr. */
#define DH_CHANNELIZER_POWER_CONFIG_V1_SIZE offsetof(dh_channelizer_power_config, d_ferr)
int  dh_channelizer_power_enable(dh_channelizer* c, const dh_channelizer_power_config* cfg);
/* new levels and hang from the next push on; the gates' state is kept.  DH_EINVAL before the enable */
int  dh_channelizer_set_squelch(dh_channelizer* c, float open_level, float close_level, uint32_t hang_blocks);
/* blocks completed by the last push: the index of the first one and how many (host arithmetic, no sync).  Column i of
 * d_power / d_gate holds block *first_block + i. */
int  dh_channelizer_power_last(dh_channelizer* c, uint64_t* first_block, size_t* n_blocks);
/* the NCO phasor P(phi) of the specification for n host phase words -> h_out [n][2] (host arithmetic, for tests) */
int  dh_channelizer_phasor(const uint32_t* h_phi, float* h_out, size_t n);

/* ------------------------------------------------------------------------
 * Pre-roll: a per-channel history ring on the device.  Own specification; the reference has no counterpart (there a
 * decoder is started by hand, before the transmission).  A band monitor learns which protocol a channel carries some
 * time AFTER its squelch opened (Protocol scan: D-Star needs three sync words 2 016 bits apart); the ring keeps every
 * channel's last `depth` samples so that the decoder is then fed from where the squelch opened, call set-up included.
 *
 * Stream.  Every channel's stream is counted from create or reset; `total` is the number of samples appended so far,
 * the same for all channels and therefore a host scalar (dh_preroll_total: host arithmetic, no sync).
 *
 * Append.  dh_preroll_append adds the first n samples of every row d_rows[b][0..n) ([n_channels][stride] float32, what
 * dh_channelizer_push wrote), gated or not.  Afterwards the ring holds samples [max(0, total - depth), total) of each
 * channel bit for bit (NaN payloads, -0 and subnormals included).  n > depth keeps the last depth samples; n = 0 changes
 * nothing and launches nothing; stride >= n, rows need no particular alignment.  Asynchronous on the stream.
 *
 * open_at.  d_counts is the channelizer's d_counts: non-zero = the channel's gate was open in this push; NULL = every
 * channel is open.  With base = total before the append: an open channel whose open_at is DH_PREROLL_NONE gets
 * open_at = base; a closed channel gets open_at = DH_PREROLL_NONE; otherwise open_at stays.  So open_at[b] is the stream
 * index of the first sample of the first push of the current run of open pushes.  dh_preroll_open_at copies the
 * n_channels values to the host and synchronises.
 *
 * Gather.  Asynchronous on the stream.  h_from is a host array of n_channels entries, uploaded by the call.  With
 * oldest = total > depth ? total - depth : 0, a wanted channel b has
 *     start_b = max(h_from[b], oldest),   first = start_b + skip,
 *     count_b = first < total ? min(max_n, total - first) : 0,
 *     d_out[b][i] = x_b[first + i] for i < count_b,   d_counts[b] = count_b.
 * A channel with h_from[b] == DH_PREROLL_NONE gets d_counts[b] = 0 and its output row is not touched.  h_start (optional,
 * host, n_channels entries) receives start_b, or DH_PREROLL_NONE for unwanted channels: host arithmetic.  A long history
 * is replayed in chunks by stepping skip by max_n, so engines keep their ordinary max_samples; the output row index is
 * the channel index, and (d_out, out_stride, d_counts, max_n) are exactly the arguments of dh_engine_push_ragged.
 *
 * Memory: the ring takes n_channels x depth x 4 bytes -- 192 channels x 2 s at 48 kS/s is 74 MB.
 * DH_EINVAL: null handles or pointers (where n or max_n is not 0), struct_size too small, n_channels outside 1 .. 65536,
 * depth outside 1 .. 2^24, stride < n, out_stride < max_n.
 * ---------------------------------------------------------------------- */
#define DH_PREROLL_NONE UINT64_MAX          /* open_at: gate closed;  from: channel not wanted */
typedef struct dh_preroll dh_preroll;
typedef struct {
    uint32_t struct_size;          /* sizeof(dh_preroll_config) */
    int32_t  device;
    uint32_t n_channels;
    uint32_t depth;                /* samples kept per channel */
    void*    stream;               /* hipStream_t; NULL = default stream */
} dh_preroll_config;
int  dh_preroll_create(const dh_preroll_config* cfg, dh_preroll** out);
void dh_preroll_destroy(dh_preroll* p);
/* back to sample 0, every open_at = DH_PREROLL_NONE */
int  dh_preroll_reset(dh_preroll* p);
int  dh_preroll_append(dh_preroll* p, const float* d_rows, size_t stride, size_t n, const uint32_t* d_counts);
int  dh_preroll_total(dh_preroll* p, uint64_t* total);
int  dh_preroll_open_at(dh_preroll* p, uint64_t* h_open_at);
int  dh_preroll_gather(dh_preroll* p, const uint64_t* h_from, uint64_t skip, size_t max_n,
                       float* d_out, size_t out_stride, uint32_t* d_counts, uint64_t* h_start);
/* dh_preroll_gather with `from` on the device already (n_channels entries, read when the launch runs): no upload, and no
 * h_start -- start_b is max(d_from[b], oldest) as above.  Same kernel, same counts. */
int  dh_preroll_gather_device(dh_preroll* p, const uint64_t* d_from, uint64_t skip, size_t max_n,
                              float* d_out, size_t out_stride, uint32_t* d_counts);

/* ------------------------------------------------------------------------
 * Band monitor: scanner, ring and decoders behind one handle.  Own specification; the reference has no counterpart.
 * A dh_monitor owns, all on the configuration's stream: one protocol-scan engine per front end that its protocols need
 * (wide10: DMR, YSF; narrow20: NXDN; fsk10: D-Star; fsk40i: POCSAG -- the engine arguments of api.SCAN_FRONTS), one
 * pre-roll ring of `depth`, one decoding engine per protocol in `protos` behind that protocol's front end, and one
 * [n_channels][max_samples] staging array.  It does not own the channelizer: d_rows, stride, n and d_counts of
 * dh_monitor_push are what dh_channelizer_push and its power stage wrote.  d_counts is read as a flag per channel
 * (non-zero: the gate is open and the channel brings all n samples); NULL: every channel is open.
 *
 * State, per channel, on the device: assigned (uint8: 0 or a DH_PROTO_*), closed_run (uint32, saturating: rounds in a
 * row with the gate closed), start (uint64: the stream index at which the decoder's input began; DH_PREROLL_NONE while
 * unassigned), opened (uint64: open_at of the channel's last open round; DH_PREROLL_NONE after create and reset).
 * dh_monitor_state copies assigned and start to the host (either pointer may be NULL) and synchronises.
 *
 * One round, dh_monitor_push with 0 < n <= max_samples (n = 0: DH_OK, nothing happens):
 *   1. The ring appends the rows (Pre-roll); open = (open_at[b] != DH_PREROLL_NONE).
 *   2. Step A, one kernel, per channel: closed_run = open ? 0 : closed_run + 1.  A closed channel that is unassigned with
 *      closed_run == 1 gets scan_reset[b] = 1 (every other channel 0); a closed channel that is assigned with
 *      closed_run >= release becomes unassigned, start = DH_PREROLL_NONE.  Then scan_counts[b] = (open && assigned == 0)
 *      ? n : 0, and for every configured protocol p live_counts[p][b] = (open && assigned == p) ? n : 0.  An open channel
 *      gets opened[b] = open_at[b].
 *   C. Naming on close -- only with some close_hits[f] != 0, and only where step A set any scan_reset: one kernel, per
 *      CLOSING channel (scan_reset[b] = 1: closed, unassigned, closed_run == 1), before step 3 forgets what it judges.
 *      Per family f in the order DMR, YSF, NXDN, D-Star, POCSAG: H_f = the sum of `hits` and D_f = the smallest
 *      best_dist over the family's patterns, read as step 5 reads `periodic` (a short row or a front end that is not
 *      configured: zeros and 255).  f is eligible iff close_hits[f] != 0 && H_f >= close_hits[f] && D_f <= close_dist[f];
 *      the eligible family with the largest H_f wins, the first in that order where two are level.  If its protocol p
 *      is configured the channel is assigned: assigned = p, start = max(opened - lead, total - depth, 0) as in step 5,
 *      new_flags[p][b] = 1, from[p][b] = start; every other new_flags entry is 0, every other from entry
 *      DH_PREROLL_NONE.  Otherwise the channel stays unassigned (the next-best family is not considered).  closed_run
 *      and scan_reset stay as step A left them.
 *   3. Where any scan_reset is set, the scan engines get dh_engine_reset_channels(scan_reset).
 *   4. Where any scan_counts is non-zero, every scan engine gets a ragged push of the rows with scan_counts.
 *   5. Step B (only then), one kernel, per channel with scan_counts != 0: the `periodic` counts of the nine patterns are
 *      summed per family -- DMR (patterns 0-3), YSF (4), NXDN (5), D-Star (6, 7), POCSAG (8) -- each pattern read from the
 *      statistics row of the scan engine of its own front end (a row of fewer than 144 bytes, or a front end that is not
 *      configured, reads as zeros).  The family with the largest sum wins, the first in that order where sums are equal.
 *      If its sum is >= confirm and its protocol p is configured, the channel is assigned: assigned = p, start =
 *      max(open_at - lead, total - depth, 0) with both differences saturating at 0 (total: after this round's append),
 *      new_flags[p][b] = 1, from[p][b] = start, scan_reset[b] = 1.  Every other new_flags entry is 0, every other from
 *      entry DH_PREROLL_NONE, every other scan_reset 0 -- except that the new_flags and from entries of a channel step C
 *      named in this round are left alone.  If the winner's protocol is not configured the channel stays unassigned; the
 *      next-best family is not considered.
 *   6. Where step 5 assigned a channel, the scan engines get dh_engine_reset_channels(scan_reset); then -- also in a round
 *      in which nothing was scanned -- per protocol p with channels new from step C or step 5:
 *      dh_engine_reset_channels(new_flags[p]) of its engine, and for skip = 0, max_samples, ... while
 *      skip < total - (the smallest start among p's new channels): dh_preroll_gather_device(from[p], skip, max_samples)
 *      into the staging array and a ragged push of it.  The ring already holds this round's samples: a channel named in
 *      this round gets no live push in it.  For a channel named on close those are the closing round's own samples,
 *      which flush the decoder's look-ahead; being closed it gets no live push, is released by step A's ordinary rule
 *      when closed_run >= release, and continues live in the same engine if its gate opens before that.
 *   7. Per protocol p with any live_counts[p] non-zero: one ragged push of the caller's rows with live_counts[p].
 *
 * The sink.  After EVERY engine push of steps 6 and 7, before the next push overwrites that engine's outputs, `sink`
 * (may be NULL) is called on the calling thread with: proto; replay = 1 (step 6) or 0 (step 7); the engine, whose
 * outputs the callee reads with the engine's own calls (dh_engine_frames, dh_engine_read_events, ...); d_counts
 * [n_channels], device: channel b took part in this push when d_counts[b] != 0; d_start [n_channels], device; skip;
 * live_first = total - n.  The first input sample of channel b's block has stream index d_start[b] + skip in a replay
 * and live_first in a live push.  d_counts and d_start are the monitor's own arrays: valid during the call only.
 *
 * What the host reads.  Steps A and B each add up one fixed-size summary block on the device -- how many channels are
 * scanned, how many have scan_reset, how many are live per protocol; how many are new per protocol and the smallest
 * start among them (steps B and C add to the same fields) -- and dh_monitor_push reads that block at most twice per round,
 * after step A and after step B, or after step C in a round where step C ran and step B did not: one small copy each,
 * which synchronises.  Without naming on close no round launches or reads anything more than before.  It reads nothing whose size grows with n_channels, uploads nothing per channel,
 * and issues a fixed number of launches per engine however many channels are reset.
 *
 * What is never decoded.  Without naming on close: a transmission that ends before the scanner has confirmed it (three
 * sync words one frame period apart, seen while the gate is open) -- a single POCSAG batch, a D-Star transmission shorter
 * than three sync periods.  With it: a transmission whose evidence stays below its family's thresholds; a family with
 * close_hits = 0 is never named on close.
 *
 * DH_EINVAL: null handle or configuration, struct_size none of the accepted sizes, n_channels outside 1 .. 65536, max_samples = 0, depth
 * outside 1 .. 2^24, protos == 0 or with bits other than DH_PROTO_DMR .. DH_PROTO_DSTAR, n > max_samples, stride < n, null
 * rows with n != 0.  dh_monitor_engine / dh_monitor_scan_engine return the owned handles (NULL: not configured, or out of
 * range) for reading outputs and statistics; they stay the monitor's and go with dh_monitor_destroy.
 * ---------------------------------------------------------------------- */
typedef struct dh_monitor dh_monitor;
typedef struct {
    uint32_t struct_size;          /* sizeof(dh_monitor_config) */
    int32_t  device;
    uint32_t n_channels, max_samples, depth, lead, confirm, release;
    uint32_t protos;               /* bit DH_PROTO_x set: that protocol is decoded */
    void*    stream;               /* hipStream_t; NULL = default stream */
    uint32_t dmr_both_slots;       /* non-zero: the DMR engine is created with DH_FLAG_DMR_BOTH_SLOTS, its blocks carry 28-byte slot-tagged
                                      records; 0 (and a struct_size that ends before this field): the reference's one active slot */
    uint32_t reserved;             /* the struct's tail padding before naming on close was added; not read */
    uint32_t close_hits[5];        /* naming on close, by family: DMR, YSF, NXDN, D-Star, POCSAG.  0: never named on close; all 0 */
    uint32_t close_dist[5];        /* (and a struct_size that ends before these fields): the mode is off.  The largest best distance accepted */
} dh_monitor_config;
/* sizeof(dh_monitor_config) before dmr_both_slots was added, and before close_hits and close_dist were: both still accepted
 * as struct_size (one of these sizes exactly, or the whole struct); the fields a shorter struct lacks are zeros */
#define DH_MONITOR_CONFIG_V1_SIZE offsetof(dh_monitor_config, dmr_both_slots)
#define DH_MONITOR_CONFIG_V2_SIZE offsetof(dh_monitor_config, close_hits)
typedef struct {
    int32_t proto, replay;
    dh_engine* engine;
    const uint32_t* d_counts;      /* [B] samples each channel brought in this push */
    const uint64_t* d_start;       /* [B] */
    uint64_t skip, live_first;
} dh_monitor_push_info;
typedef void (*dh_monitor_sink)(void* user, const dh_monitor_push_info* info);
int  dh_monitor_create(const dh_monitor_config* cfg, dh_monitor** out);
void dh_monitor_destroy(dh_monitor* m);
/* ring, every engine and the state back to where create left them */
int  dh_monitor_reset(dh_monitor* m);
int  dh_monitor_push(dh_monitor* m, const float* d_rows, size_t stride, size_t n,
                     const uint32_t* d_counts, dh_monitor_sink sink, void* user);
int  dh_monitor_state(dh_monitor* m, uint8_t* h_assigned, uint64_t* h_start);       /* synchronises */
int  dh_monitor_total(dh_monitor* m, uint64_t* total);
dh_engine* dh_monitor_engine(dh_monitor* m, int proto);
dh_engine* dh_monitor_scan_engine(dh_monitor* m, int front /* 0..3: wide10, narrow20, fsk10, fsk40i */);

/* ------------------------------------------------------------------------
 * Packed read-out: what the pushes of a round produced, in one device block.  Own specification; the reference has no
 * counterpart.  An engine's outputs are dense [B][out_cap] and [B][ev_cap] arrays that the next push overwrites; a
 * dh_outpack compacts, on the device, the rows that hold something, and appends across the pushes and engines of a round.
 * A whole round then costs one synchronisation and copies sized by what was decoded, not by B.
 *
 * Areas.  Three device areas of fixed capacity plus the header: entries[max_entries], events[max_events],
 * frames[max_frame_bytes]; max_frame_bytes is a multiple of 16 and at most 2^36 - 16.
 *
 * Candidates of an append.  The channels b of the engine, in ascending order, for which both hold:
 * d_mask == NULL || d_mask[b] != 0, and fc[b] != 0 || ec[b] != 0.  fc is the push's frame-byte count and ec its event
 * count (0 for an engine created with DH_FLAG_NO_EVENTS), both clamped to the row capacities.
 *
 * Append.  With the running totals before a candidate (E, V, F) = (n_entries, n_events, frame_bytes) and
 * pad16(n) = n rounded up to a multiple of 16, a candidate is kept iff all four hold: dropped == 0, E + 1 <= max_entries,
 * V + ec <= max_events, F + pad16(fc) <= max_frame_bytes.  A kept candidate writes
 *     entry E = { b, user, (d_tag ? d_tag[b] : 0) + tag_add mod 2^64, fc, ec, F / 16, V },
 *     frames[F, F + fc) = the row's bytes, frames[F + fc, F + pad16(fc)) = 0,
 *     events[V, V + ec) = the row's records bit for bit,
 * and the totals advance by (1, ec, pad16(fc)).  The first candidate that does not fit is dropped, and so is every later
 * candidate, in this append and in later ones until dh_outpack_clear; `dropped` counts them.  The kept set is therefore
 * always a prefix in append order, then channel order.  `appends` += 1 per call.  No byte beyond the totals is written.
 *
 * Streams.  The append is enqueued on the engine's stream, behind the push whose outputs it reads (an engine with
 * DH_FLAG_OVERLAP_PUSHES is joined first, as for any other kind of work): it is asynchronous, and the totals it starts
 * from are read on the device, so appends chain in stream order without the host knowing any total.  d_mask and d_tag
 * ([n_channels] each, device) are read when the launch runs.  DH_EINVAL if the engine's device or stream differ from the
 * pack's.  dh_outpack_clear is asynchronous on the same stream: header = 0, the areas are not touched.
 *
 * Read.  dh_outpack_read synchronises once and copies the header; then it copies exactly n_entries entries, n_events
 * events and frame_bytes bytes into the host arrays, which hold the create capacities (a NULL array is skipped).  It
 * returns DH_ECAPACITY when dropped != 0; the kept data is still delivered.  dh_outpack_device hands out the device
 * addresses of the header and the three areas (any pointer may be NULL) for consumers that stay on the device.
 *
 * DH_EINVAL: null handles or configuration, struct_size too small, max_entries == 0, max_frame_bytes not a multiple of
 * 16 or above 2^36 - 16, an engine with proto == DH_PROTO_NONE.
 *
 * Monitor.  dh_monitor_push_packed is dh_monitor_push whose internal sink, after every engine push of steps 6 and 7,
 * calls dh_outpack_append(pack, engine, d_counts, replay ? d_start : NULL, replay ? skip : live_first,
 * proto | replay << 8): an entry's tag is the stream index of its block's first input sample.  It does not clear the
 * pack and does not read it; a round through it issues no output read-back at all.  DH_EINVAL, before anything happens,
 * if the pack is NULL or not on the monitor's device and stream.
 * ---------------------------------------------------------------------- */
typedef struct dh_outpack dh_outpack;
typedef struct {
    uint32_t struct_size;          /* sizeof(dh_outpack_config) */
    int32_t  device;
    uint32_t max_entries, max_events;
    uint64_t max_frame_bytes;
    void*    stream;               /* hipStream_t; NULL = default stream */
} dh_outpack_config;
typedef struct {                   /* 32 bytes; the rest reserved, 0 */
    uint32_t n_entries, n_events;
    uint64_t frame_bytes;
    uint32_t dropped, appends;
    uint32_t reserved[2];
} dh_outpack_header;
typedef struct {                   /* 32 bytes */
    uint32_t channel, user;
    uint64_t tag;
    uint32_t n_frame_bytes, n_events, frame_offset16, event_index;
} dh_outpack_entry;
int  dh_outpack_create(const dh_outpack_config* cfg, dh_outpack** out);
void dh_outpack_destroy(dh_outpack* p);
int  dh_outpack_clear(dh_outpack* p);
int  dh_outpack_append(dh_outpack* p, dh_engine* e, const uint32_t* d_mask, const uint64_t* d_tag, uint64_t tag_add, uint32_t user);
int  dh_outpack_read(dh_outpack* p, dh_outpack_header* h_hdr, dh_outpack_entry* h_entries, dh_event* h_events, uint8_t* h_frames);
int  dh_outpack_device(dh_outpack* p, const dh_outpack_header** d_hdr, const dh_outpack_entry** d_entries,
                       const dh_event** d_events, const uint8_t** d_frames);
int  dh_monitor_push_packed(dh_monitor* m, const float* d_rows, size_t stride, size_t n, const uint32_t* d_counts, dh_outpack* pack);

/* ------------------------------------------------------------------------
 * Diagnostics: the RRC output scaling `(float)((double)sum / gain)` of
 * src/rrc_filter/rrc_filter.cpp:33 exactly as the FIR kernels evaluate it
 * (reciprocal multiply + exact-division fallback near float rounding ties).
 * d_out[i] must equal (float)((double)d_in[i] / gain) for every float.
 * ---------------------------------------------------------------------- */
int dh_debug_div_gain(const float* d_in, float* d_out, size_t n, int narrow, void* stream);
/* The slicer's `volume_sum / samplesPerSymbol` (src/gfsk_demodulator/gfsk_demodulator.cpp:83) exactly as the kernels
 * evaluate it (reciprocal multiply + exact FMA residual + correction; IEEE division for 0, tiny, huge and non-finite
 * operands).  d_out[i] must equal d_in[i] / (float) divisor for every float. */
int dh_debug_div_const(const float* d_in, float* d_out, size_t n, unsigned divisor, void* stream);
/* The matrix-core instruction behind the error-bounded wide-filter FIR (v_mfma_f32_16x16x32_f16), one tile per item:
 * d_d[t][16][16] = d_c[t][16][16] + d_a[t][16][32] x d_b[t][32][16], A and B as IEEE binary16 bit patterns.  The bound of
 * that FIR rests on a stated assumption about how the hardware adds the products (dsp_core.hpp, "(H1)"): the parity tests
 * check it through this entry. */
int dh_debug_mfma_f16(const uint16_t* d_a, const uint16_t* d_b, const float* d_c, float* d_d, size_t tiles, void* stream);
/* The split of a scaled sample into two halves as the same kernels do it: d_h1[i] = f16(x scale), d_h2[i] =
 * f16((x scale - h1) 2^11), both rounded to nearest even, subnormal halves kept. */
int dh_debug_f16_split(const float* d_in, uint16_t* d_h1, uint16_t* d_h2, size_t n, float scale, void* stream);
/* A plain streaming copy of n_bytes (a multiple of 16, both pointers 16-byte aligned): 16 bytes per lane, non-temporal
 * loads and stores, grid-stride over 2 048 workgroups.  Not part of the path -- bench.py times it on the lease it runs on
 * as the achievable HBM ceiling (read + write bytes over its duration) that the path's kernels are priced against beside
 * the 8 TB/s of the data sheet.  d_dst == NULL: the bytes are only read (eight loads in flight per lane, 8 192 workgroups) -- the read-only
 * streaming rate, which is what a kernel that mostly reads (the chain kernels) can be priced against. */
int dh_debug_copy(const void* d_src, void* d_dst, size_t n_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The seam probe: ONE primitive of the kernels' device / CPU layer (dh_portable.hpp, wave_ops.hpp) or one hand-scheduled piece
 * (dh_agc_scan) run alone, one wavefront per case, on operands the caller chooses.  Not part of any path: the parity tests hold
 * the device form and its CPU restatement to the primitive's written statement through it (tests/test_seam_primitives.py).
 *
 * Case c reads d_in + c * in_words(op) and writes d_out + c * out_words(op) (32-bit words; dh_debug_seam_probe_words).  Input:
 * four header words (the case's wave-uniform operands, h0 .. h3), then the lanes' words, word i of lane l at [4 + 64 i + l].
 * Output: word i of lane l at [64 i + l], unless stated.  Floats travel as bit patterns.  L = lane words in -> lane words out.
 *
 *   VMIN, VMAX                 L 2 -> 1    dh_vmin / dh_vmax(w0, w1)
 *   MIN3_ABS, MAX3_ABS         L 3 -> 1    dh_min3_abs / dh_max3_abs(w0, w1, w2)
 *   MAX_ABS_GROUPS5            L 20 -> 1   dh_max_abs_groups<5>, group g = words 4 g .. 4 g + 3
 *   MUL_UNIFORM                L 1 -> 1    dh_mul_uniform(h0, w0)
 *   SQRT_UPPER                 L 1 -> 1    dh_sqrt_upper(w0)
 *   DIV_CONST2                 L 2 -> 2    dh_div_const2((w0, w1), d = h0, r = h1)
 *   F2_MAC, F2_MAC_FAST        L 5 -> 2    dh_f2_mac<false / true>(c = w0, w = (w1, w2), acc = (w3, w4))
 *   F2_MAC_PAIR_LO / _HI, F2_MAC_PAIR_FAST_LO / _HI
 *                              L 4 -> 2    dh_f2_mac_pair<FAST, HALF>(cc = (h0, h1), w = (w0, w1), acc = (w2, w3))
 *   F2_FMA                     L 6 -> 2    dh_f2_fma((w0, w1), (w2, w3), (w4, w5))
 *   F2_SCALE                   L 3 -> 2    dh_f2_scale((w0, w1), w2)
 *   F16_SPLIT4_PLAIN           L 4 -> 4    dh_f16_split4_plain((w0 .. w3), scale = h0): h1 as two words (halves 0|1, 2|3), then h2
 *   WAVE_MAX, WAVE_MAX_NAN, WAVE_MIN, ROW0_MIN
 *                              L 1, ONE output word: the reduction of the lanes' w0
 *   ROW_SUM5_PAIR              L 2 -> 2    dh_row_sum5_pair(s = w0, q = w1)
 *   AGC_SCAN, AGC_SCAN_PAIRS   L 10 -> 8   dh_agc_scan<false / true>, h0 = k0, h1 = k1 (k0 < k1 <= 100), h2 = from_win (PAIRS and
 *                                          k0 = 0 only); w0, w1 = vol_old[l], [64 + l]; w2, w3 = vol_new[l], [64 + l]; w4 .. w9 = the
 *                                          lane's DhWinPair (vol0, vol1, sum0, sum1, old0, old1).  Out: S.mn[l], S.mn[64 + l], S.mx[l],
 *                                          S.mx[64 + l] (0xA5A5A5A5 where the scan wrote nothing), then the lane's DhAgcPair
 *   The LDS movers work on a block of 5 632 words that holds the bits 0x3F000000 + (h0 & 0xFFFF) + i in word i; w0 = the lane's
 *   base in words (at most 1 720).  A lane's j-th stored value is 0x4B000000 + 64 l + j.
 *   LDS_RUN20, LDS_RUN40       L 1 -> 20 / 40     dh_lds_run<20 / 40>
 *   LDS_RUN20_WITH_PAIR        L 2 -> 22          dh_lds_run20_with_pair, the pair at word w1 & ~1: v[0 .. 19], p0, p1
 *   LDS_PAIRS3_NOW             L 3 -> 6           dh_lds_pairs3_now at w0, w1, w2: a.x, a.y, b.x, b.y, c.x, c.y
 *   LDS_READS                  L 2 -> 6           ds_read2_b32 at w0; ds_read_b64 at w1 & ~1; two ds_read_b32 at w0, w0 + 1
 *   LDS_STORE4_AT (_PLAIN)     L 1, out = the block afterwards: dh_lds_store4_at<0, G, 2 G, 3 G, 4 G>, values j = 0 .. 19,
 *                                                 G = 272 (the padded window) / 256 (_PLAIN)
 *   LDS_STORE_ROW10_0 / _1000 / _2000 / _3000     L 1, out = the block: dh_lds_store_row10<K>, values j = 0 .. 9
 *   LDS_STORE_PAIR             L 1, out = the block: dh_lds_store_pair, values 0, 1
 *   LDS_STORE_ROWS10_PAIR      L 1, out = the block: dh_lds_store_rows10_pair, a = values 0 .. 9, b = values 10 .. 19
 *   LV_READ                    L 1 -> 1    word k of the output = DH_LV_READ(w0, k)
 *   LV_DOWN                    L 1 -> 4    DH_LV_DOWN(w0, lane, d) for d = 0, 1, 5, 63
 *   LS_WRITE_READ              L 4 -> 5    struct (a = w1, b = w2); for k = 0 .. 63: m0 = 0x00A50000 + k, DH_LS_WRITE(a, k, w3 of lane k),
 *                                          m0 read back, then DH_LV_READ(w0, 63 - k) and DH_LS_READ(a, k).  Out: a afterwards; the
 *                                          DH_LS_READs (word k); the DH_LV_READs (word k); b; what m0 held behind each write (word k)
 *   LS_GATHER                  L 3 -> 1    DH_LS_GATHER(a = w1, lane w2 & 63)
 *   LANES_BELOW                L 0 -> 1    DH_LANES_BELOW(h0 | h1 << 32, lane)
 *   STATE                      L 2 -> 3    DhState: load(w0); out word 0 of lane k = get(k); eight set(w1 of lane 2 i & 63, w1 of lane
 *                                          2 i + 1); out word 1 = store(); out word 2 = store_words(first = h0 & 63, n = h1): n words
 *   BITS                       L 2 -> 5    x = w0 | w1 << 32: dh_brev32(w0), dh_ffs64(x), dh_top64(x) (~0 for x = 0), dh_popc32(w0), dh_popc64(x)
 *
 * DH_EINVAL for an op that does not exist; DH_OK for cases == 0.
 * ---------------------------------------------------------------------- */
enum dh_probe_op {
    DH_PROBE_VMIN = 0, DH_PROBE_VMAX, DH_PROBE_MIN3_ABS, DH_PROBE_MAX3_ABS, DH_PROBE_MAX_ABS_GROUPS5, DH_PROBE_MUL_UNIFORM, DH_PROBE_SQRT_UPPER,
    DH_PROBE_DIV_CONST2, DH_PROBE_F2_MAC, DH_PROBE_F2_MAC_FAST, DH_PROBE_F2_MAC_PAIR_LO, DH_PROBE_F2_MAC_PAIR_HI, DH_PROBE_F2_MAC_PAIR_FAST_LO,
    DH_PROBE_F2_MAC_PAIR_FAST_HI, DH_PROBE_F2_FMA, DH_PROBE_F2_SCALE, DH_PROBE_F16_SPLIT4_PLAIN,
    DH_PROBE_WAVE_MAX, DH_PROBE_WAVE_MAX_NAN, DH_PROBE_WAVE_MIN, DH_PROBE_ROW0_MIN, DH_PROBE_ROW_SUM5_PAIR,
    DH_PROBE_AGC_SCAN, DH_PROBE_AGC_SCAN_PAIRS,
    DH_PROBE_LDS_RUN20, DH_PROBE_LDS_RUN40, DH_PROBE_LDS_RUN20_WITH_PAIR, DH_PROBE_LDS_PAIRS3_NOW, DH_PROBE_LDS_READS,
    DH_PROBE_LDS_STORE4_AT, DH_PROBE_LDS_STORE4_AT_PLAIN, DH_PROBE_LDS_STORE_ROW10_0, DH_PROBE_LDS_STORE_ROW10_1000, DH_PROBE_LDS_STORE_ROW10_2000,
    DH_PROBE_LDS_STORE_ROW10_3000, DH_PROBE_LDS_STORE_PAIR, DH_PROBE_LDS_STORE_ROWS10_PAIR,
    DH_PROBE_LV_READ, DH_PROBE_LV_DOWN, DH_PROBE_LS_WRITE_READ, DH_PROBE_LS_GATHER, DH_PROBE_LANES_BELOW, DH_PROBE_STATE, DH_PROBE_BITS,
    DH_PROBE_OP_COUNT
};
int dh_debug_seam_probe(int op, const uint32_t* d_in, uint32_t* d_out, size_t cases, void* stream);
/* words per case of an op (host only; either pointer may be NULL) */
int dh_debug_seam_probe_words(int op, size_t* in_words, size_t* out_words);

#ifdef __cplusplus
}
#endif
#endif
