// abi_impl.hpp -- the extern "C" surface of include/digiham_amd.h over dh::Engine<DH_BACKEND>.
// Included once by engine.hip (DH_BACKEND = HIP backend -> libdigiham_amd.so) and once by the
// CPU test harness (DH_BACKEND = lane-loop backend -> tests/host_harness/libdh_hostemu.so, never
// shipped and never loaded by the digiham_amd package).
//
// Before inclusion the includer defines DH_BACKEND (the duck-typed interface listed in engine_impl.hpp; which instantiation
// a launch_* runs is not the backend's to decide: launch_plan.hpp) and these free functions of its own:
//   int  dh_be_device_count();
//   const char* dh_be_last_error();
//   int  dh_be_alloc(int device, size_t bytes, void** out); int dh_be_free(void*);
//   int  dh_be_copy(void* dst, const void* src, size_t bytes, int to_host);
//   int  dh_be_frontend(const int16_t* in, size_t in_stride, float* out, size_t out_stride, float* state, size_t B, size_t n, int mode, int dcblock, void* stream);
//   int  dh_be_mfma_f16(const uint16_t* a, const uint16_t* b, const float* c, float* d, size_t tiles, void* stream);
//   int  dh_be_copy_kernel(const void* src, void* dst, size_t n_bytes, void* stream);
//   dh_be_cz_gemm / dh_be_cz_gemm_rat / dh_be_cz_fold / dh_be_cz_gemm_raster               the channelizer's matrix-core stages
//   dh_be_monitor_open, dh_be_reset_channels                                               step A of the band monitor, the masked reset
// (kernels with barriers, LDS staging, matrix-core tiles or wave votes: engine.hip defines the gfx950 launches, the harness and
// the *_core.hpp files the CPU restatements) -- and includes helper_launches.hpp, which with the core headers states ONCE, for both builds:
//   int  dh_be_fec_block(int code, void* words, uint8_t* ok, size_t n, void* stream);
//   int  dh_be_bptc(const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n, void* stream);
//   int  dh_be_trellis(const uint8_t* in, size_t in_stride, int n_dibits, uint8_t* out, size_t out_stride, uint8_t* metric, size_t n, void* stream);
//   int  dh_be_crc16(const uint8_t* in, size_t stride, int count, uint16_t* out, size_t n, void* stream);
//   int  dh_be_whitening(const uint8_t* in, uint8_t* out, size_t stride, int n_bits, size_t n, void* stream);
//   int  dh_be_dvfilter(const int16_t* in, int16_t* out, float* state, size_t B, size_t stride, size_t n, void* stream);
//   int  dh_be_div_gain(const float* in, float* out, size_t n, int narrow, void* stream);
//   int  dh_be_div_const(const float* in, float* out, size_t n, unsigned divisor, void* stream);
//   int  dh_be_f16_split(const float* in, uint16_t* h1, uint16_t* h2, size_t n, float scale, void* stream);
//   int  dh_be_seam_probe(int op, const uint32_t* in, uint32_t* out, size_t cases, void* stream);                  (seam_probe_core.hpp)
// and the other launches of the four later handles, each listed at the head of its section below:
//   dh_be_cz_window / dh_be_cz_fm / dh_be_cz_power                                         the channelizer
//   dh_be_preroll_append / dh_be_preroll_gather                                            the pre-roll ring
//   dh_be_outpack_scan / dh_be_outpack_copy                                                the packed read-out
//   dh_be_monitor_assign / dh_be_monitor_close                                             steps B and C of the band monitor
//
// A handle kind is a struct over dh_place (device, stream) with a backend `be`, scope() and release(), an init() that
// allocates through its DeviceBuffers, and a dh_*_create that validates its configuration and calls dh_create; dh_destroy,
// DH_ENTER and shares_stream() are the same for all of them.
#pragma once

#include <cstddef>
#include <numeric>

#include "engine_impl.hpp"
#include "outpack_core.hpp"

static_assert(sizeof(dh_event) == 32, "dh_event layout");

// where a handle lives: what two handles that work on each other's buffers must have in common
struct dh_place {
    int device = 0; void* stream = nullptr;
    bool shares_stream(const dh_place& o) const { return device == o.device && stream == o.stream; }
};
// one [B][stride] output of an engine: what a getter hands out and what a row read needs
struct DhRows { const void* base; size_t stride; const uint32_t* counts; size_t elem; uint32_t most; };      // stride in elements
enum { DH_ROWS_SYMBOLS, DH_ROWS_FRAMES, DH_ROWS_EVENTS, DH_ROWS_FILTERED };
struct dh_engine : dh_place {
    dh::Engine<DH_BACKEND> impl;
    DH_BACKEND& be = impl.be;                           // the face every handle shows dh_create, dh_destroy and DH_ON_DEVICE
    auto scope() const { return be.scope(); }
    void release() { impl.destroy(); }
    DhRows rows(int which) const {
        const auto& L = impl.L;
        switch (which) {
        case DH_ROWS_SYMBOLS: return { impl.syms, L.sym_stride, impl.sym_count, 1, ~0u };
        case DH_ROWS_FRAMES: return { impl.frames, L.out_cap, impl.frame_count, 1, ~0u };
        case DH_ROWS_EVENTS: return { impl.events, L.ev_cap, impl.ev_count, sizeof(dh_event), ~0u };
        default: return { impl.filtered, L.max_samples, impl.last_counts, sizeof(float), impl.last_n };     // (the last push's samples)
        }
    }
};
// the four handles that own their backend and their buffers (a handle whose release() has more to let go of hides this one)
struct dh_state : dh_place {
    DH_BACKEND be;
    dh::DeviceBuffers<DH_BACKEND> bufs{ be };           // release(), and what the handle's clear() / retune() act on
    auto scope() const { return be.scope(); }
    void release() { bufs.free_all(); }
};
// every entry that touches the device runs on its handle's device whatever the calling thread's current device is
// (HipBackend::Scope)
#define DH_ON_DEVICE(h) auto dh_on_device_ = (h)->scope(); (void) dh_on_device_
// the opening of such an entry: a null handle (or a failed argument check, which may read the handle) is answered before
// anything touches the device
#define DH_ENTER_IF(h, ok) if (!(h) || !(ok)) return DH_EINVAL; DH_ON_DEVICE(h)
#define DH_ENTER(h) DH_ENTER_IF(h, true)

// dh_*_create behind its own validation: the handle, its backend, its place, then init(handle) on the handle's device; a
// failed init lets go of whatever it had allocated
template <class H, class Cfg, class Init>
static int dh_create(const Cfg& c, H** out, Init init) {
    *out = nullptr;
    H* h = new (std::nothrow) H;
    if (!h) return DH_ENOMEM;
    int rc = h->be.open(c.device, c.stream);
    if (rc == DH_OK) {
        DH_ON_DEVICE(h);
        h->device = c.device; h->stream = c.stream;
        rc = init(*h);
        if (rc != DH_OK) h->release();
    }
    if (rc != DH_OK) { delete h; return rc; }
    *out = h;
    return DH_OK;
}
template <class H>
static void dh_destroy(H* h) {
    if (!h) return;
    {
        DH_ON_DEVICE(h);
        h->be.sync();
        h->be.close();
        h->release();
    }
    delete h;
}

// the engine's four outputs behind dh_engine_symbols / frames / events / filtered and dh_engine_read_*
static int dh_rows_view(const dh_engine* e, int which, const void** d, size_t* stride, const uint32_t** cnt) {
    const void* base = e ? e->rows(which).base : nullptr;
    if (!base) return DH_EINVAL;
    if (d) *d = base;
    if (stride) *stride = e->rows(which).stride;
    if (cnt) *cnt = e->rows(which).counts;
    return DH_OK;
}
static int dh_rows_read(dh_engine* e, int which, uint32_t ch, void* h, size_t* n) {
    DH_ENTER_IF(e, e->rows(which).base);
    const DhRows r = e->rows(which);
    return e->impl.read_row(r.base, r.elem * r.stride, ch, r.counts, r.elem, h, n, r.most);
}

enum { DH_CODE_H74 = 0, DH_CODE_H139, DH_CODE_H1511, DH_CODE_H1611, DH_CODE_QR, DH_CODE_G208, DH_CODE_G2412, DH_CODE_BCH3121 };

extern "C" {

const char* dh_version(void) { return "digiham_amd 0.1.0 (gfx950)"; }
const char* dh_last_error(void) { return dh_be_last_error(); }
int dh_device_count(void) { return dh_be_device_count(); }

int dh_device_alloc(int device, size_t bytes, void** out) { return out ? dh_be_alloc(device, bytes, out) : DH_EINVAL; }
int dh_device_free(void* p) { return dh_be_free(p); }
int dh_copy_to_host(void* dst, const void* src, size_t bytes) { return (dst && src) || !bytes ? dh_be_copy(dst, src, bytes, 1) : DH_EINVAL; }
int dh_copy_to_device(void* dst, const void* src, size_t bytes) { return (dst && src) || !bytes ? dh_be_copy(dst, src, bytes, 0) : DH_EINVAL; }

int dh_hamming_7_4(uint8_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_H74, w, ok, n, s); }
int dh_hamming_13_9(uint16_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_H139, w, ok, n, s); }
int dh_hamming_15_11(uint16_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_H1511, w, ok, n, s); }
int dh_hamming_16_11(uint16_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_H1611, w, ok, n, s); }
int dh_quadratic_residue(uint16_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_QR, w, ok, n, s); }
int dh_golay_20_8(uint32_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_G208, w, ok, n, s); }
int dh_golay_24_12(uint32_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_G2412, w, ok, n, s); }
int dh_bch_31_21(uint32_t* w, uint8_t* ok, size_t n, void* s) { return dh_be_fec_block(DH_CODE_BCH3121, w, ok, n, s); }
int dh_bptc_196_96(const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n, void* s) {
    if ((!in || !out || !ok) && n) return DH_EINVAL;
    return dh_be_bptc(in, out, ok, n, s);
}
int dh_trellis(const uint8_t* in, size_t in_stride, int n_dibits, uint8_t* out, size_t out_stride, uint8_t* metric, size_t n, void* s) {
    if (n_dibits < 1 || n_dibits > 192 || in_stride < (size_t) (n_dibits + 3) / 4 || out_stride < (size_t) (n_dibits + 7) / 8) return DH_EINVAL;
    if ((!in || !out || !metric) && n) return DH_EINVAL;
    return dh_be_trellis(in, in_stride, n_dibits, out, out_stride, metric, n, s);
}
int dh_crc16(const uint8_t* in, size_t stride, int count, uint16_t* out, size_t n, void* s) {
    if (count < 0 || stride < (size_t) count || ((!in || !out) && n)) return DH_EINVAL;
    return dh_be_crc16(in, stride, count, out, n, s);
}
int dh_whitening(const uint8_t* in, uint8_t* out, size_t stride, int n_bits, size_t n, void* s) {
    if (n_bits < 0 || n_bits > 255 || stride < (size_t) (n_bits + 7) / 8 || ((!in || !out) && n)) return DH_EINVAL;
    return dh_be_whitening(in, out, stride, n_bits, n, s);
}
int dh_dvfilter_s16(const int16_t* in, int16_t* out, float* state, size_t B, size_t stride, size_t n, void* s) {
    if (!in || !out || !state || stride < n) return DH_EINVAL;
    return dh_be_dvfilter(in, out, state, B, stride, n, s);
}

int dh_debug_div_gain(const float* in, float* out, size_t n, int narrow, void* s) {
    if ((!in || !out) && n) return DH_EINVAL;
    return dh_be_div_gain(in, out, n, narrow, s);
}

int dh_frontend_s16(const int16_t* in, size_t in_stride, float* out, size_t out_stride, float* state, size_t B, size_t n, int mode, int dcblock, void* s) {
    if (mode != DH_FE_AUDIO_S16 && mode != DH_FE_IQ_S16) return DH_EINVAL;
    if (((!in || !out) && n) || !state || out_stride < n || in_stride < n * (mode == DH_FE_IQ_S16 ? 2u : 1u)) return DH_EINVAL;
    return dh_be_frontend(in, in_stride, out, out_stride, state, B, n, mode, dcblock, s);
}

int dh_debug_div_const(const float* in, float* out, size_t n, unsigned divisor, void* s) {
    if (((!in || !out) && n) || divisor == 0) return DH_EINVAL;
    return dh_be_div_const(in, out, n, divisor, s);
}

int dh_debug_mfma_f16(const uint16_t* a, const uint16_t* b, const float* c, float* d, size_t tiles, void* s) {
    if ((!a || !b || !c || !d) && tiles) return DH_EINVAL;
    return dh_be_mfma_f16(a, b, c, d, tiles, s);
}
int dh_debug_f16_split(const float* in, uint16_t* h1, uint16_t* h2, size_t n, float scale, void* s) {
    if ((!in || !h1 || !h2) && n) return DH_EINVAL;
    return dh_be_f16_split(in, h1, h2, n, scale, s);
}
int dh_debug_seam_probe_words(int op, size_t* in_words, size_t* out_words) {
    DhProbeShape w;
    if (!dh_probe_shape(op, w)) return DH_EINVAL;
    if (in_words) *in_words = w.in_words;
    if (out_words) *out_words = w.out_words;
    return DH_OK;
}
int dh_debug_seam_probe(int op, const uint32_t* in, uint32_t* out, size_t cases, void* s) {
    DhProbeShape w;
    if (!dh_probe_shape(op, w) || ((!in || !out) && cases)) return DH_EINVAL;
    return dh_be_seam_probe(op, in, out, cases, s);
}

int dh_debug_copy(const void* src, void* dst, size_t n_bytes, void* s) {
    if ((!src && n_bytes) || (n_bytes & 15u) || (((uintptr_t) src | (uintptr_t) dst) & 15u)) return DH_EINVAL;      // (dst == null: read only)
    return dh_be_copy_kernel(src, dst, n_bytes, s);
}

int dh_engine_create(const dh_engine_config* cfg, dh_engine** out) {
    if (!cfg || !out) return DH_EINVAL;
    return dh_create(*cfg, out, [&](dh_engine& e) { return e.impl.init(*cfg); });      // (init validates: make_layout)
}
void dh_engine_destroy(dh_engine* e) { dh_destroy(e); }

int dh_engine_reset(dh_engine* e) { DH_ENTER(e); return e->impl.reset(); }
int dh_engine_set_slot_filter(dh_engine* e, uint32_t f) { DH_ENTER(e); return e->impl.set_slot_filter(f); }
int dh_engine_reset_channel(dh_engine* e, uint32_t ch) { DH_ENTER(e); return e->impl.reset_channel(ch); }
int dh_engine_reset_channels(dh_engine* e, const uint8_t* d_flags) { DH_ENTER(e); return e->impl.reset_channels(d_flags); }
int dh_engine_set_slot_filter_channel(dh_engine* e, uint32_t ch, uint32_t f) { DH_ENTER(e); return e->impl.set_slot_filter_channel(ch, f); }
int dh_engine_push(dh_engine* e, const float* d, size_t stride, size_t n) { DH_ENTER(e); return e->impl.push(d, stride, n); }
int dh_engine_push_host(dh_engine* e, const float* h, size_t stride, size_t n) { DH_ENTER(e); return e->impl.push_host(h, stride, n); }
int dh_engine_push_ragged(dh_engine* e, const float* d, size_t stride, const uint32_t* d_counts, size_t max_n) {
    DH_ENTER_IF(e, d_counts);
    return e->impl.push(d, stride, max_n, d_counts);
}
int dh_engine_push_host_ragged(dh_engine* e, const float* h, size_t stride, const uint32_t* h_counts, size_t max_n) {
    DH_ENTER_IF(e, h_counts);
    return e->impl.push_host(h, stride, max_n, h_counts);
}
int dh_engine_push_symbols(dh_engine* e, const uint8_t* d, size_t stride, const uint32_t* cnt) { DH_ENTER(e); return e->impl.push_symbols(d, stride, cnt); }

int dh_engine_filtered(dh_engine* e, const float** d, size_t* stride) { return dh_rows_view(e, DH_ROWS_FILTERED, (const void**) d, stride, nullptr); }
int dh_engine_symbols(dh_engine* e, const uint8_t** d, size_t* stride, const uint32_t** cnt) { return dh_rows_view(e, DH_ROWS_SYMBOLS, (const void**) d, stride, cnt); }
int dh_engine_frames(dh_engine* e, const uint8_t** d, size_t* stride, const uint32_t** cnt) { return dh_rows_view(e, DH_ROWS_FRAMES, (const void**) d, stride, cnt); }
int dh_engine_events(dh_engine* e, const dh_event** d, size_t* stride, const uint32_t** cnt) { return dh_rows_view(e, DH_ROWS_EVENTS, (const void**) d, stride, cnt); }
int dh_engine_debug_header(dh_engine* e, uint32_t word, uint32_t* h_out) {
    DH_ENTER(e);
    return e->impl.debug_header(word, h_out);
}
int dh_engine_timing_stats(dh_engine* e, uint32_t* h_blocks, uint32_t* h_ordered) {
    DH_ENTER(e);
    return e->impl.timing_stats(h_blocks, h_ordered);
}
int dh_engine_read_symbols(dh_engine* e, uint32_t ch, uint8_t* h, size_t* n) { return dh_rows_read(e, DH_ROWS_SYMBOLS, ch, h, n); }
int dh_engine_read_frames(dh_engine* e, uint32_t ch, uint8_t* h, size_t* n) { return dh_rows_read(e, DH_ROWS_FRAMES, ch, h, n); }
int dh_engine_read_events(dh_engine* e, uint32_t ch, dh_event* h, size_t* n) { return dh_rows_read(e, DH_ROWS_EVENTS, ch, h, n); }
int dh_engine_read_filtered(dh_engine* e, uint32_t ch, float* h, size_t* n) { return dh_rows_read(e, DH_ROWS_FILTERED, ch, h, n); }
int dh_engine_timing_enable(dh_engine* e, uint32_t max_pushes) { DH_ENTER(e); return e->impl.be.timing_enable(max_pushes); }
int dh_engine_timing_read_split(dh_engine* e, float* first_ms, uint32_t* first_channels, uint32_t* n) {
    DH_ENTER_IF(e, n);
    return e->impl.be.timing_read_split(first_ms, first_channels, n);
}
int dh_engine_timing_read(dh_engine* e, float* rrc_ms, float* slicer_ms, float* decoder_ms, uint32_t* n) {
    DH_ENTER_IF(e, n);
    return e->impl.be.timing_read(rrc_ms, slicer_ms, decoder_ms, n);
}
int dh_engine_sync(dh_engine* e) {
    DH_ENTER(e);
    if (e->impl.be.sync()) return DH_EDEVICE;
    return e->impl.check_overflow();
}

}  // extern "C"

// ---- the channelizer (channelizer_core.hpp): host bookkeeping over the backend's memory and the dh_be_cz_* launches -----
//   dh_be_cz_window(float* cur, const float* prev, uint32_t prev_n, const void* in, int cf32, uint32_t H, size_t n_in, void* stream);
//   dh_be_cz_gemm(const DhCzParams& P, void* stream);
//   dh_be_cz_gemm_rat(const DhCzRatParams& R, void* stream);      (interpolation L > 1: one converter bank per phase)
//   dh_be_cz_fold(const DhCzFoldParams& F, void* stream);         (raster: the polyphase fold of one slab of output instants)
//   dh_be_cz_gemm_raster(const DhCzRasterParams& R, void* stream);         (... and its DFT + rotation)
//   dh_be_cz_fm(const float* zbuf, float* state, float* out, size_t out_stride, uint32_t B, uint32_t n_out, int dcblock, void* stream);
//   dh_be_cz_power(const DhCzPowerParams& P, void* stream);      (only with power enabled: block power, then the gate and the counts)
// (engine.hip defines the gfx950 ones; channelizer_core.hpp the CPU harness's.)  Two window buffers take turns: a push's
// window is the last H samples of the previous one followed by the new samples.  The kind of bank -- fixed (L = 1), rational
// (L > 1) or raster (K != 0) -- enters in init()'s geometry, in word_of() / columns() and in the GEMM step of push().
struct dh_channelizer : dh_state {                      // (clear() and retune() act on what init() and power_enable() declare)
    uint32_t B = 0, D = 0, L = 1, tpad = 0, ncols = 0, max_input = 0;      // rate = input L / D; tpad: T', or K' on a raster
    uint32_t hist = 0;                                  // H: T' - 1, or P K - 1 on a raster
    int cf32 = 0, fm = 0, dcblock = 0;
    std::vector<float> taps;                            // [L][T']: the phases h_p of h, each zero-padded to T'; raster: h padded to P K
    std::vector<uint32_t> word;                         // [B] a channel's word: u_b, or c_b on a raster
    std::vector<float> cols;                            // [2][2 T'] the column pair in the making
    float* d_tables = nullptr;                          // coarse ++ fine
    uint32_t* d_word = nullptr;                         // [B]
    float* d_bmat = nullptr;                            // [L][2 T'][ncols]
    float* d_win[2] = { nullptr, nullptr };             // [H + max_input][2] each
    float* d_state = nullptr;                           // [B][DH_CZ_STATE_WORDS]
    float* d_zbuf = nullptr;                            // FM: [max_input L / D + 1][B][2]
    uint8_t* d_stage = nullptr;                         // push_host's input
    int cur = 0;
    uint32_t prev_n = 0;
    uint64_t n0 = 0;                                    // samples pushed since create / reset
    DhCzRatParams rat{};                                // rat.g: what init() fixes; a push adds its window, its output rows and its
                                                        // position (L = 1), or its slots (L > 1)
    // what only a uniform raster owns (K != 0; bmat = one bank built from G): the fold buffer and what the rotation reads;
    // K = 0: nothing of it is allocated or launched
    uint32_t K = 0;
    float* d_taps = nullptr;                            // [P K]
    float* d_fold = nullptr;                            // [slab_rows][K'][2]
    uint32_t* d_phi = nullptr;                          // [K] Phi(q)
    uint32_t slab_rows = 0;
    DhCzFoldParams fold{};
    DhCzRasterParams ras{};
    // block power and gate (dh_channelizer_power_enable); pw.L = 0: off, nothing allocated and nothing launched
    DhCzPowerParams pw{};                               // what power_enable() and set_squelch() fix; a push adds its outputs and its position
    uint32_t* d_pstate = nullptr;                       // [B][DH_CZ_PSTATE_WORDS]
    uint64_t pw_first = 0; size_t pw_n = 0;             // blocks completed by the last push
    // frequency-error blocks (d_ferr of the power configuration); fe.ferr = null: off, nothing allocated and nothing launched
    DhCzFerrParams fe{};
    float* d_fstate = nullptr;                          // [B][2][4]: two copies of a channel's (Ar, Ai, z[j-1])
    uint32_t fe_copy = 0;                               // the copy the next launch reads; it writes the other one

    size_t in_bytes() const { return cf32 ? 8u : 4u; }
    uint64_t outputs(uint64_t n) const { return (uint64_t) L * n / D; }         // outputs that exist after n input samples
    size_t bank() const { return (size_t) 2 * tpad * ncols; }
    int clear() {
        cur = 0; prev_n = 0; n0 = 0; pw_first = 0; pw_n = 0; fe_copy = 0;
        return bufs.zero_all() ? DH_EDEVICE : DH_OK;
    }
    // a channel's word from the caller's value: the increment, or (a two's-complement int32) the bin reduced into [0, K)
    uint32_t word_of(uint32_t v) const { return K ? dh_cz_raster_bin((int32_t) v, K) : v; }
    // channel ch's column pair of bank p into `cols`
    void columns(uint32_t p, uint32_t ch) {
        float* re = cols.data(), * im = re + 2 * (size_t) tpad;
        if (K) dh_cz_raster_columns(K, tpad, word[ch], re, im);
        else dh_cz_columns(taps.data() + (size_t) p * tpad, tpad, word[ch], re, im);
    }
    // ... and from there into the B operand at bmat, every bank: put(a column's first element, its 2 T' values, pitch ncols)
    template <class Put> int place(float* bmat, uint32_t ch, Put put) {
        for (uint32_t p = 0; p < L; p++) {
            columns(p, ch);
            for (uint32_t c = 0; c < 2; c++)
                if (put(bmat + p * bank() + dh_cz_col(ch, c), cols.data() + c * 2 * (size_t) tpad)) return DH_EDEVICE;
        }
        return DH_OK;
    }
    int init(const dh_channelizer_config& c, uint32_t interp, uint32_t raster) {
        B = c.n_channels; D = c.decimation; L = interp; K = raster; ncols = dh_cz_ncols(B); max_input = c.max_input;
        cf32 = c.input_format == DH_CZ_CF32; fm = c.output_mode == DH_CZ_FM; dcblock = c.dcblock != 0;
        if (K) {                                        // geometry of a raster: one bank [2 K'][ncols] of G, one fold slab
            fold.P = (c.n_taps + K - 1u) / K;
            tpad = dh_cz_tpad(K); hist = fold.P * K - 1u; slab_rows = dh_cz_fold_slab_rows(tpad);
            taps.assign((size_t) fold.P * K, 0.0f);
            std::copy(c.taps, c.taps + c.n_taps, taps.begin());
        } else {                                        // ... of L converter banks
            tpad = dh_cz_tpad_rat(c.n_taps, L); hist = tpad - 1u;
            taps.assign((size_t) L * tpad, 0.0f);
            for (uint32_t p = 0; p < L; p++) {
                const uint32_t r = (uint32_t) (((uint64_t) p * D + D - 1u) % L);
                for (uint32_t k = 0; r + (uint64_t) k * L < c.n_taps; k++) taps[(size_t) p * tpad + k] = c.taps[r + k * L];
            }
        }
        word.resize(B);
        for (uint32_t b = 0; b < B; b++) word[b] = word_of(K ? (uint32_t) c.bins[b] : c.increments[b]);
        cols.resize(4 * (size_t) tpad);
        const size_t bm = L * bank(), win = 2 * ((size_t) hist + max_input);
        bool ok = bufs.alloc(d_tables, 4 * 4096);
        ok &= bufs.alloc(d_word, B);
        ok &= bufs.alloc(d_bmat, bm);
        ok &= bufs.alloc(d_win[0], win, dh::ZERO_ON_RESET);
        ok &= bufs.alloc(d_win[1], win, dh::ZERO_ON_RESET);
        ok &= bufs.alloc(d_state, (size_t) DH_CZ_STATE_WORDS * B, dh::ZERO_PER_CHANNEL);
        if (fm) ok &= bufs.alloc(d_zbuf, 2 * ((size_t) outputs(max_input) + 1) * B);
        ok &= bufs.alloc(d_stage, in_bytes() * max_input);
        if (K) ok &= bufs.alloc(d_phi, K) && bufs.alloc(d_taps, taps.size()) && bufs.alloc(d_fold, (size_t) 2 * slab_rows * tpad);
        if (!ok) return DH_ENOMEM;
        DhCzParams& g = rat.g;
        g.bmat = d_bmat; g.coarse = d_tables; g.fine = d_tables + 8192; g.inc = d_word; g.zbuf = d_zbuf;
        g.D = D; g.tpad = tpad; g.B = B; g.ncols = ncols; g.fm = fm; rat.L = L;
        std::vector<float> bmat(bm, 0.0f);
        for (uint32_t b = 0; b < B; b++)
            place(bmat.data(), b, [&](float* dst, const float* src) { for (size_t r = 0; r < 2 * (size_t) tpad; r++) dst[r * ncols] = src[r]; return 0; });
        if (be.upload(d_tables, dh_cz_host_tables(), sizeof(float) * 4 * 4096) || be.upload(d_word, word.data(), sizeof(uint32_t) * B) ||
            be.upload(d_bmat, bmat.data(), sizeof(float) * bm)) return DH_EDEVICE;
        if (K) {
            ras.g = g; ras.g.win = d_fold; ras.cbin = d_word; ras.phi = d_phi; ras.K = K;
            fold.h = d_taps; fold.fold = d_fold; fold.K = K; fold.kpad = tpad; fold.D = D;
            std::vector<uint32_t> phi(K);
            for (uint32_t q = 0; q < K; q++) phi[q] = dh_cz_raster_phi(q, K);
            if (be.upload(d_phi, phi.data(), sizeof(uint32_t) * K) || be.upload(d_taps, taps.data(), sizeof(float) * taps.size())) return DH_EDEVICE;
        }
        const int rc = clear();
        if (rc != DH_OK) return rc;
        return be.sync() ? DH_EDEVICE : DH_OK;           // (the host copies above are released on return)
    }
    // v: the channel's new increment, or its new bin
    int retune(uint32_t ch, uint32_t v) {
        word[ch] = word_of(v);
        const size_t pitch = sizeof(float) * ncols, rows = 2 * (size_t) tpad;
        if (place(d_bmat, ch, [&](float* dst, const float* src) { return be.upload2d(dst, pitch, src, sizeof(float), sizeof(float), rows); }) ||
            be.upload(d_word + ch, &word[ch], sizeof(uint32_t)) || bufs.zero_row(ch, B)) return DH_EDEVICE;
        return be.sync() ? DH_EDEVICE : DH_OK;
    }
    // raster: the push's no outputs slab by slab -- fold, then DFT + rotation
    int push_raster(const float* w, size_t n_in, float* out, size_t out_stride, uint32_t no) {
        fold.win = w; fold.win_n = (uint32_t) (hist + n_in);
        ras.g.out = out; ras.g.out_stride = out_stride;
        ras.m0 = (uint32_t) ((outputs(n0) * D + (D - 1u)) % K);
        const uint32_t wj = hist + (uint32_t) (D - 1 - n0 % D);        // window index of x[n_j] of the push's first row
        for (uint32_t row = 0; row < no; row += slab_rows) {
            fold.wj0 = wj + row * D; fold.nrows = std::min(slab_rows, no - row);
            ras.row0 = row; ras.g.n_out = fold.nrows;
            if (dh_be_cz_fold(fold, stream) || dh_be_cz_gemm_raster(ras, stream)) return DH_EDEVICE;
        }
        return DH_OK;
    }
    static bool level_ok(float v) { return v - v == 0.0f && v >= 0.0f; }       // finite and not negative
    int set_squelch(float open_level, float close_level, uint32_t hang) {
        if (!level_ok(open_level) || !level_ok(close_level) || close_level > open_level || hang > 65535u) return DH_EINVAL;
        pw.open_level = open_level; pw.close_level = close_level; pw.hang = hang;
        return DH_OK;
    }
    int power_enable(const dh_channelizer_power_config& c) {
        // d_ferr was appended to the struct: a caller built against the older header passes the older size, and the field is
        // then not read
        const bool v1 = c.struct_size == DH_CHANNELIZER_POWER_CONFIG_V1_SIZE;
        if ((!v1 && c.struct_size != sizeof(dh_channelizer_power_config)) || c.block < 1 || c.block > 65536 || !c.d_power || !c.d_gate || !c.d_counts ||
            c.stride < ((size_t) outputs(max_input) + 1) / c.block + 1 || n0 != 0)
            return DH_EINVAL;
        const int rc = set_squelch(c.open_level, c.close_level, c.hang_blocks);
        if (rc != DH_OK) return rc;
        const size_t words = (size_t) DH_CZ_PSTATE_WORDS * B;
        if (!d_pstate && !bufs.alloc(d_pstate, words, dh::ZERO_PER_CHANNEL)) return DH_ENOMEM;
        if (be.zero(d_pstate, sizeof(uint32_t) * words)) return DH_EDEVICE;
        float* d_ferr = v1 ? nullptr : c.d_ferr;
        const size_t fwords = (size_t) DH_CZ_FSTATE_WORDS * B;
        if (d_ferr && !d_fstate && !bufs.alloc(d_fstate, fwords, dh::ZERO_PER_CHANNEL)) return DH_ENOMEM;
        if (d_ferr && be.zero(d_fstate, sizeof(float) * fwords)) return DH_EDEVICE;
        fe.ferr = d_ferr; fe.stride = c.stride; fe.B = B; fe.L = c.block; fe.fm = fm; fe_copy = 0;
        pw.pstate = d_pstate; pw.power = c.d_power; pw.gate = c.d_gate; pw.counts = c.d_counts; pw.stride = c.stride;
        pw.B = B; pw.L = c.block; pw.fm = fm; pw.inv = (float) (1.0 / (double) c.block);
        pw_first = 0; pw_n = 0;
        return DH_OK;
    }
    // block power of the push's no outputs (j0 the first), the gate and the counts; no = 0: the counts are zeros
    int power(const float* out, size_t out_stride, uint64_t j0, uint32_t no) {
        pw.z = fm ? d_zbuf : out; pw.z_stride = out_stride;
        pw.pos0 = (uint32_t) (j0 % pw.L); pw.n_out = no;
        pw.n_blocks = (uint32_t) ((j0 + no) / pw.L - j0 / pw.L);
        pw.nseg = no ? (uint32_t) (((uint64_t) pw.pos0 + no + pw.L - 1) / pw.L) : 0u;
        pw_first = j0 / pw.L; pw_n = pw.n_blocks;
        if (dh_be_cz_power(pw, stream)) return DH_EDEVICE;
        if (!fe.ferr || !no) return DH_OK;
        // the frequency-error blocks of the same segments, from one copy of the state into the other
        fe.z = pw.z; fe.z_stride = out_stride; fe.pos0 = pw.pos0; fe.n_out = no; fe.nseg = pw.nseg;
        fe.fin = d_fstate + 4u * fe_copy; fe.fout = d_fstate + 4u * (fe_copy ^ 1u);
        if (dh_be_cz_ferr(fe, stream)) return DH_EDEVICE;
        fe_copy ^= 1u;
        return DH_OK;
    }
    int push(const void* in, size_t n_in, float* out, size_t out_stride, size_t* n_out, bool host) {
        if (!n_out) return DH_EINVAL;
        *n_out = 0;
        if (n_in > max_input || (!in && n_in)) return DH_EINVAL;
        const uint64_t j0 = outputs(n0), no = outputs(n0 + n_in) - j0;
        if (no && (!out || out_stride < no)) return DH_EINVAL;
        if (!n_in) return pw.L ? power(out, out_stride, j0, 0) : DH_OK;
        const void* src = in;
        if (host) {
            if (be.upload(d_stage, in, in_bytes() * n_in)) return DH_EDEVICE;
            src = d_stage;
        }
        float* w = d_win[cur];
        if (dh_be_cz_window(w, d_win[cur ^ 1], prev_n, src, cf32, hist, n_in, stream)) return DH_EDEVICE;
        if (no) {
            rat.g.win = w; rat.g.out = out; rat.g.out_stride = out_stride;
            if (K) {
                const int rc = push_raster(w, n_in, out, out_stride, (uint32_t) no);
                if (rc != DH_OK) return rc;
            } else if (L == 1) {
                rat.g.j0 = j0; rat.g.off0 = (uint32_t) (D - 1 - n0 % D); rat.g.n_out = (uint32_t) no;
                if (dh_be_cz_gemm(rat.g, stream)) return DH_EDEVICE;
            } else {
                dh_cz_plan_rat(rat, n0, n_in);
                if (dh_be_cz_gemm_rat(rat, stream)) return DH_EDEVICE;
            }
            if (fm && dh_be_cz_fm(d_zbuf, d_state, out, out_stride, B, (uint32_t) no, dcblock, stream)) return DH_EDEVICE;
        }
        if (pw.L) { const int rc = power(out, out_stride, j0, (uint32_t) no); if (rc != DH_OK) return rc; }
        if (host && be.sync()) return DH_EDEVICE;       // the staging buffer is the next push's
        cur ^= 1; prev_n = (uint32_t) n_in; n0 += n_in;
        *n_out = (size_t) no;
        return DH_OK;
    }
};

extern "C" {

int dh_channelizer_create(const dh_channelizer_config* cfg, dh_channelizer** out) {
    if (!cfg || !out) return DH_EINVAL;
    *out = nullptr;
    const dh_channelizer_config& c = *cfg;
    // interpolation was appended to the struct: a caller built against the older header passes the older size and means L = 1
    const bool has_interp = c.struct_size >= offsetof(dh_channelizer_config, interpolation) + sizeof(c.interpolation);
    const uint32_t L = has_interp && c.interpolation ? c.interpolation : 1u;
    // raster and bins were appended after it.  raster sits in what was the older struct's tail padding, which that struct's
    // size covers and its callers never wrote, so raster is read only from a struct_size that covers bins as well: every
    // smaller size, or raster = 0, is the fixed-offset bank
    const bool has_raster = c.struct_size >= offsetof(dh_channelizer_config, bins) + sizeof(c.bins);
    const uint32_t K = has_raster ? c.raster : 0u;
    if (c.struct_size < offsetof(dh_channelizer_config, interpolation) || c.decimation < 1 || c.decimation > 1024 ||
        L > DH_CZ_MAX_L || L > c.decimation || std::gcd(L, c.decimation) != 1u || c.n_taps < 1 ||
        c.n_channels < 1 || c.n_channels > 65536 || c.max_input < 1 || c.max_input > (1u << 28) || !c.taps ||
        (c.input_format != DH_CZ_CS16 && c.input_format != DH_CZ_CF32) || (c.output_mode != DH_CZ_IQ_F32 && c.output_mode != DH_CZ_FM) ||
        (c.dcblock && c.output_mode != DH_CZ_FM))
        return DH_EINVAL;
    if (K ? !c.bins || K < 2 || K > DH_CZ_MAX_RASTER || L != 1u ||
            c.n_taps > (uint64_t) DH_CZ_MAX_FOLD_P * K || c.n_taps > DH_CZ_MAX_RASTER_TAPS
          : c.n_taps > 16384u * L || !c.increments)
        return DH_EINVAL;
    for (uint32_t k = 0; k < c.n_taps; k++)
        if (!(c.taps[k] - c.taps[k] == 0.0f)) return DH_EINVAL;        // finite taps only
    return dh_create(c, out, [&](dh_channelizer& z) { return z.init(c, L, K); });
}
void dh_channelizer_destroy(dh_channelizer* z) { dh_destroy(z); }

int dh_channelizer_reset(dh_channelizer* c) { DH_ENTER(c); return c->clear(); }
int dh_channelizer_retune(dh_channelizer* c, uint32_t ch, uint32_t u) { DH_ENTER_IF(c, ch < c->B); return c->retune(ch, u); }
int dh_channelizer_push(dh_channelizer* c, const void* d_in, size_t n_in, float* d_out, size_t out_stride, size_t* n_out) {
    DH_ENTER(c);
    return c->push(d_in, n_in, d_out, out_stride, n_out, false);
}
int dh_channelizer_push_host(dh_channelizer* c, const void* h_in, size_t n_in, float* d_out, size_t out_stride, size_t* n_out) {
    DH_ENTER(c);
    return c->push(h_in, n_in, d_out, out_stride, n_out, true);
}
int dh_channelizer_power_enable(dh_channelizer* c, const dh_channelizer_power_config* cfg) {
    DH_ENTER_IF(c, cfg);
    return c->power_enable(*cfg);
}
int dh_channelizer_set_squelch(dh_channelizer* c, float open_level, float close_level, uint32_t hang_blocks) {
    if (!c || !c->pw.L) return DH_EINVAL;
    return c->set_squelch(open_level, close_level, hang_blocks);
}
int dh_channelizer_power_last(dh_channelizer* c, uint64_t* first_block, size_t* n_blocks) {
    if (!c || !c->pw.L || !first_block || !n_blocks) return DH_EINVAL;
    *first_block = c->pw_first; *n_blocks = c->pw_n;
    return DH_OK;
}
int dh_channelizer_phasor(const uint32_t* h_phi, float* h_out, size_t n) {
    if ((!h_phi || !h_out) && n) return DH_EINVAL;
    const float* t = dh_cz_host_tables();
    for (size_t i = 0; i < n; i++) dh_cz_phasor(h_phi[i], t, t + 8192, h_out[2 * i], h_out[2 * i + 1]);
    return DH_OK;
}

}  // extern "C"

// ---- the pre-roll ring (preroll_core.hpp): host bookkeeping over the backend's memory and two launches ---------------
//   dh_be_preroll_append(const DhPrAppend& A, void* stream);
//   dh_be_preroll_gather(const DhPrGather& G, void* stream);
// (engine.hip defines the gfx950 ones; preroll_core.hpp the CPU harness's.)  `total` is the host's: every position a
// launch needs is reduced mod depth here.
struct dh_preroll : dh_state {
    uint32_t B = 0, depth = 0;
    uint64_t total = 0;
    uint32_t* d_ring = nullptr;                         // [B][depth]
    uint64_t* d_open = nullptr;                         // [B]
    uint64_t* d_from = nullptr;                         // [B]: a gather's h_from
    std::vector<uint64_t> none;                         // [B] x DH_PREROLL_NONE: what a reset uploads

    uint64_t oldest() const { return total > depth ? total - depth : 0; }
    int clear() {
        total = 0;
        if (be.upload(d_open, none.data(), sizeof(uint64_t) * B)) return DH_EDEVICE;        // (the ring needs no clearing: nothing before
        return be.sync() ? DH_EDEVICE : DH_OK;                                              // sample 0 is ever read)
    }
    int init(const dh_preroll_config& c) {
        B = c.n_channels; depth = c.depth;
        none.assign(B, DH_PREROLL_NONE);
        bool ok = bufs.alloc(d_ring, (size_t) B * depth);
        ok &= bufs.alloc(d_open, B);
        ok &= bufs.alloc(d_from, B);
        return ok ? clear() : DH_ENOMEM;
    }
    int append(const float* rows, size_t stride, size_t n, const uint32_t* counts) {
        if (!n) return DH_OK;
        if (!rows || stride < n) return DH_EINVAL;
        DhPrAppend A{};
        A.ring = d_ring; A.open_at = d_open; A.rows = (const uint32_t*) rows; A.stride = stride; A.counts = counts;
        A.B = B; A.depth = depth; A.base = total;
        A.n = (uint32_t) std::min<size_t>(n, depth);
        A.rows += n - A.n;                              // n > depth: the last depth samples of every row
        A.w0 = (uint32_t) ((total + (n - A.n)) % depth);
        if (dh_be_preroll_append(A, stream)) return DH_EDEVICE;
        total += n;
        return DH_OK;
    }
    int gather(const uint64_t* from, uint64_t skip, size_t max_n, float* out, size_t out_stride, uint32_t* counts, uint64_t* h_start) {
        if (out_stride < max_n || (max_n && (!from || !out || !counts))) return DH_EINVAL;
        if (h_start && from)
            for (uint32_t b = 0; b < B; b++) h_start[b] = from[b] == DH_PREROLL_NONE ? DH_PREROLL_NONE : dh_pr_start(from[b], oldest());
        if (max_n && be.upload(d_from, from, sizeof(uint64_t) * B)) return DH_EDEVICE;
        return gather_device(d_from, skip, max_n, out, out_stride, counts);
    }
    // ... with `from` on the device already (the band monitor's step B wrote it): no upload, no host arithmetic
    int gather_device(const uint64_t* from, uint64_t skip, size_t max_n, float* out, size_t out_stride, uint32_t* counts) {
        if (out_stride < max_n || (max_n && (!from || !out || !counts))) return DH_EINVAL;
        if (!max_n) return counts && be.zero(counts, sizeof(uint32_t) * B) ? DH_EDEVICE : DH_OK;
        DhPrGather G{};
        G.ring = d_ring; G.from = from; G.out = (uint32_t*) out; G.out_stride = out_stride; G.counts = counts;
        G.B = B; G.depth = depth; G.max_n = (uint32_t) std::min<size_t>(max_n, depth);      // (no channel holds more)
        G.total = total; G.oldest = oldest(); G.skip = skip; G.r0 = (uint32_t) (G.oldest % depth);
        return dh_be_preroll_gather(G, stream) ? DH_EDEVICE : DH_OK;
    }
};

extern "C" {

int dh_preroll_create(const dh_preroll_config* cfg, dh_preroll** out) {
    if (!cfg || !out) return DH_EINVAL;
    *out = nullptr;
    if (cfg->struct_size < sizeof(dh_preroll_config) || cfg->n_channels < 1 || cfg->n_channels > 65536 || cfg->depth < 1 ||
        cfg->depth > (1u << 24))
        return DH_EINVAL;
    return dh_create(*cfg, out, [&](dh_preroll& p) { return p.init(*cfg); });
}
void dh_preroll_destroy(dh_preroll* p) { dh_destroy(p); }

int dh_preroll_reset(dh_preroll* p) { DH_ENTER(p); return p->clear(); }
int dh_preroll_append(dh_preroll* p, const float* d_rows, size_t stride, size_t n, const uint32_t* d_counts) {
    DH_ENTER(p);
    return p->append(d_rows, stride, n, d_counts);
}
int dh_preroll_total(dh_preroll* p, uint64_t* total) {
    if (!p || !total) return DH_EINVAL;
    *total = p->total;
    return DH_OK;
}
int dh_preroll_open_at(dh_preroll* p, uint64_t* h_open_at) {
    DH_ENTER_IF(p, h_open_at);
    return p->be.download(h_open_at, p->d_open, sizeof(uint64_t) * p->B) ? DH_EDEVICE : DH_OK;
}
int dh_preroll_gather(dh_preroll* p, const uint64_t* h_from, uint64_t skip, size_t max_n, float* d_out, size_t out_stride,
                      uint32_t* d_counts, uint64_t* h_start) {
    DH_ENTER(p);
    return p->gather(h_from, skip, max_n, d_out, out_stride, d_counts, h_start);
}
int dh_preroll_gather_device(dh_preroll* p, const uint64_t* d_from, uint64_t skip, size_t max_n, float* d_out, size_t out_stride,
                             uint32_t* d_counts) {
    DH_ENTER(p);
    return p->gather_device(d_from, skip, max_n, d_out, out_stride, d_counts);
}

}  // extern "C"

// ---- the packed read-out (outpack_core.hpp): host bookkeeping over the backend's memory and two launches ---------------
//   dh_be_outpack_scan(BE& engine_backend, const DhOutpack& P);      candidates, fit rule, entries, header
//   dh_be_outpack_copy(BE& engine_backend, const DhOutpack& P);      one workgroup per entry of this append
// (engine.hip defines the gfx950 ones; outpack_core.hpp the CPU harness's.)  Both go out on the ENGINE's stream, behind the
// push whose rows they read; the host knows none of the totals.
static_assert(sizeof(dh_outpack_header) == 32 && sizeof(dh_outpack_entry) == 32, "dh_outpack layout");
struct dh_outpack : dh_state {
    DhOutpack P{};                                      // what create fixes; an append adds the engine's rows and its arguments

    int clear() { return be.zero(P.hdr, sizeof(dh_outpack_header)) ? DH_EDEVICE : DH_OK; }
    int init(const dh_outpack_config& c) {
        P.max_entries = c.max_entries; P.max_events = c.max_events; P.max_frame_bytes = c.max_frame_bytes;
        bool ok = bufs.alloc(P.hdr, 1);
        ok &= bufs.alloc(P.scratch, 2);
        ok &= bufs.alloc(P.entries, c.max_entries);
        ok &= bufs.alloc(P.events, c.max_events);
        ok &= bufs.alloc(P.frames, (size_t) c.max_frame_bytes);
        if (!ok) return DH_ENOMEM;
        const int rc = clear();
        if (rc != DH_OK) return rc;
        return be.sync() ? DH_EDEVICE : DH_OK;
    }
    int append(dh_engine* e, const uint32_t* mask, const uint64_t* tag, uint64_t tag_add, uint32_t user) {
        auto& E = e->impl;
        if (!E.frames || !shares_stream(*e)) return DH_EINVAL;       // (no frames: proto == DH_PROTO_NONE)
        DhOutpack A = P;
        A.src_frames = E.frames; A.src_fc = E.frame_count; A.out_cap = E.L.out_cap;
        A.src_events = E.events; A.src_ec = E.ev_count; A.ev_cap = E.L.ev_cap;
        A.mask = mask; A.tag = tag; A.tag_add = tag_add; A.user = user; A.B = E.L.B;
        if (dh_be_outpack_scan(E.be, A) || dh_be_outpack_copy(E.be, A)) return DH_EDEVICE;
        return DH_OK;
    }
    int read(dh_outpack_header* hdr, dh_outpack_entry* entries, dh_event* events, uint8_t* frames) {
        dh_outpack_header h;
        if (be.download(&h, P.hdr, sizeof(h))) return DH_EDEVICE;                       // (synchronises)
        if (hdr) *hdr = h;
        if (entries && h.n_entries && be.download(entries, P.entries, sizeof(dh_outpack_entry) * h.n_entries)) return DH_EDEVICE;
        if (events && h.n_events && be.download(events, P.events, sizeof(dh_event) * h.n_events)) return DH_EDEVICE;
        if (frames && h.frame_bytes && be.download(frames, P.frames, (size_t) h.frame_bytes)) return DH_EDEVICE;
        return h.dropped ? DH_ECAPACITY : DH_OK;
    }
};

extern "C" {

int dh_outpack_create(const dh_outpack_config* cfg, dh_outpack** out) {
    if (!cfg || !out) return DH_EINVAL;
    *out = nullptr;
    if (cfg->struct_size < sizeof(dh_outpack_config) || cfg->max_entries == 0 || (cfg->max_frame_bytes & 15u) ||
        cfg->max_frame_bytes > ((uint64_t) 1 << 36) - 16u)
        return DH_EINVAL;
    return dh_create(*cfg, out, [&](dh_outpack& p) { return p.init(*cfg); });
}
void dh_outpack_destroy(dh_outpack* p) { dh_destroy(p); }

int dh_outpack_clear(dh_outpack* p) { DH_ENTER(p); return p->clear(); }
int dh_outpack_append(dh_outpack* p, dh_engine* e, const uint32_t* d_mask, const uint64_t* d_tag, uint64_t tag_add, uint32_t user) {
    DH_ENTER_IF(p, e);
    return p->append(e, d_mask, d_tag, tag_add, user);
}
int dh_outpack_read(dh_outpack* p, dh_outpack_header* h_hdr, dh_outpack_entry* h_entries, dh_event* h_events, uint8_t* h_frames) {
    DH_ENTER(p);
    return p->read(h_hdr, h_entries, h_events, h_frames);
}
int dh_outpack_device(dh_outpack* p, const dh_outpack_header** d_hdr, const dh_outpack_entry** d_entries, const dh_event** d_events,
                      const uint8_t** d_frames) {
    if (!p) return DH_EINVAL;
    if (d_hdr) *d_hdr = p->P.hdr;
    if (d_entries) *d_entries = p->P.entries;
    if (d_events) *d_events = p->P.events;
    if (d_frames) *d_frames = p->P.frames;
    return DH_OK;
}

}  // extern "C"

// ---- the band monitor (monitor_core.hpp): scan engines, ring and protocol engines behind one handle ------------------
//   dh_be_monitor_open(const DhMonOpen& A, void* stream);        step A
//   dh_be_monitor_assign(const DhMonAssign& S, void* stream);    step B
//   dh_be_monitor_close(const DhMonClose& C, void* stream);      step C (naming on close)
// (engine.hip defines the gfx950 ones; monitor_core.hpp the CPU harness's.)  All the host learns of a round is the summary
// block, read once after each step; everything [B]-sized stays on the device.
struct dh_monitor : dh_state {
    uint32_t B = 0, max_samples = 0;
    dh_engine* scan[DH_MON_FRONTS] = {};               // null: no configured protocol sits behind that front end
    dh_engine* eng[DH_MON_PROTOS] = {};                // by DH_PROTO_*; null: not configured
    dh_preroll* pre = nullptr;
    float* d_stage = nullptr;                           // [B][max_samples]: a replay chunk
    uint32_t* d_chunk_counts = nullptr;                 // [B]: its counts
    DhMonSummary* d_sum = nullptr;
    DhMonSummary sum{}, sum0{};                         // what was read last; what a round starts from
    DhMonOpen A{}; DhMonAssign S{}; DhMonClose Cl{};    // what create fixes; a round adds n and total
    bool close_on = false;                              // naming on close: any close_hits != 0
    std::vector<uint64_t> none;

    static uint32_t front_of(int proto) { return proto == DH_PROTO_NXDN ? 1u : proto == DH_PROTO_DSTAR ? 2u : proto == DH_PROTO_POCSAG ? 3u : 0u; }
    void release() {                                    // (hides dh_state's: the engines and the ring first)
        for (dh_engine*& e : scan) { dh_engine_destroy(e); e = nullptr; }
        for (dh_engine*& e : eng) { dh_engine_destroy(e); e = nullptr; }
        dh_preroll_destroy(pre); pre = nullptr;
        bufs.free_all();
    }
    int clear() {
        if (be.zero(A.assigned, B) || be.zero(A.closed_run, sizeof(uint32_t) * B) || be.upload(A.start, none.data(), sizeof(uint64_t) * B) ||
            be.upload(A.opened, none.data(), sizeof(uint64_t) * B))
            return DH_EDEVICE;
        return be.sync() ? DH_EDEVICE : DH_OK;
    }
    int make_engine(const dh_monitor_config& c, uint32_t front, int proto, dh_engine** out) {
        dh_engine_config ec{};
        ec.struct_size = sizeof(dh_engine_config); ec.device = c.device; ec.n_channels = c.n_channels; ec.max_samples = c.max_samples;
        ec.rrc = front == 0u ? DH_RRC_WIDE : front == 1u ? DH_RRC_NARROW : DH_RRC_NONE;
        ec.demod = front < 2u ? DH_DEMOD_GFSK4 : DH_DEMOD_FSK2;
        ec.sps = front == 1u ? 20u : front == 3u ? 40u : 10u;
        ec.flags = (front == 3u ? DH_FLAG_FSK_INVERT : 0u) | (proto == DH_PROTO_DMR && c.dmr_both_slots ? DH_FLAG_DMR_BOTH_SLOTS : 0u);
        ec.proto = proto; ec.slot_filter = 3; ec.stream = c.stream;
        return dh_engine_create(&ec, out);
    }
    int init(const dh_monitor_config& c) {
        B = c.n_channels; max_samples = c.max_samples;
        for (uint32_t f = 0; f < DH_MON_FAMILIES; f++) {
            Cl.close_hits[f] = c.close_hits[f]; Cl.close_dist[f] = c.close_dist[f];
            close_on |= c.close_hits[f] != 0u;
        }
        none.assign(B, DH_PREROLL_NONE);
        for (int p = 1; p < (int) DH_MON_PROTOS; p++) {
            if (!(c.protos >> p & 1u)) continue;
            const uint32_t f = front_of(p);
            int rc = scan[f] ? DH_OK : make_engine(c, f, DH_PROTO_SCAN, &scan[f]);
            if (rc == DH_OK) rc = make_engine(c, f, p, &eng[p]);
            if (rc != DH_OK) return rc;
        }
        dh_preroll_config pc{};
        pc.struct_size = sizeof(pc); pc.device = c.device; pc.n_channels = B; pc.depth = c.depth; pc.stream = c.stream;
        int rc = dh_preroll_create(&pc, &pre);
        if (rc != DH_OK) return rc;
        bool ok = bufs.alloc(d_stage, (size_t) B * max_samples);
        ok &= bufs.alloc(d_chunk_counts, B);
        ok &= bufs.alloc(d_sum, 1);
        ok &= bufs.alloc(A.assigned, B); ok &= bufs.alloc(A.closed_run, B); ok &= bufs.alloc(A.start, B); ok &= bufs.alloc(A.opened, B);
        ok &= bufs.alloc(A.scan_reset, B); ok &= bufs.alloc(A.scan_counts, B);
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++)
            if (eng[p]) { ok &= bufs.alloc(A.live_counts[p], B); ok &= bufs.alloc(S.new_flags[p], B); ok &= bufs.alloc(S.from[p], B); }
        if (!ok) return DH_ENOMEM;
        A.open_at = pre->d_open; A.sum = d_sum; A.B = B; A.release = c.release;
        for (uint32_t f = 0; f < DH_MON_FRONTS; f++)
            if (scan[f]) { S.stats[f] = scan[f]->impl.frames; S.stat_count[f] = scan[f]->impl.frame_count; S.stat_stride[f] = scan[f]->impl.L.out_cap; }
        S.scan_counts = A.scan_counts; S.open_at = pre->d_open; S.assigned = A.assigned; S.start = A.start; S.scan_reset = A.scan_reset;
        S.sum = d_sum; S.B = B; S.lead = c.lead; S.depth = c.depth; S.confirm = c.confirm;
        static_cast<DhMonStats&>(Cl) = S;
        Cl.scan_reset = A.scan_reset; Cl.opened = A.opened; Cl.assigned = A.assigned; Cl.start = A.start;
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++) { Cl.new_flags[p] = S.new_flags[p]; Cl.from[p] = S.from[p]; }
        Cl.sum = d_sum; Cl.B = B; Cl.lead = c.lead; Cl.depth = c.depth;
        for (uint32_t p = 0; p < DH_MON_PROTOS; p++) sum0.min_start[p] = DH_PREROLL_NONE;
        return clear();
    }
    int reset() {
        int rc = dh_preroll_reset(pre);
        for (dh_engine* e : scan) if (e && rc == DH_OK) rc = dh_engine_reset(e);
        for (dh_engine* e : eng) if (e && rc == DH_OK) rc = dh_engine_reset(e);
        return rc == DH_OK ? clear() : rc;
    }
    int reset_scanners() {
        for (dh_engine* e : scan) if (e) { const int rc = e->impl.reset_channels(A.scan_reset); if (rc != DH_OK) return rc; }
        return DH_OK;
    }
    int read_summary() { return be.download(&sum, d_sum, sizeof(sum)) ? DH_EDEVICE : DH_OK; }      // (synchronises)
    // pack (may be null): the sink of dh_monitor_push_packed -- every engine push of steps 6 and 7 is appended to it
    int push(const float* rows, size_t stride, size_t n, const uint32_t* counts, dh_monitor_sink sink, void* user, dh_outpack* pack = nullptr) {
        if (!n) return DH_OK;
        if (!rows || n > max_samples || stride < n) return DH_EINVAL;
        int rc = pre->append(rows, stride, n, counts);                                      // 1
        if (rc != DH_OK) return rc;
        const uint64_t total = pre->total;
        if (be.upload(d_sum, &sum0, sizeof(sum0))) return DH_EDEVICE;
        A.n = (uint32_t) n;
        if (dh_be_monitor_open(A, stream)) return DH_EDEVICE;                               // 2
        if ((rc = read_summary()) != DH_OK) return rc;
        const bool closing = close_on && sum.n_reset;                                       // C, in front of the reset that
        if (closing) {                                                                      // forgets what it judges
            Cl.total = total;
            if (dh_be_monitor_close(Cl, stream)) return DH_EDEVICE;
        }
        if (sum.n_reset && (rc = reset_scanners()) != DH_OK) return rc;                     // 3
        if (sum.n_scan) {
            for (dh_engine* e : scan)                                                       // 4
                if (e && (rc = e->impl.push(rows, stride, n, A.scan_counts)) != DH_OK) return rc;
            S.total = total;
            if (dh_be_monitor_assign(S, stream)) return DH_EDEVICE;                         // 5
            if ((rc = read_summary()) != DH_OK) return rc;
        } else if (closing && (rc = read_summary()) != DH_OK) return rc;
        dh_monitor_push_info info{};
        info.live_first = total - n;
        bool any_new = false;
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++) any_new |= sum.n_new[p] != 0u;
        if (any_new && sum.n_scan && (rc = reset_scanners()) != DH_OK) return rc;           // 6 (scan_reset: the channels step B named)
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++) {
            if (!eng[p] || !sum.n_new[p]) continue;
            if ((rc = eng[p]->impl.reset_channels(S.new_flags[p])) != DH_OK) return rc;
            const uint64_t span = total - sum.min_start[p];
            for (uint64_t skip = 0; skip < span; skip += max_samples) {
                if ((rc = pre->gather_device(S.from[p], skip, max_samples, d_stage, max_samples, d_chunk_counts)) != DH_OK) return rc;
                if ((rc = eng[p]->impl.push(d_stage, max_samples, max_samples, d_chunk_counts)) != DH_OK) return rc;
                info.proto = (int32_t) p; info.replay = 1; info.engine = eng[p]; info.d_counts = d_chunk_counts; info.d_start = S.from[p]; info.skip = skip;
                if (sink) sink(user, &info);
                if (pack && (rc = pack->append(eng[p], d_chunk_counts, S.from[p], skip, p | 1u << 8)) != DH_OK) return rc;
            }
        }
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++) {                                      // 7
            if (!eng[p] || !sum.n_live[p]) continue;
            if ((rc = eng[p]->impl.push(rows, stride, n, A.live_counts[p])) != DH_OK) return rc;
            info.proto = (int32_t) p; info.replay = 0; info.engine = eng[p]; info.d_counts = A.live_counts[p]; info.d_start = A.start; info.skip = 0;
            if (sink) sink(user, &info);
            if (pack && (rc = pack->append(eng[p], A.live_counts[p], nullptr, info.live_first, p)) != DH_OK) return rc;
        }
        return DH_OK;
    }
};

extern "C" {

int dh_monitor_create(const dh_monitor_config* cfg, dh_monitor** out) {
    if (!cfg || !out) return DH_EINVAL;
    *out = nullptr;
    const bool size_ok = cfg->struct_size == DH_MONITOR_CONFIG_V1_SIZE || cfg->struct_size == DH_MONITOR_CONFIG_V2_SIZE || cfg->struct_size >= sizeof(dh_monitor_config);
    if (!size_ok || cfg->n_channels < 1 || cfg->n_channels > 65536 || cfg->max_samples < 1 ||
        cfg->depth < 1 || cfg->depth > (1u << 24) || cfg->protos == 0 || (cfg->protos & ~0x3Eu))
        return DH_EINVAL;
    // dmr_both_slots, then close_hits and close_dist were appended to the struct: a caller built against an older header
    // passes that header's size and means 0 (only the bytes the caller's struct has are read)
    dh_monitor_config c{};
    memcpy(&c, cfg, cfg->struct_size < sizeof c ? cfg->struct_size : sizeof c);
    return dh_create(c, out, [&](dh_monitor& m) { return m.init(c); });
}
void dh_monitor_destroy(dh_monitor* m) { dh_destroy(m); }

int dh_monitor_reset(dh_monitor* m) { DH_ENTER(m); return m->reset(); }
int dh_monitor_push(dh_monitor* m, const float* d_rows, size_t stride, size_t n, const uint32_t* d_counts, dh_monitor_sink sink, void* user) {
    DH_ENTER(m);
    return m->push(d_rows, stride, n, d_counts, sink, user);
}
int dh_monitor_push_packed(dh_monitor* m, const float* d_rows, size_t stride, size_t n, const uint32_t* d_counts, dh_outpack* pack) {
    DH_ENTER_IF(m, pack && pack->shares_stream(*m));
    return m->push(d_rows, stride, n, d_counts, nullptr, nullptr, pack);
}
int dh_monitor_state(dh_monitor* m, uint8_t* h_assigned, uint64_t* h_start) {
    DH_ENTER(m);
    if (h_assigned && m->be.download(h_assigned, m->A.assigned, m->B)) return DH_EDEVICE;
    if (h_start && m->be.download(h_start, m->A.start, sizeof(uint64_t) * m->B)) return DH_EDEVICE;
    return DH_OK;
}
int dh_monitor_total(dh_monitor* m, uint64_t* total) {
    if (!m || !total) return DH_EINVAL;
    *total = m->pre->total;
    return DH_OK;
}
dh_engine* dh_monitor_engine(dh_monitor* m, int proto) { return m && proto > 0 && proto < (int) DH_MON_PROTOS ? m->eng[proto] : nullptr; }
dh_engine* dh_monitor_scan_engine(dh_monitor* m, int front) { return m && front >= 0 && front < (int) DH_MON_FRONTS ? m->scan[front] : nullptr; }

}  // extern "C"
