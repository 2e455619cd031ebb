// harness.cpp -- CPU wave-emulation build of the kernel bodies (TEST INFRASTRUCTURE ONLY).
//
// Compiles digiham_amd/csrc/*_core.hpp with a plain C++ compiler: DH_FOR_LANES becomes a
// 64-iteration loop, DH_BARRIER a no-op and "device memory" is the host heap.  The helper kernels
// and their launches are the device's own text (the ends of the core headers, digiham_amd/csrc/helper_launches.hpp): a launch
// visits every block and thread of the grid the launcher computed.  What is written here is the
// backend's plumbing, the three planned launches (a loop over workgroups each; the chain's runs
// digiham_amd/csrc/chain_core.hpp, the device's chain workgroup, over the device's grids) and the
// restatements of the kernels a thread-at-a-time visit cannot run (front-end, MFMA probe, copy).
// It exports the same C ABI as libdigiham_amd.so so the CPU-only test
// tier can run the engine's orchestration and the exact wave algorithms against the oracle.
// Which instantiation serves which configuration comes from digiham_amd/csrc/launch_plan.hpp, as
// on the device: every route the device chains or splits is chained or split here, a split
// push as the split launch and its fix-up launch -- what is exercised is the hand-over itself
// (flag word, give-up, told, fix-up), in index order, not only the part arithmetic.
// It is built into tests/host_harness/libdh_hostemu.so, is never installed, and the digiham_amd
// package has no code path that loads it: the product fails loudly without the gfx950 library.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/digiham_amd.h"
#include "../../digiham_amd/csrc/helper_launches.hpp"
#include "../../digiham_amd/csrc/chain_core.hpp"

namespace {

// test only (tests/host_cpp/handle_lifecycle.cpp): k > 0 makes the k-th backend allocation from now fail, once
int g_alloc_fail_in = 0;

struct HostBackend {
    struct Scope {};
    Scope scope() const { return Scope(); }
    void close() {}
    int open(int, void*) { return 0; }
    void* alloc(size_t bytes) { return g_alloc_fail_in && !--g_alloc_fail_in ? nullptr : calloc(1, bytes ? bytes : 1); }
    void free(void* p) { ::free(p); }
    int zero(void* p, size_t bytes) { memset(p, 0, bytes); return 0; }
    int upload(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    int copy_device(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    int download2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
        return upload2d(dst, dpitch, src, spitch, width, rows);
    }
    int upload2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
        for (size_t r = 0; r < rows; r++) memcpy((char*) dst + r * dpitch, (const char*) src + r * spitch, width);
        return 0;
    }
    int download(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    int sync() { return 0; }
    void* ms() { return nullptr; }
    void timing_mark(int) {}
    void timing_next() {}
    int timing_enable(uint32_t) { return 0; }
    int timing_read(float*, float*, float*, uint32_t* n) { *n = 0; return 0; }
    int timing_read_split(float*, uint32_t*, uint32_t* n) { *n = 0; return 0; }
    bool overlap_pushes = false;                     // (a property of the GPU dispatcher; nothing to emulate)

    // Which instantiation serves which configuration is launch_plan.hpp's to say, for this backend as for the device's:
    // the run_* below are what go_* are in engine.hip, one instantiation each.
    template <class I> static int run_rrc_demod(const DhDspParams& P) {
        std::vector<float> lds(dh_dsp_shared_bytes(P.sps, I::NZ) / sizeof(float));     // exactly the device allocation
        DhDspShared S = dh_dsp_carve(lds.data(), P.sps, I::NZ);
        for (uint32_t ch = 0; ch < P.n_channels; ch++) dh_rrc_demod_channel<I::NZ, I::FAST, I::SPS, 0, I::KEEPF>(P, ch, S);
        return 0;
    }
    int launch_rrc_demod(const DhDspParams& P, uint32_t nz, bool fast) {
        return dh_plan_rrc_demod(P, nz, fast, [&](auto i) { return run_rrc_demod<decltype(i)>(P); });
    }
    template <class I> static int run_rrc_tiles(const DhRrcParams& R) {
        std::vector<float> lds(dh_dsp_shared_bytes(0, I::NZ) / sizeof(float));
        DhDspShared S = dh_dsp_carve(lds.data(), 0, I::NZ);
        const uint32_t tiles = (R.n + DH_FTILE - 1) / DH_FTILE;
        for (uint32_t ch = 0; ch < R.n_channels; ch++)
            for (uint32_t t = 0; t < tiles; t++) dh_rrc_tile<I::NZ, I::FAST>(R, ch, t, S);
        return 0;
    }
    int launch_rrc_tiles(const DhRrcParams& R, uint32_t nz, bool fast) {
        return dh_plan_rrc_tiles(nz, fast, [&](auto i) { return run_rrc_tiles<decltype(i)>(R); });
    }
    // One chain instantiation: the grids the device launches, workgroup by workgroup in ASCENDING index order (not dh_launch,
    // which visits a grid last first: the hand-over of the tail split rests on index-order dispatch), every workgroup the
    // device's own text (chain_core.hpp), slicer and decoder sharing one block as they share the LDS.  The tail split, on every
    // route the device splits: DH_TAIL_SPLIT = percent of a push where the later parts start, launch_plan.hpp's grammar and
    // launch parameters.  The policy is this backend's own -- split whenever the variable is set and the push has two samples
    // (the tests are far below the device's thresholds).  The split launch, then the fix-up launch: flag words, give-ups
    // (DH_TAIL_SPLIT_FORCE_FAIL) and the fix-up's resumption are the real protocol, run sequentially.
    uint32_t part_epoch = 0;
    template <class I> int run_chain(const DhDspParams& P, const DhDecParams& D) {
        static_assert(alignof(DhDecShared) <= 16, "operator new aligns the block");
        std::vector<float> lds((std::max(dh_dsp_shared_bytes(I::SPS ? (uint32_t) I::SPS : P.sps, I::NZ), sizeof(DhDecShared)) + 3) / sizeof(float));     // as go_chain sizes it
        auto launch = [&](const DhDspParams& Q, uint32_t grid) {
            for (uint32_t bid = 0; bid < grid; bid++) dh_chain_workgroup<I::NZ, I::FAST, I::PROTO, I::SPS>(Q, D, bid, lds.data());
        };
        const DhTailSplitEnv env = dh_tail_split_env();
        if (I::MAY_SPLIT && env.pct && P.n >= 2) {
            DhDspParams Q = P;
            const DhSplitGrids G = dh_plan_split(Q, env.pct, env.pct2, part_epoch, env.force_fail);
            launch(Q, G.split);
            Q.split_fixup = 1u;
            launch(Q, G.fixup);
        } else launch(P, P.n_channels);
        return 0;
    }
    int launch_chain(const DhDspParams& P, const DhDecParams& D, uint32_t nz, bool fast, int proto) {
        return dh_plan_chain(P, nz, fast, proto, [&](auto i) { return this->template run_chain<decltype(i)>(P, D); });
    }
};

}  // namespace

static int dh_be_device_count() { return 0; }
static const char* dh_be_last_error() { return "host emulation"; }
static int dh_be_alloc(int, size_t bytes, void** out) { *out = calloc(1, bytes ? bytes : 1); return *out ? 0 : DH_ENOMEM; }
static int dh_be_free(void* p) { free(p); return 0; }
static int dh_be_copy(void* dst, const void* src, size_t bytes, int) { if (bytes) memcpy(dst, src, bytes); return 0; }
static int dh_be_frontend(const int16_t* in, size_t in_stride, float* out, size_t out_stride, float* state, size_t B, size_t n, int mode, int dcblock, void*) {
    for (size_t ch = 0; ch < B; ch++) dh_frontend_channel(in + ch * in_stride, out + ch * out_stride, state + ch * DH_FE_STATE_WORDS, n, mode, dcblock);
    return 0;
}

// (harness: products of halves are exact in f32; a k-ordered chain of rounded additions is one of the behaviours (H1) allows)
static int dh_be_mfma_f16(const uint16_t* a, const uint16_t* b, const float* c, float* d, size_t tiles, void*) {
    for (size_t t = 0; t < tiles; t++) for (int m = 0; m < 16; m++) for (int n = 0; n < 16; n++) {
        float acc = c[t * 256 + m * 16 + n];
        for (int k = 0; k < 32; k++) acc = __builtin_fmaf(dh_f16_value(a[t * 512 + m * 32 + k]), dh_f16_value(b[t * 512 + k * 16 + n]), acc);
        d[t * 256 + m * 16 + n] = acc;
    }
    return 0;
}
static int dh_be_copy_kernel(const void* src, void* dst, size_t n_bytes, void*) { if (dst) __builtin_memcpy(dst, src, n_bytes); return 0; }
#define DH_BACKEND HostBackend
#include "../../digiham_amd/csrc/abi_impl.hpp"
