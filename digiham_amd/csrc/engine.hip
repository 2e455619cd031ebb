// engine.hip -- gfx950 kernels + HIP backend of the engine; builds libdigiham_amd.so.
//
// Launch geometry: every streaming kernel is ONE 64-lane wavefront per workgroup, one channel per
// wavefront (grid = n_channels, or channels x tiles for the stand-alone RRC).  Channels share no
// data, so the workgroup -> XCD round-robin of the dispatcher needs no remapping: each XCD's L2
// only ever holds its own channels' rows, and 16 384-channel grids give 64 workgroups per CU.
// Batch FEC kernels are one item per lane, 256-lane workgroups, grid-stride.
// The helper kernels and their launches stand at the ends of the core headers and in helper_launches.hpp, one text for this build and the
// CPU harness; the chain workgroup (slicer, decoder, the hand-over of the tail split) is chain_core.hpp, one text likewise, and
// k_chain its launch-shape wrapper; here are the kernels that need barriers, LDS staging, matrix cores or wave votes.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
// (no FMA contraction anywhere: products and sums of the exact paths round separately, as the
// reference's x86-64 SSE2 build does; the FAST FIR asks for fmaf explicitly).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/digiham_amd.h"
#include "kernels_core.hpp"
#include "outpack_core.hpp"
#include "chain_core.hpp"
#include "fec_tables.hpp"
#include "rrc_taps.h"

namespace {

thread_local std::string g_last_error;

int hip_fail(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return -1;
}
#define HIP_TRY(expr) do { if (hip_fail((expr), #expr)) return DH_EDEVICE; } while (0)

}  // namespace

// The launch of a helper kernel (the core headers and helper_launches.hpp state each one, for this build and the CPU harness; declared in dh_portable.hpp): the one place a
// launch failure is looked for, and its message names the kernel.
template <class K, class... A>
static int dh_launch(K kernel, dim3 grid, dim3 block, size_t lds_bytes, void* stream, const char* what, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t) stream, args...);
    return hip_fail(hipGetLastError(), what);
}
static int dh_fec_tables(const DhFecTables** out);
static int dh_be_golay(const DhFecTables* T, int which, uint32_t* words, uint8_t* ok, size_t n, void* stream);
#include "helper_launches.hpp"

namespace {

#define DH_TILE_LB 3
#define DH_TILES_PER_WG 4
#define DH_LB_NARROW 3   // the 161-tap kernels: 168 VGPRs (their fused FIR fits; the rounded one, now the rare path, spills a little)
#define DH_SPLIT_MIN_CHANNELS 8192   // DH_FLAG_OVERLAP_PUSHES takes effect for engines at least this large (HipBackend::go_chain)
#define DH_TAIL_SPLIT_PCT 80
#define DH_TAIL_SPLIT_PCT2 0       // a third workgroup per channel from this percentage on (0 = two parts)
#define DH_TAIL_SPLIT_MIN_CHANNELS 8192     // the tail split of the chain kernels (HipBackend::go_chain) takes effect for launches at least this wide ...
#define DH_TAIL_SPLIT_MIN_SAMPLES 65536     // ... and pushes at least this long
#ifndef DH_LB
#define DH_LB 4          // minimum waves per SIMD the wide-filter kernels are register-budgeted for (128 VGPRs)
#endif
// ---------------------------------------------------------------------------------- kernels
// second launch-bounds argument = minimum waves per SIMD: caps the VGPR budget at 128 (wide) / 256 (narrow)
// KEEPF: the launch also delivers the filtered samples (DhDspParams::filt_out; BASELINE configs[1] in one kernel)
template <int NZ, bool FAST, int SPS, int KEEPF = 0>
__global__ __launch_bounds__(DH_WAVE, (NZ > 80 ? DH_LB_NARROW : DH_LB)) void k_rrc_demod(const DhDspParams P) {
    extern __shared__ __attribute__((aligned(16))) char dh_smem[];
    DhDspShared S = dh_dsp_carve(dh_smem, SPS ? (uint32_t) SPS : P.sps, NZ);
    dh_rrc_demod_channel<NZ, FAST, SPS, 0, KEEPF>(P, blockIdx.x, S);
}

// The whole chain of one channel in one wavefront: slice this push's samples, then run the protocol decoder over
// the symbols just produced.  The decoder is latency-bound (scalar control, LDS round trips); inside this kernel
// its stalls are covered by the other wavefronts' FIR arithmetic instead of by nothing, as in a separate launch.
// The two stages use the LDS block one after the other.  The body, and the tail split's hand-over in it: dh_chain_workgroup (chain_core.hpp).
// SPS = 10 is the specialised slicer of the DMR / YSF / D-Star pipes, SPS = 0 takes the run-time value (NXDN: 20).
// PART only names the launch: with DH_FLAG_OVERLAP_PUSHES a push of a large engine goes out as two launches (PART 0 =
// the first channels on the engine's high-priority stream, PART 1 = the rest on its normal-priority one; see
// HipBackend::go_chain), and profilers should list them apart.
template <int NZ, bool FAST, int PROTO, int SPS = 10, int PART = 0>
__global__ __launch_bounds__(DH_WAVE, (NZ > 80 ? DH_LB_NARROW : DH_LB)) void k_chain(const DhDspParams P, const DhDecParams D) {
    extern __shared__ __attribute__((aligned(16))) char dh_smem[];
    dh_chain_workgroup<NZ, FAST, PROTO, SPS>(P, D, blockIdx.x, dh_smem);
}

template <int NZ, bool FAST>
__global__ __launch_bounds__(DH_WAVE, (NZ > 80 ? DH_LB_NARROW : DH_TILE_LB)) void k_rrc_tile(const DhRrcParams R) {
    extern __shared__ __attribute__((aligned(16))) char dh_smem[];
    DhDspShared S = dh_dsp_carve(dh_smem, 0u, NZ);
    // DH_TILES_PER_WG consecutive tiles of one channel per wavefront: fewer, longer-lived workgroups
    const uint32_t tiles = (R.n + DH_FTILE - 1) / DH_FTILE;
    for (uint32_t t = blockIdx.x * DH_TILES_PER_WG; t < tiles && t < (blockIdx.x + 1u) * DH_TILES_PER_WG; t++)
        dh_rrc_tile<NZ, FAST>(R, blockIdx.y, t, S);
}

// which XCD workgroup i of a launch runs on (HipBackend::tail_split_probe)
__global__ __launch_bounds__(DH_WAVE) void k_xcc_probe(uint32_t* out) {
    if (threadIdx.x == 0) out[blockIdx.x] = dh_xcc_id();
}

// what the window phases of the slicer rest on (dsp_core.hpp, P3): eight / sixteen bytes read from LDS at an address that is only four-byte
// aligned come back whole (the queues run with the LDS alignment mode "unaligned"; a mode that rounds the address down would slice wrong
// symbols after every timing step of one sample).  HipBackend::lds_unaligned_probe looks once per device and process.
__global__ __launch_bounds__(DH_WAVE) void k_lds_unaligned_probe(uint32_t* out) {
#if DH_ON_GPU         // (the LDS read helpers only exist in the device pass)
    __shared__ float w[DH_WAVE + 8];
    w[threadIdx.x] = (float) threadIdx.x;
    if (threadIdx.x < 8) w[DH_WAVE + threadIdx.x] = (float) (DH_WAVE + threadIdx.x);
    __syncthreads();
    const uint32_t a = (uint32_t) (uintptr_t) (const __attribute__((address_space(3))) float*) (w + threadIdx.x);     // lane l: word l (odd lanes: not eight-byte aligned)
    const dh_f2 p = dh_lds_read_b64<0>(a);
    const dh_v4f q = dh_lds_read_b128<4>(a);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const float l = (float) threadIdx.x;
    const bool ok = p.x == l && p.y == l + 1.0f && q.x == l + 1.0f && q.y == l + 2.0f && q.z == l + 3.0f && q.w == l + 4.0f;
    const uint64_t all = __builtin_amdgcn_ballot_w64(ok);
    if (threadIdx.x == 0) out[0] = all == ~0ull ? 1u : 2u;
#else
    (void) out;
#endif
}

// Golay: syndrome LUT (16 KiB) staged in LDS once per workgroup, then grid-stride over the words
__global__ __launch_bounds__(256) void k_golay(const DhFecTables* T, int which, uint32_t* words, uint8_t* ok, size_t n) {
    __shared__ uint32_t lut[4096];
    __shared__ DhCode code;
    const uint32_t* src = which ? T->lut_g2412 : T->lut_g208;
    for (int i = threadIdx.x; i < 4096; i += blockDim.x) lut[i] = src[i];
    if (threadIdx.x == 0) code = which ? T->g2412 : T->g208;
    __syncthreads();
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        uint32_t w = words[i];
        const bool r = dh_block_decode(code, lut, w);
        words[i] = w;
        ok[i] = r ? 1 : 0;
    }
}

// The front-end in ONE launch (round 3): a workgroup of five wavefronts takes DH_FE_CH channels through tiles of DH_FE_TS
// samples, double-buffered.  Per tile: every thread of wavefronts 1..4 converts DH_FE_SPT consecutive samples of one channel (int16 audio, or I / Q pairs through the
// polar discriminator -- 16-byte loads, 128 contiguous bytes per channel and instruction) into an LDS tile; the first
// wavefront then runs the DC blocker's recurrence, one channel per lane, reading its row of the tile (padded: conflict-free)
// and writing the result back in place; every thread stores four floats of one channel (coalesced 512-byte rows).  No float
// round trip through HBM, int16 in -> float out: 4 + 4 bytes per sample instead of 4 + 4 + 4 + 4 + a second launch.
// Same arithmetic, operation for operation, as dh_frontend_channel (the CPU harness runs that; oracle/frontend.c is the checker).
#define DH_FE_CH 16
#define DH_FE_TS 128
#define DH_FE_SPT (DH_FE_CH * DH_FE_TS / 256)          // samples a thread converts per tile (a multiple of 4)
// (four dwords from a row that is only promised to be 4-byte aligned: the plain vector type would tell the compiler 16)
typedef uint32_t dh_u4w __attribute__((ext_vector_type(4), aligned(4)));
__global__ __launch_bounds__(320) void k_fe_fused(const int16_t* in, size_t in_stride, float* out, size_t out_stride, float* state, size_t B, size_t n, int mode, int dcblock) {
#if DH_ON_GPU
    // five wavefronts: the first runs the recurrence of tile k while the other four convert tile k + 1 into the second buffer
    __shared__ float tiles[2][DH_FE_CH][DH_FE_TS + 1];
    const int lane0 = threadIdx.x;                               // < 64: the recurrence wavefront
    const int tid = (int) threadIdx.x - 64;                      // 0..255: converting / storing threads
    const size_t ch0 = blockIdx.x * (size_t) DH_FE_CH;
    static_assert(DH_FE_SPT % 4 == 0 && DH_FE_SPT >= 4 && 256 % DH_FE_CH == 0, "whole 16-byte loads per thread");
    const int c = tid >= 0 ? tid / (256 / DH_FE_CH) : 0, s0 = tid >= 0 ? (tid % (256 / DH_FE_CH)) * DH_FE_SPT : 0;
    const bool c_ok = tid >= 0 && ch0 + c < B;
    const int16_t* row = in + (c_ok ? ch0 + c : ch0) * in_stride;
    const int32_t ip0 = c_ok ? (int32_t) state[(ch0 + c) * DH_FE_STATE_WORDS + 2] : 0, qp0 = c_ok ? (int32_t) state[(ch0 + c) * DH_FE_STATE_WORDS + 3] : 0;
    const bool aligned = (((uintptr_t) row) & 3u) == 0;          // (dword loads want 4-byte alignment; odd strides of int16 audio take the scalar route)
    float xp = 0.0f, yp = 0.0f;
    const bool rec = lane0 < DH_FE_CH && ch0 + lane0 < B;
    if (rec) { xp = state[(ch0 + lane0) * DH_FE_STATE_WORDS + 0]; yp = state[(ch0 + lane0) * DH_FE_STATE_WORDS + 1]; }

    auto convert = [&](size_t t0, float (*tile)[DH_FE_TS + 1]) {
        if (!c_ok || t0 >= n) return;
        const size_t t = t0 + s0;
        if (t + DH_FE_SPT <= n && aligned && mode == DH_FE_IQ_S16) {
            uint32_t w[DH_FE_SPT + 1];                           // the pair before the first sample, then this thread's pairs
            const uint32_t* p32 = reinterpret_cast<const uint32_t*>(row + 2 * t);
#pragma unroll
            for (int j = 0; j < DH_FE_SPT / 4; j++) { const dh_u4w v = *reinterpret_cast<const dh_u4w*>(p32 + 4 * j); w[1 + 4 * j] = v[0]; w[2 + 4 * j] = v[1]; w[3 + 4 * j] = v[2]; w[4 + 4 * j] = v[3]; }
            w[0] = t ? p32[-1] : (((uint32_t) (uint16_t) (int16_t) qp0) << 16) | (uint16_t) (int16_t) ip0;
#pragma unroll
            for (int j = 0; j < DH_FE_SPT; j++) {
                const int32_t i = (int16_t) (w[j + 1] & 0xFFFFu), q = (int16_t) (w[j + 1] >> 16);
                const int32_t ip = (int16_t) (w[j] & 0xFFFFu), qp = (int16_t) (w[j] >> 16);
                tile[c][s0 + j] = dh_fe_atan2_over_pi(q * ip - i * qp, i * ip + q * qp);
            }
        } else if (t + DH_FE_SPT <= n && aligned && mode == DH_FE_AUDIO_S16 && DH_FE_SPT % 8 == 0 && (in_stride & 1u) == 0) {
            const uint32_t* p32 = reinterpret_cast<const uint32_t*>(row + t);           // eight samples per 16-byte load
#pragma unroll
            for (int j = 0; j < DH_FE_SPT / 8; j++) {
                const dh_u4w v = *reinterpret_cast<const dh_u4w*>(p32 + 4 * j);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    tile[c][s0 + 8 * j + 2 * k] = (float) (int16_t) (v[k] & 0xFFFFu) * 0.000030517578125f;
                    tile[c][s0 + 8 * j + 2 * k + 1] = (float) (int16_t) (v[k] >> 16) * 0.000030517578125f;
                }
            }
        } else {
            for (int j = 0; j < DH_FE_SPT; j++) if (t + j < n) tile[c][s0 + j] = dh_fe_convert(row, t + j, mode, ip0, qp0);
        }
    };

    if (tid >= 0) convert(0, tiles[0]);
    __syncthreads();
    size_t k = 0;
    for (size_t t0 = 0; t0 < n; t0 += DH_FE_TS, k++) {
        float (*tile)[DH_FE_TS + 1] = tiles[k & 1];
        if (tid >= 0) convert(t0 + DH_FE_TS, tiles[(k + 1) & 1]);
        else if (rec && dcblock) {
            const size_t cnt = n - t0 < DH_FE_TS ? n - t0 : DH_FE_TS;
            float* r = tile[lane0];
            size_t i = 0;
            for (; i + 8 <= cnt; i += 8) {
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; j++) x[j] = r[i + j];
#pragma unroll
                for (int j = 0; j < 8; j++) { const float d = x[j] - xp; const float f = 0.995f * yp; yp = d + f; xp = x[j]; r[i + j] = yp; }
            }
            for (; i < cnt; i++) { const float x = r[i]; const float d = x - xp; const float f = 0.995f * yp; yp = d + f; xp = x; r[i] = yp; }
        } else if (rec) {
            const size_t cnt = n - t0 < DH_FE_TS ? n - t0 : DH_FE_TS;
            xp = tile[lane0][cnt - 1]; yp = xp;
        }
        __syncthreads();
        if (tid >= 0) {
#pragma unroll
            for (int pass = 0; pass < DH_FE_CH * DH_FE_TS / (256 * 4); pass++) {
                const int e = (pass * 256 + tid) * 4, cs = e / DH_FE_TS, q0 = e % DH_FE_TS;
                if (ch0 + cs < B) {
                    float* dst = out + (ch0 + cs) * out_stride + t0 + q0;
                    if (t0 + q0 + 4 <= n && ((((uintptr_t) dst) & 15u) == 0)) {
                        dh_f4a v; v.x = tile[cs][q0]; v.y = tile[cs][q0 + 1]; v.z = tile[cs][q0 + 2]; v.w = tile[cs][q0 + 3];
                        *reinterpret_cast<dh_f4a*>(dst) = v;
                    } else {
                        for (int j = 0; j < 4; j++) if (t0 + q0 + j < n) dst[j] = tile[cs][q0 + j];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (rec) {
        float* st = state + (ch0 + lane0) * DH_FE_STATE_WORDS;
        st[0] = xp; st[1] = yp;
        if (mode == DH_FE_IQ_S16 && n) { const int16_t* r = in + (ch0 + lane0) * in_stride; st[2] = (float) r[2 * n - 2]; st[3] = (float) r[2 * n - 1]; }
    }
#endif
}

// one tile per wavefront: D = C + A x B with v_mfma_f32_16x16x32_f16 (dh_debug_mfma_f16)
__global__ __launch_bounds__(DH_WAVE) void k_mfma_f16(const uint16_t* A, const uint16_t* B, const float* C, float* D) {
#if DH_ON_GPU
    const size_t t = blockIdx.x;
    const int l = threadIdx.x, m = l & 15, q = l >> 4;
    typedef unsigned short dh_us8 __attribute__((ext_vector_type(8)));
    dh_us8 a, b;
    for (int j = 0; j < 8; j++) { a[j] = A[t * 512 + m * 32 + 8 * q + j]; b[j] = B[t * 512 + (8 * q + j) * 16 + m]; }
    dh_f32x4 c;
    for (int r = 0; r < 4; r++) c[r] = C[t * 256 + (4 * q + r) * 16 + m];
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(dh_h8, a), __builtin_bit_cast(dh_h8, b), c, 0, 0, 0);
    for (int r = 0; r < 4; r++) D[t * 256 + (4 * q + r) * 16 + m] = c[r];
#endif
}
// dh_debug_copy: the streaming ceiling of the lease (16 bytes per lane, non-temporal both ways, four pieces in flight per lane)
typedef uint32_t dh_u4s __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_copy16(const dh_u4s* __restrict__ src, dh_u4s* __restrict__ dst, size_t n16) {
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const dh_u4s a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
        const dh_u4s c = __builtin_nontemporal_load(src + i + 2 * stride), d = __builtin_nontemporal_load(src + i + 3 * stride);
        __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + stride);
        __builtin_nontemporal_store(c, dst + i + 2 * stride); __builtin_nontemporal_store(d, dst + i + 3 * stride);
    }
    for (; i < n16; i += stride) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

// ... and the read-only rate (dh_debug_copy with a null destination): eight 16-byte non-temporal loads in flight per lane, the words folded
// into a value nobody stores -- what a kernel that mostly READS (the chain kernels: 93 % of their HBM traffic) can be priced against
__device__ uint32_t g_read_sink[4];
__global__ __launch_bounds__(256) void k_read16(const dh_u4s* __restrict__ src, size_t n16) {
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x;
    dh_u4s acc = { 0, 0, 0, 0 };
    for (; i + 7 * stride < n16; i += 8 * stride) {
        dh_u4s v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __builtin_nontemporal_load(src + i + u * stride);
#pragma unroll
        for (int u = 0; u < 8; u++) acc ^= v[u];
    }
    for (; i < n16; i += stride) acc ^= __builtin_nontemporal_load(src + i);
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u && acc.x == 0x9E3779B9u) { volatile uint32_t* sink = g_read_sink; sink[0] = acc.x; sink[1] = acc.y; }      // (volatile: the variable has internal linkage and no reader -- a plain store, and with it the whole kernel, is dead code)
}

// ---------------------------------------------------------------------------------- FEC tables
std::mutex g_tables_mutex;
DhFecTables* g_tables[64] = { nullptr };

int tables_for_current_device(const DhFecTables** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return DH_EINVAL;
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    if (!g_tables[dev]) {
        DhFecTables* host = new (std::nothrow) DhFecTables;
        if (!host) return DH_ENOMEM;
        dh::build_fec_tables(*host);
        DhFecTables* d = nullptr;
        if (hip_fail(hipMalloc((void**) &d, sizeof(DhFecTables)), "hipMalloc(tables)")) { delete host; return DH_ENOMEM; }
        const hipError_t e = hipMemcpy(d, host, sizeof(DhFecTables), hipMemcpyHostToDevice);
        delete host;
        if (hip_fail(e, "hipMemcpy(tables)")) { (void) hipFree(d); return DH_EDEVICE; }
        g_tables[dev] = d;
    }
    *out = g_tables[dev];
    return DH_OK;
}

// ---------------------------------------------------------------------------------- backend
struct HipBackend {
    int device = 0;
    hipStream_t stream = nullptr;

    // Every ABI entry that allocates, enqueues or copies runs inside a Scope: the calling thread's current device becomes
    // the engine's for the duration of the call and is put back afterwards.  Without it a thread whose current device is
    // another GPU (a new thread starts on device 0; torch may have selected any) would launch on that device's NULL
    // stream with this engine's pointers -- and the engine would leave the caller's (torch's) device changed.
    struct Scope {
        int prev = -1; bool switched = false;
        explicit Scope(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess; }
        ~Scope() { if (switched) (void) hipSetDevice(prev); }
        Scope(const Scope&) = delete;
        Scope& operator=(const Scope&) = delete;
    };
    Scope scope() const { return Scope(device); }

    int open(int dev, void* s) {
        int count = 0;
        if (hip_fail(hipGetDeviceCount(&count), "hipGetDeviceCount") || count <= 0) return DH_ENODEV;
        if (dev < 0 || dev >= count) return DH_EINVAL;
        device = dev; stream = (hipStream_t) s;
        // (the first open on a device runs a one-wavefront probe kernel on a stream of its own and waits for it: it synchronises with the
        // host once, and must not happen inside a global-mode stream capture; later opens take the cached verdict)
        const char* why = nullptr;
        const int lds = lds_unaligned_probe(&why);
        if (lds < 0) { g_last_error = "the device does not return unaligned 8 / 16-byte LDS reads whole (LDS alignment mode): the slicer kernels need it"; return DH_EDEVICE; }
        if (lds == 0) { g_last_error = why ? why : "the LDS alignment probe could not run"; return DH_EDEVICE; }
        if (!tail_split_probe()) tail_split_pct = 0;              // workgroup i does not run on XCD i mod 8 here (another part, a partitioned one): one workgroup per channel
        const DhTailSplitEnv env = dh_tail_split_env();          // DH_TAIL_SPLIT, DH_TAIL_SPLIT_FORCE_FAIL (launch_plan.hpp)
        tail_split_force_fail = env.force_fail;
        if (env.set && tail_split_pct) { tail_split_pct = env.pct; tail_split_pct2 = env.pct2; }     // (the probe's verdict stands: the environment can only move the split point, or switch it off)
        return DH_OK;
    }
    void drop_timing_events() {
        for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e);
        ev.clear(); ev_cap = ev_n = 0;
    }
    void close() {                                   // engine teardown: the timing events and the engine's own streams go with it
        if (join_pending) { (void) hipStreamSynchronize(side); (void) hipStreamSynchronize(side_lo); }
        drop_timing_events();
        drop_side();
        side_failed = false;
    }

    // ---- overlapped pushes (DH_FLAG_OVERLAP_PUSHES; engines of >= DH_SPLIT_MIN_CHANNELS DMR / YSF channels).
    // The last wavefronts of a launch run on a draining chip (one wavefront per channel, ~2.5 ms each: about 1 ms of a
    // 10 ms step), and on ONE stream the next push cannot start before the last wavefront of this one has gone.  In this
    // mode a push goes out as two launches on two streams of the engine's own -- three quarters of the channels at HIGH
    // priority, the rest at normal priority -- that depend on the caller's stream only through the moment of the push
    // (the input is ready) and on their own predecessors (the channels' state).  The dispatcher places low-priority
    // workgroups exactly when the high-priority launch has none left, so the second launch fills the drain of the first
    // and the first launch of the NEXT push fills the drain of the second.  The caller's stream is joined again when
    // anything is read, reset or synchronised through the engine: until then the INPUT BUFFER OF A PUSH MUST STAY
    // UNTOUCHED (that is the contract of the flag).  Measured: -6..8 % step time at 8 192 .. 32 768 channels.
    bool overlap_pushes = false;
    // tail split of the chain launches (go_chain): share of a push, in percent, that the first workgroup of a channel
    // takes; 0 = off.  DH_TAIL_SPLIT in the environment overrides it when the engine is created (A/B runs).
    uint32_t tail_split_pct = DH_TAIL_SPLIT_PCT, tail_split_pct2 = DH_TAIL_SPLIT_PCT2, part_epoch = 0, tail_split_force_fail = 0;
    // One probe launch per device and process: `grid` one-wavefront workgroups of `kernel` leave a word each, `judge` makes 1 (holds),
    // -1 (does not) or 0 (no finding) of them.  Only a finding is recorded in `verdict` (0 unknown; the caller holds its lock): a HIP
    // call that fails leaves it unknown and `why` names the call -- the next engine probes again.  The probe runs on a stream of
    // its own: the caller's may be capturing, or hold work this must not wait for.
    template <class Judge> int run_probe(int (&verdict)[64], const char* name, void (*kernel)(uint32_t*), const char* launch, uint32_t grid, const char** why, Judge judge) {
        Scope on_device(device);
        uint32_t* d = nullptr; std::vector<uint32_t> h(grid, 0u);
        hipStream_t probe = nullptr;
        static thread_local char msg[160];
        auto failed = [&](hipError_t e, const char* call) {
            if (e == hipSuccess) return false;
            std::snprintf(msg, sizeof(msg), "the %s probe could not run: %s: %s", name, call, hipGetErrorString(e));
            (void) hipGetLastError();
            *why = msg;
            return true;
        };
        if (failed(hipStreamCreateWithFlags(&probe, hipStreamNonBlocking), "hipStreamCreateWithFlags")) return 0;
        bool bad = failed(hipMalloc((void**) &d, sizeof(uint32_t) * grid), "hipMalloc");
        if (!bad) bad = failed(hipMemsetAsync(d, 0, sizeof(uint32_t) * grid, probe), "hipMemsetAsync");
        if (!bad) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(DH_WAVE), 0, probe, d);
            bad = failed(hipGetLastError(), launch) || failed(hipStreamSynchronize(probe), "hipStreamSynchronize") ||
                  failed(hipMemcpy(h.data(), d, sizeof(uint32_t) * grid, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        if (d) (void) hipFree(d);
        (void) hipStreamDestroy(probe);
        if (bad) return 0;
        const int v = judge(h.data());
        if (v) verdict[device] = v;
        return v;
    }
    // What the tail split's cheap hand-over rests on: the part is a gfx950 and the workgroups of a launch land on XCD (index
    // mod 8) -- 4 096 workgroups record HW_REG_XCC_ID per index.  A probe that could not run leaves the split off for THIS engine.
    // (Dispatch in index order cannot be probed; a hand-over that does not come is caught at run time, see chain_core.hpp.)
    bool tail_split_probe() {
        static std::mutex m; static int verdict[64] = { 0 };
        if (device < 0 || device >= 64) return false;
        std::lock_guard<std::mutex> lock(m);
        if (verdict[device]) return verdict[device] > 0;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void) hipGetLastError(); return false; }
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) { verdict[device] = -1; return false; }
        constexpr uint32_t N = 4096;
        const char* why = nullptr;
        return run_probe(verdict, "XCD placement", k_xcc_probe, "launch of k_xcc_probe", N, &why, [](const uint32_t* h) {
            bool ok = true;
            for (uint32_t i = 0; i < N && ok; i++) ok = h[i] < 8u && h[i] == h[i & 7u];
            for (uint32_t i = 0; i < 8 && ok; i++) for (uint32_t j = 0; j < i; j++) ok = ok && h[i] != h[j];      // eight XCDs, each index class its own
            return ok ? 1 : -1;
        }) > 0;
    }
    // see k_lds_unaligned_probe.  1 = unaligned reads come back whole, -1 = they do not (measured), 0 = the probe could not run (`why` says
    // which HIP call failed: an out-of-memory or a launch failure is not an alignment finding, and is not cached)
    int lds_unaligned_probe(const char** why) {
        static std::mutex m; static int verdict[64] = { 0 };
        if (device < 0 || device >= 64) { *why = "the LDS alignment probe keeps verdicts for device indices below 64"; return 0; }
        std::lock_guard<std::mutex> lock(m);
        if (std::getenv("DH_LDS_PROBE_FORCE_FAIL")) return -1;        // tests: what an engine on a device without unaligned LDS reads is told
        if (verdict[device]) return verdict[device];
        return run_probe(verdict, "LDS alignment", k_lds_unaligned_probe, "launch of k_lds_unaligned_probe", 1u, why, [&](const uint32_t* h) {
            if (h[0] == 0u) *why = "the LDS alignment probe could not run: the probe kernel left no result";
            return h[0] == 0u ? 0 : h[0] == 1u ? 1 : -1;
        });
    }
    hipStream_t side = nullptr, side_lo = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join_lo = nullptr;
    bool side_failed = false, join_pending = false;
    bool side_ready() {
        if (side) return true;
        if (side_failed) return false;
        int least = 0, greatest = 0;
        bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least &&
                  hipStreamCreateWithPriority(&side, hipStreamNonBlocking, greatest) == hipSuccess &&
                  hipStreamCreateWithPriority(&side_lo, hipStreamNonBlocking, least) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_join_lo, hipEventDisableTiming) == hipSuccess;
        if (!ok) { (void) hipGetLastError(); drop_side(); side_failed = true; }      // no stream priorities here: plain launches
        return ok;
    }
    void drop_side() {
        for (hipEvent_t* e : { &ev_fork, &ev_join, &ev_join_lo }) { if (*e) (void) hipEventDestroy(*e); *e = nullptr; }
        for (hipStream_t* t : { &side, &side_lo }) { if (*t) (void) hipStreamDestroy(*t); *t = nullptr; }
        join_pending = false;
    }
    // the caller's stream, once everything the engine has in flight on its own streams is ordered before it
    hipStream_t ms() {
        if (join_pending) {
            join_pending = false;
            (void) hipStreamWaitEvent(stream, ev_join, 0);
            (void) hipStreamWaitEvent(stream, ev_join_lo, 0);
        }
        return stream;
    }

    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hip_fail(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc")) return nullptr;
        return p;
    }
    void free(void* p) { (void) hipFree(p); }
    int zero(void* p, size_t bytes) { return hip_fail(hipMemsetAsync(p, 0, bytes, ms()), "hipMemsetAsync"); }
    int upload(void* dst, const void* src, size_t bytes) {
        // pageable source: hipMemcpyAsync stages it before returning, so the caller may free `src`
        return hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ms()), "hipMemcpyAsync(H2D)");
    }
    int copy_device(void* dst, const void* src, size_t bytes) {
        return hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ms()), "hipMemcpyAsync(D2D)");
    }
    int download2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
        if (!width || !rows) return 0;
        if (hip_fail(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToHost, ms()), "hipMemcpy2DAsync(D2H)")) return -1;
        return hip_fail(hipStreamSynchronize(ms()), "hipStreamSynchronize");
    }
    int upload2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
        if (!width || !rows) return 0;
        return hip_fail(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyHostToDevice, ms()), "hipMemcpy2DAsync(H2D)");
    }
    int download(void* dst, const void* src, size_t bytes) {
        if (hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ms()), "hipMemcpyAsync(D2H)")) return -1;
        return hip_fail(hipStreamSynchronize(ms()), "hipStreamSynchronize");
    }
    int sync() { return hip_fail(hipStreamSynchronize(ms()), "hipStreamSynchronize"); }
    int launched(const char* what) { return hip_fail(hipGetLastError(), what); }

    // per-push stage timestamps: 6 events per recorded push (0..3 on the caller's stream, 4..5 around the first launch of a
    // split push on the side stream)
    std::vector<hipEvent_t> ev;
    std::vector<uint32_t> ev_first_part;
    uint32_t ev_cap = 0, ev_n = 0;
    int timing_enable(uint32_t max_pushes) {
        drop_timing_events();
        ev.assign((size_t) max_pushes * 6, nullptr);
        ev_first_part.assign(max_pushes, 0u);
        for (auto& e : ev) if (hip_fail(hipEventCreate(&e), "hipEventCreate")) { close(); return DH_EDEVICE; }   // all or nothing
        ev_cap = max_pushes;
        return DH_OK;
    }
    void timing_mark(int k) {
        if (ev_n >= ev_cap) return;
        if (k == 0) ev_first_part[ev_n] = 0;
        (void) hipEventRecord(ev[(size_t) ev_n * 6 + k], k < 4 ? stream : side);
    }
    void timing_next() { if (ev_n < ev_cap) ev_n++; }
    int timing_read(float* rrc, float* slicer, float* decoder, uint32_t* n) {
        if (sync()) return DH_EDEVICE;
        const uint32_t cnt = ev_n < *n ? ev_n : *n;
        for (uint32_t i = 0; i < cnt; i++) {
            float a = 0, b = 0, c = 0;
            HIP_TRY(hipEventElapsedTime(&a, ev[i * 6 + 0], ev[i * 6 + 1]));
            HIP_TRY(hipEventElapsedTime(&b, ev[i * 6 + 1], ev[i * 6 + 2]));
            HIP_TRY(hipEventElapsedTime(&c, ev[i * 6 + 2], ev[i * 6 + 3]));
            if (rrc) rrc[i] = a;
            if (slicer) slicer[i] = b;
            if (decoder) decoder[i] = c;
        }
        *n = cnt; ev_n = 0;
        return DH_OK;
    }
    // the first launch of each recorded push that went out as two (call before timing_read, which starts a new series)
    int timing_read_split(float* first_ms, uint32_t* first_channels, uint32_t* n) {
        if (sync()) return DH_EDEVICE;
        const uint32_t cnt = ev_n < *n ? ev_n : *n;
        for (uint32_t i = 0; i < cnt; i++) {
            float a = 0;
            if (ev_first_part[i]) HIP_TRY(hipEventElapsedTime(&a, ev[i * 6 + 4], ev[i * 6 + 5]));
            if (first_ms) first_ms[i] = a;
            if (first_channels) first_channels[i] = ev_first_part[i];
        }
        *n = cnt;
        return DH_OK;
    }

    template <int NZ, bool FAST, int SPS, int KEEPF = 0> int go_rrc_demod(const DhDspParams& P) {
        const size_t lds = dh_dsp_shared_bytes(P.sps, NZ);
        if (lds > 48 * 1024) {
            if (hip_fail(hipFuncSetAttribute((const void*) k_rrc_demod<NZ, FAST, SPS, KEEPF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds),
                         "hipFuncSetAttribute")) return -1;
        }
        hipLaunchKernelGGL((k_rrc_demod<NZ, FAST, SPS, KEEPF>), dim3(P.n_channels), dim3(DH_WAVE), lds, ms(), P);
        return launched("k_rrc_demod");
    }
    // (which instantiation serves which configuration: launch_plan.hpp, for this backend and the CPU harness alike)
    int launch_rrc_demod(const DhDspParams& P, uint32_t nz, bool fast) {
        return dh_plan_rrc_demod(P, nz, fast, [&](auto i) { using I = decltype(i); return go_rrc_demod<I::NZ, I::FAST, I::SPS, I::KEEPF>(P); });
    }
    template <int NZ, bool FAST, int PROTO, int SPS = 10, bool MAY_SPLIT = false> int go_chain(const DhDspParams& P, const DhDecParams& D) {
        size_t lds = dh_dsp_shared_bytes(SPS ? (uint32_t) SPS : P.sps, NZ);
        if (lds < sizeof(DhDecShared)) lds = sizeof(DhDecShared);
        if constexpr (MAY_SPLIT) {
            if (overlap_pushes && P.n_channels >= DH_SPLIT_MIN_CHANNELS && side_ready()) {
                const uint32_t first = (P.n_channels - P.n_channels / 4u) & ~63u;       // three quarters, whole multiples of 64
                DhDspParams Q = P;
                Q.ch_base = first;
                // (the caller's stream is NOT joined first: work of earlier pushes still in flight on the engine's streams
                // is ordered before these launches by those streams themselves)
                if (hip_fail(hipEventRecord(ev_fork, stream), "hipEventRecord") ||
                    hip_fail(hipStreamWaitEvent(side, ev_fork, 0), "hipStreamWaitEvent") ||
                    hip_fail(hipStreamWaitEvent(side_lo, ev_fork, 0), "hipStreamWaitEvent")) return -1;
                if (ev_n < ev_cap) ev_first_part[ev_n] = first;
                timing_mark(4);
                hipLaunchKernelGGL((k_chain<NZ, FAST, PROTO, SPS, 0>), dim3(first), dim3(DH_WAVE), lds, side, P, D);
                timing_mark(5);
                hipLaunchKernelGGL((k_chain<NZ, FAST, PROTO, SPS, 1>), dim3(P.n_channels - first), dim3(DH_WAVE), lds, side_lo, Q, D);
                join_pending = true;                // work is on the side streams from here on: whatever happens next, they must be joined
                if (hip_fail(hipEventRecord(ev_join, side), "hipEventRecord") ||
                    hip_fail(hipEventRecord(ev_join_lo, side_lo), "hipEventRecord")) {
                    (void) hipStreamSynchronize(side); (void) hipStreamSynchronize(side_lo);       // no event to wait on: drain them here
                    join_pending = false;
                    return -1;
                }
                return launched("k_chain");
            }
        }
        if constexpr (MAY_SPLIT) {
            // Tail split (see chain_core.hpp): a launch of one workgroup per channel ends with a drain of about one workgroup's
            // duration during which the chip runs half empty (start / end stamps of every wavefront, profiles/r03_d_*: 0.65 ms of a 6.2 ms step).  With the
            // last quarter of every row handed to a second workgroup of the same launch the drain consists of workgroups a
            // third as long.  Only for launches that fill the chip several times over and pushes long enough to be worth
            // two prologues.
            if (tail_split_pct > 0 && P.n_channels >= DH_TAIL_SPLIT_MIN_CHANNELS && P.n >= DH_TAIL_SPLIT_MIN_SAMPLES) {
                DhDspParams Q = P;
                const DhSplitGrids G = dh_plan_split(Q, tail_split_pct, tail_split_pct2, part_epoch, tail_split_force_fail);      // (launch_plan.hpp)
                hipLaunchKernelGGL((k_chain<NZ, FAST, PROTO, SPS, 0>), dim3(G.split), dim3(DH_WAVE), lds, ms(), Q, D);
                if (launched("k_chain")) return -1;
                // The fix-up launch (PART 1 only names it for profilers): one workgroup per channel looks at the channel's flag
                // word and leaves -- a few microseconds for the whole grid -- unless a hand-over of the launch above failed, in
                // which case it finishes that row unsplit.  Stream order makes it see everything the split launch stored.
                Q.split_fixup = 1u;
                hipLaunchKernelGGL((k_chain<NZ, FAST, PROTO, SPS, 1>), dim3(G.fixup), dim3(DH_WAVE), lds, ms(), Q, D);
                return launched("k_chain (fix-up)");
            }
        }
        hipLaunchKernelGGL((k_chain<NZ, FAST, PROTO, SPS, 0>), dim3(P.n_channels), dim3(DH_WAVE), lds, ms(), P, D);
        return launched("k_chain");
    }
    // 1 = not available for this configuration (the caller launches the two stages separately), 0 = launched
    int launch_chain(const DhDspParams& P, const DhDecParams& D, uint32_t nz, bool fast, int proto) {
        return dh_plan_chain(P, nz, fast, proto, [&](auto i) { using I = decltype(i); return go_chain<I::NZ, I::FAST, I::PROTO, I::SPS, I::MAY_SPLIT>(P, D); });
    }
    template <int NZ, bool FAST> int go_rrc_tiles(const DhRrcParams& R) {
        const uint32_t tiles = (R.n + DH_FTILE - 1) / DH_FTILE;
        // channels on grid.y: at most 65 535 per launch
        for (uint32_t b0 = 0; b0 < R.n_channels; b0 += 65535u) {
            DhRrcParams Q = R;
            Q.n_channels = std::min<uint32_t>(R.n_channels - b0, 65535u);
            Q.in = R.in + (size_t) b0 * R.in_stride; Q.out = R.out + (size_t) b0 * R.out_stride; Q.hist = R.hist + (size_t) b0 * NZ;
            if (R.n_per) Q.n_per = R.n_per + b0;
            hipLaunchKernelGGL((k_rrc_tile<NZ, FAST>), dim3((tiles + DH_TILES_PER_WG - 1) / DH_TILES_PER_WG, Q.n_channels), dim3(DH_WAVE), dh_dsp_shared_bytes(0, NZ), ms(), Q);
            if (launched("k_rrc_tile")) return -1;
        }
        return 0;
    }
    int launch_rrc_tiles(const DhRrcParams& R, uint32_t nz, bool fast) {
        return dh_plan_rrc_tiles(nz, fast, [&](auto i) { using I = decltype(i); return go_rrc_tiles<I::NZ, I::FAST>(R); });
    }
};

// ---------------------------------------------------------------------------------- channelizer (channelizer_core.hpp)
// The channelizer's GEMM on v_mfma_f32_16x16x4_f32 (bit for bit the k-ordered fmaf chain of dh_cz_output).  A workgroup of
// four wavefronts computes DH_CZ_TM = 128 output instants x 128 real columns (64 channels); wavefront w takes rows 64 (w & 1)
// and columns 64 (w >> 1) onwards as 4 x 4 tiles of 16 x 16.  K runs over the taps in chunks of DH_CZ_TAP_STEP = 16 (32 real
// K rows) staged through LDS, the next chunk's global loads issued before this chunk's 128 MFMAs per wavefront.
//   As[row][kappa], kappa = 2 i + (0 re, 1 im) of tap k0 + i; row stride 36: the 16 rows x 4 K of one operand read hit 64 banks
//   Bs[kappa][col], row stride 144: likewise for the 4 K x 16 columns
//   MFMA operands: A lane (m = l & 15, q = l >> 4) = As[row m][4 s + q], B lane (n = l & 15, q) = Bs[4 s + q][col n];
//   D lane (n, g = l >> 4), register r = (row 4 g + r, col n).  Column tile 2 c holds sixteen channels' real parts and tile
//   2 c + 1 their imaginary parts (dh_cz_col), so each lane rotates and stores its own outputs.
// One tile of a decimating converter bank: rows row0 .. row0 + 127 of nrows, row i reading the window at wbase + i step - k
// against the B operand bmat; emit(i, b, yr, yi) gets each finished pair of chains.  k_cz_gemm (L = 1), k_cz_gemm_rat (one
// phase of a rational rate) and k_cz_gemm_raster (the DFT over folded rows) are its three instantiations.
#define DH_CZ_AS 36
#define DH_CZ_BS 144
template <class Emit>
__device__ __forceinline__ void dh_cz_gemm_tile(const DhCzParams& P, const float* bmat, uint32_t wbase, uint32_t step, uint32_t row0,
                                                uint32_t nrows, Emit emit) {
#if DH_ON_GPU
    __shared__ __attribute__((aligned(16))) float As[DH_CZ_TM * DH_CZ_AS];
    __shared__ __attribute__((aligned(16))) float Bs[32 * DH_CZ_BS];
    const int tid = (int) threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t col0 = blockIdx.y * (2u * DH_CZ_TNC);
    // loaders: A -- row ar = tid >> 1, taps 8 ah .. 8 ah + 7 of the chunk (window indices descending); B -- float4 number
    // tid + 256 i of the 32 x 128 slab
    const uint32_t ar = (uint32_t) tid >> 1, ah = (uint32_t) tid & 1u;
    const bool arow_ok = row0 + ar < nrows;
    const uint32_t abase = wbase + (row0 + ar) * step - 8u * ah;
    const float2* win = (const float2*) P.win;
    const uint32_t nch = P.tpad / DH_CZ_TAP_STEP;
    float2 ra[8];
    float4 rb[4];
    auto load = [&](uint32_t c) {
        const uint32_t k0 = DH_CZ_TAP_STEP * c;
#pragma unroll
        for (int e = 0; e < 8; e++) ra[e] = arow_ok ? win[abase - k0 - (uint32_t) e] : make_float2(0.0f, 0.0f);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t q = (uint32_t) tid + 256u * i, r = q >> 5, c4 = q & 31u;
            rb[i] = *(const float4*) (bmat + (size_t) (32u * c + r) * P.ncols + col0 + 4u * c4);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int e = 0; e < 8; e++) *(float2*) (As + ar * DH_CZ_AS + 2u * (8u * ah + (uint32_t) e)) = ra[e];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t q = (uint32_t) tid + 256u * i, r = q >> 5, c4 = q & 31u;
            *(float4*) (Bs + r * DH_CZ_BS + 4u * c4) = rb[i];
        }
    };
    const int m = lane & 15, q = lane >> 4;
    const float* ap = As + (64 * (w & 1) + m) * DH_CZ_AS + q;
    const float* bp = Bs + q * DH_CZ_BS + 64 * (w >> 1) + m;
    dh_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = dh_f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    load(0);
    stash();
    __syncthreads();
    for (uint32_t c = 0; c < nch; c++) {
        if (c + 1 < nch) load(c + 1);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            float a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; t++) { a[t] = ap[16 * t * DH_CZ_AS + 4 * s]; b[t] = bp[4 * s * DH_CZ_BS + 16 * t]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (c + 1 < nch) stash();
        __syncthreads();
    }
    const int g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t row = row0 + 64u * (uint32_t) (w & 1) + 16u * i + 4u * (uint32_t) g + r;
            if (row >= nrows) continue;
#pragma unroll
            for (int cg = 0; cg < 2; cg++) {
                const uint32_t b = (col0 + 64u * (uint32_t) (w >> 1) + 32u * cg) / 2u + (uint32_t) m;
                if (b < P.B) emit(row, b, acc[i][2 * cg][r], acc[i][2 * cg + 1][r]);
            }
        }
#endif
}

__global__ __launch_bounds__(256) void k_cz_gemm(const DhCzParams P) {
    dh_cz_gemm_tile(P, P.bmat, P.off0 + (P.tpad - 1u), P.D, blockIdx.x * DH_CZ_TM, P.n_out,
                    [&](uint32_t row, uint32_t b, float yr, float yi) { dh_cz_emit(P, row, b, yr, yi); });
}

// Rational rates: blockIdx.z is the slot (one phase of the push, channelizer_core.hpp), blockIdx.x its 128-row tiles.  The
// slots of a push differ by at most one row, so at most one workgroup per slot and column tile finds nothing to do.
__global__ __launch_bounds__(256) void k_cz_gemm_rat(const DhCzRatParams R) {
    const uint32_t s = blockIdx.z, row0 = blockIdx.x * DH_CZ_TM;
    const DhCzPhase ph = R.ph[s];
    if (row0 >= ph.count) return;
    dh_cz_gemm_tile(R.g, dh_cz_bank(R.g, ph.bank), ph.wbase, R.g.D, row0, ph.count,
                    [&](uint32_t i, uint32_t b, float yr, float yi) { dh_cz_emit_at(R.g, s + R.L * i, b, ph.nj0 + i * R.g.D, yr, yi); });
}

// Uniform raster (channelizer_core.hpp): the DFT stage is the tile above with the folded rows in the window's place -- row i's
// v[r] at i K' + K' - 1 - r, so wbase = K' - 1, step = K' and tpad = K' make it the specification's chain over r.
__global__ __launch_bounds__(256) void k_cz_gemm_raster(const DhCzRasterParams R) {
    dh_cz_gemm_tile(R.g, R.g.bmat, R.g.tpad - 1u, R.g.tpad, blockIdx.x * DH_CZ_TM, R.g.n_out,
                    [&](uint32_t i, uint32_t b, float yr, float yi) { dh_cz_emit_raster(R, i, b, yr, yi); });
}

// The polyphase fold of raster mode (host body dh_cz_fold_item).  A workgroup takes DH_CZ_FOLD_ROWS = 16 consecutive output
// instants (blockIdx.x) and 256 consecutive r (blockIdx.y), lane = r: one accumulator pair per (instant, r) in registers, p
// walked in increasing order with one load of h[r + p K] per sixteen instants.  Every input sample serves about T / D
// instants, so the span the tile needs goes through LDS: for the taps p0 <= p < p1 that is the (16 - 1) D + (p1 - p0 - 1) K
// + 256 samples below x[n_row0 - r0 - p0 K], and p advances in chunks of as many p as DH_CZ_FOLD_LDS = 6144 complex samples
// (48 KB: three workgroups per CU) hold; the accumulators stay in registers across chunks.  One p always fits while
// 15 D + 256 <= 6144, that is D <= 392, for every K and P; a larger D reads the window through L2 instead (its instants
// share almost nothing: a tile's rows are then > 392 samples apart and K <= 256 of them are used per p).
// LDS layout: the span as consecutive 8-byte samples.  A lane reads sample (255 - lane) + const, so the 32 lanes of a
// ds_read_b64 group cover 256 contiguous bytes, all 64 banks once: no conflicts whatever D and K are; the staging stores
// are lane-contiguous too.
__global__ __launch_bounds__(DH_CZ_FOLD_LANES) void k_cz_fold(const DhCzFoldParams F) {
    __shared__ __attribute__((aligned(16))) float2 xs[DH_CZ_FOLD_LDS];
    const uint32_t tid = threadIdx.x, r0 = blockIdx.y * DH_CZ_FOLD_LANES, r = r0 + tid, row0 = blockIdx.x * DH_CZ_FOLD_ROWS;
    const bool live = r < F.K;
    const float2* win = (const float2*) F.win;
    const int32_t top = (int32_t) (F.wj0 + row0 * F.D) - (int32_t) r0;          // window index of x[n_row0 - r0]
    const uint32_t rowspan = (DH_CZ_FOLD_ROWS - 1u) * F.D;
    float2 acc[DH_CZ_FOLD_ROWS];
#pragma unroll
    for (int i = 0; i < DH_CZ_FOLD_ROWS; i++) acc[i] = make_float2(0.0f, 0.0f);
    if (rowspan + DH_CZ_FOLD_LANES <= DH_CZ_FOLD_LDS) {
        const uint32_t pc = dh_min(F.P, 1u + (DH_CZ_FOLD_LDS - rowspan - DH_CZ_FOLD_LANES) / F.K);
        for (uint32_t p0 = 0; p0 < F.P; p0 += pc) {
            const uint32_t p1 = dh_min(F.P, p0 + pc);
            const uint32_t len = rowspan + (p1 - p0 - 1u) * F.K + DH_CZ_FOLD_LANES;
            const int32_t lo = top - (int32_t) (DH_CZ_FOLD_LANES - 1u) - (int32_t) ((p1 - 1u) * F.K);
            __syncthreads();                            // the previous chunk has been read
            for (uint32_t t = tid; t < len; t += DH_CZ_FOLD_LANES) {
                const int32_t idx = lo + (int32_t) t;   // below the window: r >= K lanes; above: the rows past nrows
                xs[t] = idx >= 0 && (uint32_t) idx < F.win_n ? win[idx] : make_float2(0.0f, 0.0f);
            }
            __syncthreads();
            if (live)
                for (uint32_t p = p0; p < p1; p++) {
                    const float hv = F.h[r + p * F.K];
                    const float2* s = xs + (DH_CZ_FOLD_LANES - 1u - tid) + (p1 - 1u - p) * F.K;
#pragma unroll
                    for (int i = 0; i < DH_CZ_FOLD_ROWS; i++) {
                        const float2 x = s[(uint32_t) i * F.D];
                        acc[i].x = __builtin_fmaf(hv, x.x, acc[i].x); acc[i].y = __builtin_fmaf(hv, x.y, acc[i].y);
                    }
                }
        }
    } else if (live) {
        for (uint32_t p = 0; p < F.P; p++) {
            const float hv = F.h[r + p * F.K];
            const int32_t base = top - (int32_t) tid - (int32_t) (p * F.K);
#pragma unroll
            for (int i = 0; i < DH_CZ_FOLD_ROWS; i++) {
                if (row0 + (uint32_t) i < F.nrows) {
                    const float2 x = win[base + (int32_t) ((uint32_t) i * F.D)];
                    acc[i].x = __builtin_fmaf(hv, x.x, acc[i].x); acc[i].y = __builtin_fmaf(hv, x.y, acc[i].y);
                }
            }
        }
    }
    if (r >= F.kpad) return;
    float2* out = (float2*) F.fold + (size_t) row0 * F.kpad + (F.kpad - 1u - r);
#pragma unroll
    for (int i = 0; i < DH_CZ_FOLD_ROWS; i++)
        if (row0 + (uint32_t) i < F.nrows) out[(size_t) i * F.kpad] = live ? acc[i] : make_float2(0.0f, 0.0f);
}

// ---------------------------------------------------------------------------------- band monitor (monitor_core.hpp)
// Step A of a round (B and C: monitor_core.hpp): one lane per channel, 256-thread workgroups, the loop bound the same for
// every lane of a workgroup so that the votes below see whole wavefronts.  Ordinary vector stores for the state and the
// per-channel outputs; the summary block takes one vector atomic per wavefront and non-zero count.  (Written in the 256-lane
// vocabulary of dh_portable.hpp, so that the CPU tier could run it, its prologue comes out scheduled differently: DESIGN.md
// section 4.  It stays as it is, with its restatement in monitor_core.hpp.)
__global__ __launch_bounds__(256) void k_monitor_open(const DhMonOpen A) {
    const bool first = (threadIdx.x & (DH_WAVE - 1)) == 0;
    for (uint32_t base = blockIdx.x * 256u; base < A.B; base += gridDim.x * 256u) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t r = b < A.B ? dh_mon_open_channel(A, b) : 0u;
        const uint32_t n_scan = (uint32_t) __popcll(__builtin_amdgcn_ballot_w64((r & 1u) != 0u));
        const uint32_t n_reset = (uint32_t) __popcll(__builtin_amdgcn_ballot_w64((r & 2u) != 0u));
        if (first && n_scan) atomicAdd(&A.sum->n_scan, n_scan);
        if (first && n_reset) atomicAdd(&A.sum->n_reset, n_reset);
        for (uint32_t p = 1; p < DH_MON_PROTOS; p++) {
            const uint32_t n_live = (uint32_t) __popcll(__builtin_amdgcn_ballot_w64((r >> 8) == p));
            if (first && n_live) atomicAdd(&A.sum->n_live[p], n_live);
        }
    }
}

// Masked reset of an engine: workgroup i takes channels i, i + gridDim.x, ...; a channel whose flag is 0 costs one byte
// read.  The 256 lanes zero row b of every declared buffer; the fence and the barrier put those zeros in memory before
// one lane writes the few non-zero words of a fresh channel over them (the flag is the same for the whole workgroup, so
// is the way through the barrier).
__global__ __launch_bounds__(256) void k_reset_channels(const DhResetChannels R) {
    for (uint32_t b = blockIdx.x; b < R.B; b += gridDim.x) {
        if (!R.flags[b]) continue;
        dh_rst_zero_rows(R, b, threadIdx.x, 256u);
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) dh_rst_init(R, b);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------- ABI hooks
static int dh_be_device_count() {
    int count = 0;
    if (hip_fail(hipGetDeviceCount(&count), "hipGetDeviceCount")) return DH_ENODEV;
    return count;
}
static const char* dh_be_last_error() { return g_last_error.c_str(); }
static int dh_be_alloc(int device, size_t bytes, void** out) {
    HIP_TRY(hipSetDevice(device));
    if (hip_fail(hipMalloc(out, bytes ? bytes : 1), "hipMalloc")) return DH_ENOMEM;
    return DH_OK;
}
static int dh_be_free(void* p) { HIP_TRY(hipFree(p)); return DH_OK; }
static int dh_be_copy(void* dst, const void* src, size_t bytes, int to_host) {
    if (!bytes) return DH_OK;
    HIP_TRY(hipMemcpy(dst, src, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice));
    return DH_OK;
}
// (the helper kernels' hooks: the core headers and helper_launches.hpp.  Here: what those launches take from this build, and the kernels whose
// device form a thread-at-a-time visit cannot run -- the CPU harness has restatements of these)
static int dh_fec_tables(const DhFecTables** out) { return tables_for_current_device(out); }
static int dh_be_golay(const DhFecTables* T, int which, uint32_t* words, uint8_t* ok, size_t n, void* stream) {
    return dh_launch(k_golay, dim3(grid_for(n, 256 * 8)), dim3(256), 0, stream, "k_golay", T, which, words, ok, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_frontend(const int16_t* in, size_t in_stride, float* out, size_t out_stride, float* state, size_t B, size_t n, int mode, int dcblock, void* stream) {
    if (!B || !n) return DH_OK;
    return dh_launch(k_fe_fused, dim3((unsigned) ((B + DH_FE_CH - 1) / DH_FE_CH)), dim3(320), 0, stream, "k_fe_fused", in, in_stride, out, out_stride, state, B, n, mode, dcblock) ? DH_EDEVICE : DH_OK;
}
static int dh_be_mfma_f16(const uint16_t* a, const uint16_t* b, const float* c, float* d, size_t tiles, void* stream) {
    if (!tiles) return DH_OK;
    return dh_launch(k_mfma_f16, dim3((unsigned) tiles), dim3(DH_WAVE), 0, stream, "k_mfma_f16", a, b, c, d) ? DH_EDEVICE : DH_OK;
}
static int dh_be_copy_kernel(const void* src, void* dst, size_t n_bytes, void* stream) {
    if (!n_bytes) return DH_OK;
    const size_t n16 = n_bytes / 16;
    if (!dst) {
        const unsigned rgrid = (unsigned) std::min<size_t>((n16 + 255) / 256, 8192);
        return dh_launch(k_read16, dim3(rgrid), dim3(256), 0, stream, "k_read16", (const dh_u4s*) src, n16) ? DH_EDEVICE : DH_OK;
    }
    const unsigned grid = (unsigned) std::min<size_t>((n16 + 255) / 256, 2048);      // 256 CUs x 8 resident workgroups of 256
    return dh_launch(k_copy16, dim3(grid), dim3(256), 0, stream, "k_copy16", (const dh_u4s*) src, (dh_u4s*) dst, n16) ? DH_EDEVICE : DH_OK;
}

static int dh_be_cz_gemm(const DhCzParams& P, void* stream) {
    if (!P.n_out) return DH_OK;
    return dh_launch(k_cz_gemm, dim3((P.n_out + DH_CZ_TM - 1) / DH_CZ_TM, P.ncols / (2u * DH_CZ_TNC)), dim3(256), 0, stream, "k_cz_gemm", P) ? DH_EDEVICE : DH_OK;
}
static int dh_be_cz_gemm_rat(const DhCzRatParams& R, void* stream) {
    if (!R.nslots) return DH_OK;
    return dh_launch(k_cz_gemm_rat, dim3((R.ph[0].count + DH_CZ_TM - 1) / DH_CZ_TM, R.g.ncols / (2u * DH_CZ_TNC), R.nslots), dim3(256), 0,
                     stream, "k_cz_gemm_rat", R) ? DH_EDEVICE : DH_OK;
}
static int dh_be_cz_fold(const DhCzFoldParams& F, void* stream) {
    if (!F.nrows) return DH_OK;
    return dh_launch(k_cz_fold, dim3((F.nrows + DH_CZ_FOLD_ROWS - 1) / DH_CZ_FOLD_ROWS, (F.kpad + DH_CZ_FOLD_LANES - 1) / DH_CZ_FOLD_LANES),
                     dim3(DH_CZ_FOLD_LANES), 0, stream, "k_cz_fold", F) ? DH_EDEVICE : DH_OK;
}
static int dh_be_cz_gemm_raster(const DhCzRasterParams& R, void* stream) {
    if (!R.g.n_out) return DH_OK;
    return dh_launch(k_cz_gemm_raster, dim3((R.g.n_out + DH_CZ_TM - 1) / DH_CZ_TM, R.g.ncols / (2u * DH_CZ_TNC)), dim3(256), 0,
                     stream, "k_cz_gemm_raster", R) ? DH_EDEVICE : DH_OK;
}

static int dh_be_monitor_open(const DhMonOpen& A, void* stream) {
    return dh_launch(k_monitor_open, dim3(grid_for(A.B, 256)), dim3(256), 0, stream, "k_monitor_open", A) ? DH_EDEVICE : DH_OK;
}
// (on the engine's stream, behind whatever the engine has in flight on streams of its own: HipBackend::ms)
static int dh_be_reset_channels(HipBackend& be, const DhResetChannels& R) {
    return dh_launch(k_reset_channels, dim3(R.B < 2048u ? R.B : 2048u), dim3(256), 0, be.ms(), "k_reset_channels", R);
}

#define DH_BACKEND HipBackend
#include "abi_impl.hpp"
