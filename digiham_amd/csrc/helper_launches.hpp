// helper_launches.hpp -- the batch FEC kernels and the stand-alone stages (CRC, whitening, voice filter, gain division, the
// f16 split) with their launches, written ONCE for the gfx950 library and the CPU test harness.
//
// A helper kernel is a __global__ wrapper that maps (blockIdx, threadIdx) to the items of a body from the core headers, and a
// launcher that states the grid that wrapper assumes, the empty-launch early-out and the stream.  Both are compiled by both
// builds and end in dh_launch (the launch vocabulary: dh_portable.hpp), so the index maps, grid clamps and grid-stride loops
// below are what the CPU tests execute.  The helper kernels of a handle stand in the same form at the end of the core header
// that owns their bodies (kernels_core.hpp, digest_core.hpp, channelizer_core.hpp, preroll_core.hpp, monitor_core.hpp,
// outpack_core.hpp, seam_probe_core.hpp);
// these here have no such header, and their launches need the two hooks below from the build that includes them.
//
// Not written once: the kernels whose device form needs barriers over LDS staging, matrix-core tiles or wave votes (k_chain,
// k_rrc_demod, k_rrc_tile: launch_plan.hpp; k_fe_fused, k_golay, the k_cz_gemm family, k_cz_fold, k_mfma_f16, k_copy16,
// k_read16, k_reset_channels, k_monitor_open, the probes).  They stay in engine.hip, their CPU restatements where they were.
//
// The including build provides, before this header:
//   int dh_fec_tables(const DhFecTables** out)                                   the FEC tables where the kernels can read them
//   int dh_be_golay(const DhFecTables*, int which, uint32_t* words, uint8_t* ok, size_t n, void* stream)       (k_golay)
#pragma once

#include "../../include/digiham_amd.h"
#include "kernels_core.hpp"
#include "seam_probe_core.hpp"
#include "fec_tables.hpp"
#include "rrc_taps.h"

#if !DH_DEVICE_BUILD
// ---- the CPU tier's side of the two hooks (engine.hip has the device's) --------------------------------------------------
static int dh_fec_tables(const DhFecTables** out) {
    static DhFecTables* T = [] { auto* t = new DhFecTables; dh::build_fec_tables(*t); return t; }();
    *out = T;
    return DH_OK;
}
// (k_golay stages its syndrome table in LDS behind a barrier: restated, one item at a time)
static int dh_be_golay(const DhFecTables* T, int which, uint32_t* words, uint8_t* ok, size_t n, void*) {
    for (size_t i = n; i-- > 0;) dh_fec_block_item(*T, which ? 6 : 5, words, ok, i);
    return DH_OK;
}
#endif

// ---------------------------------------------------------------------------------- batch FEC and the stand-alone stages
namespace {

__global__ void k_fec_block(const DhFecTables* T, int code, void* words, uint8_t* ok, size_t n) {
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        dh_fec_block_item(*T, code, words, ok, i);
}

__global__ void k_bptc(const DhFecTables* T, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        dh_bptc_item(*T, in, out, ok, i);
}

__global__ __launch_bounds__(DH_WAVE) void k_trellis(const uint8_t* in, size_t in_stride, int n_dibits, uint8_t* out, size_t out_stride,
                                                     uint8_t* metric, size_t n) {
    __shared__ DhDecShared S;
    dh_trellis_wave(in, in_stride, n_dibits, out, out_stride, metric, n, blockIdx.x, S);
}

__global__ void k_crc16(const uint8_t* in, size_t stride, int count, uint16_t* out, size_t n) {
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        dh_crc16_item(in, stride, count, out, i);
}

__global__ void k_whitening(const uint8_t* in, uint8_t* out, size_t stride, int n_bits, size_t n) {
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        dh_whitening_item(in, out, stride, n_bits, i);
}

__global__ void k_dvfilter(const int16_t* in, int16_t* out, float* state, size_t B, size_t stride, size_t n) {
    const size_t ch = blockIdx.x * (size_t) blockDim.x + threadIdx.x;
    if (ch < B) dh_dvfilter_channel(in + ch * stride, out + ch * stride, state + ch * 22, n);
}

__global__ void k_div_gain(const float* in, float* out, size_t n, double gain, double rgain) {
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        out[i] = dh_div_gain(in[i], gain, rgain);
}

__global__ void k_div_const(const float* in, float* out, size_t n, float d, float r) {
    for (size_t i = blockIdx.x * (size_t) blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        out[i] = dh_div_const(in[i], d, r);
}

__global__ void k_f16_split(const float* in, uint16_t* h1, uint16_t* h2, size_t n, float scale) {
    for (size_t i = (blockIdx.x * (size_t) blockDim.x + threadIdx.x) * 4; i < n; i += (size_t) gridDim.x * blockDim.x * 4) {
        dh_f4 v; v.x = in[i]; v.y = i + 1 < n ? in[i + 1] : 0.0f; v.z = i + 2 < n ? in[i + 2] : 0.0f; v.w = i + 3 < n ? in[i + 3] : 0.0f;
        dh_h4 a, b;
        dh_f16_split4(v, scale, a, b);
        uint16_t t1[4], t2[4];
        __builtin_memcpy(t1, &a, sizeof(t1)); __builtin_memcpy(t2, &b, sizeof(t2));      // the four halves as the kernels store them (one 8-byte vector)
        for (int j = 0; j < 4 && i + j < n; j++) { h1[i + j] = t1[j]; h2[i + j] = t2[j]; }
    }
}

}  // namespace

static int dh_be_fec_block(int code, void* words, uint8_t* ok, size_t n, void* stream) {
    if (!n) return DH_OK;
    if (!words || !ok) return DH_EINVAL;
    const DhFecTables* T = nullptr;
    int rc = dh_fec_tables(&T);
    if (rc) return rc;
    if (code == 5 || code == 6) return dh_be_golay(T, code == 6 ? 1 : 0, (uint32_t*) words, ok, n, stream);
    return dh_launch(k_fec_block, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_fec_block", T, code, words, ok, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_bptc(const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n, void* stream) {
    if (!n) return DH_OK;
    const DhFecTables* T = nullptr;
    int rc = dh_fec_tables(&T);
    if (rc) return rc;
    return dh_launch(k_bptc, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_bptc", T, in, out, ok, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_trellis(const uint8_t* in, size_t in_stride, int n_dibits, uint8_t* out, size_t out_stride, uint8_t* metric, size_t n, void* stream) {
    if (!n) return DH_OK;
    return dh_launch(k_trellis, dim3((unsigned) ((n + 3) / 4)), dh_workgroup(DH_WAVE), 0, stream, "k_trellis", in, in_stride, n_dibits, out, out_stride, metric, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_crc16(const uint8_t* in, size_t stride, int count, uint16_t* out, size_t n, void* stream) {
    if (!n) return DH_OK;
    return dh_launch(k_crc16, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_crc16", in, stride, count, out, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_whitening(const uint8_t* in, uint8_t* out, size_t stride, int n_bits, size_t n, void* stream) {
    if (!n) return DH_OK;
    return dh_launch(k_whitening, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_whitening", in, out, stride, n_bits, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_dvfilter(const int16_t* in, int16_t* out, float* state, size_t B, size_t stride, size_t n, void* stream) {
    if (!B) return DH_OK;
    return dh_launch(k_dvfilter, dim3((unsigned) ((B + 63) / 64)), dim3(64), 0, stream, "k_dvfilter", in, out, state, B, stride, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_div_const(const float* in, float* out, size_t n, unsigned divisor, void* stream) {
    if (!n) return DH_OK;
    const float d = (float) divisor;
    return dh_launch(k_div_const, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_div_const", in, out, n, d, 1.0f / d) ? DH_EDEVICE : DH_OK;
}
static int dh_be_div_gain(const float* in, float* out, size_t n, int narrow, void* stream) {
    if (!n) return DH_OK;
    const double gain = narrow ? DH_RRC_NARROW_GAIN : DH_RRC_WIDE_GAIN;
    return dh_launch(k_div_gain, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_div_gain", in, out, n, gain, 1.0 / gain) ? DH_EDEVICE : DH_OK;
}
static int dh_be_f16_split(const float* in, uint16_t* h1, uint16_t* h2, size_t n, float scale, void* stream) {
    if (!n) return DH_OK;
    return dh_launch(k_f16_split, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, stream, "k_f16_split", in, h1, h2, n, scale) ? DH_EDEVICE : DH_OK;
}
