// channelizer_core.hpp -- dh_channelizer: one wideband complex stream -> B narrow channel rows at input_rate / D, a bank of
// digital down-converters on the matrix cores.  Shared by the gfx950 kernels in engine.hip and by the CPU test harness (the
// host bodies and the host dh_be_cz_* backends at the end of this file).  This is THIS project's own stage, so the arithmetic
// below is its specification; tests/cz_restate.c restates it from this text alone.
//
//   Input     x[n], n = 0, 1, ... counted from create / reset, x[n < 0] = 0.  DH_CZ_CS16: interleaved int16 I / Q,
//             x = (I * 2^-15, Q * 2^-15) (exact).  DH_CZ_CF32: interleaved float32, taken as is.
//   Phasor    P(phi), phi a uint32 phase word (2^32 = one turn):  v = phi + 2^7 (mod 2^32), c = v >> 20, f = (v >> 8) & 4095,
//             C[c] = ((float) cos(c * (2 pi / 4096)), (float) sin(...)),  F[f] = ((float) cos(f * (2 pi / 2^24)), (float) sin(...))
//             (double angles, libm cos / sin, one rounding to float), P = (Cr Fr - Ci Fi, Cr Fi + Ci Fr), every product and
//             sum rounded to float in that order.  |P(phi) - e^(2 pi i phi / 2^32)| <= 1e-6 (tested; ~3e-7 in fact).
//   Channels  channel b has the uint32 increment u_b (offset / input_rate * 2^32, two's complement for negative offsets);
//             phi_b(n) = u_b * n mod 2^32 in integer arithmetic.
//   Filter    h[0..T-1] (the caller's table), zero-padded to T' = 16 ceil(T / 16) taps.  G_b[k] = (h[k] * Pr, h[k] * Pi),
//             P = P(phi_b(k)), one rounding each.
//   Output j  at input index n_j = j D + D - 1 (a push yields exactly the D-blocks it completes):
//             y = sum_k G_b[k] x[n_j - k] as two fused chains over k = 0 .. T'-1 in increasing k, starting from +0:
//               yr = fma(xi, -Gi[k], fma(xr, Gr[k], yr))      yi = fma(xi, Gr[k], fma(xr, Gi[k], yi))
//             (x = x[n_j - k]; one chain per component, no split accumulators: v_mfma_f32_16x16x4_f32 is bit for bit this
//             k-ordered fmaf chain, and the K order of the GEMM below is exactly k, then re before im)
//             z_b[j] = P(-phi_b(n_j)) (x) y:  zr = (pr yr) - (pi yi),  zi = (pr yi) + (pi yr)   (products rounded, then the sum)
//   IQ_F32    row b = z_b[j] interleaved (re, im).
//   FM        w = z[j] conj(z[j-1]): wr = (zr pr') + (zi pi'),  wi = (zi pr') - (zr pi')  with z[j-1] = (pr', pi'), z[-1] = 0;
//             out = dh_fe_atan2f_over_pi(wi, wr) -- the arctangent of the receiver front-end (frontend_core.hpp); (0, 0) -> 0.
//   dcblock   (FM only) y = (x - x_prev) + 0.995f y_prev, the operations of dh_frontend_channel; x_prev = y_prev = 0 at the start.
//   Retune    replaces u_b from the next push on, recomputes G_b and zeroes channel b's z[j-1], x_prev and y_prev; the input
//             history and every other channel are untouched.
//   Denormals are kept everywhere: the host rounds taps with IEEE floats, and the kernels run in hipcc's default f32 mode
//             (float_denorm_mode_32 = 3: VALU and MFMA A / B keep subnormals, MFMA C / D never flush), which is what the
//             host's IEEE fmaf does.  A test pushes input whose products and sums are subnormal and compares device, CPU
//             emulation and the restatement byte for byte.
//
// ---- Rational rates (interpolation L > 1): output rate = input_rate L / M, M = decimation.  The specification;
// tests/cz_rational_restate.c restates it from this text alone.  Everything not mentioned is as above (input formats, P(phi),
// u_b, FM, dcblock, the power blocks / gate / counts in terms of the output index j, denormals, reset). ----
//   Ratio     1 <= L <= 64, 1 <= M <= 1024, L <= M, gcd(L, M) = 1.  L = 1 is the channelizer above, bit for bit and launch
//             for launch.
//   Prototype h[0..T) is the caller's real low-pass at the virtual rate L input_rate, 1 <= T <= 16384 L.
//   Output j  sits at the virtual index v_j = j M + M - 1: input index n_j = floor(v_j / L), tap phase r_j = v_j mod L.  With
//             p = j mod L both depend on p only: r_p = (p M + M - 1) mod L, n_j = floor(j / L) M + floor((p M + M - 1) / L).
//             Phase p's taps are h_p[k] = h[r_p + k L] for r_p + k L < T, zero-padded to the common
//             T' = 16 ceil(ceil(T / L) / 16); a phase with r_p >= T is all zeros.
//   Rotated   G_{b,p}[k] = (h_p[k] * Pr, h_p[k] * Pi), P = P(phi_b(k)), phi_b(n) = u_b n mod 2^32: n counts INPUT samples.
//   Chains    the two fused chains above over k = 0 .. T'-1 in increasing k, from +0, with x = x[n_j - k] and G = G_{b,p}.
//             The zero-stuffed virtual samples are skipped, not added (fma(0, g, y) can turn a -0 into +0); the padded
//             taps are added, as above.
//   Rotation  z_b[j] = P(-phi_b(n_j)) (x) y with n_j mod 2^32.
//   Complete  output j completes when x[n_j] has been pushed: after N input samples in total exactly floor(L N / M) outputs
//             exist, a push yields floor(L (N0 + n_in) / M) - floor(L N0 / M), and the results do not depend on how the
//             stream is cut into pushes.  The history is T' - 1 input samples.
//   Retune    of channel b recomputes G_{b,p} for all L phases and otherwise does what it does above.
//   Work      the GEMM's B operand is L banks [2 T'][ncols].  A push's outputs are split by phase: slot s < min(L, n_out)
//             holds the rows s, s + L, s + 2 L, ... of the push (phase p = (j0 + s) mod L), a decimate-by-M converter bank
//             of its own: DhCzPhase has its row count, the window index of its first row and that row's n_j.  A GEMM
//             workgroup tile belongs to one slot (k_cz_gemm_rat; host body dh_cz_output_rat).
//
// ---- Uniform raster (raster = K != 0): every channel on a multiple of input_rate / K, so all channels share ONE polyphase
// fold of the prototype and differ only in a K-point DFT.  The specification; tests/cz_raster_restate.c restates it from this
// text alone.  Everything not mentioned is as at the top (input formats, P(phi), FM, dcblock, the power blocks / gate /
// counts in terms of the output index j, denormals kept, reset). ----
//   Raster    K = raster, 2 <= K <= 16384.  Channel b sits at bins[b] * input_rate / K; c_b = bins[b] mod K reduced into
//             [0, K).  Any subset of bins, in any order, with duplicates; B <= 65536 as above.
//   Phase     for 0 <= q < K:  Phi(q) = (uint32) ((((uint64) q << 32) + K / 2) / K)   (integer division).  Phasors are
//             P(Phi(q)) of the tables above.  A phase is always formed as (c * m) mod K in integer arithmetic and then
//             mapped through Phi, never by multiplying a rounded increment: the fold relies on exact K-periodicity.
//   Prototype h[0..T) zero-padded to P K, P = ceil(T / K); 1 <= T <= 64 K and T <= 2^20.  The history is H = P K - 1 input
//             samples, x[n < 0] = 0.
//   Output j  at n_j = j D + D - 1, exactly as at the top; a push yields the D-blocks it completes and the results do not
//             depend on how the stream is cut into pushes.
//   Fold      for r = 0 .. K-1 two chains over p = 0 .. P-1 in increasing p from +0, all P terms added, the padded ones too:
//               vr = fma(h[r + p K], xr, vr)      vi = fma(h[r + p K], xi, vi)      with x = x[n_j - r - p K]
//             v is zero-padded to K' = 16 ceil(K / 16).
//   DFT       G_b[r] = P(Phi((c_b r) mod K)) for r < K and 0 for K <= r < K'.  The two chains of the top over r = 0 .. K'-1
//             from +0, the padded terms added:
//               yr = fma(vi, -Gi, fma(vr, Gr, yr))      yi = fma(vi, Gr, fma(vr, Gi, yi))
//             -- the k-ordered chain that v_mfma_f32_16x16x4_f32 computes, with v in the place of x and K' in that of T'.
//   Rotation  z = P(Phi((K - (c_b (n_j mod K)) mod K) mod K)) (x) y, products rounded, then the sum, as at the top.  n_j is
//             taken from the 64-bit stream position, not modulo 2^32.
//   Retune    of channel b gives it a new bin (dh_channelizer_retune's value read as a two's-complement int32) and
//             recomputes its column of G; it zeroes what a retune zeroes at the top; the input history is untouched.
//   Not with  interpolation > 1: DH_EINVAL.
//   Work      (1) the window with H = P K - 1; then per slab of at most DH_CZ_FOLD_SLAB_BYTES of folded rows (a multiple of
//             the GEMM's 128-row tile): (2a) dh_cz_fold_item, one (output instant, r) per lane -- row i of the slab keeps
//             v[r] at fold[i K' + K' - 1 - r], so that (2b) the GEMM tile of the top, reading "the window" at
//             (K' - 1) + i K' - k against the B operand [2 K'][ncols] built from G, computes the DFT chains unchanged
//             (k_cz_gemm_raster; host body dh_cz_output_raster) and dh_cz_emit_raster rotates.  FM, tail and power then
//             run once over the push.
//
// ---- Block power and the squelch gate (optional; dh_channelizer_power_enable).  The specification; tests/cz_power_restate.c
// restates it from this text alone. ----
//   Blocks    enabled once per channelizer with a block length L, 1 <= L <= 65536 outputs (L = 480: 10 ms at 48 kS/s).  j is
//             the global output index since create / reset (the j of n_j above).  Block m of a channel covers the outputs
//             j in [m L, (m + 1) L).  Push boundaries do not move block boundaries.
//   q         z_b[j] is the rotated output above -- the same value in both output modes: what IQ_F32 stores and what FM
//             feeds to the discriminator.  q = (zr zr) + (zi zi): both products rounded, then the sum.
//   S         starts at +0 at the beginning of every block; S = S + q[j] in increasing j: ONE chain, no split accumulators,
//             no tree.  When output (m + 1) L - 1 has been added: power[b][m] = S inv, inv = (float) (1.0 / (double) L)
//             computed on the host, the multiply rounded once.  A push that ends inside a block leaves S in the channel's
//             state and the next push continues the same chain; the position inside the block follows from j alone.
//             Infinities and NaN propagate as IEEE arithmetic has them.
//   Gate      per channel (open in {0, 1}, quiet: an unsigned counter), both 0 at create / reset.  Parameters: two finite
//             floats open_level >= close_level >= 0 and hang <= 65535 blocks.  For each completed block in order, p its power:
//               closed:  if (p >= open_level) { open = 1; quiet = 0; }
//               open:    if (p >= close_level) quiet = 0; else if (++quiet > hang) { open = 0; quiet = 0; }
//               gate[b][m] = open after the update.
//             A NaN power never opens a gate and counts as quiet; hang = 0 closes on the first quiet block;
//             open_level = close_level = 0 is "power only": every channel opens with its first block that is not NaN.
//   Counts    for a push that completes n_out outputs: counts[b] = n_out if channel b's gate was open when the push began
//             or if any gate byte this push wrote for b is 1, else 0; a push with n_out = 0 writes zeros.  That is the
//             d_counts argument of dh_engine_push_ragged.  Gating acts on whole pushes: the push in which a gate opens
//             passes completely (the pre-roll), and so does the push in which it closes.  A transmission that starts
//             inside the last, unfinished block of a push loses at most L - 1 outputs (that push is not passed; the block
//             completes in the next one, which is).
//   Retune    of channel b zeroes its S, open and quiet together with the state it zeroes anyway.  The block in progress
//             keeps its index; its value is the chain over the outputs after the retune, times inv.
//   Reset     zeroes all of it; the power configuration stays.  Enabling is only legal while no sample has been pushed
//             since create / reset (block alignment would be ambiguous otherwise).  Levels and hang may change between
//             any two pushes; the state is kept.
//   Off       a channelizer on which power was never enabled allocates nothing for it and launches exactly the kernels above.
// Work per push with power on, after the steps below: (5) dh_cz_power_segment, one lane per (channel, block segment of this
// push) -- a segment is the continuation of the carried block, a whole block, or the unfinished tail; the lane adds its
// segment in order and writes either a power value or the carried S; (6) dh_cz_gate_channel, one channel per lane: the
// recurrence over the blocks this push completed, the gate bytes, counts[b] and the state.
//
// ---- Frequency-error blocks (optional; d_ferr of dh_channelizer_power_enable).  The specification; tests/cz_ferr_restate.c
// restates it from this text alone.  Everything not mentioned is as for block power: blocks are indexed by the global output
// index j since create / reset, so push boundaries do not move block boundaries. ----
//   ABI       dh_channelizer_power_config ends in float* d_ferr ([n_channels][stride], the caller's device memory, like
//             d_power).  struct_size = DH_CHANNELIZER_POWER_CONFIG_V1_SIZE (the struct up to d_ferr): the field is not read,
//             whatever bytes follow, and the feature is off.  struct_size = the whole struct: d_ferr = NULL is off.  Every other
//             struct_size is DH_EINVAL.  Off means off: nothing more is allocated, launched or written than without the field.
//   w         for output j of channel b with p = z_b[j-1]:  a = zr pr, c = zi pi, d = zi pr, e = zr pi;  wr = a + c,
//             wi = d - e -- what dh_cz_fm_item computes, every product and sum rounded.  z is the rotated output, the same value
//             in both output modes and in all three kinds of bank; z[-1] = 0 after create and reset.
//   Chains    Ar and Ai start at +0 at the beginning of every block; Ar = Ar + wr[j], Ai = Ai + wi[j] in increasing j: ONE
//             chain each, no split accumulators, no tree.  A push that ends inside a block leaves (Ar, Ai) and z[j] in the
//             channel's state and the next push continues the same chains.
//   Value     when output (m + 1) L - 1 has been added: ferr[b][m] = dh_fe_atan2f_over_pi(Ai, Ar) (frontend_core.hpp);
//             (0, 0) -> 0, infinities and NaN propagate as its operations have them.  The unit is half the output rate:
//             Hz = ferr * output_rate / 2.  Column i of d_ferr after a push is block first_block + i of
//             dh_channelizer_power_last, as for d_power.  It is the |z|^2-weighted mean frequency of the block: strong
//             samples dominate, and an empty channel gives noise around 0.
//   Retune    of channel b zeroes its Ar, Ai and carried z.  The block in progress keeps its index; its value is the chain
//             over the outputs after the retune.  Reset zeroes everything and keeps the configuration.
//   Carried z the stage keeps its own previous z in both modes (in IQ mode nothing writes words 0 and 1 of the FM state, and
//             in FM mode dh_cz_tail_channel has overwritten them with this push's last z before this stage runs).
//   Power     power, gate, counts, the rows and dh_channelizer_power_last are byte for byte what they are without d_ferr.
// Work per push with d_ferr set and outputs completed, after (5) and (6): (7) dh_cz_ferr_segment, one lane per (channel, block
// segment of this push) with dh_cz_power_segment's item map and loads.  The state is [B][2][4] floats: two copies of
// (Ar, Ai, z re, z im) per channel, so that DeviceBuffers::zero_row clears exactly channel b's eight words; a push
// reads one copy and writes the other, the host alternating them by the parity of the pushes that launched the stage: the
// lane of segment 0 reads the carried words in the same launch in which the lane of the last segment writes the new ones,
// and nothing orders the two.  A push with no outputs launches nothing and keeps the parity.
//
// Work per push (host code in abi_impl.hpp): (1) dh_cz_window_item -- the window [H = T'-1 history samples ++ the new ones]
// as complex floats; (2) the GEMM + rotation, tiled over 128 output instants x 64 channels (k_cz_gemm; host body
// dh_cz_output); FM mode then (3) dh_cz_fm_item, one output per lane, and (4) dh_cz_tail_channel, one channel per lane:
// the DC blocker's recurrence and the carried z[j-1].  On a uniform raster (2) is the fold and the DFT, slab by slab (above).
#pragma once

#include <math.h>

#include "../../include/digiham_amd.h"
#include "frontend_core.hpp"

#define DH_CZ_TAP_STEP 16         // T' = a multiple of the K extent of one LDS chunk of the GEMM (16 taps = 32 real K)
#define DH_CZ_TM 128              // output instants per GEMM workgroup tile
#define DH_CZ_TNC 64              // channels per GEMM workgroup tile (128 real columns)
#define DH_CZ_TBITS 12            // the two phasor tables: 4096 entries each
#define DH_CZ_STATE_WORDS 4       // per channel: z[j-1] (re, im), x_prev, y_prev of the DC blocker
#define DH_CZ_PSTATE_WORDS 4      // per channel, only with power enabled (an array of its own): S (float bits), open, quiet, S of this push
#define DH_CZ_FSTATE_WORDS 8      // per channel, only with d_ferr set (an array of its own): two copies of (Ar, Ai, z[j-1] re, im)
#define DH_CZ_MAX_L 64            // interpolation: phases of a rational rate
#define DH_CZ_MAX_RASTER 16384    // raster: K, the steps per input rate
#define DH_CZ_MAX_FOLD_P 64       // raster: T <= 64 K ...
#define DH_CZ_MAX_RASTER_TAPS (1u << 20)       // ... and T <= 2^20
#define DH_CZ_FOLD_SLAB_BYTES (32u << 20)      // raster: the fold buffer, whatever max_input is
#define DH_CZ_FOLD_ROWS 16        // output instants per k_cz_fold workgroup (one accumulator pair each, per lane)
#define DH_CZ_FOLD_LANES 256      // ... and its r extent, one r per lane
#define DH_CZ_FOLD_LDS 6144       // complex samples of input span it stages at a time (48 KB)

// Column of the real GEMM for channel b, component c (0: the real output, 1: the imaginary one).  Sixteen channels' real
// columns, then their sixteen imaginary ones: a 16 x 16 MFMA tile holds one component of sixteen channels, and the lane
// that holds a channel's real part in tile 2t holds its imaginary part in tile 2t + 1 (no exchange between lanes).
DH_HD uint32_t dh_cz_col(uint32_t b, uint32_t c) { return 32u * (b >> 4) + 16u * c + (b & 15u); }
DH_HD uint32_t dh_cz_ncols(uint32_t B) { return 2u * DH_CZ_TNC * ((B + DH_CZ_TNC - 1) / DH_CZ_TNC); }
DH_HD uint32_t dh_cz_tpad(uint32_t T) { return DH_CZ_TAP_STEP * ((T + DH_CZ_TAP_STEP - 1) / DH_CZ_TAP_STEP); }

DH_HD void dh_cz_phasor(uint32_t phi, const float* coarse, const float* fine, float& pr, float& pi) {
    const uint32_t v = phi + 128u, c = v >> 20, f = (v >> 8) & 4095u;
    const float cr = coarse[2 * c], ci = coarse[2 * c + 1], fr = fine[2 * f], fi = fine[2 * f + 1];
    const float a = cr * fr, b = ci * fi, d = cr * fi, e = ci * fr;
    pr = a - b; pi = d + e;
}

struct DhCzParams {
    const float* win;             // [H + n_in][2] window: x[N0 - H .. N0 + n_in) of this push, H = T' - 1
    const float* bmat;            // [2 T'][ncols] the GEMM's B operand: row 2k (x real part) / 2k + 1 (x imaginary part)
    const float* coarse;          // [4096][2]
    const float* fine;            // [4096][2]
    const uint32_t* inc;          // [B] u_b
    float* out; size_t out_stride;        // output rows [B][out_stride] (complex pairs in IQ_F32 mode, floats in FM mode)
    float* zbuf;                  // FM mode: z of this push, [n_out][B][2]
    uint64_t j0;                  // index of the push's first output
    uint32_t off0;                // window index of x[n_{j0}] minus H: D - 1 - (N0 mod D)
    uint32_t D, tpad, B, ncols, n_out;
    int fm;                       // 0: rotated z to the output rows, 1: to zbuf
};

// the rotation and the store of output `row` of channel b at input index nj (mod 2^32), y = the two chains.  (The rotation and
// the store stand here and in dh_cz_emit_raster: behind one function of any shape tried, both GEMM kernels compile to
// other instructions.)
DH_HD void dh_cz_emit_at(const DhCzParams& P, uint32_t row, uint32_t b, uint32_t nj, float yr, float yi) {
    float pr, pi;
    dh_cz_phasor(0u - P.inc[b] * nj, P.coarse, P.fine, pr, pi);
    const float a = pr * yr, c = pi * yi, d = pr * yi, e = pi * yr;
    const float zr = a - c, zi = d + e;
    float* q = P.fm ? P.zbuf + 2 * ((size_t) row * P.B + b) : P.out + 2 * ((size_t) b * P.out_stride + row);
    q[0] = zr; q[1] = zi;
}
DH_HD void dh_cz_emit(const DhCzParams& P, uint32_t row, uint32_t b, float yr, float yi) {
    dh_cz_emit_at(P, row, b, (uint32_t) ((P.j0 + row) * (uint64_t) P.D + (P.D - 1u)), yr, yi);         // n_j mod 2^32
}

// The two chains of one output in the MFMA's K order (row 2k, then 2k + 1, k = 0 .. T'-1): bmat the B operand (bank),
// base the window index of x[n_j]
DH_HD void dh_cz_chains(const DhCzParams& P, const float* bmat, uint32_t base, uint32_t b, float& yr, float& yi) {
    const float* cr = bmat + dh_cz_col(b, 0), * ci = bmat + dh_cz_col(b, 1);
    yr = 0.0f; yi = 0.0f;
    for (uint32_t k = 0; k < P.tpad; k++) {
        const float xr = P.win[2 * (size_t) (base - k)], xi = P.win[2 * (size_t) (base - k) + 1];
        const size_t r0 = (size_t) (2 * k) * P.ncols, r1 = r0 + P.ncols;
        yr = __builtin_fmaf(xr, cr[r0], yr); yr = __builtin_fmaf(xi, cr[r1], yr);
        yi = __builtin_fmaf(xr, ci[r0], yi); yi = __builtin_fmaf(xi, ci[r1], yi);
    }
}

// Host body of the GEMM
DH_HD void dh_cz_output(const DhCzParams& P, uint32_t row, uint32_t b) {
    float yr, yi;
    dh_cz_chains(P, P.bmat, P.off0 + row * P.D + (P.tpad - 1u), b, yr, yi);
    dh_cz_emit(P, row, b, yr, yi);
}

// ---- rational rates: the slots of a push (the header comment) -------------------------------------------------------------
struct DhCzPhase {
    uint32_t count;               // outputs of this slot in the push: rows s + L i, i < count
    uint32_t wbase;               // window index of x[n_j] of its first row (row i: wbase + i M)
    uint32_t nj0;                 // that n_j mod 2^32 (row i: nj0 + i M)
    uint32_t bank;                // p = (j0 + s) mod L: the B operand is bmat + p * 2 T' ncols
};
struct DhCzRatParams {
    DhCzParams g;                 // as for L = 1 (D = M; j0 and off0 unused)
    uint32_t L, nslots;           // nslots = min(L, n_out)
    DhCzPhase ph[DH_CZ_MAX_L];
};
DH_HD uint32_t dh_cz_tpad_rat(uint32_t T, uint32_t L) { return dh_cz_tpad((T + L - 1u) / L); }
DH_HD const float* dh_cz_bank(const DhCzParams& P, uint32_t p) { return P.bmat + (size_t) p * 2u * P.tpad * P.ncols; }

// the slots of the push of n_in samples after N0: fills R.g.n_out, R.nslots and R.ph (host arithmetic)
inline void dh_cz_plan_rat(DhCzRatParams& R, uint64_t N0, uint64_t n_in) {
    const uint64_t L = R.L, M = R.g.D, j0 = L * N0 / M, no = L * (N0 + n_in) / M - j0;
    R.g.n_out = (uint32_t) no;
    R.nslots = (uint32_t) (no < L ? no : L);
    for (uint32_t s = 0; s < R.nslots; s++) {
        const uint64_t j = j0 + s, p = j % L, nj = j / L * M + (p * M + M - 1u) / L;
        R.ph[s].count = (uint32_t) ((no - s + L - 1u) / L);
        R.ph[s].wbase = (uint32_t) (R.g.tpad - 1u + (nj - N0));
        R.ph[s].nj0 = (uint32_t) nj;
        R.ph[s].bank = (uint32_t) p;
    }
}

// Host body of the rational GEMM: row i of slot s
DH_HD void dh_cz_output_rat(const DhCzRatParams& R, uint32_t s, uint32_t i, uint32_t b) {
    const DhCzPhase& ph = R.ph[s];
    float yr, yi;
    dh_cz_chains(R.g, dh_cz_bank(R.g, ph.bank), ph.wbase + i * R.g.D, b, yr, yi);
    dh_cz_emit_at(R.g, s + R.L * i, b, ph.nj0 + i * R.g.D, yr, yi);
}

// ---- uniform raster: the fold, the DFT's B operand, the rotation (the header comment) -------------------------------------
DH_HD uint32_t dh_cz_raster_phi(uint32_t q, uint32_t K) { return (uint32_t) ((((uint64_t) q << 32) + K / 2u) / K); }
DH_HD uint32_t dh_cz_raster_bin(int32_t bin, uint32_t K) { const int32_t m = bin % (int32_t) K; return (uint32_t) (m < 0 ? m + (int32_t) K : m); }
// rows of folded v one slab holds: a multiple of the GEMM's row tile, at least one tile (K' = 16384: 16 MiB)
DH_HD uint32_t dh_cz_fold_slab_rows(uint32_t kpad) {
    const uint32_t rows = DH_CZ_FOLD_SLAB_BYTES / (8u * kpad) / DH_CZ_TM * DH_CZ_TM;
    return rows ? rows : (uint32_t) DH_CZ_TM;
}

struct DhCzFoldParams {
    const float* win;             // [H + n_in][2], H = P K - 1
    const float* h;               // [P K] the prototype, zero-padded
    float* fold;                  // [slab rows][K'][2]: row i's v[r] at i K' + K' - 1 - r
    uint32_t K, kpad, P, D;
    uint32_t wj0;                 // window index of x[n_j] of the slab's first row
    uint32_t nrows;               // rows of this slab
    uint32_t win_n;               // H + n_in
};
// the two fold chains of (row, r) of a slab, r < K'; the padding K <= r < K' is written as zeros
DH_HD void dh_cz_fold_item(const DhCzFoldParams& F, uint32_t row, uint32_t r) {
    float vr = 0.0f, vi = 0.0f;
    if (r < F.K) {
        const float* x = F.win + 2 * ((size_t) F.wj0 + (size_t) row * F.D - r);
        for (uint32_t p = 0; p < F.P; p++, x -= 2 * (size_t) F.K) {
            const float hv = F.h[r + (size_t) p * F.K];
            vr = __builtin_fmaf(hv, x[0], vr); vi = __builtin_fmaf(hv, x[1], vi);
        }
    }
    float* q = F.fold + 2 * ((size_t) row * F.kpad + (F.kpad - 1u - r));
    q[0] = vr; q[1] = vi;
}

struct DhCzRasterParams {
    DhCzParams g;                 // win = the fold buffer, tpad = K', n_out = the slab's rows; inc, j0 and off0 unused
    const uint32_t* cbin;         // [B] c_b
    const uint32_t* phi;          // [K] Phi(q)
    uint32_t K;
    uint32_t row0;                // push row of the slab's first row
    uint32_t m0;                  // n_j mod K of the PUSH's first row (host, from the 64-bit position)
};
// the rotation and the store of slab row i of channel b
DH_HD void dh_cz_emit_raster(const DhCzRasterParams& R, uint32_t i, uint32_t b, float yr, float yi) {
    const uint32_t row = R.row0 + i, m = (R.m0 + row * R.g.D) % R.K, t = (R.cbin[b] * m) % R.K;
    float pr, pi;
    dh_cz_phasor(R.phi[t ? R.K - t : 0u], R.g.coarse, R.g.fine, pr, pi);
    const float a = pr * yr, c = pi * yi, d = pr * yi, e = pi * yr;
    const float zr = a - c, zi = d + e;
    float* q = R.g.fm ? R.g.zbuf + 2 * ((size_t) row * R.g.B + b) : R.g.out + 2 * ((size_t) b * R.g.out_stride + row);
    q[0] = zr; q[1] = zi;
}
// Host body of the raster GEMM: slab row i
DH_HD void dh_cz_output_raster(const DhCzRasterParams& R, uint32_t i, uint32_t b) {
    float yr, yi;
    dh_cz_chains(R.g, R.g.bmat, i * R.g.tpad + (R.g.tpad - 1u), b, yr, yi);
    dh_cz_emit_raster(R, i, b, yr, yi);
}

// element e of this push's window: the last H samples of the previous window, then the new samples converted
DH_HD void dh_cz_window_item(float* cur, const float* prev, uint32_t prev_n, const void* in, int cf32, uint32_t H, size_t e) {
    float re, im;
    if (e < H) { re = prev[2 * (prev_n + e)]; im = prev[2 * (prev_n + e) + 1]; }
    else if (cf32) { const float* s = (const float*) in + 2 * (e - H); re = s[0]; im = s[1]; }
    else { const int16_t* s = (const int16_t*) in + 2 * (e - H); re = (float) s[0] * 0.000030517578125f; im = (float) s[1] * 0.000030517578125f; }
    cur[2 * e] = re; cur[2 * e + 1] = im;
}

// FM discriminator of output j of channel b (FM mode): zbuf [n_out][B][2], z[j-1] of j = 0 from the channel's state
DH_HD void dh_cz_fm_item(const float* zbuf, const float* state, float* out, size_t out_stride, uint32_t B, uint32_t b, uint32_t j) {
    const float* z = zbuf + 2 * ((size_t) j * B + b);
    const float* p = j ? z - 2 * (size_t) B : state + (size_t) b * DH_CZ_STATE_WORDS;
    const float zr = z[0], zi = z[1], pr = p[0], pi = p[1];
    const float a = zr * pr, c = zi * pi, d = zi * pr, e = zr * pi;
    const float wr = a + c, wi = d - e;
    out[(size_t) b * out_stride + j] = dh_fe_atan2f_over_pi(wi, wr);
}

// one step of the DC blocker: y for the input x after (x_prev, y_prev)
DH_HD float dh_cz_dc_step(float x, float xp, float yp) { const float d = x - xp; const float f = 0.995f * yp; return d + f; }

// the serial part of FM mode, one channel: DC blocker over the channel's n_out outputs in place, then the carried state
DH_HD void dh_cz_tail_channel(const float* zbuf, float* state, float* out, size_t out_stride, uint32_t B, uint32_t n_out, int dcblock, uint32_t b) {
    float* st = state + (size_t) b * DH_CZ_STATE_WORDS;
    float* row = out + (size_t) b * out_stride;
    if (dcblock) {
        float xp = st[2], yp = st[3];
        uint32_t j = 0;
        for (; j + 8 <= n_out; j += 8) {          // eight loads in flight ahead of the recurrence
            float v[8];
            for (int e = 0; e < 8; e++) v[e] = row[j + e];
            for (int e = 0; e < 8; e++) { const float y = dh_cz_dc_step(v[e], xp, yp); xp = v[e]; yp = y; v[e] = y; }
            for (int e = 0; e < 8; e++) row[j + e] = v[e];
        }
        for (; j < n_out; j++) { const float x = row[j]; const float y = dh_cz_dc_step(x, xp, yp); xp = x; yp = y; row[j] = y; }
        st[2] = xp; st[3] = yp;
    }
    if (n_out) { const float* z = zbuf + 2 * ((size_t) (n_out - 1) * B + b); st[0] = z[0]; st[1] = z[1]; }
}

// ---- block power and gate (the specification in the header comment) ------------------------------------------------------
struct alignas(8) DhCzF2 { float v[2]; };               // one output: an 8-byte load
struct alignas(16) DhCzF4 { float v[4]; };              // two outputs of an IQ row: a 16-byte load

struct DhCzPowerParams {
    const float* z;               // FM mode: zbuf [n_out][B][2]; IQ mode: the caller's output rows [B][z_stride][2]
    size_t z_stride;
    uint32_t* pstate;             // [B][DH_CZ_PSTATE_WORDS]
    float* power; uint8_t* gate;  // [B][stride]: column i = block first + i of this push
    uint32_t* counts;             // [B]
    size_t stride;
    uint32_t pos0;                // j0 mod L: outputs the block in progress already holds
    uint32_t n_out, n_blocks, nseg, B, L;
    int fm;
    float inv, open_level, close_level;
    uint32_t hang;
};

DH_HD float dh_cz_q(float zr, float zi) { const float a = zr * zr, c = zi * zi; return a + c; }
DH_HD float dh_cz_bits_f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
DH_HD uint32_t dh_cz_f_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// segment s of channel b: the outputs of block (j0 / L + s) that this push holds, rows [r0, r1) of the push
DH_HD void dh_cz_power_segment(const DhCzPowerParams& P, uint32_t b, uint32_t s) {
    const uint32_t end = (s + 1u) * P.L - P.pos0;                       // row after the block's last output
    const uint32_t r0 = s ? s * P.L - P.pos0 : 0u, r1 = dh_min(end, P.n_out);
    uint32_t* st = P.pstate + (size_t) b * DH_CZ_PSTATE_WORDS;
    float S = (s == 0u && P.pos0) ? dh_cz_bits_f(st[0]) : 0.0f;
    uint32_t r = r0;
    if (P.fm) {                   // lanes on consecutive channels: 8-byte loads, 512 contiguous bytes per wave instruction
        const size_t step = 2 * (size_t) P.B;
        const float* p = P.z + 2 * ((size_t) r0 * P.B + b);
        for (; r + 8 <= r1; r += 8, p += 8 * step) {                    // eight loads in flight ahead of the chain
            DhCzF2 v[8];
            for (int e = 0; e < 8; e++) v[e] = *(const DhCzF2*) (p + e * step);
            for (int e = 0; e < 8; e++) S = S + dh_cz_q(v[e].v[0], v[e].v[1]);
        }
        for (; r < r1; r++, p += step) { const DhCzF2 v = *(const DhCzF2*) p; S = S + dh_cz_q(v.v[0], v.v[1]); }
    } else {                      // each lane along its own contiguous segment of its row
        const float* p = P.z + 2 * ((size_t) b * P.z_stride + r0);
        if (((uintptr_t) p & 7u) == 0) {
            if (((uintptr_t) p & 8u) && r < r1) { const DhCzF2 v = *(const DhCzF2*) p; S = S + dh_cz_q(v.v[0], v.v[1]); r++; p += 2; }
            for (; r + 16 <= r1; r += 16, p += 32) {                    // eight 16-byte loads in flight: one 128-byte line
                DhCzF4 v[8];
                for (int e = 0; e < 8; e++) v[e] = *(const DhCzF4*) (p + 4 * e);
                for (int e = 0; e < 8; e++) { S = S + dh_cz_q(v[e].v[0], v[e].v[1]); S = S + dh_cz_q(v[e].v[2], v[e].v[3]); }
            }
            for (; r + 2 <= r1; r += 2, p += 4) { const DhCzF4 v = *(const DhCzF4*) p; S = S + dh_cz_q(v.v[0], v.v[1]); S = S + dh_cz_q(v.v[2], v.v[3]); }
        }
        for (; r < r1; r++, p += 2) S = S + dh_cz_q(p[0], p[1]);        // the last output, or rows that are only 4-byte aligned
    }
    const bool complete = end <= P.n_out;
    if (complete) { const float pw = S * P.inv; P.power[(size_t) b * P.stride + s] = pw; }
    // The carried S goes to word 3, not to word 0: the lane of segment 0 reads word 0 in this same launch, and nothing orders
    // the two lanes.  dh_cz_gate_channel, which runs after every lane of this launch, moves it to word 0.
    if (s + 1u == P.nseg) st[3] = complete ? 0u : dh_cz_f_bits(S);
}

// the gate recurrence of channel b over the n_blocks blocks this push completed; counts[b]; the carried (open, quiet).  (The
// step stands twice, in the unrolled eight and in the tail: behind one function or lambda k_cz_gate compiles to other
// instructions.)
DH_HD void dh_cz_gate_channel(const DhCzPowerParams& P, uint32_t b) {
    uint32_t* st = P.pstate + (size_t) b * DH_CZ_PSTATE_WORDS;
    uint32_t open = st[1], quiet = st[2], any = open;
    const float* pw = P.power + (size_t) b * P.stride;
    uint8_t* g = P.gate + (size_t) b * P.stride;
    uint32_t i = 0;
    for (; i + 8 <= P.n_blocks; i += 8) {                               // eight loads in flight ahead of the recurrence
        float v[8]; uint8_t o[8];
        for (int e = 0; e < 8; e++) v[e] = pw[i + e];
        for (int e = 0; e < 8; e++) {
            if (!open) { if (v[e] >= P.open_level) { open = 1u; quiet = 0u; } }
            else if (v[e] >= P.close_level) quiet = 0u;
            else if (++quiet > P.hang) { open = 0u; quiet = 0u; }
            o[e] = (uint8_t) open; any |= open;
        }
        for (int e = 0; e < 8; e++) g[i + e] = o[e];
    }
    for (; i < P.n_blocks; i++) {
        const float p = pw[i];
        if (!open) { if (p >= P.open_level) { open = 1u; quiet = 0u; } }
        else if (p >= P.close_level) quiet = 0u;
        else if (++quiet > P.hang) { open = 0u; quiet = 0u; }
        g[i] = (uint8_t) open; any |= open;
    }
    st[1] = open; st[2] = quiet;
    if (P.nseg) st[0] = st[3];                                          // the carried S of this push (dh_cz_power_segment)
    P.counts[b] = any ? P.n_out : 0u;
}

// ---- frequency-error blocks (the specification in the header comment) ---------------------------------------------------
struct DhCzFerrParams {
    const float* z;               // as in DhCzPowerParams
    size_t z_stride;
    const float* fin;             // the state copy this push reads: channel b's (Ar, Ai, z[j-1] re, im) at fin + b DH_CZ_FSTATE_WORDS
    float* fout;                  // ... and the copy it writes, the same way
    float* ferr;                  // [B][stride]: column i = block first + i of this push
    size_t stride;
    uint32_t pos0;                // j0 mod L
    uint32_t n_out, nseg, B, L;
    int fm;
};

// output z after p = z[j-1]: w = z conj(p) as in dh_cz_fm_item, added to the two chains; z is the next output's p
DH_HD void dh_cz_ferr_step(float zr, float zi, float& pr, float& pi, float& Ar, float& Ai) {
    const float a = zr * pr, c = zi * pi, d = zi * pr, e = zr * pi;
    const float wr = a + c, wi = d - e;
    Ar = Ar + wr; Ai = Ai + wi;
    pr = zr; pi = zi;
}

// segment s of channel b, the rows [r0, r1) of the push as in dh_cz_power_segment; its first p is the carried z (s = 0) or
// row r0 - 1 of this push.  The products do not depend on the chains: the loads and they run ahead of the dependent adds.
DH_HD void dh_cz_ferr_segment(const DhCzFerrParams& P, uint32_t b, uint32_t s) {
    const uint32_t end = (s + 1u) * P.L - P.pos0;                       // row after the block's last output
    const uint32_t r0 = s ? s * P.L - P.pos0 : 0u, r1 = dh_min(end, P.n_out);
    float Ar = 0.0f, Ai = 0.0f, pr = 0.0f, pi = 0.0f;
    if (s == 0u) {
        const DhCzF4 c = *(const DhCzF4*) (P.fin + (size_t) b * DH_CZ_FSTATE_WORDS);
        if (P.pos0) { Ar = c.v[0]; Ai = c.v[1]; }
        pr = c.v[2]; pi = c.v[3];
    }
    uint32_t r = r0;
    if (P.fm) {                   // lanes on consecutive channels: 8-byte loads, 512 contiguous bytes per wave instruction
        const size_t step = 2 * (size_t) P.B;
        const float* p = P.z + 2 * ((size_t) r0 * P.B + b);
        if (s) { const DhCzF2 v = *(const DhCzF2*) (p - step); pr = v.v[0]; pi = v.v[1]; }
        for (; r + 8 <= r1; r += 8, p += 8 * step) {                    // eight loads in flight ahead of the chains
            DhCzF2 v[8];
            for (int e = 0; e < 8; e++) v[e] = *(const DhCzF2*) (p + e * step);
            for (int e = 0; e < 8; e++) dh_cz_ferr_step(v[e].v[0], v[e].v[1], pr, pi, Ar, Ai);
        }
        for (; r < r1; r++, p += step) { const DhCzF2 v = *(const DhCzF2*) p; dh_cz_ferr_step(v.v[0], v.v[1], pr, pi, Ar, Ai); }
    } else {                      // each lane along its own contiguous segment of its row
        const float* p = P.z + 2 * ((size_t) b * P.z_stride + r0);
        const bool al8 = ((uintptr_t) p & 7u) == 0;
        if (s) {
            if (al8) { const DhCzF2 v = *(const DhCzF2*) (p - 2); pr = v.v[0]; pi = v.v[1]; }
            else { pr = p[-2]; pi = p[-1]; }
        }
        if (al8) {
            if (((uintptr_t) p & 8u) && r < r1) { const DhCzF2 v = *(const DhCzF2*) p; dh_cz_ferr_step(v.v[0], v.v[1], pr, pi, Ar, Ai); r++; p += 2; }
            for (; r + 16 <= r1; r += 16, p += 32) {                    // eight 16-byte loads in flight: one 128-byte line
                DhCzF4 v[8];
                for (int e = 0; e < 8; e++) v[e] = *(const DhCzF4*) (p + 4 * e);
                for (int e = 0; e < 8; e++) { dh_cz_ferr_step(v[e].v[0], v[e].v[1], pr, pi, Ar, Ai); dh_cz_ferr_step(v[e].v[2], v[e].v[3], pr, pi, Ar, Ai); }
            }
            for (; r + 2 <= r1; r += 2, p += 4) {
                const DhCzF4 v = *(const DhCzF4*) p;
                dh_cz_ferr_step(v.v[0], v.v[1], pr, pi, Ar, Ai); dh_cz_ferr_step(v.v[2], v.v[3], pr, pi, Ar, Ai);
            }
        }
        for (; r < r1; r++, p += 2) dh_cz_ferr_step(p[0], p[1], pr, pi, Ar, Ai);           // the last output, or rows that are only 4-byte aligned
    }
    const bool complete = end <= P.n_out;
    if (complete) P.ferr[(size_t) b * P.stride + s] = dh_fe_atan2f_over_pi(Ai, Ar);
    // The carry goes to the other copy of the state (fout), never to the one the lane of segment 0 reads in this same launch
    // (fin): nothing orders the two lanes.  The host swaps the copies for the next push.
    if (s + 1u == P.nseg) {
        DhCzF4 c;
        c.v[0] = complete ? 0.0f : Ar; c.v[1] = complete ? 0.0f : Ai; c.v[2] = pr; c.v[3] = pi;
        *(DhCzF4*) (P.fout + (size_t) b * DH_CZ_FSTATE_WORDS) = c;
    }
}

// ---- host side: the phasor tables and the rotated taps (computed once per create / retune, then uploaded) ---------------
// coarse ++ fine, [2][4096][2] floats
inline const float* dh_cz_host_tables() {
    static const float* t = [] {
        float* v = new float[4 * 4096];
        const double two_pi = 6.283185307179586476925286766559;
        for (int i = 0; i < 4096; i++) {
            const double ac = (double) i * (two_pi / 4096.0), af = (double) i * (two_pi / 16777216.0);
            v[2 * i] = (float) cos(ac); v[2 * i + 1] = (float) sin(ac);
            v[8192 + 2 * i] = (float) cos(af); v[8192 + 2 * i + 1] = (float) sin(af);
        }
        return (const float*) v;
    }();
    return t;
}

// the four B-operand entries of G[k] = (gr, gi): rows 2k (x real part) and 2k + 1 (x imaginary part) of a channel's two columns
inline void dh_cz_column_entries(float gr, float gi, uint32_t k, float* re_col, float* im_col) {
    re_col[2 * k] = gr; re_col[2 * k + 1] = -gi;
    im_col[2 * k] = gi; im_col[2 * k + 1] = gr;
}

// the two GEMM columns of one channel: re_col / im_col [2 T'] (rows 2k, 2k + 1), h zero-padded to T'
inline void dh_cz_columns(const float* h, uint32_t tpad, uint32_t u, float* re_col, float* im_col) {
    const float* t = dh_cz_host_tables();
    for (uint32_t k = 0; k < tpad; k++) {
        float pr, pi;
        dh_cz_phasor(u * k, t, t + 8192, pr, pi);
        dh_cz_column_entries(h[k] * pr, h[k] * pi, k, re_col, im_col);
    }
}

// raster: the two GEMM columns of the channel on bin c (0 <= c < K): re_col / im_col [2 K'] (rows 2r, 2r + 1), G zero beyond K
inline void dh_cz_raster_columns(uint32_t K, uint32_t kpad, uint32_t c, float* re_col, float* im_col) {
    const float* t = dh_cz_host_tables();
    for (uint32_t r = 0; r < kpad; r++) {
        float gr = 0.0f, gi = 0.0f;
        if (r < K) dh_cz_phasor(dh_cz_raster_phi((uint32_t) (((uint64_t) c * r) % K), K), t, t + 8192, gr, gi);
        dh_cz_column_entries(gr, gi, r, re_col, im_col);
    }
}

#if !DH_DEVICE_BUILD
// ---- CPU restatements of the matrix-core stages (engine.hip has the gfx950 kernels; the other launches follow, one text for both builds)
static int dh_be_cz_gemm(const DhCzParams& P, void*) {
    for (uint32_t b = 0; b < P.B; b++)
        for (uint32_t row = 0; row < P.n_out; row++) dh_cz_output(P, row, b);
    return 0;
}
static int dh_be_cz_gemm_rat(const DhCzRatParams& R, void*) {
    for (uint32_t s = 0; s < R.nslots; s++)
        for (uint32_t b = 0; b < R.g.B; b++)
            for (uint32_t i = 0; i < R.ph[s].count; i++) dh_cz_output_rat(R, s, i, b);
    return 0;
}
static int dh_be_cz_fold(const DhCzFoldParams& F, void*) {
    for (uint32_t row = 0; row < F.nrows; row++)
        for (uint32_t r = 0; r < F.kpad; r++) dh_cz_fold_item(F, row, r);
    return 0;
}
static int dh_be_cz_gemm_raster(const DhCzRasterParams& R, void*) {
    for (uint32_t b = 0; b < R.g.B; b++)
        for (uint32_t i = 0; i < R.g.n_out; i++) dh_cz_output_raster(R, i, b);
    return 0;
}
#endif

// ---------------------------------------------------------------------------------- channelizer (channelizer_core.hpp)
namespace {

__global__ __launch_bounds__(256) void k_cz_window(float* cur, const float* prev, uint32_t prev_n, const void* in, int cf32, uint32_t H, size_t n) {
    for (size_t e = blockIdx.x * (size_t) blockDim.x + threadIdx.x; e < n; e += (size_t) gridDim.x * blockDim.x)
        dh_cz_window_item(cur, prev, prev_n, in, cf32, H, e);
}

__global__ __launch_bounds__(256) void k_cz_fm(const float* zbuf, const float* state, float* out, size_t out_stride, uint32_t B, uint32_t n_out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_out) return;
    for (uint32_t b = blockIdx.y; b < B; b += gridDim.y) dh_cz_fm_item(zbuf, state, out, out_stride, B, b, j);
}

__global__ __launch_bounds__(DH_WAVE) void k_cz_tail(const float* zbuf, float* state, float* out, size_t out_stride, uint32_t B, uint32_t n_out, int dcblock) {
    const uint32_t b = blockIdx.x * DH_WAVE + threadIdx.x;
    if (b < B) dh_cz_tail_channel(zbuf, state, out, out_stride, B, n_out, dcblock, b);
}

// Block power (channelizer_core.hpp): one lane per (channel, block segment of this push).  FM mode: lanes on consecutive
// channels of zbuf [n_out][B][2]; IQ mode: lanes on consecutive segments of one channel's row.
__global__ __launch_bounds__(256) void k_cz_power(const DhCzPowerParams P) {
    const size_t n = (size_t) P.B * P.nseg;
    for (size_t t = (size_t) blockIdx.x * 256u + threadIdx.x; t < n; t += (size_t) gridDim.x * 256u) {
        const uint32_t b = (uint32_t) (P.fm ? t % P.B : t / P.nseg), s = (uint32_t) (P.fm ? t / P.B : t % P.nseg);
        dh_cz_power_segment(P, b, s);
    }
}

__global__ __launch_bounds__(DH_WAVE) void k_cz_gate(const DhCzPowerParams P) {
    const uint32_t b = blockIdx.x * DH_WAVE + threadIdx.x;
    if (b < P.B) dh_cz_gate_channel(P, b);
}

}  // namespace

static int dh_be_cz_window(float* cur, const float* prev, uint32_t prev_n, const void* in, int cf32, uint32_t H, size_t n_in, void* stream) {
    const size_t n = H + n_in;
    return dh_launch(k_cz_window, dim3(grid_for(n, 256)), dim3(256), 0, stream, "k_cz_window", cur, prev, prev_n, in, cf32, H, n) ? DH_EDEVICE : DH_OK;
}
static int dh_be_cz_fm(const float* zbuf, float* state, float* out, size_t out_stride, uint32_t B, uint32_t n_out, int dcblock, void* stream) {
    if (!n_out) return DH_OK;
    if (dh_launch(k_cz_fm, dim3((n_out + 255) / 256, B < 65535u ? B : 65535u), dim3(256), 0, stream, "k_cz_fm", zbuf, state, out, out_stride, B, n_out)) return DH_EDEVICE;
    return dh_launch(k_cz_tail, dim3((B + DH_WAVE - 1) / DH_WAVE), dim3(DH_WAVE), 0, stream, "k_cz_tail", zbuf, state, out, out_stride, B, n_out, dcblock) ? DH_EDEVICE : DH_OK;
}
static int dh_be_cz_power(const DhCzPowerParams& P, void* stream) {
    if (P.nseg && dh_launch(k_cz_power, dim3(grid_for((size_t) P.B * P.nseg, 256)), dim3(256), 0, stream, "k_cz_power", P)) return DH_EDEVICE;
    return dh_launch(k_cz_gate, dim3((P.B + DH_WAVE - 1) / DH_WAVE), dim3(DH_WAVE), 0, stream, "k_cz_gate", P) ? DH_EDEVICE : DH_OK;
}

// ---------------------------------------------------------------- frequency-error blocks (after the launches above: they
// stay the text they were)
namespace {

// one lane per (channel, block segment of this push), k_cz_power's item map: FM mode lanes on consecutive channels of zbuf,
// IQ mode lanes on consecutive segments of one channel's row
__global__ __launch_bounds__(256) void k_cz_ferr(const DhCzFerrParams P) {
    const size_t n = (size_t) P.B * P.nseg;
    for (size_t t = (size_t) blockIdx.x * 256u + threadIdx.x; t < n; t += (size_t) gridDim.x * 256u) {
        const uint32_t b = (uint32_t) (P.fm ? t % P.B : t / P.nseg), s = (uint32_t) (P.fm ? t / P.B : t % P.nseg);
        dh_cz_ferr_segment(P, b, s);
    }
}

}  // namespace

// only for a push with outputs (nseg != 0)
static int dh_be_cz_ferr(const DhCzFerrParams& P, void* stream) {
    return dh_launch(k_cz_ferr, dim3(grid_for((size_t) P.B * P.nseg, 256)), dim3(256), 0, stream, "k_cz_ferr", P) ? DH_EDEVICE : DH_OK;
}
