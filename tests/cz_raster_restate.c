/* cz_raster_restate.c -- the channelizer's uniform-raster specification (digiham_amd/csrc/channelizer_core.hpp, "Uniform
 * raster") restated as plain scalar C, output by output, from the written text only: a literal triple
 * loop -- fold, DFT chain, rotation -- then FM and the DC blocker of the top of that header.  Built by
 * tests/test_channelizer_raster.py with -ffp-contract=off; every fused multiply-add below is an explicit fmaf. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static float tab_c[4096][2], tab_f[4096][2];
static int tab_ready;

static void tables(void) {
    if (tab_ready) return;
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < 4096; i++) {
        tab_c[i][0] = (float) cos((double) i * (two_pi / 4096.0));
        tab_c[i][1] = (float) sin((double) i * (two_pi / 4096.0));
        tab_f[i][0] = (float) cos((double) i * (two_pi / 16777216.0));
        tab_f[i][1] = (float) sin((double) i * (two_pi / 16777216.0));
    }
    tab_ready = 1;
}

static void phasor(uint32_t phi, float* pr, float* pi) {
    tables();
    uint32_t v = phi + (1u << 7);
    uint32_t c = v >> 20, f = (v >> 8) & 4095u;
    float p1 = tab_c[c][0] * tab_f[f][0];
    float p2 = tab_c[c][1] * tab_f[f][1];
    float p3 = tab_c[c][0] * tab_f[f][1];
    float p4 = tab_c[c][1] * tab_f[f][0];
    *pr = p1 - p2;
    *pi = p3 + p4;
}

/* Phi(q), 0 <= q < K */
static uint32_t phase_word(uint64_t q, uint32_t K) { return (uint32_t) (((q << 32) + K / 2u) / K); }

/* atan2(im, re) / pi: the front-end's polynomial (frontend_core.hpp header comment) */
static float atan2_over_pi(float im, float re) {
    if (re == 0.0f && im == 0.0f) return 0.0f;
    float are = fabsf(re), aim = fabsf(im);
    int swap = aim > are;
    float r = swap ? are / aim : aim / are;
    float s = r * r;
    static const float c[8] = { -0.0161657367f, 0.0429096138f, -0.0752896400f, 0.1065626393f, -0.1420889944f,
                                0.1999355085f, -0.3333314528f, 1.0f };
    float p = 0.0028662257f;
    for (int i = 0; i < 8; i++) { p = p * s; p = p + c[i]; }
    float a = p * r;
    if (swap) a = 1.57079632679489661923f - a;
    if (re < 0.0f) a = 3.14159265358979323846f - a;
    if (im < 0.0f) a = -a;
    return a * 0.31830988618379067154f;
}

/* The whole stream in one call.  in: n complex samples (int16 pairs if !cf32, float pairs otherwise).  The stream is cut
 * into nseg pushes starting at input index seg_start[s] (seg_start[0] = 0); channel b sits on bin bins[s * B + b] for the
 * outputs whose n_j lies in push s, and reset[s * B + b] != 0 restarts its FM / DC state at that push (a retune).
 * out: [B][n / D] floats (FM) or [B][n / D][2] (IQ); zout (may be NULL): the rotated z, [B][n / D][2], in both modes. */
void cz_raster_restate(const void* in, int cf32, size_t n, uint32_t D, const float* h, uint32_t T, uint32_t K, uint32_t B,
                       const uint64_t* seg_start, const int32_t* bins, const uint8_t* reset, uint32_t nseg, int fm, int dcblock,
                       float* out, float* zout) {
    const size_t n_out = n / D;
    const uint32_t P = (T + K - 1u) / K, Kp = 16u * ((K + 15u) / 16u);
    float* xr = (float*) malloc(sizeof(float) * (n ? n : 1));
    float* xi = (float*) malloc(sizeof(float) * (n ? n : 1));
    for (size_t i = 0; i < n; i++) {
        if (cf32) { xr[i] = ((const float*) in)[2 * i]; xi[i] = ((const float*) in)[2 * i + 1]; }
        else { xr[i] = (float) ((const int16_t*) in)[2 * i] * (1.0f / 32768.0f); xi[i] = (float) ((const int16_t*) in)[2 * i + 1] * (1.0f / 32768.0f); }
    }
    float* hp = (float*) calloc((size_t) P * K, sizeof(float));        /* h zero-padded to P K */
    memcpy(hp, h, sizeof(float) * T);
    float* vr = (float*) malloc(sizeof(float) * Kp);
    float* vi = (float*) malloc(sizeof(float) * Kp);
    for (uint32_t b = 0; b < B; b++) {
        float zpr = 0.0f, zpi = 0.0f, xp = 0.0f, yp = 0.0f;
        uint32_t s = 0;
        int have = 0;
        for (size_t j = 0; j < n_out; j++) {
            const uint64_t nj = (uint64_t) j * D + D - 1;
            uint32_t s_new = s;
            while (s_new + 1 < nseg && seg_start[s_new + 1] <= nj) s_new++;
            if (!have || s_new != s) {
                for (uint32_t t = have ? s + 1 : 1; t <= s_new; t++)
                    if (reset[(size_t) t * B + b]) { zpr = zpi = 0.0f; xp = yp = 0.0f; }
                s = s_new; have = 1;
            }
            int64_t cb = (int64_t) bins[(size_t) s * B + b] % (int64_t) K;
            if (cb < 0) cb += K;
            /* fold */
            for (uint32_t r = 0; r < Kp; r++) {
                float ar = 0.0f, ai = 0.0f;
                if (r < K)
                    for (uint32_t p = 0; p < P; p++) {
                        const int64_t idx = (int64_t) nj - (int64_t) r - (int64_t) p * K;
                        const float sr = idx >= 0 ? xr[idx] : 0.0f, si = idx >= 0 ? xi[idx] : 0.0f;
                        ar = fmaf(hp[r + (size_t) p * K], sr, ar);
                        ai = fmaf(hp[r + (size_t) p * K], si, ai);
                    }
                vr[r] = ar; vi[r] = ai;
            }
            /* DFT */
            float yr = 0.0f, yi = 0.0f;
            for (uint32_t r = 0; r < Kp; r++) {
                float gr = 0.0f, gi = 0.0f;
                if (r < K) phasor(phase_word(((uint64_t) cb * r) % K, K), &gr, &gi);
                yr = fmaf(vr[r], gr, yr); yr = fmaf(vi[r], -gi, yr);
                yi = fmaf(vr[r], gi, yi); yi = fmaf(vi[r], gr, yi);
            }
            /* rotation */
            float qr, qi;
            phasor(phase_word((K - ((uint64_t) cb * (nj % K)) % K) % K, K), &qr, &qi);
            const float m1 = qr * yr, m2 = qi * yi, m3 = qr * yi, m4 = qi * yr;
            const float zr = m1 - m2, zi = m3 + m4;
            if (zout) { zout[2 * ((size_t) b * n_out + j)] = zr; zout[2 * ((size_t) b * n_out + j) + 1] = zi; }
            if (!fm) { out[2 * ((size_t) b * n_out + j)] = zr; out[2 * ((size_t) b * n_out + j) + 1] = zi; continue; }
            const float w1 = zr * zpr, w2 = zi * zpi, w3 = zi * zpr, w4 = zr * zpi;
            float v = atan2_over_pi(w3 - w4, w1 + w2);
            zpr = zr; zpi = zi;
            if (dcblock) { const float d = v - xp; const float e = 0.995f * yp; const float y = d + e; xp = v; yp = y; v = y; }
            out[(size_t) b * n_out + j] = v;
        }
    }
    free(xr); free(xi); free(hp); free(vr); free(vi);
}
