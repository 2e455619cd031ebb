/* cz_restate.c -- the channelizer's specification (digiham_amd/csrc/channelizer_core.hpp) restated
 * as plain scalar C, output by output, from the written text only.  Built by tests/test_channelizer.py with
 * -ffp-contract=off; every fused multiply-add below is an explicit fmaf. */
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

void cz_phasor(uint32_t phi, float* pr, float* pi) {
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
 * into nseg pushes starting at input index seg_start[s] (seg_start[0] = 0); channel b uses increment inc[s * B + b] for
 * the outputs whose n_j lies in push s, and reset[s * B + b] != 0 restarts its FM / DC state at that push (a retune).
 * out: [B][n / D] floats (FM) or [B][n / D][2] (IQ). */
void cz_restate(const void* in, int cf32, size_t n, uint32_t D, const float* h, uint32_t T, uint32_t B,
                const uint64_t* seg_start, const uint32_t* inc, const uint8_t* reset, uint32_t nseg, int fm, int dcblock, float* out) {
    const size_t n_out = n / D;
    const uint32_t Tp = 16u * ((T + 15u) / 16u);
    float* xr = (float*) malloc(sizeof(float) * (n ? n : 1));
    float* xi = (float*) malloc(sizeof(float) * (n ? n : 1));
    for (size_t i = 0; i < n; i++) {
        if (cf32) { xr[i] = ((const float*) in)[2 * i]; xi[i] = ((const float*) in)[2 * i + 1]; }
        else { xr[i] = (float) ((const int16_t*) in)[2 * i] * (1.0f / 32768.0f); xi[i] = (float) ((const int16_t*) in)[2 * i + 1] * (1.0f / 32768.0f); }
    }
    float* gr = (float*) malloc(sizeof(float) * Tp);
    float* gi = (float*) malloc(sizeof(float) * Tp);
    for (uint32_t b = 0; b < B; b++) {
        float zpr = 0.0f, zpi = 0.0f, xp = 0.0f, yp = 0.0f;
        uint32_t s = 0, u = 0;
        int have = 0;
        for (size_t j = 0; j < n_out; j++) {
            const uint64_t nj = (uint64_t) j * D + D - 1;
            uint32_t s_new = s;
            while (s_new + 1 < nseg && seg_start[s_new + 1] <= nj) s_new++;
            if (!have || s_new != s) {
                for (uint32_t t = have ? s + 1 : 1; t <= s_new; t++)
                    if (reset[(size_t) t * B + b]) { zpr = zpi = 0.0f; xp = yp = 0.0f; }
                s = s_new; have = 1;
                u = inc[(size_t) s * B + b];
                for (uint32_t k = 0; k < Tp; k++) {
                    float pr, pi;
                    const float hk = k < T ? h[k] : 0.0f;
                    cz_phasor(u * k, &pr, &pi);
                    gr[k] = hk * pr; gi[k] = hk * pi;
                }
            }
            float yr = 0.0f, yi = 0.0f;
            for (uint32_t k = 0; k < Tp; k++) {
                const int64_t idx = (int64_t) nj - (int64_t) k;
                const float ar = idx >= 0 ? xr[idx] : 0.0f, ai = idx >= 0 ? xi[idx] : 0.0f;
                yr = fmaf(ar, gr[k], yr); yr = fmaf(ai, -gi[k], yr);
                yi = fmaf(ar, gi[k], yi); yi = fmaf(ai, gr[k], yi);
            }
            float qr, qi;
            cz_phasor(0u - u * (uint32_t) nj, &qr, &qi);
            const float m1 = qr * yr, m2 = qi * yi, m3 = qr * yi, m4 = qi * yr;
            const float zr = m1 - m2, zi = m3 + m4;
            if (!fm) { out[2 * ((size_t) b * n_out + j)] = zr; out[2 * ((size_t) b * n_out + j) + 1] = zi; continue; }
            const float w1 = zr * zpr, w2 = zi * zpi, w3 = zi * zpr, w4 = zr * zpi;
            float v = atan2_over_pi(w3 - w4, w1 + w2);
            zpr = zr; zpi = zi;
            if (dcblock) { const float d = v - xp; const float e = 0.995f * yp; const float y = d + e; xp = v; yp = y; v = y; }
            out[(size_t) b * n_out + j] = v;
        }
    }
    free(xr); free(xi); free(gr); free(gi);
}
