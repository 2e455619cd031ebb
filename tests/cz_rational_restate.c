/* cz_rational_restate.c -- the channelizer's rational-rate specification (digiham_amd/csrc/channelizer_core.hpp, "Rational
 * rates") restated as plain scalar C from the written text only, in its literal zero-stuffed form:
 * every output walks the prototype's taps t = 0 .. T-1 and skips those that meet a stuffed zero of the virtual stream.
 * Built by tests/test_channelizer_rational.py with -ffp-contract=off; every fused multiply-add below is an explicit fmaf. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static float cosc[4096], sinc_[4096], cosf_[4096], sinf_[4096];
static int ready;

static void phasor(uint32_t phi, float* pr, float* pi) {
    if (!ready) {
        const double turn = 6.283185307179586476925286766559;
        for (int i = 0; i < 4096; i++) {
            cosc[i] = (float) cos((double) i * (turn / 4096.0));
            sinc_[i] = (float) sin((double) i * (turn / 4096.0));
            cosf_[i] = (float) cos((double) i * (turn / 16777216.0));
            sinf_[i] = (float) sin((double) i * (turn / 16777216.0));
        }
        ready = 1;
    }
    const uint32_t v = phi + 128u;
    const uint32_t c = v >> 20, f = (v >> 8) & 4095u;
    const float a = cosc[c] * cosf_[f];
    const float b = sinc_[c] * sinf_[f];
    const float d = cosc[c] * sinf_[f];
    const float e = sinc_[c] * cosf_[f];
    *pr = a - b;
    *pi = d + e;
}

/* atan2(im, re) / pi: the front-end's polynomial (frontend_core.hpp header comment) */
static float angle_over_pi(float im, float re) {
    if (re == 0.0f && im == 0.0f) return 0.0f;
    const float are = fabsf(re), aim = fabsf(im);
    const int swap = aim > are;
    const float r = swap ? are / aim : aim / are;
    const float s = r * r;
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

typedef struct { const void* in; int cf32; size_t n; } stream_t;

/* x[idx], zero before the stream */
static void sample(const stream_t* s, int64_t idx, float* re, float* im) {
    if (idx < 0) { *re = 0.0f; *im = 0.0f; return; }
    if (s->cf32) { *re = ((const float*) s->in)[2 * idx]; *im = ((const float*) s->in)[2 * idx + 1]; }
    else {
        *re = (float) ((const int16_t*) s->in)[2 * idx] * (1.0f / 32768.0f);
        *im = (float) ((const int16_t*) s->in)[2 * idx + 1] * (1.0f / 32768.0f);
    }
}

/* one more term of the two chains: tap value hk at position k of its phase, against x[nj - k] */
static void term(const stream_t* s, uint32_t u, int64_t nj, uint32_t k, float hk, float* yr, float* yi) {
    float pr, pi, ar, ai;
    phasor(u * k, &pr, &pi);
    const float gr = hk * pr, gi = hk * pi;
    sample(s, nj - (int64_t) k, &ar, &ai);
    *yr = fmaf(ar, gr, *yr); *yr = fmaf(ai, -gi, *yr);
    *yi = fmaf(ar, gi, *yi); *yi = fmaf(ai, gr, *yi);
}

/* The whole stream in one call: n complex input samples, rate L / M, prototype h[0..T) at the virtual rate.  The stream is
 * cut into nseg pushes starting at input index seg_start[s] (seg_start[0] = 0); channel b uses increment inc[s * B + b]
 * for the outputs whose n_j lies in push s, and reset[s * B + b] != 0 restarts its FM / DC state at that push (a retune).
 * out: [B][L n / M] floats (FM) or [B][L n / M][2] (IQ). */
void cz_rational_restate(const void* in, int cf32, size_t n, uint32_t L, uint32_t M, const float* h, uint32_t T, uint32_t B,
                         const uint64_t* seg_start, const uint32_t* inc, const uint8_t* reset, uint32_t nseg, int fm, int dcblock,
                         float* out) {
    const stream_t st = { in, cf32, n };
    const size_t n_out = (size_t) ((uint64_t) L * n / M);
    const uint32_t per_phase = (T + L - 1u) / L;
    const uint32_t Tp = 16u * ((per_phase + 15u) / 16u);
    for (uint32_t b = 0; b < B; b++) {
        float zpr = 0.0f, zpi = 0.0f, xp = 0.0f, yp = 0.0f;
        uint32_t seg = 0;
        for (size_t j = 0; j < n_out; j++) {
            const int64_t v = (int64_t) j * M + M - 1;                 /* virtual index */
            const int64_t nj = v / L;                                  /* the newest real sample at or before it */
            while (seg + 1 < nseg && seg_start[seg + 1] <= (uint64_t) nj) {
                seg++;
                if (reset[(size_t) seg * B + b]) { zpr = zpi = 0.0f; xp = yp = 0.0f; }
            }
            const uint32_t u = inc[(size_t) seg * B + b];
            float yr = 0.0f, yi = 0.0f;
            uint32_t k = 0;
            for (uint32_t t = 0; t < T; t++) {
                const int64_t w = v - (int64_t) t;                     /* virtual sample under tap t */
                if (((w % (int64_t) L) + (int64_t) L) % (int64_t) L != 0) continue;     /* a stuffed zero: skipped, not added */
                term(&st, u, nj, k, h[t], &yr, &yi);                   /* w / L = nj - k */
                k++;
            }
            for (; k < Tp; k++) term(&st, u, nj, k, 0.0f, &yr, &yi);   /* the padding is added */
            float qr, qi;
            phasor(0u - u * (uint32_t) (uint64_t) nj, &qr, &qi);
            const float m1 = qr * yr, m2 = qi * yi, m3 = qr * yi, m4 = qi * yr;
            const float zr = m1 - m2, zi = m3 + m4;
            if (!fm) { out[2 * ((size_t) b * n_out + j)] = zr; out[2 * ((size_t) b * n_out + j) + 1] = zi; continue; }
            const float w1 = zr * zpr, w2 = zi * zpi, w3 = zi * zpr, w4 = zr * zpi;
            float a = angle_over_pi(w3 - w4, w1 + w2);
            zpr = zr; zpi = zi;
            if (dcblock) { const float d = a - xp; const float e = 0.995f * yp; const float y = d + e; xp = a; yp = y; a = y; }
            out[(size_t) b * n_out + j] = a;
        }
    }
}
