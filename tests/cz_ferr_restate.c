/* cz_ferr_restate.c -- the channelizer's frequency-error blocks (digiham_amd/csrc/channelizer_core.hpp)
 * restated as plain scalar C, output by output, from the written text only.  Built by tests/test_channelizer_ferr.py with
 * -O2 -ffp-contract=off.  The z rows it reads are those of the tests/cz_*restate.c of the bank, before the discriminator. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

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

/* z: [B][n][2] rotated outputs of the whole stream.  The stream is cut into npush pushes of push_len[s] outputs each
 * (their sum is <= n; outputs beyond it are ignored).  Before push s, channel b is retuned when retune[s * B + b] != 0.
 * ferr: [B][n / L], block m in column m. */
void cz_ferr_restate(const float* z, uint32_t B, size_t n, uint32_t L, const uint64_t* push_len, uint32_t npush,
                     const uint8_t* retune, float* ferr) {
    const size_t n_blocks = n / L;
    for (uint32_t b = 0; b < B; b++) {
        const float* zb = z + 2 * (size_t) b * n;
        float Ar = 0.0f, Ai = 0.0f;
        float pr = 0.0f, pi = 0.0f;                   /* z[j - 1]; z[-1] = 0 */
        uint64_t j = 0;                               /* the global output index */
        for (uint32_t s = 0; s < npush; s++) {
            if (retune[(size_t) s * B + b]) { Ar = 0.0f; Ai = 0.0f; pr = 0.0f; pi = 0.0f; }
            for (uint64_t i = 0; i < push_len[s]; i++, j++) {
                if (j % L == 0) { Ar = 0.0f; Ai = 0.0f; }                /* a block begins */
                const float zr = zb[2 * j], zi = zb[2 * j + 1];
                const float a = zr * pr;
                const float c = zi * pi;
                const float d = zi * pr;
                const float e = zr * pi;
                const float wr = a + c;
                const float wi = d - e;
                Ar = Ar + wr;
                Ai = Ai + wi;
                pr = zr; pi = zi;
                if (j % L == L - 1u) ferr[(size_t) b * n_blocks + j / L] = atan2_over_pi(Ai, Ar);
            }
        }
    }
}
