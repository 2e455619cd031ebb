/* cz_power_restate.c -- the channelizer's block power, squelch gate and push counts (digiham_amd/csrc/channelizer_core.hpp,
 * DESIGN.md section 4.6) restated as plain scalar C, output by output, from the written text only.  Built by
 * tests/test_channelizer_power.py with -O2 -ffp-contract=off.  The z rows it reads are those of tests/cz_restate.c in IQ mode. */
#include <stddef.h>
#include <stdint.h>

/* z: [B][n][2] rotated outputs of the whole stream.  The stream is cut into npush pushes of push_len[s] outputs each
 * (their sum is <= n; outputs beyond it are ignored).  Before push s, channel b is retuned when retune[s * B + b] != 0.
 * Push s uses open_level[s], close_level[s] and hang[s].
 * power, gate: [B][n / L], block m in column m.  counts: [npush][B]. */
void cz_power_restate(const float* z, uint32_t B, size_t n, uint32_t L, const float* open_level, const float* close_level,
                      const uint32_t* hang, const uint64_t* push_len, uint32_t npush, const uint8_t* retune,
                      float* power, uint8_t* gate, uint32_t* counts) {
    const size_t n_blocks = n / L;
    const float inv = (float) (1.0 / (double) L);
    for (uint32_t b = 0; b < B; b++) {
        const float* zb = z + 2 * (size_t) b * n;
        float S = 0.0f;
        int open = 0;
        uint32_t quiet = 0;
        uint64_t j = 0;                               /* the global output index */
        for (uint32_t s = 0; s < npush; s++) {
            if (retune[(size_t) s * B + b]) { S = 0.0f; open = 0; quiet = 0; }
            const int open_at_begin = open;
            int any_open_byte = 0;
            for (uint64_t i = 0; i < push_len[s]; i++, j++) {
                if (j % L == 0) S = 0.0f;             /* a block begins */
                const float zr = zb[2 * j], zi = zb[2 * j + 1];
                const float rr = zr * zr;
                const float ii = zi * zi;
                const float q = rr + ii;
                S = S + q;
                if (j % L == L - 1u) {                /* the block's last output has been added */
                    const uint64_t m = j / L;
                    const float p = S * inv;
                    if (!open) {
                        if (p >= open_level[s]) { open = 1; quiet = 0; }
                    } else {
                        if (p >= close_level[s]) quiet = 0;
                        else { quiet = quiet + 1; if (quiet > hang[s]) { open = 0; quiet = 0; } }
                    }
                    power[(size_t) b * n_blocks + m] = p;
                    gate[(size_t) b * n_blocks + m] = (uint8_t) open;
                    if (open) any_open_byte = 1;
                }
            }
            counts[(size_t) s * B + b] = (open_at_begin || any_open_byte) ? (uint32_t) push_len[s] : 0u;
        }
    }
}
