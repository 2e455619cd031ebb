// raster_lifecycle.cpp -- the channelizer's three kinds of bank (fixed offsets, a rational rate, a uniform raster) behind the
// C ABI (digiham_amd/csrc/abi_impl.hpp over the CPU backend) as a stand-alone program meant to be built with
// -fsanitize=address,undefined and run with leak detection: create and destroy, the raster's invalid configurations, a
// configuration struct of the older size that ends exactly where its heap block ends, and for every kind create with the k-th
// allocation failing for every k and ragged pushes with a retune and a reset whose every window, fold-buffer and output index
// the sanitizer checks ("device memory" is the host heap here).  Then dh_cz_plan_rat at L = 1 against the formulas a fixed
// bank's own launch takes its position from.
#include <math.h>
#include <stdio.h>

#include "../host_harness/harness.cpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static float TAPS[101];
static const int32_t BINS[5] = { 0, 12, -1, 23, -12 };
static const uint32_t INCS[5] = { 0u, 1u << 31, 0x12345678u, 0xfffff000u, 1u };

enum { FIXED, RATIONAL, RASTER };
static const char* const KIND[3] = { "fixed", "rational", "raster" };
// fixed: D = 7; rational: L / M = 3 / 7; raster: K = 24, D = 7
static dh_channelizer_config kind_cfg(int kind, int mode) {
    dh_channelizer_config c{};
    c.struct_size = sizeof(c); c.n_channels = 5; c.decimation = 7; c.taps = TAPS; c.n_taps = 101;
    c.input_format = DH_CZ_CS16; c.output_mode = mode; c.dcblock = mode == DH_CZ_FM; c.max_input = 700;
    c.interpolation = kind == RATIONAL ? 3 : 1;
    if (kind == RASTER) { c.raster = 24; c.bins = BINS; } else c.increments = INCS;
    return c;
}

int main() {
    for (int k = 0; k < 101; k++) TAPS[k] = 0.01f * (float) sin(0.3 * k + 1.0);
    dh_channelizer* z = nullptr;
    dh_channelizer* const junk = (dh_channelizer*) (uintptr_t) 16;
    const dh_channelizer_config good = kind_cfg(RASTER, DH_CZ_FM);
    // invalid configurations: DH_EINVAL, *out null, nothing allocated (an allocation would trip the armed failure)
    int cases = 0;
    auto bad = [&](auto change) {
        dh_channelizer_config c = good;
        change(c);
        z = junk; g_alloc_fail_in = 1;
        const int rc = dh_channelizer_create(&c, &z);
        if (rc != DH_EINVAL || z != nullptr || g_alloc_fail_in != 1) { printf("FAILED: invalid configuration %d gave %d\n", cases, rc); failures++; }
        g_alloc_fail_in = 0;
        cases++;
    };
    bad([](dh_channelizer_config& c) { c.raster = 1; });
    bad([](dh_channelizer_config& c) { c.raster = 16385; });
    bad([](dh_channelizer_config& c) { c.bins = nullptr; });
    bad([](dh_channelizer_config& c) { c.interpolation = 3; });
    bad([](dh_channelizer_config& c) { c.raster = 2; c.n_taps = 129; });
    bad([](dh_channelizer_config& c) { c.raster = 0; });                    // fixed offsets need increments
    bad([](dh_channelizer_config& c) { c.struct_size = sizeof(c) - 1; });   // below the whole struct: fixed offsets, so the same
    // the older struct: it ended with `interpolation` and its size covered the tail padding behind it, where raster sits now
    // and which its callers never wrote.  Its block ends where it ended (reading bins would be a heap overflow) and the
    // padding holds 0xA5: a fixed-offset bank all the same.  So is a block that ends right after `interpolation`.
    struct older_config {
        uint32_t struct_size; int32_t device; uint32_t n_channels, decimation; const float* taps; uint32_t n_taps;
        const uint32_t* increments; int32_t input_format, output_mode, dcblock; uint32_t max_input; void* stream; uint32_t interpolation;
    };
    static_assert(offsetof(older_config, interpolation) == offsetof(dh_channelizer_config, interpolation), "the older layout");
    static_assert(sizeof(older_config) > offsetof(dh_channelizer_config, raster) && sizeof(older_config) < sizeof(dh_channelizer_config),
                  "the older size covers raster and not bins");
    for (const size_t old : { sizeof(older_config), offsetof(dh_channelizer_config, raster) }) {
        char* block = (char*) malloc(old);
        dh_channelizer_config c = good;
        c.increments = INCS; c.struct_size = (uint32_t) old;
        memcpy(block, &c, old);
        for (size_t i = offsetof(dh_channelizer_config, raster); i < old; i++) block[i] = (char) 0xA5;
        CHECK(dh_channelizer_create((const dh_channelizer_config*) block, &z) == DH_OK && z && z->K == 0);
        dh_channelizer_destroy(z);
        free(block);
    }
    for (int kind : { FIXED, RATIONAL, RASTER }) {
        // the k-th allocation failing
        const dh_channelizer_config fmc = kind_cfg(kind, DH_CZ_FM);
        int k = 1;
        for (;; k++) {
            g_alloc_fail_in = k; z = junk;
            const int rc = dh_channelizer_create(&fmc, &z);
            const bool fired = g_alloc_fail_in == 0;
            g_alloc_fail_in = 0;
            if (rc == DH_OK) { CHECK(!fired && z != nullptr && z != junk && (z->K != 0) == (kind == RASTER)); dh_channelizer_destroy(z); break; }
            if (rc != DH_ENOMEM || z != nullptr || !fired || k > 100) { printf("FAILED: %s, allocation %d failing gave %d\n", KIND[kind], k, rc); failures++; break; }
        }
        // pushes: ragged lengths, a retune, a reset, both output modes; every index under the sanitizer
        const uint64_t L = fmc.interpolation;
        for (int mode : { DH_CZ_IQ_F32, DH_CZ_FM }) {
            const dh_channelizer_config c = kind_cfg(kind, mode);
            CHECK(dh_channelizer_create(&c, &z) == DH_OK);
            int16_t in[2 * 700];
            for (int i = 0; i < 1400; i++) in[i] = (int16_t) ((i * 7919) % 4001 - 2000);
            const size_t stride = 100 * L + 1, per = mode == DH_CZ_FM ? 1 : 2;
            float* rows = (float*) malloc(sizeof(float) * 5 * stride * per);
            const size_t lens[] = { 0, 1, 6, 7, 52, 0, 700, 5, 333 };
            uint64_t total = 0;
            for (int round = 0; round < 2; round++) {
                for (size_t len : lens) {
                    size_t n = 99;
                    CHECK(dh_channelizer_push_host(z, in, len, rows, stride, &n) == DH_OK && n == L * (total + len) / 7 - L * total / 7);
                    total += len;
                    if (len == 52) CHECK(dh_channelizer_retune(z, 1, (uint32_t) -5) == DH_OK && dh_channelizer_retune(z, 5, 0) == DH_EINVAL);
                }
                CHECK(dh_channelizer_reset(z) == DH_OK);
                total = 0;
            }
            free(rows);
            dh_channelizer_destroy(z);
        }
        printf("%s: %d allocations\n", KIND[kind], k - 1);
    }
    // A fixed bank's push is the rational push with one slot: dh_cz_plan_rat at L = 1 against the position a fixed bank's own
    // launch takes, written out -- j0 = N0 / D, off0 = D - 1 - N0 mod D, n_j0 = (uint32) (j0 D + D - 1).  Past 2^32 is where the
    // 64-bit and the 32-bit form of n_j have to agree.
    int points = 0;
    const uint64_t one = 1;
    for (const uint64_t D : { one, 7 * one, 50 * one })
        for (const uint64_t N0 : { 0 * one, one, D - 1, D, (one << 32) - 3, (one << 32) + D, (one << 40) + 5 })
            for (const uint64_t n_in : { 0 * one, one, D - 1, D, 1000 * one }) {
                DhCzRatParams R{};
                R.L = 1; R.g.D = (uint32_t) D; R.g.tpad = 112;
                dh_cz_plan_rat(R, N0, n_in);
                const uint64_t j0 = N0 / D, n_out = (N0 + n_in) / D - j0;
                const uint32_t off0 = (uint32_t) (D - 1 - N0 % D), n_j0 = (uint32_t) (j0 * D + D - 1);
                CHECK(R.g.n_out == n_out && R.nslots == (n_out ? 1u : 0u));
                if (n_out) CHECK(R.ph[0].count == n_out && R.ph[0].wbase == R.g.tpad - 1u + off0 && R.ph[0].nj0 == n_j0 && R.ph[0].bank == 0u);
                points++;
            }
    printf("raster: %d invalid configurations; one slot at L = 1: %d points\n", cases, points);
    if (!failures) printf("raster lifecycle: clean\n");
    return failures ? 1 : 0;
}
