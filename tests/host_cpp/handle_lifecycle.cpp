// handle_lifecycle.cpp -- create, destroy, invalid configurations, null handles and failed allocations of the five handles
// behind the C ABI (digiham_amd/csrc/abi_impl.hpp over the CPU backend), as a stand-alone program meant to be built with
// -fsanitize=address,undefined and run with leak detection: every path that lets go of a partly built handle is walked,
// and whatever it forgets is a leak report at exit.  Sizes are the smallest legal ones: 2 channels, 64 samples, a ring of
// 128, 16 taps at decimation 4.
#include <math.h>
#include <stdio.h>

#include "../host_harness/harness.cpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static const float TAPS[16] = { 0.01f, 0.02f, 0.04f, 0.06f, 0.08f, 0.1f, 0.11f, 0.12f, 0.12f, 0.11f, 0.1f, 0.08f, 0.06f, 0.04f, 0.02f, 0.01f };
static const uint32_t INCS[2] = { 0u, 1u << 30 };

static dh_engine_config engine_cfg() {
    dh_engine_config c{};
    c.struct_size = sizeof(c); c.n_channels = 2; c.max_samples = 64; c.rrc = DH_RRC_WIDE; c.demod = DH_DEMOD_GFSK4; c.sps = 10;
    c.proto = DH_PROTO_DMR; c.slot_filter = 3;
    return c;
}
static dh_channelizer_config channelizer_cfg() {
    dh_channelizer_config c{};
    c.struct_size = sizeof(c); c.n_channels = 2; c.decimation = 4; c.taps = TAPS; c.n_taps = 16; c.increments = INCS;
    c.input_format = DH_CZ_CS16; c.output_mode = DH_CZ_FM; c.dcblock = 1; c.max_input = 64; c.interpolation = 1;
    return c;
}
static dh_preroll_config preroll_cfg() {
    dh_preroll_config c{};
    c.struct_size = sizeof(c); c.n_channels = 2; c.depth = 128;
    return c;
}
static dh_outpack_config outpack_cfg() {
    dh_outpack_config c{};
    c.struct_size = sizeof(c); c.max_entries = 4; c.max_events = 8; c.max_frame_bytes = 64;
    return c;
}
static dh_monitor_config monitor_cfg() {
    dh_monitor_config c{};
    c.struct_size = sizeof(c); c.n_channels = 2; c.max_samples = 64; c.depth = 128; c.lead = 16; c.confirm = 2; c.release = 4;
    c.protos = 0x3Eu;                                  // all five: four scan engines, five protocol engines, the ring
    return c;
}

// One handle kind: a good configuration comes and goes; destroy(nullptr) is nothing; create without a configuration or an
// out pointer, and with every configuration `spoil` can make of the good one, is DH_EINVAL and leaves *out null; create
// with the k-th allocation failing, k = 1, 2, ... until it succeeds, is an error with *out null every time before.
template <class H, class Cfg, class Spoil>
static void lifecycle(const char* kind, Cfg good, int (*create)(const Cfg*, H**), void (*destroy)(H*), Spoil spoil) {
    H* h = nullptr;
    H* const junk = (H*) (uintptr_t) 16;
    CHECK(create(&good, &h) == DH_OK && h != nullptr);
    destroy(h);
    destroy(nullptr);
    CHECK(create(nullptr, &h) == DH_EINVAL && create(&good, nullptr) == DH_EINVAL);
    int cases = 0;
    spoil([&](auto change) {
        Cfg c = good;
        change(c);
        h = junk;
        const int rc = create(&c, &h);
        if (rc != DH_EINVAL || h != nullptr) { printf("FAILED %s: invalid configuration %d gave %d\n", kind, cases, rc); failures++; }
        if (rc == DH_OK && h != junk) destroy(h);
        cases++;
    });
    int k = 1;
    for (;; k++) {
        g_alloc_fail_in = k;
        h = junk;
        const int rc = create(&good, &h);
        const bool fired = g_alloc_fail_in == 0;
        g_alloc_fail_in = 0;
        if (rc == DH_OK) { CHECK(!fired && h != nullptr && h != junk); destroy(h); break; }
        if (rc != DH_ENOMEM || h != nullptr || !fired) { printf("FAILED %s: allocation %d failing gave %d\n", kind, k, rc); failures++; break; }
        if (k > 1000) { printf("FAILED %s: still failing at allocation %d\n", kind, k); failures++; break; }
    }
    printf("%s: %d invalid configurations, %d allocations\n", kind, cases, k - 1);
}

static void null_handles() {
    float f[4] = {}; uint32_t u[4] = {}; uint64_t q[4] = {}; uint8_t b[4] = {}; size_t n = 0;
    const float* pf; const uint8_t* pb; const dh_event* pe; const uint32_t* pu; dh_event ev;
    dh_engine* e = nullptr;
    const int engine[] = {
        dh_engine_reset(e), dh_engine_set_slot_filter(e, 3), dh_engine_reset_channel(e, 0), dh_engine_reset_channels(e, b),
        dh_engine_set_slot_filter_channel(e, 0, 3), dh_engine_push(e, f, 4, 4), dh_engine_push_host(e, f, 4, 4),
        dh_engine_push_ragged(e, f, 4, u, 4), dh_engine_push_host_ragged(e, f, 4, u, 4), dh_engine_push_symbols(e, b, 4, u),
        dh_engine_filtered(e, &pf, &n), dh_engine_symbols(e, &pb, &n, &pu), dh_engine_frames(e, &pb, &n, &pu), dh_engine_events(e, &pe, &n, &pu),
        dh_engine_debug_header(e, 0, u), dh_engine_timing_stats(e, u, u), dh_engine_read_symbols(e, 0, b, &n), dh_engine_read_frames(e, 0, b, &n),
        dh_engine_read_events(e, 0, &ev, &n), dh_engine_read_filtered(e, 0, f, &n), dh_engine_timing_enable(e, 1),
        dh_engine_timing_read_split(e, f, u, u), dh_engine_timing_read(e, f, f, f, u), dh_engine_sync(e) };
    for (int rc : engine) CHECK(rc == DH_EINVAL);
    dh_channelizer* z = nullptr;
    dh_channelizer_power_config pc{};
    const int channelizer[] = {
        dh_channelizer_reset(z), dh_channelizer_retune(z, 0, 0), dh_channelizer_push(z, b, 0, f, 4, &n), dh_channelizer_push_host(z, b, 0, f, 4, &n),
        dh_channelizer_power_enable(z, &pc), dh_channelizer_set_squelch(z, 1.0f, 0.5f, 0), dh_channelizer_power_last(z, q, &n) };
    for (int rc : channelizer) CHECK(rc == DH_EINVAL);
    dh_preroll* p = nullptr;
    const int preroll[] = {
        dh_preroll_reset(p), dh_preroll_append(p, f, 4, 4, u), dh_preroll_total(p, q), dh_preroll_open_at(p, q),
        dh_preroll_gather(p, q, 0, 4, f, 4, u, q), dh_preroll_gather_device(p, q, 0, 4, f, 4, u) };
    for (int rc : preroll) CHECK(rc == DH_EINVAL);
    dh_outpack* o = nullptr;
    dh_outpack_header hdr;
    const dh_outpack_header* dh; const dh_outpack_entry* de;
    const int outpack[] = { dh_outpack_clear(o), dh_outpack_append(o, e, u, q, 0, 0), dh_outpack_read(o, &hdr, nullptr, nullptr, nullptr),
                            dh_outpack_device(o, &dh, &de, &pe, &pb) };
    for (int rc : outpack) CHECK(rc == DH_EINVAL);
    dh_monitor* m = nullptr;
    const int monitor[] = { dh_monitor_reset(m), dh_monitor_push(m, f, 4, 4, u, nullptr, nullptr), dh_monitor_push_packed(m, f, 4, 4, u, o),
                            dh_monitor_state(m, b, q), dh_monitor_total(m, q) };
    for (int rc : monitor) CHECK(rc == DH_EINVAL);
    CHECK(dh_monitor_engine(m, DH_PROTO_DMR) == nullptr && dh_monitor_scan_engine(m, 0) == nullptr);

    // ... and a live handle that is handed a null one
    dh_outpack_config oc = outpack_cfg();
    dh_monitor_config mc = monitor_cfg();
    CHECK(dh_outpack_create(&oc, &o) == DH_OK && dh_monitor_create(&mc, &m) == DH_OK);
    CHECK(dh_outpack_append(o, nullptr, u, q, 0, 0) == DH_EINVAL && dh_monitor_push_packed(m, f, 4, 4, u, nullptr) == DH_EINVAL);
    dh_monitor_destroy(m);
    dh_outpack_destroy(o);
}

int main() {
    lifecycle("dh_engine", engine_cfg(), dh_engine_create, dh_engine_destroy, [](auto bad) {
        bad([](dh_engine_config& c) { c.struct_size = sizeof(c) - 4; });
        bad([](dh_engine_config& c) { c.n_channels = 0; });
        bad([](dh_engine_config& c) { c.max_samples = 0; });
        bad([](dh_engine_config& c) { c.rrc = DH_RRC_CUSTOM + 1; });
        bad([](dh_engine_config& c) { c.rrc = DH_RRC_CUSTOM; });                                   // no table
        bad([](dh_engine_config& c) { c.rrc = DH_RRC_CUSTOM; c.rrc_taps = TAPS; c.rrc_nzeros = 15; c.rrc_gain = 0.0; });
        bad([](dh_engine_config& c) { c.rrc = DH_RRC_CUSTOM; c.rrc_taps = TAPS; c.rrc_nzeros = 15; c.rrc_gain = 1.0; c.flags = DH_FLAG_FAST_FIR; });
        bad([](dh_engine_config& c) { c.rrc = DH_RRC_CUSTOM; c.rrc_taps = TAPS; c.rrc_nzeros = 15; c.rrc_gain = 1.0; c.struct_size = DH_ENGINE_CONFIG_V1_SIZE; });
        bad([](dh_engine_config& c) { c.demod = 3; });
        bad([](dh_engine_config& c) { c.proto = DH_PROTO_SCAN + 1; });
        bad([](dh_engine_config& c) { c.sps = 2; });
        bad([](dh_engine_config& c) { c.sps = DH_MAX_SPS + 1; });
        bad([](dh_engine_config& c) { c.rrc = DH_RRC_NONE; c.demod = DH_DEMOD_NONE; c.proto = DH_PROTO_NONE; });
    });
    lifecycle("dh_channelizer", channelizer_cfg(), dh_channelizer_create, dh_channelizer_destroy, [](auto bad) {
        static float nan_taps[16];
        for (int i = 0; i < 16; i++) nan_taps[i] = TAPS[i];
        nan_taps[7] = NAN;
        bad([](dh_channelizer_config& c) { c.struct_size = offsetof(dh_channelizer_config, interpolation) - 4; });
        bad([](dh_channelizer_config& c) { c.decimation = 0; });
        bad([](dh_channelizer_config& c) { c.decimation = 1025; });
        bad([](dh_channelizer_config& c) { c.decimation = 128; c.interpolation = DH_CZ_MAX_L + 1; });
        bad([](dh_channelizer_config& c) { c.interpolation = 5; });                                 // L > D
        bad([](dh_channelizer_config& c) { c.interpolation = 2; });                                 // gcd(L, D) != 1
        bad([](dh_channelizer_config& c) { c.n_taps = 0; });
        bad([](dh_channelizer_config& c) { c.n_taps = 16385; });
        bad([](dh_channelizer_config& c) { c.n_channels = 0; });
        bad([](dh_channelizer_config& c) { c.n_channels = 65537; });
        bad([](dh_channelizer_config& c) { c.max_input = 0; });
        bad([](dh_channelizer_config& c) { c.max_input = (1u << 28) + 1; });
        bad([](dh_channelizer_config& c) { c.taps = nullptr; });
        bad([](dh_channelizer_config& c) { c.increments = nullptr; });
        bad([](dh_channelizer_config& c) { c.input_format = 0; });
        bad([](dh_channelizer_config& c) { c.output_mode = 0; });
        bad([](dh_channelizer_config& c) { c.output_mode = DH_CZ_IQ_F32; });                       // dcblock without FM
        bad([](dh_channelizer_config& c) { c.taps = nan_taps; });
    });
    lifecycle("dh_preroll", preroll_cfg(), dh_preroll_create, dh_preroll_destroy, [](auto bad) {
        bad([](dh_preroll_config& c) { c.struct_size = sizeof(c) - 4; });
        bad([](dh_preroll_config& c) { c.n_channels = 0; });
        bad([](dh_preroll_config& c) { c.n_channels = 65537; });
        bad([](dh_preroll_config& c) { c.depth = 0; });
        bad([](dh_preroll_config& c) { c.depth = (1u << 24) + 1; });
    });
    lifecycle("dh_outpack", outpack_cfg(), dh_outpack_create, dh_outpack_destroy, [](auto bad) {
        bad([](dh_outpack_config& c) { c.struct_size = sizeof(c) - 4; });
        bad([](dh_outpack_config& c) { c.max_entries = 0; });
        bad([](dh_outpack_config& c) { c.max_frame_bytes = 72; });                                  // no multiple of 16
        bad([](dh_outpack_config& c) { c.max_frame_bytes = (uint64_t) 1 << 36; });
    });
    lifecycle("dh_monitor", monitor_cfg(), dh_monitor_create, dh_monitor_destroy, [](auto bad) {
        bad([](dh_monitor_config& c) { c.struct_size = sizeof(c) - 4; });
        bad([](dh_monitor_config& c) { c.n_channels = 0; });
        bad([](dh_monitor_config& c) { c.n_channels = 65537; });
        bad([](dh_monitor_config& c) { c.max_samples = 0; });
        bad([](dh_monitor_config& c) { c.depth = 0; });
        bad([](dh_monitor_config& c) { c.depth = (1u << 24) + 1; });
        bad([](dh_monitor_config& c) { c.protos = 0; });
        bad([](dh_monitor_config& c) { c.protos = 0x40u; });                                        // DH_PROTO_SCAN is no protocol to decode
        bad([](dh_monitor_config& c) { c.protos = 0x3Fu; });                                        // nor is DH_PROTO_NONE
    });
    null_handles();
    printf(failures ? "handle lifecycle: %d checks failed\n" : "handle lifecycle: clean\n", failures);
    return failures ? 1 : 0;
}
