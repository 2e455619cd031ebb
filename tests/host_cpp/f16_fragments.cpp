// f16_fragments.cpp -- prints what the host hands the split-f16 FIR (digiham_amd/csrc/dsp_core.hpp: dh_f16_tap_fragments,
// dh_f16_error_coefficient) for the three kinds of engine: the wide filter in the one-chain form, the wide filter of an engine
// that keeps its filtered samples, the narrow filter.  One line per kind:
//   <name> <one_chain> <ok> <coefficient, float bits> <number of words> <the fragment words, hex>
// tests/test_fir_one_chain.py rebuilds the words from the tap tables and compares.
#include <stdio.h>
#include <string.h>

#include "../../digiham_amd/csrc/kernels_core.hpp"
#include "../../digiham_amd/csrc/rrc_taps.h"

static void show(const char* name, int narrow, int keepf) {
    float full[DH_RRC_MAX_TAPS];
    dh_rrc_expand_taps(narrow, full);
    const uint32_t nz = narrow ? DH_RRC_NARROW_NZEROS : DH_RRC_WIDE_NZEROS;
    const double gain = narrow ? DH_RRC_NARROW_GAIN : DH_RRC_WIDE_GAIN;
    static DhF16Taps F;
    memset(&F, 0, sizeof(F));
    const bool one = dh_f16_one_chain(nz, keepf);
    const bool ok = dh_f16_tap_fragments(full, nz, one, F);          // (reads the first half of the table, as an engine's copy holds it)
    const float coef = dh_f16_error_coefficient(F, nz, gain);
    uint32_t bits;
    memcpy(&bits, &coef, 4);
    const uint32_t words = 2u * F.ksteps * DH_WAVE * 4u;
    printf("%s %d %d %08x %u", name, one ? 1 : 0, ok ? 1 : 0, (unsigned) bits, (unsigned) words);
    const uint32_t* w = &F.frag[0][0][0];
    for (uint32_t i = 0; i < words; i++) printf(" %08x", (unsigned) w[i]);
    printf("\n");
}

int main() {
    show("wide", 0, 0);
    show("wide_keep", 0, 1);
    show("wide_keep_fast", 0, 2);
    show("narrow", 1, 0);
    return 0;
}
