// raster_slab_rows.cpp -- prints, for the K given as its argument, the implementation's own DH_CZ_FOLD_SLAB_BYTES and
// dh_cz_fold_slab_rows(K') (digiham_amd/csrc/channelizer_core.hpp): the test of a push longer than one fold slab sizes its
// input from these, not from a copy of the constant.
#include <stdio.h>
#include <stdlib.h>

#include "../../digiham_amd/csrc/kernels_core.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const uint32_t K = (uint32_t) strtoul(argv[1], nullptr, 10);
    if (K < 2 || K > DH_CZ_MAX_RASTER) return 2;
    printf("%u %u\n", (unsigned) DH_CZ_FOLD_SLAB_BYTES, (unsigned) dh_cz_fold_slab_rows(dh_cz_tpad(K)));
    return 0;
}
