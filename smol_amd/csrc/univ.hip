// mc_univ_kernel instantiations (the universal backstop kernel, mc_univ.h)
#include "mc_univ.h"

int smolmc_univ_selector(const smolmc_handle *h, const UParams &up) {
    const bool table = h->cfg.step_type == SMOLMC_STEP_TABLE_FLIP, k1 = up.all_k1 != 0;
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 256;
    const bool dense = (long long)h->R > 2ll * 4 * cus; // more than two walkers per SIMD
    return (up.dict_lds ? UNIV_SEL_DICT : 0) | (up.occ_lds ? UNIV_SEL_OCC_LDS : 0) | (k1 ? UNIV_SEL_K1 : 0) |
           (table ? UNIV_SEL_TABLE : 0) | (dense ? UNIV_SEL_DENSE : 0);
}

int smolmc_launch_univ(smolmc_handle *h, const UParams &up, int replay) {
    const int wpb = h->univ_wpb;
    const size_t lds = (size_t)up.lds_shared + (size_t)up.lds_per_wave * wpb;
    const int sel = smolmc_univ_selector(h, up);
    void (*kern)(const UParams, const int) = (sel & UNIV_SEL_DICT) ? smolmc_univ_kernel_dict(sel & 15) : univ_select<false>(sel & 15);
    const unsigned grid = (unsigned)((h->R + wpb - 1) / wpb);
    return launch_timed(h, kern, dim3(grid), dim3(64 * wpb), lds, up, replay);
}
