// mc_lean_multi_kernel / mc_table_multi_kernel instantiations with per-walker chemical potentials
// (smolmc_set_walker_mu), NSLOT = 8: the plain and the biased (MCBias) families
#include "mc_lean_multi.h"

int smolmc_launch_multi_wmu_8(smolmc_handle *h, const LeanParams &lp) {
    return launch_multi_wmu_nslot<8>(h, lp);
}
int smolmc_launch_multi_bias_wmu_8(smolmc_handle *h, const LeanParams &lp) {
    return launch_multi_bias_wmu_nslot<8>(h, lp);
}
int smolmc_launch_multi_table_bias_wmu_8(smolmc_handle *h, const LeanParams &lp) {
    return launch_table_multi_bias_wmu_nslot<8>(h, lp);
}
