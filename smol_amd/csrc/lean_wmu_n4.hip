// mc_lean_kernel / mc_table_kernel instantiations with per-walker chemical potentials (smolmc_set_walker_mu), NSLOT = 4:
// the plain, biased (MCBias) and KF families
#include "mc_lean.h"

int smolmc_launch_lean_wmu_4(smolmc_handle *h, const LeanParams &lp) {
    return launch_lean_wmu_nslot<4>(h, lp);
}
int smolmc_launch_lean_bias_wmu_4(smolmc_handle *h, const LeanParams &lp) {
    return launch_lean_bias_wmu_nslot<4>(h, lp);
}
int smolmc_launch_lean_corr_wmu_4(smolmc_handle *h, const LeanParams &lp) {
    return launch_lean_corr_wmu_nslot<4>(h, lp);
}
int smolmc_launch_table_bias_wmu_4(smolmc_handle *h, const LeanParams &lp) {
    return launch_table_bias_wmu_nslot<4>(h, lp);
}
