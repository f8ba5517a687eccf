// mc_lean_multi_kernel Wang-Landau instantiations (several site classes / update_period > 1), NSLOT = 4
#include "mc_lean_multi.h"

int smolmc_launch_multi_wl_4(smolmc_handle *h, const LeanParams &lp) { return launch_multi_wl_nslot<4, MV_WL>(h, lp); }
