// mc_wl_kernel instantiations with per-walker windows (smolmc_set_wl_windows), NSLOT = 4: a translation unit of its
// own, so that no kernel of wl_n4.hip moves
#include "mc_wl.h"

int smolmc_launch_wl_win_4(smolmc_handle *h, const LeanParams &lp) { return launch_wl_win_nslot<4>(h, lp); }
