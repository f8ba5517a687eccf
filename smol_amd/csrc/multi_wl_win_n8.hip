// mc_lean_multi_kernel Wang-Landau instantiations with per-walker windows (smolmc_set_wl_windows), NSLOT = 8: a
// translation unit of its own, so that no kernel of multi_wl_n8.hip moves
#include "mc_lean_multi.h"

int smolmc_launch_multi_wl_win_8(smolmc_handle *h, const LeanParams &lp) { return launch_multi_wl_win_nslot<8>(h, lp); }
