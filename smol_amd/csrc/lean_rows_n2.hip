// mc_lean_kernel instantiations of the solo rows variants (per-slot gather widths, index rows by LDS address) for NSLOT = 2
#include "mc_lean.h"

int smolmc_launch_lean_rows_2(smolmc_handle *h, const LeanParams &lp) {
    return launch_lean_rows_nslot<2>(h, lp);
}
