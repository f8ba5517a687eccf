// mc_dist_kernel instantiation (distance objective, native Philox stream), NSLOT = 4
#include "mc_dist.h"

int smolmc_launch_dist_4(smolmc_handle *h, const DistParams &P) { return launch_dist_nslot<4, false>(h, P); }
