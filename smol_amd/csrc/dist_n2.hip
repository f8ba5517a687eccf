// mc_dist_kernel instantiation (distance objective, native Philox stream), NSLOT = 2
#include "mc_dist.h"

int smolmc_launch_dist_2(smolmc_handle *h, const DistParams &P) { return launch_dist_nslot<2, false>(h, P); }
