// mc_dist_kernel instantiation (distance objective, host-provided steps and uniforms), NSLOT = 4
#include "mc_dist.h"

int smolmc_launch_dist_replay_4(smolmc_handle *h, const DistParams &P) { return launch_dist_nslot<4, true>(h, P); }
