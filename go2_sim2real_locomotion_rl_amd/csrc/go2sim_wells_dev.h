// go2sim_wells_dev.h -- the spawn draw of the stairwell env (include/go2sim_wells.h states the law; the name here follows it), for csrc/go2sim.hip
// (k_env_well_spawn).  The scan's heightfield lookup is in csrc/go2sim_envlaunch_dev.h with the other launches'.
#ifndef GO2SIM_WELLS_DEV_H
#define GO2SIM_WELLS_DEV_H
#include <hip/hip_runtime.h>

#include "../../include/go2sim_wells.h"

// "The well spawn": one coordinate; centre = the configured double, u01 = dm_u01 of the coordinate's word
__host__ __device__ inline float well_spawn_coord(double centre, float u01) {
  const double a = -GO2SIM_WELLS_SPAWN_JITTER, b = GO2SIM_WELLS_SPAWN_JITTER;
  return (float)(centre + (a + (b - a) * (double)u01));
}

#endif
