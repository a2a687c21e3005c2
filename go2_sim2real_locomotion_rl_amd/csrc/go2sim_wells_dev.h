// go2sim_wells_dev.h -- the device functions of the stairwell env (include/go2sim_wells.h states the law; the names here follow it): the heightfield
// lookup of the scan and the spawn draws of one env.  Shared by csrc/go2sim.hip (k_env_well_spawn) and csrc/go2sim_wells.hip (k_wells_step).
#ifndef GO2SIM_WELLS_DEV_H
#define GO2SIM_WELLS_DEV_H
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/go2sim_detmath.h"
#include "../../include/go2sim_wells.h"

// what the device functions see of the heightfield
struct WellField {
  const float* hf;          // [rows][cols] metres, rows along world x
  int rows, cols;           // >= 1 each
  float ox, oy, hs;         // world position of cell (0, 0), cell size
};

// trunc toward zero, then clamp to [0, n - 1], by comparisons a NaN fails (it selects 0): never an index outside the field
__device__ __forceinline__ int well_cell_index(float q, int n) {
  if (!(q >= 1.0f)) return 0;                    // negatives, [0, 1) and NaN
  if (q >= (float)(n - 1)) return n - 1;         // +inf included
  return (int)q;
}

// "The scan": one point of env (px, py, pz) with yaw sine s and cosine c
__device__ __forceinline__ float well_scan_point(const WellField& F, float px, float py, float pz, float s, float c, float lx, float ly) {
  const float wx = px + c * lx - s * ly;
  const float wy = py + s * lx + c * ly;
  const int col = well_cell_index((wx - F.ox) / F.hs, F.rows);
  const int row = well_cell_index((wy - F.oy) / F.hs, F.cols);
  return F.hf[(size_t)col * F.cols + row] - pz;
}

// "The well spawn": one coordinate; centre = the configured double, u01 = dm_u01 of the coordinate's word
__host__ __device__ inline float well_spawn_coord(double centre, float u01) {
  const double a = -GO2SIM_WELLS_SPAWN_JITTER, b = GO2SIM_WELLS_SPAWN_JITTER;
  return (float)(centre + (a + (b - a) * (double)u01));
}

#endif
