// go2sim_tiles.hip -- the ground-height query of the rough-terrain walk env on arbitrary points (include/go2sim_tiles.h), on gfx950.  The header states
// the law; the device function is the one the env step runs (csrc/go2sim_tiles_dev.h).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/go2sim_tiles.h"
#include "go2sim_tiles_dev.h"

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_tiles: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

constexpr int WG = 256;

// one lane per point; consecutive lanes read consecutive (x, y) pairs and write consecutive heights
__global__ __launch_bounds__(WG) void k_tiles_query(TileField T, const float* __restrict__ xy, int n, float* __restrict__ out) {
  const int k = blockIdx.x * WG + threadIdx.x;
  if (k >= n) return;
  out[k] = tile_ground_height(T, xy[2 * (size_t)k], xy[2 * (size_t)k + 1]);
}

}  // namespace

extern "C" int go2sim_tiles_query(go2sim_t* h, const float* xy_dev, int n, float* out_dev, void* stream) {
  if (!h || n < 0 || (n > 0 && (!xy_dev || !out_dev))) return GO2SIM_E_BADARG;
  TileField T;
  float org[2];
  { const int rc = go2sim_tiles_env_field(h, &T.hf, &T.rows, &T.cols, org, &T.hs); if (rc != GO2SIM_E_OK) return rc; }
  T.ox = org[0]; T.oy = org[1];
  if (n == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL(k_tiles_query, dim3((n + WG - 1) / WG), dim3(WG), 0, (hipStream_t)stream, T, xy_dev, n, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
