// go2sim_wells.hip -- the scan handle of the stairwell env (include/go2sim_wells.h): the critic's nx x ny body-frame height scan, the assembly of the
// wider privileged row and the alive term, on gfx950.  The header states the law and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/go2sim_detmath.h"
#include "../../include/go2sim_wells.h"
#include "go2sim_wells_dev.h"

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_wells: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

constexpr int WAVE = 64, WG = 256, ENVS_PER_WG = WG / WAVE;
constexpr int EXTRA = GO2SIM_WELLS_PRIV_EXTRA;

// what the kernels see of one handle
struct WellsDev {
  WellField F;
  const float *lx, *ly;            // [npts] the sample points, point k = i * ny + j
  float *alive_sum, *alive_ep;     // [n_envs]
  int* alive_steps;                // [n_envs]
  int n_envs, npts;
  float inc, dt;
};

struct Pose {
  const float *pos, *quat;
  long long pcs, pes, qcs, qes;
};

// "alive_ep[b] = alive_sum[b] / (f32(max(alive_steps[b], 1)) * f32(dt))", then both := 0
__device__ __forceinline__ void alive_hand_over(const WellsDev& D, int b, float sum, int steps) {
  const float ep_steps = (float)(steps < 1 ? 1 : steps);
  D.alive_ep[b] = sum / (ep_steps * D.dt);
  D.alive_sum[b] = 0.0f;
  D.alive_steps[b] = 0;
}

// One wavefront per env.  Every lane holds the env's pose, yaw, sine and cosine (wave-uniform values); lane t owns the columns t, t + 64, ... of the output
// row (a copied column below n_copy, point col - n_copy from there on), so that consecutive lanes write consecutive floats of the row.  Lane 0: the alive term.
__global__ __launch_bounds__(WG) void k_wells_step(WellsDev D, Pose P, const uint8_t* __restrict__ reset, const float* __restrict__ priv, int n_in,
                                                   float* __restrict__ priv_out, float* __restrict__ rew) {
  const int b = blockIdx.x * ENVS_PER_WG + (threadIdx.x / WAVE), t = threadIdx.x % WAVE;
  if (b >= D.n_envs) return;
  const int n_copy = priv ? n_in + EXTRA : 0;                       // without the inner row the output is the scan alone
  const int w = n_copy + D.npts;
  const float px = P.pos[(size_t)b * P.pes], py = P.pos[P.pcs + (size_t)b * P.pes], pz = P.pos[2 * P.pcs + (size_t)b * P.pes];
  const float qw = P.quat[(size_t)b * P.qes], qx = P.quat[P.qcs + (size_t)b * P.qes], qy = P.quat[2 * P.qcs + (size_t)b * P.qes],
              qz = P.quat[3 * P.qcs + (size_t)b * P.qes];
  const float yaw = dm_atan2(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
  float s, c;
  dm_sincos(yaw, &s, &c);
  float* __restrict__ prow = priv_out + (size_t)b * w;
  const float* __restrict__ pin = priv ? priv + (size_t)b * n_copy : nullptr;
  for (int col = t; col < w; col += WAVE) {
    float v;
    if (col < n_copy) v = pin[col];
    else { const int k = col - n_copy; v = well_scan_point(D.F, px, py, pz, s, c, D.lx[k], D.ly[k]); }
    prow[col] = v;
  }
  if (t == 0 && rew) {                                             // this lane alone reads and writes the env's cells
    rew[b] = rew[b] + D.inc;
    const float sum = D.alive_sum[b] + D.inc;
    const int steps = D.alive_steps[b] + 1;
    if (reset && reset[b]) alive_hand_over(D, b, sum, steps);
    else { D.alive_sum[b] = sum; D.alive_steps[b] = steps; }
  }
}

__global__ __launch_bounds__(WG) void k_wells_clear(WellsDev D, const int* __restrict__ idx, int n_sel) {
  const int r = blockIdx.x * WG + threadIdx.x;
  if (r >= (idx ? n_sel : D.n_envs)) return;
  const int b = idx ? idx[r] : r;
  if (b >= 0 && b < D.n_envs) alive_hand_over(D, b, D.alive_sum[b], D.alive_steps[b]);
}

}  // namespace

struct go2sim_wells {
  int device = 0;
  WellsDev dev = {};
  float* hf = nullptr;
  float* pts = nullptr;      // lx | ly
  float* alive = nullptr;    // alive_sum | alive_ep
  int* steps = nullptr;
  int n_levels = 1;
};

extern "C" {

int go2sim_wells_create(int device, const go2sim_wells_cfg_t* cfg, const int16_t* hf, const float* xs, const float* ys, go2sim_wells_t** out) {
  if (!out || !cfg || !hf || !xs || !ys) return GO2SIM_E_BADARG;
  const go2sim_wells_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.nx < 1 || c.nx > GO2SIM_WELLS_AXIS_MAX || c.ny < 1 || c.ny > GO2SIM_WELLS_AXIS_MAX || c.n_levels < 1 || c.n_levels > GO2SIM_WELLS_LEVELS_MAX)
    return GO2SIM_E_BADARG;
  if (c.hf_rows < 1 || c.hf_cols < 1 || (long long)c.hf_rows * c.hf_cols > (1LL << 30) || !(c.horizontal_scale > 0.0) || !(c.dt > 0.0)) return GO2SIM_E_BADARG;
  const double all[] = {c.origin_x, c.origin_y, c.vertical_scale, c.alive_scale};
  for (double v : all)
    if (v != v) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(device));
  go2sim_wells* h = new (std::nothrow) go2sim_wells();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  h->n_levels = c.n_levels;
  const size_t cells = (size_t)c.hf_rows * c.hf_cols, npts = (size_t)c.nx * c.ny, n = (size_t)c.n_envs;
  if (hipMalloc((void**)&h->hf, cells * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->pts, 2 * npts * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&h->alive, 2 * n * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->steps, n * sizeof(int)) != hipSuccess) {
    go2sim_wells_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  std::vector<float> hfm(cells), pts(2 * npts);
  for (size_t k = 0; k < cells; ++k) hfm[k] = (float)hf[k] * (float)c.vertical_scale;      // as go2sim_set_terrain forms the env's own copy
  for (int i = 0; i < c.nx; ++i)
    for (int j = 0; j < c.ny; ++j) { pts[(size_t)i * c.ny + j] = xs[i]; pts[npts + (size_t)i * c.ny + j] = ys[j]; }
  if (hipMemcpy(h->hf, hfm.data(), cells * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->pts, pts.data(), 2 * npts * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemset(h->alive, 0, 2 * n * sizeof(float)) != hipSuccess ||
      hipMemset(h->steps, 0, n * sizeof(int)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    go2sim_wells_destroy(h);
    return GO2SIM_E_HIP;
  }
  WellsDev& D = h->dev;
  D.F = WellField{h->hf, c.hf_rows, c.hf_cols, (float)c.origin_x, (float)c.origin_y, (float)c.horizontal_scale};
  D.lx = h->pts; D.ly = h->pts + npts; D.alive_sum = h->alive; D.alive_ep = h->alive + n; D.alive_steps = h->steps;
  D.n_envs = c.n_envs; D.npts = (int)npts;
  D.inc = (float)(c.alive_scale * c.dt); D.dt = (float)c.dt;
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_wells_destroy(go2sim_wells_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree(h->hf); (void)hipFree(h->pts); (void)hipFree(h->alive); (void)hipFree(h->steps);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_wells_clear(go2sim_wells_t* h, const int* envs_idx, int n_sel, void* stream) {
  if (!h || (envs_idx && n_sel < 0)) return GO2SIM_E_BADARG;
  const int total = envs_idx ? n_sel : h->dev.n_envs;
  if (total == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL(k_wells_clear, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->dev, envs_idx, n_sel);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_wells_get_alive(go2sim_wells_t* h, float* sum, int32_t* steps, void* stream) {
  if (!h || !sum || !steps) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(sum, h->dev.alive_sum, (size_t)h->dev.n_envs * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(steps, h->dev.alive_steps, (size_t)h->dev.n_envs * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return GO2SIM_E_OK;
}

int go2sim_wells_set_alive(go2sim_wells_t* h, const float* sum, const int32_t* steps, void* stream) {
  if (!h || !sum || !steps) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(h->dev.alive_sum, sum, (size_t)h->dev.n_envs * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dev.alive_steps, steps, (size_t)h->dev.n_envs * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                          // the sources are the caller's host memory
  return GO2SIM_E_OK;
}

int go2sim_wells_alive_ep(go2sim_wells_t* h, const float** alive_ep_dev, float* inc) {
  if (!h || !alive_ep_dev || !inc) return GO2SIM_E_BADARG;
  *alive_ep_dev = h->dev.alive_ep; *inc = h->dev.inc;
  return GO2SIM_E_OK;
}

int go2sim_wells_step(go2sim_wells_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                      long long quat_comp_stride, long long quat_env_stride, const uint8_t* reset, const float* priv, int n_in, float* priv_out,
                      float* rew, void* stream) {
  if (!h || n != h->dev.n_envs || !pos || !quat || !priv_out || n_in < 0 || n_in > (1 << 20)) return GO2SIM_E_BADARG;
  if (pos_comp_stride < 0 || pos_env_stride < 0 || quat_comp_stride < 0 || quat_env_stride < 0) return GO2SIM_E_BADARG;
  if ((priv == nullptr) != (n_in == 0) || (const float*)priv_out == priv) return GO2SIM_E_BADARG;
  const Pose P = {pos, quat, pos_comp_stride, pos_env_stride, quat_comp_stride, quat_env_stride};
  hipLaunchKernelGGL(k_wells_step, dim3((n + ENVS_PER_WG - 1) / ENVS_PER_WG), dim3(WG), 0, (hipStream_t)stream, h->dev, P, reset, priv, n_in, priv_out, rew);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
