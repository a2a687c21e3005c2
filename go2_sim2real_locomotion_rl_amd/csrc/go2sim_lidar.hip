// go2sim_lidar.hip -- the LIDAR terrain scan (include/go2sim_lidar.h): the actor's noisy body-frame height profile with its one-step memory, the critic's
// clean one, and the assembly of the wider observation rows, on gfx950.  The header states the law, the draw layout and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/go2sim_detmath.h"
#include "../../include/go2sim_lidar.h"

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_lidar: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

constexpr int WAVE = 64, WG = 256, ENVS_PER_WG = WG / WAVE;
constexpr int EXTRA = GO2SIM_LIDAR_PRIV_EXTRA;

// what the kernels see of one handle
struct LidarDev {
  const float* hf;                 // [rows][cols] metres
  const float *ax, *ay, *cx, *cy;  // the sample points
  float* stored;                   // [n_envs][n_actor]
  int rows, cols, n_envs, n_actor, n_critic;
  float ox, oy, hs, clip, scale;
  float noise_std, offset_std;
  double dropout_prob, latency_prob, blackout_prob;     // multiplied with L in float64, then rounded (the header's thresholds)
  double phase1, gate;
  int dr_schedule, curriculum_enabled;
  uint32_t k0, k1;                 // the seed's words
};

struct Pose {
  const float *pos, *quat;
  long long pcs, pes, qcs, qes;
};

// _get_dr_level, go2_env_stair_lidar.py:1197-1220
__device__ __forceinline__ double dr_level(const LidarDev& D, double t) {
  if (!D.dr_schedule) return t;
  if (t < D.gate) return D.phase1;
  double den = 1.0 - D.gate;
  if (den < 1e-6) den = 1e-6;
  double pr = (t - D.gate) / den;
  pr = pr < 0.0 ? 0.0 : (pr > 1.0 ? 1.0 : pr);
  return D.phase1 + (1.0 - D.phase1) * pr;
}

// trunc toward zero, then clamp to [0, n - 1], by comparisons a NaN fails (it selects 0): never an index outside the field
__device__ __forceinline__ int cell_index(float q, int n) {
  if (!(q >= 1.0f)) return 0;                    // negatives, [0, 1) and NaN
  if (q >= (float)(n - 1)) return n - 1;         // +inf included
  return (int)q;
}

__device__ __forceinline__ float raw_height(const LidarDev& D, float px, float py, float pz, float s, float c, float lx, float ly) {
  const float wx = px + c * lx - s * ly;
  const float wy = py + s * lx + c * ly;
  const int col = cell_index((wx - D.ox) / D.hs, D.rows);
  const int row = cell_index((wy - D.oy) / D.hs, D.cols);
  return D.hf[(size_t)col * D.cols + row] - pz;
}

__device__ __forceinline__ float clip_scale(const LidarDev& D, float v) {
  v = v < -D.clip ? -D.clip : (v > D.clip ? D.clip : v);     // a NaN stays a NaN, as torch.clamp leaves it
  return v * D.scale;
}

// One wavefront per env.  Every lane holds the env's pose, yaw, sine, cosine, level and env-level draws (wave-uniform values); lane t owns the points t, t + 64, ...
// and the columns t, t + 64, ... of the copied inner rows, so that consecutive lanes write consecutive floats of a row.
__global__ __launch_bounds__(WG) void k_lidar_step(LidarDev D, Pose P, const uint8_t* __restrict__ reset, const double* __restrict__ level, uint32_t step,
                                                   const float* __restrict__ obs, const float* __restrict__ priv, int n_in, float* __restrict__ obs_out,
                                                   float* __restrict__ priv_out) {
  const int b = blockIdx.x * ENVS_PER_WG + (threadIdx.x / WAVE), t = threadIdx.x % WAVE;
  if (b >= D.n_envs) return;
  const int na = D.n_actor, nc = D.n_critic;
  const int extra = obs ? EXTRA : 0;                              // without inner rows the outputs are the scans alone
  const int w_obs = n_in + na, w_priv = n_in + na + extra + nc;
  float* __restrict__ orow = obs_out + (size_t)b * w_obs;
  float* __restrict__ prow = priv_out + (size_t)b * w_priv;
  if (obs) {
    const float* __restrict__ oi = obs + (size_t)b * n_in;
    const float* __restrict__ pi = priv + (size_t)b * (n_in + EXTRA);
    for (int i = t; i < n_in; i += WAVE) { orow[i] = oi[i]; prow[i] = pi[i]; }
    for (int i = t; i < EXTRA; i += WAVE) prow[n_in + na + i] = pi[n_in + i];
  }
  const bool was_reset = reset && reset[b];
  if (was_reset) {
    for (int k = t; k < na; k += WAVE) { D.stored[(size_t)b * na + k] = 0.0f; orow[n_in + k] = 0.0f; prow[n_in + k] = 0.0f; }
    for (int k = t; k < nc; k += WAVE) prow[n_in + na + extra + k] = 0.0f;
    return;
  }
  const float px = P.pos[(size_t)b * P.pes], py = P.pos[P.pcs + (size_t)b * P.pes], pz = P.pos[2 * P.pcs + (size_t)b * P.pes];
  const float qw = P.quat[(size_t)b * P.qes], qx = P.quat[P.qcs + (size_t)b * P.qes], qy = P.quat[2 * P.qcs + (size_t)b * P.qes],
              qz = P.quat[3 * P.qcs + (size_t)b * P.qes];
  const float yaw = dm_atan2(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
  float s, c;
  dm_sincos(yaw, &s, &c);
  for (int k = t; k < nc; k += WAVE) prow[n_in + na + extra + k] = clip_scale(D, raw_height(D, px, py, pz, s, c, D.cx[k], D.cy[k]));
  if (na == 0) return;
  const double L = dr_level(D, D.curriculum_enabled ? *level : 1.0);
  const bool on = L > 0.0;
  const float Lf = (float)L;
  const bool do_noise = on && D.noise_std > 0.0f, do_drop = on && D.dropout_prob > 0.0, do_off = on && D.offset_std > 0.0f;
  const bool do_lat = on && D.latency_prob > 0.0, do_black = on && D.blackout_prob > 0.0;
  bool stale = false, black = false;
  float off = 0.0f;
  if (do_off || do_lat || do_black) {
    const dm_u4 r = dm_philox((uint32_t)b, step, GO2SIM_LIDAR_RNG_PURPOSE, 0u, D.k0, D.k1);
    float zb, z1;
    dm_normal2(r.v[2], r.v[3], &zb, &z1);
    off = (zb * D.offset_std) * Lf;
    stale = do_lat && dm_u01(r.v[0]) < (float)(D.latency_prob * L);
    black = do_black && dm_u01(r.v[1]) < (float)(D.blackout_prob * L);
  }
  const float drop_thr = (float)(D.dropout_prob * L);
  for (int k = t; k < na; k += WAVE) {
    float v = raw_height(D, px, py, pz, s, c, D.ax[k], D.ay[k]);
    if (do_noise || do_drop) {
      const dm_u4 r = dm_philox((uint32_t)b, step, GO2SIM_LIDAR_RNG_PURPOSE, 1u + (uint32_t)(k >> 1), D.k0, D.k1);
      if (do_noise) {
        float z0, z1;
        dm_normal2(r.v[0], r.v[1], &z0, &z1);
        v = v + (((k & 1) ? z1 : z0) * D.noise_std) * Lf;
      }
      if (do_drop && dm_u01(r.v[2 + (k & 1)]) < drop_thr) v = 0.0f;
    }
    if (do_off) v = v + off;
    float* st = D.stored + (size_t)b * na + k;                     // this lane alone reads and writes the cell
    if (stale) v = *st;
    if (black) v = 0.0f;
    v = clip_scale(D, v);
    *st = v; orow[n_in + k] = v; prow[n_in + k] = v;
  }
}

__global__ __launch_bounds__(WG) void k_lidar_clear(float* __restrict__ stored, int n_envs, int n_actor, const int* __restrict__ idx, int n_sel) {
  const long long i = (long long)blockIdx.x * WG + threadIdx.x, total = (long long)(idx ? n_sel : n_envs) * n_actor;
  if (i >= total) return;
  const int r = (int)(i / n_actor), k = (int)(i - (long long)r * n_actor);
  const int b = idx ? idx[r] : r;
  if (b >= 0 && b < n_envs) stored[(size_t)b * n_actor + k] = 0.0f;
}

}  // namespace

struct go2sim_lidar {
  int device = 0;
  LidarDev dev = {};
  float* hf = nullptr;
  float* pts = nullptr;     // ax | ay | cx | cy
  float* stored = nullptr;
  uint32_t step = 0;
};

extern "C" {

int go2sim_lidar_create(int device, const go2sim_lidar_cfg_t* cfg, const int16_t* hf, const float* actor_xy, const float* critic_xy, uint64_t seed,
                        go2sim_lidar_t** out) {
  if (!out || !cfg || !hf) return GO2SIM_E_BADARG;
  const go2sim_lidar_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.n_actor < 0 || c.n_critic < 0 || c.n_actor + c.n_critic == 0 || c.n_actor > (1 << 16) || c.n_critic > (1 << 16)) return GO2SIM_E_BADARG;
  if (c.hf_rows < 1 || c.hf_cols < 1 || (long long)c.hf_rows * c.hf_cols > (1LL << 30) || !(c.horizontal_scale > 0.0) || !(c.height_clip >= 0.0)) return GO2SIM_E_BADARG;
  if ((c.n_actor > 0 && !actor_xy) || (c.n_critic > 0 && !critic_xy)) return GO2SIM_E_BADARG;
  const double all[] = {c.height_noise_std, c.dropout_prob, c.vertical_offset_std, c.latency_prob, c.full_blackout_prob, c.height_scale, c.dr_phase1_level,
                        c.dr_terrain_gate, c.origin_x, c.origin_y, c.vertical_scale};
  for (double v : all)
    if (v != v) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(device));
  go2sim_lidar* h = new (std::nothrow) go2sim_lidar();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  const size_t cells = (size_t)c.hf_rows * c.hf_cols, npts = 2 * ((size_t)c.n_actor + c.n_critic), nst = (size_t)c.n_envs * (c.n_actor > 0 ? c.n_actor : 1);
  if (hipMalloc((void**)&h->hf, cells * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->pts, npts * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&h->stored, nst * sizeof(float)) != hipSuccess) {
    go2sim_lidar_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  std::vector<float> hfm(cells), pts(npts);
  for (size_t k = 0; k < cells; ++k) hfm[k] = (float)hf[k] * (float)c.vertical_scale;      // as go2sim_set_terrain forms the env's own copy
  for (int k = 0; k < 2 * c.n_actor; ++k) pts[k] = actor_xy[k];
  for (int k = 0; k < 2 * c.n_critic; ++k) pts[2 * (size_t)c.n_actor + k] = critic_xy[k];
  if (hipMemcpy(h->hf, hfm.data(), cells * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->pts, pts.data(), npts * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemset(h->stored, 0, nst * sizeof(float)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    go2sim_lidar_destroy(h);
    return GO2SIM_E_HIP;
  }
  LidarDev& D = h->dev;
  D.hf = h->hf; D.ax = h->pts; D.ay = D.ax + c.n_actor; D.cx = D.ay + c.n_actor; D.cy = D.cx + c.n_critic; D.stored = h->stored;
  D.rows = c.hf_rows; D.cols = c.hf_cols; D.n_envs = c.n_envs; D.n_actor = c.n_actor; D.n_critic = c.n_critic;
  D.ox = (float)c.origin_x; D.oy = (float)c.origin_y; D.hs = (float)c.horizontal_scale; D.clip = (float)c.height_clip; D.scale = (float)c.height_scale;
  D.noise_std = (float)c.height_noise_std; D.offset_std = (float)c.vertical_offset_std;
  D.dropout_prob = c.dropout_prob; D.latency_prob = c.latency_prob; D.blackout_prob = c.full_blackout_prob;
  D.phase1 = c.dr_phase1_level; D.gate = c.dr_terrain_gate; D.dr_schedule = c.dr_schedule != 0; D.curriculum_enabled = c.curriculum_enabled != 0;
  D.k0 = (uint32_t)seed; D.k1 = (uint32_t)(seed >> 32);
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_lidar_destroy(go2sim_lidar_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree(h->hf); (void)hipFree(h->pts); (void)hipFree(h->stored);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_lidar_get_step(go2sim_lidar_t* h, uint32_t* step) {
  if (!h || !step) return GO2SIM_E_BADARG;
  *step = h->step;
  return GO2SIM_E_OK;
}

int go2sim_lidar_set_step(go2sim_lidar_t* h, uint32_t step) {
  if (!h) return GO2SIM_E_BADARG;
  h->step = step;
  return GO2SIM_E_OK;
}

int go2sim_lidar_clear(go2sim_lidar_t* h, const int* envs_idx, int n_sel, void* stream) {
  if (!h || (envs_idx && n_sel < 0)) return GO2SIM_E_BADARG;
  const long long total = (long long)(envs_idx ? n_sel : h->dev.n_envs) * h->dev.n_actor;
  if (total == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL(k_lidar_clear, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->stored, h->dev.n_envs, h->dev.n_actor, envs_idx, n_sel);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_lidar_get_scan(go2sim_lidar_t* h, float* scan, void* stream) {
  if (!h || !scan) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (h->dev.n_actor > 0) HIPCHK(hipMemcpyAsync(scan, h->stored, (size_t)h->dev.n_envs * h->dev.n_actor * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return GO2SIM_E_OK;
}

int go2sim_lidar_set_scan(go2sim_lidar_t* h, const float* scan, void* stream) {
  if (!h || !scan) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (h->dev.n_actor > 0) HIPCHK(hipMemcpyAsync(h->stored, scan, (size_t)h->dev.n_envs * h->dev.n_actor * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                          // the source is the caller's host memory
  return GO2SIM_E_OK;
}

int go2sim_lidar_step(go2sim_lidar_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                      long long quat_comp_stride, long long quat_env_stride, const uint8_t* reset, const double* level, const float* obs, const float* priv,
                      int n_in, float* obs_out, float* priv_out, void* stream) {
  if (!h || n != h->dev.n_envs || !pos || !quat || !obs_out || !priv_out || n_in < 0 || n_in > (1 << 20)) return GO2SIM_E_BADARG;
  if (pos_comp_stride < 0 || pos_env_stride < 0 || quat_comp_stride < 0 || quat_env_stride < 0) return GO2SIM_E_BADARG;
  if (h->dev.curriculum_enabled && !level) return GO2SIM_E_BADARG;
  if ((obs == nullptr) != (priv == nullptr) || (obs == nullptr) != (n_in == 0)) return GO2SIM_E_BADARG;
  if (obs_out == priv_out || (obs && ((const float*)obs_out == obs || (const float*)obs_out == priv || (const float*)priv_out == obs || (const float*)priv_out == priv)))
    return GO2SIM_E_BADARG;
  const Pose P = {pos, quat, pos_comp_stride, pos_env_stride, quat_comp_stride, quat_env_stride};
  hipLaunchKernelGGL(k_lidar_step, dim3((n + ENVS_PER_WG - 1) / ENVS_PER_WG), dim3(WG), 0, (hipStream_t)stream, h->dev, P, reset, level, h->step, obs, priv, n_in,
                     obs_out, priv_out);
  HIPCHK(hipGetLastError());
  h->step += 1u;
  return GO2SIM_E_OK;
}

}  // extern "C"
