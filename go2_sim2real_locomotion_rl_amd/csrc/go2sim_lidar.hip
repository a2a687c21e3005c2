// go2sim_lidar.hip -- the LIDAR terrain scan (include/go2sim_lidar.h): the actor's noisy body-frame height profile with its one-step memory, the critic's
// clean one, and the assembly of the wider observation rows, on gfx950.  The header states the law, the draw layout and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/go2sim_lidar.h"
#include "go2sim_envlaunch_dev.h"

namespace {

constexpr char TAG[] = "go2sim_lidar";
constexpr int EXTRA = GO2SIM_LIDAR_PRIV_EXTRA;

// what the kernels see of one handle
struct LidarDev {
  const float* hf;                 // Field's members are this one, rows, cols, ox, oy and hs
  const float *ax, *ay, *cx, *cy;  // the sample points: one allocation, in this order
  float* stored;                   // [n_envs][n_actor]
  int rows, cols, n_envs, n_actor, n_critic;
  float ox, oy, hs, clip, scale;
  float noise_std, offset_std;
  double dropout_prob, latency_prob, blackout_prob;     // multiplied with L in float64, then rounded (the header's thresholds)
  DrSched dr;
  uint32_t k0, k1;                 // the seed's words
};

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
  const Base B = load_base(P, b);
  for (int k = t; k < nc; k += WAVE) prow[n_in + na + extra + k] = clip_scale(D, scan_point(D, B.px, B.py, B.pz, B.s, B.c, D.cx[k], D.cy[k]));
  if (na == 0) return;
  const double L = dr_level(D.dr, level);
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
    float v = scan_point(D, B.px, B.py, B.pz, B.s, B.c, D.ax[k], D.ay[k]);
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

}  // namespace

struct go2sim_lidar {
  int device = 0;
  LidarDev dev = {};
  uint32_t step = 0;
};

extern "C" {

int go2sim_lidar_create(int device, const go2sim_lidar_cfg_t* cfg, const int16_t* hf, const float* actor_xy, const float* critic_xy, uint64_t seed,
                        go2sim_lidar_t** out) {
  if (!out || !cfg || !hf) return GO2SIM_E_BADARG;
  const go2sim_lidar_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.n_actor < 0 || c.n_critic < 0 || c.n_actor + c.n_critic == 0 || c.n_actor > (1 << 16) || c.n_critic > (1 << 16)) return GO2SIM_E_BADARG;
  if (!field_args_ok(c.hf_rows, c.hf_cols, c.horizontal_scale) || !(c.height_clip >= 0.0)) return GO2SIM_E_BADARG;
  if ((c.n_actor > 0 && !actor_xy) || (c.n_critic > 0 && !critic_xy)) return GO2SIM_E_BADARG;
  if (nan_in({c.height_noise_std, c.dropout_prob, c.vertical_offset_std, c.latency_prob, c.full_blackout_prob, c.height_scale, c.dr_phase1_level,
              c.dr_terrain_gate, c.origin_x, c.origin_y, c.vertical_scale}))
    return GO2SIM_E_BADARG;
  HIPCHK(TAG, hipSetDevice(device));
  go2sim_lidar* h = new (std::nothrow) go2sim_lidar();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  LidarDev& D = h->dev;
  const size_t npts = 2 * ((size_t)c.n_actor + c.n_critic), nst = (size_t)c.n_envs * (c.n_actor > 0 ? c.n_actor : 1);
  std::vector<float> pts(npts);
  for (int k = 0; k < 2 * c.n_actor; ++k) pts[k] = actor_xy[k];
  for (int k = 0; k < 2 * c.n_critic; ++k) pts[2 * (size_t)c.n_actor + k] = critic_xy[k];
  int rc = upload_field(&D, hf, c.hf_rows, c.hf_cols, c.origin_x, c.origin_y, c.horizontal_scale, c.vertical_scale);
  if (rc == GO2SIM_E_OK) rc = dev_array((float**)&D.ax, pts.data(), npts);
  if (rc == GO2SIM_E_OK) rc = dev_array(&D.stored, (const float*)nullptr, nst);
  if (rc == GO2SIM_E_OK && hipDeviceSynchronize() != hipSuccess) rc = GO2SIM_E_HIP;
  if (rc != GO2SIM_E_OK) {
    go2sim_lidar_destroy(h);
    return rc;
  }
  D.ay = D.ax + c.n_actor; D.cx = D.ay + c.n_actor; D.cy = D.cx + c.n_critic;
  D.n_envs = c.n_envs; D.n_actor = c.n_actor; D.n_critic = c.n_critic;
  D.clip = (float)c.height_clip; D.scale = (float)c.height_scale;
  D.noise_std = (float)c.height_noise_std; D.offset_std = (float)c.vertical_offset_std;
  D.dropout_prob = c.dropout_prob; D.latency_prob = c.latency_prob; D.blackout_prob = c.full_blackout_prob;
  D.dr = DrSched{c.dr_phase1_level, c.dr_terrain_gate, c.dr_schedule != 0, c.curriculum_enabled != 0};
  D.k0 = (uint32_t)seed; D.k1 = (uint32_t)(seed >> 32);
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_lidar_destroy(go2sim_lidar_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree((void*)h->dev.hf); (void)hipFree((void*)h->dev.ax); (void)hipFree(h->dev.stored);
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
  return h ? clear_rows(TAG, h->dev.stored, h->dev.n_envs, h->dev.n_actor, envs_idx, n_sel, stream) : GO2SIM_E_BADARG;
}

int go2sim_lidar_get_scan(go2sim_lidar_t* h, float* scan, void* stream) {
  if (!h || !scan) return GO2SIM_E_BADARG;
  return copy_wait(TAG, hipMemcpyDeviceToHost, stream, {{scan, h->dev.stored, (size_t)h->dev.n_envs * h->dev.n_actor * sizeof(float)}});
}

int go2sim_lidar_set_scan(go2sim_lidar_t* h, const float* scan, void* stream) {
  if (!h || !scan) return GO2SIM_E_BADARG;
  return copy_wait(TAG, hipMemcpyHostToDevice, stream, {{h->dev.stored, scan, (size_t)h->dev.n_envs * h->dev.n_actor * sizeof(float)}});
}

int go2sim_lidar_step(go2sim_lidar_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                      long long quat_comp_stride, long long quat_env_stride, const uint8_t* reset, const double* level, const float* obs, const float* priv,
                      int n_in, float* obs_out, float* priv_out, void* stream) {
  if (!h || n != h->dev.n_envs || !pose_args_ok(pos, pos_comp_stride, pos_env_stride, quat, quat_comp_stride, quat_env_stride)) return GO2SIM_E_BADARG;
  if ((h->dev.dr.curriculum_enabled && !level) || !rows_args_ok(obs, priv, n_in, obs_out, priv_out)) return GO2SIM_E_BADARG;
  const Pose P = {pos, quat, pos_comp_stride, pos_env_stride, quat_comp_stride, quat_env_stride};
  hipLaunchKernelGGL(k_lidar_step, dim3((n + ENVS_PER_WG - 1) / ENVS_PER_WG), dim3(WG), 0, (hipStream_t)stream, h->dev, P, reset, level, h->step, obs, priv, n_in,
                     obs_out, priv_out);
  HIPCHK(TAG, hipGetLastError());
  h->step += 1u;
  return GO2SIM_E_OK;
}

}  // extern "C"
