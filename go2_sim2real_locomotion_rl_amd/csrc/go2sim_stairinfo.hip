// go2sim_stairinfo.hip -- the four-value stair info (include/go2sim_stairinfo.h): the edge detector on the heightfield, the per-row step sizes, the actor's
// degraded copy with its one-step memory, the critic's clean one, and the assembly of the wider observation rows, on gfx950.  The header states the law, the
// draw layout and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "../../include/go2sim_stairinfo.h"
#include "go2sim_envlaunch_dev.h"

namespace {

constexpr char TAG[] = "go2sim_stairinfo";
constexpr int NV = GO2SIM_STAIRINFO_N, EXTRA = GO2SIM_STAIRINFO_PRIV_EXTRA;
constexpr int MAX_SAMPLES = GO2SIM_STAIRINFO_MAX_SAMPLES, MAX_ROWS = GO2SIM_STAIRINFO_MAX_ROWS;
static_assert(MAX_SAMPLES <= WAVE, "one lane per pair of neighbouring samples");

// what the kernels see of one handle
struct StairDev {
  const float* hf;                  // Field's members are this one, rows, cols, ox, oy and hs
  const float* xs;                  // [n_samples]; one allocation with the two below, in this order
  const float *row_h, *row_d;       // [n_rows]
  float* stored;                    // [n_envs][4]
  int rows, cols, n_envs, n_samples, n_rows;
  float ox, oy, hs, max_range, thr;
  float s_e, s_h, s_d, s_dir;
  float std_e, std_h, std_d;
  double flip_prob, latency_prob, blackout_prob;     // multiplied with L in float64, then rounded (the header's thresholds)
  DrSched dr;
  uint32_t k0, k1;                  // the seed's words
};

// One wavefront per env.  Every lane holds the env's pose, yaw, sine, cosine, level and draws (wave-uniform values); lane t owns the neighbouring samples
// (t, t + 1), lane j < 4 entry j of the stored row, and lane t the columns t, t + 64, ... of the copied inner rows, so that consecutive lanes write
// consecutive floats of a row.
__global__ __launch_bounds__(WG) void k_stairinfo_step(StairDev D, Pose P, const int* __restrict__ terrain_row, const uint8_t* __restrict__ reset,
                                                       const double* __restrict__ level, uint32_t step, const float* __restrict__ obs,
                                                       const float* __restrict__ priv, int n_in, float* __restrict__ obs_out, float* __restrict__ priv_out) {
  const int b = blockIdx.x * ENVS_PER_WG + (threadIdx.x / WAVE), t = threadIdx.x % WAVE;
  if (b >= D.n_envs) return;                                        // whole wavefronts leave: b is the same on all 64 lanes
  const int extra = obs ? EXTRA : 0;                                // without inner rows the outputs are the fours alone
  const int w_obs = n_in + NV, w_priv = n_in + NV + extra + NV;
  float* __restrict__ orow = obs_out + (size_t)b * w_obs;
  float* __restrict__ prow = priv_out + (size_t)b * w_priv;
  if (obs) {
    const float* __restrict__ oi = obs + (size_t)b * n_in;
    const float* __restrict__ pi = priv + (size_t)b * (n_in + EXTRA);
    for (int i = t; i < n_in; i += WAVE) { orow[i] = oi[i]; prow[i] = pi[i]; }
    for (int i = t; i < EXTRA; i += WAVE) prow[n_in + NV + i] = pi[n_in + i];
  }
  float* st = D.stored + (size_t)b * NV + (t < NV ? t : 0);         // lane j < 4 alone reads and writes cell j
  if (reset && reset[b]) {
    if (t < NV) { *st = 0.0f; orow[n_in + t] = 0.0f; prow[n_in + t] = 0.0f; prow[n_in + NV + extra + t] = 0.0f; }
    return;
  }
  const Base B = load_base(P, b);
  // the edge detector: lane t < n_samples - 1 forms dh_t; the first edge is the lowest set bit of the ballot
  const int np = D.n_samples - 1;
  const int k = t < np ? t : np - 1;                                // lanes beyond the pairs repeat the last one and do not vote
  const float x0 = D.xs[k], x1 = D.xs[k + 1];
  const float dh = height_ahead(D, B.px, B.py, B.s, B.c, x1) - height_ahead(D, B.px, B.py, B.s, B.c, x0);
  const unsigned long long sig = __ballot(t < np && fabsf(dh) > D.thr);
  const unsigned long long up = __ballot(dh > 0.0f);
  const int first = sig ? __ffsll((unsigned long long)sig) - 1 : 0;
  float edge = D.max_range, dir = 0.0f;
  if (sig) {
    edge = (D.xs[first] + D.xs[first + 1]) / 2.0f;
    dir = ((up >> first) & 1ull) ? 1.0f : -1.0f;                    // |dh| > threshold >= 0: never 0
  }
  int r = terrain_row ? terrain_row[b] : 0;
  r = r < 0 ? 0 : (r >= D.n_rows ? D.n_rows - 1 : r);
  float height = D.row_h[r], depth = D.row_d[r];
  const float c0 = edge * D.s_e, c1 = height * D.s_h, c2 = depth * D.s_d, c3 = dir * D.s_dir;
  // the actor's copy
  const double L = dr_level(D.dr, level);
  const bool on = L > 0.0;
  const float Lf = (float)L;
  if (on) {
    const bool do_e = D.std_e > 0.0f, do_h = D.std_h > 0.0f, do_d = D.std_d > 0.0f;
    if (do_e || do_h || do_d) {
      const dm_u4 rz = dm_philox((uint32_t)b, step, GO2SIM_STAIRINFO_RNG_PURPOSE, 0u, D.k0, D.k1);
      float z_e, z_h, z_d, z_x;
      dm_normal2(rz.v[0], rz.v[1], &z_e, &z_h);
      dm_normal2(rz.v[2], rz.v[3], &z_d, &z_x);
      if (do_e) {
        edge = edge + (z_e * D.std_e) * Lf;
        edge = edge < 0.0f ? 0.0f : (edge > D.max_range ? D.max_range : edge);
      }
      if (do_h) height = height + (z_h * D.std_h) * Lf;
      if (do_d) depth = depth + (z_d * D.std_d) * Lf;
    }
    const bool do_flip = D.flip_prob > 0.0, do_lat = D.latency_prob > 0.0, do_black = D.blackout_prob > 0.0;
    if (do_flip || do_lat || do_black) {
      const dm_u4 ru = dm_philox((uint32_t)b, step, GO2SIM_STAIRINFO_RNG_PURPOSE, 1u, D.k0, D.k1);
      if (do_flip && dm_u01(ru.v[0]) < (float)(D.flip_prob * L)) dir = -dir;
      if (do_lat && dm_u01(ru.v[1]) < (float)(D.latency_prob * L)) {
        const float prev = *st;                                     // lane 0: the stored edge, lane 3: the stored direction; the other lanes' values are not used
        edge = prev / D.s_e;
        dir = prev / D.s_dir;
      }
      if (do_black && dm_u01(ru.v[2]) < (float)(D.blackout_prob * L)) { edge = D.max_range; dir = 0.0f; }
    }
  }
  if (t < NV) {
    const float a = t == 0 ? edge * D.s_e : (t == 1 ? height * D.s_h : (t == 2 ? depth * D.s_d : dir * D.s_dir));
    const float cl = t == 0 ? c0 : (t == 1 ? c1 : (t == 2 ? c2 : c3));
    *st = a; orow[n_in + t] = a; prow[n_in + t] = a; prow[n_in + NV + extra + t] = cl;
  }
}

}  // namespace

struct go2sim_stairinfo {
  int device = 0;
  StairDev dev = {};
  uint32_t step = 0;
};

extern "C" {

int go2sim_stairinfo_create(int device, const go2sim_stairinfo_cfg_t* cfg, const int16_t* hf, const float* sample_x, const float* row_heights,
                            const float* row_depths, uint64_t seed, go2sim_stairinfo_t** out) {
  if (!out || !cfg || !hf || !sample_x || !row_heights || !row_depths) return GO2SIM_E_BADARG;
  const go2sim_stairinfo_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.n_samples < 2 || c.n_samples > MAX_SAMPLES || c.n_rows < 1 || c.n_rows > MAX_ROWS) return GO2SIM_E_BADARG;
  if (!field_args_ok(c.hf_rows, c.hf_cols, c.horizontal_scale)) return GO2SIM_E_BADARG;
  if (!(c.max_range >= 0.0) || !(c.threshold >= 0.0) || !std::isfinite(c.max_range) || !std::isfinite(c.threshold)) return GO2SIM_E_BADARG;
  if (nan_in({c.edge_dist_scale, c.height_scale, c.depth_scale, c.direction_scale, c.edge_noise_std, c.height_noise_std, c.depth_noise_std,
              c.direction_flip_prob, c.latency_prob, c.full_blackout_prob, c.dr_phase1_level, c.dr_terrain_gate, c.origin_x, c.origin_y, c.horizontal_scale,
              c.vertical_scale}))
    return GO2SIM_E_BADARG;
  HIPCHK(TAG, hipSetDevice(device));
  go2sim_stairinfo* h = new (std::nothrow) go2sim_stairinfo();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  StairDev& D = h->dev;
  std::vector<float> tab((size_t)c.n_samples + 2 * (size_t)c.n_rows);
  for (int k = 0; k < c.n_samples; ++k) tab[k] = sample_x[k];
  for (int k = 0; k < c.n_rows; ++k) { tab[c.n_samples + k] = row_heights[k]; tab[c.n_samples + c.n_rows + k] = row_depths[k]; }
  int rc = upload_field(&D, hf, c.hf_rows, c.hf_cols, c.origin_x, c.origin_y, c.horizontal_scale, c.vertical_scale);
  if (rc == GO2SIM_E_OK) rc = dev_array((float**)&D.xs, tab.data(), tab.size());
  if (rc == GO2SIM_E_OK) rc = dev_array(&D.stored, (const float*)nullptr, (size_t)c.n_envs * NV);
  if (rc == GO2SIM_E_OK && hipDeviceSynchronize() != hipSuccess) rc = GO2SIM_E_HIP;
  if (rc != GO2SIM_E_OK) {
    go2sim_stairinfo_destroy(h);
    return rc;
  }
  D.row_h = D.xs + c.n_samples; D.row_d = D.row_h + c.n_rows;
  D.n_envs = c.n_envs; D.n_samples = c.n_samples; D.n_rows = c.n_rows;
  D.max_range = (float)c.max_range; D.thr = (float)c.threshold;
  D.s_e = (float)c.edge_dist_scale; D.s_h = (float)c.height_scale; D.s_d = (float)c.depth_scale; D.s_dir = (float)c.direction_scale;
  D.std_e = (float)c.edge_noise_std; D.std_h = (float)c.height_noise_std; D.std_d = (float)c.depth_noise_std;
  D.flip_prob = c.direction_flip_prob; D.latency_prob = c.latency_prob; D.blackout_prob = c.full_blackout_prob;
  D.dr = DrSched{c.dr_phase1_level, c.dr_terrain_gate, c.dr_schedule != 0, c.curriculum_enabled != 0};
  D.k0 = (uint32_t)seed; D.k1 = (uint32_t)(seed >> 32);
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_stairinfo_destroy(go2sim_stairinfo_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree((void*)h->dev.hf); (void)hipFree((void*)h->dev.xs); (void)hipFree(h->dev.stored);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_stairinfo_get_step(go2sim_stairinfo_t* h, uint32_t* step) {
  if (!h || !step) return GO2SIM_E_BADARG;
  *step = h->step;
  return GO2SIM_E_OK;
}

int go2sim_stairinfo_set_step(go2sim_stairinfo_t* h, uint32_t step) {
  if (!h) return GO2SIM_E_BADARG;
  h->step = step;
  return GO2SIM_E_OK;
}

int go2sim_stairinfo_clear(go2sim_stairinfo_t* h, const int* envs_idx, int n_sel, void* stream) {
  return h ? clear_rows(TAG, h->dev.stored, h->dev.n_envs, NV, envs_idx, n_sel, stream) : GO2SIM_E_BADARG;
}

int go2sim_stairinfo_get_state(go2sim_stairinfo_t* h, float* rows4, void* stream) {
  if (!h || !rows4) return GO2SIM_E_BADARG;
  return copy_wait(TAG, hipMemcpyDeviceToHost, stream, {{rows4, h->dev.stored, (size_t)h->dev.n_envs * NV * sizeof(float)}});
}

int go2sim_stairinfo_set_state(go2sim_stairinfo_t* h, const float* rows4, void* stream) {
  if (!h || !rows4) return GO2SIM_E_BADARG;
  return copy_wait(TAG, hipMemcpyHostToDevice, stream, {{h->dev.stored, rows4, (size_t)h->dev.n_envs * NV * sizeof(float)}});
}

int go2sim_stairinfo_step(go2sim_stairinfo_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                          long long quat_comp_stride, long long quat_env_stride, const int* terrain_row, const uint8_t* reset, const double* level,
                          const float* obs, const float* priv, int n_in, float* obs_out, float* priv_out, void* stream) {
  if (!h || n != h->dev.n_envs || !pose_args_ok(pos, pos_comp_stride, pos_env_stride, quat, quat_comp_stride, quat_env_stride)) return GO2SIM_E_BADARG;
  if (!terrain_row && h->dev.n_rows > 1) return GO2SIM_E_BADARG;
  if ((h->dev.dr.curriculum_enabled && !level) || !rows_args_ok(obs, priv, n_in, obs_out, priv_out)) return GO2SIM_E_BADARG;
  const Pose P = {pos, quat, pos_comp_stride, pos_env_stride, quat_comp_stride, quat_env_stride};
  hipLaunchKernelGGL(k_stairinfo_step, dim3((n + ENVS_PER_WG - 1) / ENVS_PER_WG), dim3(WG), 0, (hipStream_t)stream, h->dev, P, terrain_row, reset, level, h->step,
                     obs, priv, n_in, obs_out, priv_out);
  HIPCHK(TAG, hipGetLastError());
  h->step += 1u;
  return GO2SIM_E_OK;
}

}  // extern "C"
