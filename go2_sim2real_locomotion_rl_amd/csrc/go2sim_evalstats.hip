// go2sim_evalstats.hip -- the evaluation statistics (include/go2sim_evalstats.h): per-env and per-bin records of command tracking, falls and motor
// load, one launch after the env step's own, on gfx950.  The header states the law and the launches; this file follows its names.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/go2sim_evalstats.h"
#include "go2sim_envlaunch_dev.h"

namespace {

constexpr char TAG[] = "go2sim_evalstats";
constexpr int M = GO2SIM_ES_M, NSUMS = GO2SIM_ES_NSUMS, K = GO2SIM_EI_K, KB = GO2SIM_EBIN_K, NDOF = GO2SIM_EVALSTATS_NDOF;

// what the kernels see of one handle
struct EvalDev {
  double *run_f, *tot_f;      // [M][n_envs] each (one allocation, run | tot)
  int *run_i, *tot_i;         // [K][n_envs] each (one allocation, run | tot)
  int* bins;                  // [n_envs]
  double* bin_f;              // [n_bins][M]
  long long* bin_i;           // [n_bins][KB]
  double torque_limit, dof_vel_limit;
  int n_envs, n_bins, settle_steps, max_episodes;
  uint32_t foot_mask;
};

using View = go2sim_evalstats_view_t;

__device__ __forceinline__ double at(const View& v, int i, int b) { return (double)v.p[i * v.comp_stride + b * v.env_stride]; }
__device__ __forceinline__ double take_max(double x, double m) { return x > m ? x : m; }      // a NaN x compares false

// One lane per env: this lane alone reads and writes the env's cells.
__global__ __launch_bounds__(WG) void k_evalstats_step(EvalDev D, go2sim_evalstats_in_t in) {
  const int b = blockIdx.x * WG + threadIdx.x;
  if (b >= D.n_envs) return;
  const size_t n = (size_t)D.n_envs;
  const int episodes = D.tot_i[GO2SIM_EI_EPISODES * n + b];
  if (episodes >= D.max_episodes) return;
  if (in.reset[b]) {                                                        // the episode closes
#pragma unroll
    for (int q = 0; q < M; ++q) {
      const double r = D.run_f[q * n + b], t = D.tot_f[q * n + b];
      D.tot_f[q * n + b] = q < NSUMS ? t + r : take_max(r, t);
      D.run_f[q * n + b] = 0.0;
    }
    D.tot_i[GO2SIM_EI_EPISODES * n + b] = episodes + 1;
    D.tot_i[GO2SIM_EI_FALLS * n + b] += (in.time_out[b] == 0.0f) ? 1 : 0;
#pragma unroll
    for (int q = GO2SIM_EI_LENGTH_STEPS; q < K; ++q) {
      D.tot_i[q * n + b] += D.run_i[q * n + b];
      D.run_i[q * n + b] = 0;
    }
    return;
  }
  const int k = D.run_i[GO2SIM_EI_LENGTH_STEPS * n + b];
  D.run_i[GO2SIM_EI_LENGTH_STEPS * n + b] = k + 1;
  if (k < D.settle_steps) return;
  // the sample
  const float vxf = in.base_lin_vel.p[b * in.base_lin_vel.env_stride], vyf = in.base_lin_vel.p[in.base_lin_vel.comp_stride + b * in.base_lin_vel.env_stride];
  const double cx = at(in.commands, 0, b), cy = at(in.commands, 1, b), cyaw = at(in.commands, 2, b);
  const double vx = (double)vxf, vy = (double)vyf, wz = at(in.base_ang_vel, 2, b);
  const double gx = at(in.projected_gravity, 0, b), gy = at(in.projected_gravity, 1, b);
  const double ex = cx - vx, ey = cy - vy, ew = cyaw - wz;
  double power = 0.0, tau2 = 0.0, peak_tau = D.run_f[GO2SIM_ES_PEAK_TORQUE * n + b], peak_qd = D.run_f[GO2SIM_ES_PEAK_DOF_VEL * n + b];
  bool over_tau = false, over_qd = false;
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    const double tau = at(in.torque, j, b), qd = at(in.dof_vel, j, b);
    const double atau = fabs(tau), aqd = fabs(qd);
    power = power + fabs(tau * qd);
    tau2 = tau2 + tau * tau;
    peak_tau = take_max(atau, peak_tau);
    peak_qd = take_max(aqd, peak_qd);
    over_tau = over_tau || (atau > D.torque_limit);
    over_qd = over_qd || (aqd > D.dof_vel_limit);
  }
  double peak_foot = D.run_f[GO2SIM_ES_PEAK_FOOT_FORCE * n + b];
  const float* __restrict__ f = in.cf + (size_t)b * in.cf_env_stride;
#pragma unroll
  for (int l = 0; l < GO2SIM_EVALSTATS_LINKS_MAX; ++l) {
    if (!((D.foot_mask >> l) & 1u)) continue;                               // wave-uniform
    const float fx = f[l * in.cf_link_stride], fy = f[in.cf_comp_stride + l * in.cf_link_stride], fz = f[2 * in.cf_comp_stride + l * in.cf_link_stride];
    peak_foot = take_max((double)dm_sqrt((fx * fx + fy * fy) + fz * fz), peak_foot);
  }
  const double speed = (double)dm_sqrt(vxf * vxf + vyf * vyf);
  const double add[NSUMS] = {1.0, ex * ex + ey * ey, ew * ew, vx, vy, wz, power, tau2, gx * gx + gy * gy, speed};
#pragma unroll
  for (int q = 0; q < NSUMS; ++q) D.run_f[q * n + b] = D.run_f[q * n + b] + add[q];
  D.run_f[GO2SIM_ES_PEAK_TORQUE * n + b] = peak_tau;
  D.run_f[GO2SIM_ES_PEAK_DOF_VEL * n + b] = peak_qd;
  D.run_f[GO2SIM_ES_PEAK_FOOT_FORCE * n + b] = peak_foot;
  if (over_tau) D.run_i[GO2SIM_EI_OVER_TORQUE * n + b] += 1;
  if (over_qd) D.run_i[GO2SIM_EI_OVER_DOF_VEL * n + b] += 1;
}

// run := 0, tot := 0, one lane per selected env
__global__ __launch_bounds__(WG) void k_evalstats_clear(EvalDev D, const int* __restrict__ idx, int n_sel) {
  const int r = blockIdx.x * WG + threadIdx.x;
  if (r >= (idx ? n_sel : D.n_envs)) return;
  const int b = idx ? idx[r] : r;
  if (b < 0 || b >= D.n_envs) return;
  const size_t n = (size_t)D.n_envs;
  for (int q = 0; q < M; ++q) { D.run_f[q * n + b] = 0.0; D.tot_f[q * n + b] = 0.0; }
  for (int q = 0; q < K; ++q) { D.run_i[q * n + b] = 0; D.tot_i[q * n + b] = 0; }
}

// the tree of the header over the WG lanes' partials: stride 128 .. 1, OP(left, right); -> lane 0's value (valid in lane 0)
template <class T, class OP>
__device__ __forceinline__ T tree(T* s, T p, OP op) {
  const int i = threadIdx.x;
  __syncthreads();                                                          // the previous entry's reads of s are done
  s[i] = p;
  __syncthreads();
  for (int stride = WG / 2; stride >= 1; stride >>= 1) {
    if (i < stride) s[i] = op(s[i], s[i + stride]);
    __syncthreads();
  }
  return s[0];
}

// One workgroup per bin; lane i walks the envs i, i + 256, .. once per entry.
__global__ __launch_bounds__(WG) void k_evalstats_reduce(EvalDev D) {
  __shared__ double sf[WG];
  __shared__ long long si[WG];
  const int k = blockIdx.x, i = threadIdx.x;
  const size_t n = (size_t)D.n_envs;
  const auto add_f = [](double a, double c) { return a + c; };
  const auto max_f = [](double a, double c) { return c > a ? c : a; };
  const auto add_i = [](long long a, long long c) { return a + c; };
  for (int q = 0; q < M; ++q) {
    double p = 0.0;
    for (int e = i; e < D.n_envs; e += WG)
      if (D.bins[e] == k) p = q < NSUMS ? p + D.tot_f[q * n + e] : max_f(p, D.tot_f[q * n + e]);
    const double v = q < NSUMS ? tree(sf, p, add_f) : tree(sf, p, max_f);
    if (i == 0) D.bin_f[(size_t)k * M + q] = v;
  }
  for (int q = 0; q < KB; ++q) {
    long long p = 0;
    for (int e = i; e < D.n_envs; e += WG)
      if (D.bins[e] == k)
        p += q < K ? (long long)D.tot_i[q * n + e] : q == GO2SIM_EBIN_ENVS ? 1LL : (D.tot_i[GO2SIM_EI_EPISODES * n + e] >= D.max_episodes ? 1LL : 0LL);
    const long long v = tree(si, p, add_i);
    if (i == 0) D.bin_i[(size_t)k * KB + q] = v;
  }
}

bool view_ok(const View& v) { return v.p && v.comp_stride >= 0 && v.env_stride >= 0; }

bool bins_ok(const int32_t* bins, int n_envs, int n_bins) {
  for (int b = 0; bins && b < n_envs; ++b)
    if (bins[b] < 0 || bins[b] >= n_bins) return false;
  return true;
}

}  // namespace

struct go2sim_evalstats {
  int device = 0;
  EvalDev dev = {};
};

extern "C" {

int go2sim_evalstats_create(int device, const go2sim_evalstats_cfg_t* cfg, const int32_t* bins, go2sim_evalstats_t** out) {
  if (!out || !cfg) return GO2SIM_E_BADARG;
  const go2sim_evalstats_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.n_bins < 1 || c.settle_steps < 0 || c.max_episodes < 1 || c.n_links < 1 || c.n_links > GO2SIM_EVALSTATS_LINKS_MAX || !(c.dt > 0.0))
    return GO2SIM_E_BADARG;
  const uint32_t allowed = c.n_links == 32 ? 0xFFFFFFFFu : ((1u << c.n_links) - 1u);
  if ((c.foot_mask & ~allowed) || nan_in({c.torque_limit, c.dof_vel_limit}) || !bins_ok(bins, c.n_envs, c.n_bins)) return GO2SIM_E_BADARG;
  HIPCHK(TAG, hipSetDevice(device));
  go2sim_evalstats* h = new (std::nothrow) go2sim_evalstats();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  EvalDev& D = h->dev;
  const size_t n = (size_t)c.n_envs;
  D.n_envs = c.n_envs; D.n_bins = c.n_bins; D.settle_steps = c.settle_steps; D.max_episodes = c.max_episodes;
  D.torque_limit = c.torque_limit; D.dof_vel_limit = c.dof_vel_limit; D.foot_mask = c.foot_mask;
  int rc = dev_array(&D.run_f, (const double*)nullptr, 2 * M * n);
  if (rc == GO2SIM_E_OK) rc = dev_array(&D.run_i, (const int*)nullptr, 2 * K * n);
  if (rc == GO2SIM_E_OK) rc = dev_array(&D.bins, (const int*)bins, n);
  if (rc == GO2SIM_E_OK) rc = dev_array(&D.bin_f, (const double*)nullptr, (size_t)c.n_bins * M);
  if (rc == GO2SIM_E_OK) rc = dev_array(&D.bin_i, (const long long*)nullptr, (size_t)c.n_bins * KB);
  if (rc == GO2SIM_E_OK && hipDeviceSynchronize() != hipSuccess) rc = GO2SIM_E_HIP;
  if (rc != GO2SIM_E_OK) {
    go2sim_evalstats_destroy(h);
    return rc;
  }
  D.tot_f = D.run_f + M * n; D.tot_i = D.run_i + K * n;
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_evalstats_destroy(go2sim_evalstats_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  EvalDev& D = h->dev;
  (void)hipFree(D.run_f); (void)hipFree(D.run_i); (void)hipFree(D.bins); (void)hipFree(D.bin_f); (void)hipFree(D.bin_i);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_evalstats_set_bins(go2sim_evalstats_t* h, const int32_t* bins, void* stream) {
  if (!h || !bins || !bins_ok(bins, h->dev.n_envs, h->dev.n_bins)) return GO2SIM_E_BADARG;
  return copy_wait(TAG, hipMemcpyHostToDevice, stream, {{h->dev.bins, bins, (size_t)h->dev.n_envs * sizeof(int)}});
}

int go2sim_evalstats_step(go2sim_evalstats_t* h, int n, const go2sim_evalstats_in_t* in, void* stream) {
  if (!h || !in || n != h->dev.n_envs) return GO2SIM_E_BADARG;
  for (const View* v : {&in->commands, &in->base_lin_vel, &in->base_ang_vel, &in->projected_gravity, &in->dof_vel, &in->torque})
    if (!view_ok(*v)) return GO2SIM_E_BADARG;
  if (!in->cf || in->cf_comp_stride < 0 || in->cf_link_stride < 0 || in->cf_env_stride < 0 || !in->reset || !in->time_out) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_evalstats_step, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->dev, *in);
  HIPCHK(TAG, hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_evalstats_clear(go2sim_evalstats_t* h, const int* envs_idx, int n_sel, void* stream) {
  if (!h || (envs_idx && n_sel < 0)) return GO2SIM_E_BADARG;
  const int total = envs_idx ? n_sel : h->dev.n_envs;
  if (total == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL(k_evalstats_clear, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->dev, envs_idx, n_sel);
  HIPCHK(TAG, hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_evalstats_reduce(go2sim_evalstats_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_evalstats_reduce, dim3((unsigned)h->dev.n_bins), dim3(WG), 0, (hipStream_t)stream, h->dev);
  HIPCHK(TAG, hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_evalstats_get_state(go2sim_evalstats_t* h, double* run_f, int32_t* run_i, double* tot_f, int32_t* tot_i, double* bin_f, int64_t* bin_i,
                               void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  const EvalDev& D = h->dev;
  const size_t n = (size_t)D.n_envs, nb = (size_t)D.n_bins;
  const auto bytes = [](const void* dst, size_t b) { return dst ? b : (size_t)0; };
  return copy_wait(TAG, hipMemcpyDeviceToHost, stream,
                   {{run_f, D.run_f, bytes(run_f, M * n * sizeof(double))}, {run_i, D.run_i, bytes(run_i, K * n * sizeof(int))},
                    {tot_f, D.tot_f, bytes(tot_f, M * n * sizeof(double))}, {tot_i, D.tot_i, bytes(tot_i, K * n * sizeof(int))},
                    {bin_f, D.bin_f, bytes(bin_f, nb * M * sizeof(double))}, {bin_i, D.bin_i, bytes(bin_i, nb * KB * sizeof(long long))}});
}

int go2sim_evalstats_episodes(go2sim_evalstats_t* h, const int32_t** episodes_dev) {
  if (!h || !episodes_dev) return GO2SIM_E_BADARG;
  *episodes_dev = h->dev.tot_i + (size_t)GO2SIM_EI_EPISODES * h->dev.n_envs;
  return GO2SIM_E_OK;
}

}  // extern "C"
