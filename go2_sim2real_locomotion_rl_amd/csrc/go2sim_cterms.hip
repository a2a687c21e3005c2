// go2sim_cterms.hip -- the contact terms (include/go2sim_cterms.h): the reference's body_contact and stumble reward terms on the links' net contact
// forces, one launch after the step's own, on gfx950.  The header states the law and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <new>

#include "../../include/go2sim_cterms.h"
#include "../../include/go2sim_detmath.h"

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_cterms: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

constexpr int WG = 256, NT = GO2SIM_CTERMS_N, BODY = GO2SIM_CTERMS_BODY, STUMBLE = GO2SIM_CTERMS_STUMBLE;

// what the kernels see of one handle; per-term arrays are [NT][n_envs]
struct CtermsDev {
  float *sum, *ep;
  int* steps;
  int n_envs;
  uint32_t mask[NT];
  int on[NT];          // the term's scale is not zero
  float inc[NT], thr[NT];
  float dt;
};

// "ep_t[b] = sum_t[b] / (f32(max(steps_t[b], 1)) * f32(dt))", then both := 0
__device__ __forceinline__ void hand_over(const CtermsDev& D, int t, int b, float sum, int steps) {
  const size_t k = (size_t)t * D.n_envs + b;
  const float ep_steps = (float)(steps < 1 ? 1 : steps);
  D.ep[k] = sum / (ep_steps * D.dt);
  D.sum[k] = 0.0f;
  D.steps[k] = 0;
}

// "rew[b] = rew[b] + term; sum_t[b] = sum_t[b] + term; steps_t[b] += 1", then the hand-over of a reset env; -> the new rew[b]
__device__ __forceinline__ float apply_term(const CtermsDev& D, int t, int b, float r, float term, bool is_reset) {
  const size_t k = (size_t)t * D.n_envs + b;
  const float sum = D.sum[k] + term;
  const int steps = D.steps[k] + 1;
  if (is_reset) hand_over(D, t, b, sum, steps);
  else { D.sum[k] = sum; D.steps[k] = steps; }
  return r + term;
}

// One lane per env: this lane alone reads and writes the env's cells.
__global__ __launch_bounds__(WG) void k_cterms_step(CtermsDev D, const float* __restrict__ cf, long long cs, long long ls, long long es,
                                                    const uint8_t* __restrict__ reset, float* __restrict__ rew, float* __restrict__ count_out) {
  const int b = blockIdx.x * WG + threadIdx.x;
  if (b >= D.n_envs) return;
  const uint32_t either = D.mask[BODY] | D.mask[STUMBLE];
  const float* __restrict__ f = cf + (size_t)b * es;
  int count = 0;
  float pen = 0.0f;
#pragma unroll
  for (int l = 0; l < GO2SIM_CTERMS_LINKS_MAX; ++l) {
    if (!((either >> l) & 1u)) continue;                               // wave-uniform
    const float fx = f[l * ls], fy = f[cs + l * ls], fz = f[2 * cs + l * ls];
    const float n = dm_sqrt((fx * fx + fy * fy) + fz * fz);
    if ((D.mask[BODY] >> l) & 1u) count += (n > D.thr[BODY]) ? 1 : 0;
    if ((D.mask[STUMBLE] >> l) & 1u) {
      const float d = n - D.thr[STUMBLE];
      pen = pen + (d < 0.0f ? 0.0f : d);                               // a NaN d stays
    }
  }
  const float fcount = (float)count;
  if (count_out) count_out[b] = fcount;
  if (!rew || !(D.on[BODY] | D.on[STUMBLE])) return;
  const bool is_reset = reset && reset[b];
  float r = rew[b];
  if (D.on[BODY]) r = apply_term(D, BODY, b, r, fcount * D.inc[BODY], is_reset);
  if (D.on[STUMBLE]) r = apply_term(D, STUMBLE, b, r, pen * D.inc[STUMBLE], is_reset);
  rew[b] = r;
}

__global__ __launch_bounds__(WG) void k_cterms_clear(CtermsDev D, const int* __restrict__ idx, int n_sel) {
  const int r = blockIdx.x * WG + threadIdx.x;
  if (r >= (idx ? n_sel : D.n_envs)) return;
  const int b = idx ? idx[r] : r;
  if (b < 0 || b >= D.n_envs) return;
  for (int t = 0; t < NT; ++t) hand_over(D, t, b, D.sum[(size_t)t * D.n_envs + b], D.steps[(size_t)t * D.n_envs + b]);
}

}  // namespace

struct go2sim_cterms {
  int device = 0;
  CtermsDev dev = {};
  float* fbuf = nullptr;     // sum | ep
  int* steps = nullptr;
};

extern "C" {

int go2sim_cterms_create(int device, const go2sim_cterms_cfg_t* cfg, go2sim_cterms_t** out) {
  if (!out || !cfg) return GO2SIM_E_BADARG;
  const go2sim_cterms_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.n_links < 1 || c.n_links > GO2SIM_CTERMS_LINKS_MAX || !(c.dt > 0.0)) return GO2SIM_E_BADARG;
  const uint32_t allowed = c.n_links == 32 ? 0xFFFFFFFFu : ((1u << c.n_links) - 1u);
  if ((c.body_mask | c.stumble_mask) & ~allowed) return GO2SIM_E_BADARG;
  const double all[] = {c.body_contact_scale, c.stumble_scale, c.body_contact_threshold, c.stumble_threshold};
  for (double v : all)
    if (v != v) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(device));
  go2sim_cterms* h = new (std::nothrow) go2sim_cterms();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  const size_t n = (size_t)c.n_envs;
  if (hipMalloc((void**)&h->fbuf, 2 * NT * n * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->steps, NT * n * sizeof(int)) != hipSuccess) {
    go2sim_cterms_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  if (hipMemset(h->fbuf, 0, 2 * NT * n * sizeof(float)) != hipSuccess || hipMemset(h->steps, 0, NT * n * sizeof(int)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    go2sim_cterms_destroy(h);
    return GO2SIM_E_HIP;
  }
  CtermsDev& D = h->dev;
  D.sum = h->fbuf; D.ep = h->fbuf + NT * n; D.steps = h->steps;
  D.n_envs = c.n_envs; D.dt = (float)c.dt;
  D.mask[BODY] = c.body_mask; D.mask[STUMBLE] = c.stumble_mask;
  D.on[BODY] = c.body_contact_scale != 0.0; D.on[STUMBLE] = c.stumble_scale != 0.0;
  D.inc[BODY] = (float)(c.body_contact_scale * c.dt); D.inc[STUMBLE] = (float)(c.stumble_scale * c.dt);
  D.thr[BODY] = (float)c.body_contact_threshold; D.thr[STUMBLE] = (float)c.stumble_threshold;
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_cterms_destroy(go2sim_cterms_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree(h->fbuf); (void)hipFree(h->steps);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_cterms_step(go2sim_cterms_t* h, int n, const float* cf, long long comp_stride, long long link_stride, long long env_stride,
                       const uint8_t* reset, float* rew, float* count_out, void* stream) {
  if (!h || !cf || n != h->dev.n_envs || comp_stride < 0 || link_stride < 0 || env_stride < 0) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_cterms_step, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->dev, cf, comp_stride, link_stride,
                     env_stride, reset, rew, count_out);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_cterms_clear(go2sim_cterms_t* h, const int* envs_idx, int n_sel, void* stream) {
  if (!h || (envs_idx && n_sel < 0)) return GO2SIM_E_BADARG;
  const int total = envs_idx ? n_sel : h->dev.n_envs;
  if (total == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL(k_cterms_clear, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->dev, envs_idx, n_sel);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_cterms_get_state(go2sim_cterms_t* h, float* sum, int32_t* steps, float* ep, void* stream) {
  if (!h || !sum || !steps || !ep) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)NT * h->dev.n_envs;
  HIPCHK(hipMemcpyAsync(sum, h->dev.sum, n * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(steps, h->dev.steps, n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(ep, h->dev.ep, n * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return GO2SIM_E_OK;
}

int go2sim_cterms_set_state(go2sim_cterms_t* h, const float* sum, const int32_t* steps, const float* ep, void* stream) {
  if (!h || !sum || !steps || !ep) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)NT * h->dev.n_envs;
  HIPCHK(hipMemcpyAsync(h->dev.sum, sum, n * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dev.steps, steps, n * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dev.ep, ep, n * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                          // the sources are the caller's host memory
  return GO2SIM_E_OK;
}

int go2sim_cterms_ep(go2sim_cterms_t* h, const float** body_ep_dev, const float** stumble_ep_dev, float* inc_body, float* inc_stumble) {
  if (!h || !body_ep_dev || !stumble_ep_dev || !inc_body || !inc_stumble) return GO2SIM_E_BADARG;
  *body_ep_dev = h->dev.ep + (size_t)BODY * h->dev.n_envs; *stumble_ep_dev = h->dev.ep + (size_t)STUMBLE * h->dev.n_envs;
  *inc_body = h->dev.inc[BODY]; *inc_stumble = h->dev.inc[STUMBLE];
  return GO2SIM_E_OK;
}

}  // extern "C"
