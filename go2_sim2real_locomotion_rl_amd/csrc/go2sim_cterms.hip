// go2sim_cterms.hip -- the contact terms (include/go2sim_cterms.h): the reference's body_contact and stumble reward terms on the links' net contact
// forces, one launch after the step's own, on gfx950.  The header states the law and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/go2sim_cterms.h"
#include "go2sim_envlaunch_dev.h"

namespace {

constexpr char TAG[] = "go2sim_cterms";
constexpr int NT = GO2SIM_CTERMS_N, BODY = GO2SIM_CTERMS_BODY, STUMBLE = GO2SIM_CTERMS_STUMBLE;

// what the kernels see of one handle
struct CtermsDev {
  float *sum, *ep;     // the episode terms' members are these two, steps, n_envs and dt
  int* steps;
  int n_envs;
  uint32_t mask[NT];
  int on[NT];          // the term's scale is not zero
  float inc[NT], thr[NT];
  float dt;
};

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
  if (D.on[BODY]) r = r + count_term(D, BODY, b, fcount * D.inc[BODY], is_reset);
  if (D.on[STUMBLE]) r = r + count_term(D, STUMBLE, b, pen * D.inc[STUMBLE], is_reset);
  rew[b] = r;
}

}  // namespace

struct go2sim_cterms {
  int device = 0;
  CtermsDev dev = {};
};

extern "C" {

int go2sim_cterms_create(int device, const go2sim_cterms_cfg_t* cfg, go2sim_cterms_t** out) {
  if (!out || !cfg) return GO2SIM_E_BADARG;
  const go2sim_cterms_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.n_links < 1 || c.n_links > GO2SIM_CTERMS_LINKS_MAX || !(c.dt > 0.0)) return GO2SIM_E_BADARG;
  const uint32_t allowed = c.n_links == 32 ? 0xFFFFFFFFu : ((1u << c.n_links) - 1u);
  if ((c.body_mask | c.stumble_mask) & ~allowed) return GO2SIM_E_BADARG;
  if (nan_in({c.body_contact_scale, c.stumble_scale, c.body_contact_threshold, c.stumble_threshold})) return GO2SIM_E_BADARG;
  HIPCHK(TAG, hipSetDevice(device));
  go2sim_cterms* h = new (std::nothrow) go2sim_cterms();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  CtermsDev& D = h->dev;
  int rc = alloc_terms(&D, NT, c.n_envs, c.dt);
  if (rc == GO2SIM_E_OK && hipDeviceSynchronize() != hipSuccess) rc = GO2SIM_E_HIP;
  if (rc != GO2SIM_E_OK) {
    go2sim_cterms_destroy(h);
    return rc;
  }
  D.mask[BODY] = c.body_mask; D.mask[STUMBLE] = c.stumble_mask;
  D.on[BODY] = c.body_contact_scale != 0.0; D.on[STUMBLE] = c.stumble_scale != 0.0;
  D.inc[BODY] = (float)(c.body_contact_scale * c.dt); D.inc[STUMBLE] = (float)(c.stumble_scale * c.dt);
  D.thr[BODY] = (float)c.body_contact_threshold; D.thr[STUMBLE] = (float)c.stumble_threshold;
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_cterms_destroy(go2sim_cterms_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  free_terms(&h->dev);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_cterms_step(go2sim_cterms_t* h, int n, const float* cf, long long comp_stride, long long link_stride, long long env_stride,
                       const uint8_t* reset, float* rew, float* count_out, void* stream) {
  if (!h || !cf || n != h->dev.n_envs || comp_stride < 0 || link_stride < 0 || env_stride < 0) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_cterms_step, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, h->dev, cf, comp_stride, link_stride,
                     env_stride, reset, rew, count_out);
  HIPCHK(TAG, hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_cterms_clear(go2sim_cterms_t* h, const int* envs_idx, int n_sel, void* stream) {
  return h ? clear_terms<NT>(TAG, h->dev, envs_idx, n_sel, stream) : GO2SIM_E_BADARG;
}

int go2sim_cterms_get_state(go2sim_cterms_t* h, float* sum, int32_t* steps, float* ep, void* stream) {
  if (!h || !sum || !steps || !ep) return GO2SIM_E_BADARG;
  const CtermsDev& E = h->dev;
  const size_t n = (size_t)NT * E.n_envs;
  return copy_wait(TAG, hipMemcpyDeviceToHost, stream, {{sum, E.sum, n * sizeof(float)}, {steps, E.steps, n * sizeof(int)}, {ep, E.ep, n * sizeof(float)}});
}

int go2sim_cterms_set_state(go2sim_cterms_t* h, const float* sum, const int32_t* steps, const float* ep, void* stream) {
  if (!h || !sum || !steps || !ep) return GO2SIM_E_BADARG;
  const CtermsDev& E = h->dev;
  const size_t n = (size_t)NT * E.n_envs;
  return copy_wait(TAG, hipMemcpyHostToDevice, stream, {{E.sum, sum, n * sizeof(float)}, {E.steps, steps, n * sizeof(int)}, {E.ep, ep, n * sizeof(float)}});
}

int go2sim_cterms_ep(go2sim_cterms_t* h, const float** body_ep_dev, const float** stumble_ep_dev, float* inc_body, float* inc_stumble) {
  if (!h || !body_ep_dev || !stumble_ep_dev || !inc_body || !inc_stumble) return GO2SIM_E_BADARG;
  *body_ep_dev = h->dev.ep + (size_t)BODY * h->dev.n_envs; *stumble_ep_dev = h->dev.ep + (size_t)STUMBLE * h->dev.n_envs;
  *inc_body = h->dev.inc[BODY]; *inc_stumble = h->dev.inc[STUMBLE];
  return GO2SIM_E_OK;
}

}  // extern "C"
