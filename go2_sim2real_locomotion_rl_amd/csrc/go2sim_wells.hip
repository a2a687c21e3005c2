// go2sim_wells.hip -- the scan handle of the stairwell env (include/go2sim_wells.h): the critic's nx x ny body-frame height scan, the assembly of the
// wider privileged row and the alive term, on gfx950.  The header states the law and the launch; this file follows its names.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/go2sim_wells.h"
#include "go2sim_envlaunch_dev.h"

namespace {

constexpr char TAG[] = "go2sim_wells";
constexpr int EXTRA = GO2SIM_WELLS_PRIV_EXTRA;

// what the kernels see of one handle
struct WellsDev {
  Field F;
  const float *lx, *ly;            // [npts] the sample points, point k = i * ny + j; one allocation, in this order
  float *sum, *ep;                 // the alive term: the episode terms' members are these two, steps, n_envs and dt
  int* steps;
  int n_envs, npts;
  float inc, dt;
};

// One wavefront per env.  Every lane holds the env's pose, yaw, sine and cosine (wave-uniform values); lane t owns the columns t, t + 64, ... of the output
// row (a copied column below n_copy, point col - n_copy from there on), so that consecutive lanes write consecutive floats of the row.  Lane 0: the alive term.
__global__ __launch_bounds__(WG) void k_wells_step(WellsDev D, Pose P, const uint8_t* __restrict__ reset, const float* __restrict__ priv, int n_in,
                                                   float* __restrict__ priv_out, float* __restrict__ rew) {
  const int b = blockIdx.x * ENVS_PER_WG + (threadIdx.x / WAVE), t = threadIdx.x % WAVE;
  if (b >= D.n_envs) return;
  const int n_copy = priv ? n_in + EXTRA : 0;                       // without the inner row the output is the scan alone
  const int w = n_copy + D.npts;
  const Base B = load_base(P, b);
  float* __restrict__ prow = priv_out + (size_t)b * w;
  const float* __restrict__ pin = priv ? priv + (size_t)b * n_copy : nullptr;
  for (int col = t; col < w; col += WAVE) {
    float v;
    if (col < n_copy) v = pin[col];
    else { const int k = col - n_copy; v = scan_point(D.F, B.px, B.py, B.pz, B.s, B.c, D.lx[k], D.ly[k]); }
    prow[col] = v;
  }
  if (t == 0 && rew) {                                             // this lane alone reads and writes the env's cells
    rew[b] = rew[b] + D.inc;
    count_term(D, 0, b, D.inc, reset);
  }
}

}  // namespace

struct go2sim_wells {
  int device = 0;
  WellsDev dev = {};
  int n_levels = 1;
};

extern "C" {

int go2sim_wells_create(int device, const go2sim_wells_cfg_t* cfg, const int16_t* hf, const float* xs, const float* ys, go2sim_wells_t** out) {
  if (!out || !cfg || !hf || !xs || !ys) return GO2SIM_E_BADARG;
  const go2sim_wells_cfg_t& c = *cfg;
  if (c.n_envs < 1 || c.nx < 1 || c.nx > GO2SIM_WELLS_AXIS_MAX || c.ny < 1 || c.ny > GO2SIM_WELLS_AXIS_MAX || c.n_levels < 1 || c.n_levels > GO2SIM_WELLS_LEVELS_MAX)
    return GO2SIM_E_BADARG;
  if (!field_args_ok(c.hf_rows, c.hf_cols, c.horizontal_scale) || !(c.dt > 0.0)) return GO2SIM_E_BADARG;
  if (nan_in({c.origin_x, c.origin_y, c.vertical_scale, c.alive_scale})) return GO2SIM_E_BADARG;
  HIPCHK(TAG, hipSetDevice(device));
  go2sim_wells* h = new (std::nothrow) go2sim_wells();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device;
  h->n_levels = c.n_levels;
  WellsDev& D = h->dev;
  const size_t npts = (size_t)c.nx * c.ny;
  std::vector<float> pts(2 * npts);
  for (int i = 0; i < c.nx; ++i)
    for (int j = 0; j < c.ny; ++j) { pts[(size_t)i * c.ny + j] = xs[i]; pts[npts + (size_t)i * c.ny + j] = ys[j]; }
  int rc = upload_field(&D.F, hf, c.hf_rows, c.hf_cols, c.origin_x, c.origin_y, c.horizontal_scale, c.vertical_scale);
  if (rc == GO2SIM_E_OK) rc = dev_array((float**)&D.lx, pts.data(), 2 * npts);
  if (rc == GO2SIM_E_OK) rc = alloc_terms(&D, 1, c.n_envs, c.dt);
  if (rc == GO2SIM_E_OK && hipDeviceSynchronize() != hipSuccess) rc = GO2SIM_E_HIP;
  if (rc != GO2SIM_E_OK) {
    go2sim_wells_destroy(h);
    return rc;
  }
  D.ly = D.lx + npts; D.npts = (int)npts;
  D.inc = (float)(c.alive_scale * c.dt);
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_wells_destroy(go2sim_wells_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree((void*)h->dev.F.hf); (void)hipFree((void*)h->dev.lx); free_terms(&h->dev);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_wells_clear(go2sim_wells_t* h, const int* envs_idx, int n_sel, void* stream) {
  return h ? clear_terms<1>(TAG, h->dev, envs_idx, n_sel, stream) : GO2SIM_E_BADARG;
}

int go2sim_wells_get_alive(go2sim_wells_t* h, float* sum, int32_t* steps, void* stream) {
  if (!h || !sum || !steps) return GO2SIM_E_BADARG;
  const WellsDev& E = h->dev;
  return copy_wait(TAG, hipMemcpyDeviceToHost, stream, {{sum, E.sum, E.n_envs * sizeof(float)}, {steps, E.steps, E.n_envs * sizeof(int)}});
}

int go2sim_wells_set_alive(go2sim_wells_t* h, const float* sum, const int32_t* steps, void* stream) {
  if (!h || !sum || !steps) return GO2SIM_E_BADARG;
  const WellsDev& E = h->dev;
  return copy_wait(TAG, hipMemcpyHostToDevice, stream, {{E.sum, sum, E.n_envs * sizeof(float)}, {E.steps, steps, E.n_envs * sizeof(int)}});
}

int go2sim_wells_alive_ep(go2sim_wells_t* h, const float** alive_ep_dev, float* inc) {
  if (!h || !alive_ep_dev || !inc) return GO2SIM_E_BADARG;
  *alive_ep_dev = h->dev.ep; *inc = h->dev.inc;
  return GO2SIM_E_OK;
}

int go2sim_wells_step(go2sim_wells_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                      long long quat_comp_stride, long long quat_env_stride, const uint8_t* reset, const float* priv, int n_in, float* priv_out,
                      float* rew, void* stream) {
  if (!h || n != h->dev.n_envs || !pose_args_ok(pos, pos_comp_stride, pos_env_stride, quat, quat_comp_stride, quat_env_stride)) return GO2SIM_E_BADARG;
  if (!priv_out || n_in < 0 || n_in > (1 << 20) || (priv == nullptr) != (n_in == 0) || (const float*)priv_out == priv) return GO2SIM_E_BADARG;
  const Pose P = {pos, quat, pos_comp_stride, pos_env_stride, quat_comp_stride, quat_env_stride};
  hipLaunchKernelGGL(k_wells_step, dim3((n + ENVS_PER_WG - 1) / ENVS_PER_WG), dim3(WG), 0, (hipStream_t)stream, h->dev, P, reset, priv, n_in, priv_out, rew);
  HIPCHK(TAG, hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
