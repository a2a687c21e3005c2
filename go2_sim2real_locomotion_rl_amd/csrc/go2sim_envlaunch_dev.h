// go2sim_envlaunch_dev.h -- what the env's after-step launches share (csrc/go2sim_lidar.hip, go2sim_stairinfo.hip, go2sim_wells.hip, go2sim_cterms.hip):
// the heightfield view and its two body-frame lookups, the base pose, the DR level, the stored-row memory, the episode terms, and the host helpers of
// the create / get / set / clear entry points.  The public headers state the laws; every operation sequence here is theirs (-ffp-contract=off).
// A Dev struct goes to its kernel by value, and its member order is the kernel's argument layout.  So the functions here are templates on the members
// they name: `F` is Field or a Dev struct with Field's members, `E` a Dev struct with the episode terms' members.
#ifndef GO2SIM_ENVLAUNCH_DEV_H
#define GO2SIM_ENVLAUNCH_DEV_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/go2sim.h"
#include "../../include/go2sim_detmath.h"

namespace {

constexpr int WAVE = 64, WG = 256, ENVS_PER_WG = WG / WAVE;

// ---- the heightfield: members hf, rows, cols, ox, oy, hs ------------------------------------------------------------------------------------------
struct Field {
  const float* hf;          // [rows][cols] metres, rows along world x
  int rows, cols;           // >= 1 each
  float ox, oy, hs;         // world position of cell (0, 0), cell size
};

// trunc toward zero, then clamp to [0, n - 1], by comparisons a NaN fails (it selects 0): never an index outside the field
__device__ __forceinline__ int cell_index(float q, int n) {
  if (!(q >= 1.0f)) return 0;                    // negatives, [0, 1) and NaN
  if (q >= (float)(n - 1)) return n - 1;         // +inf included
  return (int)q;
}

// the scans' lookup: the point (lx, ly) of the body frame of an env at (px, py, pz) with yaw sine s and cosine c, relative to the base height
template <class F_>
__device__ __forceinline__ float scan_point(const F_& F, float px, float py, float pz, float s, float c, float lx, float ly) {
  const float wx = px + c * lx - s * ly;
  const float wy = py + s * lx + c * ly;
  const int col = cell_index((wx - F.ox) / F.hs, F.rows);
  const int row = cell_index((wy - F.oy) / F.hs, F.cols);
  return F.hf[(size_t)col * F.cols + row] - pz;
}

// the stair info's lookup: forward only, the field's own height
template <class F_>
__device__ __forceinline__ float height_ahead(const F_& F, float px, float py, float s, float c, float lx) {
  const float wx = px + c * lx;
  const float wy = py + s * lx;
  const int col = cell_index((wx - F.ox) / F.hs, F.rows);
  const int row = cell_index((wy - F.oy) / F.hs, F.cols);
  return F.hf[(size_t)col * F.cols + row];
}

// ---- the base pose -----------------------------------------------------------------------------------------------------------------------------
struct Pose {
  const float *pos, *quat;
  long long pcs, pes, qcs, qes;     // component and env strides, in elements
};

struct Base {
  float px, py, pz, s, c;           // position, sine and cosine of the yaw
};

__device__ __forceinline__ Base load_base(const Pose& P, int b) {
  Base B;
  B.px = P.pos[(size_t)b * P.pes]; B.py = P.pos[P.pcs + (size_t)b * P.pes]; B.pz = P.pos[2 * P.pcs + (size_t)b * P.pes];
  const float qw = P.quat[(size_t)b * P.qes], qx = P.quat[P.qcs + (size_t)b * P.qes], qy = P.quat[2 * P.qcs + (size_t)b * P.qes],
              qz = P.quat[3 * P.qcs + (size_t)b * P.qes];
  const float yaw = dm_atan2(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
  dm_sincos(yaw, &B.s, &B.c);
  return B;
}

inline bool pose_args_ok(const float* pos, long long pcs, long long pes, const float* quat, long long qcs, long long qes) {
  return pos && quat && pcs >= 0 && pes >= 0 && qcs >= 0 && qes >= 0;
}

// the inner rows of the two layouts that widen both rows: both or neither, and no output row on top of another row
inline bool rows_args_ok(const float* obs, const float* priv, int n_in, const float* obs_out, const float* priv_out) {
  if (!obs_out || !priv_out || n_in < 0 || n_in > (1 << 20)) return false;
  if ((obs == nullptr) != (priv == nullptr) || (obs == nullptr) != (n_in == 0)) return false;
  return obs_out != priv_out && !(obs && (obs_out == obs || obs_out == priv || priv_out == obs || priv_out == priv));
}

// ---- the DR level: _get_dr_level, go2_env_stair_lidar.py:1197-1220 and go2_env_stair_lidar_2.py --------------------------------------------------
struct DrSched {
  double phase1, gate;
  int dr_schedule, curriculum_enabled;
};

// of the curriculum level the env's globals hold (read only with the curriculum enabled)
__device__ __forceinline__ double dr_level(const DrSched& S, const double* level) {
  const double t = S.curriculum_enabled ? *level : 1.0;
  if (!S.dr_schedule) return t;
  if (t < S.gate) return S.phase1;
  double den = 1.0 - S.gate;
  if (den < 1e-6) den = 1e-6;
  double pr = (t - S.gate) / den;
  pr = pr < 0.0 ? 0.0 : (pr > 1.0 ? 1.0 : pr);
  return S.phase1 + (1.0 - S.phase1) * pr;
}

// ---- the episode terms: members float *sum, *ep (one allocation, sum | ep) and int* steps, each [NT][n_envs]; int n_envs; float dt ------------------

// "ep_t[b] = sum_t[b] / (f32(max(steps_t[b], 1)) * f32(dt))", then both := 0
template <class E_>
__device__ __forceinline__ void hand_over(const E_& E, int t, int b, float sum, int steps) {
  const size_t k = (size_t)t * E.n_envs + b;
  const float ep_steps = (float)(steps < 1 ? 1 : steps);
  E.ep[k] = sum / (ep_steps * E.dt);
  E.sum[k] = 0.0f;
  E.steps[k] = 0;
}

// env b's reset flag: a kernel with several terms reads it once and hands the value on, a kernel with one term hands the array on (read after the sums)
__device__ __forceinline__ bool reset_flag(bool flag, int) { return flag; }
__device__ __forceinline__ bool reset_flag(const uint8_t* reset, int b) { return reset && reset[b]; }

// "sum_t[b] = sum_t[b] + term; steps_t[b] += 1", then the hand-over of a reset env; -> term, for the caller's "rew[b] = rew[b] + term"
template <class E_, class R_>
__device__ __forceinline__ float count_term(const E_& E, int t, int b, float term, R_ reset) {
  const size_t k = (size_t)t * E.n_envs + b;
  const float sum = E.sum[k] + term;
  const int steps = E.steps[k] + 1;
  if (reset_flag(reset, b)) hand_over(E, t, b, sum, steps);
  else { E.sum[k] = sum; E.steps[k] = steps; }
  return term;
}

// the hand-over without a step, one lane per selected env
template <int NT, class E_>
__global__ __launch_bounds__(WG) void k_terms_clear(E_ E, const int* __restrict__ idx, int n_sel) {
  const int r = blockIdx.x * WG + threadIdx.x;
  if (r >= (idx ? n_sel : E.n_envs)) return;
  const int b = idx ? idx[r] : r;
  if (b < 0 || b >= E.n_envs) return;
  for (int t = 0; t < NT; ++t) hand_over(E, t, b, E.sum[(size_t)t * E.n_envs + b], E.steps[(size_t)t * E.n_envs + b]);
}

// ---- the stored rows [n_envs][width]: := 0, one lane per cell of a selected env -------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_rows_clear(float* __restrict__ stored, int n_envs, int width, const int* __restrict__ idx, int n_sel) {
  const long long i = (long long)blockIdx.x * WG + threadIdx.x, total = (long long)(idx ? n_sel : n_envs) * width;
  if (i >= total) return;
  const int r = (int)(i / width), k = (int)(i - (long long)r * width);
  const int b = idx ? idx[r] : r;
  if (b >= 0 && b < n_envs) stored[(size_t)b * width + k] = 0.0f;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------------
#define HIPCHK(tag, x)                                                                              \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s failed: %s\n", tag, #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

inline bool nan_in(std::initializer_list<double> values) {
  for (double v : values)
    if (v != v) return true;
  return false;
}

// n elements on the device, a copy of `host` or zeros; the caller waits for the device and frees *p whatever the status
template <class T>
int dev_array(T** p, const T* host, size_t n) {
  if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) return GO2SIM_E_NOMEM;
  const hipError_t e = host ? hipMemcpy(*p, host, n * sizeof(T), hipMemcpyHostToDevice) : hipMemset(*p, 0, n * sizeof(T));
  return e == hipSuccess ? GO2SIM_E_OK : GO2SIM_E_HIP;
}

inline bool field_args_ok(int rows, int cols, double horizontal_scale) {
  return rows >= 1 && cols >= 1 && (long long)rows * cols <= (1LL << 30) && horizontal_scale > 0.0;
}

// the int16 field in metres, as go2sim_set_terrain forms the env's own copy; free with hipFree((void*)F->hf)
template <class F_>
int upload_field(F_* F, const int16_t* hf, int rows, int cols, double ox, double oy, double horizontal_scale, double vertical_scale) {
  std::vector<float> metres((size_t)rows * cols);
  for (size_t k = 0; k < metres.size(); ++k) metres[k] = (float)hf[k] * (float)vertical_scale;
  F->rows = rows; F->cols = cols; F->ox = (float)ox; F->oy = (float)oy; F->hs = (float)horizontal_scale;
  return dev_array((float**)&F->hf, metres.data(), metres.size());
}

template <class E_>
int alloc_terms(E_* E, int nt, int n_envs, double dt) {
  const size_t n = (size_t)nt * n_envs;
  E->n_envs = n_envs; E->dt = (float)dt;
  const int rc = dev_array(&E->sum, (const float*)nullptr, 2 * n);
  if (rc != GO2SIM_E_OK) return rc;
  E->ep = E->sum + n;
  return dev_array(&E->steps, (const int*)nullptr, n);
}

template <class E_>
void free_terms(E_* E) { (void)hipFree(E->sum); (void)hipFree(E->steps); }

// copies between the caller's host memory and the device, in order on the stream, then the wait (a host source must outlive the copy)
struct Span {
  void* dst;
  const void* src;
  size_t bytes;
};

inline int copy_wait(const char* tag, hipMemcpyKind kind, void* stream, std::initializer_list<Span> spans) {
  hipStream_t s = (hipStream_t)stream;
  for (const Span& c : spans)
    if (c.bytes) HIPCHK(tag, hipMemcpyAsync(c.dst, c.src, c.bytes, kind, s));
  HIPCHK(tag, hipStreamSynchronize(s));
  return GO2SIM_E_OK;
}

inline int clear_rows(const char* tag, float* stored, int n_envs, int width, const int* envs_idx, int n_sel, void* stream) {
  if (envs_idx && n_sel < 0) return GO2SIM_E_BADARG;
  const long long total = (long long)(envs_idx ? n_sel : n_envs) * width;
  if (total == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL(k_rows_clear, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, stored, n_envs, width, envs_idx, n_sel);
  HIPCHK(tag, hipGetLastError());
  return GO2SIM_E_OK;
}

template <int NT, class E_>
int clear_terms(const char* tag, const E_& E, const int* envs_idx, int n_sel, void* stream) {
  if (envs_idx && n_sel < 0) return GO2SIM_E_BADARG;
  const int total = envs_idx ? n_sel : E.n_envs;
  if (total == 0) return GO2SIM_E_OK;
  hipLaunchKernelGGL((k_terms_clear<NT, E_>), dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, E, envs_idx, n_sel);
  HIPCHK(tag, hipGetLastError());
  return GO2SIM_E_OK;
}

}  // namespace

#endif
