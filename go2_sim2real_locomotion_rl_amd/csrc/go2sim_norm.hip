// go2sim_norm.hip -- the empirical observation normaliser (include/go2sim_norm.h): running column statistics and (x - mean) / (std + eps) on gfx950.
// The header states the law, the numeric contract and the launches; this file follows its names.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/go2sim_norm.h"
#include "go2sim_norm_dev.h"   // Mom, mom_merge, fold_chunks, norm_law: shared with go2sim_rnd.hip

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_norm: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

constexpr int MOM_WG = 1024;                // its lanes
constexpr int APPLY_WG = 256, APPLY_ROWS = 32;
enum { MODE_PLAIN = 0, MODE_CHUNKS = 1, MODE_RECORDS = 2 };

// what the kernels see of one handle
struct NormDev {
  float *mean, *var, *sd;        // the state, [d] each
  long long* count;
  float *pmean, *pvar;           // the state as it was when the call began (k_norm_moments / k_norm_snapshot write it, k_norm_apply reads it)
  long long* pcount;
  double* part;                  // [chunk][2][d]: the chunk's column means, then its centred squares
  int d;
  float eps;
  double until;
};
struct NormJob {
  NormDev N;
  const float* x;
  float* y;
};

// column c's moments over the records (rec points at this normaliser's part of record 0), folded in record order; empty records are passed over
__device__ __forceinline__ Mom fold_records(const double* __restrict__ rec, int n_rec, int rec_len, int d, int c) {
  Mom a = {0.0, 0.0, 0.0};
  for (int i = 0; i < n_rec; ++i) {
    const double* r = rec + (size_t)i * rec_len;
    const double nb = r[0];
    if (!(nb > 0.0)) continue;
    if (a.n == 0.0) { a.n = nb; a.mean = r[1 + c]; a.M2 = r[1 + d + c]; }
    else mom_merge(a, nb, r[1 + c], r[1 + d + c]);
  }
  return a;
}

// One workgroup per chunk of CH rows (blockIdx.x) and normaliser (blockIdx.y).  The chunk is CH * d consecutive floats; with W = min(d, 1024) and
// R = 1024 / W, lane t = rl * W + cl (rl < R) owns column c0 + cl and the chunk's rows rl, rl + R, ...: a pass reads R consecutive rows with consecutive lanes.
__global__ __launch_bounds__(MOM_WG) void k_norm_moments(NormJob j0, NormJob j1, int n_rows, int snapshot) {
  __shared__ double red[MOM_WG];
  __shared__ double cm[MOM_WG];
  const NormJob& J = blockIdx.y ? j1 : j0;
  const int d = J.N.d, t = threadIdx.x;
  const int W = min(d, MOM_WG), R = MOM_WG / W, rl = t / W, cl = t - rl * W;
  const int lo = blockIdx.x * CH, hi = min(n_rows, lo + CH);
  if (snapshot && blockIdx.x == 0) {
    for (int c = t; c < d; c += MOM_WG) { J.N.pmean[c] = J.N.mean[c]; J.N.pvar[c] = J.N.var[c]; }
    if (t == 0) *J.N.pcount = *J.N.count;
  }
  const float* __restrict__ x = J.x;
  for (int c0 = 0; c0 < d; c0 += W) {
    const int c = c0 + cl;
    const bool own = rl < R && c < d;
    double s = 0.0;
    if (own) {
#pragma unroll 8
      for (int r = lo + rl; r < hi; r += R) s += (double)x[(size_t)r * d + c];
    }
    red[t] = s;
    __syncthreads();
    if (t < W) {
      double a = 0.0;
      for (int k = 0; k < R; ++k) a += red[k * W + t];
      cm[t] = a / (double)(hi - lo);
    }
    __syncthreads();
    const double mu = cm[cl];
    double q = 0.0;
    if (own) {
#pragma unroll 8
      for (int r = lo + rl; r < hi; r += R) { const double e = (double)x[(size_t)r * d + c] - mu; q += e * e; }
    }
    red[t] = q;
    __syncthreads();
    if (t < W && c0 + t < d) {
      double a = 0.0;
      for (int k = 0; k < R; ++k) a += red[k * W + t];
      J.N.part[(size_t)(2 * blockIdx.x) * d + c0 + t] = cm[t];
      J.N.part[(size_t)(2 * blockIdx.x + 1) * d + c0 + t] = a;
    }
    __syncthreads();
  }
}

// the chunk moments of go2sim_norm_moments as one record per normaliser: n, mean[d], M2[d]
__global__ __launch_bounds__(APPLY_WG) void k_norm_record(NormJob j0, NormJob j1, int n_rows, double* __restrict__ record, int off1) {
  const NormJob& J = blockIdx.y ? j1 : j0;
  double* rec = record + (blockIdx.y ? off1 : 0);
  const int d = J.N.d, c = blockIdx.x * APPLY_WG + threadIdx.x;
  if (c >= d) return;
  Mom a = {0.0, 0.0, 0.0};
  if (n_rows > 0) a = fold_chunks(J.N.part, d, c, n_rows);
  if (c == 0) rec[0] = a.n;
  rec[1 + c] = a.mean;
  rec[1 + d + c] = a.M2;
}

__global__ __launch_bounds__(APPLY_WG) void k_norm_snapshot(NormJob j0, NormJob j1) {
  const NormJob& J = blockIdx.y ? j1 : j0;
  const int c = blockIdx.x * APPLY_WG + threadIdx.x;
  if (c < J.N.d) { J.N.pmean[c] = J.N.mean[c]; J.N.pvar[c] = J.N.var[c]; }
  if (c == 0) *J.N.pcount = *J.N.count;
}

// APPLY_ROWS rows per workgroup (blockIdx.x) and normaliser (blockIdx.y); lane t = rl * W + cl owns column c0 + cl of the rows rl, rl + R, ... as above.
// MODE_PLAIN reads the live state and writes none of it.  The other modes read the copy the call's first launch made: whether the statistics move is the
// same for every workgroup (the copied count, the batch's n), and only then workgroup 0 stores the new state, which no lane of this launch reads.
__global__ __launch_bounds__(APPLY_WG) void k_norm_apply(NormJob j0, NormJob j1, int n_rows, int mode, const double* __restrict__ records, int n_rec,
                                                         int rec_len, int off1) {
  const NormJob& J = blockIdx.y ? j1 : j0;
  const int d = J.N.d, t = threadIdx.x;
  const int W = min(d, APPLY_WG), R = APPLY_WG / W, rl = t / W, cl = t - rl * W;
  if (rl >= R) return;
  const double* rec = records + (blockIdx.y ? off1 : 0);
  bool move = false;
  long long cnt = 0;
  if (mode != MODE_PLAIN) {
    cnt = *J.N.pcount;
    move = !(J.N.until > 0.0) || (double)cnt < J.N.until;
  }
  const int row0 = blockIdx.x * APPLY_ROWS, row1 = min(n_rows, row0 + APPLY_ROWS);
  const float* __restrict__ x = J.x;
  float* __restrict__ y = J.y;
  for (int c = cl; c < d; c += W) {
    float m32, s32;
    Mom b = {0.0, 0.0, 0.0};
    if (move) b = mode == MODE_CHUNKS ? fold_chunks(J.N.part, d, c, n_rows) : fold_records(rec, n_rec, rec_len, d, c);
    if (move && b.n > 0.0) {                                   // b.n is the same in every column
      const double m = (double)J.N.pmean[c], v = (double)J.N.pvar[c];
      double m1, v1;
      norm_law(m, v, cnt, b, m1, v1);
      m32 = (float)m1;
      s32 = (float)sqrt(v1);
      if (blockIdx.x == 0 && rl == 0) {
        J.N.mean[c] = m32; J.N.var[c] = (float)v1; J.N.sd[c] = s32;
        if (c == 0) *J.N.count = cnt + (long long)b.n;
      }
    } else {
      m32 = J.N.mean[c]; s32 = J.N.sd[c];
    }
    const float den = s32 + J.N.eps;
#pragma unroll 4
    for (int r = row0 + rl; r < row1; r += R) y[(size_t)r * d + c] = (x[(size_t)r * d + c] - m32) / den;
  }
}

}  // namespace

struct go2sim_norm {
  int device = 0, d = 0;
  NormDev dev = {};
  void* state = nullptr;                  // count, pcount | mean, var, sd, pmean, pvar
  int part_chunks = 0;                    // chunks the workspace holds
  std::vector<double*> parts;             // every workspace ever allocated (the last is in use); freed by go2sim_norm_destroy
};

namespace {

int ensure_chunks(go2sim_norm* h, int n_rows) {
  const int nch = (n_rows + CH - 1) / CH;
  if (nch <= h->part_chunks) return GO2SIM_E_OK;
  int cap = h->part_chunks > 0 ? h->part_chunks : 16;
  while (cap < nch) cap *= 2;
  double* p = nullptr;
  if (hipMalloc((void**)&p, (size_t)cap * 2 * h->d * sizeof(double)) != hipSuccess) return GO2SIM_E_NOMEM;
  h->parts.push_back(p);
  h->dev.part = p;
  h->part_chunks = cap;
  return GO2SIM_E_OK;
}

// the argument checks of the two stepping calls; x and y may be NULL only where no row is read
int check_step(go2sim_norm* a, const float* x_a, float* y_a, go2sim_norm* b, const float* x_b, float* y_b, int n_rows) {
  if (!a || n_rows < 0 || (b && (b == a || b->device != a->device))) return GO2SIM_E_BADARG;
  if (n_rows > 0 && (!x_a || !y_a || (const float*)y_a == x_a)) return GO2SIM_E_BADARG;
  if (n_rows > 0 && b && (!x_b || !y_b || (const float*)y_b == x_b)) return GO2SIM_E_BADARG;
  return GO2SIM_E_OK;
}

inline int max_d(const go2sim_norm* a, const go2sim_norm* b) { return b && b->d > a->d ? b->d : a->d; }

}  // namespace

extern "C" {

int go2sim_norm_create(int device, int n_features, double eps, double until, go2sim_norm_t** out) {
  if (!out || n_features < 1 || n_features > (1 << 24) || !(eps >= 0.0) || until != until) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(device));
  go2sim_norm* h = new (std::nothrow) go2sim_norm();
  if (!h) return GO2SIM_E_NOMEM;
  const size_t d = (size_t)n_features;
  h->device = device; h->d = n_features;
  if (hipMalloc(&h->state, 2 * sizeof(long long) + 5 * d * sizeof(float)) != hipSuccess) { delete h; return GO2SIM_E_NOMEM; }
  NormDev& N = h->dev;
  N.count = (long long*)h->state; N.pcount = N.count + 1;
  N.mean = (float*)(N.count + 2); N.var = N.mean + d; N.sd = N.var + d; N.pmean = N.sd + d; N.pvar = N.pmean + d;
  N.d = n_features; N.eps = (float)eps; N.until = until;
  if (ensure_chunks(h, 16 * CH) != GO2SIM_E_OK) { (void)hipFree(h->state); delete h; return GO2SIM_E_NOMEM; }
  std::vector<float> zero(d, 0.0f), one(d, 1.0f);
  const int rc = go2sim_norm_set_state(h, zero.data(), one.data(), one.data(), 0, nullptr);
  if (rc != GO2SIM_E_OK) { go2sim_norm_destroy(h); return rc; }
  HIPCHK(hipDeviceSynchronize());
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_norm_destroy(go2sim_norm_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  for (double* p : h->parts) (void)hipFree(p);
  (void)hipFree(h->state);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_norm_get_state(go2sim_norm_t* h, float* mean, float* var, float* std, int64_t* count, void* stream) {
  if (!h || !mean || !var || !std || !count) return GO2SIM_E_BADARG;
  const size_t nb = (size_t)h->d * sizeof(float);
  long long cnt = 0;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(mean, h->dev.mean, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(var, h->dev.var, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(std, h->dev.sd, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&cnt, h->dev.count, sizeof(cnt), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *count = (int64_t)cnt;
  return GO2SIM_E_OK;
}

int go2sim_norm_set_state(go2sim_norm_t* h, const float* mean, const float* var, const float* std, int64_t count, void* stream) {
  if (!h || !mean || !var || !std || count < 0) return GO2SIM_E_BADARG;
  const size_t nb = (size_t)h->d * sizeof(float);
  const long long cnt = (long long)count;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(h->dev.mean, mean, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dev.var, var, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dev.sd, std, nb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->dev.count, &cnt, sizeof(cnt), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                          // the sources are the caller's (and this frame's) host memory
  return GO2SIM_E_OK;
}

int go2sim_norm_step(go2sim_norm_t* a, const float* x_a, float* y_a, go2sim_norm_t* b, const float* x_b, float* y_b, int n_rows, int update, void* stream) {
  int rc = check_step(a, x_a, y_a, b, x_b, y_b, n_rows);
  if (rc != GO2SIM_E_OK || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (update) {
    if ((rc = ensure_chunks(a, n_rows)) != GO2SIM_E_OK || (b && (rc = ensure_chunks(b, n_rows)) != GO2SIM_E_OK)) return rc;
  }
  NormJob j0 = {a->dev, x_a, y_a}, j1 = {b ? b->dev : a->dev, x_b, y_b};
  const int nj = b ? 2 : 1;
  if (update) {
    hipLaunchKernelGGL(k_norm_moments, dim3((n_rows + CH - 1) / CH, nj), dim3(MOM_WG), 0, s, j0, j1, n_rows, 1);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_norm_apply, dim3((n_rows + APPLY_ROWS - 1) / APPLY_ROWS, nj), dim3(APPLY_WG), 0, s, j0, j1, n_rows, update ? MODE_CHUNKS : MODE_PLAIN,
                     (const double*)nullptr, 0, 0, 0);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_norm_record_len(go2sim_norm_t* a, go2sim_norm_t* b, int* len) {
  if (!a || !len) return GO2SIM_E_BADARG;
  *len = 1 + 2 * a->d + (b ? 1 + 2 * b->d : 0);
  return GO2SIM_E_OK;
}

int go2sim_norm_moments(go2sim_norm_t* a, const float* x_a, go2sim_norm_t* b, const float* x_b, int n_rows, double* record_dev, void* stream) {
  if (!a || !record_dev || n_rows < 0 || (b && (b == a || b->device != a->device))) return GO2SIM_E_BADARG;
  if (n_rows > 0 && (!x_a || (b && !x_b))) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = ensure_chunks(a, n_rows)) != GO2SIM_E_OK || (b && (rc = ensure_chunks(b, n_rows)) != GO2SIM_E_OK)) return rc;
  NormJob j0 = {a->dev, x_a, nullptr}, j1 = {b ? b->dev : a->dev, x_b, nullptr};
  const int nj = b ? 2 : 1;
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_norm_moments, dim3((n_rows + CH - 1) / CH, nj), dim3(MOM_WG), 0, s, j0, j1, n_rows, 0);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_norm_record, dim3((max_d(a, b) + APPLY_WG - 1) / APPLY_WG, nj), dim3(APPLY_WG), 0, s, j0, j1, n_rows, record_dev, 1 + 2 * a->d);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_norm_merge_step(go2sim_norm_t* a, const float* x_a, float* y_a, go2sim_norm_t* b, const float* x_b, float* y_b, int n_rows, const double* records_dev,
                           int n_records, int update, void* stream) {
  const int rc = check_step(a, x_a, y_a, b, x_b, y_b, n_rows);
  if (rc != GO2SIM_E_OK) return rc;
  if (n_records < 0 || (n_records > 0 && !records_dev)) return GO2SIM_E_BADARG;
  const bool upd = update && n_records > 0;
  if (n_rows == 0 && !upd) return GO2SIM_E_OK;
  hipStream_t s = (hipStream_t)stream;
  NormJob j0 = {a->dev, x_a, y_a}, j1 = {b ? b->dev : a->dev, x_b, y_b};
  const int nj = b ? 2 : 1;
  int len = 0;
  (void)go2sim_norm_record_len(a, b, &len);
  if (upd) {
    hipLaunchKernelGGL(k_norm_snapshot, dim3((max_d(a, b) + APPLY_WG - 1) / APPLY_WG, nj), dim3(APPLY_WG), 0, s, j0, j1);
    HIPCHK(hipGetLastError());
  }
  const int blocks = n_rows > 0 ? (n_rows + APPLY_ROWS - 1) / APPLY_ROWS : 1;
  hipLaunchKernelGGL(k_norm_apply, dim3(blocks, nj), dim3(APPLY_WG), 0, s, j0, j1, n_rows, upd ? MODE_RECORDS : MODE_PLAIN, records_dev, n_records, len, 1 + 2 * a->d);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
