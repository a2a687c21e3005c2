// go2sim_distill.hip -- teacher-student distillation (include/go2sim_distill.h): the collection step that runs student and teacher in one launch and the
// behaviour-cloning update of the student.  gfx950 only.
//
// The collection step is the policy step's two kernels (go2sim_mlp_dev.h): k_mlp_forward with the teacher where the critic sits, k_policy_sample on the
// student's mean.  A window of the update is walked in sub-batches of sub_rows rows; one sub-batch is, on the caller's stream and without atomics,
//   k_train_forward     (go2sim_train_dev.h) the student's forward with the hidden activations kept, rows read through the window's index list
//   k_distill_head      one row per lane: residual, rho into a float64 per-workgroup partial, rho' / (N A) into dZ [rows][Apad] with zero padding
//   per layer, last to first: k_bwd_dw, k_bwd_db, k_bwd_da   (go2sim_train_dev.h, one network per launch)
//   k_reduce_partials   (one sub-batch) or k_distill_accumulate (several): the chunk slabs added in chunk order in float64; the second keeps the float64 sum
//                       across sub-batches and rounds after the last one, which is the same sequence of additions as one pass over all chunks
// and after the last sub-batch k_distill_finalize adds the head's partials of the whole window in workgroup order.  The optimizer is k_sumsq + k_adam of
// the PPO update over the student's padded parameters alone (no critic, no std block).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <new>
#include <vector>

#define GO2SIM_MLP_ACT_KERNELS
#include "go2sim_mlp_dev.h"
#include "go2sim_train_dev.h"
#include "../../include/go2sim_distill.h"

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_distill: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

// the handle's scalar block has the layout k_adam knows (S_LR, S_NORM); the running sum of the pairs' losses takes a slot the PPO sums use there
constexpr int D_SUM_LOSS = S_SUM_VL;

struct DistillHeadArgs {
  const float* mu;             // [n][A]: this sub-batch's forward
  const float* teacher;        // [.][A], rows through idx
  const int32_t* idx;
  float* dz;                   // [n][Apad]
  double* part;                // [workgroups]
  int n, A, Apad, huber;
  double w;                    // 1 / (N A)
};

// One row per lane.  The loop runs over the Apad columns of dZ whatever the data; padded columns and nothing else get an exact zero.
__global__ __launch_bounds__(WGT) void k_distill_head(DistillHeadArgs h) {
  __shared__ double s_red[WGT];
  const int r = blockIdx.x * WGT + threadIdx.x;
  double sum = 0.0;
  if (r < h.n) {
    const size_t src = (size_t)h.idx[r];
    for (int a = 0; a < h.Apad; ++a) {
      float g = 0.0f;
      if (a < h.A) {
        const double d = (double)h.mu[(size_t)r * h.A + a] - (double)h.teacher[src * h.A + a];
        double rho, drho;
        if (h.huber) {
          const double ad = fabs(d);
          rho = ad <= 1.0 ? 0.5 * d * d : ad - 0.5;
          drho = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
        } else {
          rho = d * d;
          drho = 2.0 * d;
        }
        sum += rho;
        g = (float)(drho * h.w);
      }
      h.dz[(size_t)r * h.Apad + a] = g;
    }
  }
  const double t = wg_sum(s_red, sum);
  if (threadIdx.x == 0) h.part[blockIdx.x] = t;
}

// one thread: the window's (or the tail's) head partials in workgroup order, weighted once, onto the running sum
__global__ void k_distill_finalize(const double* __restrict__ part, int n_wg, double w, double* __restrict__ scal) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < n_wg; ++i) s += part[i];
  scal[D_SUM_LOSS] += s * w;
}

// k_reduce_partials across sub-batches: entry i continues the float64 sum of the earlier sub-batches' chunks (first: from zero) and is rounded into the
// gradient vector after the last one
__global__ __launch_bounds__(WGT) void k_distill_accumulate(const float* __restrict__ partial, int n_chunks, size_t slab, double* __restrict__ acc, int first, int last,
                                                            float* __restrict__ grads) {
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= slab) return;
  double s = first ? 0.0 : acc[i];
  for (int c = 0; c < n_chunks; ++c) s += (double)partial[(size_t)c * slab + i];
  if (last) grads[i] = (float)s;
  else acc[i] = s;
}

// the row-index list of one update: entry cnt N + j is row (cnt % T) N + j, cnt over the E T pairs in the order the windows take them
__global__ __launch_bounds__(WGT) void k_distill_rows(int32_t* __restrict__ idx, long long total, int T, int N) {
  const long long i = (long long)blockIdx.x * WGT + threadIdx.x;
  if (i >= total) return;
  const long long cnt = i / N;
  idx[i] = (int32_t)((cnt % T) * N + (i - cnt * N));
}

__global__ void k_distill_reset(double* scal) { if (blockIdx.x == 0 && threadIdx.x == 0) scal[D_SUM_LOSS] = 0.0; }
__global__ void k_distill_stats(const double* __restrict__ scal, double step, double pairs, double windows, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  out[GO2SIM_DISTILL_ST_LOSS] = scal[D_SUM_LOSS] / (pairs > 0.0 ? pairs : 1.0);
  out[GO2SIM_DISTILL_ST_LR] = scal[S_LR]; out[GO2SIM_DISTILL_ST_GRAD_NORM] = scal[S_NORM];
  out[GO2SIM_DISTILL_ST_STEP] = step; out[GO2SIM_DISTILL_ST_PAIRS] = pairs; out[GO2SIM_DISTILL_ST_WINDOWS] = windows;
}

struct DSeg { size_t pad_off; int ld, rows, cols; size_t flat_off; };

}  // namespace

struct go2sim_distill {
  go2sim_mlp* student = nullptr;
  go2sim_distill_cfg_t cfg{};
  int A = 0, Apad = 0, max_rows = 0, sub = 0, ws_rows = 0;
  size_t nP = 0, n_flat = 0;   // padded / flat size of the student's parameters
  float* fbuf = nullptr;      // grads | m | v
  float* wbuf = nullptr;      // mu | activations | dz ping-pong | partial slabs, for ws_rows rows
  float *grads = nullptr, *m = nullptr, *v = nullptr, *mu = nullptr, *partial = nullptr;
  ActWs ws{};
  float* dz[2] = {nullptr, nullptr};
  double* dbuf = nullptr;     // scal[S_N] | sq_part[NORM_WG] | acc[nP] | head partials
  double *scal = nullptr, *sq_part = nullptr, *acc = nullptr, *head_part = nullptr;
  int max_head_wg = 0;
  long long step = 0, pairs = 0, windows = 0;
  int32_t* rows = nullptr;    // the row-index list of go2sim_distill_update, for (rows_T, rows_N, rows_E)
  int rows_T = 0, rows_N = 0, rows_E = 0;
  std::vector<DSeg> segs;
};

namespace {

BwdLayer student_layer(const go2sim_distill* h, int lb, const float* obs) {
  const go2sim_mlp* M = h->student;
  BwdLayer L{};
  const int l = M->n_layers - 1 - lb;                      // lb counts from the last layer
  if (l < 0) return L;
  L.active = 1;
  L.N = M->dev.npad[l]; L.K = M->dev.kpad[l]; L.act = M->dev.act;
  L.dz = h->dz[l & 1];
  L.W = M->dev.W[l];
  if (l == 0) { L.aprev = obs; L.lda = M->dims[0]; L.kmax = M->dims[0]; L.gather = 1; L.dzprev = nullptr; }
  else { L.aprev = h->ws.a[l - 1]; L.lda = L.K; L.kmax = L.K; L.gather = 0; L.dzprev = h->dz[(l - 1) & 1]; }
  L.w_off = (size_t)(M->dev.W[l] - M->dparams);
  L.b_off = (size_t)(M->dev.b[l] - M->dparams);
  return L;
}

float* vec_of(go2sim_distill* h, int which) {
  return which == GO2SIM_DISTILL_PARAMS ? h->student->dparams : which == GO2SIM_DISTILL_GRADS ? h->grads : which == GO2SIM_DISTILL_ADAM_M ? h->m
         : which == GO2SIM_DISTILL_ADAM_V ? h->v : nullptr;
}

// forward and head of rows idx[0 .. n), with `backward` the gradient as well; the running loss sum moves by the rows' sum of rho / (N A)
int launch_window(go2sim_distill* h, const float* obs, const float* teacher, const int32_t* idx, int n, int n_envs, bool backward, hipStream_t st) {
  const go2sim_mlp* M = h->student;
  const double w = 1.0 / ((double)n_envs * (double)h->A);
  const int nsub = (n + h->sub - 1) / h->sub;
  const size_t slab = h->nP;
  const BwdLayer off_layer{};                              // the second network's slot of the shared kernels stays empty
  for (int s = 0; s < nsub; ++s) {
    const int off = s * h->sub, m = n - off < h->sub ? n - off : h->sub;
    const int32_t* ix = idx + off;
    hipLaunchKernelGGL(k_train_forward<false>, dim3((m + TM - 1) / TM, 1), dim3(64 * NWAVE), 0, st, M->dev, obs, h->mu, h->ws, M->dev, obs, h->mu, h->ws, ix, m, m,
                       MirTab{nullptr, nullptr}, MirTab{nullptr, nullptr});
    DistillHeadArgs ha{};
    ha.mu = h->mu; ha.teacher = teacher; ha.idx = ix; ha.dz = h->dz[(M->n_layers - 1) & 1]; ha.part = h->head_part + off / WGT;
    ha.n = m; ha.A = h->A; ha.Apad = h->Apad; ha.huber = h->cfg.loss_type == GO2SIM_DISTILL_HUBER; ha.w = w;
    hipLaunchKernelGGL(k_distill_head, dim3((m + WGT - 1) / WGT), dim3(WGT), 0, st, ha);
    if (!backward) continue;
    const int n_chunks = (m + RCH - 1) / RCH;
    for (int lb = 0; lb < M->n_layers; ++lb) {
      const BwdLayer L = student_layer(h, lb, obs);
      const int groups = ((L.N / 16 + DW_TN - 1) / DW_TN) * ((L.K / 16 + DW_TK - 1) / DW_TK);
      hipLaunchKernelGGL(k_bwd_dw<false>, dim3(groups, n_chunks, 1), dim3(WGT), 0, st, L, off_layer, ix, m, m, h->partial, slab);
      hipLaunchKernelGGL(k_bwd_db, dim3(L.N / 16, n_chunks, 1), dim3(WGT), 0, st, L, off_layer, m, h->partial, slab);
      if (L.dzprev) hipLaunchKernelGGL(k_bwd_da<false>, dim3((m + TM - 1) / TM, 1), dim3(64 * NWAVE), 0, st, L, off_layer, m);
    }
    const dim3 grid((unsigned)((slab + WGT - 1) / WGT));
    if (nsub == 1) hipLaunchKernelGGL(k_reduce_partials, grid, dim3(WGT), 0, st, h->partial, n_chunks, slab, h->grads);
    else hipLaunchKernelGGL(k_distill_accumulate, grid, dim3(WGT), 0, st, h->partial, n_chunks, slab, h->acc, s == 0 ? 1 : 0, s == nsub - 1 ? 1 : 0, h->grads);
  }
  hipLaunchKernelGGL(k_distill_finalize, dim3(1), dim3(1), 0, st, h->head_part, (n + WGT - 1) / WGT, w, h->scal);
  HIPCHK(hipGetLastError());
  h->pairs += n / n_envs;
  return GO2SIM_E_OK;
}

bool window_ok(const go2sim_distill* h, const float* obs, const float* teacher, const int32_t* idx, int n_rows, int n_envs) {
  return h && obs && teacher && idx && n_envs >= 1 && n_rows >= 1 && n_rows <= h->max_rows && n_rows % n_envs == 0;
}

int pack_all(go2sim_distill* h, int which, int to_padded, float* flat, hipStream_t st) {
  if (!h || !flat || !vec_of(h, which)) return GO2SIM_E_BADARG;
  float* base = vec_of(h, which);
  for (const DSeg& s : h->segs)
    hipLaunchKernelGGL(k_pack, dim3((s.rows * s.cols + WGT - 1) / WGT), dim3(WGT), 0, st, to_padded, base + s.pad_off, s.ld, flat + s.flat_off, s.rows, s.cols);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // namespace

extern "C" {

int go2sim_distill_act(go2sim_mlp_t* student, go2sim_mlp_t* teacher, const float* obs, const float* teacher_obs, const float* std_dev, int n_rows, uint64_t seed,
                       uint32_t step, int deterministic, float* actions, float* mean, float* teacher_actions, void* stream) {
  if (!student || !teacher || !obs || !teacher_obs || !std_dev || !actions || !mean || !teacher_actions || n_rows < 0) return GO2SIM_E_BADARG;
  const int A = student->dims[student->n_layers];
  if (teacher->dims[teacher->n_layers] != A || teacher->device != student->device) return GO2SIM_E_BADARG;
  if (n_rows == 0) return GO2SIM_E_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mlp_forward, dim3((n_rows + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, student->dev, obs, mean, teacher->dev, teacher_obs, teacher_actions, n_rows);
  hipLaunchKernelGGL(k_policy_sample, dim3((n_rows + 63) / 64), dim3(64), 0, st, mean, std_dev, n_rows, A, seed, step, deterministic, actions, (float*)nullptr);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_distill_create(go2sim_mlp_t* student, int n_actions, const go2sim_distill_cfg_t* cfg, int max_window_rows, go2sim_distill_t** out) {
  if (!student || !cfg || !out || max_window_rows < 1 || n_actions < 1 || student->dims[student->n_layers] != n_actions) return GO2SIM_E_BADARG;
  if (!(cfg->learning_rate > 0.0) || (cfg->loss_type != GO2SIM_DISTILL_MSE && cfg->loss_type != GO2SIM_DISTILL_HUBER)) return GO2SIM_E_BADARG;
  if (cfg->sub_rows < 0 || cfg->sub_rows % RCH || std::isnan(cfg->max_grad_norm)) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(student->device));
  go2sim_distill* h = new (std::nothrow) go2sim_distill();
  if (!h) return GO2SIM_E_NOMEM;
  const go2sim_mlp* M = student;
  h->student = student; h->cfg = *cfg; h->A = n_actions; h->Apad = round16(n_actions); h->max_rows = max_window_rows;
  h->sub = cfg->sub_rows ? cfg->sub_rows : GO2SIM_DISTILL_SUB_ROWS;
  h->ws_rows = max_window_rows < h->sub ? max_window_rows : h->sub;
  h->nP = M->padded;
  size_t flat = 0;
  for (int l = 0; l < M->n_layers; ++l) {
    h->segs.push_back(DSeg{(size_t)(M->dev.W[l] - M->dparams), M->dev.kpad[l], M->dims[l + 1], M->dims[l], flat}); flat += (size_t)M->dims[l] * M->dims[l + 1];
    h->segs.push_back(DSeg{(size_t)(M->dev.b[l] - M->dparams), M->dims[l + 1], 1, M->dims[l + 1], flat}); flat += M->dims[l + 1];
  }
  h->n_flat = flat;
  auto al16 = [](size_t n) { return (n + 15) / 16 * 16; };   // every region starts 64-byte aligned (float4 loads)
  const size_t R = (size_t)h->ws_rows;
  int wmax = 16;
  size_t need = al16(R * h->A);
  for (int l = 0; l < M->n_layers; ++l) { if (l < M->n_layers - 1) need += R * M->dev.npad[l]; if (M->dev.npad[l] > wmax) wmax = M->dev.npad[l]; }
  const size_t dz_sz = R * wmax;
  const int chunks = (int)((R + RCH - 1) / RCH);
  need += 2 * dz_sz + (size_t)chunks * h->nP;
  h->max_head_wg = (max_window_rows + WGT - 1) / WGT;
  const size_t nd = S_N + NORM_WG + h->nP + (size_t)h->max_head_wg;
  if (hipMalloc((void**)&h->fbuf, 3 * h->nP * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->wbuf, need * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&h->dbuf, nd * sizeof(double)) != hipSuccess) {
    go2sim_distill_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  if (hipMemset(h->fbuf, 0, 3 * h->nP * sizeof(float)) != hipSuccess || hipMemset(h->wbuf, 0, need * sizeof(float)) != hipSuccess ||
      hipMemset(h->dbuf, 0, nd * sizeof(double)) != hipSuccess || hipMemcpy(h->dbuf + S_LR, &cfg->learning_rate, sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    fprintf(stderr, "go2sim_distill: initialising the trainer failed: %s\n", hipGetErrorString(hipGetLastError()));
    go2sim_distill_destroy(h);
    return GO2SIM_E_HIP;
  }
  h->grads = h->fbuf; h->m = h->grads + h->nP; h->v = h->m + h->nP;
  h->scal = h->dbuf; h->sq_part = h->scal + S_N; h->acc = h->sq_part + NORM_WG; h->head_part = h->acc + h->nP;
  float* p = h->wbuf;
  h->mu = p; p += al16(R * h->A);
  for (int l = 0; l < M->n_layers - 1; ++l) { h->ws.a[l] = p; p += R * M->dev.npad[l]; }
  h->dz[0] = p; p += dz_sz; h->dz[1] = p; p += dz_sz;
  h->partial = p;
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_distill_destroy(go2sim_distill_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  if (h->fbuf) (void)hipFree(h->fbuf);
  if (h->wbuf) (void)hipFree(h->wbuf);
  if (h->dbuf) (void)hipFree(h->dbuf);
  if (h->rows) (void)hipFree(h->rows);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_distill_window_grad(go2sim_distill_t* h, const float* obs, const float* teacher_actions, const int32_t* idx, int n_rows, int n_envs, void* stream) {
  if (!window_ok(h, obs, teacher_actions, idx, n_rows, n_envs)) return GO2SIM_E_BADARG;
  return launch_window(h, obs, teacher_actions, idx, n_rows, n_envs, true, (hipStream_t)stream);
}

int go2sim_distill_loss_only(go2sim_distill_t* h, const float* obs, const float* teacher_actions, const int32_t* idx, int n_rows, int n_envs, void* stream) {
  if (!window_ok(h, obs, teacher_actions, idx, n_rows, n_envs)) return GO2SIM_E_BADARG;
  return launch_window(h, obs, teacher_actions, idx, n_rows, n_envs, false, (hipStream_t)stream);
}

int go2sim_distill_apply(go2sim_distill_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const double t = (double)(h->step + 1);                  // the handle's count moves once the launches are accepted
  AdamArgs a{};
  a.p_actor = h->student->dparams; a.g = h->grads; a.m = h->m; a.v = h->v;
  a.nA = h->nP; a.nC = 0; a.n_tot = h->nP; a.A = 0; a.sq_part = h->sq_part; a.scal = h->scal;
  a.max_norm = h->cfg.max_grad_norm > 0.0 ? h->cfg.max_grad_norm : std::numeric_limits<double>::infinity();   // no clip: the coefficient is min(1, inf) = 1, exact
  a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.eps;
  a.bc1 = 1.0 - std::pow(h->cfg.beta1, t); a.bc2_sqrt = std::sqrt(1.0 - std::pow(h->cfg.beta2, t));
  hipLaunchKernelGGL(k_sumsq, dim3(NORM_WG), dim3(WGT), 0, st, h->grads, h->nP, h->sq_part);
  hipLaunchKernelGGL(k_adam<false>, dim3((unsigned)((h->nP + WGT - 1) / WGT)), dim3(WGT), 0, st, a);
  HIPCHK(hipGetLastError());
  h->step += 1; h->windows += 1;
  return GO2SIM_E_OK;
}

int go2sim_distill_update(go2sim_distill_t* h, const float* obs, const float* teacher_actions, int T, int N, int E, int G, void* stream) {
  if (!h || !obs || !teacher_actions || T < 1 || N < 1 || E < 1 || G < 1) return GO2SIM_E_BADARG;
  const long long total = (long long)E * T * N;
  if ((long long)G * N > h->max_rows || total > 0x7fffffffLL || (long long)T * N > 0x7fffffffLL / MAXW) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (!h->rows || h->rows_T != T || h->rows_N != N || h->rows_E != E) {        // once per shape
    if (h->rows) { (void)hipFree(h->rows); h->rows = nullptr; }
    if (hipMalloc((void**)&h->rows, (size_t)total * sizeof(int32_t)) != hipSuccess) return GO2SIM_E_NOMEM;
    hipLaunchKernelGGL(k_distill_rows, dim3((unsigned)((total + WGT - 1) / WGT)), dim3(WGT), 0, st, h->rows, total, T, N);
    HIPCHK(hipGetLastError());
    h->rows_T = T; h->rows_N = N; h->rows_E = E;
  }
  int rc = go2sim_distill_reset_stats(h, stream);
  const int pairs = E * T, n_win = pairs / G, tail = pairs - n_win * G;
  for (int w = 0; w < n_win && rc == GO2SIM_E_OK; ++w) {
    rc = launch_window(h, obs, teacher_actions, h->rows + (size_t)w * G * N, G * N, N, true, st);
    if (rc == GO2SIM_E_OK) rc = go2sim_distill_apply(h, stream);
  }
  if (rc == GO2SIM_E_OK && tail > 0) rc = launch_window(h, obs, teacher_actions, h->rows + (size_t)n_win * G * N, tail * N, N, false, st);
  return rc;
}

int go2sim_distill_n_params(go2sim_distill_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->n_flat;
  return GO2SIM_E_OK;
}
int go2sim_distill_export(go2sim_distill_t* h, int which, float* flat_dev, void* stream) { return pack_all(h, which, 0, flat_dev, (hipStream_t)stream); }
int go2sim_distill_import(go2sim_distill_t* h, int which, const float* flat_dev, void* stream) {
  return pack_all(h, which, 1, const_cast<float*>(flat_dev), (hipStream_t)stream);
}
int go2sim_distill_n_padded(go2sim_distill_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->nP;
  return GO2SIM_E_OK;
}
int go2sim_distill_export_padded(go2sim_distill_t* h, int which, float* padded_dev, void* stream) {
  if (!h || !padded_dev || !vec_of(h, which)) return GO2SIM_E_BADARG;
  HIPCHK(hipMemcpyAsync(padded_dev, vec_of(h, which), h->nP * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GO2SIM_E_OK;
}

int go2sim_distill_set_step(go2sim_distill_t* h, long long step, double learning_rate, void* stream) {
  if (!h || step < 0 || !(learning_rate > 0.0)) return GO2SIM_E_BADARG;
  h->step = step;
  hipLaunchKernelGGL(k_set_lr, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal, learning_rate);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
int go2sim_distill_reset_stats(go2sim_distill_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_reset, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal);
  HIPCHK(hipGetLastError());
  h->pairs = 0; h->windows = 0;
  return GO2SIM_E_OK;
}
int go2sim_distill_stats(go2sim_distill_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal, (double)h->step, (double)h->pairs, (double)h->windows, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
