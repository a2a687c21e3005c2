// go2sim_distill.hip -- teacher-student distillation (include/go2sim_distill.h): the collection step that runs student and teacher in one launch and the
// behaviour-cloning update of the student.  gfx950 only.
//
// The collection step is the policy step's two kernels (go2sim_mlp_dev.h): k_mlp_forward with the teacher where the critic sits, k_policy_sample on the
// student's mean.  A window of the update is walked in sub-batches of sub_rows rows; one sub-batch is, on the caller's stream and without atomics,
//   k_train_forward     (go2sim_train_dev.h) the student's forward with the hidden activations kept, rows read through the window's index list
//   k_distill_head      (go2sim_distill_dev.h, shared with the recurrent student's update) one row per lane: residual, rho into a float64 per-workgroup partial, rho' / (N A) into dZ [rows][Apad] with zero padding
//   per layer, last to first: k_bwd_dw, k_bwd_db, k_bwd_da   (launch_backward of go2sim_trainer_host.h, one network per launch)
//   k_reduce_partials   (one sub-batch) or k_distill_accumulate (several): the chunk slabs added in chunk order in float64; the second keeps the float64 sum
//                       across sub-batches and rounds after the last one, which is the same sequence of additions as one pass over all chunks
// and after the last sub-batch k_distill_finalize adds the head's partials of the whole window in workgroup order.  The optimizer is k_sumsq + k_adam of
// the PPO update over the student's padded parameters alone (no critic, no std block).  The host code that drives all of this but the head -- the
// optimizer state and its step, the packing, the workspace carving, the backward schedule -- is the PPO update's too (go2sim_trainer_host.h); the float64
// sum across sub-batches and the head's partials sit in the optimizer state's tail.
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
#include "go2sim_distill_dev.h"   // the head, the float64 sum across sub-batches and the statistics: shared with go2sim_rdistill.hip
#define GO2SIM_HIPCHK_TAG "go2sim_distill"
#include "go2sim_trainer_host.h"
#include "../../include/go2sim_distill.h"

static_assert((int)GO2SIM_DISTILL_GRADS == (int)GO2SIM_PPO_GRADS && (int)GO2SIM_DISTILL_ADAM_M == (int)GO2SIM_PPO_ADAM_M && (int)GO2SIM_DISTILL_ADAM_V == (int)GO2SIM_PPO_ADAM_V,
              "opt_vec serves both enums");

namespace {

// the row-index list of one update: entry cnt N + j is row (cnt % T) N + j, cnt over the E T pairs in the order the windows take them
__global__ __launch_bounds__(WGT) void k_distill_rows(int32_t* __restrict__ idx, long long total, int T, int N) {
  const long long i = (long long)blockIdx.x * WGT + threadIdx.x;
  if (i >= total) return;
  const long long cnt = i / N;
  idx[i] = (int32_t)((cnt % T) * N + (i - cnt * N));
}

}  // namespace

struct go2sim_distill {
  go2sim_mlp* student = nullptr;
  go2sim_distill_cfg_t cfg{};
  int A = 0, Apad = 0, max_rows = 0, sub = 0, ws_rows = 0;
  size_t nP = 0, n_flat = 0;   // padded / flat size of the student's parameters
  OptState opt;               // over nP floats; its tail: acc[nP] | head partials
  float* wbuf = nullptr;      // mu | activations | dz ping-pong | partial slabs, for ws_rows rows
  float *mu = nullptr, *partial = nullptr;
  NetWs nw{};
  double *acc = nullptr, *head_part = nullptr;
  int max_head_wg = 0;
  long long pairs = 0, windows = 0;
  int32_t* rows = nullptr;    // the row-index list of go2sim_distill_update, for (rows_T, rows_N, rows_E)
  int rows_T = 0, rows_N = 0, rows_E = 0;
  std::vector<Seg> segs;
};

namespace {

float* vec_of(go2sim_distill* h, int which) { return which == GO2SIM_DISTILL_PARAMS ? h->student->dparams : opt_vec(h->opt, which); }

// forward and head of rows idx[0 .. n), with `backward` the gradient as well; the running loss sum moves by the rows' sum of rho / (N A)
int launch_window(go2sim_distill* h, const float* obs, const float* teacher, const int32_t* idx, int n, int n_envs, bool backward, hipStream_t st) {
  const go2sim_mlp* M = h->student;
  const double w = 1.0 / ((double)n_envs * (double)h->A);
  const int nsub = (n + h->sub - 1) / h->sub;
  const size_t slab = h->nP;
  for (int s = 0; s < nsub; ++s) {
    const int off = s * h->sub, m = n - off < h->sub ? n - off : h->sub;
    const int32_t* ix = idx + off;
    hipLaunchKernelGGL(k_train_forward<false>, dim3((m + TM - 1) / TM, 1), dim3(64 * NWAVE), 0, st, M->dev, obs, h->mu, h->nw.a, M->dev, obs, h->mu, h->nw.a, ix, m, m,
                       MirTab{nullptr, nullptr}, MirTab{nullptr, nullptr});
    DistillHeadArgs ha{};
    ha.mu = h->mu; ha.teacher = teacher; ha.idx = ix; ha.dz = h->nw.dz[(M->n_layers - 1) & 1]; ha.part = h->head_part + off / WGT;
    ha.n = m; ha.A = h->A; ha.Apad = h->Apad; ha.huber = h->cfg.loss_type == GO2SIM_DISTILL_HUBER; ha.w = w;
    hipLaunchKernelGGL(k_distill_head, dim3((m + WGT - 1) / WGT), dim3(WGT), 0, st, ha);
    if (!backward) continue;
    const int n_chunks = (m + RCH - 1) / RCH;
    BwdLayer L[MAXL][2] = {};                              // the second network's slot of the shared kernels stays empty
    for (int lb = 0; lb < M->n_layers; ++lb) L[lb][0] = bwd_layer(M, h->nw, lb, obs, 1, MirTab{nullptr, nullptr}, 0);
    launch_backward<false, false>(L, M->n_layers, BwdRun{1, ix, m, m, h->partial, slab, st});
    const dim3 grid((unsigned)((slab + WGT - 1) / WGT));
    if (nsub == 1) hipLaunchKernelGGL(k_reduce_partials, grid, dim3(WGT), 0, st, h->partial, n_chunks, slab, h->opt.grads);
    else hipLaunchKernelGGL(k_distill_accumulate, grid, dim3(WGT), 0, st, h->partial, n_chunks, slab, h->acc, s == 0 ? 1 : 0, s == nsub - 1 ? 1 : 0, h->opt.grads);
  }
  hipLaunchKernelGGL(k_distill_finalize, dim3(1), dim3(1), 0, st, h->head_part, (n + WGT - 1) / WGT, w, h->opt.scal);
  HIPCHK(hipGetLastError());
  h->pairs += n / n_envs;
  return GO2SIM_E_OK;
}

bool window_ok(const go2sim_distill* h, const float* obs, const float* teacher, const int32_t* idx, int n_rows, int n_envs) {
  return h && obs && teacher && idx && n_envs >= 1 && n_rows >= 1 && n_rows <= h->max_rows && n_rows % n_envs == 0;
}

int pack_all(go2sim_distill* h, int which, int to_padded, float* flat, hipStream_t st) {
  if (!h || !flat || !vec_of(h, which)) return GO2SIM_E_BADARG;
  float* base[1] = {vec_of(h, which)};
  return pack_segs(h->segs, base, to_padded, flat, st);
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
  mlp_segs(h->segs, 0, M, h->n_flat);
  const size_t R = (size_t)h->ws_rows;
  const int chunks = (int)((R + RCH - 1) / RCH);
  const size_t need = al16(R * h->A) + net_ws_floats(M, R) + (size_t)chunks * h->nP;
  h->max_head_wg = (max_window_rows + WGT - 1) / WGT;
  if (!opt_alloc(h->opt, h->nP, h->nP + (size_t)h->max_head_wg) || hipMalloc((void**)&h->wbuf, need * sizeof(float)) != hipSuccess) {
    go2sim_distill_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  if (!opt_zero(h->opt, cfg->learning_rate, h->wbuf, need)) {
    fprintf(stderr, "go2sim_distill: initialising the trainer failed: %s\n", hipGetErrorString(hipGetLastError()));
    go2sim_distill_destroy(h);
    return GO2SIM_E_HIP;
  }
  h->acc = h->opt.tail; h->head_part = h->acc + h->nP;
  h->mu = h->wbuf;
  h->partial = net_ws_carve(M, R, h->mu + al16(R * h->A), h->nw);
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_distill_destroy(go2sim_distill_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  opt_free(h->opt);
  if (h->wbuf) (void)hipFree(h->wbuf);
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
  AdamArgs a{};
  a.p_actor = h->student->dparams; a.nA = h->nP;
  a.max_norm = h->cfg.max_grad_norm > 0.0 ? h->cfg.max_grad_norm : std::numeric_limits<double>::infinity();   // no clip: the coefficient is min(1, inf) = 1, exact
  a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.eps;
  const int rc = opt_apply<false>(h->opt, a, (hipStream_t)stream);
  if (rc == GO2SIM_E_OK) h->windows += 1;
  return rc;
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
  if (!h) return GO2SIM_E_BADARG;
  return opt_export_padded(h->opt, vec_of(h, which), padded_dev, (hipStream_t)stream);
}

int go2sim_distill_set_step(go2sim_distill_t* h, long long step, double learning_rate, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  return opt_set_step(h->opt, step, learning_rate, (hipStream_t)stream);
}
int go2sim_distill_reset_stats(go2sim_distill_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_reset, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal);
  HIPCHK(hipGetLastError());
  h->pairs = 0; h->windows = 0;
  return GO2SIM_E_OK;
}
int go2sim_distill_stats(go2sim_distill_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal, (double)h->opt.step, (double)h->pairs, (double)h->windows, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
