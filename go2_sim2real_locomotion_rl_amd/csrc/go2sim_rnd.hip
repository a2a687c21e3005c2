// go2sim_rnd.hip -- random network distillation (include/go2sim_rnd.h): the per-env-step intrinsic reward and the update of the predictor.  gfx950 only.
// The header states the law; this file follows its names.
//
// The step is two launches on the caller's stream:
//   k_mlp_forward   (go2sim_mlp_dev.h) target and predictor side by side, the target where the actor sits
//   k_rnd_reward    one row per lane, one workgroup per chunk of GO2SIM_NORM_ROW_CHUNK rows: the embedding distance r in float64, avg, the chunk's float64
//                   moments of avg in row order; the workgroup that draws the last ticket folds the chunks (fold_chunks, norm_law of go2sim_norm_dev.h: the
//                   observation normaliser's own code on one column), stores the state and writes intrinsic and rewards_total of every row
// A mini-batch of the update is, without atomics,
//   k_train_forward     (go2sim_train_dev.h) predictor AND target in one launch, rows read through the index list; the predictor's hidden activations are
//                       kept for the backward pass.  The target runs the same layer loop as k_mlp_forward (mlp_layer), so its embedding has go2sim_mlp_forward's
//                       bits; that its activations are stored too is the price of not gathering the rows a second time.
//   k_distill_head      (go2sim_distill_dev.h) the MSE head with weight 1 / (n_rows E) on the two embeddings, row for row (an identity index list)
//   k_bwd_dw, k_bwd_db, k_bwd_da per layer (launch_backward), k_reduce_partials, k_distill_finalize (the head's partials in workgroup order)
// and the optimizer is k_sumsq + k_adam over the predictor's padded parameters with the clip coefficient min(1, inf) = 1.
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
#include "go2sim_distill_dev.h"   // the MSE head, its finalize, the running loss and the statistics block
#include "go2sim_norm_dev.h"      // fold_chunks, norm_law: the reward normaliser is the observation normaliser's law on one column
#define GO2SIM_HIPCHK_TAG "go2sim_rnd"
#include "go2sim_trainer_host.h"
#include "../../include/go2sim_rnd.h"

static_assert((int)GO2SIM_RND_GRADS == (int)GO2SIM_PPO_GRADS && (int)GO2SIM_RND_ADAM_M == (int)GO2SIM_PPO_ADAM_M && (int)GO2SIM_RND_ADAM_V == (int)GO2SIM_PPO_ADAM_V,
              "opt_vec serves both enums");
static_assert((int)GO2SIM_RND_ST_LOSS == (int)GO2SIM_DISTILL_ST_LOSS && (int)GO2SIM_RND_ST_LR == (int)GO2SIM_DISTILL_ST_LR &&
              (int)GO2SIM_RND_ST_GRAD_NORM == (int)GO2SIM_DISTILL_ST_GRAD_NORM && (int)GO2SIM_RND_ST_STEP == (int)GO2SIM_DISTILL_ST_STEP &&
              (int)GO2SIM_RND_ST_MINIBATCHES == (int)GO2SIM_DISTILL_ST_PAIRS && (int)GO2SIM_RND_ST_APPLIES == (int)GO2SIM_DISTILL_ST_WINDOWS &&
              GO2SIM_RND_N_STATS == GO2SIM_DISTILL_N_STATS, "k_distill_stats writes this header's block");
static_assert(CH == WGT, "k_rnd_reward: one lane per row of a chunk");

namespace {

constexpr float RND_GAMMA = 0.99f;
constexpr double RND_UNTIL = 1.0e8;

// the reward normaliser's state on the device
struct RndState {
  long long count;
  unsigned ticket, pad;
  float mean, var, sd, pad2;
};

struct RndStepArgs {
  const float *t, *p;          // [n][E]: the embeddings of this step
  const float* rewards;        // [n]
  float *r, *avg;              // [n]: the distance before the normaliser, the discounted sum
  float *intrinsic, *total;    // [n]
  double* part;                // [chunks][2]: the chunk's mean of avg, then its centred squares
  RndState* st;
  int n, E, norm;
  float w;
};

__device__ __forceinline__ void rnd_write(const RndStepArgs& a, int i, float r) {
  const float b = a.w * r;
  a.intrinsic[i] = b;
  a.total[i] = a.rewards[i] + b;
}

__global__ __launch_bounds__(CH) void k_rnd_reward(RndStepArgs a) {
  __shared__ double red[CH];
  __shared__ double s_mu;
  __shared__ float s_sd;
  __shared__ int s_last;
  const int t = threadIdx.x, i = blockIdx.x * CH + t;
  const bool on = i < a.n;
  float r = 0.0f;
  if (on) {
    double s = 0.0;
    for (int e = 0; e < a.E; ++e) {
      const double d = (double)a.t[(size_t)i * a.E + e] - (double)a.p[(size_t)i * a.E + e];
      s += d * d;
    }
    r = (float)sqrt(s);
    a.r[i] = r;
  }
  if (!a.norm) {
    if (on) rnd_write(a, i, r);
    return;
  }
  float av = 0.0f;
  if (on) {
    av = RND_GAMMA * a.avg[i] + r;
    a.avg[i] = av;
  }
  // the chunk's moments as k_norm_moments forms them for a column: the rows in row order, the mean first, then the squares centred on it
  const int rows = chunk_rows(blockIdx.x, a.n);
  red[t] = on ? (double)av : 0.0;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < rows; ++k) s += red[k];
    s_mu = s / (double)rows;
  }
  __syncthreads();
  const double e = (double)av - s_mu;
  red[t] = on ? e * e : 0.0;
  __syncthreads();
  if (t == 0) {
    double q = 0.0;
    for (int k = 0; k < rows; ++k) q += red[k];
    a.part[2 * blockIdx.x] = s_mu;
    a.part[2 * blockIdx.x + 1] = q;
  }
  // the last workgroup to arrive folds: every lane's stores (r, avg, part) are released before the ticket is drawn, and acquired behind it
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = __hip_atomic_fetch_add(&a.st->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (t == 0) {
    const long long cnt = a.st->count;
    float sd = a.st->sd;
    if ((double)cnt < RND_UNTIL) {
      const Mom b = fold_chunks(a.part, 1, 0, a.n);
      double m1, v1;
      norm_law((double)a.st->mean, (double)a.st->var, cnt, b, m1, v1);
      sd = (float)sqrt(v1);
      a.st->mean = (float)m1; a.st->var = (float)v1; a.st->sd = sd;
      a.st->count = cnt + (long long)b.n;
    }
    s_sd = sd;
    __hip_atomic_store(&a.st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next step's launch starts from zero
  }
  __syncthreads();
  const float sd = s_sd;
  for (int k = t; k < a.n; k += CH) {
    const float rk = a.r[k];
    rnd_write(a, k, sd > 0.0f ? rk / sd : rk);
  }
}

__global__ __launch_bounds__(WGT) void k_rnd_iota(int32_t* __restrict__ idx, int n) {
  const int i = blockIdx.x * WGT + threadIdx.x;
  if (i < n) idx[i] = i;
}

}  // namespace

struct go2sim_rnd {
  go2sim_mlp *pred = nullptr, *target = nullptr;
  go2sim_rnd_cfg_t cfg{};
  int E = 0, Epad = 0, D = 0, max_rows = 0;
  size_t nP = 0, n_flat = 0;  // padded / flat size of the predictor's parameters
  OptState opt;               // over nP floats; its tail: head partials | chunk moments of avg
  float* wbuf = nullptr;      // mu | tg | r | avg | predictor's activations and dz | target's activations | partial slabs, for max_rows rows
  float *mu = nullptr, *tg = nullptr, *r = nullptr, *avg = nullptr, *partial = nullptr;
  NetWs nw{};
  ActWs tw{};
  double *head_part = nullptr, *mom_part = nullptr;
  int32_t* iota = nullptr;
  RndState* st = nullptr;
  long long minibatches = 0, applies = 0;
  int last_rows = 0;
  std::vector<Seg> segs;
};

namespace {

float* vec_of(go2sim_rnd* h, int which) { return which == GO2SIM_RND_PARAMS ? h->pred->dparams : opt_vec(h->opt, which); }

int pack_all(go2sim_rnd* h, int which, int to_padded, float* flat, hipStream_t st) {
  if (!h || !flat || !vec_of(h, which)) return GO2SIM_E_BADARG;
  float* base[1] = {vec_of(h, which)};
  return pack_segs(h->segs, base, to_padded, flat, st);
}

int set_state_host(go2sim_rnd* h, float mean, float var, float sd, long long count, hipStream_t s) {
  RndState v{};
  v.count = count; v.ticket = 0; v.mean = mean; v.var = var; v.sd = sd;
  HIPCHK(hipMemcpyAsync(h->st, &v, sizeof(v), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return GO2SIM_E_OK;
}

}  // namespace

extern "C" {

int go2sim_rnd_create(go2sim_mlp_t* predictor, go2sim_mlp_t* target, const go2sim_rnd_cfg_t* cfg, int max_rows, go2sim_rnd_t** out) {
  if (!predictor || !target || !cfg || !out || max_rows < 1 || predictor == target) return GO2SIM_E_BADARG;
  const int E = predictor->dims[predictor->n_layers];
  if (target->dims[target->n_layers] != E || target->dims[0] != predictor->dims[0] || target->device != predictor->device) return GO2SIM_E_BADARG;
  if (!(cfg->learning_rate > 0.0) || (long long)max_rows > 0x7fffffffLL / MAXW) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(predictor->device));
  go2sim_rnd* h = new (std::nothrow) go2sim_rnd();
  if (!h) return GO2SIM_E_NOMEM;
  const go2sim_mlp *P = predictor, *T = target;
  h->pred = predictor; h->target = target; h->cfg = *cfg; h->E = E; h->Epad = round16(E); h->D = P->dims[0]; h->max_rows = max_rows;
  h->nP = P->padded;
  mlp_segs(h->segs, 0, P, h->n_flat);
  const size_t R = (size_t)max_rows;
  const int chunks = (int)((R + RCH - 1) / RCH), head_wg = (int)((R + WGT - 1) / WGT), mom_chunks = (int)((R + CH - 1) / CH);
  size_t t_act = 0;
  for (int l = 0; l < T->n_layers - 1; ++l) t_act += R * T->dev.npad[l];
  const size_t need = 2 * al16(R * E) + 2 * al16(R) + net_ws_floats(P, R) + t_act + (size_t)chunks * h->nP;
  if (!opt_alloc(h->opt, h->nP, (size_t)head_wg + 2 * (size_t)mom_chunks) || hipMalloc((void**)&h->wbuf, need * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&h->iota, R * sizeof(int32_t)) != hipSuccess || hipMalloc((void**)&h->st, sizeof(RndState)) != hipSuccess) {
    go2sim_rnd_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  hipLaunchKernelGGL(k_rnd_iota, dim3((unsigned)((R + WGT - 1) / WGT)), dim3(WGT), 0, 0, h->iota, max_rows);
  if (!opt_zero(h->opt, cfg->learning_rate, h->wbuf, need) || set_state_host(h, 0.0f, 1.0f, 1.0f, 0, nullptr) != GO2SIM_E_OK) {
    fprintf(stderr, "go2sim_rnd: initialising the trainer failed: %s\n", hipGetErrorString(hipGetLastError()));
    go2sim_rnd_destroy(h);
    return GO2SIM_E_HIP;
  }
  h->head_part = h->opt.tail; h->mom_part = h->head_part + head_wg;
  float* p = h->wbuf;
  h->mu = p; p += al16(R * E);
  h->tg = p; p += al16(R * E);
  h->r = p; p += al16(R);
  h->avg = p; p += al16(R);
  p = net_ws_carve(P, R, p, h->nw);
  for (int l = 0; l < T->n_layers - 1; ++l) { h->tw.a[l] = p; p += R * T->dev.npad[l]; }
  h->partial = p;
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_rnd_destroy(go2sim_rnd_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  opt_free(h->opt);
  if (h->wbuf) (void)hipFree(h->wbuf);
  if (h->iota) (void)hipFree(h->iota);
  if (h->st) (void)hipFree(h->st);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_rnd_step(go2sim_rnd_t* h, const float* s, const float* rewards, int n_rows, double weight, float* intrinsic, float* rewards_total, void* stream) {
  if (!h || !s || !rewards || !intrinsic || !rewards_total || n_rows < 0 || n_rows > h->max_rows) return GO2SIM_E_BADARG;
  if (n_rows == 0) return GO2SIM_E_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mlp_forward, dim3((n_rows + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, h->target->dev, s, h->tg, h->pred->dev, s, h->mu, n_rows);
  RndStepArgs a{};
  a.t = h->tg; a.p = h->mu; a.rewards = rewards; a.r = h->r; a.avg = h->avg; a.intrinsic = intrinsic; a.total = rewards_total; a.part = h->mom_part; a.st = h->st;
  a.n = n_rows; a.E = h->E; a.norm = h->cfg.reward_normalization ? 1 : 0; a.w = (float)weight;
  hipLaunchKernelGGL(k_rnd_reward, dim3((n_rows + CH - 1) / CH), dim3(CH), 0, st, a);
  HIPCHK(hipGetLastError());
  h->last_rows = n_rows;
  return GO2SIM_E_OK;
}

int go2sim_rnd_last_step(go2sim_rnd_t* h, float* target_emb, float* predictor_emb, float* r, int n_rows, void* stream) {
  if (!h || !target_emb || !predictor_emb || !r || n_rows < 0 || n_rows > h->last_rows) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) return GO2SIM_E_OK;
  HIPCHK(hipMemcpyAsync(target_emb, h->tg, (size_t)n_rows * h->E * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(predictor_emb, h->mu, (size_t)n_rows * h->E * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(r, h->r, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToDevice, st));
  return GO2SIM_E_OK;
}

int go2sim_rnd_minibatch_grad(go2sim_rnd_t* h, const float* s, const int32_t* idx, int n, void* stream) {
  if (!h || !s || !idx || n < 1 || n > h->max_rows) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const go2sim_mlp *P = h->pred, *T = h->target;
  h->last_rows = 0;                                       // the embeddings of the last step are overwritten
  hipLaunchKernelGGL(k_train_forward<false>, dim3((n + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, P->dev, s, h->mu, h->nw.a, T->dev, s, h->tg, h->tw, idx, n, n,
                     MirTab{nullptr, nullptr}, MirTab{nullptr, nullptr});
  const double w = 1.0 / ((double)n * (double)h->E);
  DistillHeadArgs ha{};
  ha.mu = h->mu; ha.teacher = h->tg; ha.idx = h->iota; ha.dz = h->nw.dz[(P->n_layers - 1) & 1]; ha.part = h->head_part;
  ha.n = n; ha.A = h->E; ha.Apad = h->Epad; ha.huber = 0; ha.w = w;
  const int head_wg = (n + WGT - 1) / WGT;
  hipLaunchKernelGGL(k_distill_head, dim3(head_wg), dim3(WGT), 0, st, ha);
  const int n_chunks = (n + RCH - 1) / RCH;
  const size_t slab = h->nP;
  BwdLayer L[MAXL][2] = {};                               // the second network's slot of the shared kernels stays empty
  for (int lb = 0; lb < P->n_layers; ++lb) L[lb][0] = bwd_layer(P, h->nw, lb, s, 1, MirTab{nullptr, nullptr}, 0);
  launch_backward<false, false>(L, P->n_layers, BwdRun{1, idx, n, n, h->partial, slab, st});
  hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)((slab + WGT - 1) / WGT)), dim3(WGT), 0, st, h->partial, n_chunks, slab, h->opt.grads);
  hipLaunchKernelGGL(k_distill_finalize, dim3(1), dim3(1), 0, st, h->head_part, head_wg, w, h->opt.scal);
  HIPCHK(hipGetLastError());
  h->minibatches += 1;
  return GO2SIM_E_OK;
}

int go2sim_rnd_apply(go2sim_rnd_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  AdamArgs a{};
  a.p_actor = h->pred->dparams; a.nA = h->nP;
  a.max_norm = std::numeric_limits<double>::infinity();   // no clip: the coefficient is min(1, inf) = 1, exact
  a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.eps;
  const int rc = opt_apply<false>(h->opt, a, (hipStream_t)stream);
  if (rc == GO2SIM_E_OK) h->applies += 1;
  return rc;
}

int go2sim_rnd_update(go2sim_rnd_t* h, const float* s, const int32_t* idx, int n_rows_total, int n_epochs, int n_mini_batches, void* stream) {
  if (!h || !s || !idx || n_rows_total < 1 || n_epochs < 1 || n_mini_batches < 1) return GO2SIM_E_BADARG;
  const int mbs = n_rows_total / n_mini_batches;
  if (mbs < 1 || mbs > h->max_rows) return GO2SIM_E_BADARG;
  int rc = go2sim_rnd_reset_stats(h, stream);
  for (int e = 0; e < n_epochs && rc == GO2SIM_E_OK; ++e)
    for (int i = 0; i < n_mini_batches && rc == GO2SIM_E_OK; ++i) {
      rc = go2sim_rnd_minibatch_grad(h, s, idx + (size_t)i * mbs, mbs, stream);
      if (rc == GO2SIM_E_OK) rc = go2sim_rnd_apply(h, stream);
    }
  return rc;
}

int go2sim_rnd_n_params(go2sim_rnd_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->n_flat;
  return GO2SIM_E_OK;
}
int go2sim_rnd_export(go2sim_rnd_t* h, int which, float* flat_dev, void* stream) { return pack_all(h, which, 0, flat_dev, (hipStream_t)stream); }
int go2sim_rnd_import(go2sim_rnd_t* h, int which, const float* flat_dev, void* stream) {
  return pack_all(h, which, 1, const_cast<float*>(flat_dev), (hipStream_t)stream);
}
int go2sim_rnd_n_padded(go2sim_rnd_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->nP;
  return GO2SIM_E_OK;
}
int go2sim_rnd_export_padded(go2sim_rnd_t* h, int which, float* padded_dev, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  return opt_export_padded(h->opt, vec_of(h, which), padded_dev, (hipStream_t)stream);
}

int go2sim_rnd_set_step(go2sim_rnd_t* h, long long step, double learning_rate, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  return opt_set_step(h->opt, step, learning_rate, (hipStream_t)stream);
}
int go2sim_rnd_reset_stats(go2sim_rnd_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_reset, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal);
  HIPCHK(hipGetLastError());
  h->minibatches = 0; h->applies = 0;
  return GO2SIM_E_OK;
}
int go2sim_rnd_stats(go2sim_rnd_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_distill_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal, (double)h->opt.step, (double)h->minibatches, (double)h->applies, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_rnd_get_reward_state(go2sim_rnd_t* h, float* mean, float* var, float* std, int64_t* count, float* avg, int n_avg, void* stream) {
  if (!h || !mean || !var || !std || !count || n_avg < 0 || n_avg > h->max_rows || (n_avg > 0 && !avg)) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  RndState v{};
  HIPCHK(hipMemcpyAsync(&v, h->st, sizeof(v), hipMemcpyDeviceToHost, s));
  if (n_avg > 0) HIPCHK(hipMemcpyAsync(avg, h->avg, (size_t)n_avg * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *mean = v.mean; *var = v.var; *std = v.sd; *count = (int64_t)v.count;
  return GO2SIM_E_OK;
}

int go2sim_rnd_set_reward_state(go2sim_rnd_t* h, float mean, float var, float std, int64_t count, const float* avg, int n_avg, void* stream) {
  if (!h || count < 0 || n_avg < 0 || n_avg > h->max_rows || (n_avg > 0 && !avg)) return GO2SIM_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(h->avg, 0, (size_t)h->max_rows * sizeof(float), s));
  if (n_avg > 0) HIPCHK(hipMemcpyAsync(h->avg, avg, (size_t)n_avg * sizeof(float), hipMemcpyHostToDevice, s));
  return set_state_host(h, mean, var, std, (long long)count, s);
}

}  // extern "C"
