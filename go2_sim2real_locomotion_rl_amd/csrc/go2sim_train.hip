// go2sim_train.hip -- the PPO update next to the policy step (include/go2sim_train.h).  gfx950 only.
//
// One mini-batch is a fixed sequence of launches on the caller's stream, no host synchronisation and no floating-point atomics anywhere:
//   k_train_forward   the layer loop of the inference kernel (go2sim_mlp_dev.h), rows read through the permutation index; every hidden layer's
//                     post-activation [rows][npad] goes to the workspace, the outputs to mu [rows][A] / v [rows].  Actor and critic share the launch.
//   k_ppo_head        one lane per row: logp, ratio, kl, the two losses, d loss / d mu and d loss / d v (these are the last layers' dZ), per-workgroup
//                     float64 partial sums of surrogate, value loss, kl and d loss / d sigma[A].  Per-row scalars are evaluated in float64 and rounded once.
//   k_ppo_finalize    adds the partials in workgroup order, applies the learning-rate rule to the device-side learning rate, writes the std gradient
//                     and the running sums of the reported means.
//   per layer, last to first (both networks per launch):
//     k_bwd_dw        dW = dZ^T A_prev per row chunk of GO2SIM_PPO_ROW_CHUNK rows: a workgroup owns 2 x 4 output tiles of 16 x 16, its four wavefronts
//                     take a quarter of the chunk's rows each (8 independent accumulators per wavefront, chains of 128 rows), their results are added
//                     in wavefront order through LDS and written to the chunk's slab of partials.
//     k_bwd_db        db = column sums of dZ per chunk (float64: 16 row slices per column, added in slice order), into the same slab.
//     k_bwd_da        dZ_prev = (dZ W) * f'(A_prev) (f: the network's activation, ELU by default), 32 rows per workgroup, 4 accumulators per wavefront.  W is read strided ([npad][kpad], the
//                     reduction runs over its rows): no transposed copy of the weights is kept, the optimizer writes one array per layer.
//                     Not launched for the first layer.
//   k_reduce_partials adds the chunk slabs in chunk order in float64 and rounds once: the padded gradient vector.
// A shard of a mini-batch that spans ranks (go2sim_ppo_shard_grad / go2sim_ppo_shard_reduce) runs the same launches with the global row weight and
// replaces k_ppo_finalize and k_reduce_partials by
//   k_shard_record    the same two sums (chunk slabs in chunk order, head partials in workgroup order) left in float64: the shard's record.
//   k_shard_reduce    one pass over [records][padded vector]: adds the records in record order, rounds once into the gradient vector, the entropy term
//                     on the std block.   k_shard_scalars: one workgroup, the three sums over the records' rows and the learning-rate rule.
// The optimizer is two launches: k_sumsq (per-workgroup float64 sums of squares, pairwise tree) and k_adam (every workgroup adds those in the same
// order, then clip coefficient and Adam in one pass over the padded parameters, written into the arrays go2sim_policy_act reads and into std).
// Adam's per-element arithmetic is float64 on fp32 state, rounded once per stored value.
// Mirror symmetry (go2sim_ppo_set_mirror): the same launches over 2 n rows, row n + r the mirror of row r.  No mirrored row is ever stored: the input tile
// load of k_train_forward and the first layer's A_prev read of k_bwd_dw read row idx[r] through the signed column permutation (tables staged in LDS,
// respectively in registers, once per workgroup); k_ppo_head permutes the actions the same way, reads row r's scalars, adds the mirror-loss term to
// the mirrored rows' dZ and sums (mu' - target)^2 in one more float64 partial column.  The kernels that gather are templates on the mirror: a handle
// without tables runs the code it ran before.
// Recurrent policy (go2sim_ppo_create_recurrent, include/go2sim_rnn.h; the end of this file): an LSTM memory in front of each network.  A mini-batch is an env
// block with all its steps: T launches of k_lstm_cell (go2sim_lstm_dev.h), the launches above on the T x block rows of h' (k_bwd_da<true> also writes the first
// layer's d loss / d h'), T launches of k_lstm_bptt back through time, then k_bwd_dw / k_bwd_db for the memories' weights.  The memories' segments follow the two
// networks in the padded vectors, so the chunk reduction, the norm and k_adam<true> cover them.  A handle without memories runs the plain instantiations.
// Padding: padded rows of dZ^T and padded columns of A_prev are exact zeros, so padded gradient entries are sums of exact zeros, and Adam leaves a
// zero parameter with zero gradient, m and v at zero.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "go2sim_mlp_dev.h"
#include "go2sim_train_dev.h"  // the kernels shared with go2sim_distill.hip: k_train_forward, k_bwd_dw / db / da, k_reduce_partials, k_sumsq, k_adam, k_pack
#define GO2SIM_HIPCHK_TAG "go2sim_train"
#include "go2sim_trainer_host.h"  // the host side shared with go2sim_distill.hip: HIPCHK, the optimizer state, packing, workspaces, the backward schedule
#include "go2sim_lstm_dev.h"   // the memories of a recurrent policy: LstmDev, struct go2sim_lstm, k_lstm_cell, k_lstm_bptt
#include "../../include/go2sim_train.h"
#include "../../include/go2sim_rnn.h"

namespace {

struct HeadArgs {
  const float *mu, *val;                                  // [n][A], [n]: this mini-batch's forward
  go2sim_ppo_batch_t b;
  const float* std_;
  const int32_t* idx;
  float *dz_actor, *dz_critic;                            // [rows][Apad], [rows][16]
  double* part;                                           // [workgroups][3 + A], with a mirror [workgroups][4 + A]
  int n, A, Apad, use_clipped;
  double clip, vl_coef;
  double w;                                               // weight of a row in the means: 1 / n, or 1 / (rows of all shards); with augmentation half of it
  // mirror: rows [n, n_rows) are the mirrors of rows [0, n)
  int n_rows, ppo_on_mirrors, use_mirror_loss;
  MirTab ta;                                              // the action table
  double w_sym;                                           // mirror_loss_coeff * 2 / (n A) (n over all shards)
};

// the action of row r as the head sees it: the stored one, or its mirror
template <bool MIR>
__device__ __forceinline__ double head_action(const HeadArgs& h, size_t src, int a, bool mirrored, const int32_t* s_asrc, const float* s_asign) {
  if (MIR && mirrored) return (double)(s_asign[a] * h.b.actions[src * h.A + s_asrc[a]]);
  return h.b.actions[src * h.A + a];
}

template <bool MIR>
__global__ __launch_bounds__(WGT) void k_ppo_head(HeadArgs h) {
  __shared__ double s_red[WGT];
  __shared__ int32_t s_asrc[MIR ? MAXW : 1];
  __shared__ float s_asign[MIR ? MAXW : 1];
  const int r = blockIdx.x * WGT + threadIdx.x, A = h.A;
  const int n_rows = MIR ? h.n_rows : h.n;
  const bool mirrored = MIR && r >= h.n && r < n_rows;
  const bool on = MIR ? (r < h.n || (mirrored && h.ppo_on_mirrors)) : r < h.n;   // the PPO terms of this row count
  if (MIR) {
    for (int a = threadIdx.x; a < A; a += WGT) { s_asrc[a] = h.ta.src[a]; s_asign[a] = h.ta.sign[a]; }
    __syncthreads();
  }
  double sur = 0.0, vl = 0.0, kl = 0.0, dlogp = 0.0, sym = 0.0;
  size_t src = 0;
  if (MIR && mirrored) {
    src = (size_t)h.idx[r - h.n];
    // mirror loss: mu(M_o obs_q)[a] against the detached target (M_a mu(obs_q))[a]; without PPO weight on this row the loop below does not run
    for (int a = 0; a < h.Apad; ++a) {
      float g = 0.0f;
      if (a < A) {
        const double d = (double)h.mu[(size_t)r * A + a] - (double)(s_asign[a] * h.mu[(size_t)(r - h.n) * A + s_asrc[a]]);
        sym += d * d;
        if (h.use_mirror_loss && !on) g = (float)(h.w_sym * d);
      }
      if (!on) h.dz_actor[(size_t)r * h.Apad + a] = g;
    }
    if (!on)
      for (int c = 0; c < 16; ++c) h.dz_critic[(size_t)r * 16 + c] = 0.0f;
  }
  if (on) {
    if (!mirrored) src = (size_t)h.idx[r];
    const double w = h.w;
    double lp = 0.0;
    for (int a = 0; a < A; ++a) {
      const double x = head_action<MIR>(h, src, a, mirrored, s_asrc, s_asign), m = h.mu[(size_t)r * A + a], s = h.std_[a];
      const double d = x - m;
      lp += -(d * d) / (2.0 * (s * s)) - log(s) - 0.91893853320467274178;
      if (!mirrored) {                                     // kl_mean is taken over the original rows
        const double os = h.b.old_sigma[src * A + a], om = h.b.old_mu[src * A + a], dm = om - m;
        kl += log(s / os + 1e-5) + (os * os + dm * dm) / (2.0 * (s * s)) - 0.5;
      }
    }
    const double adv = h.b.advantages[src];
    const double ratio = exp(lp - (double)h.b.old_log_prob[src]);
    const double lo = 1.0 - h.clip, hi = 1.0 + h.clip;
    const bool inside = ratio >= lo && ratio <= hi;
    const double rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
    const double s1 = -adv * ratio, s2 = -adv * rc;
    sur = s1 > s2 ? s1 : s2;
    // torch's max(): the larger arm takes the gradient, equal arms share it; clamp passes it inside its range only
    const double g_ratio = inside ? -adv : (s1 > s2 ? -adv : (s1 == s2 ? -0.5 * adv : 0.0));
    dlogp = g_ratio * ratio * w;
    const double v = h.val[r], tv = h.b.target_values[src], ret = h.b.returns[src];
    double dv;
    if (h.use_clipped) {
      const double dvt = v - tv;
      const bool vin = dvt >= -h.clip && dvt <= h.clip;
      const double vc = tv + (dvt < -h.clip ? -h.clip : (dvt > h.clip ? h.clip : dvt));
      const double e1 = (v - ret) * (v - ret), e2 = (vc - ret) * (vc - ret);
      vl = e1 > e2 ? e1 : e2;
      dv = vin ? 2.0 * (v - ret) : (e1 > e2 ? 2.0 * (v - ret) : (e1 == e2 ? (v - ret) : 0.0));
    } else {
      vl = (ret - v) * (ret - v);
      dv = 2.0 * (v - ret);
    }
    dv = dv * h.vl_coef * w;
    for (int a = 0; a < h.Apad; ++a) {
      float g = 0.0f;
      if (a < A) {
        const double x = head_action<MIR>(h, src, a, mirrored, s_asrc, s_asign), m = h.mu[(size_t)r * A + a], s = h.std_[a];
        double gd = dlogp * (x - m) / (s * s);
        if (MIR && mirrored && h.use_mirror_loss) gd += h.w_sym * (m - (double)(s_asign[a] * h.mu[(size_t)(r - h.n) * A + s_asrc[a]]));
        g = (float)gd;
      }
      h.dz_actor[(size_t)r * h.Apad + a] = g;
    }
    for (int c = 0; c < 16; ++c) h.dz_critic[(size_t)r * 16 + c] = c == 0 ? (float)dv : 0.0f;
  }
  double* part = h.part + (size_t)blockIdx.x * ((MIR ? 4 : 3) + A);
  double t;
  t = wg_sum(s_red, sur); if (threadIdx.x == 0) part[0] = t;
  t = wg_sum(s_red, vl);  if (threadIdx.x == 0) part[1] = t;
  t = wg_sum(s_red, kl);  if (threadIdx.x == 0) part[2] = t;
  for (int a = 0; a < A; ++a) {                           // d logp / d sigma_a = (a - mu)^2 / sigma^3 - 1 / sigma
    double g = 0.0;
    if (on) {
      const double x = head_action<MIR>(h, src, a, mirrored, s_asrc, s_asign), m = h.mu[(size_t)r * A + a], s = h.std_[a];
      const double d = x - m;
      g = dlogp * ((d * d) / (s * s * s) - 1.0 / s);
    }
    t = wg_sum(s_red, g); if (threadIdx.x == 0) part[3 + a] = t;
  }
  if (MIR) { t = wg_sum(s_red, sym); if (threadIdx.x == 0) part[3 + A] = t; }
}

// the mini-batch's means are known: entropy, the learning-rate rule on kl_mean, the running sums of the reported means (one thread)
__device__ __forceinline__ void close_minibatch(double sur_mean, double vl_mean, double kl_mean, double sym_mean, int A, const float* __restrict__ std_,
                                                double* __restrict__ scal, double desired_kl, double lr_min, double lr_max, int adaptive) {
  double ent = 0.0;
  for (int a = 0; a < A; ++a) ent += 0.5 + 0.5 * 1.8378770664093454836 + log((double)std_[a]);
  if (adaptive) {
    double lr = scal[S_LR];
    if (kl_mean > 2.0 * desired_kl) lr = fmax(lr_min, lr / 1.5);
    else if (kl_mean < desired_kl / 2.0 && kl_mean > 0.0) lr = fmin(lr_max, lr * 1.5);
    scal[S_LR] = lr;
  }
  scal[S_KL] = kl_mean;
  scal[S_SUM_SUR] += sur_mean; scal[S_SUM_VL] += vl_mean; scal[S_SUM_ENT] += ent; scal[S_COUNT] += 1.0;
  scal[S_SUM_SYM] += sym_mean;
}

// one workgroup: column q of the head's partials is added in workgroup order by lane q (q = 0 surrogate, 1 value loss, 2 kl, 3 + a d sigma_a, with a
// mirror 3 + A the mirror loss).  n: original rows; n_ppo: rows in the means of surrogate and value loss (2 n under augmentation); ncol: columns of `part`
__global__ __launch_bounds__(64) void k_ppo_finalize(const double* __restrict__ part, int n_wg, int ncol, int n, int n_ppo, int A, const float* __restrict__ std_,
                                                     double* __restrict__ scal, float* __restrict__ grad_std, double entropy_coef, double desired_kl, double lr_min,
                                                     double lr_max, int adaptive) {
  __shared__ double s4[4];
  if (threadIdx.x == 0) s4[3] = 0.0;
  for (int q = threadIdx.x; q < ncol; q += 64) {
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += part[(size_t)w * ncol + q];
    if (q < 2) s4[q] = s / (double)n_ppo;
    else if (q == 2) s4[q] = s / (double)n;
    else if (q < 3 + A) grad_std[q - 3] = (float)(s - entropy_coef / (double)std_[q - 3]);     // the entropy bonus: - entropy_coef * d/d sigma sum_a log sigma
    else s4[3] = s / ((double)n * (double)A);
  }
  __syncthreads();
  if (threadIdx.x == 0) close_minibatch(s4[0], s4[1], s4[2], s4[3], A, std_, scal, desired_kl, lr_min, lr_max, adaptive);
}


// A shard's record (include/go2sim_train.h): entry i of [0, slab) is k_reduce_partials' sum without the rounding, the Apad entries after it are the
// head's d loss / d sigma partials added in workgroup order (no entropy term), the last four the sums of surrogate, value loss, kl and the row count.
// With a mirror one more entry follows: the sum of (mu' - target)^2 (column 3 + A of the head's partials, ncol = 4 + A).
__global__ __launch_bounds__(WGT) void k_shard_record(const float* __restrict__ partial, int n_chunks, size_t slab, const double* __restrict__ part, int n_wg,
                                                      int ncol, int A, int Apad, int n_rows, double* __restrict__ rec) {
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= slab + (size_t)Apad + 4 + (size_t)(ncol - 3 - A)) return;
  double s = 0.0;
  if (i < slab) {
    for (int c = 0; c < n_chunks; ++c) s += (double)partial[(size_t)c * slab + i];
  } else {
    const int k = (int)(i - slab);
    int q = -1;                                            // column of the head's partials
    if (k < Apad) { if (k < A) q = 3 + k; }
    else if (k - Apad < 3) q = k - Apad;
    else if (k - Apad == 3) s = (double)n_rows;
    else q = 3 + A;
    if (q >= 0)
      for (int w = 0; w < n_wg; ++w) s += part[(size_t)w * ncol + q];
  }
  rec[i] = s;
}

// entry i of the padded gradient vector: the records' entries added in record order, rounded once; the std block takes the entropy bonus here
__global__ __launch_bounds__(WGT) void k_shard_reduce(const double* __restrict__ rec, int n_rec, size_t len, size_t slab, int A, int Apad,
                                                      const float* __restrict__ std_, double entropy_coef, float* __restrict__ grads) {
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= slab + (size_t)Apad) return;
  double s = 0.0;
  for (int r = 0; r < n_rec; ++r) s += rec[(size_t)r * len + i];
  if (i < slab) grads[i] = (float)s;
  else {
    const int a = (int)(i - slab);
    grads[i] = a < A ? (float)(s - entropy_coef / (double)std_[a]) : 0.0f;
  }
}

// one workgroup: lane q adds scalar q of the records in record order (surrogate, value loss, kl, rows, with a mirror the mirror-loss sum); the scalars
// start at `off`.  ppo_mult: 2 under augmentation (surrogate and value loss are means over originals and mirrors), else 1
__global__ __launch_bounds__(64) void k_shard_scalars(const double* __restrict__ rec, int n_rec, size_t len, size_t off, int n_scal, int ppo_mult, int A,
                                                      const float* __restrict__ std_, double* __restrict__ scal, double desired_kl, double lr_min, double lr_max,
                                                      int adaptive) {
  __shared__ double s5[5];
  if (threadIdx.x < 5) {
    double s = 0.0;
    if ((int)threadIdx.x < n_scal)
      for (int r = 0; r < n_rec; ++r) s += rec[(size_t)r * len + off + threadIdx.x];
    s5[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = (int)s5[3], n_ppo = ppo_mult * n;        // the divisors as k_ppo_finalize forms them
    close_minibatch(s5[0] / (double)n_ppo, s5[1] / (double)n_ppo, s5[2] / (double)n, s5[4] / ((double)n * (double)A), A, std_, scal, desired_kl, lr_min, lr_max,
                    adaptive);
  }
}

__global__ void k_reset_stats(double* scal) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal[S_SUM_VL] = 0.0; scal[S_SUM_SUR] = 0.0; scal[S_SUM_ENT] = 0.0; scal[S_COUNT] = 0.0; scal[S_SUM_SYM] = 0.0; }
}
__global__ void k_sym_loss(const double* __restrict__ scal, double* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = scal[S_SUM_SYM] / (scal[S_COUNT] > 0.0 ? scal[S_COUNT] : 1.0);
}
__global__ void k_stats(const double* __restrict__ scal, double step, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double c = scal[S_COUNT] > 0.0 ? scal[S_COUNT] : 1.0;
  out[GO2SIM_PPO_ST_VALUE_LOSS] = scal[S_SUM_VL] / c; out[GO2SIM_PPO_ST_SURROGATE] = scal[S_SUM_SUR] / c; out[GO2SIM_PPO_ST_ENTROPY] = scal[S_SUM_ENT] / c;
  out[GO2SIM_PPO_ST_KL] = scal[S_KL]; out[GO2SIM_PPO_ST_LR] = scal[S_LR]; out[GO2SIM_PPO_ST_GRAD_NORM] = scal[S_NORM];
  out[GO2SIM_PPO_ST_STEP] = step; out[GO2SIM_PPO_ST_COUNT] = scal[S_COUNT];
}

}  // namespace

struct go2sim_ppo {
  go2sim_mlp *actor = nullptr, *critic = nullptr;
  go2sim_ppo_cfg_t cfg{};
  int A = 0, Apad = 0, max_rows = 0, max_chunks = 0, max_head_wg = 0;
  size_t nA = 0, nC = 0, n_flat = 0;
  OptState opt;               // the optimizer's vectors over slab + Apad floats, the scalars, the step count
  float* wbuf = nullptr;      // the workspaces of ws_rows rows: mu | val | per network activations, dz ping-pong | partial slabs
  float *mu = nullptr, *val = nullptr, *partial = nullptr;
  NetWs nw[2]{};
  double* hbuf = nullptr;     // head partials, [workgroups of ws_rows][4 + A]
  double* head_part = nullptr;
  size_t ws_rows = 0;         // max_rows, twice that once a mirror has been set
  std::vector<Seg> segs;      // base 0 actor, 1 critic, 2 std, 3 memory_a, 4 memory_c
  // mirror symmetry (go2sim_ppo_set_mirror): the tables live in one device allocation each, obs | critic obs | actions
  int mirror = 0, use_aug = 0, use_mloss = 0;
  double mirror_coeff = 0.0;
  int32_t* mir_src = nullptr;
  float* mir_sign = nullptr;
  MirTab tab[3]{};            // 0 actor input, 1 critic input, 2 actions
  // recurrent policy (go2sim_ppo_create_recurrent): the two memories, their blocks after the networks in the padded vectors, the per-step workspaces
  go2sim_lstm* mem[2] = {nullptr, nullptr};
  size_t nM[2] = {0, 0};
  size_t slab = 0;            // nA + nC + nM[0] + nM[1]: what the row chunks reduce; the std block follows
  int rnn = 0, T = 0, nb_max = 0;
  float* rbuf = nullptr;      // per memory: gates | dz [R][4 Hpad], hprev | cprev | hout | cout [R][H], dh_mlp [R][Hpad], dc [nb_max][Hpad]
  int32_t* ibuf = nullptr;    // idx_b [R] (rows of the env block in the batch arrays) | idx_id [R] (0 .. R - 1)
  float *r_gates[2]{}, *r_dz[2]{}, *r_hprev[2]{}, *r_cprev[2]{}, *r_hout[2]{}, *r_cout[2]{}, *r_dh[2]{}, *r_dc[2]{};
  int32_t *idx_b = nullptr, *idx_id = nullptr;
};

namespace {
BwdLayer bwd_layer(const go2sim_ppo* h, int net, int lb, const go2sim_ppo_batch_t* batch) {
  return bwd_layer(net == 0 ? h->actor : h->critic, h->nw[net], lb, net == 0 ? batch->obs : batch->critic_obs, 1, h->tab[net], net == 0 ? 0 : h->nA);
}
// (re)allocates the row workspaces for R rows; the optimizer's vectors and the scalars are not touched.  hipFree waits for the device.
int alloc_workspaces(go2sim_ppo* h, size_t R) {
  const go2sim_mlp* nets[2] = {h->actor, h->critic};
  size_t need = al16(R * h->A) + al16(R) + net_ws_floats(nets[0], R) + net_ws_floats(nets[1], R);
  const int chunks = (int)((R + RCH - 1) / RCH), head_wg = (int)((R + WGT - 1) / WGT);
  const size_t slab = h->slab;
  need += (size_t)chunks * slab;
  const size_t nd = (size_t)head_wg * (4 + h->A);
  float* wb = nullptr;
  double* hb = nullptr;
  if (hipMalloc((void**)&wb, need * sizeof(float)) != hipSuccess) return GO2SIM_E_NOMEM;
  if (hipMalloc((void**)&hb, nd * sizeof(double)) != hipSuccess) { (void)hipFree(wb); return GO2SIM_E_NOMEM; }
  if (hipMemset(wb, 0, need * sizeof(float)) != hipSuccess || hipMemset(hb, 0, nd * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fprintf(stderr, "go2sim_train: initialising the workspaces failed: %s\n", hipGetErrorString(hipGetLastError()));
    (void)hipFree(wb); (void)hipFree(hb);
    return GO2SIM_E_HIP;
  }
  if (h->wbuf) (void)hipFree(h->wbuf);
  if (h->hbuf) (void)hipFree(h->hbuf);
  h->wbuf = wb; h->hbuf = hb; h->head_part = hb; h->ws_rows = R; h->max_chunks = chunks; h->max_head_wg = head_wg;
  float* p = wb;
  h->mu = p; p += al16(R * h->A); h->val = p; p += al16(R);
  for (int net = 0; net < 2; ++net) p = net_ws_carve(nets[net], R, p, h->nw[net]);
  h->partial = p;
  return GO2SIM_E_OK;
}
int pack_all(go2sim_ppo* h, int which, int to_padded, float* flat, float* std_dev, hipStream_t st) {
  if (!h || !flat || which < GO2SIM_PPO_PARAMS || which > GO2SIM_PPO_ADAM_V) return GO2SIM_E_BADARG;
  if (which == GO2SIM_PPO_PARAMS && !std_dev) return GO2SIM_E_BADARG;
  float* base[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (which == GO2SIM_PPO_PARAMS) {
    base[0] = h->actor->dparams; base[1] = h->critic->dparams; base[2] = std_dev;
    if (h->rnn) { base[3] = h->mem[0]->dparams; base[4] = h->mem[1]->dparams; }
  } else {
    float* v = opt_vec(h->opt, which);
    base[0] = v; base[1] = v + h->nA; base[2] = v + h->slab; base[3] = v + h->nA + h->nC; base[4] = base[3] + h->nM[0];
  }
  return pack_segs(h->segs, base, to_padded, flat, st);
}

// the row workspaces of a recurrent handle: R = T x nb_max rows per memory
int alloc_rnn_workspaces(go2sim_ppo* h) {
  const size_t R = (size_t)h->T * h->nb_max;
  size_t need = 0;
  for (int net = 0; net < 2; ++net) {
    const size_t H = h->mem[net]->H, Hp = h->mem[net]->dev.Hpad;
    need += 2 * al16(R * 4 * Hp) + 4 * al16(R * H) + al16(R * Hp) + al16((size_t)h->nb_max * Hp);
  }
  if (hipMalloc((void**)&h->rbuf, need * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->ibuf, 2 * R * sizeof(int32_t)) != hipSuccess) return GO2SIM_E_NOMEM;
  HIPCHK(hipMemset(h->rbuf, 0, need * sizeof(float)));
  float* p = h->rbuf;
  for (int net = 0; net < 2; ++net) {
    const size_t H = h->mem[net]->H, Hp = h->mem[net]->dev.Hpad;
    h->r_gates[net] = p; p += al16(R * 4 * Hp); h->r_dz[net] = p; p += al16(R * 4 * Hp);
    h->r_hprev[net] = p; p += al16(R * H); h->r_cprev[net] = p; p += al16(R * H); h->r_hout[net] = p; p += al16(R * H); h->r_cout[net] = p; p += al16(R * H);
    h->r_dh[net] = p; p += al16(R * Hp); h->r_dc[net] = p; p += al16((size_t)h->nb_max * Hp);
  }
  h->idx_b = h->ibuf; h->idx_id = h->ibuf + R;
  hipLaunchKernelGGL(k_iota, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, 0, h->idx_id, (int)R);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return GO2SIM_E_OK;
}

// go2sim_ppo_create and go2sim_ppo_create_recurrent (ma, mc and n_steps set: max_rows = n_steps x the envs of a mini-batch)
int create_impl(go2sim_mlp_t* actor, go2sim_mlp_t* critic, go2sim_lstm* ma, go2sim_lstm* mc, int n_steps, int n_actions, const go2sim_ppo_cfg_t* cfg, int max_rows,
                go2sim_ppo_t** out) {
  if (!actor || !critic || !cfg || !out || max_rows < 1 || n_actions < 1) return GO2SIM_E_BADARG;
  if (actor->dims[actor->n_layers] != n_actions || critic->dims[critic->n_layers] != 1 || actor->device != critic->device) return GO2SIM_E_BADARG;
  if (!(cfg->learning_rate > 0.0) || !(cfg->clip_param >= 0.0)) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(actor->device));
  go2sim_ppo* h = new (std::nothrow) go2sim_ppo();
  if (!h) return GO2SIM_E_NOMEM;
  h->actor = actor; h->critic = critic; h->cfg = *cfg; h->A = n_actions; h->Apad = round16(n_actions); h->max_rows = max_rows;
  h->nA = actor->padded; h->nC = critic->padded;
  if (ma) { h->rnn = 1; h->mem[0] = ma; h->mem[1] = mc; h->nM[0] = ma->padded; h->nM[1] = mc->padded; h->T = n_steps; h->nb_max = max_rows / n_steps; }
  h->slab = h->nA + h->nC + h->nM[0] + h->nM[1];
  // flat (state-dict) order: actor W0, b0, ..., critic W0, b0, ..., (the memories,) std
  size_t flat = 0;
  mlp_segs(h->segs, 0, actor, flat);
  mlp_segs(h->segs, 1, critic, flat);
  if (h->rnn) { lstm_segs(h->segs, 3, ma, flat); lstm_segs(h->segs, 4, mc, flat); }
  h->segs.push_back(Seg{2, 0, n_actions, 1, n_actions, flat}); flat += n_actions;
  h->n_flat = flat;
  if (!opt_alloc(h->opt, h->slab + h->Apad, 0)) {
    go2sim_ppo_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  if (!opt_zero(h->opt, cfg->learning_rate, nullptr, 0)) {
    fprintf(stderr, "go2sim_train: initialising the optimizer state failed: %s\n", hipGetErrorString(hipGetLastError()));
    go2sim_ppo_destroy(h);
    return GO2SIM_E_HIP;
  }
  int rc = alloc_workspaces(h, (size_t)max_rows);
  if (rc == GO2SIM_E_OK && h->rnn) rc = alloc_rnn_workspaces(h);
  if (rc != GO2SIM_E_OK) {
    go2sim_ppo_destroy(h);
    return rc;
  }
  *out = h;
  return GO2SIM_E_OK;
}
}  // namespace

extern "C" {

int go2sim_ppo_create(go2sim_mlp_t* actor, go2sim_mlp_t* critic, int n_actions, const go2sim_ppo_cfg_t* cfg, int max_rows, go2sim_ppo_t** out) {
  return create_impl(actor, critic, nullptr, nullptr, 0, n_actions, cfg, max_rows, out);
}

int go2sim_ppo_create_recurrent(go2sim_mlp_t* actor, go2sim_mlp_t* critic, go2sim_lstm_t* mem_a, go2sim_lstm_t* mem_c, int n_actions, const go2sim_ppo_cfg_t* cfg,
                                int n_steps, int max_envs, go2sim_ppo_t** out) {
  if (!actor || !critic || !mem_a || !mem_c || n_steps < 1 || max_envs < 1 || (long long)n_steps * max_envs > 0x7fffffffLL / 4 / MAXW) return GO2SIM_E_BADARG;
  if (mem_a->H != actor->dims[0] || mem_c->H != critic->dims[0] || mem_a->device != actor->device || mem_c->device != actor->device) return GO2SIM_E_BADARG;
  return create_impl(actor, critic, mem_a, mem_c, n_steps, n_actions, cfg, n_steps * max_envs, out);
}

int go2sim_ppo_destroy(go2sim_ppo_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  if (h->rbuf) (void)hipFree(h->rbuf);
  if (h->ibuf) (void)hipFree(h->ibuf);
  opt_free(h->opt);
  if (h->wbuf) (void)hipFree(h->wbuf);
  if (h->hbuf) (void)hipFree(h->hbuf);
  if (h->mir_src) (void)hipFree(h->mir_src);
  if (h->mir_sign) (void)hipFree(h->mir_sign);
  delete h;
  return GO2SIM_E_OK;
}

}  // extern "C"

// the head's arguments for n rows of this mini-batch's forward (n_rows with their mirrors), a row weighing w; no mirror terms
static HeadArgs head_args(const go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, int n_rows, double w) {
  HeadArgs ha{};
  ha.mu = h->mu; ha.val = h->val; ha.b = *b; ha.std_ = std_dev; ha.idx = idx;
  ha.dz_actor = h->nw[0].dz[(h->actor->n_layers - 1) & 1]; ha.dz_critic = h->nw[1].dz[(h->critic->n_layers - 1) & 1];
  ha.part = h->head_part; ha.n = n; ha.A = h->A; ha.Apad = h->Apad; ha.use_clipped = h->cfg.use_clipped_value_loss;
  ha.clip = h->cfg.clip_param; ha.vl_coef = h->cfg.value_loss_coef; ha.w = w; ha.n_rows = n_rows;
  return ha;
}

// The launches of one mini-batch.  record == nullptr: the rows are the whole mini-batch (k_ppo_finalize, k_reduce_partials); otherwise they are a shard of it
// and the sums stay in float64 in `record`.  w: 1 / (rows of the mini-batch over all shards).  With a mirror the forward and the head run over 2 n rows
// (the mirror loss is always reported), the backward too unless both flags are off: then no mirrored row carries a gradient.
template <bool MIR>
static int launch_grad_t(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, double w, double* record, hipStream_t st) {
  const go2sim_mlp *Ma = h->actor, *Mc = h->critic;
  const int n_fwd = MIR ? 2 * n : n, n_bwd = (MIR && (h->use_aug || h->use_mloss)) ? 2 * n : n;
  const int ncol = (MIR ? 4 : 3) + h->A;
  hipLaunchKernelGGL(k_train_forward<MIR>, dim3((n_fwd + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, Ma->dev, b->obs, h->mu, h->nw[0].a, Mc->dev, b->critic_obs, h->val,
                     h->nw[1].a, idx, n_fwd, n, h->tab[0], h->tab[1]);
  const int n_wg = (n_fwd + WGT - 1) / WGT;
  HeadArgs ha = head_args(h, b, std_dev, idx, n, n_fwd, (MIR && h->use_aug) ? 0.5 * w : w);      // 1 / (2 n): halving is exact
  ha.ppo_on_mirrors = MIR && h->use_aug; ha.use_mirror_loss = MIR && h->use_mloss; ha.ta = h->tab[2];
  ha.w_sym = h->mirror_coeff * 2.0 * w / (double)h->A;
  hipLaunchKernelGGL(k_ppo_head<MIR>, dim3(n_wg), dim3(WGT), 0, st, ha);
  if (!record)
    hipLaunchKernelGGL(k_ppo_finalize, dim3(1), dim3(64), 0, st, h->head_part, n_wg, ncol, n, (MIR && h->use_aug) ? 2 * n : n, h->A, std_dev, h->opt.scal,
                       h->opt.grads + h->slab, h->cfg.entropy_coef, h->cfg.desired_kl, h->cfg.lr_min, h->cfg.lr_max, h->cfg.adaptive);
  const int n_chunks = (n_bwd + RCH - 1) / RCH;
  const size_t slab = h->slab;
  const int depth = Ma->n_layers > Mc->n_layers ? Ma->n_layers : Mc->n_layers;
  BwdLayer L[MAXL][2];
  for (int lb = 0; lb < depth; ++lb)
    for (int net = 0; net < 2; ++net) L[lb][net] = bwd_layer(h, net, lb, b);
  launch_backward<MIR, false>(L, depth, BwdRun{2, idx, n_bwd, n, h->partial, slab, st});
  if (!record)
    hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)((slab + WGT - 1) / WGT)), dim3(WGT), 0, st, h->partial, n_chunks, slab, h->opt.grads);
  else
    hipLaunchKernelGGL(k_shard_record, dim3((unsigned)((h->opt.n_tot + 5 + WGT - 1) / WGT)), dim3(WGT), 0, st, h->partial, n_chunks, slab, h->head_part, n_wg, ncol, h->A,
                       h->Apad, n, record);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
static int launch_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, double w, double* record, hipStream_t st) {
  return h->mirror ? launch_grad_t<true>(h, b, std_dev, idx, n, w, record, st) : launch_grad_t<false>(h, b, std_dev, idx, n, w, record, st);
}

extern "C" {

static bool batch_ok(const go2sim_ppo_batch_t* b) {
  return b && b->obs && b->critic_obs && b->actions && b->target_values && b->returns && b->advantages && b->old_log_prob && b->old_mu && b->old_sigma;
}

int go2sim_ppo_minibatch_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, void* stream) {
  if (!h || h->rnn || !std_dev || !idx || n < 1 || n > h->max_rows || !batch_ok(b)) return GO2SIM_E_BADARG;
  return launch_grad(h, b, std_dev, idx, n, 1.0 / (double)n, nullptr, (hipStream_t)stream);
}

int go2sim_ppo_shard_len(go2sim_ppo_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->opt.n_tot + 4 + (h->mirror ? 1 : 0);
  return GO2SIM_E_OK;
}

int go2sim_ppo_shard_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, long long n_global, double* record,
                          void* stream) {
  if (!h || h->rnn || !std_dev || !idx || !record || n < 1 || n > h->max_rows || n_global < (long long)n || !batch_ok(b)) return GO2SIM_E_BADARG;
  return launch_grad(h, b, std_dev, idx, n, 1.0 / (double)n_global, record, (hipStream_t)stream);
}

int go2sim_ppo_shard_reduce(go2sim_ppo_t* h, const double* records, int n_records, const float* std_dev, void* stream) {
  if (!h || h->rnn || !records || !std_dev || n_records < 1) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t slab = h->slab, len = h->opt.n_tot + 4 + (h->mirror ? 1 : 0);
  hipLaunchKernelGGL(k_shard_reduce, dim3((unsigned)((h->opt.n_tot + WGT - 1) / WGT)), dim3(WGT), 0, st, records, n_records, len, slab, h->A, h->Apad, std_dev,
                     h->cfg.entropy_coef, h->opt.grads);
  hipLaunchKernelGGL(k_shard_scalars, dim3(1), dim3(64), 0, st, records, n_records, len, h->opt.n_tot, h->mirror ? 5 : 4, (h->mirror && h->use_aug) ? 2 : 1, h->A,
                     std_dev, h->opt.scal, h->cfg.desired_kl, h->cfg.lr_min, h->cfg.lr_max, h->cfg.adaptive);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_ppo_set_mirror(go2sim_ppo_t* h, const go2sim_ppo_mirror_t* m, void* stream) {
  if (!h || (h->rnn && m)) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (!m) {                                                // back to the plain path; the larger workspaces stay
    h->mirror = h->use_aug = h->use_mloss = 0;
    h->mirror_coeff = 0.0;
    return GO2SIM_E_OK;
  }
  if (!m->obs_src || !m->obs_sign || !m->critic_src || !m->critic_sign || !m->action_src || !m->action_sign || !std::isfinite(m->mirror_loss_coeff))
    return GO2SIM_E_BADARG;
  const int width[3] = {h->actor->dims[0], h->critic->dims[0], h->A};
  const int32_t* src[3] = {m->obs_src, m->critic_src, m->action_src};
  const float* sign[3] = {m->obs_sign, m->critic_sign, m->action_sign};
  const int total = width[0] + width[1] + width[2];
  std::vector<int32_t> hs((size_t)total);
  std::vector<float> hg((size_t)total);
  int off[3], o = 0;
  for (int t = 0; t < 3; ++t) {
    off[t] = o;
    HIPCHK(hipMemcpyAsync(hs.data() + o, src[t], width[t] * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hg.data() + o, sign[t], width[t] * sizeof(float), hipMemcpyDeviceToHost, st));
    o += width[t];
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int t = 0; t < 3; ++t) {                            // indices in range, every index once, signs +1 or -1
    std::vector<char> seen((size_t)width[t], 0);
    for (int j = 0; j < width[t]; ++j) {
      const int32_t k = hs[off[t] + j];
      const float g = hg[off[t] + j];
      if (k < 0 || k >= width[t] || seen[k] || !(g == 1.0f || g == -1.0f)) return GO2SIM_E_BADARG;
      seen[k] = 1;
    }
  }
  if (h->ws_rows < 2 * (size_t)h->max_rows) {
    const int rc = alloc_workspaces(h, 2 * (size_t)h->max_rows);
    if (rc != GO2SIM_E_OK) return rc;
  }
  if (!h->mir_src) {
    if (hipMalloc((void**)&h->mir_src, total * sizeof(int32_t)) != hipSuccess || hipMalloc((void**)&h->mir_sign, total * sizeof(float)) != hipSuccess) return GO2SIM_E_NOMEM;
  }
  HIPCHK(hipMemcpyAsync(h->mir_src, hs.data(), total * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->mir_sign, hg.data(), total * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));                       // the host vectors go out of scope
  for (int t = 0; t < 3; ++t) h->tab[t] = MirTab{h->mir_src + off[t], h->mir_sign + off[t]};
  h->mirror = 1; h->use_aug = m->use_data_augmentation != 0; h->use_mloss = m->use_mirror_loss != 0; h->mirror_coeff = m->mirror_loss_coeff;
  return GO2SIM_E_OK;
}

int go2sim_ppo_symmetry_loss(go2sim_ppo_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_sym_loss, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_ppo_apply(go2sim_ppo_t* h, float* std_dev, void* stream) {
  if (!h || !std_dev) return GO2SIM_E_BADARG;
  AdamArgs a{};
  a.p_actor = h->actor->dparams; a.p_critic = h->critic->dparams; a.p_std = std_dev; a.nA = h->nA; a.nC = h->nC; a.A = h->A;
  if (h->rnn) { a.p_ma = h->mem[0]->dparams; a.p_mc = h->mem[1]->dparams; a.nMa = h->nM[0]; a.nMc = h->nM[1]; }
  a.max_norm = h->cfg.max_grad_norm; a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.eps;
  return h->rnn ? opt_apply<true>(h->opt, a, (hipStream_t)stream) : opt_apply<false>(h->opt, a, (hipStream_t)stream);
}

int go2sim_ppo_update(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, float* std_dev, const int32_t* perm, int n_rows_total, int n_epochs, int n_mini_batches, void* stream) {
  if (!h || h->rnn || !b || !std_dev || !perm || n_epochs < 1 || n_mini_batches < 1 || n_rows_total < n_mini_batches) return GO2SIM_E_BADARG;
  const int mbs = n_rows_total / n_mini_batches;
  if (mbs > h->max_rows) return GO2SIM_E_BADARG;
  int rc = go2sim_ppo_reset_stats(h, stream);
  for (int e = 0; e < n_epochs && rc == GO2SIM_E_OK; ++e)
    for (int i = 0; i < n_mini_batches && rc == GO2SIM_E_OK; ++i) {
      rc = go2sim_ppo_minibatch_grad(h, b, std_dev, perm + (size_t)i * mbs, mbs, stream);
      if (rc == GO2SIM_E_OK) rc = go2sim_ppo_apply(h, std_dev, stream);
    }
  return rc;
}

int go2sim_ppo_n_params(go2sim_ppo_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->n_flat;
  return GO2SIM_E_OK;
}
int go2sim_ppo_export(go2sim_ppo_t* h, int which, float* flat_dev, const float* std_dev, void* stream) {
  return pack_all(h, which, 0, flat_dev, const_cast<float*>(std_dev), (hipStream_t)stream);
}
int go2sim_ppo_import(go2sim_ppo_t* h, int which, const float* flat_dev, float* std_dev, void* stream) {
  return pack_all(h, which, 1, const_cast<float*>(flat_dev), std_dev, (hipStream_t)stream);
}
int go2sim_ppo_n_padded(go2sim_ppo_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->opt.n_tot;
  return GO2SIM_E_OK;
}
int go2sim_ppo_export_padded(go2sim_ppo_t* h, int which, float* padded_dev, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  return opt_export_padded(h->opt, opt_vec(h->opt, which), padded_dev, (hipStream_t)stream);
}

int go2sim_ppo_set_step(go2sim_ppo_t* h, long long step, double learning_rate, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  return opt_set_step(h->opt, step, learning_rate, (hipStream_t)stream);
}
int go2sim_ppo_reset_stats(go2sim_ppo_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_reset_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
int go2sim_ppo_stats(go2sim_ppo_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->opt.scal, (double)h->opt.step, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"

// ---- recurrent policy (include/go2sim_rnn.h) ------------------------------------------------------------------------------------------------------
namespace {
size_t lstm_flat_size(int I, int H) { return (size_t)4 * H * ((size_t)I + H + 2); }
// flat (weight_ih, weight_hh, bias_ih, bias_hh) <-> the zero-padded device layout, on the host
void lstm_pack(const go2sim_lstm* h, const float* flat, float* padded, bool to_padded) {
  const int I = h->I, H = h->H, Ip = h->dev.Ipad, Hp = h->dev.Hpad;
  float* pd[4] = {padded, padded + (size_t)4 * Hp * Ip, padded + (size_t)4 * Hp * Ip + (size_t)4 * Hp * Hp, padded + (size_t)4 * Hp * Ip + (size_t)4 * Hp * Hp + (size_t)4 * Hp};
  const size_t fo[4] = {0, (size_t)4 * H * I, (size_t)4 * H * I + (size_t)4 * H * H, (size_t)4 * H * I + (size_t)4 * H * H + (size_t)4 * H};
  const int cols[4] = {I, H, 1, 1}, ld[4] = {Ip, Hp, 1, 1};
  for (int m = 0; m < 4; ++m)
    for (int q = 0; q < 4; ++q)
      for (int j = 0; j < H; ++j) {
        float* p = pd[m] + ((size_t)q * Hp + j) * ld[m];
        float* f = const_cast<float*>(flat) + fo[m] + ((size_t)q * H + j) * cols[m];
        if (to_padded) memcpy(p, f, sizeof(float) * cols[m]);
        else memcpy(f, p, sizeof(float) * cols[m]);
      }
}
bool state_ok(const go2sim_ppo_rnn_state_t* s) { return s && s->h_a && s->c_a && s->h_c && s->c_c && s->dones; }

// The launches of one recurrent mini-batch: the env block [e0, e0 + nb) of a rollout of T x B rows; n = T nb rows, row t nb + j is batch row t B + e0 + j.
int launch_grad_rnn(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const go2sim_ppo_rnn_state_t* s, const float* std_dev, int B, int e0, int nb, hipStream_t st) {
  const go2sim_mlp *Ma = h->actor, *Mc = h->critic;
  const int T = h->T, n = T * nb;
  const float* x[2] = {b->obs, b->critic_obs};
  const float *h0[2] = {s->h_a, s->h_c}, *c0[2] = {s->c_a, s->c_c};
  int wmax = 1;                                            // column groups of the widest memory
  for (int net = 0; net < 2; ++net) { const int g = (h->mem[net]->dev.Hpad / 16 + NWAVE - 1) / NWAVE; if (g > wmax) wmax = g; }
  hipLaunchKernelGGL(k_rnn_idx, dim3((n + 255) / 256), dim3(256), 0, st, h->idx_b, n, nb, B, e0);
  for (int t = 0; t < T; ++t) {
    CellNet c[2];
    for (int net = 0; net < 2; ++net) {
      const go2sim_lstm* m = h->mem[net];
      const size_t H = m->H, Hp = m->dev.Hpad, o = (size_t)t * nb;
      CellNet& N = c[net];
      N.M = m->dev; N.x = x[net] + ((size_t)t * B + e0) * m->I; N.ldx = m->I;
      N.hin = t == 0 ? h0[net] + (size_t)e0 * H : h->r_hout[net] + (o - nb) * H;
      N.cin = t == 0 ? c0[net] + (size_t)e0 * H : h->r_cout[net] + (o - nb) * H;
      N.hout = h->r_hout[net] + o * H; N.cout = h->r_cout[net] + o * H;
      N.gates = h->r_gates[net] + o * 4 * Hp; N.hprev = h->r_hprev[net] + o * H; N.cprev = h->r_cprev[net] + o * H;
      N.active = 1;
    }
    hipLaunchKernelGGL(k_lstm_cell<true>, dim3((nb + TM - 1) / TM, wmax, 2), dim3(64 * NWAVE), 0, st, c[0], c[1],
                       t == 0 ? (const uint8_t*)nullptr : s->dones + (size_t)(t - 1) * B + e0, nb);
  }
  hipLaunchKernelGGL(k_train_forward<false>, dim3((n + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, Ma->dev, h->r_hout[0], h->mu, h->nw[0].a, Mc->dev, h->r_hout[1], h->val,
                     h->nw[1].a, h->idx_id, n, n, h->tab[0], h->tab[1]);
  const int n_wg = (n + WGT - 1) / WGT, ncol = 3 + h->A;
  const HeadArgs ha = head_args(h, b, std_dev, h->idx_b, n, n, 1.0 / (double)n);
  hipLaunchKernelGGL(k_ppo_head<false>, dim3(n_wg), dim3(WGT), 0, st, ha);
  hipLaunchKernelGGL(k_ppo_finalize, dim3(1), dim3(64), 0, st, h->head_part, n_wg, ncol, n, n, h->A, std_dev, h->opt.scal, h->opt.grads + h->slab, h->cfg.entropy_coef,
                     h->cfg.desired_kl, h->cfg.lr_min, h->cfg.lr_max, h->cfg.adaptive);
  const int n_chunks = (n + RCH - 1) / RCH;
  const size_t slab = h->slab;
  const int depth = Ma->n_layers > Mc->n_layers ? Ma->n_layers : Mc->n_layers;
  BwdLayer L[MAXL][2];
  for (int lb = 0; lb < depth; ++lb)
    for (int net = 0; net < 2; ++net) {
      BwdLayer& Q = L[lb][net];
      Q = bwd_layer(h, net, lb, b);
      if (!Q.active || (net == 0 ? Ma : Mc)->n_layers - 1 - lb != 0) continue;
      // the first layer reads the memory's h' [n][H] and hands d loss / d h' back
      Q.aprev = h->r_hout[net]; Q.gather = 0; Q.dzprev = h->r_dh[net]; Q.lin = 1;
    }
  launch_backward<false, true>(L, depth, BwdRun{2, h->idx_id, n, n, h->partial, slab, st});
  for (int t = T - 1; t >= 0; --t) {
    BpttNet c[2];
    for (int net = 0; net < 2; ++net) {
      const go2sim_lstm* m = h->mem[net];
      const size_t H = m->H, Hp = m->dev.Hpad, o = (size_t)t * nb;
      BpttNet& N = c[net];
      N.M = m->dev; N.dz_next = h->r_dz[net] + (o + nb) * 4 * Hp; N.dh_mlp = h->r_dh[net] + o * Hp; N.gates = h->r_gates[net] + o * 4 * Hp;
      N.cprev = h->r_cprev[net] + o * H; N.cout = h->r_cout[net] + o * H; N.dc = h->r_dc[net]; N.dz = h->r_dz[net] + o * 4 * Hp; N.active = 1;
    }
    hipLaunchKernelGGL(k_lstm_bptt, dim3((nb + TM - 1) / TM, wmax, 2), dim3(64 * NWAVE), 0, st, c[0], c[1], s->dones + (size_t)t * B + e0, t < T - 1 ? 1 : 0, nb);
  }
  // the memories' weight gradients over all n rows: dW_ih = dz^T x (rows through idx_b), dW_hh = dz^T h_prev, db_ih = db_hh = column sums of dz
  for (int part = 0; part < 2; ++part) {
    BwdLayer L[2];
    for (int net = 0; net < 2; ++net) {
      const go2sim_lstm* m = h->mem[net];
      const int Hp = m->dev.Hpad, Ip = m->dev.Ipad;
      const size_t off = h->nA + h->nC + (net == 0 ? 0 : h->nM[0]), o_hh = (size_t)4 * Hp * Ip, o_bi = o_hh + (size_t)4 * Hp * Hp;
      BwdLayer& Q = L[net];
      Q = BwdLayer{};
      Q.active = 1; Q.dz = h->r_dz[net]; Q.N = 4 * Hp;
      if (part == 0) { Q.aprev = x[net]; Q.K = Ip; Q.lda = m->I; Q.kmax = m->I; Q.gather = 1; Q.W = m->dev.Wih; Q.w_off = off; Q.b_off = off + o_bi; }
      else { Q.aprev = h->r_hprev[net]; Q.K = Hp; Q.lda = m->H; Q.kmax = m->H; Q.gather = 0; Q.W = m->dev.Whh; Q.w_off = off + o_hh; Q.b_off = off + o_bi + (size_t)4 * Hp; }
    }
    launch_dw_db<false>(L[0], L[1], BwdRun{2, h->idx_b, n, n, h->partial, slab, st});
  }
  hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)((slab + WGT - 1) / WGT)), dim3(WGT), 0, st, h->partial, n_chunks, slab, h->opt.grads);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
}  // namespace

extern "C" {

int go2sim_lstm_create(int device, int n_in, int n_hidden, const float* params, size_t n_params, go2sim_lstm_t** out) {
  if (!params || !out || n_in < 1 || n_in > MAXW || n_hidden < 1 || n_hidden > MAXW || n_params != lstm_flat_size(n_in, n_hidden)) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(device));
  go2sim_lstm* h = new (std::nothrow) go2sim_lstm();
  if (!h) return GO2SIM_E_NOMEM;
  h->device = device; h->I = n_in; h->H = n_hidden; h->n_params = n_params;
  const int Ip = round16(n_in), Hp = round16(n_hidden);
  h->padded = (size_t)4 * Hp * ((size_t)Ip + Hp + 2);
  if (hipMalloc((void**)&h->dparams, h->padded * sizeof(float)) != hipSuccess) { delete h; return GO2SIM_E_NOMEM; }
  h->dev.I = n_in; h->dev.H = n_hidden; h->dev.Ipad = Ip; h->dev.Hpad = Hp;
  h->dev.Wih = h->dparams; h->dev.Whh = h->dev.Wih + (size_t)4 * Hp * Ip; h->dev.bih = h->dev.Whh + (size_t)4 * Hp * Hp; h->dev.bhh = h->dev.bih + (size_t)4 * Hp;
  const int rc = go2sim_lstm_set_params(h, params, n_params, nullptr);
  if (rc != GO2SIM_E_OK) { (void)hipFree(h->dparams); delete h; return rc; }
  HIPCHK(hipDeviceSynchronize());
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_lstm_destroy(go2sim_lstm_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  (void)hipFree(h->dparams);
  delete h;
  return GO2SIM_E_OK;
}

int go2sim_lstm_set_params(go2sim_lstm_t* h, const float* params, size_t n_params, void* stream) {
  if (!h || !params || n_params != h->n_params) return GO2SIM_E_BADARG;
  std::vector<float> packed(h->padded, 0.0f);
  lstm_pack(h, params, packed.data(), true);
  HIPCHK(hipMemcpyAsync(h->dparams, packed.data(), h->padded * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));      // `packed` is a temporary
  return GO2SIM_E_OK;
}

int go2sim_lstm_get_params(go2sim_lstm_t* h, float* params, size_t n_params, void* stream) {
  if (!h || !params || n_params != h->n_params) return GO2SIM_E_BADARG;
  std::vector<float> packed(h->padded);
  HIPCHK(hipMemcpyAsync(packed.data(), h->dparams, h->padded * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  lstm_pack(h, params, packed.data(), false);
  return GO2SIM_E_OK;
}

int go2sim_lstm_step(go2sim_lstm_t* mem_a, const float* x_a, const float* h_in_a, const float* c_in_a, float* h_out_a, float* c_out_a, go2sim_lstm_t* mem_c,
                     const float* x_c, const float* h_in_c, const float* c_in_c, float* h_out_c, float* c_out_c, const uint8_t* reset, int n_rows, void* stream) {
  if (!mem_a || !x_a || !h_in_a || !c_in_a || !h_out_a || !c_out_a || h_out_a == h_in_a || n_rows < 0) return GO2SIM_E_BADARG;
  if (mem_c && (!x_c || !h_in_c || !c_in_c || !h_out_c || !c_out_c || h_out_c == h_in_c)) return GO2SIM_E_BADARG;
  if (n_rows == 0) return GO2SIM_E_OK;
  CellNet c[2] = {};
  c[0].M = mem_a->dev; c[0].x = x_a; c[0].ldx = mem_a->I; c[0].hin = h_in_a; c[0].cin = c_in_a; c[0].hout = h_out_a; c[0].cout = c_out_a; c[0].active = 1;
  int groups = (mem_a->dev.Hpad / 16 + NWAVE - 1) / NWAVE;
  if (mem_c) {
    c[1].M = mem_c->dev; c[1].x = x_c; c[1].ldx = mem_c->I; c[1].hin = h_in_c; c[1].cin = c_in_c; c[1].hout = h_out_c; c[1].cout = c_out_c; c[1].active = 1;
    const int g = (mem_c->dev.Hpad / 16 + NWAVE - 1) / NWAVE;
    if (g > groups) groups = g;
  }
  hipLaunchKernelGGL(k_lstm_cell<false>, dim3((n_rows + TM - 1) / TM, groups, mem_c ? 2 : 1), dim3(64 * NWAVE), 0, (hipStream_t)stream, c[0], c[1], reset, n_rows);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_ppo_rnn_minibatch_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const go2sim_ppo_rnn_state_t* s, const float* std_dev, int n_envs, int env0, int n_block,
                                  void* stream) {
  if (!h || !h->rnn || !std_dev || !batch_ok(b) || !state_ok(s)) return GO2SIM_E_BADARG;
  if (n_block < 1 || n_block > h->nb_max || env0 < 0 || n_envs < 1 || env0 > n_envs - n_block || (long long)h->T * n_envs > 0x7fffffffLL / MAXW) return GO2SIM_E_BADARG;
  return launch_grad_rnn(h, b, s, std_dev, n_envs, env0, n_block, (hipStream_t)stream);
}

int go2sim_ppo_rnn_update(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const go2sim_ppo_rnn_state_t* s, float* std_dev, int n_envs, int n_epochs, int n_mini_batches,
                          void* stream) {
  if (!h || !h->rnn || !std_dev || !batch_ok(b) || !state_ok(s) || n_epochs < 1 || n_mini_batches < 1 || n_envs < n_mini_batches || n_envs % n_mini_batches) return GO2SIM_E_BADARG;
  const int nb = n_envs / n_mini_batches;
  if (nb > h->nb_max || (long long)h->T * n_envs > 0x7fffffffLL / MAXW) return GO2SIM_E_BADARG;
  int rc = go2sim_ppo_reset_stats(h, stream);
  for (int e = 0; e < n_epochs && rc == GO2SIM_E_OK; ++e)
    for (int i = 0; i < n_mini_batches && rc == GO2SIM_E_OK; ++i) {
      rc = go2sim_ppo_rnn_minibatch_grad(h, b, s, std_dev, n_envs, i * nb, nb, stream);
      if (rc == GO2SIM_E_OK) rc = go2sim_ppo_apply(h, std_dev, stream);
    }
  return rc;
}

}  // extern "C"
