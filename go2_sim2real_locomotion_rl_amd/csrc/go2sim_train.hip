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
//     k_bwd_da        dZ_prev = (dZ W) * ELU'(A_prev), 32 rows per workgroup, 4 accumulators per wavefront.  W is read strided ([npad][kpad], the
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
#include "../../include/go2sim_train.h"

namespace {

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "go2sim_train: %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

constexpr int RCH = GO2SIM_PPO_ROW_CHUNK, WGT = 256, NORM_WG = 256;
constexpr int DW_TN = 2, DW_TK = 4;                       // output tiles of a k_bwd_dw workgroup: 32 rows of dW (n) x 64 columns (k)
enum { S_LR = 0, S_KL, S_SUM_VL, S_SUM_SUR, S_SUM_ENT, S_COUNT, S_NORM, S_SUM_SYM, S_N };

struct ActWs { float* a[MAXL]; };                        // post-activations of the hidden layers, [rows][npad[l]]
// one signed permutation (M x)[j] = sign[j] x[src[j]], device tables owned by the handle
struct MirTab { const int32_t* src; const float* sign; };

// a workgroup's sum of one float64 per lane in a fixed order (pairwise tree), valid on every lane
__device__ __forceinline__ double wg_sum(double* s, double v) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int k = WGT / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
    __syncthreads();
  }
  return s[0];
}

// MIR: rows [n_orig, B) are the mirrors of rows [0, B - n_orig): row idx[gr - n_orig] read through the network's input table (t0 actor, t1 critic)
template <bool MIR>
__global__ __launch_bounds__(64 * NWAVE) void k_train_forward(MlpDev M0, const float* __restrict__ x0, float* __restrict__ y0, ActWs w0,
                                                              MlpDev M1, const float* __restrict__ x1, float* __restrict__ y1, ActWs w1,
                                                              const int32_t* __restrict__ idx, int B, int n_orig, MirTab t0, MirTab t1) {
  __shared__ alignas(16) float act[2][TM][LDW];
  __shared__ int32_t s_src[MIR ? MAXW : 1];
  __shared__ float s_sign[MIR ? MAXW : 1];
  const MlpDev& M = blockIdx.y == 0 ? M0 : M1;
  const ActWs& ws = blockIdx.y == 0 ? w0 : w1;
  const float* __restrict__ x = blockIdx.y == 0 ? x0 : x1;
  float* __restrict__ y = blockIdx.y == 0 ? y0 : y1;
  const int row0 = blockIdx.x * TM;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (MIR && row0 + TM > n_orig) {                         // this workgroup holds mirrored rows: the table goes to LDS once
    const MirTab& t = blockIdx.y == 0 ? t0 : t1;
    const int d0 = M.din[0];
    for (int k = tid; k < d0; k += 64 * NWAVE) { s_src[k] = t.src[k]; s_sign[k] = t.sign[k]; }
    __syncthreads();
  }
  {
    const int K0 = M.kpad[0], d0 = M.din[0];
    for (int i = tid; i < TM * K0; i += 64 * NWAVE) {
      int r = i / K0, k = i - r * K0, gr = row0 + r;
      float v = 0.0f;
      if (gr < B && k < d0) {
        if (MIR && gr >= n_orig) v = s_sign[k] * x[(size_t)idx[gr - n_orig] * d0 + s_src[k]];
        else v = x[(size_t)idx[gr] * d0 + k];
      }
      act[0][r][k] = v;
    }
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < M.n_layers; ++l) {
    const int tiles_per_wave = (M.npad[l] / 16 + NWAVE - 1) / NWAVE;
    if (tiles_per_wave >= 4) mlp_layer<4>(M, l, act[cur], act[cur ^ 1], y, row0, B, wave, lane);
    else if (tiles_per_wave >= 2) mlp_layer<2>(M, l, act[cur], act[cur ^ 1], y, row0, B, wave, lane);
    else mlp_layer<1>(M, l, act[cur], act[cur ^ 1], y, row0, B, wave, lane);
    __syncthreads();
    cur ^= 1;
    if (l < M.n_layers - 1) {                              // the next layer only reads this buffer: no barrier needed after the copy
      const int N = M.npad[l];
      float* __restrict__ dst = ws.a[l];
      for (int i = tid; i < TM * N; i += 64 * NWAVE) {
        int r = i / N, n = i - r * N, gr = row0 + r;
        if (gr < B) dst[(size_t)gr * N + n] = act[cur][r][n];
      }
    }
  }
}

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

// one layer of one network as the backward kernels see it
struct BwdLayer {
  const float* dz;      // [rows][N]  d loss / d pre-activation of this layer
  const float* aprev;   // [rows][lda] input of this layer: the previous layer's post-activation (lda = K), or the observations (lda = din, rows through idx)
  const float* W;       // [N][K]
  float* dzprev;        // [rows][K], written by k_bwd_da (hidden layers only)
  int N, K, lda, kmax;  // kmax: columns of aprev that exist (din for the input layer, K otherwise)
  int gather;           // aprev rows are read through idx
  MirTab mir;           // gather layers under a mirror: rows >= n_orig read row idx[r - n_orig] through this table
  int active;           // this network has this layer
  size_t w_off, b_off;  // offsets of dW / db in a slab of partials (= in the padded gradient vector)
};

template <bool MIR>
__global__ __launch_bounds__(WGT) void k_bwd_dw(BwdLayer L0, BwdLayer L1, const int32_t* __restrict__ idx, int n_rows, int n_orig, float* __restrict__ partial,
                                                size_t slab) {
  __shared__ float red[NWAVE][DW_TN * DW_TK * 4][64];
  const BwdLayer& L = blockIdx.z == 0 ? L0 : L1;
  if (!L.active) return;
  const int ntn = L.N / 16, ntk = L.K / 16, gk_n = (ntk + DW_TK - 1) / DW_TK, gn_n = (ntn + DW_TN - 1) / DW_TN;
  if ((int)blockIdx.x >= gk_n * gn_n) return;
  const int gn = blockIdx.x / gk_n, gk = blockIdx.x - gn * gk_n, c = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  int ncol[DW_TN], kcol[DW_TK];
#pragma unroll
  for (int t = 0; t < DW_TN; ++t) { int nt = gn * DW_TN + t; if (nt >= ntn) nt = ntn - 1; ncol[t] = nt * 16 + col; }
#pragma unroll
  for (int t = 0; t < DW_TK; ++t) { int kt = gk * DW_TK + t; if (kt >= ntk) kt = ntk - 1; kcol[t] = kt * 16 + col; }
  f32x4 acc[DW_TN][DW_TK];
#pragma unroll
  for (int a = 0; a < DW_TN; ++a)
#pragma unroll
    for (int b = 0; b < DW_TK; ++b) acc[a][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int rbeg = c * RCH + wave * (RCH / NWAVE);
  int rend = rbeg + RCH / NWAVE;
  if (rend > n_rows) rend = n_rows;
  const gcfp dz = (gcfp)L.dz;
  const gcfp ap = (gcfp)L.aprev;
  int msrc[DW_TK];                                         // this lane's columns of the mirror table, read once
  float msign[DW_TK];
  const bool mir_layer = MIR && L.gather;
  if (MIR) {
#pragma unroll
    for (int t = 0; t < DW_TK; ++t) {
      const bool kon = mir_layer && kcol[t] < L.kmax;
      msrc[t] = kon ? L.mir.src[kcol[t]] : kcol[t];
      msign[t] = kon ? L.mir.sign[kcol[t]] : 1.0f;
    }
  }
  for (int r0 = rbeg; r0 < rend; r0 += 4) {                // reduction index of the matrix instruction: row r0 + (lane >> 4)
    const int r = r0 + kq;
    const bool ron = r < rend;
    const bool rmir = mir_layer && r >= n_orig;
    const size_t rs = ron ? (L.gather ? (size_t)idx[rmir ? r - n_orig : r] : (size_t)r) : 0;
    float av[DW_TN], bv[DW_TK];
#pragma unroll
    for (int t = 0; t < DW_TN; ++t) av[t] = ron ? dz[(size_t)r * L.N + ncol[t]] : 0.0f;
#pragma unroll
    for (int t = 0; t < DW_TK; ++t) {
      if (MIR) {
        const float v = (ron && kcol[t] < L.kmax) ? ap[rs * L.lda + (rmir ? msrc[t] : kcol[t])] : 0.0f;
        bv[t] = rmir ? msign[t] * v : v;
      } else {
        bv[t] = (ron && kcol[t] < L.kmax) ? ap[rs * L.lda + kcol[t]] : 0.0f;
      }
    }
#pragma unroll
    for (int a = 0; a < DW_TN; ++a)
#pragma unroll
      for (int b = 0; b < DW_TK; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < DW_TN; ++a)
#pragma unroll
    for (int b = 0; b < DW_TK; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave][(a * DW_TK + b) * 4 + i][lane] = acc[a][b][i];
  __syncthreads();
  float* __restrict__ out = partial + (size_t)c * slab + L.w_off;
  for (int e = tid; e < DW_TN * DW_TK * 4 * 64; e += WGT) {
    const int q = e >> 6, ln = e & 63, t = q >> 2, i = q & 3, a = t / DW_TK, b = t - a * DW_TK;
    const int nt = gn * DW_TN + a, kt = gk * DW_TK + b;
    if (nt >= ntn || kt >= ntk) continue;
    const float s = ((red[0][q][ln] + red[1][q][ln]) + red[2][q][ln]) + red[3][q][ln];
    const int nrow = nt * 16 + 4 * (ln >> 4) + i, kc = kt * 16 + (ln & 15);   // accumulator element i: row 4 * (lane >> 4) + i, column lane & 15
    out[(size_t)nrow * L.K + kc] = s;
  }
}

// db of one chunk: a workgroup owns 16 columns; lane (slice, column) adds the 32 rows of its slice in float64, the 16 slices are added in slice order
__global__ __launch_bounds__(WGT) void k_bwd_db(BwdLayer L0, BwdLayer L1, int n_rows, float* __restrict__ partial, size_t slab) {
  __shared__ double s_part[16][16];
  const BwdLayer& L = blockIdx.z == 0 ? L0 : L1;
  if (!L.active || (int)blockIdx.x * 16 >= L.N) return;
  const int col = threadIdx.x & 15, slice = threadIdx.x >> 4, ncol = blockIdx.x * 16 + col, c = blockIdx.y;
  constexpr int SL = RCH / 16;
  const int rbeg = c * RCH + slice * SL;
  int rend = rbeg + SL;
  if (rend > n_rows) rend = n_rows;
  double s = 0.0;
  for (int r = rbeg; r < rend; ++r) s += (double)L.dz[(size_t)r * L.N + ncol];
  s_part[slice][col] = s;
  __syncthreads();
  if (slice == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += s_part[k][col];
    partial[(size_t)c * slab + L.b_off + ncol] = (float)t;
  }
}

// dZ_prev[r][k] = (sum_n dZ[r][n] W[n][k]) * ELU'(A_prev[r][k]); ELU' from the stored post-activation a: 1 for a > 0, a + 1 otherwise
__global__ __launch_bounds__(64 * NWAVE) void k_bwd_da(BwdLayer L0, BwdLayer L1, int n_rows) {
  constexpr int TG = 2;
  const BwdLayer& L = blockIdx.y == 0 ? L0 : L1;
  if (!L.active) return;
  const int row0 = blockIdx.x * TM, N = L.N, K = L.K, ktiles = K / 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  const gcfp W = (gcfp)L.W;
  const gcfp dz = (gcfp)L.dz;
  bool ron[RT];
  size_t roff[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) { const int r = row0 + 16 * rt + col; ron[rt] = r < n_rows; roff[rt] = ron[rt] ? (size_t)r * N + 4 * kq : 0; }
  for (int g0 = wave * TG; g0 < ktiles; g0 += NWAVE * TG) {
    f32x4 acc[RT][TG];
    int kc[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const int kt = (g0 + t < ktiles) ? g0 + t : ktiles - 1;
      kc[t] = kt * 16 + col;
    }
    for (int j = 0; j < N; j += 16) {                      // reduction index: n = j + 4 (lane >> 4) + s
      f32x4 av[RT];
      float wv[TG][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) av[rt] = ron[rt] ? *(gcf4p)(dz + roff[rt] + j) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < TG; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) wv[t][s] = W[(size_t)(j + 4 * kq + s) * K + kc[t]];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][s], wv[t][s], acc[rt][t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      if (g0 + t >= ktiles) break;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = row0 + 16 * rt + 4 * kq + i;
          if (r < n_rows) {
            const float a = L.aprev[(size_t)r * K + kc[t]];
            L.dzprev[(size_t)r * K + kc[t]] = acc[rt][t][i] * (a > 0.0f ? 1.0f : a + 1.0f);
          }
        }
    }
  }
}

__global__ __launch_bounds__(WGT) void k_reduce_partials(const float* __restrict__ partial, int n_chunks, size_t slab, float* __restrict__ grads) {
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= slab) return;
  double s = 0.0;
  for (int c = 0; c < n_chunks; ++c) s += (double)partial[(size_t)c * slab + i];
  grads[i] = (float)s;
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

__global__ __launch_bounds__(WGT) void k_sumsq(const float* __restrict__ g, size_t n, double* __restrict__ part) {
  __shared__ double s_red[WGT];
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * WGT + threadIdx.x; i < n; i += (size_t)NORM_WG * WGT) s += (double)g[i] * (double)g[i];
  const double t = wg_sum(s_red, s);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

struct AdamArgs {
  float *p_actor, *p_critic, *p_std, *g, *m, *v;
  size_t nA, nC, n_tot;                                   // padded sizes; the std block follows the two networks
  int A;
  const double* sq_part;
  double* scal;
  double max_norm, b1, b2, eps, bc1, bc2_sqrt;            // bc1 = 1 - b1^t, bc2_sqrt = sqrt(1 - b2^t), from the step count in float64 on the host
};

__global__ __launch_bounds__(WGT) void k_adam(AdamArgs a) {
  __shared__ double s_coef;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < NORM_WG; ++i) s += a.sq_part[i];   // every workgroup adds in the same order: the same bits everywhere
    const double norm = sqrt(s);
    double coef = a.max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
    s_coef = coef;
    if (blockIdx.x == 0) a.scal[S_NORM] = norm;
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= a.n_tot) return;
  float* p;
  if (i < a.nA) p = a.p_actor + i;
  else if (i < a.nA + a.nC) p = a.p_critic + (i - a.nA);
  else { const size_t k = i - a.nA - a.nC; if (k >= (size_t)a.A) return; p = a.p_std + k; }
  const double g = (double)a.g[i] * s_coef;
  const double m = a.b1 * (double)a.m[i] + (1.0 - a.b1) * g;
  const double v = a.b2 * (double)a.v[i] + (1.0 - a.b2) * (g * g);
  a.g[i] = (float)g; a.m[i] = (float)m; a.v[i] = (float)v;
  const double step_size = a.scal[S_LR] / a.bc1;
  *p = (float)((double)*p - step_size * (m / (sqrt(v) / a.bc2_sqrt + a.eps)));
}

// flat [rows][cols] <-> padded [rows][ld]
__global__ __launch_bounds__(WGT) void k_pack(int to_padded, float* __restrict__ padded, int ld, float* __restrict__ flat, int rows, int cols) {
  const int i = blockIdx.x * WGT + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i - r * cols;
  if (to_padded) padded[(size_t)r * ld + c] = flat[i];
  else flat[i] = padded[(size_t)r * ld + c];
}
__global__ void k_set_lr(double* scal, double lr) { if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_LR] = lr; }
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

struct Seg { int base; size_t pad_off; int ld, rows, cols; size_t flat_off; };   // base 0 actor, 1 critic, 2 std

}  // namespace

struct go2sim_ppo {
  go2sim_mlp *actor = nullptr, *critic = nullptr;
  go2sim_ppo_cfg_t cfg{};
  int A = 0, Apad = 0, max_rows = 0, max_chunks = 0, max_head_wg = 0;
  size_t nA = 0, nC = 0, n_tot = 0, n_flat = 0;
  float* fbuf = nullptr;      // the optimizer's vectors: grads | m | v
  float* wbuf = nullptr;      // the workspaces of ws_rows rows: mu | val | activations | dz ping-pong | partial slabs
  float *grads = nullptr, *m = nullptr, *v = nullptr, *mu = nullptr, *val = nullptr, *partial = nullptr;
  ActWs ws[2]{};
  float* dz[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  double* dbuf = nullptr;     // scal[S_N] | sq_part[NORM_WG]
  double* hbuf = nullptr;     // head partials, [workgroups of ws_rows][4 + A]
  double *scal = nullptr, *sq_part = nullptr, *head_part = nullptr;
  size_t ws_rows = 0;         // max_rows, twice that once a mirror has been set
  long long step = 0;
  std::vector<Seg> segs;
  // mirror symmetry (go2sim_ppo_set_mirror): the tables live in one device allocation each, obs | critic obs | actions
  int mirror = 0, use_aug = 0, use_mloss = 0;
  double mirror_coeff = 0.0;
  int32_t* mir_src = nullptr;
  float* mir_sign = nullptr;
  MirTab tab[3]{};            // 0 actor input, 1 critic input, 2 actions
};

namespace {
BwdLayer bwd_layer(const go2sim_ppo* h, int net, int lb, const go2sim_ppo_batch_t* batch) {
  const go2sim_mlp* M = net == 0 ? h->actor : h->critic;
  BwdLayer L{};
  const int l = M->n_layers - 1 - lb;                      // lb counts from the last layer
  if (l < 0) return L;
  L.active = 1;
  L.N = M->dev.npad[l]; L.K = M->dev.kpad[l];
  L.dz = h->dz[net][l & 1];
  L.W = M->dev.W[l];
  if (l == 0) {
    L.aprev = net == 0 ? batch->obs : batch->critic_obs; L.lda = M->dims[0]; L.kmax = M->dims[0]; L.gather = 1; L.dzprev = nullptr;
    L.mir = h->tab[net];
  } else {
    L.aprev = h->ws[net].a[l - 1]; L.lda = L.K; L.kmax = L.K; L.gather = 0; L.dzprev = h->dz[net][(l - 1) & 1];
  }
  L.w_off = (size_t)(M->dev.W[l] - M->dparams) + (net == 0 ? 0 : h->nA);
  L.b_off = (size_t)(M->dev.b[l] - M->dparams) + (net == 0 ? 0 : h->nA);
  return L;
}
// (re)allocates the row workspaces for R rows; the optimizer's vectors and the scalars are not touched.  hipFree waits for the device.
int alloc_workspaces(go2sim_ppo* h, size_t R) {
  const go2sim_mlp* nets[2] = {h->actor, h->critic};
  auto al16 = [](size_t n) { return (n + 15) / 16 * 16; };   // every region starts 64-byte aligned (float4 loads)
  size_t need = al16(R * h->A) + al16(R);
  size_t dz_sz[2] = {0, 0};
  for (int net = 0; net < 2; ++net) {
    const go2sim_mlp* M = nets[net];
    int wmax = 16;
    for (int l = 0; l < M->n_layers; ++l) { if (l < M->n_layers - 1) need += R * M->dev.npad[l]; if (M->dev.npad[l] > wmax) wmax = M->dev.npad[l]; }
    dz_sz[net] = R * wmax;
    need += 2 * dz_sz[net];
  }
  const int chunks = (int)((R + RCH - 1) / RCH), head_wg = (int)((R + WGT - 1) / WGT);
  const size_t slab = h->nA + h->nC;
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
  for (int net = 0; net < 2; ++net) {
    const go2sim_mlp* M = nets[net];
    for (int l = 0; l < M->n_layers - 1; ++l) { h->ws[net].a[l] = p; p += R * M->dev.npad[l]; }
    h->dz[net][0] = p; p += dz_sz[net]; h->dz[net][1] = p; p += dz_sz[net];
  }
  h->partial = p;
  return GO2SIM_E_OK;
}
float* vec_of(go2sim_ppo* h, int which) {
  return which == GO2SIM_PPO_GRADS ? h->grads : which == GO2SIM_PPO_ADAM_M ? h->m : which == GO2SIM_PPO_ADAM_V ? h->v : nullptr;
}
int pack_all(go2sim_ppo* h, int which, int to_padded, float* flat, float* std_dev, hipStream_t st) {
  if (!h || !flat || which < GO2SIM_PPO_PARAMS || which > GO2SIM_PPO_ADAM_V) return GO2SIM_E_BADARG;
  if (which == GO2SIM_PPO_PARAMS && !std_dev) return GO2SIM_E_BADARG;
  float* base[3];
  if (which == GO2SIM_PPO_PARAMS) { base[0] = h->actor->dparams; base[1] = h->critic->dparams; base[2] = std_dev; }
  else { float* v = vec_of(h, which); base[0] = v; base[1] = v + h->nA; base[2] = v + h->nA + h->nC; }
  for (const Seg& s : h->segs)
    hipLaunchKernelGGL(k_pack, dim3((s.rows * s.cols + WGT - 1) / WGT), dim3(WGT), 0, st, to_padded, base[s.base] + s.pad_off, s.ld, flat + s.flat_off, s.rows, s.cols);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
}  // namespace

extern "C" {

int go2sim_ppo_create(go2sim_mlp_t* actor, go2sim_mlp_t* critic, int n_actions, const go2sim_ppo_cfg_t* cfg, int max_rows, go2sim_ppo_t** out) {
  if (!actor || !critic || !cfg || !out || max_rows < 1 || n_actions < 1) return GO2SIM_E_BADARG;
  if (actor->dims[actor->n_layers] != n_actions || critic->dims[critic->n_layers] != 1 || actor->device != critic->device) return GO2SIM_E_BADARG;
  if (!(cfg->learning_rate > 0.0) || !(cfg->clip_param >= 0.0)) return GO2SIM_E_BADARG;
  HIPCHK(hipSetDevice(actor->device));
  go2sim_ppo* h = new (std::nothrow) go2sim_ppo();
  if (!h) return GO2SIM_E_NOMEM;
  h->actor = actor; h->critic = critic; h->cfg = *cfg; h->A = n_actions; h->Apad = round16(n_actions); h->max_rows = max_rows;
  h->nA = actor->padded; h->nC = critic->padded; h->n_tot = h->nA + h->nC + h->Apad;
  // flat (state-dict) order: actor W0, b0, ..., critic W0, b0, ..., std
  size_t flat = 0;
  for (int net = 0; net < 2; ++net) {
    const go2sim_mlp* M = net == 0 ? actor : critic;
    for (int l = 0; l < M->n_layers; ++l) {
      h->segs.push_back(Seg{net, (size_t)(M->dev.W[l] - M->dparams), M->dev.kpad[l], M->dims[l + 1], M->dims[l], flat}); flat += (size_t)M->dims[l] * M->dims[l + 1];
      h->segs.push_back(Seg{net, (size_t)(M->dev.b[l] - M->dparams), M->dims[l + 1], 1, M->dims[l + 1], flat}); flat += M->dims[l + 1];
    }
  }
  h->segs.push_back(Seg{2, 0, n_actions, 1, n_actions, flat}); flat += n_actions;
  h->n_flat = flat;
  const size_t nd = S_N + NORM_WG;
  if (hipMalloc((void**)&h->fbuf, 3 * h->n_tot * sizeof(float)) != hipSuccess || hipMalloc((void**)&h->dbuf, nd * sizeof(double)) != hipSuccess) {
    go2sim_ppo_destroy(h);
    return GO2SIM_E_NOMEM;
  }
  if (hipMemset(h->fbuf, 0, 3 * h->n_tot * sizeof(float)) != hipSuccess || hipMemset(h->dbuf, 0, nd * sizeof(double)) != hipSuccess ||
      hipMemcpy(h->dbuf + S_LR, &cfg->learning_rate, sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fprintf(stderr, "go2sim_train: initialising the optimizer state failed: %s\n", hipGetErrorString(hipGetLastError()));
    go2sim_ppo_destroy(h);
    return GO2SIM_E_HIP;
  }
  h->grads = h->fbuf; h->m = h->grads + h->n_tot; h->v = h->m + h->n_tot;
  h->scal = h->dbuf; h->sq_part = h->dbuf + S_N;
  const int rc = alloc_workspaces(h, (size_t)max_rows);
  if (rc != GO2SIM_E_OK) {
    go2sim_ppo_destroy(h);
    return rc;
  }
  *out = h;
  return GO2SIM_E_OK;
}

int go2sim_ppo_destroy(go2sim_ppo_t* h) {
  if (!h) return GO2SIM_E_BADARG;
  if (h->fbuf) (void)hipFree(h->fbuf);
  if (h->wbuf) (void)hipFree(h->wbuf);
  if (h->dbuf) (void)hipFree(h->dbuf);
  if (h->hbuf) (void)hipFree(h->hbuf);
  if (h->mir_src) (void)hipFree(h->mir_src);
  if (h->mir_sign) (void)hipFree(h->mir_sign);
  delete h;
  return GO2SIM_E_OK;
}

}  // extern "C"

// The launches of one mini-batch.  record == nullptr: the rows are the whole mini-batch (k_ppo_finalize, k_reduce_partials); otherwise they are a shard of it
// and the sums stay in float64 in `record`.  w: 1 / (rows of the mini-batch over all shards).  With a mirror the forward and the head run over 2 n rows
// (the mirror loss is always reported), the backward too unless both flags are off: then no mirrored row carries a gradient.
template <bool MIR>
static int launch_grad_t(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, double w, double* record, hipStream_t st) {
  const go2sim_mlp *Ma = h->actor, *Mc = h->critic;
  const int n_fwd = MIR ? 2 * n : n, n_bwd = (MIR && (h->use_aug || h->use_mloss)) ? 2 * n : n;
  const int ncol = (MIR ? 4 : 3) + h->A;
  hipLaunchKernelGGL(k_train_forward<MIR>, dim3((n_fwd + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, Ma->dev, b->obs, h->mu, h->ws[0], Mc->dev, b->critic_obs, h->val,
                     h->ws[1], idx, n_fwd, n, h->tab[0], h->tab[1]);
  const int n_wg = (n_fwd + WGT - 1) / WGT;
  HeadArgs ha{};
  ha.mu = h->mu; ha.val = h->val; ha.b = *b; ha.std_ = std_dev; ha.idx = idx;
  ha.dz_actor = h->dz[0][(Ma->n_layers - 1) & 1]; ha.dz_critic = h->dz[1][(Mc->n_layers - 1) & 1];
  ha.part = h->head_part; ha.n = n; ha.A = h->A; ha.Apad = h->Apad; ha.use_clipped = h->cfg.use_clipped_value_loss;
  ha.clip = h->cfg.clip_param; ha.vl_coef = h->cfg.value_loss_coef;
  ha.w = (MIR && h->use_aug) ? 0.5 * w : w;                // 1 / (2 n): halving is exact
  ha.n_rows = n_fwd; ha.ppo_on_mirrors = MIR && h->use_aug; ha.use_mirror_loss = MIR && h->use_mloss; ha.ta = h->tab[2];
  ha.w_sym = h->mirror_coeff * 2.0 * w / (double)h->A;
  hipLaunchKernelGGL(k_ppo_head<MIR>, dim3(n_wg), dim3(WGT), 0, st, ha);
  if (!record)
    hipLaunchKernelGGL(k_ppo_finalize, dim3(1), dim3(64), 0, st, h->head_part, n_wg, ncol, n, (MIR && h->use_aug) ? 2 * n : n, h->A, std_dev, h->scal,
                       h->grads + h->nA + h->nC, h->cfg.entropy_coef, h->cfg.desired_kl, h->cfg.lr_min, h->cfg.lr_max, h->cfg.adaptive);
  const int n_chunks = (n_bwd + RCH - 1) / RCH;
  const size_t slab = h->nA + h->nC;
  const int depth = Ma->n_layers > Mc->n_layers ? Ma->n_layers : Mc->n_layers;
  for (int lb = 0; lb < depth; ++lb) {
    const BwdLayer L0 = bwd_layer(h, 0, lb, b), L1 = bwd_layer(h, 1, lb, b);
    int groups = 1, nmax = 16, any_da = 0;
    for (const BwdLayer* L : {&L0, &L1}) {
      if (!L->active) continue;
      const int g = ((L->N / 16 + DW_TN - 1) / DW_TN) * ((L->K / 16 + DW_TK - 1) / DW_TK);
      if (g > groups) groups = g;
      if (L->N > nmax) nmax = L->N;
      if (L->dzprev) any_da = 1;
    }
    // only a launch that holds a first layer gathers: the others run the instantiation without the table code in their row loop
    if (MIR && ((L0.active && L0.gather) || (L1.active && L1.gather)))
      hipLaunchKernelGGL(k_bwd_dw<true>, dim3(groups, n_chunks, 2), dim3(WGT), 0, st, L0, L1, idx, n_bwd, n, h->partial, slab);
    else
      hipLaunchKernelGGL(k_bwd_dw<false>, dim3(groups, n_chunks, 2), dim3(WGT), 0, st, L0, L1, idx, n_bwd, n, h->partial, slab);
    hipLaunchKernelGGL(k_bwd_db, dim3(nmax / 16, n_chunks, 2), dim3(WGT), 0, st, L0, L1, n_bwd, h->partial, slab);
    if (any_da) {
      BwdLayer D0 = L0, D1 = L1;                           // a network at its first layer has no dA to compute
      if (!D0.dzprev) D0.active = 0;
      if (!D1.dzprev) D1.active = 0;
      hipLaunchKernelGGL(k_bwd_da, dim3((n_bwd + TM - 1) / TM, 2), dim3(64 * NWAVE), 0, st, D0, D1, n_bwd);
    }
  }
  if (!record)
    hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)((slab + WGT - 1) / WGT)), dim3(WGT), 0, st, h->partial, n_chunks, slab, h->grads);
  else
    hipLaunchKernelGGL(k_shard_record, dim3((unsigned)((h->n_tot + 5 + WGT - 1) / WGT)), dim3(WGT), 0, st, h->partial, n_chunks, slab, h->head_part, n_wg, ncol, h->A,
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
  if (!h || !std_dev || !idx || n < 1 || n > h->max_rows || !batch_ok(b)) return GO2SIM_E_BADARG;
  return launch_grad(h, b, std_dev, idx, n, 1.0 / (double)n, nullptr, (hipStream_t)stream);
}

int go2sim_ppo_shard_len(go2sim_ppo_t* h, size_t* out) {
  if (!h || !out) return GO2SIM_E_BADARG;
  *out = h->n_tot + 4 + (h->mirror ? 1 : 0);
  return GO2SIM_E_OK;
}

int go2sim_ppo_shard_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, const float* std_dev, const int32_t* idx, int n, long long n_global, double* record,
                          void* stream) {
  if (!h || !std_dev || !idx || !record || n < 1 || n > h->max_rows || n_global < (long long)n || !batch_ok(b)) return GO2SIM_E_BADARG;
  return launch_grad(h, b, std_dev, idx, n, 1.0 / (double)n_global, record, (hipStream_t)stream);
}

int go2sim_ppo_shard_reduce(go2sim_ppo_t* h, const double* records, int n_records, const float* std_dev, void* stream) {
  if (!h || !records || !std_dev || n_records < 1) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t slab = h->nA + h->nC, len = h->n_tot + 4 + (h->mirror ? 1 : 0);
  hipLaunchKernelGGL(k_shard_reduce, dim3((unsigned)((h->n_tot + WGT - 1) / WGT)), dim3(WGT), 0, st, records, n_records, len, slab, h->A, h->Apad, std_dev,
                     h->cfg.entropy_coef, h->grads);
  hipLaunchKernelGGL(k_shard_scalars, dim3(1), dim3(64), 0, st, records, n_records, len, h->n_tot, h->mirror ? 5 : 4, (h->mirror && h->use_aug) ? 2 : 1, h->A,
                     std_dev, h->scal, h->cfg.desired_kl, h->cfg.lr_min, h->cfg.lr_max, h->cfg.adaptive);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_ppo_set_mirror(go2sim_ppo_t* h, const go2sim_ppo_mirror_t* m, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
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
  hipLaunchKernelGGL(k_sym_loss, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

int go2sim_ppo_apply(go2sim_ppo_t* h, float* std_dev, void* stream) {
  if (!h || !std_dev) return GO2SIM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const double t = (double)(h->step + 1);                  // the handle's count moves once the launches are accepted
  AdamArgs a{};
  a.p_actor = h->actor->dparams; a.p_critic = h->critic->dparams; a.p_std = std_dev; a.g = h->grads; a.m = h->m; a.v = h->v;
  a.nA = h->nA; a.nC = h->nC; a.n_tot = h->n_tot; a.A = h->A; a.sq_part = h->sq_part; a.scal = h->scal;
  a.max_norm = h->cfg.max_grad_norm; a.b1 = h->cfg.beta1; a.b2 = h->cfg.beta2; a.eps = h->cfg.eps;
  a.bc1 = 1.0 - std::pow(h->cfg.beta1, t); a.bc2_sqrt = std::sqrt(1.0 - std::pow(h->cfg.beta2, t));
  hipLaunchKernelGGL(k_sumsq, dim3(NORM_WG), dim3(WGT), 0, st, h->grads, h->n_tot, h->sq_part);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((h->n_tot + WGT - 1) / WGT)), dim3(WGT), 0, st, a);
  HIPCHK(hipGetLastError());
  h->step += 1;
  return GO2SIM_E_OK;
}

int go2sim_ppo_update(go2sim_ppo_t* h, const go2sim_ppo_batch_t* b, float* std_dev, const int32_t* perm, int n_rows_total, int n_epochs, int n_mini_batches, void* stream) {
  if (!h || !b || !std_dev || !perm || n_epochs < 1 || n_mini_batches < 1 || n_rows_total < n_mini_batches) return GO2SIM_E_BADARG;
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
  *out = h->n_tot;
  return GO2SIM_E_OK;
}
int go2sim_ppo_export_padded(go2sim_ppo_t* h, int which, float* padded_dev, void* stream) {
  if (!h || !padded_dev || !vec_of(h, which)) return GO2SIM_E_BADARG;
  HIPCHK(hipMemcpyAsync(padded_dev, vec_of(h, which), h->n_tot * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GO2SIM_E_OK;
}

int go2sim_ppo_set_step(go2sim_ppo_t* h, long long step, double learning_rate, void* stream) {
  if (!h || step < 0 || !(learning_rate > 0.0)) return GO2SIM_E_BADARG;
  h->step = step;
  hipLaunchKernelGGL(k_set_lr, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal, learning_rate);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
int go2sim_ppo_reset_stats(go2sim_ppo_t* h, void* stream) {
  if (!h) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_reset_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
int go2sim_ppo_stats(go2sim_ppo_t* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return GO2SIM_E_BADARG;
  hipLaunchKernelGGL(k_stats, dim3(1), dim3(1), 0, (hipStream_t)stream, h->scal, (double)h->step, out_dev);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

}  // extern "C"
