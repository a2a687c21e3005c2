// go2sim_train_dev.h -- private to csrc/: the kernels every update shares, next to go2sim_mlp_dev.h.  The PPO update (go2sim_train.hip) and the
// distillation updates (go2sim_distill.hip, go2sim_rdistill.hip) include it; each keeps its own loss head, and both drive these kernels through the host code of
// go2sim_trainer_host.h (optimizer state, packing, workspaces, the backward schedule).  Not part of the C ABI.
//   k_train_forward   the layer loop of the inference kernel with every hidden layer's post-activation kept in the workspace
//   k_bwd_dw / k_bwd_db / k_bwd_da   the chunked backward of one layer of one or two networks (go2sim_train.hip describes them)
//   k_reduce_partials the chunk slabs added in chunk order in float64, rounded once
//   k_sumsq / k_adam  the global norm, the clip coefficient and Adam in one pass over the padded parameters
//   k_pack / k_set_lr flat <-> padded copies of one tensor, the device-side learning rate
// The scalar block `scal` both handles keep starts with the same slots (S_LR ... S_N): k_adam reads S_LR and writes S_NORM.
#ifndef GO2SIM_TRAIN_DEV_H
#define GO2SIM_TRAIN_DEV_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "go2sim_mlp_dev.h"
#include "../../include/go2sim_train.h"

namespace {

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
  int lin;              // k_bwd_da<true>: the layer's input is a memory's h, not an activation's output: dzprev = dZ W without the derivative's factor
  int act;              // GO2SIM_ACT_* of the network (MlpDev::act): the derivative k_bwd_da multiplies by
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

// one accumulator tile of k_bwd_da times the activation's derivative, from the stored post-activation (act_bwd, go2sim_mlp_dev.h)
template <int ACT>
__device__ __forceinline__ void bwd_store_dzprev(const f32x4 (&acc)[RT], const float* __restrict__ aprev, float* __restrict__ dzprev, int row0, int n_rows, int K, int kc, int kq) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row0 + 16 * rt + 4 * kq + i;
      if (r < n_rows) {
        const float a = aprev[(size_t)r * K + kc];
        dzprev[(size_t)r * K + kc] = acc[rt][i] * act_bwd<ACT>(a);
      }
    }
}

// dZ_prev[r][k] = (sum_n dZ[r][n] W[n][k]) * f'(A_prev[r][k]); f' of the network's activation (L.act) from the stored post-activation a: for ELU 1 for
// a > 0, a + 1 otherwise
// RNN: a first layer behind a memory (L.lin) writes d loss / d h; the plain instantiation is the kernel as it was
template <bool RNN>
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
      f32x4 tile[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) tile[rt] = acc[rt][t];
      if (RNN && L.lin) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = row0 + 16 * rt + 4 * kq + i;
            if (r < n_rows) L.dzprev[(size_t)r * K + kc[t]] = tile[rt][i];
          }
        continue;
      }
#define GO2SIM_STORE_DZPREV(A) bwd_store_dzprev<A>(tile, L.aprev, L.dzprev, row0, n_rows, K, kc[t], kq)
      GO2SIM_ACT_DISPATCH(L.act, GO2SIM_STORE_DZPREV)
#undef GO2SIM_STORE_DZPREV
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

__global__ __launch_bounds__(WGT) void k_sumsq(const float* __restrict__ g, size_t n, double* __restrict__ part) {
  __shared__ double s_red[WGT];
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * WGT + threadIdx.x; i < n; i += (size_t)NORM_WG * WGT) s += (double)g[i] * (double)g[i];
  const double t = wg_sum(s_red, s);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

struct AdamArgs {
  float *p_actor, *p_critic, *p_std, *g, *m, *v;
  size_t nA, nC, n_tot;                                   // padded sizes; the std block follows the two networks (and the memories)
  float *p_ma, *p_mc;                                     // k_adam<true>: the two memories' parameters, nMa + nMc entries after the networks
  size_t nMa, nMc;
  int A;
  const double* sq_part;
  double* scal;
  double max_norm, b1, b2, eps, bc1, bc2_sqrt;            // bc1 = 1 - b1^t, bc2_sqrt = sqrt(1 - b2^t), from the step count in float64 on the host
};

template <bool RNN>
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
  else if (RNN && i < a.nA + a.nC + a.nMa) p = a.p_ma + (i - a.nA - a.nC);
  else if (RNN && i < a.nA + a.nC + a.nMa + a.nMc) p = a.p_mc + (i - a.nA - a.nC - a.nMa);
  else { const size_t k = i - a.nA - a.nC - (RNN ? a.nMa + a.nMc : 0); if (k >= (size_t)a.A) return; p = a.p_std + k; }
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

}  // namespace
#endif
