// go2sim_mlp_dev.h -- private to csrc/: the device-side record of one MLP, the handle behind go2sim_mlp_t and the fused layer loop, shared by the
// inference source (go2sim_policy.hip) and the training sources (go2sim_train.hip, go2sim_distill.hip, go2sim_rdistill.hip).  Not part of the C ABI.
#ifndef GO2SIM_MLP_DEV_H
#define GO2SIM_MLP_DEV_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/go2sim.h"
#include "../../include/go2sim_activation.h"
#include "../../include/go2sim_detmath.h"
#include "../../include/go2sim_policy.h"
#include "../../include/go2sim_rng.h"   // GO2SIM_RNG_POLICY_NOISE: the env holds purposes 1..10 and 16, the sensors 12..15

#ifndef MLP_KU
#define MLP_KU 1
#endif
#ifndef MLP_RT
#define MLP_RT 2
#endif

struct MlpDev {
  int n_layers;
  int din[GO2SIM_MLP_MAX_LAYERS], dout[GO2SIM_MLP_MAX_LAYERS], kpad[GO2SIM_MLP_MAX_LAYERS], npad[GO2SIM_MLP_MAX_LAYERS];
  const float* W[GO2SIM_MLP_MAX_LAYERS];   // [npad][kpad], zero padded
  const float* b[GO2SIM_MLP_MAX_LAYERS];   // [npad], zero padded
  int act;                                 // GO2SIM_ACT_* of the hidden layers (include/go2sim_activation.h); 0 = ELU
};

struct go2sim_mlp {
  int device = 0;
  int n_layers = 0;
  int dims[GO2SIM_MLP_MAX_LAYERS + 1] = {0};
  size_t n_params = 0;
  float* dparams = nullptr;   // padded weights + biases, one allocation: per layer W [npad][kpad] then b [npad]
  size_t padded = 0;
  MlpDev dev{};
  float* scratch_mean = nullptr; int scratch_rows = 0;   // mean buffer of go2sim_policy_act when the caller passes mean == NULL
};

namespace {

// weights and biases are reached through pointers stored in the MlpDev record: without the address space the compiler issues FLAT loads, whose
// counters do not retire in order, and then waits for every outstanding load before each use
constexpr int MAXL = GO2SIM_MLP_MAX_LAYERS, MAXW = GO2SIM_MLP_MAX_WIDTH, RT = MLP_RT, TM = 16 * RT, NWAVE = 4, LDW = MAXW + 4;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) float* gcfp;
typedef const __attribute__((address_space(1))) f32x4* gcf4p;

inline int round16(int v) { return (v + 15) / 16 * 16; }

__device__ __forceinline__ float elu1(float v) { return v > 0.0f ? v : dm_exp(v) - 1.0f; }   // nn.ELU(alpha=1)
// The other activations of include/go2sim_activation.h (the table, the non-finite cases and the error bounds are derived there).  Every argument of
// dm_exp is <= 0: no form overflows.  A NaN fails every comparison and reaches the arithmetic.
constexpr float SELU_L = 1.0507009873554805f, SELU_LA = 1.7580993408473766f, LRELU_SLOPE = 0.01f;   // nn.SELU's scale and scale * alpha, nn.LeakyReLU's slope
__device__ __forceinline__ float selu1(float v) { return v > 0.0f ? SELU_L * v : SELU_LA * (dm_exp(v) - 1.0f); }
__device__ __forceinline__ float relu1(float v) { return v < 0.0f ? 0.0f : v; }                     // not v > 0 ? v : 0: relu(NaN) is NaN
__device__ __forceinline__ float lrelu1(float v) { return v > 0.0f ? v : LRELU_SLOPE * v; }
__device__ __forceinline__ float tanh1(float v) {
  const float e = dm_exp(-2.0f * dm_abs(v)), t = (1.0f - e) / (1.0f + e);
  return __builtin_copysignf(t, v);                                                                 // tanh(-0) = -0, as torch
}
__device__ __forceinline__ float sigmoid1(float v) {
  const float e = dm_exp(-dm_abs(v)), d = 1.0f + e;
  return v >= 0.0f ? 1.0f / d : e / d;
}
template <int ACT>
__device__ __forceinline__ float act_fwd(float v) {
  return ACT == GO2SIM_ACT_ELU ? elu1(v) : ACT == GO2SIM_ACT_SELU ? selu1(v) : ACT == GO2SIM_ACT_RELU ? relu1(v) : ACT == GO2SIM_ACT_LRELU ? lrelu1(v)
         : ACT == GO2SIM_ACT_TANH ? tanh1(v) : ACT == GO2SIM_ACT_SIGMOID ? sigmoid1(v) : v;
}
// d activation / d pre-activation from the stored post-activation a
template <int ACT>
__device__ __forceinline__ float act_bwd(float a) {
  return ACT == GO2SIM_ACT_ELU ? (a > 0.0f ? 1.0f : a + 1.0f) : ACT == GO2SIM_ACT_SELU ? (a > 0.0f ? SELU_L : a + SELU_LA) : ACT == GO2SIM_ACT_RELU ? (a > 0.0f ? 1.0f : 0.0f)
         : ACT == GO2SIM_ACT_LRELU ? (a > 0.0f ? 1.0f : LRELU_SLOPE) : ACT == GO2SIM_ACT_TANH ? 1.0f - a * a : ACT == GO2SIM_ACT_SIGMOID ? a * (1.0f - a) : 1.0f;
}
// The activation is uniform over a launch's workgroup (a field of the MlpDev record): one scalar branch per epilogue selects the instantiation, so the
// ELU epilogue's instruction stream is the one it was.
#define GO2SIM_ACT_DISPATCH(act, CALL)                       \
  switch (act) {                                             \
    case GO2SIM_ACT_SELU: CALL(GO2SIM_ACT_SELU); break;      \
    case GO2SIM_ACT_RELU: CALL(GO2SIM_ACT_RELU); break;      \
    case GO2SIM_ACT_LRELU: CALL(GO2SIM_ACT_LRELU); break;    \
    case GO2SIM_ACT_TANH: CALL(GO2SIM_ACT_TANH); break;      \
    case GO2SIM_ACT_SIGMOID: CALL(GO2SIM_ACT_SIGMOID); break;  \
    case GO2SIM_ACT_IDENTITY: CALL(GO2SIM_ACT_IDENTITY); break; \
    default: CALL(GO2SIM_ACT_ELU); break;                    \
  }

// bias and activation of one accumulator tile of a hidden layer into the other LDS buffer
template <int ACT>
__device__ __forceinline__ void mlp_store_hidden(const f32x4 (&acc)[RT], float bv, float (*out)[LDW], int n, int dout, int kq) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = acc[rt][i] + bv;
      out[16 * rt + 4 * kq + i][n] = n < dout ? act_fwd<ACT>(v) : 0.0f;   // the K padding of the next layer is zero whatever the inputs and the activation
                                                                          // (sigmoid(0) = 0.5): a non-finite activation times the padded weight 0 would be
                                                                          // NaN here and in every output after it
    }
}

// One layer for the RT x 16 rows of the workgroup.  A wavefront works on TG output tiles (16 columns each) at a time: RT x TG independent accumulators
// share one weight fragment per (tile, K step) over the row tiles and one A fragment per (row tile, K step) over the output tiles.
template <int TG>
__device__ __forceinline__ void mlp_layer(const MlpDev& M, int l, const float (*in)[LDW], float (*out)[LDW], float* __restrict__ y, int row0, int B, int wave, int lane) {
  const int K = M.kpad[l], N = M.npad[l], dout = M.dout[l], ntiles = N / 16;
  const gcfp W = (gcfp)M.W[l];
  const gcfp bias = (gcfp)M.b[l];
  const bool last = l == M.n_layers - 1;
  const int arow = lane & 15, kq = lane >> 4;
  const float* ap = &in[arow][4 * kq];
  for (int g0 = wave * TG; g0 < ntiles; g0 += NWAVE * TG) {
    f32x4 acc[RT][TG];
    gcfp wrow[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const int nt = (g0 + t < ntiles) ? g0 + t : ntiles - 1;          // a short last group recomputes the last tile (not stored)
      wrow[t] = W + (size_t)(nt * 16 + arow) * K + 4 * kq;
    }
    // K steps in groups of KU: the weight fragments of a whole group are requested first, then the matrix instructions of its steps are issued in
    // order, each step waiting only for its own fragments (the counter retires in order), so the L2 latency of the weight stream is paid once per
    // group instead of once per step -- one wavefront per SIMD has nothing else to hide it.  (A hand-issued double buffer across the loop back edge
    // was tried: the register copies the compiler places on that edge read the buffer before its loads have landed.)
    constexpr int KU = MLP_KU;
    for (int j0 = 0; j0 < K; j0 += 16 * KU) {
      f32x4 wv[KU][TG];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int j = (j0 + 16 * u < K) ? j0 + 16 * u : K - 16;         // (a short last group re-reads the last step: no branch around the loads)
#pragma unroll
        for (int t = 0; t < TG; ++t) wv[u][t] = *(gcf4p)(wrow[t] + j);
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        if (j0 + 16 * u < K) {
          float4 av[RT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) av[rt] = *(const float4*)(ap + (size_t)rt * 16 * LDW + j0 + 16 * u);
#pragma unroll
          for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
              acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].x, wv[u][t][0], acc[rt][t], 0, 0, 0);   // k = j + 4 q + 0, q = 0..3
              acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].y, wv[u][t][1], acc[rt][t], 0, 0, 0);   // k = j + 4 q + 1
              acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].z, wv[u][t][2], acc[rt][t], 0, 0, 0);
              acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].w, wv[u][t][3], acc[rt][t], 0, 0, 0);
            }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      if (g0 + t >= ntiles) break;
      const int n = (g0 + t) * 16 + arow;                              // accumulator element i of this lane: row 4 * (lane >> 4) + i, column lane & 15
      const float bv = bias[n];
      if (last) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int gr = row0 + 16 * rt + 4 * kq + i;
            const float v = acc[rt][t][i] + bv;
            if (gr < B && n < dout) y[(size_t)gr * dout + n] = v;
          }
      } else {
        f32x4 tile[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) tile[rt] = acc[rt][t];
#define GO2SIM_STORE_HIDDEN(A) mlp_store_hidden<A>(tile, bv, out, n, dout, kq)
        GO2SIM_ACT_DISPATCH(M.act, GO2SIM_STORE_HIDDEN)
#undef GO2SIM_STORE_HIDDEN
      }
    }
  }
}

// The two kernels of a policy step, for the sources that act (go2sim_policy.hip, go2sim_distill.hip, go2sim_rdistill.hip): they define GO2SIM_MLP_ACT_KERNELS before the include, so
// that a source that only trains does not carry a copy.
#ifdef GO2SIM_MLP_ACT_KERNELS
// blockIdx.y selects the network: actor and critic of one policy step (student and teacher of one distillation step) share a launch (2 x 128
// workgroups of 32 rows at 4096 rows, one per CU)
__global__ __launch_bounds__(64 * NWAVE) void k_mlp_forward(MlpDev M0, const float* __restrict__ x0, float* __restrict__ y0,
                                                            MlpDev M1, const float* __restrict__ x1, float* __restrict__ y1, int B) {
  __shared__ alignas(16) float act[2][TM][LDW];
  const MlpDev& M = blockIdx.y == 0 ? M0 : M1;
  const float* __restrict__ x = blockIdx.y == 0 ? x0 : x1;
  float* __restrict__ y = blockIdx.y == 0 ? y0 : y1;
  const int row0 = blockIdx.x * TM;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  {
    const int K0 = M.kpad[0], d0 = M.din[0];
    for (int idx = tid; idx < TM * K0; idx += 64 * NWAVE) {
      int r = idx / K0, k = idx - r * K0, gr = row0 + r;
      act[0][r][k] = (gr < B && k < d0) ? x[(size_t)gr * d0 + k] : 0.0f;
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
  }
}

// Normal(mean, std).sample() + log_prob, one lane per row (A <= 16 actions)
__global__ __launch_bounds__(64) void k_policy_sample(const float* __restrict__ mean, const float* __restrict__ std_, int B, int A, uint64_t seed, uint32_t step,
                                                      int deterministic, float* __restrict__ actions, float* __restrict__ log_prob) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float lp = 0.0f;
  for (int blk = 0; 4 * blk < A; ++blk) {
    float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!deterministic) {
      dm_u4 r = dm_philox((uint32_t)b, step, GO2SIM_RNG_POLICY_NOISE, (uint32_t)blk, (uint32_t)seed, (uint32_t)(seed >> 32));
      dm_normal2(r.v[0], r.v[1], &n[0], &n[1]); dm_normal2(r.v[2], r.v[3], &n[2], &n[3]);
    }
    for (int k = 0; k < 4; ++k) {
      const int a = 4 * blk + k;
      if (a >= A) break;
      const float mu = mean[(size_t)b * A + a], sd = std_[a];
      const float act = mu + sd * n[k];
      actions[(size_t)b * A + a] = act;
      const float d = act - mu;
      lp = lp + ((-(d * d) / (2.0f * (sd * sd)) - dm_log(sd)) - 0.91893853320467274178f);
    }
  }
  if (log_prob) log_prob[b] = lp;
}
#endif  // GO2SIM_MLP_ACT_KERNELS

}  // namespace
#endif
