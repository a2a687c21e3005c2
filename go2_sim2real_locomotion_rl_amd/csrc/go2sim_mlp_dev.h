// go2sim_mlp_dev.h -- private to csrc/: the device-side record of one MLP, the handle behind go2sim_mlp_t and the fused layer loop, shared by the
// inference source (go2sim_policy.hip) and the training source (go2sim_train.hip).  Not part of the C ABI.
#ifndef GO2SIM_MLP_DEV_H
#define GO2SIM_MLP_DEV_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/go2sim.h"
#include "../../include/go2sim_detmath.h"
#include "../../include/go2sim_policy.h"

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
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 16 * rt + 4 * kq + i;
          const float v = acc[rt][t][i] + bv;
          if (last) {
            const int gr = row0 + r;
            if (gr < B && n < dout) y[(size_t)gr * dout + n] = v;
          } else {
            out[r][n] = n < dout ? elu1(v) : 0.0f;                       // the K padding of the next layer is zero whatever the inputs: a non-finite
                                                                         // activation times the padded weight 0 would be NaN here and in every output after it
          }
        }
    }
  }
}

}  // namespace
#endif
