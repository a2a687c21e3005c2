// go2sim_lstm_dev.h -- private to csrc/: the device-side record of one LSTM memory, the handle behind go2sim_lstm_t and the two kernels that walk
// through time (include/go2sim_rnn.h): the cell step and the backward-through-time step.  Included by go2sim_train.hip and go2sim_rdistill.hip.  Not part of the C ABI.
//
// Both kernels tile the hidden units, never the 4 H gate columns as one row: a workgroup owns TM = 32 rows and NWAVE x 16 hidden units, a wavefront one
// 16-unit column tile.  In the cell step the wavefront holds the four gate accumulators of its units for both row tiles (8 accumulators), so i, f, g, o
// of one unit meet in one lane and the cell law runs on the accumulators: no gate row is ever staged in LDS.  Operands are read straight from global
// memory (x and h rows are short and L2-resident; the weights stream as in mlp_layer); neither kernel uses LDS or a barrier.
// Summation order of one gate pre-activation: acc = 0; the K blocks of 16 of x (zero padded), then those of h; in a block for s in 0..3: for q in 0..3:
// k = 16 block + 4 q + s: acc = fma(in[k], W[n][k], acc); then (acc + b_ih) + b_hh.
#ifndef GO2SIM_LSTM_DEV_H
#define GO2SIM_LSTM_DEV_H
#include "go2sim_mlp_dev.h"

struct LstmDev {
  int I, H, Ipad, Hpad;
  const float* Wih;   // [4 Hpad][Ipad], gate q's unit j in row q Hpad + j, zero padded
  const float* Whh;   // [4 Hpad][Hpad]
  const float* bih;   // [4 Hpad]
  const float* bhh;   // [4 Hpad]
};

struct go2sim_lstm {
  int device = 0, I = 0, H = 0;
  size_t n_params = 0, padded = 0;
  float* dparams = nullptr;   // W_ih | W_hh | b_ih | b_hh, one allocation
  LstmDev dev{};
};

namespace {

// sigmoid and tanh from dm_exp of a non-positive argument: no overflow, the same bits on every run
__device__ __forceinline__ float lstm_sigmoid(float z) {
  const float e = dm_exp(-dm_abs(z));
  return z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}
__device__ __forceinline__ float lstm_tanh(float z) {
  const float a = dm_abs(z);
  float t;
  if (a < 0.3f) {                                         // 1 - exp(-2a) cancels here: the odd series, truncation below 2^-28 relative at 0.3
    const float a2 = a * a;
    float p = -0.00886323552990219656886f;                // -1382 / 155925
    p = p * a2 + 0.0218694885361552028219f;               // 62 / 2835
    p = p * a2 - 0.0539682539682539682540f;               // -17 / 315
    p = p * a2 + 0.133333333333333333333f;                // 2 / 15
    p = p * a2 - 0.333333333333333333333f;
    t = a + a * (a2 * p);
  } else {
    const float e = dm_exp(-2.0f * a);
    t = (1.0f - e) / (1.0f + e);
  }
  return z < 0.0f ? -t : t;
}

// one memory as the cell kernel sees it; all state arrays [rows][H], unpadded
struct CellNet {
  LstmDev M;
  const float* x;       // [rows][ldx], I columns exist
  int ldx;
  const float *hin, *cin;
  float *hout, *cout;
  float* gates;         // STORE: [rows][4 Hpad] i | f | g | o, padded entries zero
  float *hprev, *cprev; // STORE: the masked state entering the step
  int active;
};

// reset: rows with a non-zero entry enter the step with h = c = 0
template <bool STORE>
__global__ __launch_bounds__(64 * NWAVE) void k_lstm_cell(CellNet n0, CellNet n1, const uint8_t* __restrict__ reset, int n_rows) {
  const CellNet& N = blockIdx.z == 0 ? n0 : n1;
  if (!N.active) return;
  const int I = N.M.I, H = N.M.H, Ipad = N.M.Ipad, Hpad = N.M.Hpad;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  const int jt = blockIdx.y * NWAVE + wave;               // this wavefront's tile of 16 hidden units
  if (jt * 16 >= Hpad) return;
  const int row0 = blockIdx.x * TM, u = jt * 16 + col;
  f32x4 acc[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[rt][q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  bool ron[RT], hon[RT];
  size_t ar[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {                        // the A operand's row of this lane
    const int r = row0 + 16 * rt + col;
    ron[rt] = r < n_rows;
    ar[rt] = ron[rt] ? (size_t)r : 0;
    hon[rt] = ron[rt] && !(reset && reset[ar[rt]]);
  }
  const gcfp x = (gcfp)N.x;
  const gcfp hin = (gcfp)N.hin;
  {
    const gcfp W = (gcfp)N.M.Wih;
    for (int j = 0; j < Ipad; j += 16) {
      f32x4 wv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) wv[q] = *(gcf4p)(W + (size_t)(q * Hpad + u) * Ipad + j + 4 * kq);
      float av[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = j + 4 * kq + s;
          av[rt][s] = (ron[rt] && k < I) ? x[ar[rt] * N.ldx + k] : 0.0f;
        }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][s], wv[q][s], acc[rt][q], 0, 0, 0);
    }
  }
  {
    const gcfp W = (gcfp)N.M.Whh;
    for (int j = 0; j < Hpad; j += 16) {
      f32x4 wv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) wv[q] = *(gcf4p)(W + (size_t)(q * Hpad + u) * Hpad + j + 4 * kq);
      float av[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = j + 4 * kq + s;
          av[rt][s] = (hon[rt] && k < H) ? hin[ar[rt] * H + k] : 0.0f;
        }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][s], wv[q][s], acc[rt][q], 0, 0, 0);
    }
  }
  // accumulator element i of this lane: row 4 * (lane >> 4) + i, unit u
  float bi[4], bh[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { bi[q] = N.M.bih[q * Hpad + u]; bh[q] = N.M.bhh[q * Hpad + u]; }
  const bool uon = u < H;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row0 + 16 * rt + 4 * kq + i;
      if (r >= n_rows) continue;
      const bool keep = !(reset && reset[r]);
      float ig = 0.0f, fg = 0.0f, gg = 0.0f, og = 0.0f, cp = 0.0f, hp = 0.0f;
      if (uon) {
        if (keep) { cp = N.cin[(size_t)r * H + u]; hp = N.hin[(size_t)r * H + u]; }
        ig = lstm_sigmoid((acc[rt][0][i] + bi[0]) + bh[0]);
        fg = lstm_sigmoid((acc[rt][1][i] + bi[1]) + bh[1]);
        gg = lstm_tanh((acc[rt][2][i] + bi[2]) + bh[2]);
        og = lstm_sigmoid((acc[rt][3][i] + bi[3]) + bh[3]);
        const float cn = fg * cp + ig * gg;
        N.cout[(size_t)r * H + u] = cn;
        N.hout[(size_t)r * H + u] = og * lstm_tanh(cn);
        if (STORE) { N.cprev[(size_t)r * H + u] = cp; N.hprev[(size_t)r * H + u] = hp; }
      }
      if (STORE) {
        float* __restrict__ g = N.gates + (size_t)r * 4 * Hpad + u;
        g[0] = ig; g[Hpad] = fg; g[2 * Hpad] = gg; g[3 * Hpad] = og;
      }
    }
}

// one memory at step t of the walk back through time
struct BpttNet {
  LstmDev M;
  const float* dz_next;  // [rows][4 Hpad]: dz of step t + 1 (not read at the last step)
  const float* dh_mlp;   // [rows][Hpad]: d loss / d h'[t] from the MLP's first layer
  const float* gates;    // [rows][4 Hpad] of step t
  const float *cprev, *cout;   // [rows][H] of step t
  float* dc;             // [rows][Hpad] carried: read as d loss / d c'[t] coming from step t + 1, written as dc f for step t - 1
  float* dz;             // [rows][4 Hpad] of step t
  int active;
};

// dh = dh_mlp[t] + dz[t+1] W_hh, dc = dc_carried + dh o (1 - tanh^2 c'); cut (u8 [rows]: dones[t]) zeroes both carried terms; has_next = 0 at t = T - 1
__global__ __launch_bounds__(64 * NWAVE) void k_lstm_bptt(BpttNet n0, BpttNet n1, const uint8_t* __restrict__ cut, int has_next, int n_rows) {
  const BpttNet& N = blockIdx.z == 0 ? n0 : n1;
  if (!N.active) return;
  const int H = N.M.H, Hpad = N.M.Hpad, NZ = 4 * Hpad;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  const int jt = blockIdx.y * NWAVE + wave;
  if (jt * 16 >= Hpad) return;
  const int row0 = blockIdx.x * TM, u = jt * 16 + col;
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if (has_next) {
    const gcfp W = (gcfp)N.M.Whh;
    const gcfp dzn = (gcfp)N.dz_next;
    bool ron[RT];
    size_t roff[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { const int r = row0 + 16 * rt + col; ron[rt] = r < n_rows; roff[rt] = ron[rt] ? (size_t)r * NZ + 4 * kq : 0; }
    // reduction index: n = j + 16 v + 4 (lane >> 4) + s.  NZ = 4 Hpad is a multiple of 64: the operands of four steps of 16 are requested together, then
    // their matrix instructions are issued in step order (the fma chain is the one of the plain loop)
    constexpr int KU = 4;
    for (int j = 0; j < NZ; j += 16 * KU) {
      f32x4 av[KU][RT];
      float wv[KU][4];
#pragma unroll
      for (int v = 0; v < KU; ++v) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) av[v][rt] = ron[rt] ? *(gcf4p)(dzn + roff[rt] + j + 16 * v) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s) wv[v][s] = W[(size_t)(j + 16 * v + 4 * kq + s) * Hpad + u];
      }
#pragma unroll
      for (int v = 0; v < KU; ++v)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[v][rt][s], wv[v][s], acc[rt], 0, 0, 0);
    }
  }
  const bool uon = u < H;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row0 + 16 * rt + 4 * kq + i;
      if (r >= n_rows) continue;
      float dzi = 0.0f, dzf = 0.0f, dzg = 0.0f, dzo = 0.0f, dcp = 0.0f;
      if (uon) {
        const bool carry = has_next && !cut[r];
        const float dh = carry ? N.dh_mlp[(size_t)r * Hpad + u] + acc[rt][i] : N.dh_mlp[(size_t)r * Hpad + u];
        const float* __restrict__ g = N.gates + (size_t)r * NZ + u;
        const float ig = g[0], fg = g[Hpad], gg = g[2 * Hpad], og = g[3 * Hpad];
        const float tc = lstm_tanh(N.cout[(size_t)r * H + u]);
        float dc = dh * og * (1.0f - tc * tc);
        if (carry) dc = N.dc[(size_t)r * Hpad + u] + dc;
        dzi = dc * gg * (ig * (1.0f - ig));
        dzf = dc * N.cprev[(size_t)r * H + u] * (fg * (1.0f - fg));
        dzg = dc * ig * (1.0f - gg * gg);
        dzo = dh * tc * (og * (1.0f - og));
        dcp = dc * fg;
      }
      float* __restrict__ d = N.dz + (size_t)r * NZ + u;
      d[0] = dzi; d[Hpad] = dzf; d[2 * Hpad] = dzg; d[3 * Hpad] = dzo;
      N.dc[(size_t)r * Hpad + u] = dcp;
    }
}

// the rows of an env block in the rollout's arrays: idx[t * nb + j] = t * B + e0 + j
__global__ __launch_bounds__(256) void k_rnn_idx(int32_t* __restrict__ idx, int n, int nb, int B, int e0) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int t = r / nb, j = r - t * nb;
  idx[r] = t * B + e0 + j;
}
__global__ __launch_bounds__(256) void k_iota(int32_t* __restrict__ idx, int n) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n) idx[r] = r;
}

}  // namespace
#endif
