// go2sim_trainer_host.h -- private to csrc/: the host side every update shares, next to the kernels of go2sim_train_dev.h.  The PPO update
// (go2sim_train.hip) and the distillation updates (go2sim_distill.hip, go2sim_rdistill.hip) are handles that own an OptState and call these pieces; each keeps its own loss
// head, statistics, argument checks and (PPO) mirror tables, shard records and recurrent workspaces.  Not part of the C ABI.
//   HIPCHK            the status check, tagged with the including file's GO2SIM_HIPCHK_TAG
//   OptState          grads | m | v and scal | sq_part | tail, the step count; opt_apply = k_sumsq + k_adam
//   Seg               flat (state-dict) <-> padded packing of a list of tensors
//   NetWs, BwdLayer   one network's row workspaces carved from a cursor, one layer of it as the backward kernels see it
//   launch_backward   the per-layer schedule k_bwd_dw, k_bwd_db, k_bwd_da from the last layer to the first, for one or two networks
// Everything here builds its descriptors on the stack and launches on the caller's stream: no allocation, synchronisation or device query per call.
#ifndef GO2SIM_TRAINER_HOST_H
#define GO2SIM_TRAINER_HOST_H
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "go2sim_mlp_dev.h"
#include "go2sim_train_dev.h"

#ifndef GO2SIM_HIPCHK_TAG
#error "define GO2SIM_HIPCHK_TAG (the file's name in its messages) before including go2sim_trainer_host.h"
#endif
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, GO2SIM_HIPCHK_TAG ": %s failed: %s\n", #x, hipGetErrorString(e_)); return GO2SIM_E_HIP; } \
  } while (0)

namespace {

inline size_t al16(size_t n) { return (n + 15) / 16 * 16; }   // every region starts 64-byte aligned (float4 loads)

// ---- the optimizer ---------------------------------------------------------------------------------------------------------------------------------
struct OptState {
  size_t n_tot = 0;           // padded floats of every vector
  float* fbuf = nullptr;      // grads | m | v
  double* dbuf = nullptr;     // scal[S_N] | sq_part[NORM_WG] | tail (the caller's doubles)
  float *grads = nullptr, *m = nullptr, *v = nullptr;
  double *scal = nullptr, *sq_part = nullptr, *tail = nullptr;
  size_t n_tail = 0;
  long long step = 0;
};

inline bool opt_alloc(OptState& o, size_t n_tot, size_t n_tail) {
  o.n_tot = n_tot; o.n_tail = n_tail;
  if (hipMalloc((void**)&o.fbuf, 3 * n_tot * sizeof(float)) != hipSuccess || hipMalloc((void**)&o.dbuf, (S_N + NORM_WG + n_tail) * sizeof(double)) != hipSuccess) return false;
  o.grads = o.fbuf; o.m = o.grads + n_tot; o.v = o.m + n_tot;
  o.scal = o.dbuf; o.sq_part = o.scal + S_N; o.tail = o.sq_part + NORM_WG;
  return true;
}
// zeroes the vectors, `ws` (a float workspace of the caller's that is zeroed with them, or nullptr) and the doubles, sets the learning rate, waits
inline bool opt_zero(OptState& o, double learning_rate, float* ws, size_t n_ws) {
  return hipMemset(o.fbuf, 0, 3 * o.n_tot * sizeof(float)) == hipSuccess && (!ws || hipMemset(ws, 0, n_ws * sizeof(float)) == hipSuccess) &&
         hipMemset(o.dbuf, 0, (S_N + NORM_WG + o.n_tail) * sizeof(double)) == hipSuccess &&
         hipMemcpy(o.dbuf + S_LR, &learning_rate, sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
}
inline void opt_free(OptState& o) {
  if (o.fbuf) (void)hipFree(o.fbuf);
  if (o.dbuf) (void)hipFree(o.dbuf);
}
// GRADS / ADAM_M / ADAM_V of either header's enum (PARAMS = 0 is not the optimizer's)
inline float* opt_vec(OptState& o, int which) { return which == GO2SIM_PPO_GRADS ? o.grads : which == GO2SIM_PPO_ADAM_M ? o.m : which == GO2SIM_PPO_ADAM_V ? o.v : nullptr; }

// One step.  `a` names the parameter blocks (p_actor / nA, p_critic / nC, p_std / A, with RNN p_ma / nMa and p_mc / nMc) and max_norm, b1, b2, eps; the
// vectors, the bias corrections of step + 1 and the scalars are filled here.  The count moves once the launches are accepted.
// (RNN, and MIR / MIRROR below, are template parameters so that a file instantiates only the kernels it launches.)
template <bool RNN>
int opt_apply(OptState& o, AdamArgs a, hipStream_t st) {
  const double t = (double)(o.step + 1);
  a.g = o.grads; a.m = o.m; a.v = o.v; a.n_tot = o.n_tot; a.sq_part = o.sq_part; a.scal = o.scal;
  a.bc1 = 1.0 - std::pow(a.b1, t); a.bc2_sqrt = std::sqrt(1.0 - std::pow(a.b2, t));
  hipLaunchKernelGGL(k_sumsq, dim3(NORM_WG), dim3(WGT), 0, st, o.grads, o.n_tot, o.sq_part);
  hipLaunchKernelGGL(k_adam<RNN>, dim3((unsigned)((o.n_tot + WGT - 1) / WGT)), dim3(WGT), 0, st, a);
  HIPCHK(hipGetLastError());
  o.step += 1;
  return GO2SIM_E_OK;
}
inline int opt_set_step(OptState& o, long long step, double learning_rate, hipStream_t st) {
  if (step < 0 || !(learning_rate > 0.0)) return GO2SIM_E_BADARG;
  o.step = step;
  hipLaunchKernelGGL(k_set_lr, dim3(1), dim3(1), 0, st, o.scal, learning_rate);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}
// a padded vector (`src`: opt_vec, or a parameter array of n_tot floats) as it is
inline int opt_export_padded(OptState& o, const float* src, float* padded_dev, hipStream_t st) {
  if (!padded_dev || !src) return GO2SIM_E_BADARG;
  HIPCHK(hipMemcpyAsync(padded_dev, src, o.n_tot * sizeof(float), hipMemcpyDeviceToDevice, st));
  return GO2SIM_E_OK;
}

// ---- flat (state-dict) <-> padded ------------------------------------------------------------------------------------------------------------------
struct Seg { int base; size_t pad_off; int ld, rows, cols; size_t flat_off; };   // one tensor: rows x cols at pad_off of base pointer `base`, ld apart

// W_0, b_0, W_1, b_1, ... of one network
inline void mlp_segs(std::vector<Seg>& segs, int base, const go2sim_mlp* M, size_t& flat) {
  for (int l = 0; l < M->n_layers; ++l) {
    segs.push_back(Seg{base, (size_t)(M->dev.W[l] - M->dparams), M->dev.kpad[l], M->dims[l + 1], M->dims[l], flat}); flat += (size_t)M->dims[l] * M->dims[l + 1];
    segs.push_back(Seg{base, (size_t)(M->dev.b[l] - M->dparams), M->dims[l + 1], 1, M->dims[l + 1], flat}); flat += M->dims[l + 1];
  }
}
// one memory (go2sim_lstm) in the flat order weight_ih, weight_hh, bias_ih, bias_hh; a gate's block of H rows sits Hpad rows apart
template <class Lstm>
void lstm_segs(std::vector<Seg>& segs, int base, const Lstm* m, size_t& flat) {
  const int H = m->H, I = m->I, Hp = m->dev.Hpad, Ip = m->dev.Ipad;
  const size_t o_hh = (size_t)4 * Hp * Ip, o_bi = o_hh + (size_t)4 * Hp * Hp, o_bh = o_bi + (size_t)4 * Hp;
  for (int q = 0; q < 4; ++q) { segs.push_back(Seg{base, (size_t)q * Hp * Ip, Ip, H, I, flat}); flat += (size_t)H * I; }
  for (int q = 0; q < 4; ++q) { segs.push_back(Seg{base, o_hh + (size_t)q * Hp * Hp, Hp, H, H, flat}); flat += (size_t)H * H; }
  for (int q = 0; q < 4; ++q) { segs.push_back(Seg{base, o_bi + (size_t)q * Hp, H, 1, H, flat}); flat += H; }
  for (int q = 0; q < 4; ++q) { segs.push_back(Seg{base, o_bh + (size_t)q * Hp, H, 1, H, flat}); flat += H; }
}
inline int pack_segs(const std::vector<Seg>& segs, float* const* base, int to_padded, float* flat, hipStream_t st) {
  for (const Seg& s : segs)
    hipLaunchKernelGGL(k_pack, dim3((s.rows * s.cols + WGT - 1) / WGT), dim3(WGT), 0, st, to_padded, base[s.base] + s.pad_off, s.ld, flat + s.flat_off, s.rows, s.cols);
  HIPCHK(hipGetLastError());
  return GO2SIM_E_OK;
}

// ---- one network's row workspaces ------------------------------------------------------------------------------------------------------------------
struct NetWs {
  ActWs a;                    // the hidden layers' post-activations
  float* dz[2];               // dZ ping-pong: layer l's in dz[l & 1], [rows][widest npad]
};
inline size_t dz_floats(const go2sim_mlp* M, size_t R) {
  int wmax = 16;
  for (int l = 0; l < M->n_layers; ++l) if (M->dev.npad[l] > wmax) wmax = M->dev.npad[l];
  return R * wmax;
}
inline size_t net_ws_floats(const go2sim_mlp* M, size_t R) {
  size_t need = 2 * dz_floats(M, R);
  for (int l = 0; l < M->n_layers - 1; ++l) need += R * M->dev.npad[l];
  return need;
}
// carves net_ws_floats(M, R) floats at `p`; -> the cursor behind them
inline float* net_ws_carve(const go2sim_mlp* M, size_t R, float* p, NetWs& w) {
  for (int l = 0; l < M->n_layers - 1; ++l) { w.a.a[l] = p; p += R * M->dev.npad[l]; }
  w.dz[0] = p; p += dz_floats(M, R); w.dz[1] = p; p += dz_floats(M, R);
  return p;
}

// Layer lb, counted from the last, of network M whose parameters sit at `off` in the slab.  The first layer reads x0 [.][dims[0]] (gather: rows through
// the index list, under a mirror through `mir`).
inline BwdLayer bwd_layer(const go2sim_mlp* M, const NetWs& w, int lb, const float* x0, int gather, MirTab mir, size_t off) {
  BwdLayer L{};
  const int l = M->n_layers - 1 - lb;
  if (l < 0) return L;
  L.active = 1;
  L.N = M->dev.npad[l]; L.K = M->dev.kpad[l]; L.act = M->dev.act;
  L.dz = w.dz[l & 1];
  L.W = M->dev.W[l];
  if (l == 0) { L.aprev = x0; L.lda = M->dims[0]; L.kmax = M->dims[0]; L.gather = gather; L.dzprev = nullptr; L.mir = mir; }
  else { L.aprev = w.a.a[l - 1]; L.lda = L.K; L.kmax = L.K; L.gather = 0; L.dzprev = w.dz[(l - 1) & 1]; }
  L.w_off = (size_t)(M->dev.W[l] - M->dparams) + off;
  L.b_off = (size_t)(M->dev.b[l] - M->dparams) + off;
  return L;
}

// ---- the backward schedule -------------------------------------------------------------------------------------------------------------------------
// where the launches of one gradient write and which rows they read
struct BwdRun {
  int nets;                   // networks per launch (grid z): 2 for actor and critic, 1 for a student (the second slot stays inactive)
  const int32_t* idx;         // row index list of the gather layers
  int n_rows, n_orig;         // rows in the launches; rows below n_orig are originals, the others their mirrors
  float* partial;             // [chunks][slab]
  size_t slab;
  hipStream_t st;
};

// dW and db of one layer of each network, per row chunk.  MIR: k_bwd_dw reads the gather layers' mirrored rows through their tables
template <bool MIR>
void launch_dw_db(const BwdLayer& L0, const BwdLayer& L1, const BwdRun& r) {
  int groups = 1, nmax = 16;
  for (const BwdLayer* L : {&L0, &L1}) {
    if (!L->active) continue;
    const int g = ((L->N / 16 + DW_TN - 1) / DW_TN) * ((L->K / 16 + DW_TK - 1) / DW_TK);
    if (g > groups) groups = g;
    if (L->N > nmax) nmax = L->N;
  }
  const int n_chunks = (r.n_rows + RCH - 1) / RCH;
  hipLaunchKernelGGL(k_bwd_dw<MIR>, dim3(groups, n_chunks, r.nets), dim3(WGT), 0, r.st, L0, L1, r.idx, r.n_rows, r.n_orig, r.partial, r.slab);
  hipLaunchKernelGGL(k_bwd_db, dim3(nmax / 16, n_chunks, r.nets), dim3(WGT), 0, r.st, L0, L1, r.n_rows, r.partial, r.slab);
}

// L[lb][net], lb = 0 the last layers, `depth` of them.  MIRROR: a launch that holds a gathering first layer takes k_bwd_dw<true> (the others run the
// instantiation without the table code in their row loop).  RNN: every layer hands dZ back (k_bwd_da<true>, the first layers to the memories' h');
// otherwise k_bwd_da<false> runs for the networks that have a dzprev and is skipped when none has (a network at its first layer has no dA to compute).
template <bool MIRROR, bool RNN>
void launch_backward(const BwdLayer (*L)[2], int depth, const BwdRun& r) {
  const dim3 da_grid((r.n_rows + TM - 1) / TM, r.nets);
  for (int lb = 0; lb < depth; ++lb) {
    const BwdLayer &L0 = L[lb][0], &L1 = L[lb][1];
    if (MIRROR && ((L0.active && L0.gather) || (L1.active && L1.gather))) launch_dw_db<MIRROR>(L0, L1, r);
    else launch_dw_db<false>(L0, L1, r);
    if (RNN) {
      hipLaunchKernelGGL(k_bwd_da<RNN>, da_grid, dim3(64 * NWAVE), 0, r.st, L0, L1, r.n_rows);
    } else if ((L0.active && L0.dzprev) || (L1.active && L1.dzprev)) {
      BwdLayer D0 = L0, D1 = L1;
      if (!D0.dzprev) D0.active = 0;
      if (!D1.dzprev) D1.active = 0;
      hipLaunchKernelGGL(k_bwd_da<RNN>, da_grid, dim3(64 * NWAVE), 0, r.st, D0, D1, r.n_rows);
    }
  }
}

}  // namespace
#endif
